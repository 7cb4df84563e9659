"""Prompt-lookup drafts in the batched slot loop against the plain slot loop at the 7b shape (random init, the persona prompt):
aggregate tok/s and ms per step of ``SlotLoop`` (what ``generate_batch`` runs without ``lookup``) and of ``LookupSlotLoop`` at
(S, k) in {(4, 3), (8, 3), (4, 7), (8, 7)}, with a full-acceptance corpus (the context tail followed by the answer itself: every
draft is right) and with an empty one (nothing to copy: every step pays S * (k + 1) rows for S tokens, unless the output repeats
itself).  All S sequences decode the same prompt in arenas of their own.  Same process, legs interleaved, medians.  Prints one
JSON line.  The loops are driven directly, with generate_batch's replay policy, because the corpus of a leg is chosen here
(generate_batch builds it from the staged ids and the prompt); the host's detokenising per token is in neither leg.
``--share-trunk`` adds, next to every lookup leg, the same leg with ``lookup_slot_loop(share_trunk=True)`` (the S
prompts are over one schema, so every staged row is shared and read once per step for all draft rows of all sequences) and the
ratio of the shared to the unshared lookup leg per (S, k).

    python tools/batch_lookup_bench.py [--new 64] [--repeats 5] [--out profiles/batch_lookup_bench.json]
    python tools/batch_lookup_bench.py --share-trunk            # -> profiles/batch_lookup_trunk_bench.json

``--slot-kv int8 --lookup 3 7 [--slot-drop-fp16] [--weight-format mxfp4]`` measures something else: the lookup loop over
the fp16 arenas against the lookup loop over int8 images (``lookup_slot_loop(kv="int8")``; with ``--slot-drop-fp16`` also
``keep_arenas=False``) at S = 4 / 8 with the full-acceptance corpus, legs interleaved with the order rotating -- per leg the median
[min .. max] of the HIP-event time of ONE replay over all replays of all repetitions, ``slot_kv_bytes()``, the first step's max
|dlogit| against the fp16 leg and the share of sequence 0's tokens that agree with it.

    python tools/batch_lookup_bench.py --slot-kv int8 --lookup 3 7 --slot-drop-fp16   # -> profiles/lookup_slot_kv_q8_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prompt-cache_amd")]
from promptcache_amd import CacheEngine, Prompt, synth  # noqa: E402
from promptcache_amd.model import Llama2  # noqa: E402

CASES = ((4, 3), (8, 3), (4, 7), (8, 7))


def prefill(lm, eng, prompt, S):
    pasts, firsts, p0s, ids0 = [], [], [], None
    for j in range(S):
        ids, pos, _, cache = eng.process(prompt, slot=j)
        out = lm(input_ids=torch.tensor([ids]), position_ids=torch.tensor([pos]), past_key_values=cache, use_cache=True)
        pasts.append(out.past_key_values)
        firsts.append(int(out.logits[0, -1].argmax()))
        p0s.append(max(pos) + 2)
        ids0 = ids
    return ids0, pasts, firsts, p0s


def run_slots(lm, eng, prompt, S, n_new):
    """-> (first token and the n_new tokens behind it of sequence 0, seconds from the first enqueue to the last token on the
    host, per-step ms)."""
    _, pasts, firsts, p0s = prefill(lm, eng, prompt, S)
    loop = lm.hf_model.slot_loop(pasts, firsts, p0s, n_new)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.enqueue()
    toks = []
    for i in range(n_new):
        if loop.n <= i + 1 and loop.n < n_new:
            loop.enqueue()
        row = [loop.token(j, i) for j in range(S)]
        toks.append(row[0])
    dt = time.perf_counter() - t0
    ms = [loop.elapsed_ms(i) for i in range(n_new)]
    loop.close([n_new] * S)
    return firsts[0], toks, dt, ms


def run_lookup(lm, eng, prompt, S, n_new, k, corpus, share=False, info=None, **mode):
    """-> (tokens of sequence 0, seconds as in run_slots, per-step ms, steps taken).  The replay policy is generate_batch's.
    ``mode``: ``kv`` / ``keep_arenas`` of ``lookup_slot_loop``; ``info`` then takes the loop's class, ``slot_kv_bytes()`` and split
    count."""
    _, pasts, firsts, p0s = prefill(lm, eng, prompt, S)
    loop = lm.hf_model.lookup_slot_loop(pasts, firsts, p0s, n_new, k, [corpus] * S, share_trunk=share, **mode)
    assert loop is not None and bool(loop.nsplit_trunk) == share
    if info is not None and share:
        info.update(trunk_rows=max(T for _, T in loop.trunks), keys=max(loop.len0), nsplit_own=loop.nsplit, nsplit_trunk=loop.nsplit_trunk)
    elif info is not None:
        info.update(loop=type(loop).__name__, slot_kv_bytes=loop.slot_kv_bytes(), keys=max(loop.len0), nsplit=loop.nsplit,
                    qcap=getattr(loop, "qcap", None))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, i = [[] for _ in range(S)], 0
    while min(map(len, got)) < n_new:
        if loop.n <= i:
            loop.enqueue()
        if loop.n == i + 1 and min(map(len, got)) + k + 1 < n_new:
            loop.enqueue()                       # one replay ahead while the step in flight cannot exhaust every budget
        for j in range(S):
            got[j] += loop.tokens(j, i)
        i += 1
    dt = time.perf_counter() - t0
    ms = [loop.elapsed_ms(j) for j in range(i)]
    loop.close([n_new] * S)
    return got[0], dt, ms, i


def first_logits(lm, eng, prompt, S, n_new, k, corpus, **mode):
    """The logits of the first replay, [S * (k + 1)][V] on the host."""
    _, pasts, firsts, p0s = prefill(lm, eng, prompt, S)
    loop = lm.hf_model.lookup_slot_loop(pasts, firsts, p0s, n_new, k, [corpus] * S, **mode)
    loop.enqueue()
    torch.cuda.synchronize()
    out = loop.logits.float().cpu()
    loop.close([0] * S)
    return out


def slot_kv_legs(lm, eng, prompt, args, full, T):
    """The fp16-arena lookup leg against the int8 legs of the same commit -> the result dict."""
    N = args.new
    modes = {"fp16": {}, "int8": dict(kv="int8")}
    if args.slot_drop_fp16:
        modes["int8_only"] = dict(kv="int8", keep_arenas=False)
    legs = [(f"S{S}_k{k}_{m}", S, k, m) for S in (4, 8) for k in args.lookup for m in modes]
    info, acc = {}, {}
    for name, S, k, m in legs:                                       # warm: graphs captured; accuracy against the fp16 leg
        run_lookup(lm, eng, prompt, S, N, k, full, info=info.setdefault(name, {}), **modes[m])
    for S in (4, 8):
        for k in args.lookup:
            base = first_logits(lm, eng, prompt, S, N, k, full)
            for m in modes:
                if m != "fp16":
                    acc[f"S{S}_k{k}_{m}"] = round(float((first_logits(lm, eng, prompt, S, N, k, full, **modes[m]) - base).abs().max()), 5)
    ms_all = {leg[0]: [] for leg in legs}
    rate = {leg[0]: [] for leg in legs}
    toks0, steps = {}, {}
    for rep in range(args.repeats):
        print(f"[batch_lookup_bench] repetition {rep + 1} of {args.repeats}", file=sys.stderr, flush=True)
        order = legs[rep % len(legs):] + legs[:rep % len(legs)]      # the order rotates
        for name, S, k, m in order:
            toks0[name], dt, ms, steps[name] = run_lookup(lm, eng, prompt, S, N, k, full, **modes[m])
            ms_all[name] += ms
            rate[name].append(S * N / dt)
    stat = lambda v: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]
    res = {"shape": "llama2-7b (random init)", "weight_format": args.weight_format, "new_tokens": N,
           "prompt": "persona-structured schema, S copies in arenas of their own, full-acceptance corpus",
           "how": "same process, legs interleaved with the order rotating, %d repetitions; replay_ms: median, min, max of the HIP-event "
                  "time of one replay over all replays of all repetitions" % args.repeats,
           "replay_ms": {n: stat(v) for n, v in ms_all.items()},
           "tokens_per_s": {n: round(statistics.median(v), 1) for n, v in rate.items()},
           "steps": steps, "loops": info,
           "first_step_max_abs_dlogit_vs_fp16": acc,
           "greedy_agreement_with_fp16": {n: round(sum(a == b for a, b in zip(toks0[n][:N], toks0[f"S{S}_k{k}_fp16"][:N])) / N, 3)
                                          for n, S, k, m in legs if m != "fp16"},
           "tokens_equal_slot_loop_fp16": {n: toks0[n][:N] == T for n, _, _, m in legs if m == "fp16"}}
    rm = res["replay_ms"]
    res["int8_median_below_fp16_min"] = {n: rm[n][0] < rm[f"S{S}_k{k}_fp16"][1] for n, S, k, m in legs if m != "fp16"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64, help="tokens per sequence (behind the first)")
    ap.add_argument("--repeats", type=int, default=5, help="interleaved repetitions per leg (medians)")
    ap.add_argument("--share-trunk", action="store_true", help="add the lookup legs with share_trunk=True")
    ap.add_argument("--out", default=None, help="default with --share-trunk: profiles/batch_lookup_trunk_bench.json")
    ap.add_argument("--slot-kv", default="fp16", help="int8: the lookup loop over int8 images against the fp16-arena lookup loop")
    ap.add_argument("--lookup", type=int, nargs="*", default=[3, 7], help="with --slot-kv int8: the draft counts")
    ap.add_argument("--slot-drop-fp16", action="store_true", help="with --slot-kv int8: also keep_arenas=False")
    ap.add_argument("--weight-format", default="fp16", help="fp16 or mxfp4")
    args = ap.parse_args()
    if args.slot_kv == "int8" and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "lookup_slot_kv_q8_bench.json")
    if args.share_trunk and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "batch_lookup_trunk_bench.json")
    assert torch.cuda.is_available(), "batch_lookup_bench measures on the GPU"
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0,
                **({"weight_format": args.weight_format} if args.weight_format != "fp16" else {}))
    assert lm.hf_model.lookup_available() and lm.hf_model.slot_loop_available()
    eng = CacheEngine(4096, lm, slots=8)
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    prompt = Prompt(pp, [fmt])
    N = args.new
    ctx_ids, _, _, _ = prefill(lm, eng, prompt, 1)
    first, T, _, _ = run_slots(lm, eng, prompt, 1, N)                # warm + the answer the full-acceptance corpus copies
    full = list(ctx_ids)[-8:] + [first] + T
    if args.slot_kv == "int8":
        res = slot_kv_legs(lm, eng, prompt, args, full, T)
        if args.out and args.weight_format != "fp16" and os.path.exists(args.out):      # (one file: a key per weight format)
            with open(args.out) as f:
                res = {**json.load(f), args.weight_format: res}
        line = json.dumps(res)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    legs = [(f"slots_S{S}", S, None, None, False) for S in sorted({s for s, _ in CASES})]
    for S, k in CASES:
        for name, c in (("full", full), ("empty", [])):
            legs.append((f"lookup_S{S}_k{k}_{name}", S, k, c, False))
            if args.share_trunk:
                legs.append((f"lookup_trunk_S{S}_k{k}_{name}", S, k, c, True))
    shared_info = {}
    for name, S, k, c, share in legs:                                # warm: graphs captured
        if k is None:
            run_slots(lm, eng, prompt, S, N)
        else:
            run_lookup(lm, eng, prompt, S, N, k, c, share, shared_info.setdefault(name, {}) if share else None)
    rate = {leg[0]: [] for leg in legs}
    step_ms = {leg[0]: [] for leg in legs}
    steps, same = {}, {}
    for rep in range(args.repeats):
        print(f"[batch_lookup_bench] repetition {rep + 1} of {args.repeats}", file=sys.stderr, flush=True)
        for name, S, k, c, share in legs:
            if k is None:
                _, toks, dt, ms = run_slots(lm, eng, prompt, S, N)
                steps[name] = N
            else:
                toks, dt, ms, steps[name] = run_lookup(lm, eng, prompt, S, N, k, c, share)
            same[name] = toks[:N] == T
            rate[name].append(S * N / dt)
            step_ms[name].append(statistics.median(ms))
    result = {"shape": "llama2-7b (random init)", "prompt": "persona-structured schema, S copies in arenas of their own", "new_tokens": N,
              "how": "same process, legs interleaved, %d repetitions, medians; aggregate tokens per wall-clock second from the first "
                     "enqueue to the last token on the host; step_ms: HIP events around one replay" % args.repeats,
              "tokens_per_s": {n: round(statistics.median(v), 1) for n, v in rate.items()},
              "tokens_per_s_min_max": {n: [round(min(v), 1), round(max(v), 1)] for n, v in rate.items()},
              "step_ms": {n: round(statistics.median(v), 4) for n, v in step_ms.items()},
              "steps": steps, "tokens_equal_slot_loop": same}
    tp = result["tokens_per_s"]
    result["ratio_to_slot_loop"] = {n: round(tp[n] / tp[f"slots_S{S}"], 3) for n, S, k, _, _ in legs if k is not None}
    if args.share_trunk:
        sm = result["step_ms"]
        result["shared_trunk"] = shared_info
        result["shared_to_unshared_tokens_per_s"] = {n: round(tp[n] / tp[n.replace("lookup_trunk_", "lookup_")], 3)
                                                     for n, _, _, _, share in legs if share}
        result["shared_to_unshared_step_ms"] = {n: round(sm[n] / sm[n.replace("lookup_trunk_", "lookup_")], 3)
                                                for n, _, _, _, share in legs if share}
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
