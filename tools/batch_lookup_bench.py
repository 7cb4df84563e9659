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


def run_lookup(lm, eng, prompt, S, n_new, k, corpus, share=False, info=None):
    """-> (tokens of sequence 0, seconds as in run_slots, per-step ms, steps taken).  The replay policy is generate_batch's."""
    _, pasts, firsts, p0s = prefill(lm, eng, prompt, S)
    loop = lm.hf_model.lookup_slot_loop(pasts, firsts, p0s, n_new, k, [corpus] * S, share_trunk=share)
    assert loop is not None and bool(loop.nsplit_trunk) == share
    if info is not None:
        info.update(trunk_rows=max(T for _, T in loop.trunks), keys=max(loop.len0), nsplit_own=loop.nsplit, nsplit_trunk=loop.nsplit_trunk)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64, help="tokens per sequence (behind the first)")
    ap.add_argument("--repeats", type=int, default=5, help="interleaved repetitions per leg (medians)")
    ap.add_argument("--share-trunk", action="store_true", help="add the lookup legs with share_trunk=True")
    ap.add_argument("--out", default=None, help="default with --share-trunk: profiles/batch_lookup_trunk_bench.json")
    args = ap.parse_args()
    if args.share_trunk and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "batch_lookup_trunk_bench.json")
    assert torch.cuda.is_available(), "batch_lookup_bench measures on the GPU"
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0)
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
