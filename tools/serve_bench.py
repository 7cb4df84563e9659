"""Continuous batching against static waves, same process, same box: 7b shape (random init), bench.py's persona schema, greedy,
32 prompts through 8 slots with max_new_tokens drawn once from {16, 32, 64, 128} (fixed seed).  (a) generate_batch in four waves of
8 -- a wave lasts as long as its longest sequence -- and (b) serve, which refills a slot as soon as its sequence ends.  Aggregate
decoded tokens per second (prefills included in both: admission prefills are serve's cost), their ratio, the ratio of replay
counts the host simulation gives for the same lengths (slot_scheduler.replay_count), and serve's mean idle-row fraction.
--repeats interleaved repetitions, medians reported.  One JSON line.

    python tools/serve_bench.py [--out profiles/r10_serve.json]
    python tools/serve_bench.py --only-serve        # (b) alone, warm + one: the run to put under rocprofv3 --kernel-trace --stats
    python tools/serve_bench.py --lookup 3 7 --repeats 5 [--out profiles/serve_lookup_bench.json]

--lookup K [K ...]: prompt-lookup drafts in the serving loop (serve(lookup=K)) against plain serve, legs interleaved in
one process: per K a leg whose corpus is the plain leg's own output of the request behind what serve gives it (every draft right)
and a leg with an empty corpus (nothing to copy but the sequence's own output).  Medians of --repeats; tokens per second over the
whole run, prefills included, plus replays and tokens per replay.  With ``--slot-kv int8 [--slot-drop-fp16]`` every right-corpus leg
runs once more over int8 K/V images (serve(lookup=K, slot_kv="int8"[, keep_arenas=False])).
With ``--loop-prefill`` the legs are, per K and corpus, serve(lookup=K) with serial admission prefills against
serve(lookup=K, loop_prefill=True), interleaved with the order rotating: tokens per second, replays and the per-request time to the
first token as median [min .. max].

    python tools/serve_bench.py --lookup 3 7 --loop-prefill --repeats 5 [--out profiles/serve_loop_prefill_bench.json]
"""
import argparse
import dataclasses
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prompt-cache_amd")]
from promptcache_amd import CacheEngine, GenerationEngine, GenerationParameters, Prompt, synth  # noqa: E402
from promptcache_amd.model import Llama2  # noqa: E402
from promptcache_amd.slot_scheduler import replay_count  # noqa: E402


def waves(ge, eng, prompts, lens, slots):
    """(a): waves of ``slots`` prompts through generate_batch, each wave with ONE max_new_tokens (its longest request: the shorter
    ones are cut on the host, their rows stay in the step).  -> (seconds, tokens that were asked for, replays)."""
    torch.cuda.synchronize()
    t0, replays = time.perf_counter(), 0
    for w in range(0, len(prompts), slots):
        chunk, want = prompts[w:w + slots], lens[w:w + slots]
        params = GenerationParameters(temperature=0.0, max_new_tokens=max(want), stop_token_ids=[], stop_str=[])
        reqs = [eng.process(p, slot=k) for k, p in enumerate(chunk)]
        for _k, _out in ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, stream_interval=10 ** 9):
            pass
        replays += max(want) - 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, sum(lens), replays


def served(ge, eng, prompts, lens, lookup=0, **kw):
    """(b): serve (``kw``: further arguments of ``serve``).  -> (seconds, tokens decoded, replays, idle-row fraction)."""
    base = GenerationParameters(temperature=0.0, stop_token_ids=[], stop_str=[])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _r, _out in ge.serve(eng, ((p, dataclasses.replace(base, max_new_tokens=n)) for p, n in zip(prompts, lens)),
                             stream_interval=10 ** 9, lookup=lookup, **kw):
        pass
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = ge.last_serve_stats
    return dt, sum(len(t) for t in ge.last_serve_tokens.values()), st["replays"], 1.0 - st["live_rows"] / max(1, st["replays"] * eng.slots)


def lookup_legs(ge, eng, prompts, lens, ks, repeats, slots, modes=None):
    """Plain serve and, per k, serve(lookup=k) with a full-acceptance and an empty corpus, interleaved.  -> the result dict.
    ``modes`` (``--slot-kv int8 [--slot-drop-fp16]``): name -> further arguments of ``serve``; every lookup leg with
    the right corpus then runs once more per mode (``lookup3_right_int8``, ...), in the same interleaving."""
    real = type(ge)._lookup_corpus
    served(ge, eng, prompts, lens)                                    # (the plain leg's outputs: what a right draft copies)
    answers = {r: list(t) for r, t in ge.last_serve_tokens.items()}

    def leg(k, corpus, kw):
        order = iter(range(len(prompts)))                             # (asked once per request, in the order they are pulled)
        if corpus == "right":
            ge._lookup_corpus = lambda cache, ids: real(cache, ids) + answers[next(order)]
        elif corpus == "none":
            ge._lookup_corpus = lambda cache, ids: []
        try:
            dt, n, replays, idle = served(ge, eng, prompts, lens, k, **kw)
        finally:
            ge.__dict__.pop("_lookup_corpus", None)
        same = sum(answers[r] == list(t) for r, t in ge.last_serve_tokens.items())
        return dict(tok_s=n / dt, replays=replays, tokens=n, seconds=dt, same_as_plain=same)
    legs = [("plain", 0, None, {})] + [(f"lookup{k}_{c}", k, c, {}) for k in ks for c in ("right", "none")]
    legs += [(f"lookup{k}_right_{m}", k, "right", kw) for k in ks for m, kw in (modes or {}).items()]
    for name, k, c, kw in legs[1:]:
        leg(k, c, kw)                                                 # warm: the (S, k) step is captured
    runs = {name: [] for name, _, _, _ in legs}
    for _ in range(repeats):
        for name, k, c, kw in legs:
            runs[name].append(leg(k, c, kw))
            print(f"{name}: {runs[name][-1]['tok_s']:.1f} tok/s, {runs[name][-1]['replays']} replays", file=sys.stderr, flush=True)
    out = {}
    for name, rs in runs.items():
        out[name] = {"tok_s": round(statistics.median(r["tok_s"] for r in rs), 1), "replays": rs[-1]["replays"], "tokens": rs[-1]["tokens"],
                     "tokens_per_replay": round(rs[-1]["tokens"] / max(1, rs[-1]["replays"]), 2),
                     "requests_equal_to_plain": rs[-1]["same_as_plain"]}
    for name in out:
        out[name]["over_plain"] = round(out[name]["tok_s"] / out["plain"]["tok_s"], 3)
    return {"shape": "llama2-7b (random init)", "requests": len(prompts), "slots": slots, "max_new_tokens": lens,
            "how": "greedy; decoded tokens per second over the whole serve run, prefills included; plain serve and serve(lookup=k) legs "
                   f"interleaved in one process, {repeats} repetitions, median; 'right': the corpus holds the plain leg's output of the "
                   "request (every draft right), 'none': an empty corpus (nothing to copy but the sequence's own output)",
            "legs": out}


def loop_prefill_legs(ge, eng, prompts, lens, ks, repeats, slots):
    """Per k and corpus ('right' / 'none' as in ``lookup_legs``): serve(lookup=k) and serve(lookup=k, loop_prefill=True), interleaved
    in one process with the order rotating.  -> the result dict: tok/s over the whole run, replays and the time to the first token
    of the requests admitted into the running loop (those behind the first fill), each as median [min .. max]."""
    real = type(ge)._lookup_corpus
    served(ge, eng, prompts, lens)
    answers = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    base = GenerationParameters(temperature=0.0, stop_token_ids=[], stop_str=[])

    def leg(k, corpus, in_loop):
        order = iter(range(len(prompts)))
        if corpus == "right":
            ge._lookup_corpus = lambda cache, ids: real(cache, ids) + answers[next(order)]
        else:
            ge._lookup_corpus = lambda cache, ids: []
        ttft = {}
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r, out in ge.serve(eng, ((p, dataclasses.replace(base, max_new_tokens=n)) for p, n in zip(prompts, lens)),
                                   stream_interval=10 ** 9, lookup=k, loop_prefill=in_loop):
                ttft.setdefault(r, out.elapsed_time)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            ge.__dict__.pop("_lookup_corpus", None)
        st = ge.last_serve_stats
        n = sum(len(t) for t in ge.last_serve_tokens.values())
        same = sum(answers[r] == list(t) for r, t in ge.last_serve_tokens.items())
        return dict(tok_s=n / dt, replays=st["replays"], tokens=n, ttft=[ttft[r] for r in sorted(ttft) if r >= slots],
                    loop_prefills=st.get("loop_prefills", 0), same_as_plain=same)

    def mmm(v, nd=1):
        return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}
    legs = [(f"lookup{k}_{c}_{'loop' if il else 'serial'}", k, c, il) for k in ks for c in ("right", "none") for il in (False, True)]
    for _, k, c, il in legs:
        leg(k, c, il)                                                 # warm: both (S, k) steps captured
    runs = {name: [] for name, _, _, _ in legs}
    for r in range(repeats):
        for j in range(0, len(legs), 2):                              # (the two legs of a pair side by side, the order rotating)
            for name, k, c, il in (legs[j:j + 2] if r % 2 == 0 else legs[j:j + 2][::-1]):
                runs[name].append(leg(k, c, il))
                print(f"{name}: {runs[name][-1]['tok_s']:.1f} tok/s, {runs[name][-1]['replays']} replays", file=sys.stderr, flush=True)
    out = {}
    for name, rs in runs.items():
        out[name] = {"tok_s": mmm([r["tok_s"] for r in rs]), "replays": mmm([r["replays"] for r in rs], 0), "tokens": rs[-1]["tokens"],
                     "ttft_ms_admitted": mmm([t for r in rs for t in r["ttft"]], 2), "loop_prefills": rs[-1]["loop_prefills"],
                     "requests_equal_to_plain": rs[-1]["same_as_plain"]}
    for name in out:
        if name.endswith("_loop"):
            serial = out[name[:-4] + "serial"]
            out[name]["median_over_serial_median"] = round(out[name]["tok_s"]["median"] / serial["tok_s"]["median"], 3)
            out[name]["gain_claimed"] = out[name]["tok_s"]["median"] > serial["tok_s"]["max"]
    return {"shape": "llama2-7b (random init)", "requests": len(prompts), "slots": slots, "max_new_tokens": lens,
            "how": "greedy; decoded tokens per second over the whole serve run; serve(lookup=k) with serial admission prefills against "
                   f"serve(lookup=k, loop_prefill=True), one process, pairs interleaved with the order rotating, {repeats} repetitions, "
                   "median [min .. max]; ttft_ms_admitted: Output.elapsed_time of the first output of every request behind the first "
                   "fill (serial: the prefill's device time; loop: wall time from admission to the read of the first token); a gain "
                   "is claimed only where the in-loop median exceeds the serial leg's maximum", "legs": out}


def slot_drop_legs(ge, eng, prompts, lens, repeats, slots, fmt_w):
    """serve(slot_kv="int8") and serve(slot_kv="int8", keep_arenas=False), interleaved with the order rotating."""
    legs = {"int8": dict(slot_kv="int8"), "int8_only": dict(slot_kv="int8", keep_arenas=False)}
    answers = {}
    for name, kw in legs.items():                                     # warm: both steps captured
        served(ge, eng, prompts, lens, **kw)
        answers[name] = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    runs = {name: [] for name in legs}
    for r in range(repeats):
        for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            dt, n, replays, _ = served(ge, eng, prompts, lens, **legs[name])
            runs[name].append(n / dt)
            print(f"{name}: {n / dt:.1f} tok/s, {replays} replays", file=sys.stderr, flush=True)
    out = {name: {"tok_s": {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}}
           for name, v in runs.items()}
    return {"shape": "llama2-7b (random init)", "weight_format": fmt_w, "requests": len(prompts), "slots": slots, "max_new_tokens": lens,
            "how": "greedy; decoded tokens per second over the whole serve run, prefills included; legs interleaved in one process, "
                   f"order rotating, {repeats} repetitions", "legs": out,
            "requests_with_equal_tokens": sum(answers["int8"][r] == answers["int8_only"][r] for r in answers["int8"])}


def share_trunk_legs(ge, eng, prompts, lens, repeats, slots, fmt_w):
    """serve(slot_kv="int8") -- the baseline --, serve(slot_kv="int8", share_trunk=True) and, for context, the fp16
    serve(share_trunk=True), interleaved in one process with the order rotating.  tok/s over the whole run, median [min .. max]; a
    gain is claimed only where the shared median exceeds the unshared leg's maximum."""
    legs = {"int8": dict(slot_kv="int8"), "int8_trunk": dict(slot_kv="int8", share_trunk=True), "fp16_trunk": dict(share_trunk=True)}
    answers = {}
    for name, kw in legs.items():                                     # warm: every step captured
        served(ge, eng, prompts, lens, **kw)
        answers[name] = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    runs = {name: [] for name in legs}
    names = list(legs)
    for r in range(repeats):
        for name in names[r % len(names):] + names[:r % len(names)]:
            dt, n, replays, _ = served(ge, eng, prompts, lens, **legs[name])
            runs[name].append(n / dt)
            print(f"{name}: {n / dt:.1f} tok/s, {replays} replays", file=sys.stderr, flush=True)
    out = {name: {"tok_s": {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}}
           for name, v in runs.items()}
    out["int8_trunk"]["median_over_int8_median"] = round(out["int8_trunk"]["tok_s"]["median"] / out["int8"]["tok_s"]["median"], 3)
    out["int8_trunk"]["gain_claimed"] = out["int8_trunk"]["tok_s"]["median"] > out["int8"]["tok_s"]["max"]
    return {"shape": "llama2-7b (random init)", "weight_format": fmt_w, "requests": len(prompts), "slots": slots, "max_new_tokens": lens,
            "how": "greedy; decoded tokens per second over the whole serve run, prefills included; legs interleaved in one process, "
                   f"order rotating, {repeats} repetitions, median [min .. max]", "legs": out,
            "requests_with_equal_tokens": sum(answers["int8"][r] == answers["int8_trunk"][r] for r in answers["int8"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share-trunk", action="store_true",
                    help="serve(slot_kv='int8') against serve(slot_kv='int8', share_trunk=True) and the fp16 serve(share_trunk=True) "
                         "(DESIGN 3.33); --out merges under the weight format and the slot count")
    ap.add_argument("--lookup", type=int, nargs="*", default=[])
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-serve", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--slot-drop-fp16", action="store_true",
                    help="serve(slot_kv='int8') against serve(slot_kv='int8', keep_arenas=False); --out merges under the weight format")
    ap.add_argument("--slot-kv", default="fp16", help="int8 with --lookup: add serve(lookup=k, slot_kv='int8') legs (and, with "
                                                      "--slot-drop-fp16, keep_arenas=False legs) to the lookup legs")
    ap.add_argument("--loop-prefill", action="store_true",
                    help="with --lookup: serve(lookup=k) against serve(lookup=k, loop_prefill=True) (DESIGN 3.30)")
    ap.add_argument("--weight-format", default="fp16", help="fp16 or mxfp4 (with PC_W4_STREAM / PC_W4_MAX_ROWS from the environment)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "serve_bench measures on the GPU"
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0, weight_format=args.weight_format)
    eng = CacheEngine(4096, lm, slots=args.slots)
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    cut = pp.rfind("</prompt>")
    prompts = [Prompt(pp[:cut] + f"<user>{synth.words(4 + r % 5, 7000 + r)}</user>" + pp[cut:], [fmt]) for r in range(args.requests)]
    rng = random.Random(10)
    lens = [rng.choice((16, 32, 64, 128)) for _ in range(args.requests)]                 # drawn once, fixed seed
    ge = GenerationEngine(lm)
    assert ge.serve_plan()[0], ge.serve_plan()[1]
    served(ge, eng, prompts, lens)                                    # warm: graphs captured, code objects loaded
    if args.share_trunk:
        res = share_trunk_legs(ge, eng, prompts, lens, args.repeats, args.slots, args.weight_format)
        if args.out:
            merged = {}
            if os.path.exists(args.out):
                with open(args.out) as fh:
                    merged = json.loads(fh.read() or "{}")
            merged.setdefault("serve", {})[f"weights_{args.weight_format}_S{args.slots}"] = res
            with open(args.out, "w") as fh:
                fh.write(json.dumps(merged, indent=1) + "\n")
        print(json.dumps(res))
        return
    if args.lookup and args.loop_prefill:
        res = loop_prefill_legs(ge, eng, prompts, lens, args.lookup, args.repeats, args.slots)
        res["weight_format"] = args.weight_format
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
        return
    if args.lookup and args.slot_kv == "int8":                         # serve(lookup=k) over fp16 arenas against the int8 modes
        modes = {"int8": dict(slot_kv="int8")}
        if args.slot_drop_fp16:
            modes["int8_only"] = dict(slot_kv="int8", keep_arenas=False)
        res = lookup_legs(ge, eng, prompts, lens, args.lookup, args.repeats, args.slots, modes)
        res["weight_format"] = args.weight_format
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        print(json.dumps(res))
        return
    if args.slot_drop_fp16:
        res = slot_drop_legs(ge, eng, prompts, lens, args.repeats, args.slots, args.weight_format)
        if args.out:
            merged = {}
            if os.path.exists(args.out):
                with open(args.out) as fh:
                    merged = json.loads(fh.read() or "{}")
            merged.setdefault("serve", {})["weights_" + args.weight_format] = res
            with open(args.out, "w") as fh:
                fh.write(json.dumps(merged, indent=1) + "\n")
        print(json.dumps(res))
        return
    if args.lookup:
        line = json.dumps(lookup_legs(ge, eng, prompts, lens, args.lookup, args.repeats, args.slots))
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    if args.only_serve:
        dt, n, replays, idle = served(ge, eng, prompts, lens)
        print(json.dumps({"serve_tok_s": round(n / dt, 1), "replays": replays, "idle_row_fraction": round(idle, 3)}))
        return
    waves(ge, eng, prompts, lens, args.slots)
    a, b = [], []
    for _ in range(args.repeats):
        a.append(waves(ge, eng, prompts, lens, args.slots))
        b.append(served(ge, eng, prompts, lens))
    ra = statistics.median(n / dt for dt, n, _ in a)
    rb = statistics.median(n / dt for dt, n, _, _ in b)
    sim_waves = sum(max(lens[w:w + args.slots]) - 1 for w in range(0, len(lens), args.slots))
    sim_serve = replay_count(lens, args.slots)
    result = {"shape": "llama2-7b (random init)", "requests": args.requests, "slots": args.slots, "max_new_tokens": lens,
              "how": "greedy; decoded tokens per second over the whole run, prefills included; (a) generate_batch in waves of "
                     f"{args.slots}, (b) serve; {args.repeats} interleaved repetitions, median",
              "waves_tok_s": round(ra, 1), "serve_tok_s": round(rb, 1), "serve_over_waves": round(rb / ra, 3),
              "replays_waves": sim_waves, "replays_serve_simulated": sim_serve, "replays_serve_measured": b[-1][2],
              "replay_count_ratio": round(sim_waves / sim_serve, 3), "serve_idle_row_fraction": round(statistics.median(x[3] for x in b), 3),
              "waves_idle_row_fraction": round(1.0 - sum(n - 1 for n in lens) / (sim_waves * args.slots), 3)}
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
