"""Continuous batching against static waves, same process, same box: 7b shape (random init), bench.py's persona schema, greedy,
32 prompts through 8 slots with max_new_tokens drawn once from {16, 32, 64, 128} (fixed seed).  (a) generate_batch in four waves of
8 -- a wave lasts as long as its longest sequence -- and (b) serve, which refills a slot as soon as its sequence ends.  Aggregate
decoded tokens per second (prefills included in both: admission prefills are serve's cost), their ratio, the ratio of replay
counts the host simulation gives for the same lengths (slot_scheduler.replay_count), and serve's mean idle-row fraction.
--repeats interleaved repetitions, medians reported.  One JSON line.

    python tools/serve_bench.py [--out profiles/r10_serve.json]
    python tools/serve_bench.py --only-serve        # (b) alone, warm + one: the run to put under rocprofv3 --kernel-trace --stats
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


def served(ge, eng, prompts, lens):
    """(b): serve.  -> (seconds, tokens decoded, replays, idle-row fraction)."""
    base = GenerationParameters(temperature=0.0, stop_token_ids=[], stop_str=[])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _r, _out in ge.serve(eng, ((p, dataclasses.replace(base, max_new_tokens=n)) for p, n in zip(prompts, lens)),
                             stream_interval=10 ** 9):
        pass
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = ge.last_serve_stats
    return dt, sum(len(t) for t in ge.last_serve_tokens.values()), st["replays"], 1.0 - st["live_rows"] / max(1, st["replays"] * eng.slots)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-serve", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "serve_bench measures on the GPU"
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0)
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
