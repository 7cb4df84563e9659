"""What the token-control node costs: 7b shape (random init, V = 32 000), bench.py's persona schema, one process, the
legs of every comparison interleaved with the order rotating.

  (a) the GreedyLoop step with controls off / on
  (b) the SlotLoop step at S = 8 with controls off / on
  (c) the LookupSlotLoop step at S = 8, k = 3 (32 rows) with controls off / on
  (d) pc_logit_adjust alone at rows 1 / 8 / 32 / 64, V = 32 000 / 128 256, under a full block

"on" is the worst block a request can bring: 64 bias entries, an allow-list and ``min_new_tokens`` with 8 stop ids held back on
every row.  "off" is the step as it is without the feature: same graph keys, same launches.  Step times come from the HIP events
around one replay (``elapsed_ms``), kernel times from events around a run of back-to-back launches; median [min .. max] per leg.
There is no pass threshold: the option is opt-in and costs what it costs.  What the run records is whether the median of the on
leg lies inside the off leg's own min .. max spread.

    python tools/token_controls_bench.py [--steps 48] [--repeats 3] [--out profiles/token_controls_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prompt-cache_amd")]
from promptcache_amd import CacheEngine, Prompt, _native, synth  # noqa: E402
from promptcache_amd.model import Llama2  # noqa: E402
from promptcache_amd.modes import token_controls  # noqa: E402

DEV = "cuda:0"


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def compare(times, names):
    """One row: every leg's summary, each leg's median minus the off leg's, and whether it lies inside the off leg's spread."""
    row = {f"{nm}_ms": summary(times[nm]) for nm in names}
    off = row[f"{names[0]}_ms"]
    row["off_spread_ms"] = round(off["max"] - off["min"], 4)
    for nm in names[1:]:
        row[f"{nm}_minus_off_ms"] = round(row[f"{nm}_ms"]["median"] - off["median"], 4)
        row[f"{nm}_median_inside_off_min_max"] = off["min"] <= row[f"{nm}_ms"]["median"] <= off["max"]
    return row


def interleaved(legs, run, repeats):
    """``run(leg)`` -> ms list; repetition 0 (graph capture) dropped, the order rotating from one repetition to the next."""
    times = {nm: [] for nm in legs}
    for r in range(repeats + 1):
        order = legs[r % len(legs):] + legs[:r % len(legs)]
        for nm in order:
            ms = run(nm)
            if r:
                times[nm] += ms
    return times


def full_controls(V, first):
    """64 bias entries (half of them bans), an allow-list of every fourth token and 8 stop ids held back for the whole run."""
    bias = {1 + 97 * j: (-float("inf") if j % 2 else 0.25 * j) for j in range(64)}
    return token_controls(logit_bias=bias, allowed_token_ids=sorted(set(range(0, V, 4)) | {first}), min_new_tokens=10 ** 6,
                          stop_token_ids=[8 * j for j in range(8)], vocab=V)


def kernel_alone(repeats):
    rows_out = {}
    launches = 50
    for V in (32000, 128256):
        x = torch.randn((64, V), dtype=torch.float32, device=DEV) * 3.0
        out = torch.empty((64, V), dtype=torch.float32, device=DEV)
        ctl = full_controls(V, 0)
        blk = _native.logit_ctl_bytes(ctl.bias, True, 10 ** 6, ctl.stop_ids)
        bits = torch.zeros((V + 31) // 32, dtype=torch.int32)
        bits[:] = 0x11111111
        for R in (1, 8, 32, 64):
            S, rps = (R, 1) if R <= 8 else (R // 4, 4)
            blocks = torch.frombuffer(bytearray(blk * S), dtype=torch.uint8).to(DEV)
            allowed = bits.repeat(S, 1).to(DEV)
            length = torch.zeros(S, dtype=torch.int32, device=DEV)
            us = []
            for r in range(repeats + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    _native.logit_adjust(x, V, V, S, rps, blocks, allowed, length, out, V)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    us.append(e0.elapsed_time(e1) * 1e3 / launches)
            rows_out[f"V={V} rows={R}"] = {"us_per_launch": summary(us), "bytes_moved": 2 * R * V * 4}
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "token_controls_bench measures on the GPU"
    steps, warm, S, k = args.steps, 8, 8, 3
    lm = Llama2("llama2-7b", device=DEV, random_init=True, seed=0)
    m = lm.hf_model
    V = m.config.vocab_size
    eng = CacheEngine(4096, lm, slots=S)
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    prompt = Prompt(pp, [fmt])
    pre = []
    for s in range(S):
        ids, pos, _, cache = eng.process(prompt, slot=s)
        out = lm(input_ids=torch.tensor([ids], device=DEV), position_ids=torch.tensor([pos], device=DEV), past_key_values=cache, use_cache=True)
        past = out.past_key_values
        pre.append((past, past.arena.length, int(torch.argmax(out.logits[0, -1])), max(pos) + 2))
    keys = pre[0][1]
    ctl = full_controls(V, pre[0][2])
    kw_of = {"off": {}, "on": {"token_controls": ctl}}

    def pasts(n):
        for past, n0, _, _ in pre[:n]:
            past.arena.length = n0                                            # (rows behind it are dead: the loop rewrites them)
        return [p[0] for p in pre[:n]]

    def timed(loop, consumed):
        try:
            for _ in range(steps):
                loop.enqueue()
            return [loop.elapsed_ms(i) for i in range(warm, steps)]
        finally:
            loop.close(consumed)

    def greedy(leg):
        return timed(m.greedy_loop(pasts(1)[0], pre[0][2], pre[0][3], steps + 1, **kw_of[leg]), 0)

    def slots(leg):
        return timed(m.slot_loop(pasts(S), [p[2] for p in pre], [p[3] for p in pre], steps + 1, **kw_of[leg]), [0] * S)

    def lookup_slots(leg):
        return timed(m.lookup_slot_loop(pasts(S), [p[2] for p in pre], [p[3] for p in pre], steps * (k + 1) + 1, k, [[] for _ in range(S)],
                                        **kw_of[leg]), [0] * S)

    base = set(m._graphs)
    legs = ["off", "on"]
    result = {"shape": f"llama2-7b (random init), V = {V}", "prompt": f"persona schema, {keys} keys per sequence after the prefill",
              "steps": steps, "warm_steps_dropped": warm, "repeats": args.repeats,
              "controls_on": "64 bias entries (32 of them bans), an allow-list of every fourth token, min_new_tokens with 8 stop ids held "
                             "back on every row",
              "how": "loops stepped by hand, greedy; ms per replay from the HIP events around it (elapsed_ms), steps "
                     f"{warm}..{steps - 1} of every repetition; legs interleaved, order rotating, repetition 0 dropped; median [min .. max]; "
                     "kernel alone: events around 50 back-to-back launches",
              "greedy_loop": compare(interleaved(legs, greedy, args.repeats), legs),
              "slot_loop_S8": compare(interleaved(legs, slots, args.repeats), legs),
              "lookup_slot_loop_S8_k3": compare(interleaved(legs, lookup_slots, args.repeats), legs),
              "kernel_alone": kernel_alone(args.repeats)}
    new = set(m._graphs) - base
    result["graph_keys"] = {"off_without_ctl": sum("ctl" not in key for key in new), "on_with_ctl": sum("ctl" in key for key in new)}
    line = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
