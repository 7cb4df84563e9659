"""fp16 vs int8 module KV store (CacheEngine(module_kv=...)) on bench.py's workload, in ONE process with interleaved repetitions.

Legs (llama2-7b shape, random weights, the persona schema and prompt of bench.py; every leg re-stages the whole prompt per step):
  host/fp16, host/int8          module KV in pinned host memory, gathered over PCIe (pc_kv_gather / pc_kv_gather_q8)
  device/fp16                   the default: staging left to the first forward's attention launches (no gather launch)
  device/fp16-explicit          PC_DEFER_GATHER=0's step: kv_copy_kernel on the same rows the int8 leg expands
  device/int8                   pc_kv_gather_q8 from HBM
Per leg: store bytes (CacheEngine.module_bytes), gather ms (HIP events around the launch, median) and TTFT ms (wall clock around
process() + the first lm() call + synchronize, as bench.py times its step; median and mean).  Accuracy record: max |logit_int8mode -
logit_fp16mode| over the prompt's rows and how many of the first 32 greedy tokens agree.

    python tools/kv_q8_bench.py --steps 40 --warmup 8 --out profiles/r08_kv_q8.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "prompt-cache_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--max-ctx", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--greedy-tokens", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_kv_q8.json"))
    a = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    ge.build()
    from promptcache_amd import CacheEngine, GenerationEngine, GenerationParameters, Prompt, synth
    from promptcache_amd.model import Llama2

    lm = Llama2(a.model, device="cuda:0", random_init=True, seed=0)
    fmt = lm.get_formatter()
    schema_pml, prompt_pml = synth.persona_like()
    prompt = Prompt(prompt_pml, [fmt])
    L, Hkv, D = lm.get_cache_shape()

    legs = {}
    for tier in ("host", "device"):
        for kv in ("fp16", "int8"):
            eng = CacheEngine(a.max_ctx, lm, module_memory=tier, module_kv=kv)
            eng.add_schema(fmt(schema_pml))
            eng.prompt_cache.record_events = True
            legs[f"{tier}/{kv}"] = eng
    names = ["host/fp16", "host/int8", "device/fp16", "device/fp16-explicit", "device/int8"]
    samples = {n: dict(ttft=[], gather=[]) for n in names}

    def step(name):
        eng = legs[name.replace("-explicit", "")]
        pc = eng.prompt_cache
        deferred = pc.defer_gather
        if name.endswith("-explicit"):
            pc.defer_gather = False
        try:
            pc.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, pos, _, cache = eng.process(prompt)
            out = lm(input_ids=torch.tensor([ids], dtype=torch.long), position_ids=torch.tensor([pos], dtype=torch.long),
                     past_key_values=cache, use_cache=True)
            torch.cuda.synchronize()
            ttft = (time.perf_counter() - t0) * 1e3
        finally:
            pc.defer_gather = deferred
        ev = pc.last_gather_events
        return ttft, (ev[0].elapsed_time(ev[1]) if ev is not None else None), len(pc), len(ids), out

    logits = {}
    for it in range(a.warmup + a.steps):
        for name in (names if it % 2 == 0 else names[::-1]):        # interleaved, order alternating
            ttft, gather, S, q, out = step(name)
            if it >= a.warmup:
                samples[name]["ttft"].append(ttft)
                if gather is not None:
                    samples[name]["gather"].append(gather)
            logits[name] = out.logits[0].float().clone()

    P = L * 2 * Hkv
    moved = {"fp16": S * P * D * 2 * 2, "int8": S * P * (D + 4) + S * P * D * 2}      # bytes read + written per gather
    result = {"workload": f"{a.model} shape (random weights), persona schema and prompt of bench.py: S = {S} staged rows, q = {q} new tokens, "
                          f"{len(legs['device/int8'].prompt_cache.staged)} segments; {a.steps} interleaved steps after {a.warmup} warm-up",
              "legs": {}}
    for name in names:
        kv = "int8" if name.endswith("int8") else "fp16"
        eng = legs[name.replace("-explicit", "")]
        g = samples[name]["gather"]
        gm = statistics.median(g) if g else None
        result["legs"][name] = {
            "store_bytes": eng.module_bytes("persona"),
            "gather_ms_median": gm, "gather_ms_min": min(g) if g else None,
            "gather_bytes_moved": moved[kv] if g else None,
            "gather_GBps": (moved[kv] / (gm * 1e-3) / 1e9) if g else None,
            "ttft_ms_median": statistics.median(samples[name]["ttft"]), "ttft_ms_mean": statistics.fmean(samples[name]["ttft"]),
        }
    lg = result["legs"]
    result["ratios"] = {
        "store_bytes_int8_over_fp16": lg["device/int8"]["store_bytes"] / lg["device/fp16"]["store_bytes"],
        "host_gather_int8_over_fp16": lg["host/int8"]["gather_ms_median"] / lg["host/fp16"]["gather_ms_median"],
        "host_ttft_int8_over_fp16": lg["host/int8"]["ttft_ms_median"] / lg["host/fp16"]["ttft_ms_median"],
        "device_gather_int8_over_kv_copy": lg["device/int8"]["gather_ms_median"] / lg["device/fp16-explicit"]["gather_ms_median"],
        "device_ttft_int8_over_fp16_default": lg["device/int8"]["ttft_ms_median"] / lg["device/fp16"]["ttft_ms_median"],
    }

    # ---- accuracy of the format on this workload (a property of the format, recorded, not bounded) ----
    def greedy(name):
        eng = legs[name]
        ids, pos, _, cache = eng.process(prompt)
        params = GenerationParameters(temperature=0.0, max_new_tokens=a.greedy_tokens, stop_token_ids=[], stop_str=[])
        return [o.new_text for o in GenerationEngine(lm).generate(ids, pos, params, cache, stream_interval=1)]

    t16, t8 = greedy("device/fp16"), greedy("device/int8")
    agree = 0
    for x, y in zip(t16, t8):
        if x != y:
            break
        agree += 1
    result["accuracy"] = {
        "max_abs_logit_diff_int8_vs_fp16_mode": float((logits["device/int8"] - logits["device/fp16"]).abs().max()),
        "max_abs_logit_fp16_mode": float(logits["device/fp16"].abs().max()),
        "host_tier_equals_device_tier_bitwise": bool(torch.equal(logits["host/int8"], logits["device/int8"])),
        "greedy_tokens_compared": min(len(t16), len(t8)), "greedy_tokens_agreeing_prefix": agree,
        "first_greedy_tokens_agree": agree == min(len(t16), len(t8)) == a.greedy_tokens,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
