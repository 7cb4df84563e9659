"""Batched decode against one-after-another decode, same process, same box: 7b shape (random init), bench.py's persona schema,
greedy.  (a) B calls of generate() one after another through the device greedy loop -- how B prompts are served without
generate_batch -- and (b) generate_batch over B slots, for B in --batches; decode tokens per second summed over the sequences,
prefills excluded from both; --repeats interleaved repetitions, medians reported.  Also the byte-model ratio
B (W + K) / (W + B K) from the weight bytes W a decode step streams and the K/V bytes K a sequence's step reads.  One JSON line.

    python tools/batch_decode_bench.py [--new 64] [--out profiles/r09_batch_decode.json]
    python tools/batch_decode_bench.py --only-batch 8        # (b) at B = 8 alone: the run to put under rocprofv3 --kernel-trace --stats
    python tools/batch_decode_bench.py --share-trunk [--out profiles/r10_trunk_decode.json]
        # (c) as well: generate_batch(share_trunk=True), interleaved with (a) and (b) in the same process, next to the extended
        # byte model B (W + K) / (W + K_t + B K_o) (K_t: the shared staged rows, read once; K_o: a sequence's own rows)
    python tools/batch_decode_bench.py --slot-kv int8 [--weight-format mxfp4] [--out profiles/slot_kv_q8_bench.json]
        # the slot loop over int8 K/V images (slot_loop(kv="int8")) beside the fp16 slot loop: same process, same
        # model, same prefilled slots, S = 4 / 8 / 16; the two legs interleaved with the order rotating; step time from the HIP
        # events around one replay, median [min .. max]; plus the accuracy record of sequence 0: max |logit_int8 - logit_fp16|
        # of the first loop step and how many of 32 greedy tokens agree.  --out merges the run into the file under its
        # weight format, so the fp16 and the MXFP4 run share one JSON.
    python tools/batch_decode_bench.py --slot-kv int8 --slot-drop-fp16 [--weight-format mxfp4] [--out profiles/slot_kv_only_bench.json]
        # int8-only residency (slot_loop(kv="int8", keep_arenas=False)) beside today's int8 mode, S = 8 / 16: (a)
        # torch.cuda.memory_allocated() after the first fill for the fp16 loop, the int8 mode and int8-only -- the latter with
        # every sequence prefilled in ONE arena, measured before the other slots' arenas exist; (b) step time, legs interleaved
        # with the order rotating.  --out merges under "decode" / the weight format.
    python tools/batch_decode_bench.py --slot-kv int8 --share-trunk [--weight-format mxfp4] [--out profiles/slot_trunk_q8_bench.json]
        # shared trunks over int8 images (slot_loop(each=True, kv="int8", trunks=...)) beside the unshared int8 loop
        # and the fp16 shared trunk, S = 4 / 8 / 16, loops built directly (generate_batch refuses the pair); step time, legs
        # interleaved, next to the byte model (W + S K) / (W + K_t + S K_o).  --out merges under "decode" / the weight format.
        # --batches 8 --repeats 1: the run to put under rocprofv3 --kernel-trace --stats.
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
from promptcache_amd import CacheEngine, GenerationEngine, GenerationParameters, Prompt, synth  # noqa: E402
from promptcache_amd.model import Llama2  # noqa: E402


def serial_rate(ge, eng, prompt, params, B):
    """(a): B generations one after another; decode seconds = first Output to last Output of each, summed."""
    dt, n = 0.0, 0
    for _ in range(B):
        ids, pos, _, cache = eng.process(prompt)
        t0 = None
        for _out in ge.generate(ids, pos, params, cache, stream_interval=10 ** 9):
            if t0 is None:
                t0 = time.perf_counter()
        torch.cuda.synchronize()
        dt += time.perf_counter() - t0
        n += params.max_new_tokens - 1
    return n / dt


def batch_rate(ge, eng, prompt, params, B, share=False):
    """(b): one generate_batch over B slots; decode seconds = the last first-token Output (all prefills done) to the end.
    (c): the same with ``share_trunk=True``."""
    reqs = [eng.process(prompt, slot=k) for k in range(B)]
    firsts, t0 = 0, None
    for _k, _out in ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, stream_interval=10 ** 9, share_trunk=share):
        firsts += 1
        if firsts == B:
            t0 = time.perf_counter()
    torch.cuda.synchronize()
    return B * (params.max_new_tokens - 1) / (time.perf_counter() - t0)


def slot_kv_bench(args):
    """--slot-kv int8: fp16 leg and int8 leg of the slot loop, stepped by hand (SlotLoop.enqueue / elapsed_ms)."""
    steps, warm = max(args.new, 40), 8
    fmt_w = args.weight_format
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0, **({"weight_format": fmt_w} if fmt_w != "fp16" else {}))
    m = lm.hf_model
    sizes = [int(b) for b in args.batches.split(",")] if args.batches != "1,2,4,8,16" else [4, 8, 16]
    eng = CacheEngine(4096, lm, slots=max(sizes))
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    prompt = Prompt(pp, [fmt])
    pre = []                                                                   # per slot: (past, rows after the prefill, token, position)
    for k in range(max(sizes)):
        ids, pos, _, cache = eng.process(prompt, slot=k)
        out = lm(input_ids=torch.tensor([ids], device="cuda:0"), position_ids=torch.tensor([pos], device="cuda:0"),
                 past_key_values=cache, use_cache=True)
        past = out.past_key_values
        pre.append((past, past.arena.length, int(torch.argmax(out.logits[0, -1])), max(pos) + 2))
    keys = pre[0][1]
    result = {"shape": "llama2-7b (random init)", "weight_format": fmt_w, "prompt": f"persona schema, {keys} keys per slot after the prefill",
              "steps": steps, "warm_steps_dropped": warm, "repeats": args.repeats,
              "how": "SlotLoop stepped by hand, greedy; ms per replay from the HIP events around it (SlotLoop.elapsed_ms), steps "
                     f"{warm}..{steps - 1} of every repetition; legs interleaved, order rotating; median [min .. max]", "rows": {}}

    def leg(S, kv):
        pasts = []
        for past, n0, _, _ in pre[:S]:
            past.arena.length = n0                                             # (rows behind it are dead: the loop rewrites them)
            pasts.append(past)
        loop = m.slot_loop(pasts, [t for _, _, t, _ in pre[:S]], [p for _, _, _, p in pre[:S]], steps + 1, kv=kv)
        try:
            loop.enqueue()
            torch.cuda.synchronize()
            first = loop.logits[0].clone()
            for _ in range(steps - 1):
                loop.enqueue()
            toks = [loop.token(0, i) for i in range(steps)]
            ms = [loop.elapsed_ms(i) for i in range(warm, steps)]
        finally:
            loop.close([0] * S)
        return ms, first, toks

    for S in sizes:
        times = {"fp16": [], "int8": []}
        acc = None
        for r in range(args.repeats + 1):                                       # (repetition 0 captures the graphs: dropped)
            order = ["fp16", "int8"] if r % 2 == 0 else ["int8", "fp16"]
            got = {kv: leg(S, kv) for kv in order}
            if r == 0:
                d = float((got["int8"][1] - got["fp16"][1]).abs().max())
                agree = sum(int(a == b) for a, b in zip(got["int8"][2][:32], got["fp16"][2][:32]))
                first_diff = next((i for i, (a, b) in enumerate(zip(got["int8"][2][:32], got["fp16"][2][:32])) if a != b), None)
                acc = {"max_abs_dlogit_first_step": d, "greedy_tokens_agree_of_32": agree, "first_disagreement": first_diff,
                       "max_abs_logit_fp16_first_step": float(got["fp16"][1].abs().max())}
                continue
            for kv in order:
                times[kv] += got[kv][0]
        row = {}
        for kv in ("fp16", "int8"):
            row[kv + "_ms"] = {"median": round(statistics.median(times[kv]), 4), "min": round(min(times[kv]), 4),
                               "max": round(max(times[kv]), 4), "n": len(times[kv])}
        f, q = row["fp16_ms"], row["int8_ms"]
        row["gain_ms"] = round(f["median"] - q["median"], 4)
        row["gain_us_per_layer"] = round((f["median"] - q["median"]) * 1e3 / m.L, 2)
        row["fp16_spread_ms"] = round(f["max"] - f["min"], 4)
        row["int8_median_below_fp16_min"] = q["median"] < f["min"]
        row["gain_exceeds_fp16_spread"] = (f["median"] - q["median"]) > (f["max"] - f["min"])
        row["accuracy_sequence_0"] = acc
        row["kv_bytes_fp16_per_step"] = S * m.L * 2 * m.Hkv * keys * m.D * 2
        row["kv_bytes_int8_per_step"] = S * m.L * 2 * m.Hkv * keys * (m.D + 4)
        result["rows"][str(S)] = row
        print(json.dumps({str(S): row}), file=sys.stderr, flush=True)
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                merged = json.loads(fh.read() or "{}")
        merged["weights_" + fmt_w] = result
        with open(args.out, "w") as fh:
            fh.write(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))


def slot_kv_only_bench(args):
    """--slot-kv int8 --slot-drop-fp16: memory after the first fill and step time of the int8-only loop beside today's int8 mode."""
    import gc
    steps, warm = max(args.new, 40), 8
    fmt_w = args.weight_format
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0, **({"weight_format": fmt_w} if fmt_w != "fp16" else {}))
    m = lm.hf_model
    sizes = [int(b) for b in args.batches.split(",")] if args.batches != "1,2,4,8,16" else [8, 16]
    mem_model = torch.cuda.memory_allocated()
    eng = CacheEngine(4096, lm, slots=max(sizes))
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    prompt = Prompt(pp, [fmt])
    mem_engine = torch.cuda.memory_allocated()                                 # model + modules + slot 0's arena

    def prefill(slot):
        ids, pos, _, cache = eng.process(prompt, slot=slot)
        out = lm(input_ids=torch.tensor([ids], device="cuda:0"), position_ids=torch.tensor([pos], device="cuda:0"),
                 past_key_values=cache, use_cache=True)
        past = out.past_key_values
        return past, past.arena.length, int(torch.argmax(out.logits[0, -1])), max(pos) + 2

    def forget():                                                              # the loop states (images, fresh rows) and their graphs
        m.__dict__.pop("_slot_sts", None)
        m._graphs.clear()
        gc.collect()

    arena_bytes = eng.prompt_cache.arena.buf.numel() * 2
    mem = {}
    for S in sizes:                                                            # (a) int8-only first: one arena exists
        forget()
        loop = None
        for k in range(S):
            past, n0, tok, pos = prefill(0)
            if loop is None:
                loop = m.slot_loop([past], [tok], [pos], steps + 1, each=True, slots=S, slot_index=[0], max_keys=4096, kv="int8",
                                   keep_arenas=False)
            else:
                loop.admit(k, past, tok, pos, steps + 1, None, 0, (), ())
            del past
        torch.cuda.synchronize()
        mem[S] = {"int8_only": {"allocated": torch.cuda.memory_allocated(), "slot_kv_bytes": loop.slot_kv_bytes(),
                                "beyond_engine": torch.cuda.memory_allocated() - mem_engine}}
        loop.close({})
        del loop
    forget()
    pre = [prefill(k) for k in range(max(sizes))]                              # now every slot's arena exists
    keys = pre[0][1]
    for S in sizes:
        for kv in ("fp16", "int8"):
            forget()
            loop = m.slot_loop([p[0] for p in pre[:S]], [p[2] for p in pre[:S]], [p[3] for p in pre[:S]], steps + 1, each=True, slots=S,
                               max_keys=4096, kv=kv)
            torch.cuda.synchronize()
            # (arenas of slots S.. exist by now at the smaller S: counted out)
            extra = (max(sizes) - S) * arena_bytes
            mem[S][kv] = {"allocated": torch.cuda.memory_allocated() - extra, "slot_kv_bytes": loop.slot_kv_bytes(),
                          "beyond_engine": torch.cuda.memory_allocated() - extra - mem_engine}
            loop.close({})
            del loop
    forget()
    row_bytes = m.L * 2 * m.Hkv * m.D * 2
    result = {"shape": "llama2-7b (random init)", "weight_format": fmt_w, "prompt": f"persona schema, {keys} keys per slot after the prefill",
              "steps": steps, "warm_steps_dropped": warm, "repeats": args.repeats, "arena_rows": 4096,
              "memory_how": "torch.cuda.memory_allocated() with the loop built and every sequence entered (each=True, max_keys 4096); "
                            "beyond_engine: minus model + schema modules + slot 0's arena; int8_only measured before the arenas of slots "
                            "1.. exist, the other two with the arenas of slots beyond S counted out",
              "allocated_model": mem_model, "allocated_model_modules_one_arena": mem_engine, "arena_bytes": arena_bytes,
              "kv_row_bytes_fp16": row_bytes,
              "how": "SlotLoop stepped by hand, greedy; ms per replay from the HIP events around it (SlotLoop.elapsed_ms), steps "
                     f"{warm}..{steps - 1} of every repetition; legs interleaved, order rotating; median [min .. max]", "rows": {}}

    def leg(S, only):
        pasts = []
        for past, n0, _, _ in pre[:S]:
            past.arena.length = n0
            pasts.append(past)
        loop = m.slot_loop(pasts, [t for _, _, t, _ in pre[:S]], [p for _, _, _, p in pre[:S]], steps + 1, kv="int8",
                           **({"keep_arenas": False} if only else {}))
        try:
            for _ in range(steps):
                loop.enqueue()
            toks = [loop.token(0, i) for i in range(steps)]
            ms = [loop.elapsed_ms(i) for i in range(warm, steps)]
        finally:
            loop.close([0] * S)
        return ms, toks

    for S in sizes:
        times = {"int8": [], "int8_only": []}
        same = None
        for r in range(args.repeats + 1):                                       # (repetition 0 captures the graphs: dropped)
            order = ["int8", "int8_only"] if r % 2 == 0 else ["int8_only", "int8"]
            got = {name: leg(S, name == "int8_only") for name in order}
            if r == 0:
                same = got["int8"][1] == got["int8_only"][1]
                continue
            for name in order:
                times[name] += got[name][0]
        row = {name + "_ms": {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}
               for name, v in times.items()}
        row["int8_only_median_within_int8_max"] = row["int8_only_ms"]["median"] <= row["int8_ms"]["max"]
        row["tokens_of_sequence_0_equal"] = same
        row["memory"] = mem[S]
        row["arithmetic_bytes"] = {"fp16": S * 4096 * row_bytes, "int8": S * 4096 * row_bytes + S * 4096 * (row_bytes // 2 // m.D) * (m.D + 4),
                                   "int8_only": S * 4096 * (row_bytes // 2 // m.D) * (m.D + 4) + S * row_bytes + 4096 * row_bytes}
        result["rows"][str(S)] = row
        print(json.dumps({str(S): row}), file=sys.stderr, flush=True)
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                merged = json.loads(fh.read() or "{}")
        merged.setdefault("decode", {})["weights_" + fmt_w] = result
        with open(args.out, "w") as fh:
            fh.write(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))


def slot_trunk_q8_bench(args):
    """--slot-kv int8 --share-trunk: the each=True slot loop over int8 images without trunks (the baseline), with trunks
    (slot_loop(each=True, kv="int8", trunks=...)) and, for context, the fp16 loop with trunks; built directly, since
    generate_batch refuses the pair.  Same process, same prefilled slots, legs interleaved with the order rotating."""
    from promptcache_amd.model.kv_arena import common_trunks
    steps, warm = max(args.new, 40), 8
    fmt_w = args.weight_format
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0, **({"weight_format": fmt_w} if fmt_w != "fp16" else {}))
    m, c = lm.hf_model, lm.hf_model.config
    sizes = [int(b) for b in args.batches.split(",")] if args.batches != "1,2,4,8,16" else [4, 8, 16]
    eng = CacheEngine(4096, lm, slots=max(sizes))
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    prompt = Prompt(pp, [fmt])
    pre = []                                                                   # per slot: (past, rows after the prefill, token, position)
    for k in range(max(sizes)):
        ids, pos, _, cache = eng.process(prompt, slot=k)
        out = lm(input_ids=torch.tensor([ids], device="cuda:0"), position_ids=torch.tensor([pos], device="cuda:0"),
                 past_key_values=cache, use_cache=True)
        past = out.past_key_values
        pre.append((past, past.arena.length, int(torch.argmax(out.logits[0, -1])), max(pos) + 2))
    keys = pre[0][1]
    hid, inter = c.hidden_size, c.intermediate_size
    dec = 2 * m.L * ((m.H + 2 * m.Hkv) * m.D * hid + m.H * m.D * hid + 3 * inter * hid)          # fp16 bytes of the decoder linears
    W = (dec * 17 // 64 if fmt_w == "mxfp4" else dec) + 2 * c.vocab_size * hid                     # (4.25 bits per MXFP4 weight)
    result = {"shape": "llama2-7b (random init)", "weight_format": fmt_w, "prompt": f"persona schema, {keys} keys per slot after the prefill",
              "steps": steps, "warm_steps_dropped": warm, "repeats": args.repeats, "weight_bytes_per_step": W,
              "how": "SlotLoop(each=True, max_keys 4096) stepped by hand, greedy; ms per replay from the HIP events around it "
                     f"(SlotLoop.elapsed_ms), steps {warm}..{steps - 1} of every repetition; legs interleaved, order rotating; median "
                     "[min .. max]; byte model: (W + S K) / (W + K_t + S K_o) with int8 image bytes; a gain is claimed only where the "
                     "shared median lies below the unshared leg's minimum", "rows": {}}

    def leg(S, name):
        pasts = []
        for past, n0, _, _ in pre[:S]:
            past.arena.length = n0                                             # (rows behind it are dead: the loop rewrites them)
            pasts.append(past)
        trunks = None if name == "int8" else common_trunks([p.arena.layout for p in pasts])
        loop = m.slot_loop(pasts, [t for _, _, t, _ in pre[:S]], [p for _, _, _, p in pre[:S]], steps + 1, None, [0] * S, [()] * S, (),
                           slots=S, each=True, max_keys=4096, trunks=trunks, kv="fp16" if name == "fp16_trunk" else "int8")
        assert (loop.nsplit_trunk > 0) == (name != "int8"), (name, trunks)
        try:
            for _ in range(steps):
                loop.enqueue()
            toks = [loop.token(0, i) for i in range(steps)]
            ms = [loop.elapsed_ms(i) for i in range(warm, steps)]
        finally:
            loop.close({k: 0 for k in range(S)})
        return ms, toks, (trunks[0][1] if trunks else 0, loop.nsplit, loop.nsplit_trunk)

    names = ["int8", "int8_trunk", "fp16_trunk"]
    for S in sizes:
        times = {name: [] for name in names}
        same = info = None
        for r in range(args.repeats + 1):                                       # (repetition 0 captures the graphs: dropped)
            order = names[r % 3:] + names[:r % 3]
            got = {name: leg(S, name) for name in order}
            if r == 0:
                same = got["int8"][1] == got["int8_trunk"][1]
                info = got["int8_trunk"][2]
                continue
            for name in order:
                times[name] += got[name][0]
        row = {name + "_ms": {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}
               for name, v in times.items()}
        T = info[0]
        K, Kt = m.L * 2 * m.Hkv * keys * (m.D + 4), m.L * 2 * m.Hkv * T * (m.D + 4)
        u, s = row["int8_ms"], row["int8_trunk_ms"]
        row.update({"trunk_rows": T, "nsplit_own": info[1], "nsplit_trunk": info[2], "kv_bytes_int8_per_slot": K, "trunk_bytes_int8": Kt,
                    "byte_model_ratio": round((W + S * K) / (W + Kt + S * (K - Kt)), 3),
                    "unshared_over_shared": round(u["median"] / s["median"], 3),
                    "fraction_of_byte_model": round(u["median"] / s["median"] / ((W + S * K) / (W + Kt + S * (K - Kt))), 3),
                    "shared_median_below_unshared_min": s["median"] < u["min"], "tokens_of_sequence_0_equal": same})
        result["rows"][str(S)] = row
        print(json.dumps({str(S): row}), file=sys.stderr, flush=True)
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                merged = json.loads(fh.read() or "{}")
        merged.setdefault("decode", {})["weights_" + fmt_w] = result
        with open(args.out, "w") as fh:
            fh.write(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64, help="greedy tokens per sequence")
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-batch", type=int, default=0, help="run (b) at this B alone, twice (warm + one), and print its rate")
    ap.add_argument("--share-trunk", action="store_true", help="add leg (c): generate_batch(share_trunk=True)")
    ap.add_argument("--slot-kv", choices=("fp16", "int8"), default="fp16",
                    help="int8: measure the slot loop over int8 K/V images beside the fp16 slot loop (S = 4 / 8 / 16, or --batches)")
    ap.add_argument("--slot-drop-fp16", action="store_true",
                    help="with --slot-kv int8: measure int8-only residency (keep_arenas=False) beside today's int8 mode: memory and step time")
    ap.add_argument("--weight-format", choices=("fp16", "mxfp4"), default="fp16", help="with --slot-kv int8: the decoder weights")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "batch_decode_bench measures on the GPU"
    if args.slot_drop_fp16:
        assert args.slot_kv == "int8", "--slot-drop-fp16 needs --slot-kv int8"
        return slot_kv_only_bench(args)
    if args.slot_kv == "int8" and args.share_trunk:
        return slot_trunk_q8_bench(args)
    if args.slot_kv == "int8":
        return slot_kv_bench(args)
    batches = [int(b) for b in args.batches.split(",")]
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0)
    eng = CacheEngine(4096, lm, slots=max(batches + [args.only_batch]))
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    prompt = Prompt(pp, [fmt])
    ge = GenerationEngine(lm)
    params = GenerationParameters(temperature=0.0, max_new_tokens=args.new, stop_token_ids=[], stop_str=[])
    assert ge.batch_plan(max(batches), params)[0], ge.batch_plan(max(batches), params)[1]
    if args.only_batch:
        batch_rate(ge, eng, prompt, params, args.only_batch, args.share_trunk)
        row = {"B": args.only_batch, "batch_tok_s": round(batch_rate(ge, eng, prompt, params, args.only_batch, args.share_trunk), 1)}
        if args.share_trunk:
            row["share_trunk"] = True
        print(json.dumps(row))
        return

    m, c = lm.hf_model, lm.hf_model.config
    hid, inter = c.hidden_size, c.intermediate_size
    W = 2 * (m.L * ((m.H + 2 * m.Hkv) * m.D * hid + m.H * m.D * hid + 3 * inter * hid) + c.vocab_size * hid)      # fp16 bytes per step
    ids, _, _, cache = eng.process(prompt)
    staged = len(eng.prompt_cache)
    keys = staged + len(ids) + args.new // 2                                   # mean keys a step reads
    K = 2 * m.L * 2 * m.Hkv * m.D * keys
    result = {"shape": "llama2-7b (random init)", "prompt": f"persona schema, {staged} staged + {len(ids)} new tokens", "new_tokens": args.new,
              "how": "greedy; decode tok/s summed over sequences, prefills excluded; (a) B x generate one after another, (b) generate_batch; "
                     f"{args.repeats} interleaved repetitions, median", "weight_bytes": W, "kv_bytes_per_sequence": K, "rows": {}}
    Kt = 2 * m.L * 2 * m.Hkv * m.D * staged                                    # the rows every slot staged: one trunk
    for B in batches:                                                          # warm: graphs captured, code objects loaded
        batch_rate(ge, eng, prompt, params, B)
        if args.share_trunk:
            batch_rate(ge, eng, prompt, params, B, True)
    serial_rate(ge, eng, prompt, params, 1)
    a = {B: [] for B in batches}
    b = {B: [] for B in batches}
    sh = {B: [] for B in batches}
    for _ in range(args.repeats):
        for B in batches:
            a[B].append(serial_rate(ge, eng, prompt, params, B))
            b[B].append(batch_rate(ge, eng, prompt, params, B))
            if args.share_trunk:
                sh[B].append(batch_rate(ge, eng, prompt, params, B, True))
    for B in batches:
        ra, rb = statistics.median(a[B]), statistics.median(b[B])
        model = B * (W + K) / (W + B * K)
        result["rows"][str(B)] = {"serial_tok_s": round(ra, 1), "batch_tok_s": round(rb, 1), "batch_over_serial": round(rb / ra, 3),
                                  "byte_model_ratio": round(model, 3), "fraction_of_byte_model": round(rb / ra / model, 3)}
        if args.share_trunk:
            rs = statistics.median(sh[B])
            model_s = B * (W + K) / (W + Kt + B * (K - Kt)) if B > 1 else 1.0
            result["rows"][str(B)].update({"shared_tok_s": round(rs, 1), "shared_over_serial": round(rs / ra, 3),
                                           "shared_over_unshared": round(rs / rb, 3), "trunk_byte_model_ratio": round(model_s, 3)})
    if args.share_trunk:
        result["trunk_bytes"] = Kt
    if "8" in result["rows"]:
        result["bar_met_at_B8"] = result["rows"]["8"]["fraction_of_byte_model"] >= 0.5
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
