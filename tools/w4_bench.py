"""MXFP4 decoder weights against fp16 and int8, same process, same box: 7b shape (random init), the persona prompt bench.py
times.  Four models, built one after another and measured INTERLEAVED (repetition r of every leg before repetition r + 1 of any, the order rotating by one leg per repetition):

    (a) fp16                 weight_format="fp16"
    (b) mxfp4                weight_format="mxfp4": the <= 16-row projections stream the 4-bit images (pc_gemm_w4)
    (c) mxfp4_fp16_images    the same weights W' with PC_W4_STREAM=0: the parent's kernels on the fp16 images of W'
    (d) int8_weight_only     load_in_8bit with PC_INT8_WEIGHT_ONLY=1

Per leg: TTFT (CacheEngine.process + the first forward, 12 new rows over the staged modules) and its two parts, the GreedyLoop
rate (generate, greedy; first Output to last, host clock) and the one-row decode step on the device's clock (--new GreedyLoop
replays between two events), the SlotLoop rate at 4 / 8 / 16 slots (generate_batch; tokens summed over the
sequences, prefills excluded; null where the model has no batched loop), resident weight bytes.  Medians of --repeats
repetitions with the spread (min, max, and (max - min) / median).  The condition the mode is held to: (b) faster than (c) by
more than (c)'s own spread on the 12-row cached step and on the one-row decode step.  Also max |dlogit| of the first forward's
last row between the legs ((a)-(b): the format's accuracy on this model; (b)-(c): the same weights on two kernels).

    python tools/w4_bench.py [--repeats 20] [--new 48] [--out profiles/w4_bench.json]
    python tools/w4_bench.py --only mxfp4       # leg (b)'s step alone: the run to put under rocprofv3 --kernel-trace --stats

``--rows``: the 17..64-row steps, legs (b) with PC_W4_MAX_ROWS=64 (pc_gemm_w4_rows) and (c), interleaved in the same
rotating order: the cached step at 17 / 32 / 48 / 64 new rows (HIP events around the forward) and the LookupSlotLoop step at 8 slots
with k = 3 and k = 7 (32 and 64 rows; an empty corpus, HIP events around one replay).  The default of PC_W4_MAX_ROWS the numbers
imply: the largest of {16, 32, 48, 64} such that at it and at every smaller measured row count (b)'s median beats (c)'s by more
than (c)'s own (max - min) / median.

    python tools/w4_bench.py --rows [--repeats 10] [--out profiles/w4_rows_bench.json]
    python tools/w4_bench.py --rows --only mxfp4     # leg (b)'s steps alone, for rocprofv3 --kernel-trace --stats

``--resident``: keep_fp16=False against keep_fp16=True, two MXFP4 models in one process, the order of the two
alternating between repetitions, every time from HIP events, median [min .. max]: resident bytes of both legs; pc_w4_expand alone
on the four 7b projections in both layouts (us, read + written bytes/s) with kv_copy_kernel's rate from the same run next to it;
the cached step at 12 / 40 / 64 rows and the one-row decode step (the dropped leg launches nothing new there: its median has to lie
inside the kept leg's min .. max); the cached step at 130 / 258 rows, the no-cache persona prefill and the persona schema encode
(the price of the mode, as a ratio to the kept leg).

    python tools/w4_bench.py --resident [--repeats 10] [--out profiles/w4_resident_bench.json]
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

LEGS = {
    "fp16": (dict(weight_format="fp16"), {}),
    "mxfp4": (dict(weight_format="mxfp4"), {"PC_W4_STREAM": "1"}),
    "mxfp4_fp16_images": (dict(weight_format="mxfp4"), {"PC_W4_STREAM": "0"}),
    "int8_weight_only": (dict(weight_format="fp16", load_in_8bit=True), {"PC_INT8_WEIGHT_ONLY": "1"}),
    "mxfp4_keep_fp16": (dict(weight_format="mxfp4", keep_fp16=True), {"PC_W4_STREAM": "1"}),          # --resident
    "mxfp4_drop_fp16": (dict(weight_format="mxfp4", keep_fp16=False), {"PC_W4_STREAM": "1"}),
}
RESIDENT_SMALL, RESIDENT_LARGE = (12, 40, 64), (130, 258)
SLOTS = (4, 8, 16)
ROW_COUNTS = (17, 32, 48, 64)
LOOKUP_CASES = ((8, 3), (8, 7))


def weight_bytes(m) -> int:
    """Bytes of every tensor the model keeps resident for its weights (each storage once)."""
    seen, total = set(), 0
    tensors = [m.embed, m.norm, m.lm_head, m.lm_head_f] + [v for lw in m.layers for v in lw.values()]
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.untyped_storage().data_ptr() not in seen:
            seen.add(t.untyped_storage().data_ptr())
            total += t.untyped_storage().nbytes()
    return total


class Leg:
    def __init__(self, name, extra_env=None):
        kw, env = LEGS[name]
        env = dict(env, **(extra_env or {}))
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0, **kw)
            self.resident_bytes = self.lm.hf_model.resident_bytes()        # (before any forward leaves a workspace behind)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        self.name = name
        self.eng = CacheEngine(4096, self.lm, slots=max(SLOTS))
        fmt = self.lm.get_formatter()
        sp, pp = synth.persona_like()
        self.schema_text = fmt(sp)
        self.eng.add_schema(self.schema_text)
        self.prompt = Prompt(pp, [fmt])
        self.ge = GenerationEngine(self.lm)

    def ttft(self):
        """(process ms, first forward ms, last-row logits)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, pos, _, cache = self.eng.process(self.prompt)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = self.lm(input_ids=torch.tensor([ids], device="cuda:0"), position_ids=torch.tensor([pos], device="cuda:0"),
                      past_key_values=cache, use_cache=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return 1e3 * (t1 - t0), 1e3 * (t2 - t1), out.logits[0, -1].float().clone(), len(ids)

    def greedy_rate(self, params):
        ids, pos, _, cache = self.eng.process(self.prompt)
        t0 = None
        for _out in self.ge.generate(ids, pos, params, cache, stream_interval=10 ** 9):
            if t0 is None:
                t0 = time.perf_counter()
        torch.cuda.synchronize()
        return (params.max_new_tokens - 1) / (time.perf_counter() - t0)

    def decode_step_ms(self, n):
        """One-row decode step on the device's clock: n GreedyLoop replays behind the cached prefill, first replay's start event
        to the last one's end event (None where the model has no device loop)."""
        m = self.lm.hf_model
        ids, pos, _, cache = self.eng.process(self.prompt)
        out = self.lm(input_ids=torch.tensor([ids], device="cuda:0"), position_ids=torch.tensor([pos], device="cuda:0"),
                      past_key_values=cache, use_cache=True)
        past = out.past_key_values
        if not m.can_loop(past):
            return None
        g = m.greedy_loop(past, int(torch.argmax(out.logits[0, -1])), max(pos) + 2, n)
        if g is None:
            return None
        for _ in range(n):
            g.enqueue()
        torch.cuda.synchronize()
        ms = g.events[0][0].elapsed_time(g.events[-1][1]) / n
        g.close(n)
        return ms

    def slot_rate(self, params, B):
        if not self.ge.batch_plan(B, params)[0]:
            return None
        reqs = [self.eng.process(self.prompt, slot=k) for k in range(B)]
        firsts, t0 = 0, None
        for _k, _out in self.ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, stream_interval=10 ** 9):
            firsts += 1
            if firsts == B:
                t0 = time.perf_counter()
        torch.cuda.synchronize()
        return B * (params.max_new_tokens - 1) / (time.perf_counter() - t0)


    # ---- the 17..64-row steps (--rows) ----
    def question(self, rows):
        """The persona prompt with a question that gives exactly ``rows`` new rows over the staged modules."""
        fmt = self.lm.get_formatter()
        for qlen in range(1, 2 * rows):
            _, pp = synth.persona_like(question_len=qlen)
            prompt = Prompt(pp, [fmt])
            if len(self.eng.process(prompt)[0]) == rows:
                return prompt
        raise RuntimeError(f"no question length gives {rows} new rows")

    def step_ms(self, prompt):
        """The cached step between two HIP events (process excluded) -> (ms, last-row logits)."""
        ids, pos, _, cache = self.eng.process(prompt)
        ii, pp = torch.tensor([ids], device="cuda:0"), torch.tensor([pos], device="cuda:0")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = self.lm(input_ids=ii, position_ids=pp, past_key_values=cache, use_cache=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out.logits[0, -1].float().clone()

    def lookup_step_ms(self, S, k, n_new):
        """Median ms of one LookupSlotLoop replay at S slots (S * (k + 1) rows), an empty corpus: every step verifies k drafts
        per slot only where the output repeats itself."""
        pasts, firsts, p0s = [], [], []
        for j in range(S):
            ids, pos, _, cache = self.eng.process(self.prompt, slot=j)
            out = self.lm(input_ids=torch.tensor([ids]), position_ids=torch.tensor([pos]), past_key_values=cache, use_cache=True)
            pasts.append(out.past_key_values)
            firsts.append(int(out.logits[0, -1].argmax()))
            p0s.append(max(pos) + 2)
        loop = self.lm.hf_model.lookup_slot_loop(pasts, firsts, p0s, n_new, k, [[]] * S)
        assert loop is not None
        got, i = [0] * S, 0
        while min(got) < n_new:
            if loop.n <= i:
                loop.enqueue()
            for j in range(S):
                got[j] += len(loop.tokens(j, i))
            i += 1
        ms = [loop.elapsed_ms(j) for j in range(i)]
        loop.close([n_new] * S)
        return statistics.median(ms)


    # ---- keep_fp16=False against keep_fp16=True (--resident) ----
    def nocache_ms(self):
        """The persona prompt without the cache, between two HIP events -> (ms, rows)."""
        ids, pos, _, cache = self.eng.process(self.prompt, no_cache=True)
        ii, pp = torch.tensor([ids], device="cuda:0"), torch.tensor([pos], device="cuda:0")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.lm(input_ids=ii, position_ids=pp, past_key_values=cache, use_cache=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), len(ids)

    def encode_tok_s(self):
        """The persona schema encoded again (its module KV dropped first): module tokens stored per second between two HIP events."""
        name = next(iter(self.eng.schemas))
        self.eng.remove_schema(name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.eng.add_schema(self.schema_text)
        e1.record()
        torch.cuda.synchronize()
        toks = sum(len(c) for c in self.eng.schemas[name].cache_l1.values())
        return toks / (1e-3 * e0.elapsed_time(e1))


def _events_us(fn, inner):
    """``inner`` back-to-back launches of ``fn`` between two HIP events -> us per launch."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / inner


def expand_micro(m, repeats, inner=10):
    """pc_w4_expand alone on layer 0's four projections, both layouts, and kv_copy_kernel (pc_kv_gather of one 512-row segment
    of the 7b geometry: 268 MB read, 268 MB written) in the same rotation."""
    from promptcache_amd import _native as n
    lw = m.layers[0]
    cases = {}
    for key in ("wqkv", "wo", "wgu", "wdown"):
        ci, si = lw[key + "_c4"], lw[key + "_e4"]
        N, K = 16 * ci.shape[0], 128 * ci.shape[1]
        nbytes = N * K // 2 + N * K // 32 + 2 * N * K
        out = m._w16_scratch
        perm = m._qkv_perm_i32 if key == "wqkv" else None
        cases[f"{key}_{N}x{K}_frag"] = (nbytes, lambda ci=ci, si=si, N=N, K=K, perm=perm: n.w4_expand(ci, si, out, N, K, n.W4_EXPAND_FRAG, row_perm=perm))
        cases[f"{key}_{N}x{K}_rowmajor"] = (nbytes, lambda ci=ci, si=si, N=N, K=K: n.w4_expand(ci, si, out, N, K, n.W4_EXPAND_ROWMAJOR, ld_out=K))
    L, Hkv, D, rows = m.L, m.Hkv, m.D, 512
    src = torch.randn((L, 2, Hkv, rows, D), device="cuda:0").half()
    dst = torch.empty((L, 2, Hkv, rows, D), dtype=torch.float16, device="cuda:0")
    cases["kv_copy_kernel"] = (2 * src.numel() * 2, lambda: n.kv_gather([src.data_ptr()], [rows], [0], dst, L, Hkv, D, rows))
    rec = {k: [] for k in cases}
    for k, (_, fn) in cases.items():
        _events_us(fn, 3)
    names = list(cases)
    for rep in range(repeats):
        for k in names[rep % len(names):] + names[:rep % len(names)]:
            rec[k].append(_events_us(cases[k][1], inner))
    res = {}
    for k, v in rec.items():
        sm = summary(v)
        sm["bytes"] = cases[k][0]
        sm["GB_s"] = {"at_" + q: round(cases[k][0] / (1e-6 * sm[q]) / 1e9, 1) for q in ("median", "min", "max")}   # (of the TIME)
        res[k] = sm
    return res


def resident_mode(args):
    legs = []
    names = ("mxfp4_keep_fp16", "mxfp4_drop_fp16")
    for name in (names[::-1] if args.drop_first else names):       # (--drop-first: the models allocated in the other order)
        legs.append(Leg(name, {"PC_W4_MAX_ROWS": "64"}))
        print(f"[w4_bench] {name}: {legs[-1].resident_bytes / 1e9:.2f} GB resident", file=sys.stderr, flush=True)
    legs.sort(key=lambda leg: names.index(leg.name))
    prompts = {leg.name: {r: leg.question(r) for r in RESIDENT_SMALL + RESIDENT_LARGE} for leg in legs}
    keys = [f"step{r}_ms" for r in RESIDENT_SMALL + RESIDENT_LARGE] + ["decode_step_ms", "nocache_prefill_ms", "encode_tok_s"]
    info = {}

    def once(leg, r):
        for rows in RESIDENT_SMALL + RESIDENT_LARGE:
            ms, lg = leg.step_ms(prompts[leg.name][rows])
            info[(leg.name, rows)] = lg
            if r is not None:
                r[f"step{rows}_ms"].append(ms)
        dm = leg.decode_step_ms(args.new)
        ms, info["nocache_rows"] = leg.nocache_ms()
        ts = leg.encode_tok_s()
        if r is not None:
            r["decode_step_ms"].append(dm); r["nocache_prefill_ms"].append(ms); r["encode_tok_s"].append(ts)
    for leg in legs:                                   # warm: graphs captured, code objects loaded
        for _ in range(2):
            once(leg, None)
    rec = {leg.name: {k: [] for k in keys} for leg in legs}
    for rep in range(args.repeats):
        for leg in (legs if rep % 2 == 0 else legs[::-1]):
            once(leg, rec[leg.name])
        print(f"[w4_bench] repetition {rep + 1} / {args.repeats}", file=sys.stderr, flush=True)
    kept, drop = legs
    result = {"shape": "llama2-7b (random init)",
              "prompt": "persona schema; cached steps of %s new rows; no-cache prefill of %d rows" % (list(RESIDENT_SMALL + RESIDENT_LARGE), info["nocache_rows"]),
              "built_first": "mxfp4_drop_fp16" if args.drop_first else "mxfp4_keep_fp16",
              "how": f"{args.repeats} repetitions, the order of the two legs alternating; HIP events around every timed region; median, min, "
                     "max, spread = (max - min) / median; PC_W4_MAX_ROWS=64 in both legs; encode_tok_s = module tokens stored / time of add_schema",
              "legs": {leg.name: dict({k: summary(v, 1 if k.endswith("tok_s") else 3) for k, v in rec[leg.name].items()},
                                      resident_bytes=leg.resident_bytes, weight_bytes=weight_bytes(leg.lm.hf_model)) for leg in legs},
              "pc_w4_expand": expand_micro(drop.lm.hf_model, args.repeats)}
    a, b = result["legs"][kept.name], result["legs"][drop.name]
    result["resident_bytes_ratio_drop_over_keep"] = round(drop.resident_bytes / kept.resident_bytes, 4)
    result["bit_equal_last_row_logits"] = {str(r): bool(torch.equal(info[(kept.name, r)], info[(drop.name, r)])) for r in RESIDENT_SMALL + RESIDENT_LARGE}
    result["no_new_launch_steps_drop_median_inside_keep_min_max"] = {
        k: {"drop_median": b[k]["median"], "keep_min": a[k]["min"], "keep_max": a[k]["max"],
            "inside": bool(a[k]["min"] <= b[k]["median"] <= a[k]["max"])}
        for k in [f"step{r}_ms" for r in RESIDENT_SMALL] + ["decode_step_ms"]}
    result["cost_ratio_drop_over_keep"] = {k: round(b[k]["median"] / a[k]["median"], 4)
                                           for k in [f"step{r}_ms" for r in RESIDENT_LARGE] + ["nocache_prefill_ms", "encode_tok_s"]}
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


def rows_mode(args):
    names = [args.only] if args.only else ["mxfp4", "mxfp4_fp16_images"]
    legs = [Leg(n, {"PC_W4_MAX_ROWS": "64"}) for n in names]
    n_new = min(args.new, 24)
    prompts = {leg.name: {r: leg.question(r) for r in ROW_COUNTS} for leg in legs}
    keys = [f"step{r}_ms" for r in ROW_COUNTS] + [f"lookup_S{S}_k{k}_step_ms" for S, k in LOOKUP_CASES]

    def once(leg, r, logits):
        for rows in ROW_COUNTS:
            ms, lg = leg.step_ms(prompts[leg.name][rows])
            logits[(leg.name, rows)] = lg
            if r is not None:
                r[f"step{rows}_ms"].append(ms)
        for S, k in LOOKUP_CASES:
            ms = leg.lookup_step_ms(S, k, n_new)
            if r is not None:
                r[f"lookup_S{S}_k{k}_step_ms"].append(ms)
    logits = {}
    for leg in legs:                                   # warm: graphs captured, code objects loaded
        for _ in range(2):
            once(leg, None, logits)
    repeats = 3 if args.only else args.repeats
    rec = {leg.name: {k: [] for k in keys} for leg in legs}
    for rep in range(repeats):
        for leg in legs[rep % len(legs):] + legs[:rep % len(legs)]:
            once(leg, rec[leg.name], logits)
    result = {"shape": "llama2-7b (random init)", "prompt": "persona schema, questions of %s new rows; slot lookup at %s (slots, k), empty corpus"
              % (list(ROW_COUNTS), list(LOOKUP_CASES)),
              "how": f"{repeats} interleaved repetitions, leg order rotating; HIP events around the forward / one replay; median, min, "
                     "max, spread = (max - min) / median; PC_W4_MAX_ROWS=64 in both legs",
              "legs": {leg.name: {k: summary(v) for k, v in rec[leg.name].items()} for leg in legs}}
    if len(legs) == 2:
        b, c = result["legs"]["mxfp4"], result["legs"]["mxfp4_fp16_images"]
        cond = {}
        for key in keys:
            gain = (c[key]["median"] - b[key]["median"]) / c[key]["median"]
            cond[key] = {"b_median": b[key]["median"], "c_median": c[key]["median"], "gain": round(gain, 4),
                         "c_spread": c[key]["spread"], "met": bool(gain > c[key]["spread"])}
        result["condition_b_faster_than_c_by_more_than_c_spread"] = cond
        rows_of = {f"step{r}_ms": r for r in ROW_COUNTS}
        rows_of.update({f"lookup_S{S}_k{k}_step_ms": S * (k + 1) for S, k in LOOKUP_CASES})
        default = 16
        for cand in (32, 48, 64):
            if all(cond[key]["met"] for key, r in rows_of.items() if r <= cand):
                default = cand
            else:
                break
        result["implied_default_PC_W4_MAX_ROWS"] = default
        result["max_dlogit_b_vs_c"] = {str(r): float((logits[("mxfp4", r)] - logits[("mxfp4_fp16_images", r)]).abs().max()) for r in ROW_COUNTS}
    line = json.dumps(result)
    if args.out and not args.only:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


def summary(vals, nd=3):
    vals = [v for v in vals if v is not None]
    if not vals:
        return None
    med = statistics.median(vals)
    return {"median": round(med, nd), "min": round(min(vals), nd), "max": round(max(vals), nd),
            "spread": round((max(vals) - min(vals)) / med, 4), "n": len(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--new", type=int, default=48, help="greedy tokens per sequence")
    ap.add_argument("--legs", default=",".join(list(LEGS)[:4]))
    ap.add_argument("--only", default=None, help="one leg's cached step and decode loop alone (warm + 3 repetitions), no JSON file")
    ap.add_argument("--rows", action="store_true", help="the 17..64-row steps: legs (b) and (c) with PC_W4_MAX_ROWS=64")
    ap.add_argument("--resident", action="store_true", help="keep_fp16=False against keep_fp16=True (DESIGN 3.26)")
    ap.add_argument("--drop-first", action="store_true", help="--resident: build the keep_fp16=False model first")
    ap.add_argument("--out", default=None, help="default profiles/w4_bench.json (--rows: profiles/w4_rows_bench.json, "
                                                "--resident: profiles/w4_resident_bench.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "w4_resident_bench.json" if args.resident else
                                "w4_rows_bench.json" if args.rows else "w4_bench.json")
    assert torch.cuda.is_available(), "w4_bench measures on the GPU"
    if args.resident:
        return resident_mode(args)
    if args.rows:
        return rows_mode(args)
    params = GenerationParameters(temperature=0.0, max_new_tokens=args.new, stop_token_ids=[], stop_str=[])
    if args.only:
        leg = Leg(args.only)
        for _ in range(4):
            leg.ttft()
            leg.greedy_rate(params)
        print(json.dumps({"leg": args.only, "first_forward_ms": round(leg.ttft()[1], 3), "greedy_tok_s": round(leg.greedy_rate(params), 1)}))
        return
    legs = [Leg(n) for n in args.legs.split(",")]
    for leg in legs:                                   # warm: graphs captured, code objects loaded
        for _ in range(3):
            leg.ttft()
        leg.greedy_rate(params)
        leg.decode_step_ms(args.new)
        for B in SLOTS:
            leg.slot_rate(params, B)
    rec = {leg.name: {"process_ms": [], "first_forward_ms": [], "ttft_ms": [], "greedy_tok_s": [], "decode_step_ms": [],
                      **{f"slot{B}_tok_s": [] for B in SLOTS}} for leg in legs}
    logits, rows = {}, None
    for rep in range(args.repeats):
        for leg in legs[rep % len(legs):] + legs[:rep % len(legs)]:     # (the order rotates: no leg always runs behind the same one)
            r = rec[leg.name]
            p, f, lg, rows = leg.ttft()
            r["process_ms"].append(p); r["first_forward_ms"].append(f); r["ttft_ms"].append(p + f)
            logits[leg.name] = lg
            r["greedy_tok_s"].append(leg.greedy_rate(params))
            r["decode_step_ms"].append(leg.decode_step_ms(args.new))
            for B in SLOTS:
                r[f"slot{B}_tok_s"].append(leg.slot_rate(params, B))
    result = {"shape": "llama2-7b (random init)", "prompt": f"persona schema, {rows} new rows over the staged modules",
              "new_tokens": args.new, "how": f"{args.repeats} interleaved repetitions, leg order rotating; median, min, max, spread = (max - min) / median",
              "legs": {}}
    for leg in legs:
        row = {k: summary(v, 1 if k.endswith("tok_s") else 3) for k, v in rec[leg.name].items()}
        row["weight_bytes"] = weight_bytes(leg.lm.hf_model)
        result["legs"][leg.name] = row

    def dl(a, b):
        return None if a not in logits or b not in logits else float((logits[a] - logits[b]).abs().max())
    result["max_dlogit"] = {"fp16_vs_mxfp4": dl("fp16", "mxfp4"), "mxfp4_vs_mxfp4_fp16_images": dl("mxfp4", "mxfp4_fp16_images")}
    if "mxfp4" in result["legs"] and "mxfp4_fp16_images" in result["legs"]:
        b, c = result["legs"]["mxfp4"], result["legs"]["mxfp4_fp16_images"]
        cond = {}
        for key in ("first_forward_ms", "decode_step_ms"):
            if b[key] is None or c[key] is None:
                continue
            gain = (c[key]["median"] - b[key]["median"]) / c[key]["median"]
            cond[key] = {"b_median": b[key]["median"], "c_median": c[key]["median"], "gain": round(gain, 4),
                         "c_spread": c[key]["spread"], "met": bool(gain > c[key]["spread"])}
        result["condition_b_faster_than_c_by_more_than_c_spread"] = cond
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
