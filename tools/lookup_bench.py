"""Prompt-lookup speculative decoding against the plain greedy loop at the 7b shape (random init, the persona prompt): tok/s of
``GreedyLoop`` and of ``LookupLoop`` at k in {3, 7, 15} with a full-acceptance corpus (the context tail followed by the answer
itself: every draft is right) and with an empty one (the worst case: every step pays k + 1 rows for one token, unless the output
repeats itself), and the per-step time of the k + 1-row step against the one-row step.  Same process, interleaved repetitions,
medians.  Prints one JSON line.

    python tools/lookup_bench.py [--new 64] [--repeats 5] [--out profiles/lookup_bench.json]

``--sampled``: the same comparison for sampled generations -- ``SampleLoop`` against ``SampleLookupLoop`` at k in {3, 7}, with the
corpus set to the ``SampleLoop`` leg's own output for that seed (every draft is right) and with nothing to copy, at the demo's
parameters (T = 1, top_p = 0.95) and at T = 0.7, rp = 1.1, top_p = 0.9, top_k = 40; every leg reports whether it emitted the
``SampleLoop`` leg's tokens.

    python tools/lookup_bench.py --sampled [--new 64] [--repeats 5] [--out profiles/lookup_sample_bench.json]
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
from promptcache_amd import CacheEngine, GenerationParameters, Prompt, synth  # noqa: E402
from promptcache_amd.model import Llama2  # noqa: E402

KS = (3, 7, 15)


def prefill(lm, eng, prompt):
    ids, pos, _, cache = eng.process(prompt)
    out = lm(input_ids=torch.tensor([ids]), position_ids=torch.tensor([pos]), past_key_values=cache, use_cache=True)
    return ids, out.past_key_values, int(out.logits[0, -1].argmax()), max(pos) + 2


def run_greedy(lm, eng, prompt, n_new):
    """-> (tokens, seconds from the first enqueue to the last token on the host, per-step ms)."""
    _, past, first, p0 = prefill(lm, eng, prompt)
    loop = lm.hf_model.greedy_loop(past, first, p0, n_new)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.enqueue()
    toks = []
    for i in range(n_new):
        if loop.n <= i + 1 and loop.n < n_new:
            loop.enqueue()
        toks.append(loop.token(i))
    dt = time.perf_counter() - t0
    ms = [loop.elapsed_ms(i) for i in range(n_new)]
    loop.close(n_new)
    return first, toks, dt, ms


def run_lookup(lm, eng, prompt, n_new, k, corpus):
    _, past, first, p0 = prefill(lm, eng, prompt)
    loop = lm.hf_model.lookup_loop(past, first, p0, n_new, k, corpus)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks, i = [], 0
    while len(toks) < n_new:
        if loop.n <= i:
            loop.enqueue()
        if loop.n == i + 1 and len(toks) + k + 1 < n_new:
            loop.enqueue()                       # one replay ahead while the step in flight cannot exhaust the budget
        toks += loop.tokens(i)
        i += 1
    dt = time.perf_counter() - t0
    ms = [loop.elapsed_ms(j) for j in range(i)]
    loop.close(n_new)
    return toks, dt, ms, i


SAMPLED_KS = (3, 7)
SAMPLED_PARAMS = {"demo_T1_p0.95": dict(temperature=1.0, top_p=0.95),
                  "T0.7_rp1.1_p0.9_k40": dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40)}
SEED = 1234


def prefill_sampled(lm, eng, prompt, params):
    """-> (prompt ids, past, first token: drawn from the prefill's last row at step 0 as generate() draws it, its position)."""
    ids, pos, _, cache = eng.process(prompt)
    out = lm(input_ids=torch.tensor([ids]), position_ids=torch.tensor([pos]), past_key_values=cache, use_cache=True)
    first = lm.hf_model.sample_token(out.logits[0, -1], params, SEED, ids)
    return list(ids), out.past_key_values, first, max(pos) + 2


def run_sample(lm, eng, prompt, n_new, params):
    ids, past, first, p0 = prefill_sampled(lm, eng, prompt, params)
    loop = lm.hf_model.sample_loop(past, first, p0, n_new + 1, params, SEED, ids + [first])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.enqueue()
    toks = []
    for i in range(n_new):
        if loop.n <= i + 1 and loop.n < n_new:
            loop.enqueue()
        toks.append(loop.token(i))
    dt = time.perf_counter() - t0
    ms = [loop.elapsed_ms(i) for i in range(n_new)]
    loop.close(n_new)
    return first, toks, dt, ms


def run_sample_lookup(lm, eng, prompt, n_new, params, k, corpus):
    ids, past, first, p0 = prefill_sampled(lm, eng, prompt, params)
    loop = lm.hf_model.lookup_loop(past, first, p0, n_new, k, corpus, params=params, seed=SEED, history_ids=ids + [first])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks, i = [], 0
    while len(toks) < n_new:
        if loop.n <= i:
            loop.enqueue()
        if loop.n == i + 1 and len(toks) + k + 1 < n_new:
            loop.enqueue()                       # one replay ahead while the step in flight cannot exhaust the budget
        toks += loop.tokens(i)
        i += 1
    dt = time.perf_counter() - t0
    ms = [loop.elapsed_ms(j) for j in range(i)]
    loop.close(n_new)
    return first, toks, dt, ms, i


def main_sampled(args, lm, eng, prompt):
    N = args.new
    ctx_ids, _, _, _ = prefill(lm, eng, prompt)
    legs = []
    for pname, kw in SAMPLED_PARAMS.items():
        params = GenerationParameters(max_new_tokens=N + 1, stop_token_ids=[], stop_str=[], **kw)
        first, T, _, _ = run_sample(lm, eng, prompt, N, params)        # warm + the answer the full-acceptance corpus copies
        full = list(ctx_ids)[-8:] + [first] + T
        legs.append((f"{pname}/sample", params, None, None, (first, T)))
        for k in SAMPLED_KS:
            for cname, c in (("full", full), ("empty", [])):
                legs.append((f"{pname}/lookup_k{k}_{cname}", params, k, c, (first, T)))
                run_sample_lookup(lm, eng, prompt, N, params, k, c)  # warm: graphs captured
    rate = {leg[0]: [] for leg in legs}
    step_ms = {leg[0]: [] for leg in legs}
    steps, same = {}, {}
    for _ in range(args.repeats):
        for name, params, k, c, (first, T) in legs:
            if k is None:
                f, toks, dt, ms = run_sample(lm, eng, prompt, N, params)
                steps[name] = N
            else:
                f, toks, dt, ms, steps[name] = run_sample_lookup(lm, eng, prompt, N, params, k, c)
            same[name] = same.get(name, True) and f == first and toks[:N] == T
            rate[name].append(N / dt)
            step_ms[name].append(statistics.median(ms))
    result = {"shape": "llama2-7b (random init)", "prompt": "persona-structured schema, the decode leg's prompt", "new_tokens": N,
              "seed": SEED, "params": SAMPLED_PARAMS,
              "how": "same process, legs interleaved, %d repetitions, medians; wall clock from the first enqueue to the last token "
                     "on the host; step_ms: HIP events around one replay; full: the corpus is the sample leg's own output, empty: "
                     "nothing to copy but the output itself" % args.repeats,
              "tokens_per_s": {n: round(statistics.median(v), 1) for n, v in rate.items()},
              "tokens_per_s_min_max": {n: [round(min(v), 1), round(max(v), 1)] for n, v in rate.items()},
              "step_ms": {n: round(statistics.median(v), 4) for n, v in step_ms.items()},
              "steps": steps, "tokens_equal_sample_loop": same}
    result["speedup_over_sample_loop"] = {n: round(v / result["tokens_per_s"][n.split("/")[0] + "/sample"], 3)
                                          for n, v in result["tokens_per_s"].items() if not n.endswith("/sample")}
    result["all_legs_equal_sample_loop"] = all(same.values())
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64, help="tokens per generation (behind the first)")
    ap.add_argument("--repeats", type=int, default=5, help="interleaved repetitions per leg (medians)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sampled", action="store_true", help="SampleLoop against SampleLookupLoop instead (see above)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lookup_bench measures on the GPU"
    lm = Llama2("llama2-7b", device="cuda:0", random_init=True, seed=0)
    assert lm.hf_model.lookup_available()
    eng = CacheEngine(4096, lm)
    fmt = lm.get_formatter()
    sp, pp = synth.persona_like()
    eng.add_schema(fmt(sp))
    prompt = Prompt(pp, [fmt])
    if args.sampled:
        line = json.dumps(main_sampled(args, lm, eng, prompt))
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    N = args.new
    ctx_ids, _, _, _ = prefill(lm, eng, prompt)
    first, T, _, _ = run_greedy(lm, eng, prompt, N)                  # warm + the answer the full-acceptance corpus copies
    full = list(ctx_ids)[-8:] + [first] + T
    legs = [("greedy", None, None)] + [(f"lookup_k{k}_{name}", k, c) for k in KS for name, c in (("full", full), ("empty", []))]
    for name, k, c in legs[1:]:
        run_lookup(lm, eng, prompt, N, k, c)                         # warm: graphs captured
    rate = {name: [] for name, _, _ in legs}
    step_ms = {name: [] for name, _, _ in legs}
    steps, same = {}, {}
    for _ in range(args.repeats):
        for name, k, c in legs:
            if k is None:
                _, toks, dt, ms = run_greedy(lm, eng, prompt, N)
                steps[name] = N
            else:
                toks, dt, ms, n_steps = run_lookup(lm, eng, prompt, N, k, c)
                steps[name] = n_steps
            same[name] = toks[:N] == T
            rate[name].append(N / dt)
            step_ms[name].append(statistics.median(ms))
    result = {"shape": "llama2-7b (random init)", "prompt": "persona-structured schema, the decode leg's prompt", "new_tokens": N,
              "how": "same process, legs interleaved, %d repetitions, medians; wall clock from the first enqueue to the last token "
                     "on the host; step_ms: HIP events around one replay" % args.repeats,
              "tokens_per_s": {n: round(statistics.median(v), 1) for n, v in rate.items()},
              "tokens_per_s_min_max": {n: [round(min(v), 1), round(max(v), 1)] for n, v in rate.items()},
              "step_ms": {n: round(statistics.median(v), 4) for n, v in step_ms.items()},
              "steps": steps, "tokens_equal_greedy": same}
    g = result["tokens_per_s"]["greedy"]
    result["speedup_over_greedy"] = {n: round(v / g, 3) for n, v in result["tokens_per_s"].items() if n != "greedy"}
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
