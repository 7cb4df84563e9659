"""Counterpart of the reference's ``demo.py`` (:23-103) on the MI355X path: same call order --
model adapter -> ``CacheEngine(max_ctx, lm)`` -> ``add_schema(read_file(xml, [formatter]), max_tokens)`` -> ``Prompt`` ->
``process`` (with the adapter's ``use_full_position_ids``) -> ``GenerationEngine.generate`` -- run once with the prompt
cache and once with ``no_cache=True``, printing the two timed intervals of each (gather, first forward).

    python demo.py                                   # llama2-7b shape, random weights, synthetic game-like schema
    python demo.py --model falcon --schema my.xml --prompt-file my_prompt.xml
    python demo.py --model /path/to/hf/checkpoint    # real weights + tokenizer when a directory is available

There is no network on the build / bench machines, so without a checkpoint directory the adapters use seeded random
weights at the named shape and the deterministic stand-in tokenizer: the text is noise, the timings are real.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "prompt-cache_amd"))

from promptcache_amd import CacheEngine, GenerationEngine, GenerationParameters, Prompt, read_file, synth  # noqa: E402
from promptcache_amd.model import CodeLlama, Falcon, Llama2, Mpt  # noqa: E402

ADAPTERS = {"llama": (Llama2, "llama2-7b"), "codellama": (CodeLlama, "codellama-7b"), "falcon": (Falcon, "falcon-7b"),
            "mpt": (Mpt, "mpt-7b")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama", help="llama | codellama | falcon | mpt | <HF checkpoint directory>")
    ap.add_argument("--schema", help="PML schema file (default: a synthetic game-like schema, 7 modules)")
    ap.add_argument("--prompt-file", help="PML prompt file referencing the schema")
    ap.add_argument("--max-ctx", type=int, default=5000)
    ap.add_argument("--max-tokens", type=int, default=800)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--module-kv", choices=("fp16", "int8"), default=None,
                    help="module KV store format (default: PC_MODULE_KV, else fp16); int8 = 0.516 of the fp16 bytes")
    ap.add_argument("--batch", type=int, default=0,
                    help="also decode N copies of the prompt with different questions together (generate_batch; N <= 16)")
    ap.add_argument("--share-trunk", action="store_true",
                    help="with --batch: read the module rows the N prompts have in common once per step for all of them "
                         "(with --lookup K as well: once for all K + 1 draft rows of all of them); with --serve N --slot-kv int8: "
                         "the serving loop reads a group's shared rows once per step from the leader's int8 image "
                         "(serve(slot_kv='int8', share_trunk=True)); not with --lookup or --slot-drop-fp16 there")
    ap.add_argument("--slot-kv", choices=("fp16", "int8"), default=None,
                    help="with --batch / --serve: what the batched loop's attention reads (default: PC_SLOT_KV, else fp16); int8 = "
                         "int8 images of the slots' K/V rows, about half the bytes per step, the format's accuracy, and 0.516 of a "
                         "slot buffer MORE memory per slot (the fp16 buffers stay); with --share-trunk under --serve only; with --lookup K under "
                         "--serve only (serve(lookup=K, slot_kv='int8'): the K + 1 row step reads the images), not under --batch alone")
    ap.add_argument("--slot-drop-fp16", action="store_true",
                    help="with --serve and --slot-kv int8: no slot keeps an fp16 buffer (keep_arenas=False; default: "
                         "PC_SLOT_KEEP_ARENAS): every prompt is prefilled in one shared buffer and lives on as its int8 image")
    ap.add_argument("--serve", type=int, default=0,
                    help="serve N prompts with mixed max_new_tokens through --batch slots (continuous batching: a finished "
                         "sequence's slot takes the next prompt while the others keep decoding)")
    ap.add_argument("--lookup", type=int, default=None,
                    help="prompt-lookup speculative decoding for the greedy single-prompt generation: draft up to K tokens (1..15; "
                         "try 7) from the context per step and verify them in one K+1-row forward (default: PC_LOOKUP, else off); "
                         "with --batch also for the batched loop (generate_batch(lookup=K): N * (K + 1) <= 64 rows per step) and "
                         "with --serve for the serving loop (serve(lookup=K): sampled requests draft and verify too)")
    ap.add_argument("--loop-prefill", action="store_true", default=None,
                    help="with --serve and --lookup K: a request admitted into the running loop is prefilled inside its step -- K + 1 "
                         "of its new tokens per replay, nobody else waits (serve(loop_prefill=True)); not with --slot-kv int8")
    ap.add_argument("--lookup-sampled", action="store_true", default=None,
                    help="with --lookup K: sampled generations (and greedy ones with a repetition penalty) draft and verify too, "
                         "the sampler drawing every row (SampleLookupLoop; default: PC_LOOKUP_SAMPLE=1, else off)")
    ap.add_argument("--weights", choices=("fp16", "mxfp4"), default=None,
                    help="decoder weight format (default: PC_WEIGHTS, else fp16); mxfp4 = OCP MX 4-bit blocks, Llama family: the "
                         "cached step and decode stream 4.25 bits per weight")
    ap.add_argument("--drop-fp16", action="store_true",
                    help="with --weights mxfp4: keep only the 4-bit images of the decoder weights resident (keep_fp16=False; default: "
                         "PC_W4_KEEP_FP16); passes above 64 rows expand each projection just in time")
    ap.add_argument("--logprobs", type=int, default=None,
                    help="print every generated token with its log-probability and its N most likely alternatives (0..8), under the "
                         "model's own distribution: the log-softmax of the raw logits, before temperature, penalty, top-p and top-k "
                         "(GenerationParameters.logprobs; with --batch for all sequences, with --serve as serve(logprobs=N))")
    ap.add_argument("--ban", type=int, nargs="+", default=None, metavar="ID",
                    help="token ids that may not be generated (GenerationParameters.banned_token_ids: a logit bias of -inf, applied in "
                         "front of temperature, penalty, top-p and top-k; with --serve as serve(token_controls=True))")
    ap.add_argument("--allow", type=int, nargs="+", default=None, metavar="ID",
                    help="the only token ids that may be generated (GenerationParameters.allowed_token_ids)")
    ap.add_argument("--min-new", type=int, default=0, metavar="N",
                    help="hold the stop token ids back for the first N generated tokens (GenerationParameters.min_new_tokens)")
    a = ap.parse_args()
    skw = dict(keep_arenas=False) if a.slot_drop_fp16 else {}
    wkw = dict(weight_format=a.weights, **(dict(keep_fp16=False) if a.drop_fp16 else {}))

    if os.path.isdir(a.model):
        import json
        arch = json.load(open(os.path.join(a.model, "config.json"))).get("model_type", "llama")
        lm = {"falcon": Falcon, "mpt": Mpt}.get(arch, Llama2)(a.model, **wkw)
    else:
        cls, shape = ADAPTERS[a.model]
        lm = cls(shape, random_init=True, **wkw)
    preproc = [lm.get_formatter()]
    cache_engine = CacheEngine(a.max_ctx, lm, module_kv=a.module_kv, slots=max(1, a.batch))
    gen_engine = GenerationEngine(lm, lookup=a.lookup, lookup_sampled=a.lookup_sampled)
    if a.schema:
        cache_engine.add_schema(read_file(a.schema, preproc), max_tokens=a.max_tokens)
        prompt_text = open(a.prompt_file).read()
    else:
        schema_text, prompt_text = synth.flat_docs("code-generation-game", 30, (306, 76, 800, 800, 800, 800, 800), 12)
        cache_engine.add_schema(lm.get_formatter()(schema_text), max_tokens=a.max_tokens)
    print(f"module KV ({cache_engine.module_kv}, {cache_engine.module_memory} tier): " +
          ", ".join(f"{nm} {b / 2 ** 20:.1f} MiB" for nm, b in cache_engine.module_bytes().items()))
    params = GenerationParameters(temperature=1.0, repetition_penalty=1.0, top_p=0.95, top_k=-1,
                                  max_new_tokens=a.max_new_tokens, stop_token_ids=lm.stop_token_ids, stop_str=lm.stop_str,
                                  logprobs=a.logprobs, banned_token_ids=a.ban, allowed_token_ids=a.allow, min_new_tokens=a.min_new)
    prompt = Prompt(prompt_text, preproc)
    for no_cache in (False, True, False):       # the first pass also warms the hipGraph / allocator
        token_ids, position_ids, cache_time, cache = cache_engine.process(
            prompt, no_cache=no_cache, return_full_position_ids=lm.use_full_position_ids)
        last = None
        for last in gen_engine.generate(token_ids, position_ids, params, cache, stream_interval=2,
                                        use_full_position_ids=lm.use_full_position_ids):
            pass
        staged = 0 if cache is None else cache[0][0].shape[1]
        print(f"{'no_cache' if no_cache else 'cached  '}: staged {staged:5d} + new {len(token_ids):5d} tokens | "
              f"gather {cache_time:7.3f} ms | first forward {last.elapsed_time:8.3f} ms | "
              f"TTFT {cache_time + last.elapsed_time:8.3f} ms | {a.max_new_tokens} tokens in {last.response_time:8.2f} ms")
    print("Assistant:", (last.new_text[:120] + " ...") if last else "")
    if last is not None and last.logprobs is not None:
        for r in last.logprobs:                  # one line per token: the token, then its alternatives by log-probability
            alts = "  ".join(f"{lm.decode([i])!r} {lp:.3f}" for i, lp in r.top)
            print(f"  {lm.decode([r.token])!r:>16} {r.logprob:9.3f}" + (f"   | {alts}" if alts else ""))
        print(f"  mean log-probability {sum(r.logprob for r in last.logprobs) / len(last.logprobs):.3f} over {len(last.logprobs)} tokens")
    if a.batch:
        import time
        # the same module selection with N different questions, one staged buffer (slot) each, decoded in one device loop
        cut = prompt_text.rfind("</prompt>")
        reqs = []
        for k in range(a.batch):
            pk = Prompt(prompt_text[:cut] + f"<user>{synth.words(4 + k % 5, 4000 + k)}</user>" + prompt_text[cut:], preproc)
            ids, pos, _, cache = cache_engine.process(pk, return_full_position_ids=lm.use_full_position_ids, slot=k)
            reqs.append((ids, pos, cache))
        batched, why = gen_engine.batch_plan(len(reqs), params, slot_kv=a.slot_kv)
        # (int8 images under lookup are serve's: generate_batch refuses the pair, so this batch decodes one token per step)
        lookup_b = 0 if a.slot_kv == "int8" and a.lookup else a.lookup
        # (likewise shared trunks over int8 images, DESIGN 3.33: serve's; this batch reads every slot's own image)
        share_b = a.share_trunk and a.slot_kv != "int8"
        for _pass in ("warm", "timed"):              # (the first pass captures the batched step)
            lasts = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k, out in gen_engine.generate_batch(reqs, params, stream_interval=2, share_trunk=share_b,
                                                     lookup=lookup_b, slot_kv=a.slot_kv):
                lasts[k] = out
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        n_tok = a.batch * a.max_new_tokens               # (fewer where a stop token or stop string ended a sequence early)
        print(f"batch of {a.batch} ({'one device loop' + (', int8 K/V images' if 'int8' in why else '') if batched else 'one after another: ' + why}): up to {n_tok} tokens in "
              f"{dt * 1e3:8.2f} ms, prefills included: {n_tok / dt:8.1f} tokens/s aggregate")
        print("Assistant[0]:", lasts[0].new_text[:120] + " ...")
    if a.serve:
        import dataclasses
        import time
        cut = prompt_text.rfind("</prompt>")
        budgets = [max(2, a.max_new_tokens // d) for d in (4, 1, 2, 8)]

        def stream():                                 # (lazy: a prompt is pulled when a slot is free)
            for r in range(a.serve):
                pr = Prompt(prompt_text[:cut] + f"<user>{synth.words(4 + r % 5, 5000 + r)}</user>" + prompt_text[cut:], preproc)
                yield pr, dataclasses.replace(params, max_new_tokens=budgets[r % len(budgets)])
        pkw = dict(loop_prefill=True) if a.loop_prefill else {}
        batched, why = gen_engine.serve_plan(a.lookup or 0, cache_engine.slots, slot_kv=a.slot_kv, **skw, **pkw)
        for _pass in ("warm", "timed"):
            lasts = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r, out in gen_engine.serve(cache_engine, stream(), stream_interval=2, share_trunk=a.share_trunk, lookup=a.lookup,
                                              slot_kv=a.slot_kv, logprobs=a.logprobs,
                                              token_controls=params.token_controls is not None or None, **skw, **pkw):
                lasts[r] = out
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        if batched:
            n_tok = sum(len(t) for t in gen_engine.last_serve_tokens.values())
            st = gen_engine.last_serve_stats
            print(f"served {a.serve} prompts through {cache_engine.slots} slots: {n_tok} tokens in {dt * 1e3:8.2f} ms, prefills included: "
                  f"{n_tok / dt:8.1f} tokens/s aggregate, {st['replays']} replays, "
                  f"{1.0 - st['live_rows'] / max(1, st['replays'] * cache_engine.slots):.2f} of the rows idle ({why})")
        else:
            print(f"served {a.serve} prompts one after another ({why}) in {dt * 1e3:8.2f} ms")
        print("Assistant[0]:", lasts[0].new_text[:120] + " ...")


if __name__ == "__main__":
    main()
