"""Helpers of tests/test_gpu_trunk.py: the ``mid``-shaped model over the ``deep`` persona schema with one staged buffer per
slot, a B = 1 prefill into a slot, and small device-tensor shorthands."""
import dataclasses

import torch

DEV = "cuda:0"
SENT = 77.0             # sentinel of memory nothing may write
PICKS = [((0, 1), 8), ((1, 2), 6), ((2, 0), 11), ((1, 1), 3)]
TRAITS = (("age", (30, 26, 33)), ("home", (41, 37, 44)))


def native():
    from promptcache_amd import _native
    _native.load()
    return _native


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def mid_setup(layers, seed, slots, picks_qlens, max_ctx=2048):
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    shape = dataclasses.replace(SHAPES["mid"], num_hidden_layers=layers, name=f"mid{layers}")
    w16 = make_weights_np(shape, seed, 2.0)
    lm = Llama2(name=shape.name, shape=shape, weights=w16, device=DEV)
    eng = CacheEngine(max_ctx, lm, slots=slots)
    prompts = []
    for pick, qlen in picks_qlens:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    eng.add_schema(lm.get_formatter()(sp))
    return shape, w16, lm, eng, prompts


def prefill(lm, eng, prompt, slot):
    ids, pos, _, cache = eng.process(prompt, slot=slot)
    out = lm(input_ids=torch.tensor([ids], device=DEV), position_ids=torch.tensor([pos], device=DEV), past_key_values=cache,
             use_cache=True)
    return ids, pos, out


def collect(gen):
    outs = {}
    for k, o in gen:
        outs.setdefault(k, []).append(o)
    return outs
