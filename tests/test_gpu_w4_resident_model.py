"""LlamaHIP(weight_format="mxfp4", keep_fp16=False): the model keeps the two 4-bit images of every decoder linear and no fp16
image of W'; a projection above PC_W4_MAX_ROWS rows is preceded by a ``pc_w4_expand`` of its weight into the model's one scratch.

Two models on the same weights, ``keep_fp16=True`` and ``False``, shapes mid64 and mid64_gqa at three layers (set up as
tests/test_gpu_w4_rows_model.py sets up).  The expansion is exact and the same kernels run on the same bytes, so every comparison
between the two is ``torch.equal``.  A counting shim around ``_native.w4_expand`` pins where the expansions happen."""
import dataclasses
import functools
import gc
import os
import sys

import numpy as np
import pytest
import torch

from oracle import engine_oracle as eo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOGIT_TOL = 1e-2        # tests/test_gpu_engine.py: the project's bar
SHAPES2 = ["mid64", "mid64_gqa"]
PICKS = [((0, 1), 8), ((1, 2), 6), ((2, 0), 11), ((1, 1), 3)]
TRAITS = (("age", (30, 26, 33)), ("home", (41, 37, 44)))
LINEARS = ("wqkv", "wo", "wgu", "wdown")


def _shape(name, layers=3):
    from promptcache_amd.model.config import SHAPES
    return dataclasses.replace(SHAPES[name], num_hidden_layers=layers, name=f"{name}-{layers}")


def _weights(shape, seed=9):
    from promptcache_amd.model.weights import make_weights_np
    return make_weights_np(shape, seed, 2.0)


class _Leg:
    """One model with its engine (schema encoded) and the prompts of PICKS."""

    def __init__(self, shape, w16, keep, dense):
        from promptcache_amd import CacheEngine, Prompt, synth
        from promptcache_amd.model import Llama2
        self.lm = Llama2(name=shape.name, shape=shape, weights=w16, device=DEV, weight_format="mxfp4", keep_fp16=keep)
        self.m = m = self.lm.hf_model
        assert m.w4 and m.w4_stream and m.keep_fp16 == keep
        if dense:                      # every pass above 64 rows on the many-row stack (_forward_dense), encode passes included
            m.MID_MAX_ROWS, m.encode_mid = m.SKINNY_MAX_ROWS, False
        self.eng = CacheEngine(2048, self.lm, slots=4)
        self.prompts = []
        for pick, qlen in PICKS:
            sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=pick)
            self.prompts.append(Prompt(pp, [self.lm.get_formatter()]))
        self.schema_text = self.lm.get_formatter()(sp)

    def question(self, rows):
        """The prompt whose cached step has exactly ``rows`` new rows (rows = question_len + a constant)."""
        from promptcache_amd import Prompt, synth

        def make(qlen):
            _, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=(0, 1))
            return Prompt(pp, [self.lm.get_formatter()])
        base = len(self.eng.process(make(4))[0]) - 4
        prompt = make(rows - base)
        assert len(self.eng.process(prompt)[0]) == rows, (rows, base)
        return prompt

    def prefill(self, prompt, slot=0, no_cache=False):
        ids, pos, _, cache = self.eng.process(prompt, slot=slot, no_cache=no_cache)
        out = self.lm(input_ids=torch.tensor([ids], device=DEV), position_ids=torch.tensor([pos], device=DEV), past_key_values=cache,
                      use_cache=True)
        return ids, pos, out

    def step(self, tok, pos, past):
        return self.lm(input_ids=torch.tensor([[tok]], device=DEV), position_ids=torch.tensor([[pos]], device=DEV),
                       past_key_values=past, use_cache=True)


def _pair(name, max_rows=64, dense=False):
    return _pair_cached(name, max_rows, dense)


@functools.lru_cache(maxsize=None)
def _pair_cached(name, max_rows, dense):
    """(kept leg, dropped leg, expand calls of the dropped leg's add_schema) on the same weights.  The environment is read by the
    constructors only (PC_W4_MAX_ROWS) and restored here: the pair is shared by the tests of this module."""
    from promptcache_amd import _native
    old = {k: os.environ.get(k) for k in ("PC_W4_MAX_ROWS", "PC_W4_STREAM", "PC_W4_KEEP_FP16")}
    os.environ["PC_W4_MAX_ROWS"] = str(max_rows)
    os.environ.pop("PC_W4_STREAM", None)
    os.environ.pop("PC_W4_KEEP_FP16", None)
    try:
        shape = _shape(name)
        w16 = _weights(shape)
        kept, drop = _Leg(shape, w16, True, dense), _Leg(shape, w16, False, dense)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert kept.m.w4_max_rows == max_rows and drop.m.w4_max_rows == max_rows
    real, calls = _native.w4_expand, []
    _native.w4_expand = lambda *a, **kw: (calls.append(a[3:6]), real(*a, **kw))[1]
    try:
        kept.eng.add_schema(kept.schema_text)
        assert calls == []
        drop.eng.add_schema(drop.schema_text)
    finally:
        _native.w4_expand = real
    return kept, drop, shape, tuple(calls)


def _count_calls(monkeypatch):
    """Wrap ``_native.w4_expand``: the list grows by (calling method, N, K, layout) of every call (a captured step calls it
    while it is captured; replays call nothing)."""
    from promptcache_amd import _native
    real, calls = _native.w4_expand, []

    def shim(codes_img, scales_img, out, N, K, layout=0, **kw):
        calls.append((sys._getframe(2).f_code.co_name, N, K, layout))
        return real(codes_img, scales_img, out, N, K, layout, **kw)
    monkeypatch.setattr(_native, "w4_expand", shim)
    return calls


def _new_rows(out, rows):
    """The rows a forward appended: the arena's fp16 K / V rows and, where the arena keeps one, the live rows of the residual tail
    (the rows behind ``tail_len`` were never written)."""
    a = out.past_key_values.arena
    tail = None if a.tail_lo is None else a.tail_lo[:, :, :, :, :a.tail_len].clone()
    return a.buf[:, :, :, :, a.length - rows:a.length].clone(), tail, a.tail_len


def _same_rows(x, y):
    assert torch.equal(x[0], y[0]) and x[2] == y[2] and (x[1] is None) == (y[1] is None)
    assert x[1] is None or torch.equal(x[1], y[1])


# ---------------------------------------------------------------------------------------------------
# bit equality of every forward
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", SHAPES2)
def test_schema_encode_and_no_cache_prefill_are_bit_equal(name, dense, monkeypatch):
    """Module KV after add_schema and the no-cache prefill, on the row-split stack (default) and with every pass above 64 rows
    forced onto _forward_dense (gemm_dense_qkv_rope included)."""
    kept, drop, shape, enc_calls = _pair(name, dense=dense)
    L = shape.num_hidden_layers
    a, b = list(kept.eng.schemas["deep"].cache_l1.values()), list(drop.eng.schemas["deep"].cache_l1.values())
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert torch.equal(x.store, y.store)
    # a kv-only pass stops behind the last layer's q|k|v: 4 (L - 1) + 1 expansions per pass
    assert len(enc_calls) > 0 and len(enc_calls) % (4 * (L - 1) + 1) == 0, len(enc_calls)
    # row-major images for pc_gemm_dense; by default the passes of 65..512 rows without a per-row prefix take fragment images
    assert {c[2] for c in enc_calls} <= ({1} if dense else {0, 1}), enc_calls[:4]
    calls = _count_calls(monkeypatch)
    _, _, o1 = kept.prefill(kept.prompts[0], no_cache=True)
    assert calls == []
    ids, _, o2 = drop.prefill(drop.prompts[0], no_cache=True)
    assert len(ids) > 64 and torch.equal(o1.logits, o2.logits)
    # (eager on the many-row stack: exactly one pass; the row-split stack is captured, possibly behind a warm-up: whole passes)
    assert len(calls) == 4 * L if dense else (len(calls) > 0 and len(calls) % (4 * L) == 0), len(calls)
    assert {c[0] for c in calls} == ({"_proj", "_forward_dense"} if dense else {"_forward_skinny"}), calls
    _same_rows(_new_rows(o1, len(ids)), _new_rows(o2, len(ids)))


@pytest.mark.parametrize("rows", [12, 40, 100, 130])
@pytest.mark.parametrize("name", SHAPES2)
def test_cached_step_is_bit_equal(name, rows, monkeypatch):
    """12 rows: pc_gemm_w4; 40: pc_gemm_w4_rows; 100 and 130: the row-split stack in its captured 16-row bucket, run twice (the
    second run replays the graph, whose expand nodes fill the scratch again)."""
    kept, drop, shape, _ = _pair(name)
    L = shape.num_hidden_layers
    pk, pd = kept.question(rows), drop.question(rows)
    calls = _count_calls(monkeypatch)
    want = []
    for _ in range(2):
        ids, _, o = kept.prefill(pk)
        want.append((o.logits.clone(), _new_rows(o, rows)))
    assert len(ids) == rows and calls == []
    assert torch.equal(want[0][0], want[1][0])
    seen = []
    for r in range(2):
        _, _, o = drop.prefill(pd)
        assert torch.equal(o.logits, want[r][0]), (rows, r)
        _same_rows(_new_rows(o, rows), want[r][1])
        seen.append(len(calls))
    if rows <= 64:
        assert calls == []                                      # the step streams the 4-bit images: nothing to expand
    else:
        # captured once (the capture may be preceded by an eager warm-up of the same launches): whole layers of four
        assert seen[0] > 0 and seen[0] % (4 * L) == 0 and {c[0] for c in calls} == {"_forward_skinny"} and {c[3] for c in calls} == {0}
        if drop.m.use_graphs and drop.m.graph_mid:
            assert seen[1] == seen[0]                           # the replay launches nothing from Python


def test_40_rows_with_w4_max_rows_16(monkeypatch):
    """PC_W4_MAX_ROWS=16: the 40-row step runs pc_gemm on expanded fragment images inside its captured graph."""
    kept, drop, shape, _ = _pair("mid64", max_rows=16)
    pk, pd = kept.question(40), drop.question(40)
    calls = _count_calls(monkeypatch)
    for r in range(2):
        before = len(calls)
        _, _, o1 = kept.prefill(pk)
        assert len(calls) == before                                # the kept model expands nothing
        _, _, o2 = drop.prefill(pd)
        assert torch.equal(o1.logits, o2.logits), r
        _same_rows(_new_rows(o1, 40), _new_rows(o2, 40))
    # (the step's graph and the sibling row tiles captured behind it: whole layers of four)
    assert len(calls) > 0 and len(calls) % (4 * shape.num_hidden_layers) == 0
    assert {c[0] for c in calls} == {"_forward_skinny"} and {c[3] for c in calls} == {0}


@pytest.mark.parametrize("name", SHAPES2)
def test_decode_steps_are_bit_equal_and_expand_nothing(name, monkeypatch):
    kept, drop, shape, _ = _pair(name)
    calls = _count_calls(monkeypatch)
    outs = []
    for leg in (kept, drop):
        ids, pos, out = leg.prefill(leg.prompts[0])
        rows = [out.logits[0, -1].clone()]
        tok, p, past = int(torch.argmax(rows[0])), max(pos) + 2, out.past_key_values
        for _ in range(4):
            out = leg.step(tok, p, past)
            rows.append(out.logits[0, -1].clone())
            tok, p, past = int(torch.argmax(rows[-1])), p + 1, out.past_key_values
        outs.append((torch.stack(rows), _new_rows(out, len(ids) + 4)))
    assert len(ids) <= 16 and calls == []
    assert torch.equal(outs[0][0], outs[1][0])
    _same_rows(outs[0][1], outs[1][1])


def test_generate_with_lookup_and_generate_batch_reproduce_the_texts(monkeypatch):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    kept, drop, shape, _ = _pair("mid64_gqa")
    params = GenerationParameters(temperature=0.0, max_new_tokens=16, stop_token_ids=[])
    calls = _count_calls(monkeypatch)
    texts = []
    for leg in (kept, drop):
        ge = GenerationEngine(leg.lm, lookup=3)
        ids, pos, _, cache = leg.eng.process(leg.prompts[0])
        solo = list(ge.generate(ids, pos, params, cache))[-1].new_text
        reqs = [leg.eng.process(p, slot=j) for j, p in enumerate(leg.prompts)]
        last = {}
        for j, o in GenerationEngine(leg.lm).generate_batch([(r[0], r[1], r[3]) for r in reqs], params, lookup=0):
            last[j] = o.new_text
        texts.append((solo, [last[j] for j in range(4)]))
    assert texts[0] == texts[1] and len(texts[0][0]) > 0
    assert calls == []                  # k + 1 = 4 rows per verify step, 4 rows per slot step: the 4-bit images all the way


# ---------------------------------------------------------------------------------------------------
# the oracle on the rebuilt W', residency
# ---------------------------------------------------------------------------------------------------

def test_dequantized_weights_of_the_dropped_model_against_the_oracle():
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    kept, drop, shape, _ = _pair("mid64_gqa")
    m = drop.m
    wk, wd = kept.m.dequantized_weights(), m.dequantized_weights()
    assert sorted(wk) == sorted(wd)
    for k in wk:
        assert torch.equal(wk[k].view(torch.int16), wd[k].view(torch.int16)), k
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    model = LlamaOracle(cfg, {k: v.float().cpu().numpy() for k, v in wd.items()})
    sc = drop.eng.get_schema("deep")
    jobs = []
    for p in sc.encode_paths():
        sf = sc.get_scaffold(p)
        jobs.append(dict(token_ids=sf.token_ids(), position_ids=sf.position_ids(), targets=sf.select(p).all_token_sequences()))
    lib = eo.encode_schema(model, jobs)
    ids, pos, out = drop.prefill(drop.prompts[0])
    used = [mm.token_sequence for mm in drop.eng.slot_cache(0).staged]
    _, S, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
    worst = float(np.abs(out.logits[0, -1].cpu().numpy() - olog[0, -1]).max())
    print(f"W4_RESIDENT mid64_gqa: {len(ids)}-row cached prefill of the keep_fp16=False model vs the oracle on its W': "
          f"max|dlogit| = {worst:.2e}")
    assert worst < LOGIT_TOL, worst


@pytest.mark.parametrize("name", SHAPES2)
def test_resident_bytes_match_the_formula(name):
    """A fresh keep_fp16=False model holds, counted once per storage: the 4-bit images (N K / 2 code bytes + N K / 32 scale
    bytes per linear), the layer norms, the embeddings, the final norm, both lm_head images, the scratch (the largest
    projection, gate|up, in fp16) and its index words (the q|k|v permutation as int64 and int32, the rotary frequencies)."""
    from promptcache_amd.model.llama_hip import LlamaHIP
    shape = _shape(name)
    w16 = _weights(shape)
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.memory_allocated()
    m = LlamaHIP(shape, w16, device=DEV, weight_format="mxfp4", keep_fp16=False)
    hid, inter, V, L = shape.hidden_size, shape.intermediate_size, shape.vocab_size, shape.num_hidden_layers
    HD, W = m.H * m.D, (m.H + 2 * m.Hkv) * m.D
    lin = W * hid + hid * HD + 2 * inter * hid + hid * inter
    images = L * (lin // 2 + lin // 32)
    norms = (2 * L + 1) * hid * 2
    emb_head = 3 * V * hid * 2
    scratch = 2 * inter * hid * 2
    index = W * 8 + W * 4 + (m.D // 2) * 4
    assert m._w16_scratch.numel() == 2 * inter * hid
    assert m.resident_bytes() == images + norms + emb_head + scratch + index, (m.resident_bytes(), images, norms, emb_head, scratch, index)
    for lw in m.layers:
        for k, v in lw.items():
            assert not (isinstance(v, torch.Tensor) and v.dtype == torch.float16 and v.dim() >= 2), k
            assert v is not None or k.split("_")[0] in LINEARS
        assert all(lw[k] is None and lw[k + "_f"] is None for k in LINEARS)
    # ... and the allocator agrees up to its block rounding: nothing else survived the constructor
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - free0
    assert m.resident_bytes() <= held <= m.resident_bytes() + 512 * len(m.resident_tensors()), (held, m.resident_bytes())
    kept = LlamaHIP(shape, w16, device=DEV, weight_format="mxfp4")
    assert kept.keep_fp16 and kept._w16_scratch is None
    assert kept.resident_bytes() == m.resident_bytes() - scratch + 2 * L * lin * 2
