"""LlamaHIP(weight_format="mxfp4") with PC_W4_MAX_ROWS=64: the 17..64-row steps -- the cached step with a 17..64-token question
(the generic loop of ``_forward_skinny``) and the slot-lookup verify step of S * (k + 1) rows -- stream the 4-bit images through
pc_gemm_w4_rows.  Shapes mid64 and mid64_gqa at three layers, built as tests/test_gpu_w4_model.py builds them; every test wraps
``_native.gemm_w4_rows`` in a counting shim and asserts that the step went through it."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import engine_oracle as eo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOGIT_TOL = 1e-2        # tests/test_gpu_engine.py: the project's bar
SHAPES2 = ["mid64", "mid64_gqa"]
PICKS = [((0, 1), 8), ((1, 2), 6), ((2, 0), 11), ((1, 1), 3), ((0, 0), 5), ((2, 2), 9), ((2, 1), 7), ((0, 2), 4)]
TRAITS = (("age", (30, 26, 33)), ("home", (41, 37, 44)))


def _shape(name, layers=3):
    from promptcache_amd.model.config import SHAPES
    return dataclasses.replace(SHAPES[name], num_hidden_layers=layers, name=f"{name}-{layers}")


def _weights(shape, seed=9):
    from promptcache_amd.model.weights import make_weights_np
    return make_weights_np(shape, seed, 2.0)


def _setup(name, slots, picks, monkeypatch, stream=True, max_rows=64, seed=9):
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    monkeypatch.setenv("PC_W4_STREAM", "1" if stream else "0")
    monkeypatch.setenv("PC_W4_MAX_ROWS", str(max_rows))
    shape = _shape(name)
    w16 = _weights(shape, seed)
    lm = Llama2(name=shape.name, shape=shape, weights=w16, device=DEV, weight_format="mxfp4")
    m = lm.hf_model
    assert m.weight_format == "mxfp4" and m.w4 and m.w4_stream == stream and m.w4_max_rows == max_rows
    eng = CacheEngine(2048, lm, slots=slots)
    prompts = []
    for pick, qlen in picks:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    eng.add_schema(lm.get_formatter()(sp))
    return shape, w16, lm, eng, prompts


STEP, LOOKUP = "_forward_skinny", "_forward_lookup_slots"      # the two flows that call pc_gemm_w4_rows


def _count_calls(monkeypatch):
    """Wrap ``_native.gemm_w4_rows``: the list grows by (calling method, rows) of every call (a captured step calls it while it is
    captured; the prefills of a batch are cached steps of their own)."""
    import sys
    from promptcache_amd import _native
    real, calls = _native.gemm_w4_rows, []

    def shim(codes_img, scales_img, xf_hi, xf_lo, M, *a, **kw):
        calls.append((sys._getframe(1).f_code.co_name, M))
        return real(codes_img, scales_img, xf_hi, xf_lo, M, *a, **kw)
    monkeypatch.setattr(_native, "gemm_w4_rows", shim)
    return calls


def _rows_of(calls, flow):
    return [M for who, M in calls if who == flow]


def _oracle(shape, m):
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    return LlamaOracle(cfg, {k: v.float().cpu().numpy() for k, v in m.dequantized_weights().items()})


def _library(model, eng):
    sc = eng.get_schema("deep")
    jobs = []
    for p in sc.encode_paths():
        sf = sc.get_scaffold(p)
        jobs.append(dict(token_ids=sf.token_ids(), position_ids=sf.position_ids(), targets=sf.select(p).all_token_sequences()))
    return eo.encode_schema(model, jobs)


def _prefill(lm, eng, prompt, slot):
    ids, pos, _, cache = eng.process(prompt, slot=slot)
    out = lm(input_ids=torch.tensor([ids], device=DEV), position_ids=torch.tensor([pos], device=DEV), past_key_values=cache,
             use_cache=True)
    return ids, pos, out


def _step(lm, tok, pos, past):
    return lm(input_ids=torch.tensor([[tok]], device=DEV), position_ids=torch.tensor([[pos]], device=DEV), past_key_values=past,
              use_cache=True)


def _question(lm, eng, rows):
    """The prompt whose cached step has exactly ``rows`` new rows."""
    from promptcache_amd import Prompt, synth
    for qlen in range(2, rows + 1):
        _, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=(0, 1))
        prompt = Prompt(pp, [lm.get_formatter()])
        if len(eng.process(prompt)[0]) == rows:
            return prompt
    raise AssertionError(f"no question length gives {rows} new rows")


def _cached_step_run(name, rows, monkeypatch, stream, max_rows=64, oracle=True, decode=4):
    """First forward of a ``rows``-row question and ``decode`` decode steps; returns (logit rows, new K / V rows + residuals, calls)."""
    calls = _count_calls(monkeypatch)
    shape, w16, lm, eng, _ = _setup(name, 1, PICKS[:1], monkeypatch, stream, max_rows)
    m = lm.hf_model
    prompt = _question(lm, eng, rows)
    ids, pos, out = _prefill(lm, eng, prompt, 0)
    assert len(ids) == rows
    logits = [out.logits[0, -1].cpu().numpy()]
    full = out.logits[0].cpu().numpy()
    a = out.past_key_values.arena
    assert m.tail_supported and a.tail_lo is not None and a.tail_len == rows
    tail = a.tail_lo[:, :, :, :, :rows].float().cpu().numpy()
    assert float((tail != 0).mean()) > 0.5
    new = a.buf[:, :, :, :, a.length - rows:a.length].float().cpu().numpy() + tail
    worst = 0.0
    if oracle:
        model = _oracle(shape, m)
        lib = _library(model, eng)
        used = [mm.token_sequence for mm in eng.slot_cache(0).staged]
        _, S, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        worst = float(np.abs(logits[0] - olog[0, -1]).max())
        assert worst < LOGIT_TOL, (stream, "first forward", rows, worst)
    tok, p, past = int(np.argmax(logits[0])), max(pos) + 2, out.past_key_values
    for i in range(decode):
        out = _step(lm, tok, p, past)
        logits.append(out.logits[0, -1].cpu().numpy())
        if oracle:
            olog, present = model.forward(np.array([[tok]]), np.array([[p]]), past=present)
            err = float(np.abs(logits[-1] - olog[0, -1]).max())
            worst = max(worst, err)
            assert err < LOGIT_TOL, (stream, i, rows, err)
        tok, p, past = int(np.argmax(logits[-1])), p + 1, out.past_key_values
    if oracle:
        print(f"W4_ROWS_MODEL {name} rows={rows} stream={int(stream)}: first forward + {decode} decode steps vs the oracle on W': "
              f"max|dlogit| = {worst:.2e}")
    monkeypatch.undo()
    return np.stack(logits), full, new, list(calls)


def _went_through(calls, rows):
    """The step is captured at its row tile (the bucketed small-q graphs: 20 rows replay the 32-row graph) and the sibling tiles
    are captured behind it: every call has 17..64 rows and the step's own tile is among them."""
    got = _rows_of(calls, STEP)
    assert len(got) == len(calls) and all(16 < M <= 64 for M in got) and (rows in got or -(-rows // 16) * 16 in got), (rows, sorted(set(calls)))


@pytest.mark.parametrize("rows", [20, 40, 64])
@pytest.mark.parametrize("name", SHAPES2)
def test_cached_step_of_17_to_64_rows_against_the_oracle_on_w_prime(name, rows, monkeypatch):
    """The step on the 4-bit images and the same step with PC_W4_STREAM=0 (the fp16 images of W'), both below the project's bar
    against LlamaOracle on W'; the differences between the two runs are printed, not bounded."""
    got, _, new4, calls = _cached_step_run(name, rows, monkeypatch, True)
    _went_through(calls, rows)
    ref, _, new16, none = _cached_step_run(name, rows, monkeypatch, False)
    assert none == []
    print(f"W4_ROWS_MODEL {name} rows={rows}: 4-bit images vs fp16 images of W': max|dlogit| = {float(np.abs(got - ref).max()):.2e}")
    print(f"W4_ROWS_MODEL {name} rows={rows}: new K / V rows (fp16 + residual), 4-bit vs fp16 images: max|d| = "
          f"{float(np.abs(new4 - new16).max()):.2e} at max|kv| = {float(np.abs(new16).max()):.2f}")


def test_cached_step_with_the_decode_tail(monkeypatch):
    monkeypatch.setenv("PC_DECODE_TAIL", "1")
    _, _, _, calls = _cached_step_run("mid64_gqa", 40, monkeypatch, True)
    _went_through(calls, 40)


def test_the_gate_keeps_the_step_on_the_fp16_images(monkeypatch):
    """PC_W4_MAX_ROWS=16: the 40-row step never calls pc_gemm_w4_rows and its logits are the PC_W4_STREAM=0 run's, bit for bit."""
    _, full16, _, calls = _cached_step_run("mid64", 40, monkeypatch, True, max_rows=16, oracle=False, decode=0)
    assert calls == []
    _, full0, _, none = _cached_step_run("mid64", 40, monkeypatch, False, max_rows=16, oracle=False, decode=0)
    assert none == [] and np.array_equal(full16.view(np.int32), full0.view(np.int32))


@pytest.mark.parametrize("slots,k,share", [(4, 7, False), (8, 3, False), (8, 3, True)])
def test_slot_lookup_of_32_rows_emits_greedy_decoding_tokens(slots, k, share, monkeypatch):
    """generate_batch(lookup=k) over S slots, S * (k + 1) = 32 rows per verify step on the 4-bit images: the texts are plain
    generate_batch's and solo generate's."""
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    calls = _count_calls(monkeypatch)
    shape, w16, lm, eng, prompts = _setup("mid64_gqa", slots, PICKS[:slots], monkeypatch)
    params = GenerationParameters(temperature=0.0, max_new_tokens=24, stop_token_ids=[])
    ge = GenerationEngine(lm)
    texts = []
    for lookup in (0, k):
        reqs = [eng.process(p, slot=j) for j, p in enumerate(prompts)]
        before = len(calls)
        last = {}
        kw = dict(share_trunk=True) if share else {}
        for j, o in ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, lookup=lookup, **kw):
            last[j] = o.new_text
        texts.append([last[j] for j in range(slots)])
        verify = _rows_of(calls[before:], LOOKUP)
        if lookup:
            assert verify and set(verify) == {slots * (k + 1)}, verify
        else:
            assert verify == []                                   # S <= 16 rows per plain step: pc_gemm_w4
    assert texts[0] == texts[1]
    for j in (0, slots - 1):
        ids, pos, _, cache = eng.process(prompts[j])
        assert list(ge.generate(ids, pos, params, cache))[-1].new_text == texts[1][j], j


@pytest.mark.parametrize("slots", [4, 5])                        # 16 rows: pc_gemm_w4 as before; 20 rows: pc_gemm_w4_rows
def test_serve_with_lookup_equals_plain_serve(slots, monkeypatch):
    """Six requests, greedy and sampled in turn, through S slots with lookup = 3: every request's tokens are plain serve's on the
    same seeds (tests/test_gpu_w4_model.py::test_serve_six_requests_through_three_slots is the pattern)."""
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters as G
    calls = _count_calls(monkeypatch)
    shape, w16, lm, eng, prompts = _setup("mid64", slots, PICKS[:6], monkeypatch)
    ge = GenerationEngine(lm)
    assert ge.serve_plan()[0]
    max_news = [9, 14, 6, 11, 8, 12]
    kinds = [dict(temperature=0.0), dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40), dict(temperature=0.0),
             dict(temperature=1.3, repetition_penalty=1.3, top_p=0.8, top_k=12), dict(temperature=0.0, repetition_penalty=1.2),
             dict(temperature=0.0)]

    def run(lookup):
        reqs = [(prompts[r], G(max_new_tokens=max_news[r], stop_token_ids=[], **kinds[r])) for r in range(6)]
        torch.manual_seed(5)
        last = {}
        for r, o in ge.serve(eng, iter(reqs), lookup=lookup):
            last[r] = o
        tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
        assert sorted(last) == list(range(6)) and [len(tokens[r]) for r in range(6)] == max_news
        return tokens, {r: last[r].new_text for r in range(6)}
    plain, plain_text = run(0)
    assert _rows_of(calls, LOOKUP) == []
    got, got_text = run(3)
    verify = _rows_of(calls, LOOKUP)
    if slots * 4 > 16:
        assert verify and set(verify) == {slots * 4}, verify
    else:
        assert verify == []
    for r in range(6):
        assert got[r] == plain[r], (r, got[r], plain[r])
        assert got_text[r] == plain_text[r], r
