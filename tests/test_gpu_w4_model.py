"""LlamaHIP(weight_format="mxfp4"): the model is the fp16 model with the dequantised weights W' -- so every oracle applies with
W' at the project's bars -- and its <= 16-row projections stream the 4-bit images (pc_gemm_w4).  Shapes mid64 and mid64_gqa,
three layers, weights as the engine tests draw them."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import engine_oracle as eo
from tests import mxfp4_ref as mx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOGIT_TOL = 1e-2        # tests/test_gpu_engine.py: the project's bar
MARGIN = 2e-2           # a token is compared where the oracle's own top-2 margin exceeds twice the bar
SHAPES2 = ["mid64", "mid64_gqa"]
PICKS = [((0, 1), 8), ((1, 2), 6), ((2, 0), 11), ((1, 1), 3), ((0, 0), 5), ((2, 2), 9)]
TRAITS = (("age", (30, 26, 33)), ("home", (41, 37, 44)))


def _shape(name, layers=3):
    from promptcache_amd.model.config import SHAPES
    return dataclasses.replace(SHAPES[name], num_hidden_layers=layers, name=f"{name}-{layers}")


def _weights(shape, seed=9):
    from promptcache_amd.model.weights import make_weights_np
    return make_weights_np(shape, seed, 2.0)


def _setup(name, slots, picks, monkeypatch=None, stream=True, seed=9):
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    if monkeypatch is not None:
        monkeypatch.setenv("PC_W4_STREAM", "1" if stream else "0")
    shape = _shape(name)
    w16 = _weights(shape, seed)
    lm = Llama2(name=shape.name, shape=shape, weights=w16, device=DEV, weight_format="mxfp4")
    m = lm.hf_model
    assert m.weight_format == "mxfp4" and m.w4 and m.w4_stream == stream
    eng = CacheEngine(2048, lm, slots=slots)
    prompts = []
    for pick, qlen in picks:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    eng.add_schema(lm.get_formatter()(sp))
    return shape, w16, lm, eng, prompts


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


@pytest.mark.parametrize("name", SHAPES2)
def test_dequantized_weights_are_the_restatements(name):
    from promptcache_amd.model.llama_hip import LlamaHIP
    shape = _shape(name, 2)
    w16 = _weights(shape)
    m = LlamaHIP(shape, w16, device=DEV, weight_format="mxfp4")
    d = m.dequantized_weights()
    assert sorted(d) == sorted(w16)
    for k, v in w16.items():
        got = d[k].cpu().numpy()
        assert got.dtype == np.float16 and got.shape == v.shape, k
        if k.split(".")[-1] in ("wq", "wk", "wv", "wo", "gate", "up", "down"):
            want = mx.dequantize(*mx.quantize(v)).astype(np.float16)
            assert not np.array_equal(want, v.astype(np.float16)), k
        else:
            want = v.astype(np.float16)                    # embed, the norms and lm_head stay fp16
        assert np.array_equal(got, want), k
    lw = m.layers[0]
    assert lw["wqkv_c4"].dtype == torch.uint8 and lw["wdown_e4"].dtype == torch.uint8
    assert m.slot_loop_available() and m.lookup_available()


@pytest.mark.parametrize("name", SHAPES2)
def test_cached_prefill_and_decode_against_the_oracle_on_w_prime(name, monkeypatch):
    """A 12-row cached prefill over staged modules and 8 decode steps against LlamaOracle on W', the device leading; the same
    run with PC_W4_STREAM=0 (the fp16 images of W') at the same bar; the difference between the two runs is printed."""
    from promptcache_amd import Prompt, synth
    runs, tails, news = {}, {}, {}
    for stream in (True, False):
        shape, w16, lm, eng, _ = _setup(name, 1, PICKS[:1], monkeypatch, stream)
        m = lm.hf_model
        for qlen in range(2, 16):                          # the question length that gives 12 new rows
            _, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=(0, 1))
            prompt = Prompt(pp, [lm.get_formatter()])
            if len(eng.process(prompt)[0]) == 12:
                break
        model = _oracle(shape, m)
        lib = _library(model, eng)
        ids, pos, out = _prefill(lm, eng, prompt, 0)
        assert len(ids) == 12
        used = [mm.token_sequence for mm in eng.slot_cache(0).staged]
        _, S, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        rows = [out.logits[0, -1].cpu().numpy()]
        worst = float(np.abs(rows[0] - olog[0, -1]).max())
        assert worst < LOGIT_TOL, (stream, "prefill", worst)
        # the prompt's own K / V rows keep their fp16 residuals in either run (the tail pc_rope_append_ex / the fused epilogue write)
        a = out.past_key_values.arena
        assert m.tail_supported and m._lo_mode == 1 and a.tail_lo is not None and a.tail_len == 12
        tails[stream] = a.tail_lo[:, :, :, :, :12].float().cpu().numpy()
        news[stream] = a.buf[:, :, :, :, a.length - 12:a.length].float().cpu().numpy() + tails[stream]
        tok, p, past = int(np.argmax(rows[0])), max(pos) + 2, out.past_key_values
        for i in range(8):
            out = _step(lm, tok, p, past)
            olog, present = model.forward(np.array([[tok]]), np.array([[p]]), past=present)
            rows.append(out.logits[0, -1].cpu().numpy())
            err = float(np.abs(rows[-1] - olog[0, -1]).max())
            worst = max(worst, err)
            assert err < LOGIT_TOL, (stream, i, err)
            tok, p, past = int(np.argmax(rows[-1])), p + 1, out.past_key_values
        print(f"W4_MODEL {name} stream={int(stream)}: 12-row cached prefill + 8 decode steps vs the oracle on W': max|dlogit| = {worst:.2e}")
        runs[stream] = np.stack(rows)
        del lm, eng, m
    print(f"W4_MODEL {name}: 4-bit images vs fp16 images of W': max|dlogit| = {float(np.abs(runs[True] - runs[False]).max()):.2e}")
    assert float((tails[True] != 0).mean()) > 0.5 and float((tails[False] != 0).mean()) > 0.5
    d = float(np.abs(news[True] - news[False]).max())
    print(f"W4_MODEL {name}: new K / V rows (fp16 + residual), 4-bit vs fp16 images: max|d| = {d:.2e} at max|kv| = {float(np.abs(news[False]).max()):.2f}")
    assert d < 1e-3            # the same rows in the same places (an fp16 ulp at |kv| ~ 4 is 4e-3: the residuals are in)


@pytest.mark.parametrize("name", SHAPES2)
def test_decode_tail_continues_through_the_decode_steps(name, monkeypatch):
    """PC_DECODE_TAIL=1 on the 4-bit images: every decode step appends its residual row behind the prefill's (the row offset is read
    on the device, pc_rope_append_ex lo_row0 = -2), stepping and GreedyLoop give the same tokens, logits at the project's bar."""
    monkeypatch.setenv("PC_DECODE_TAIL", "1")
    shape, w16, lm, eng, prompts = _setup(name, 1, PICKS[:1], monkeypatch, True)
    m = lm.hf_model
    assert m.decode_tail and m.tail_supported
    model = _oracle(shape, m)
    lib = _library(model, eng)
    ids, pos, out = _prefill(lm, eng, prompts[0], 0)
    used = [mm.token_sequence for mm in eng.slot_cache(0).staged]
    _, S, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
    a = out.past_key_values.arena
    n0, rows0, q = a.length, a.buf[:, :, :, :, :a.length].clone(), len(ids)
    tail0 = a.tail_lo.clone()
    first, p0 = int(torch.argmax(out.logits[0, -1])), max(pos) + 2
    tok, past, stepped, worst = first, out.past_key_values, [], 0.0
    for i in range(8):
        o = _step(lm, tok, p0 + i, past)
        olog, present = model.forward(np.array([[tok]]), np.array([[p0 + i]]), past=present)
        worst = max(worst, float(np.abs(o.logits[0, -1].cpu().numpy() - olog[0, -1]).max()))
        tok, past = int(torch.argmax(o.logits[0, -1])), o.past_key_values
        stepped.append(tok)
    assert worst < LOGIT_TOL, worst
    assert a.tail_len == q + 8 and m._lo_mode == 2
    lo = a.tail_lo[:, :, :, :, q:q + 8]
    assert float((lo != 0).float().mean()) > 0.5                        # the decoded rows' residuals were written
    print(f"W4_MODEL {name} PC_DECODE_TAIL=1: 8 decode steps vs the oracle on W': max|dlogit| = {worst:.2e}")
    stepped_tail = a.tail_lo[:, :, :, :, :q + 8].clone()
    with torch.inference_mode():                         # (the tail was allocated inside a forward: an inference tensor)
        a.buf[:, :, :, :, :n0].copy_(rows0)
        a.tail_lo.copy_(tail0)
    a.length, a.tail_len = n0, q
    g = m.greedy_loop(a.views(n0), first, p0, 8)
    looped = [g.token(g.enqueue()) for _ in range(8)]
    g.close(8)
    assert looped == stepped
    assert torch.equal(a.tail_lo[:, :, :, :, :q + 8].view(torch.int16), stepped_tail.view(torch.int16))


@pytest.mark.parametrize("name", SHAPES2)
def test_greedy_loop_tokens_equal_stepping_through_the_model(name):
    from promptcache_amd.model.llama_hip import GreedyLoop
    shape, w16, lm, eng, prompts = _setup(name, 1, PICKS[:1])
    m = lm.hf_model
    N = 24
    ids, pos, out = _prefill(lm, eng, prompts[0], 0)
    a = out.past_key_values.arena
    n0, rows0 = a.length, a.buf[:, :, :, :, :a.length].clone()
    first, p0 = int(torch.argmax(out.logits[0, -1])), max(pos) + 2
    stepped, tok, past = [], first, out.past_key_values
    for i in range(N):
        o = _step(lm, tok, p0 + i, past)
        tok, past = int(torch.argmax(o.logits[0, -1])), o.past_key_values
        stepped.append(tok)
    a.buf[:, :, :, :, :n0].copy_(rows0)
    a.length = n0
    g = m.greedy_loop(a.views(n0), first, p0, N)
    assert type(g) is GreedyLoop
    looped = [g.token(g.enqueue()) for _ in range(N)]
    g.close(N)
    assert looped == stepped and len(set(looped)) > 4


@pytest.mark.parametrize("name", SHAPES2)
def test_generate_batch_over_four_slots(name):
    """Each sequence's tokens equal its tokens alone in a loop of the same slot count and max_keys, and the oracle-fed greedy
    tokens wherever the oracle's top-2 margin exceeds 2e-2."""
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    shape, w16, lm, eng, prompts = _setup(name, 4, PICKS[:4])
    m = lm.hf_model
    ge = GenerationEngine(lm)
    max_new = 16
    params = GenerationParameters(temperature=0.0, max_new_tokens=max_new, stop_token_ids=[])
    assert ge.batch_plan(4, params)[0] and ge.serve_plan()[0]
    model = _oracle(shape, m)
    lib = _library(model, eng)
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
    outs = {}
    for k, o in ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params):
        outs[k] = o
    max_keys = max(eng.slot_cache(k).arena.length for k in range(4)) + 1      # (prefill rows + decode steps + 1: the batch's own bound)
    compared = 0
    for k, prompt in enumerate(prompts):
        ids, pos, out = _prefill(lm, eng, prompt, k)
        first, p0 = int(torch.argmax(out.logits[0, -1])), max(pos) + 2
        # the oracle, fed the tokens the solo loop produces
        used = [mm.token_sequence for mm in eng.slot_cache(k).staged]
        _, S, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        loop = m.slot_loop([out.past_key_values], [first], [p0], max_new - 1, slots=4, max_keys=max_keys)
        assert loop is not None and loop.S == 4
        solo = [first]
        try:
            for i in range(max_new - 1):
                loop.enqueue()
                solo.append(loop.token(0, i))
        finally:
            loop.close([max_new - 1])
        assert outs[k].new_text == lm.decode(solo), k
        top2 = np.sort(olog[0, -1])[-2:]
        if top2[1] - top2[0] > MARGIN:
            assert int(np.argmax(olog[0, -1])) == solo[0], (k, "first")
            compared += 1
        for i in range(max_new - 1):
            olog, present = model.forward(np.array([[solo[i]]]), np.array([[p0 + i]]), past=present)
            top2 = np.sort(olog[0, -1])[-2:]
            if top2[1] - top2[0] > MARGIN:
                assert int(np.argmax(olog[0, -1])) == solo[i + 1], (k, i)
                compared += 1
    print(f"W4_MODEL {name}: generate_batch over 4 slots, {compared} of {4 * max_new} tokens compared with the oracle (margin > {MARGIN})")
    assert compared > 2 * max_new


def test_serve_six_requests_through_three_slots():
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    shape, w16, lm, eng, prompts = _setup("mid64", 3, PICKS)
    ge = GenerationEngine(lm)
    assert ge.serve_plan()[0]
    max_news = [9, 14, 6, 11, 8, 12]

    def requests(which):
        return [(prompts[r], GenerationParameters(temperature=0.0, max_new_tokens=max_news[r], stop_token_ids=[])) for r in which]
    last = {}
    for r, o in ge.serve(eng, requests(range(6))):
        last[r] = o
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert sorted(last) == list(range(6)) and [len(tokens[r]) for r in range(6)] == max_news
    for r in range(6):
        solo_out = None
        for _, o in ge.serve(eng, requests([r])):
            solo_out = o
        assert list(ge.last_serve_tokens[0]) == tokens[r], r
        assert solo_out.new_text == last[r].new_text, r


def test_the_three_refusals():
    from promptcache_amd.model import Falcon, Llama2
    from promptcache_amd.model.config import FALCON_SHAPES, SHAPES
    from promptcache_amd.model.llama_hip import LlamaHIP
    mid = dataclasses.replace(SHAPES["mid"], num_hidden_layers=1, name="mid-1")
    free0 = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="intermediate_size"):
        LlamaHIP(mid, _weights(mid), device=DEV, weight_format="mxfp4")
    ok = _shape("mid64", 1)
    with pytest.raises(ValueError, match="load_in_8bit"):
        Llama2(name=ok.name, shape=ok, weights=_weights(ok), device=DEV, weight_format="mxfp4", load_in_8bit=True)
    fs = dataclasses.replace(next(iter(FALCON_SHAPES.values())), num_hidden_layers=1)
    with pytest.raises(ValueError, match="Llama family"):
        Falcon(name=fs.name, shape=fs, weights={}, device=DEV, weight_format="mxfp4")
    with pytest.raises(ValueError, match="weight_format"):
        LlamaHIP(ok, _weights(ok), device=DEV, weight_format="int4")
    assert torch.cuda.memory_allocated() == free0            # refused before anything was allocated


def test_lookup_loops_emit_greedy_decoding_tokens():
    """Prompt-lookup drafts verified on the 4-bit images (k + 1 <= 16 rows in the single loop, S * (k + 1) <= 16 in the slot
    loop): the texts are plain greedy decoding's."""
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    shape, w16, lm, eng, prompts = _setup("mid64_gqa", 2, PICKS[:2])
    params = GenerationParameters(temperature=0.0, max_new_tokens=24, stop_token_ids=[])
    plain, look = GenerationEngine(lm), GenerationEngine(lm, lookup=7)
    ids, pos, _, cache = eng.process(prompts[0])
    want = list(plain.generate(ids, pos, params, cache))[-1].new_text
    ids, pos, _, cache = eng.process(prompts[0])
    assert list(look.generate(ids, pos, params, cache))[-1].new_text == want
    texts = []
    for lookup in (0, 3):
        reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
        last = {}
        for k, o in plain.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, lookup=lookup):
            last[k] = o.new_text
        texts.append([last[0], last[1]])
    assert texts[0] == texts[1] and texts[0][0] == want
