"""The batched slot loop over int8 K / V images on the GPU (LlamaHIP.slot_loop(kv="int8")): against the numpy oracle
with the device leading and the oracle fed the DEVICE's dequantised image rows, the images bit for bit against
tests/kv_q8_ref.py of the fp16 arenas after every step, slot invariance (fp16 and MXFP4 weights), GenerationEngine.generate_batch
and serve with ``slot_kv="int8"``, the fp16 mode untouched, and the refusals."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import kv_q8_ref as q8
from tests.test_gpu_slots import LOGIT_TOL, PICKS, _collect, _prefill

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAITS = (("age", (30, 26, 33)), ("home", (41, 37, 44)))
MAX_CTX = 2048


def _prompts(lm, picks):
    from promptcache_amd import Prompt, synth
    prompts = []
    for pick, qlen in picks:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    return lm.get_formatter()(sp), prompts


def _build(name, layers, seed, **kw):
    from promptcache_amd import CacheEngine
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    shape = dataclasses.replace(SHAPES[name], num_hidden_layers=layers, name=f"{name}{layers}")
    w16 = make_weights_np(shape, seed, 2.0)
    lm = Llama2(name=shape.name, shape=shape, weights=w16, device=DEV, **kw)
    schema, prompts = _prompts(lm, PICKS + [((0, 0), 6)])
    eng = CacheEngine(MAX_CTX, lm, slots=4)
    eng.add_schema(schema)
    assert lm.hf_model.slot_loop_available() and lm.hf_model.D == 128
    return shape, w16, lm, eng, prompts, schema


@pytest.fixture(scope="module")
def mid4():
    return _build("mid", 4, 13)


def _images(loop, slot):
    """(codes, scale) [L][2][Hkv][qcap][D] / [L][2][Hkv][qcap] of the loop's image of slot index ``slot``, as on the device now."""
    m = loop.m
    c, s = q8.unpack(loop.kvq[slot].cpu().numpy(), m.L * 2 * m.Hkv, loop.qcap, m.D)
    return c.reshape(m.L, 2, m.Hkv, loop.qcap, m.D), s.reshape(m.L, 2, m.Hkv, loop.qcap)


def _assert_image_is_the_quantised_arena(loop, k, rows, what):
    """Image rows [0, rows) of sequence k's slot == kv_q8_ref.quantise of its fp16 arena rows, bit for bit."""
    a = loop.arenas[k]
    c, s = _images(loop, loop.idx[k])
    wc, ws = q8.quantise(a.buf[0, :, :, :, :rows].cpu().numpy())
    assert np.array_equal(c[:, :, :, :rows], wc), f"{what}: sequence {k}, codes of image rows [0, {rows}) differ from the quantised arena"
    assert np.array_equal(s[:, :, :, :rows].view(np.uint32), ws.view(np.uint32)), f"{what}: sequence {k}, scales differ"
    return c, s


def test_int8_slot_loop_against_the_oracle_on_the_devices_image_and_image_consistency(mid4):
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    shape, w16, lm, eng, prompts, _ = mid4
    m = lm.hf_model
    steps = 8
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    model = LlamaOracle(cfg, {k: v.astype(np.float32) for k, v in w16.items()})
    pasts, toks, poss, lens = [], [], [], []
    for k in range(4):
        ids, pos, out = _prefill(lm, eng, prompts[k], k)
        pasts.append(out.past_key_values)
        toks.append(int(torch.argmax(out.logits[0, -1])))            # the device leads from the first token on
        poss.append(max(pos) + 2)
        lens.append(out.past_key_values.arena.length)
    assert len(set(lens)) == 4, lens                                  # ragged slots
    loop = m.slot_loop(pasts, toks, poss, steps + 1, kv="int8")
    assert loop is not None and loop.S == 4 and loop.kv == "int8" and loop.qcap >= max(a.cap for a in loop.arenas)
    worst = 0.0
    try:
        for i in range(steps):
            torch.cuda.synchronize()
            past = []
            for k in range(4):                                        # what the step is about to read: the DEVICE's image rows
                c, s = _assert_image_is_the_quantised_arena(loop, k, lens[k] + i, f"before step {i}")
                n = lens[k] + i
                deq = c[:, :, :, :n].astype(np.float32) * s[:, :, :, :n, None]
                past.append([(deq[l, 0][None], deq[l, 1][None]) for l in range(shape.num_hidden_layers)])
            loop.enqueue()
            torch.cuda.synchronize()
            dev_logits = loop.logits.cpu().numpy()
            for k in range(4):
                olog, _ = model.forward(np.array([[toks[k]]]), np.array([[poss[k]]]), past=past[k])      # (+ its own exact new row)
                err = float(np.abs(dev_logits[k] - olog[0, -1]).max())
                worst = max(worst, err)
                assert err < LOGIT_TOL, (i, k, err)
                tok = loop.token(k, i)
                assert tok == int(np.argmax(dev_logits[k])), (i, k)
                toks[k], poss[k] = tok, poss[k] + 1
        for k in range(4):
            _assert_image_is_the_quantised_arena(loop, k, lens[k] + steps, "after the last step")
    finally:
        loop.close([steps] * 4)
    print(f"[mid, 4 layers] SlotLoop(kv='int8'), 4 ragged slots, {steps} steps, oracle fed the device's dequantised image rows and "
          f"tokens: max|dlogit| = {worst:.2e}")
    for k in range(4):
        assert loop.arenas[k].length == lens[k] + steps


def _invariance(lm, eng, prompts, steps=16):
    """Sequence 0 alone at slot index 3 of 4, and among three busy slots at index 2: tokens, logits and image rows."""
    m = lm.hf_model
    snap = []
    for k in range(4):
        ids, pos, out = _prefill(lm, eng, prompts[k], k)
        a = out.past_key_values.arena
        snap.append((out.past_key_values, a.buf[:, :, :, :, :a.length].clone(), a.length, int(torch.argmax(out.logits[0, -1])), max(pos) + 2))

    def run(which, slot_index):
        pasts, toks, poss = [], [], []
        for k in which:
            past, rows0, n0, tok, p0 = snap[k]
            past.arena.buf[:, :, :, :, :n0].copy_(rows0)
            past.arena.length = n0
            pasts.append(past)
            toks.append(tok)
            poss.append(p0)
        j = which.index(0)
        loop = m.slot_loop(pasts, toks, poss, steps + 1, slots=4, slot_index=slot_index, kv="int8")
        rows, tokens = [], [toks[j]]
        try:
            for i in range(steps):
                loop.enqueue()
                torch.cuda.synchronize()
                rows.append(loop.logits[slot_index[j]].clone())
                tokens.append(loop.token(j, i))
            n = snap[0][2] + steps
            c, s = _images(loop, slot_index[j])
            img = (c[:, :, :, :n].copy(), s[:, :, :, :n].copy().view(np.uint32))
        finally:
            loop.close([steps] * len(which))
        return torch.stack(rows), tokens, img

    solo = run([0], [3])
    crowd = run([0, 1, 2, 3], [2, 0, 1, 3])
    assert None not in solo[1] and solo[1] == crowd[1]
    bad = [i for i in range(steps) if not torch.equal(solo[0][i].view(torch.int32), crowd[0][i].view(torch.int32))]
    assert not bad, f"logits rows differ at steps {bad[:8]} ({len(bad)} of {steps})"
    assert np.array_equal(solo[2][0], crowd[2][0]) and np.array_equal(solo[2][1], crowd[2][1]), "image rows differ"


def test_int8_slot_loop_is_slot_invariant_over_16_steps(mid4):
    _, _, lm, eng, prompts, _ = mid4
    _invariance(lm, eng, prompts)


def test_int8_slot_loop_is_slot_invariant_with_mxfp4_weights():
    _, _, lm, eng, prompts, _ = _build("mid64", 3, 9, weight_format="mxfp4")
    assert lm.hf_model.w4_stream
    _invariance(lm, eng, prompts)


def test_generate_batch_int8_equals_the_loop_stepped_by_hand_and_fp16_mode_is_untouched(mid4, monkeypatch):
    from promptcache_amd import _native
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    _, _, lm, eng, prompts, _ = mid4
    m = lm.hf_model
    ge = GenerationEngine(lm)
    max_new = 12
    params = GenerationParameters(temperature=0.0, max_new_tokens=max_new, stop_token_ids=[])
    pasts, toks, poss = [], [], []
    for k in range(4):
        ids, pos, out = _prefill(lm, eng, prompts[k], k)
        pasts.append(out.past_key_values); toks.append(int(torch.argmax(out.logits[0, -1]))); poss.append(max(pos) + 2)
    hand = [[t] for t in toks]
    loop = m.slot_loop(pasts, toks, poss, max_new - 1, kv="int8")
    for i in range(max_new - 1):
        loop.enqueue()
        for k in range(4):
            hand[k].append(loop.token(k, i))
    loop.close([max_new - 1] * 4)
    assert all(None not in h for h in hand)

    def batch(**kw):
        reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts[:4])]
        outs = _collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, **kw))
        for k in range(4):                                              # the arenas stay complete: prefill rows + decoded rows
            assert eng.slot_cache(k).arena.length == len(eng.slot_cache(k)) + len(reqs[k][0]) + max_new - 1
        return [outs[k][-1].new_text for k in range(4)]
    assert ge.batch_plan(4, params, slot_kv="int8") == (True, "one device loop over all sequences, K/V read from int8 images (slot_kv='int8')")
    assert batch(slot_kv="int8") == [lm.decode(h) for h in hand]
    monkeypatch.setenv("PC_SLOT_KV", "int8")
    assert batch() == [lm.decode(h) for h in hand]
    monkeypatch.delenv("PC_SLOT_KV")
    # fp16 mode: no call of the new entries, the tokens of the unparameterised call
    calls = []
    for name in ("attn_decode_slots_q8", "kv_quant_q8_rows"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    m._graphs.clear()                                                    # (a step captured earlier would hide the launches)
    plain = batch()
    assert batch(slot_kv="fp16") == plain and calls == []
    batch(slot_kv="int8")
    assert calls.count("kv_quant_q8_rows") == 4 and calls.count("attn_decode_slots_q8") == 2 * m.L      # (the eager pass + the capture)
    # refusals, before anything is asked of the model
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts[:4])]
    for kw, word in ((dict(lookup=3), "lookup"), (dict(share_trunk=True), "share_trunk")):
        with pytest.raises(ValueError, match=word):
            next(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, slot_kv="int8", **kw))
    with pytest.raises(ValueError, match="share_trunk"):
        m.slot_loop(pasts, toks, poss, 4, kv="int8", share_trunk=True)
    with pytest.raises(ValueError, match="must be one of"):
        m.slot_loop(pasts, toks, poss, 4, kv="fp8")


def test_serve_int8_gives_every_request_the_tokens_it_gets_alone(mid4, monkeypatch):
    from promptcache_amd import CacheEngine
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    from tests.test_gpu_serve import _snapshots
    _, _, lm, _, prompts, schema = mid4
    m = lm.hf_model
    eng = CacheEngine(MAX_CTX, lm, slots=2)
    eng.add_schema(schema)
    ge = GenerationEngine(lm)
    assert ge.serve_plan(slot_kv="int8")[1].endswith("K/V read from int8 images (slot_kv='int8')")
    budgets = [5, 12, 9, 7, 10]
    snaps, loops, retired = _snapshots(monkeypatch, m)
    reqs = [(p, GenerationParameters(temperature=0.0, max_new_tokens=mn)) for p, mn in zip(prompts, budgets)]
    outs = _collect(ge.serve(eng, iter(reqs), slot_kv="int8"))
    monkeypatch.undo()
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert sorted(outs) == list(range(5)) and len(snaps) == 5 and len(loops) == 1 and loops[0].kv == "int8"
    assert [len(tokens[r]) for r in range(5)] == budgets and m._live_loop is None
    starts = {t[1]: t[3] for t in ge.last_serve_trace if t[0] == "start"}
    assert starts[0] == 0 and starts[1] == 0 and all(starts[r] > 0 for r in (2, 3, 4))      # three were admitted into the running loop
    for k, length, len0, consumed in retired:                            # the fp16 arenas stay complete
        assert length == len0 + consumed
    for r in range(5):                                                   # alone, same slots and same capacity
        snap = snaps[r]
        a = eng.slot_cache(0).arena
        a.pending = None
        a.buf[:, :, :, :, :snap["n0"]].copy_(snap["rows"])
        a.length = snap["n0"]
        loop = m.slot_loop([a.views(snap["n0"])], [snap["token"]], [snap["position"]], snap["max_new"], snap["params"], [snap["seed"]],
                           [snap["history"]], snap["stop_ids"], slots=2, each=True, max_keys=eng.max_ctx_length, kv="int8")
        solo = [snap["token"]]
        try:
            for i in range(snap["max_new"]):
                loop.enqueue()
                t = loop.token(0, i)
                if t is None:
                    break
                solo.append(t)
        finally:
            loop.close({0: len(solo) - 1})
        assert tokens[r] == solo, r
        assert outs[r][-1].new_text == lm.decode(solo), r
