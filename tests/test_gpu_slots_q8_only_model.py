"""The batched slot loop without fp16 slot arenas on the GPU (LlamaHIP.slot_loop(kv="int8", keep_arenas=False)): four
ragged sequences prefilled in turn in ONE arena and admitted into an each=True loop, against the default int8 loop over four
arenas -- logits and images bit for bit, the shared arena overwritten with NaN --, with fp16 and with MXFP4 weights;
GenerationEngine.serve(slot_kv="int8", keep_arenas=False) against serve(slot_kv="int8"); a sequence whose image fills; and the
mode off launching neither new entry."""
import pytest
import torch

from tests.test_gpu_slots import _collect, _prefill
from tests.test_gpu_slots_q8_model import MAX_CTX, _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 8


@pytest.fixture(scope="module")
def mid4():
    return _build("mid", 4, 13)


def _image_rows(loop, slot, n):
    """Rows [0, n) of every plane of the loop's image of slot index ``slot``, on the device: (codes [P][n][D], scale bits [P][n])."""
    m = loop.m
    P, qcap, D = m.L * 2 * m.Hkv, loop.qcap, m.D
    img = loop.kvq[slot]
    codes = img[:P * qcap * D].view(P, qcap, D)[:, :n]
    scale = img[P * qcap * D:P * qcap * (D + 4)].view(torch.int32).view(P, qcap)[:, :n]
    return codes.clone(), scale.clone()


def _first(lm, eng, prompt, slot):
    ids, pos, out = _prefill(lm, eng, prompt, slot)
    return out.past_key_values, int(torch.argmax(out.logits[0, -1])), max(pos) + 2


def _steps(loop, lens):
    """STEPS replays -> per step (logits, image rows [0, len + step + 1) of every slot, tokens)."""
    got = []
    for i in range(STEPS):
        loop.enqueue()
        torch.cuda.synchronize()
        got.append((loop.logits.clone(), [_image_rows(loop, k, lens[k] + i + 1) for k in range(4)], [loop.token(k, i) for k in range(4)]))
    return got


def _one_arena_vs_four(lm, eng, prompts):
    """The staged layout of a prompt follows the modules' usage counters, so two prefills of one prompt need not leave the same
    rows: the four arenas of the reference loop are given the very rows the shared arena held when each sequence entered."""
    from promptcache_amd.model.llama_hip import SlotLoopQ8, SlotLoopQ8Only
    m = lm.hf_model
    common = dict(each=True, slots=4, max_keys=MAX_CTX, kv="int8")
    loop, entered = None, []
    for k in range(4):                                                                   # every prefill in slot 0's arena
        past, tok, pos = _first(lm, eng, prompts[k], 0)
        arena = past.arena
        entered.append((arena.buf[:, :, :, :, :arena.length].clone(), arena.length, tok, pos))
        if loop is None:
            loop = m.slot_loop([past], [tok], [pos], STEPS + 1, slot_index=[0], keep_arenas=False, **common)
            assert type(loop) is SlotLoopQ8Only
        else:
            assert loop.admit(k, past, tok, pos, STEPS + 1, None, 0, (), ()) == k
        del past
    lens = [e[1] for e in entered]
    assert len(set(lens)) == 4, lens                                                     # ragged
    try:
        assert all(a.buf is None for a in loop.arenas) and loop.n == 0
        images, qcap = sum(t.numel() for t in loop.kvq), loop.qcap
        assert loop.slot_kv_bytes() == images + 4 * m.L * 2 * m.Hkv * m.D * 2            # images + fresh rows: no arena counted
        with torch.inference_mode():
            arena.buf.view(torch.int16).fill_(0x7e00)                                    # NaN everywhere: nothing may read it
        got = _steps(loop, lens)
    finally:
        loop.close({k: STEPS for k in range(4)})
    assert m._live_loop is None and torch.all(arena.buf.view(torch.int16) == 0x7e00), "the shared arena was written"
    with torch.inference_mode():
        arena.buf.zero_()
        for t in loop.kvq:                                                               # (the loops of one model share their images)
            t.fill_(0x55)
    del loop

    pasts = []
    for k, (rows, n, _, _) in enumerate(entered):                                        # four arenas holding those rows
        a = _first(lm, eng, prompts[k], k)[0].arena
        with torch.inference_mode():
            a.pending = None
            a.buf[:, :, :, :, :n].copy_(rows)
            a.length = n
        pasts.append(a.views(n))
    ref = m.slot_loop(pasts, [e[2] for e in entered], [e[3] for e in entered], STEPS + 1, slot_index=[0, 1, 2, 3], **common)
    assert type(ref) is SlotLoopQ8 and ref.qcap == qcap
    try:
        assert ref.slot_kv_bytes() == images + 4 * arena.buf.numel() * 2
        want = _steps(ref, lens)
    finally:
        ref.close({k: STEPS for k in range(4)})
    for i in range(STEPS):
        (logits, rows, toks), (wlogits, wrows, wtoks) = got[i], want[i]
        bad = [k for k in range(4) if not torch.equal(logits[k].view(torch.int32), wlogits[k].view(torch.int32))]
        assert not bad, f"step {i}: logits rows of slots {bad} differ"
        assert toks == wtoks and None not in toks
        for k in range(4):
            assert torch.equal(rows[k][0], wrows[k][0]) and torch.equal(rows[k][1], wrows[k][1]), f"step {i}: image rows of slot {k} differ"


def test_one_shared_arena_equals_four_arenas_bit_for_bit(mid4):
    _, _, lm, eng, prompts, _ = mid4
    _one_arena_vs_four(lm, eng, prompts)


def test_one_shared_arena_equals_four_arenas_with_mxfp4_weights():
    _, _, lm, eng, prompts, _ = _build("mid64", 3, 9, weight_format="mxfp4")
    assert lm.hf_model.w4_stream
    _one_arena_vs_four(lm, eng, prompts)


def test_serve_without_arenas_gives_the_tokens_of_the_int8_mode(mid4, monkeypatch):
    from promptcache_amd import CacheEngine
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    _, _, lm, _, prompts, schema = mid4
    m = lm.hf_model
    ge = GenerationEngine(lm)
    budgets = [5, 12, 9, 7, 10]
    reqs = [(p, GenerationParameters(temperature=0.0, max_new_tokens=mn)) for p, mn in zip(prompts, budgets)]
    loops = []
    real = m.slot_loop
    monkeypatch.setattr(m, "slot_loop", lambda *a, **k: (loops.append(real(*a, **k)), loops[-1])[1])

    def run(**kw):
        eng = CacheEngine(MAX_CTX, lm, slots=2)
        eng.add_schema(schema)
        outs = _collect(ge.serve(eng, iter(reqs), slot_kv="int8", **kw))
        return eng, outs, {r: list(t) for r, t in ge.last_serve_tokens.items()}, list(ge.last_serve_trace)

    eng0, outs0, tokens0, trace0 = run()
    assert eng0._slot_caches[1] is not None and [len(tokens0[r]) for r in range(5)] == budgets
    eng1, outs1, tokens1, trace1 = run(keep_arenas=False)
    assert "keep_arenas=False" in ge.serve_plan(slot_kv="int8", keep_arenas=False)[1]
    for r in range(5):
        assert tokens1[r] == tokens0[r], r
        assert outs1[r][-1].new_text == outs0[r][-1].new_text, r
    assert trace1 == trace0                                                              # the scheduler saw the same run
    starts = {t[1]: t[3] for t in trace1 if t[0] == "start"}
    assert starts[0] == 0 and starts[1] == 0 and all(starts[r] > 0 for r in (2, 3, 4))   # three were admitted into the running loop
    assert eng1._slot_caches[1] is None                                                  # slot 1's buffer was never allocated
    assert len(loops) == 2 and type(loops[1]).__name__ == "SlotLoopQ8Only" and len(loops[1].arenas) == 5
    images = sum(t.numel() for t in loops[1].kvq)
    assert loops[1].slot_kv_bytes() == images + 2 * m.L * 2 * m.Hkv * m.D * 2            # images + fresh rows, no arena
    assert loops[0].slot_kv_bytes() == images + 2 * eng0.slot_cache(0).arena.buf.numel() * 2
    assert m._live_loop is None
    monkeypatch.setenv("PC_SLOT_KEEP_ARENAS", "0")                                       # the environment asks for the same mode
    eng2, _, tokens2, _ = run()
    assert tokens2 == tokens0 and eng2._slot_caches[1] is None and type(loops[2]).__name__ == "SlotLoopQ8Only"


def test_a_sequence_whose_image_fills_ends_like_one_whose_arena_is_full(mid4):
    _, _, lm, eng, prompts, _ = mid4
    m = lm.hf_model
    past, tok, pos = _first(lm, eng, prompts[0], 0)
    n0 = past.arena.length
    room = 6
    loop = m.slot_loop([past], [tok], [pos], 2, each=True, slots=8, slot_index=[5], max_keys=n0 + room, kv="int8", keep_arenas=False)
    assert loop.qcap == n0 + room
    try:
        for i in range(3):
            loop.enqueue()
        assert loop.token(0, 1) is not None and loop.token(0, 2) is None                 # (out of budget)
        loop.retire(0, 2)
        past, tok, pos = _first(lm, eng, prompts[0], 0)
        k = loop.admit(5, past, tok, pos, 50, None, 0, (), ())
        del past
        got = []
        for i in range(3, 3 + room + 2):
            loop.enqueue()
            got.append(loop.token(k, i))
        torch.cuda.synchronize()
        # pc_sample_advance_slots' rule with cap = qcap: the step that leaves len + 1 >= cap is the last one
        assert [t is not None for t in got] == [True] * (room - 1) + [False] * 3, got
        assert int(loop.st["live"][5]) == 0 and int(loop.st["len"][5]) == n0 + room - 1 and int(loop.st["cap"][5]) == loop.qcap
    finally:
        loop.close({})
    assert m._live_loop is None


def test_an_entering_sequence_with_more_rows_than_the_images_raises(mid4):
    _, _, lm, eng, prompts, _ = mid4
    m = lm.hf_model
    past, tok, pos = _first(lm, eng, prompts[3], 0)                                      # the shortest prompt sizes the images
    n3 = past.arena.length
    loop = m.slot_loop([past], [tok], [pos], 1, each=True, slots=16, slot_index=[0], kv="int8", keep_arenas=False)
    try:
        assert loop.qcap == n3 + 3
        past, tok, pos = _first(lm, eng, prompts[2], 0)
        assert past.arena.length > loop.qcap
        with pytest.raises(RuntimeError, match="int8 images"):
            loop.admit(1, past, tok, pos, 4, None, 0, (), ())
    finally:
        loop.close({})


def test_mode_off_launches_neither_new_entry(mid4, monkeypatch):
    from promptcache_amd import _native
    _, _, lm, eng, prompts, _ = mid4
    m = lm.hf_model
    calls = []
    for name in ("rope_append_slots_q8", "attn_decode_slots_q8_fresh"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    m._graphs.clear()                                                                    # (a step captured earlier would hide the launches)

    def step(**kw):
        past, tok, pos = _first(lm, eng, prompts[1], 0)
        loop = m.slot_loop([past], [tok], [pos], 3, each=True, slots=2, max_keys=MAX_CTX, **kw)
        try:
            loop.enqueue()
            return loop.token(0, 0)
        finally:
            loop.close({0: 1})
    step()
    t8 = step(kv="int8")
    assert calls == []
    assert step(kv="int8", keep_arenas=False) == t8
    assert calls.count("rope_append_slots_q8") == 2 * m.L and calls.count("attn_decode_slots_q8_fresh") == 2 * m.L    # eager pass + capture
