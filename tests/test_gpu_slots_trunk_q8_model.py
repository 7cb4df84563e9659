"""Shared trunks over int8 K / V images in the model and the serving loop (LlamaHIP.slot_loop(each=True, kv="int8", trunks=...),
serve(slot_kv="int8", share_trunk=True)): the loop with trunks against the same loop without on the same rows, the
serve scenario of the fp16 shared trunk over images, MXFP4 weights, PC_TRUNK_VERIFY on arenas and on images, the mode off, and the
refusals on the real model."""
import pytest
import torch

from tests.test_gpu_slots import LOGIT_TOL, PICKS, _collect, _mid_setup, _prefill
from tests.test_gpu_slots_q8_model import _build

pytestmark = pytest.mark.gpu
STEPS = 16


@pytest.fixture
def trunk_env(monkeypatch):
    monkeypatch.setenv("PC_SLOT_TRUNK_MIN", "1")
    monkeypatch.setenv("PC_TRUNK_VERIFY", "1")
    for name in ("PC_SLOT_KV", "PC_SLOT_TRUNK", "PC_SLOT_KEEP_ARENAS", "PC_SERVE_LOOKUP"):
        monkeypatch.delenv(name, raising=False)


def _count(monkeypatch, names):
    from promptcache_amd import _native
    calls = []
    for name in names:
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    return calls


def _snap(lm, eng, prompts, n):
    snap = []
    for k in range(n):
        ids, pos, out = _prefill(lm, eng, prompts[k], k)
        a = out.past_key_values.arena
        snap.append((out.past_key_values, a.buf[:, :, :, :, :a.length].clone(), a.length, int(torch.argmax(out.logits[0, -1])), max(pos) + 2))
    return snap


def _restore(snap):
    for past, rows0, n0, _, _ in snap:
        past.arena.buf[:, :, :, :, :n0].copy_(rows0)
        past.arena.length = n0


def test_loop_with_trunks_against_the_loop_without_on_the_same_rows(trunk_env):
    """Four sequences over one schema; the two loops sum the same dequantised numbers in another order: the first step's logits
    within LOGIT_TOL, the tokens of all 16 steps equal.  Measured on MI355X: see DESIGN 3.33."""
    from promptcache_amd.model.kv_arena import common_trunks
    _, _, lm, eng, prompts = _mid_setup(3, 9, 4, PICKS)
    m = lm.hf_model
    assert m.slot_trunk_q8_available()
    snap = _snap(lm, eng, prompts, 4)
    trunks = common_trunks([s[0].arena.layout for s in snap])
    assert all(l == 0 for l, _ in trunks) and trunks[0][1] > 0, trunks
    T = trunks[0][1]
    assert all(T <= s[2] for s in snap)

    def run(tr):
        _restore(snap)
        loop = m.slot_loop([s[0] for s in snap], [s[3] for s in snap], [s[4] for s in snap], STEPS + 1, None, [0] * 4, [()] * 4, (),
                           slots=4, each=True, max_keys=eng.max_ctx_length, trunks=tr, kv="int8")
        assert loop.kv == "int8" and (loop.nsplit_trunk > 0) == (tr is not None)
        rows, toks = [], [[] for _ in range(4)]
        try:
            for i in range(STEPS):
                loop.enqueue()
                torch.cuda.synchronize()
                rows.append(loop.logits[:4].clone())
                for k in range(4):
                    toks[k].append(loop.token(k, i))
        finally:
            loop.close({k: STEPS for k in range(4)})
        return torch.stack(rows), toks, (loop.nsplit, loop.nsplit_trunk)
    shared, plain = run(trunks), run(None)
    assert shared[2][0] == plain[2][0]                                    # the same own split count: the same max_keys
    d0 = float((shared[0][0] - plain[0][0]).abs().max())
    top2 = torch.topk(plain[0], 2, dim=-1).values
    margin = float((top2[..., 0] - top2[..., 1]).min())
    dall = float((shared[0] - plain[0]).abs().max())
    print(f"[mid, 3 layers] slot_loop(each, int8) with trunks (T = {T}, splits own {shared[2][0]} / trunk {shared[2][1]}) vs without: "
          f"step 0 max|dlogit| = {d0:.2e}, all {STEPS} steps {dall:.2e}, smallest top-two margin of the unshared run = {margin:.2e}")
    assert d0 < LOGIT_TOL
    for k in range(4):
        assert None not in plain[1][k] and shared[1][k] == plain[1][k], (k, shared[1][k], plain[1][k])


def test_serve_int8_with_share_trunk_protects_the_leader_and_lets_a_request_join(trunk_env, monkeypatch):
    """tests/test_gpu_serve.py's shared-trunk scenario with slot_kv="int8": the tokens of the unshared int8 run."""
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    from tests.test_gpu_serve import _snapshots
    _, _, lm, eng, prompts = _mid_setup(3, 9, 3, PICKS)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    max_new = [4, 14, 16, 8]                                             # the leader (request 0, slot 0) ends first

    def reqs():
        return [(p, GenerationParameters(temperature=0.0, max_new_tokens=mn)) for p, mn in zip(prompts, max_new)]
    plain = _collect(ge.serve(eng, reqs(), slot_kv="int8"))
    plain_tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    snaps, loops, retired = _snapshots(monkeypatch, m)
    calls = _count(monkeypatch, ("attn_decode_slots_trunk_q8", "attn_decode_slots_q8", "attn_decode_slots_trunk"))
    m._graphs.clear()                                                    # (a step captured earlier would hide the launches)
    outs = _collect(ge.serve(eng, reqs(), slot_kv="int8", share_trunk=True))
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    trace = list(ge.last_serve_trace)
    loop = loops[0]
    assert loop.kv == "int8" and loop.nsplit_trunk > 0 and all(loop.trunks[k][0] == 0 for k in range(3))
    T = loop.trunks[0][1]
    assert loop.trunks[3] == (0, T)                                       # the fourth request joined the group
    assert calls.count("attn_decode_slots_trunk_q8") == 2 * m.L and set(calls) == {"attn_decode_slots_trunk_q8"}   # eager pass + capture
    assert any("trunk" in k and "q8" in k for k in m._graphs)
    # the leader's slot was held while members lived: request 3 went to another slot, slot 0 was freed after the last member
    assert ("hold", 0) in [t[:2] for t in trace]
    pull3 = next(t for t in trace if t[0] == "pull" and t[1] == 3)
    assert pull3[2] != 0
    pos = {(t[0], t[1]): j for j, t in enumerate(trace) if t[0] in ("hold", "free")}
    last_member_end = max(j for j, t in enumerate(trace) if t[0] == "finish" and t[1] in (1, 2, 3))
    assert pos[("hold", 0)] < pos[("free", 0)] and pos[("free", 0)] > last_member_end
    assert not any(t[0] == "pull" and t[2] == 0 and t[1] != 0 for t in trace)
    for r in range(4):
        assert tokens[r] == plain_tokens[r] and len(tokens[r]) == max_new[r], r
        assert outs[r][-1].new_text == plain[r][-1].new_text, r
    for k, length, len0, consumed in retired:                            # the fp16 arenas stay complete
        assert length == len0 + consumed
    # the environment spelling selects the same mode
    monkeypatch.setenv("PC_SLOT_KV", "int8")
    monkeypatch.setenv("PC_SLOT_TRUNK", "1")
    _collect(ge.serve(eng, reqs()))
    assert loops[-1].kv == "int8" and loops[-1].nsplit_trunk > 0
    assert {r: list(t) for r, t in ge.last_serve_tokens.items()} == tokens


def test_serve_int8_with_share_trunk_and_mxfp4_weights_gives_the_unshared_tokens(trunk_env):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    _, _, lm, eng, prompts, _ = _build("mid64", 3, 9, weight_format="mxfp4")
    assert lm.hf_model.w4_stream and lm.hf_model.slot_trunk_q8_available()
    ge = GenerationEngine(lm)
    max_new = [5, 12, 9, 7, 10]                                          # four slots: the fifth request joins the running loop

    def reqs():
        return [(p, GenerationParameters(temperature=0.0, max_new_tokens=mn)) for p, mn in zip(prompts, max_new)]
    _collect(ge.serve(eng, reqs(), slot_kv="int8"))
    plain = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    _collect(ge.serve(eng, reqs(), slot_kv="int8", share_trunk=True))
    shared = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert [len(plain[r]) for r in range(5)] == max_new and shared == plain
    assert any(k[0] == "slots" and "trunk" in k and "q8" in k for k in lm.hf_model._graphs)


def test_trunk_verify_catches_a_mismatch_in_the_arena_and_in_the_image(trunk_env):
    from promptcache_amd.model.kv_arena import common_trunks
    _, _, lm, eng, prompts = _mid_setup(3, 9, 2, PICKS[:2])
    m = lm.hf_model
    snap = _snap(lm, eng, prompts, 2)
    trunks = common_trunks([s[0].arena.layout for s in snap])
    T = trunks[1][1]
    assert trunks == [(0, T), (0, T)] and T > 3

    def build():
        return m.slot_loop([s[0] for s in snap], [s[3] for s in snap], [s[4] for s in snap], 4, None, [0, 0], [(), ()], (), slots=2,
                           each=True, max_keys=eng.max_ctx_length, trunks=trunks, kv="int8")
    # a member whose arena trunk rows were altered before entry
    cell = snap[1][0].arena.buf[0, 1, 1, 0, 3, 5:6]
    keep = cell.clone()
    cell.copy_(keep + 1.0)
    with pytest.raises(RuntimeError, match="PC_TRUNK_VERIFY.*slot 1"):
        build()
    cell.copy_(keep)
    _restore(snap)
    loop = build()                                                       # ... and equal rows pass, images included
    try:
        loop._trunk_verify_images(1, 0, T)
        s0 = m.L * 2 * m.Hkv * loop.qcap * m.D                           # where the image's scales start
        with torch.inference_mode():                                     # (the images are inference tensors)
            byte = loop.kvq[1][3 * m.D + 7: 3 * m.D + 8]                 # plane 0, row 3 < T: a code of the member's image
            byte.copy_(byte ^ 1)
            with pytest.raises(RuntimeError, match="PC_TRUNK_VERIFY: image rows.*slot 1"):
                loop._trunk_verify_images(1, 0, T)
            byte.copy_(byte ^ 1)
            loop._trunk_verify_images(1, 0, T)
            scale = loop.kvq[1][s0 + 4 * 2: s0 + 4 * 2 + 1]              # plane 0, the scale of row 2
            scale.copy_(scale ^ 1)
            with pytest.raises(RuntimeError, match="PC_TRUNK_VERIFY: image rows"):
                loop._trunk_verify_images(1, 0, T)
    finally:
        loop.close({0: 0, 1: 0})


def test_mode_off_launches_nothing_new_and_the_pair_stays_refused_elsewhere(trunk_env, monkeypatch):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    _, _, lm, eng, prompts = _mid_setup(3, 9, 3, PICKS)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    G = GenerationParameters
    reqs = lambda: [(p, G(temperature=0.0, max_new_tokens=4)) for p in prompts[:3]]
    calls = _count(monkeypatch, ("attn_decode_slots_trunk_q8",))
    m._graphs.clear()
    _collect(ge.serve(eng, reqs(), slot_kv="int8"))
    keys = [k for k in m._graphs if k[0] == "slots"]
    assert calls == [] and keys and all("trunk" not in k for k in keys)
    assert any(k[:2] == ("slots", 3) and k[3:5] == ("each", "q8") and len(k) == 6 for k in keys), keys      # today's key: (.., nsplit, "each", "q8", qcap)
    _collect(ge.serve(eng, reqs(), share_trunk=True))                    # the fp16 shared trunk: its own entry, not the new one
    assert calls == []
    # refusals on the real model, before anything is asked of it
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.serve(eng, reqs(), lookup=3, slot_kv="int8", share_trunk=True))
    with pytest.raises(ValueError, match="keep_arenas=False"):
        next(ge.serve(eng, reqs(), slot_kv="int8", share_trunk=True, keep_arenas=False))
    batch = [eng.process(p, slot=k) for k, p in enumerate(prompts[:3])]
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.generate_batch([(r[0], r[1], r[3]) for r in batch], G(temperature=0.0, max_new_tokens=4), slot_kv="int8", share_trunk=True))
    assert m._live_loop is None
