"""Batched decode over slots on the GPU: pc_rope_append_slots / pc_attn_decode_slots / pc_sample_advance_slots through the C-ABI
against tests/slots_ref.py and the existing B = 1 entries, slot invariance bit for bit, SlotLoop against the numpy oracle, and
GenerationEngine.generate_batch / CacheEngine(slots=...) end to end."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import engine_oracle as eo
from oracle import llama_oracle as orc
from tests import slots_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATT_TOL = 2e-4          # tests/test_gpu_baseline_sizes.py test_attention_at_baseline_sizes_vs_pinned_oracle: the small-q path vs attention_core
LOGIT_TOL = 1e-2        # tests/test_gpu_engine.py: the project's bar
MARGIN = 1e-4           # tests/test_gpu_sample.py: draws are compared where the reference's own decision is not a near-tie
SENT = 77.0             # sentinel of memory nothing may write


def _n():
    from promptcache_amd import _native
    _native.load()
    return _native


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


class Slots:
    """S slots with arenas [L][2][Hkv][cap][D] of their own (sentinel-filled, ``lens[b]`` random staged rows; None: idle)."""

    def __init__(self, rng, lens, caps, Hkv, D, L=2):
        self.S, self.L, self.Hkv, self.D = len(lens), L, Hkv, D
        self.lens = [0 if n is None else n for n in lens]
        self.live = [0 if n is None else 1 for n in lens]
        self.caps = list(caps)
        self.arenas = []
        for n, cap in zip(self.lens, self.caps):
            a = torch.full((L, 2, Hkv, cap, D), SENT, dtype=torch.float16, device=DEV)
            if n:
                kv = rng.standard_normal((L, 2, Hkv, n, D), dtype=np.float32)
                kv[:, 0] *= 0.7
                a[:, :, :, :n] = torch.from_numpy(kv.astype(np.float16)).to(DEV)
            self.arenas.append(a)
        self.kv_base = torch.tensor([a.data_ptr() for a in self.arenas], dtype=torch.int64, device=DEV)
        self.cap, self.len, self.livet = _i32(self.caps), _i32(self.lens), _i32(self.live)


def _rope_np(x, cs):
    """x [heads][D] fp32, cs [D/2][2]: q cos + rotate_half(q) sin in fp32."""
    half = x.shape[1] // 2
    c, s = cs[:, 0][None], cs[:, 1][None]
    lo, hi = x[:, :half], x[:, half:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=1).astype(np.float32)


def _append_and_attend(n, sl, qkv, pos, H, layer, nsplit, out=None):
    """One pc_rope_append_slots + pc_attn_decode_slots over ``sl``; -> (q_hi, q_lo, out_hi, out_lo, cs)."""
    S, Hkv, D = sl.S, sl.Hkv, sl.D
    cs = torch.empty((S, D // 2, 2), dtype=torch.float32, device=DEV)
    inv_freq = (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))).to(DEV)
    n.rope_table(_i32(pos), inv_freq, cs, S, D)
    qh = torch.full((S, H * D), SENT, dtype=torch.float16, device=DEV)
    ql = torch.full((S, H * D), SENT, dtype=torch.float16, device=DEV)
    n.rope_append_slots(qkv, qkv.shape[1], 0, qh, ql, H * D, cs, sl.kv_base, sl.cap, sl.len, sl.livet, S, layer, H, Hkv, D)
    ws = torch.empty(n.attn_decode_slots_workspace_bytes(S, H, D, nsplit) // 4, dtype=torch.float32, device=DEV)
    if out is None:
        out = (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
               torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
    n.attn_decode_slots(qh, ql, H * D, sl.kv_base, sl.cap, sl.len, sl.livet, S, layer, H, Hkv, D, 1.0 / np.sqrt(D), nsplit, ws, out)
    torch.cuda.synchronize()
    return qh, ql, out[0], out[1], cs


ATTN_CASES = [
    # H, Hkv, D, nsplit, lens (None: idle slot)
    (32, 32, 128, 4, [0, 1, 63, 64, 65, 255, 257, 1737, 8258, None, 5, None, 100, 64, 1000, 2]),       # S = 16, MHA, 32 heads
    (32, 32, 128, 8, [1737]),                                                                         # S = 1
    (4, 2, 128, 4, [1, 63, None, 64, 255, 257, None, 1737]),                                          # S = 8, mid_gqa's ratio
    (16, 2, 128, 32, [0, 8258, 65]),                                                                  # S = 3, 8 : 1
    (8, 1, 128, 1, [257, None, 1737]),                                                                # S = 3, MQA
    (8, 8, 64, 4, [0, 1, 63, 64, 65, 255, 257, 1737, 8258, None, 5, None, 100, 64, 1000, 2]),          # S = 16, D = 64
    (16, 2, 64, 2, [65, None, 0, 1737, 255, 64, 1, 8258]),                                            # S = 8, D = 64, 8 : 1
    (12, 1, 64, 5, [1737]),                                                                           # S = 1, D = 64, MQA, 12 heads = 8 + 4
]


@pytest.mark.parametrize("H,Hkv,D,nsplit,lens", ATTN_CASES)
def test_ragged_attention_and_append_vs_the_reference(H, Hkv, D, nsplit, lens):
    n = _n()
    rng = np.random.default_rng(H * 1000 + D + len(lens))
    S, layer = len(lens), 1
    caps = [(0 if m is None else m) + 1 + 3 * (b % 4) for b, m in enumerate(lens)]       # different capacities, some exactly len + 1
    sl = Slots(rng, lens, caps, Hkv, D)
    before = [a.clone() for a in sl.arenas]
    W = (H + 2 * Hkv) * D
    qkv_np = rng.standard_normal((S, W), dtype=np.float32)
    qkv_np[:, H * D:(H + Hkv) * D] *= 0.7
    pos = [int(p) for p in rng.integers(0, 4000, S)]
    qh, ql, oh, ol, cs = _append_and_attend(n, sl, torch.from_numpy(qkv_np).to(DEV), pos, H, layer, nsplit)
    got = (n.from_act_frags(oh, S).float() + n.from_act_frags(ol, S).float()).cpu().numpy()
    raw = n.from_act_frags(oh, S).cpu().numpy()
    cs_np = cs.cpu().numpy()
    worst = 0.0
    for b, m in enumerate(lens):
        a, a0 = sl.arenas[b], before[b]
        if m is None:
            assert np.all(raw[b] == SENT) and torch.all(qh[b] == SENT), f"idle slot {b} was written"
            assert torch.equal(a, a0)
            continue
        # every arena byte outside the appended row of this layer is unchanged
        keep = torch.ones_like(a, dtype=torch.bool)
        keep[layer, :, :, m] = False
        assert torch.equal(a[keep], a0[keep]), f"slot {b}: bytes outside the appended row changed"
        q = _rope_np(qkv_np[b, :H * D].reshape(H, D), cs_np[b])
        q_dev = (qh[b].float() + ql[b].float()).cpu().numpy().reshape(H, D)
        assert np.abs(q_dev - q).max() < 1e-5
        k = a[layer, 0, :, :m + 1].float().cpu().numpy()
        v = a[layer, 1, :, :m + 1].float().cpu().numpy()
        k_new = _rope_np(qkv_np[b, H * D:(H + Hkv) * D].reshape(Hkv, D), cs_np[b])
        assert np.abs(k[:, m] - k_new).max() < 4e-3 and np.array_equal(v[:, m], qkv_np[b, (H + Hkv) * D:].reshape(Hkv, D).astype(np.float16).astype(np.float32))
        want = ref.attend_slot(q, k, v).reshape(H * D)
        core = orc.attention_core(q[None, :, None, :], k[None], v[None], m, H // Hkv)[0, :, 0, :].reshape(H * D)
        err = max(float(np.abs(got[b] - want).max()), float(np.abs(got[b] - core).max()))
        worst = max(worst, err)
        print(f"[slots attention H={H} Hkv={Hkv} D={D} nsplit={nsplit}] slot {b}: {m} + 1 keys, max|d| = {err:.2e}")
        assert np.isfinite(got[b]).all() and err < ATT_TOL, (b, m, err)
    print(f"[slots attention H={H} Hkv={Hkv} D={D} S={S}] worst max|d| = {worst:.2e}")


def _solo_vs_crowd(n, rng, H, Hkv, D, nsplit, m, slot_a, slot_b):
    """The same sequence (m staged rows) alone at ``slot_a`` of 8 and among seven busy slots at ``slot_b``."""
    W = (H + 2 * Hkv) * D
    row = rng.standard_normal((W,), dtype=np.float32)
    staged = rng.standard_normal((2, 2, Hkv, m, D), dtype=np.float32).astype(np.float16)
    res = []
    for slot, others in ((slot_a, None), (slot_b, [300, 1, 2000, 64, 777, 65, 1200])):
        lens = [None] * 8 if others is None else list(others[:slot]) + [m] + list(others[slot:])
        lens[slot] = m
        caps = [(0 if x is None else x) + 9 + b for b, x in enumerate(lens)]
        caps[slot] = m + 5                                     # the sequence's own arena has the same shape in both runs
        sl = Slots(rng, lens, caps, Hkv, D)
        sl.arenas[slot][:, :, :, :m] = torch.from_numpy(staged).to(DEV)
        qkv = rng.standard_normal((8, W), dtype=np.float32)
        qkv[slot] = row
        pos = [int(p) for p in rng.integers(0, 4000, 8)]
        pos[slot] = 1234
        qh, ql, oh, ol, _ = _append_and_attend(n, sl, torch.from_numpy(qkv).to(DEV), pos, H, 1, nsplit)
        res.append((n.from_act_frags(oh, 8)[slot].clone(), n.from_act_frags(ol, 8)[slot].clone(), qh[slot].clone(), ql[slot].clone(),
                    sl.arenas[slot][1, :, :, m].clone()))
    return res


@pytest.mark.parametrize("H,Hkv,D,nsplit,m", [(32, 32, 128, 4, 1737), (4, 2, 128, 8, 8258), (8, 1, 64, 2, 257)])
def test_kernels_are_slot_invariant_bit_for_bit(H, Hkv, D, nsplit, m):
    n = _n()
    solo, crowd = _solo_vs_crowd(n, np.random.default_rng(m), H, Hkv, D, nsplit, m, 2, 5)
    for x, y, what in zip(solo, crowd, ("out hi", "out lo", "q hi", "q lo", "appended K / V row")):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), what


def _append_ex(n, qkv_row, cs_row, arena, layer, H, Hkv, D, past, cap):
    """pc_rope_append_ex, B = 1, one token: the existing entry the slot kernel must reproduce."""
    qo = torch.empty((1, H * D), dtype=torch.float16, device=DEV)
    qol = torch.empty((1, H * D), dtype=torch.float16, device=DEV)
    q, k, v = qkv_row[:H * D], qkv_row[H * D:(H + Hkv) * D], qkv_row[(H + Hkv) * D:]
    W = qkv_row.numel()
    rc = n.load().pc_rope_append_ex(q.data_ptr(), W, W, qo.data_ptr(), qol.data_ptr(), H * D, H * D, k.data_ptr(), v.data_ptr(), W, W,
                                    arena[layer, 0].data_ptr(), arena[layer, 1].data_ptr(), arena.stride(0), cap * D,
                                    cs_row.data_ptr(), 1, H, Hkv, D, 1, past, cap, 1, None, None, None, 0, 0, 0, 0,
                                    torch.cuda.current_stream().cuda_stream)
    n.check(rc, "pc_rope_append_ex")
    return qo, qol


@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 128), (8, 2, 64)])
def test_appended_rows_equal_rope_append_ex_and_a_full_slot_is_left_alone(H, Hkv, D):
    n = _n()
    rng = np.random.default_rng(D)
    lens, caps = [10, 0, None, 33, 7], [40, 8, 16, 40, 7]               # slot 4: len == cap
    sl = Slots(rng, lens, caps, Hkv, D, L=3)
    twins = [a.clone() for a in sl.arenas]
    full_before = sl.arenas[4].clone()
    S, W, k_steps = 5, (H + 2 * Hkv) * D, 3
    inv_freq = (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))).to(DEV)
    for step in range(k_steps):
        pos = [int(p) for p in rng.integers(0, 3000, S)]
        cs = torch.empty((S, D // 2, 2), dtype=torch.float32, device=DEV)
        n.rope_table(_i32(pos), inv_freq, cs, S, D)
        for layer in range(3):
            qkv = torch.from_numpy(rng.standard_normal((S, W), dtype=np.float32)).to(DEV)
            qh = torch.zeros((S, H * D), dtype=torch.float16, device=DEV)
            ql = torch.zeros((S, H * D), dtype=torch.float16, device=DEV)
            n.rope_append_slots(qkv, W, 0, qh, ql, H * D, cs, sl.kv_base, sl.cap, sl.len, sl.livet, S, layer, H, Hkv, D)
            for b in (0, 1, 3):
                qo, qol = _append_ex(n, qkv[b], cs[b], twins[b], layer, H, Hkv, D, lens[b] + step, caps[b])
                assert torch.equal(qo[0].view(torch.int16), qh[b].view(torch.int16))
                assert torch.equal(qol[0].view(torch.int16), ql[b].view(torch.int16))
        sl.len += sl.livet * (sl.len < sl.cap).int()
    torch.cuda.synchronize()
    for b in (0, 1, 3):
        assert torch.equal(sl.arenas[b].view(torch.int16), twins[b].view(torch.int16)), b
        rows = sl.arenas[b][:, :, :, lens[b]:lens[b] + k_steps]
        assert not torch.any(rows == SENT)
    assert torch.equal(sl.arenas[2], twins[2]) and torch.equal(sl.arenas[4], full_before)
    # ... and the advance launch switches the full slot off without touching its words
    V = 1001
    st = _AdvState(S, V, lens=[int(x) for x in sl.len.cpu()], caps=caps, live=sl.live)
    st.set_params(0.0, 1.0, 1.0, -1)
    st.advance(torch.from_numpy(rng.standard_normal((S, V), dtype=np.float32)).to(DEV))
    torch.cuda.synchronize()
    assert st.live.cpu().tolist() == [1, 1, 0, 1, 0] and int(st.len[4]) == 7 and int(st.ctr[4]) == 0 and int(st.pos[4]) == 100


class _AdvState:
    """Device words of pc_sample_advance_slots."""

    def __init__(self, S, V, lens, caps, live, histories=None, budget=50, step=0, seeds=None, stop=(), ring=16):
        from promptcache_amd.model.llama_hip import _history_bits
        self.S, self.V, self.ring_cap = S, V, ring
        self.ids = torch.full((S,), -5, dtype=torch.int64, device=DEV)
        self.pos = torch.full((S,), 100, dtype=torch.int32, device=DEV)
        self.len, self.cap, self.live = _i32(lens), _i32(caps), _i32(live)
        self.budget = torch.full((S,), budget, dtype=torch.int32, device=DEV)
        self.ctr = torch.full((S,), step, dtype=torch.int32, device=DEV)
        self.ring = torch.full((S * ring,), -1, dtype=torch.int32, device=DEV)
        self.seeds = torch.tensor(seeds if seeds is not None else [0] * S, dtype=torch.int64, device=DEV)
        self.stop = _i32(list(stop) + [-1] * (8 - len(stop)))
        self.hist = torch.stack([_history_bits(h, V) for h in (histories or [()] * S)]).to(DEV)
        self.params = torch.zeros(24, dtype=torch.uint8, device=DEV)

    def set_params(self, T, rp, tp, tk):
        from promptcache_amd import _native
        self.params.copy_(torch.frombuffer(bytearray(_native.sample_params_bytes(T, rp, tp, tk, 0)), dtype=torch.uint8))

    def advance(self, logits, processed=None):
        from promptcache_amd import _native
        _native.sample_advance_slots(logits, logits.stride(0), self.V, self.params, self.seeds, self.hist, self.ids, self.pos, self.len,
                                     self.cap, self.live, self.budget, self.stop, self.ring, self.ctr, self.ring_cap, self.S, processed)


@pytest.mark.parametrize("V", [32000, 1001])
@pytest.mark.parametrize("T,rp,tp,tk", [(0.0, 1.0, 1.0, -1), (0.7, 1.1, 0.9, 40)])
def test_advance_equals_the_reference_per_slot(V, T, rp, tp, tk):
    from promptcache_amd.model.llama_hip import _history_bits
    rng = np.random.default_rng(V + int(T * 10))
    S, steps = 8, 6
    live0 = [1, 1, 0, 1, 1, 1, 0, 1]
    lens0, caps = [50 + 3 * b for b in range(S)], [1000] * S
    hists = [set(int(t) for t in rng.integers(b * (V // S), (b + 1) * (V // S), 30)) for b in range(S)]     # disjoint ranges per slot
    seeds = [int(s) for s in rng.integers(0, 2 ** 62, S)]
    x0 = (rng.standard_normal((S, V)) * 2.0).astype(np.float32)
    stop_tok = ref.advance_slot(dict(ids=0, pos=0, len=1, cap=9, live=1, budget=9, ctr=3, seed=seeds[3]), x0[3], set(hists[3]), T, rp, tp, tk, ())[0]
    st = _AdvState(S, V, lens0, caps, live0, histories=hists, budget=4, step=3, seeds=seeds, stop=(stop_tok,))
    st.set_params(T, rp, tp, tk)
    want = [dict(ids=-5, pos=100, len=lens0[b], cap=caps[b], live=live0[b], budget=4, ctr=3, seed=seeds[b]) for b in range(S)]
    whist = [set(h) for h in hists]
    checked = 0
    for step in range(steps):
        x = x0 if step == 0 else (rng.standard_normal((S, V)) * 2.0).astype(np.float32)
        buf = torch.full((S, V + 4), 7.0, dtype=torch.float32, device=DEV)              # (row stride V + 4)
        logits = buf[:, :V]
        logits.copy_(torch.from_numpy(x))
        proc = torch.full((S, V), SENT, dtype=torch.float32, device=DEV)
        was_live = [w["live"] for w in want]
        st.advance(logits, proc)
        torch.cuda.synchronize()
        ids, pos, ln, live, bud, ctr = (t.cpu().tolist() for t in (st.ids, st.pos, st.len, st.live, st.budget, st.ctr))
        proc = proc.cpu().numpy()
        for b in range(S):
            tok, margin, wproc = ref.advance_slot(want[b], x[b], whist[b], T, rp, tp, tk, (stop_tok,))
            if not was_live[b]:
                assert np.all(proc[b] == SENT)
                assert (ids[b], pos[b], ln[b], live[b], bud[b], ctr[b]) == tuple(want[b][k] for k in ("ids", "pos", "len", "live", "budget", "ctr")), (step, b)
                continue
            assert np.isfinite(proc[b][ids[b]])
            both = np.isfinite(proc[b]) & np.isfinite(wproc)
            assert np.array_equal(proc[b][both], wproc[both])                        # temperature and penalty are IEEE-exact
            if margin > MARGIN:
                assert ids[b] == tok, (step, b, ids[b], tok, margin)
                checked += 1
            else:                                                                     # follow the device through a near-tie
                whist[b].discard(tok); whist[b].add(ids[b]); want[b]["ids"] = ids[b]
                want[b]["live"] = int(not (ids[b] == stop_tok or want[b]["budget"] <= 0 or want[b]["len"] + 1 >= want[b]["cap"]))
            assert (pos[b], ln[b], live[b], bud[b], ctr[b]) == tuple(want[b][k] for k in ("pos", "len", "live", "budget", "ctr")), (step, b)
            assert int(st.ring[b * st.ring_cap + (ctr[b] - 1) % st.ring_cap]) == ids[b]
        if step == 0:
            assert live[3] == 0 and [live[b] for b in (0, 1, 4, 5, 7)] == [1] * 5          # the stop id ended exactly its slot
    assert checked >= 20, checked
    assert st.live.cpu().tolist() == [0] * S                                           # budget 4: everybody is done after 4 steps
    got_hist = st.hist.cpu()
    for b in range(S):                                                                 # histories do not leak between slots
        assert torch.equal(got_hist[b], _history_bits(sorted(whist[b]), V)), b


# ---- the model: SlotLoop --------------------------------------------------------------------------------------------------
def _mid_setup(layers, seed, slots, picks_qlens, max_ctx=2048):
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    shape = dataclasses.replace(SHAPES["mid"], num_hidden_layers=layers, name=f"mid{layers}")
    w16 = make_weights_np(shape, seed, 2.0)
    lm = Llama2(name=shape.name, shape=shape, weights=w16, device=DEV)
    traits = (("age", (30, 26, 33)), ("home", (41, 37, 44)))
    eng = CacheEngine(max_ctx, lm, slots=slots)
    prompts = []
    for pick, qlen in picks_qlens:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=traits, question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    eng.add_schema(lm.get_formatter()(sp))
    return shape, w16, lm, eng, prompts


def _prefill(lm, eng, prompt, slot):
    ids, pos, _, cache = eng.process(prompt, slot=slot)
    out = lm(input_ids=torch.tensor([ids], device=DEV), position_ids=torch.tensor([pos], device=DEV), past_key_values=cache,
             use_cache=True)
    return ids, pos, out


PICKS = [((0, 1), 8), ((1, 2), 6), ((2, 0), 11), ((1, 1), 3)]


def test_slot_loop_against_the_oracle_with_the_device_leading():
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    steps = 24
    shape, w16, lm, eng, prompts = _mid_setup(24, 13, 4, PICKS)
    m = lm.hf_model
    assert m.decode_tail is False and m.slot_loop_available()
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    model = LlamaOracle(cfg, {k: v.astype(np.float32) for k, v in w16.items()})
    sc = eng.get_schema("deep")
    jobs = []
    for p in sc.encode_paths():
        sf = sc.get_scaffold(p)
        jobs.append(dict(token_ids=sf.token_ids(), position_ids=sf.position_ids(), targets=sf.select(p).all_token_sequences()))
    lib = eo.encode_schema(model, jobs)
    pasts, toks, poss, presents, lens = [], [], [], [], []
    for k, prompt in enumerate(prompts):
        ids, pos, out = _prefill(lm, eng, prompt, k)
        used = [mm.token_sequence for mm in eng.slot_cache(k).staged]
        _, S, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        assert float(np.abs(out.logits[0, -1].cpu().numpy() - olog[0, -1]).max()) < LOGIT_TOL
        pasts.append(out.past_key_values)
        toks.append(int(torch.argmax(out.logits[0, -1])))            # the device leads from the first token on
        poss.append(max(pos) + 2)
        presents.append(present)
        lens.append(S + len(ids))
    assert len(set(lens)) == 4, lens                                  # ragged slots
    loop = m.slot_loop(pasts, toks, poss, steps + 1)
    assert loop is not None and loop.S == 4
    worst = 0.0
    try:
        for i in range(steps):
            loop.enqueue()
            torch.cuda.synchronize()
            dev_logits = loop.logits.cpu().numpy()
            for k in range(4):
                olog, presents[k] = model.forward(np.array([[toks[k]]]), np.array([[poss[k]]]), past=presents[k])
                err = float(np.abs(dev_logits[k] - olog[0, -1]).max())
                worst = max(worst, err)
                assert err < LOGIT_TOL, (i, k, err)
                tok = loop.token(k, i)
                assert tok == int(np.argmax(dev_logits[k])), (i, k)   # the device's token is the argmax of its own row
                toks[k], poss[k] = tok, poss[k] + 1
    finally:
        loop.close([steps] * 4)
    print(f"[24 layers] SlotLoop, 4 ragged slots, {steps} steps, oracle fed the device's tokens: max|dlogit| = {worst:.2e}")
    for k in range(4):
        assert loop.arenas[k].length == lens[k] + steps


def test_slot_loop_is_slot_invariant_over_32_steps():
    picks = PICKS + [((0, 0), 6), ((2, 2), 9), ((0, 2), 4), ((2, 1), 7)]
    shape, w16, lm, eng, prompts = _mid_setup(3, 9, 8, picks)
    m = lm.hf_model
    steps = 32

    # one B = 1 prefill per prompt; every run below restarts from a byte copy of the arenas it left, so that the runs differ in
    # nothing but the slots
    snap = []
    for k in range(8):
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
        a = pasts[j].arena
        start = a.buf[:, :, :, :, :a.length].clone()
        loop = m.slot_loop(pasts, toks, poss, steps + 1, slots=8, slot_index=slot_index)
        rows, tokens = [], [toks[j]]
        try:
            for i in range(steps):
                loop.enqueue()
                torch.cuda.synchronize()
                rows.append(loop.logits[slot_index[j]].clone())
                tokens.append(loop.token(j, i))
        finally:
            loop.close([steps] * len(which))
        a = loop.arenas[j]
        return torch.stack(rows), tokens, a.buf[:, :, :, :, :a.length].clone(), start

    solo = run([0], [3])                                                # alone, seven idle slots
    crowd = run(list(range(8)), [6, 0, 1, 2, 3, 4, 5, 7])               # among seven busy ones, at another index
    half = run([0, 1, 2], [0, 5, 7])                                    # ... and with some slots idle
    for other in (crowd, half):
        assert torch.equal(solo[3].view(torch.int16), other[3].view(torch.int16)), "the B = 1 prefills of the runs differ"
        assert solo[1] == other[1]
        bad = [i for i in range(steps) if not torch.equal(solo[0][i].view(torch.int32), other[0][i].view(torch.int32))]
        assert not bad, f"logits rows differ at steps {bad[:8]} ({len(bad)} of {steps})"
        assert torch.equal(solo[2].view(torch.int16), other[2].view(torch.int16))


def _collect(gen):
    outs = {}
    for k, o in gen:
        outs.setdefault(k, []).append(o)
    return outs


def test_generate_batch_equals_slot_loop_stepped_by_hand_and_generate():
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    shape, w16, lm, eng, prompts = _mid_setup(3, 9, 4, PICKS)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    max_new = 20
    params = GenerationParameters(temperature=0.0, max_new_tokens=max_new, stop_token_ids=[])
    # by hand
    pasts, toks, poss = [], [], []
    for k, p in enumerate(prompts):
        ids, pos, out = _prefill(lm, eng, p, k)
        pasts.append(out.past_key_values); toks.append(int(torch.argmax(out.logits[0, -1]))); poss.append(max(pos) + 2)
    hand = [[t] for t in toks]
    loop = m.slot_loop(pasts, toks, poss, max_new - 1)
    for i in range(max_new - 1):
        loop.enqueue()
        for k in range(4):
            hand[k].append(loop.token(k, i))
    loop.close([max_new - 1] * 4)
    assert all(None not in h for h in hand)
    # generate_batch
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
    outs = _collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params))
    for k in range(4):
        assert outs[k][-1].new_text == lm.decode(hand[k]), k
        assert len(outs[k]) == len([s for s in range(max_new) if s % 2 == 0 or s == max_new - 1]), k
        assert eng.slot_cache(k).arena.length == len(eng.slot_cache(k)) + len(reqs[k][0]) + max_new - 1
    # ... and per-prompt generate over slot 0 gives the same texts and the same number of Outputs
    for k, p in enumerate(prompts):
        ids, pos, _, cache = eng.process(p)
        single = list(ge.generate(ids, pos, params, cache))
        assert single[-1].new_text == outs[k][-1].new_text and len(single) == len(outs[k]), k
    # stop tokens that hit different sequences at different steps: the others run on to max_new_tokens
    stops = [hand[0][5], hand[2][11]]
    sp = GenerationParameters(temperature=0.0, max_new_tokens=max_new, stop_token_ids=stops)
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
    outs2 = _collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], sp))
    ended = 0
    for k, p in enumerate(prompts):
        cut = next((i for i, t in enumerate(hand[k]) if t in stops), max_new - 1)
        ended += cut < max_new - 1
        assert outs2[k][-1].new_text == lm.decode(hand[k][:cut + 1]), k
        ids, pos, _, cache = eng.process(p)
        single = list(ge.generate(ids, pos, sp, cache))                 # ends at the same token generate ends at
        assert single[-1].new_text == outs2[k][-1].new_text and len(single) == len(outs2[k]), k
    assert 2 <= ended < 4
    # a stop string ends its sequence only
    word = lm.decode(hand[1][7:9]).strip()
    if word and word not in lm.decode(hand[1][:7]):
        ss = GenerationParameters(temperature=0.0, max_new_tokens=max_new, stop_str=[word])
        reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
        outs3 = _collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], ss))
        for k, p in enumerate(prompts):
            ids, pos, _, cache = eng.process(p)
            single = list(ge.generate(ids, pos, ss, cache))
            assert [o.new_text for o in single] == [o.new_text for o in outs3[k]], k
    # sampled: reproducible under torch.manual_seed, one stream per sequence
    sm = GenerationParameters(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40, max_new_tokens=12)
    texts = []
    for _ in range(2):
        torch.manual_seed(5)
        reqs = [eng.process(prompts[0], slot=k) for k in range(4)]         # the same prompt four times
        o = _collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], sm))
        texts.append([o[k][-1].new_text for k in range(4)])
    assert texts[0] == texts[1] and len(set(texts[0])) > 1
    torch.manual_seed(5)
    ids, pos, _, cache = eng.process(prompts[0])
    assert list(ge.generate(ids, pos, sm, cache))[-1].new_text == texts[0][0]      # sequence 0 draws generate's stream


def test_abandoned_batch_generator_rewinds_every_arena_and_slots_do_not_disturb_each_other():
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    shape, w16, lm, eng, prompts = _mid_setup(3, 9, 2, PICKS[:2])
    ge = GenerationEngine(lm)
    params = GenerationParameters(temperature=0.0, max_new_tokens=16)
    # slot 0 alone, before slot 1 exists
    ids, pos, _, cache = eng.process(prompts[0])
    first = [o.new_text for o in ge.generate(ids, pos, params, cache)]
    assert eng._slot_caches[1] is None
    ids, pos, _, cache = eng.process(prompts[0])
    _ = cache[0][0]                                                     # (carry out the staging)
    a0 = eng.prompt_cache.arena
    staged0, len0 = a0.buf[:, :, :, :, :a0.length].clone(), a0.length
    eng.process(prompts[1], slot=1)
    _ = eng.slot_cache(1).cache[0][0]
    assert a0.length == len0 and torch.equal(a0.buf[:, :, :, :, :len0].view(torch.int16), staged0.view(torch.int16))
    assert [o.new_text for o in ge.generate(ids, pos, params, cache)] == first
    # abandon a batch at a yield
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts[:2])]
    gen = ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params)
    seen = {0: 0, 1: 0}
    for k, o in gen:
        seen[k] += 1
        if seen[0] >= 3 and seen[1] >= 3:
            break
    gen.close()
    assert lm.hf_model._live_loop is None
    # Outputs come at steps 0, 2, 4, ...: three Outputs of sequence k = tokens of steps 0..4 consumed at least
    for k in range(2):
        a = eng.slot_cache(k).arena
        used = a.length - (len(eng.slot_cache(k)) + len(reqs[k][0]))
        assert 4 <= used <= 5, (k, used)
    ids, pos, _, cache = eng.process(prompts[0])
    assert [o.new_text for o in ge.generate(ids, pos, params, cache)] == first


def test_generate_batch_falls_back_to_generate_where_no_slot_loop_exists():
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    from promptcache_amd.model import Falcon
    from promptcache_amd.model.config import FALCON_SHAPES
    from promptcache_amd.model.weights import make_falcon_weights_np
    shape = FALCON_SHAPES["falcon-mid"]
    lm = Falcon(name="falcon-mid", shape=shape, weights=make_falcon_weights_np(shape, 3, 2.0), device=DEV)
    ge = GenerationEngine(lm)
    params = GenerationParameters(temperature=0.0, max_new_tokens=8)
    assert not ge.batch_plan(2, params)[0]
    eng = CacheEngine(1024, lm, slots=2)
    prompts = []
    for pick, qlen in PICKS[:2]:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=(("age", (30, 26, 33)), ("home", (41, 37, 44))),
                                    question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    eng.add_schema(lm.get_formatter()(sp))
    want = []
    for p in prompts:
        ids, pos, _, cache = eng.process(p)
        want.append([o.new_text for o in ge.generate(ids, pos, params, cache)])
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
    outs = _collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params))
    assert [[o.new_text for o in outs[k]] for k in range(2)] == want
