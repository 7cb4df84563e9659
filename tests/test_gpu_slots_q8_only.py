"""The two entries of the int8-only slot residency on the GPU (csrc/pc_slots_q8.hip), through the C-ABI:
pc_rope_append_slots_q8 against pc_rope_append_slots into a scratch arena (q planes and fresh rows bit for bit) and against
tests/kv_q8_ref.py (image row len bit for bit), every other byte of images, fresh-row buffers and guards untouched;
pc_attn_decode_slots_q8_fresh against pc_attn_decode_slots_q8 bit for bit, with no image byte written; slot invariance bit for
bit; argument errors that leave every output alone."""
import numpy as np
import pytest
import torch

from tests import kv_q8_ref as q8
from tests.test_gpu_slots_q8 import DEV, F32, GB, GUARD, LAYER, SENT, D, L, Q8Slots, _i32, _n, _q, _split16

pytestmark = pytest.mark.gpu
QCAP = 1024
S = 3
DEAD = None
# (len, cap) per slot, three slots per launch: the issue's lengths, a dead slot, a slot with len = cap (below qcap), a slot with
# len >= qcap (its cap lies above: only the image bound stops it), and a short slot whose projection row holds an infinity
CASES = {
    "0/1/255": [(0, 1024), (1, 1024), (255, 1024)],
    "700/1022/dead": [(700, 1024), (1022, 1024), (DEAD, 1024)],
    "full/past-image/inf": [(512, 512), (1024, 2048), (5, 1024)],
}
INF_CASE, INF_SLOT = "full/past-image/inf", 2


class Fresh:
    """S fresh-row buffers [P][D] fp16 between one guard row on either side, and S images of QCAP rows per plane in the NaN-scale
    guard pattern (codes 0x55, scales NaN) between guard bytes."""

    def __init__(self, Hkv):
        self.Hkv, self.P = Hkv, L * 2 * Hkv
        self.bufs = [torch.full((self.P + 2, D), SENT, dtype=torch.float16, device=DEV) for _ in range(S)]
        self.kv_base = torch.tensor([t.data_ptr() + D * 2 for t in self.bufs], dtype=torch.int64, device=DEV)
        codes, scale = np.full((self.P, QCAP, D), 0x55, dtype=np.int8), np.full((self.P, QCAP), np.nan, dtype=F32)
        self.image0 = np.concatenate([np.full(GUARD, GB, np.uint8), q8.pack(codes, scale), np.full(GUARD, GB, np.uint8)])
        self.images = [torch.from_numpy(self.image0).to(DEV) for _ in range(S)]
        self.kvq_base = torch.tensor([t.data_ptr() + GUARD for t in self.images], dtype=torch.int64, device=DEV)

    def planes(self, b):
        """-> slot b's fresh rows [L][2][Hkv][D] as int16 bits, after checking its guard rows."""
        t = self.bufs[b].cpu()
        assert torch.all(t[0] == SENT) and torch.all(t[-1] == SENT), f"slot {b}: a guard row of the fresh-row buffer was written"
        return t[1:-1].view(torch.int16).numpy().reshape(L, 2, self.Hkv, D)

    def expected_image(self, b, new16=None, m=None):
        """The initial bytes, with row m of layer LAYER's planes replaced by the quantised ``new16`` [k|v][Hkv][D]."""
        img = self.image0.copy()
        if new16 is not None:
            c, s = q8.unpack(img[GUARD:-GUARD], self.P, QCAP, D)
            c, s = c.reshape(L, 2, self.Hkv, QCAP, D), s.reshape(L, 2, self.Hkv, QCAP)
            c[LAYER, :, :, m], s[LAYER, :, :, m] = q8.quantise(new16)
        return img


def _append_both(n, rng, H, Hkv, layout, spec, inf_slot=None):
    """pc_rope_append_slots into scratch arenas and pc_rope_append_slots_q8 on the same inputs -> everything both wrote."""
    W = (H + 2 * Hkv) * D
    qkv = rng.standard_normal((S, W), dtype=F32)
    if inf_slot is not None:
        qkv[inf_slot, (H + Hkv + Hkv - 1) * D + 77] = np.inf                       # V of the last kv head
    ang = rng.uniform(0, 6.28, (S, D // 2)).astype(F32)
    cs = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(F32)).to(DEV)
    qkv_t = torch.from_numpy(qkv).to(DEV)
    lens = [9 if m is DEAD else m for m, _ in spec]
    caps = [c for _, c in spec]
    live = [0 if m is DEAD else 1 for m, _ in spec]
    arenas = [torch.full((L, 2, Hkv, c, D), SENT, dtype=torch.float16, device=DEV) for c in caps]
    kv_base = torch.tensor([a.data_ptr() for a in arenas], dtype=torch.int64, device=DEV)
    cap_t, len_t, live_t = _i32(caps), _i32(lens), _i32(live)
    mk = lambda: torch.full((S, H * D), SENT, dtype=torch.float16, device=DEV)
    qh0, ql0, qh1, ql1 = mk(), mk(), mk(), mk()
    n.rope_append_slots(qkv_t, W, layout, qh0, ql0, H * D, cs, kv_base, cap_t, len_t, live_t, S, LAYER, H, Hkv, D)
    fr = Fresh(Hkv)
    n.rope_append_slots_q8(qkv_t, W, layout, qh1, ql1, H * D, cs, fr.kv_base, cap_t, len_t, live_t, S, LAYER, H, Hkv, D, fr.kvq_base,
                           QCAP, L)
    torch.cuda.synchronize()
    bits = lambda t: t.cpu().view(torch.int16).numpy()
    return dict(arenas=[bits(a) for a in arenas], q0=(bits(qh0), bits(ql0)), q1=(bits(qh1), bits(ql1)), fresh=fr, lens=lens, caps=caps,
                live=live)


SENT16 = int(np.float16(SENT).view(np.int16))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2)])
def test_append_vs_the_parent_and_the_quantiser(H, Hkv, layout, case):
    n = _n()
    rng = np.random.default_rng(H * 100 + Hkv * 10 + layout + len(case))
    r = _append_both(n, rng, H, Hkv, layout, CASES[case], INF_SLOT if case == INF_CASE else None)
    fr = r["fresh"]
    for b in range(S):
        m, c = r["lens"][b], r["caps"][b]
        runs = bool(r["live"][b]) and m < c and m < QCAP
        rows = fr.planes(b)
        img = fr.images[b].cpu().numpy()
        if not runs:
            assert np.all(r["q1"][0][b] == SENT16) and np.all(r["q1"][1][b] == SENT16), f"slot {b}: q rows of an idle slot were written"
            assert np.all(rows == SENT16), f"slot {b}: the fresh-row buffer of an idle slot was written"
            assert np.array_equal(img, fr.image0), f"slot {b}: the image of an idle slot was written"
            continue
        assert np.array_equal(r["q1"][0][b], r["q0"][0][b]) and np.array_equal(r["q1"][1][b], r["q0"][1][b]), f"slot {b}: q hi / lo rows differ"
        parent = r["arenas"][b][LAYER, :, :, m]                                  # [k|v][Hkv][D] bits the parent appended
        assert not np.all(parent == SENT16)
        assert np.array_equal(rows[LAYER], parent), f"slot {b} (len {m}): fresh K / V rows differ from the parent's arena row"
        assert np.all(np.delete(rows, LAYER, axis=0) == SENT16), f"slot {b}: a fresh row of another layer was written"
        want = fr.expected_image(b, parent.view(np.float16), m)
        diff = np.flatnonzero(img != want)
        assert diff.size == 0, f"slot {b} (len {m}): {diff.size} image bytes differ; first at byte {int(diff[0]) - GUARD}"
        if case == INF_CASE and b == INF_SLOT:
            codes, scale = q8.unpack(img[GUARD:-GUARD], fr.P, QCAP, D)
            codes, scale = codes.reshape(L, 2, Hkv, QCAP, D), scale.reshape(L, 2, Hkv, QCAP)
            assert np.isnan(scale[LAYER, 1, Hkv - 1, m]) and not codes[LAYER, 1, Hkv - 1, m].any()
            assert np.isfinite(scale[LAYER, 0, :, m]).all() and np.isfinite(scale[LAYER, 1, :Hkv - 1, m]).all()


@pytest.mark.parametrize("H,Hkv,layout,m", [(4, 4, 1, 700), (4, 2, 0, 255)])
def test_append_is_slot_invariant_bit_for_bit(H, Hkv, layout, m):
    """A slot alone at index 0, and at index 2 behind two busy slots: identical q rows, fresh rows and image row."""
    n = _n()
    res = []
    for slot, spec in ((0, [(m, 1024), (DEAD, 1024), (DEAD, 1024)]), (2, [(33, 1024), (1000, 1024), (m, 1024)])):
        rng = np.random.default_rng(m)
        W = (H + 2 * Hkv) * D
        qkv = rng.standard_normal((S, W), dtype=F32)
        ang = rng.uniform(0, 6.28, (S, D // 2)).astype(F32)
        own_row, own_ang = np.random.default_rng(7).standard_normal(W, dtype=F32), np.random.default_rng(8).uniform(0, 6.28, D // 2).astype(F32)
        qkv[slot], ang[slot] = own_row, own_ang
        cs = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(F32)).to(DEV)
        fr = Fresh(Hkv)
        qh = torch.full((S, H * D), SENT, dtype=torch.float16, device=DEV)
        ql = qh.clone()
        n.rope_append_slots_q8(torch.from_numpy(qkv).to(DEV), W, layout, qh, ql, H * D, cs, fr.kv_base, _i32([c for _, c in spec]),
                               _i32([9 if v is DEAD else v for v, _ in spec]), _i32([0 if v is DEAD else 1 for v, _ in spec]), S, LAYER, H,
                               Hkv, D, fr.kvq_base, QCAP, L)
        torch.cuda.synchronize()
        codes, scale = q8.unpack(fr.images[slot].cpu().numpy()[GUARD:-GUARD], fr.P, QCAP, D)
        res.append((qh[slot].cpu().view(torch.int16).numpy(), ql[slot].cpu().view(torch.int16).numpy(), fr.planes(slot)[LAYER].copy(),
                    codes.reshape(L, 2, Hkv, QCAP, D)[LAYER, :, :, m].copy(), scale.reshape(L, 2, Hkv, QCAP)[LAYER, :, :, m].view(np.uint32).copy()))
    for a, b, what in zip(res[0], res[1], ("q_hi", "q_lo", "fresh rows", "codes", "scales")):
        assert np.array_equal(a, b), what


# ---- the attention ---------------------------------------------------------------------------------------------------------------
def _attend_both(n, sl, q, H, nsplit):
    """pc_attn_decode_slots_q8 over arenas + images, and pc_attn_decode_slots_q8_fresh over fresh rows (the arenas' rows ``len``) +
    the same images' rows [0, len) -> the two pairs of output planes as bits, and the fresh leg's images."""
    Sn, Hkv = sl.S, sl.Hkv
    hi, lo = _split16(q.reshape(Sn, H * D))
    qh, ql = torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV)
    words = n.attn_decode_slots_workspace_bytes(Sn, H, D, nsplit) // 4
    fresh = []
    for b in range(Sn):
        f = torch.full((sl.P + 2, D), SENT, dtype=torch.float16, device=DEV)
        if sl.lens[b] < sl.caps[b]:
            f[1:-1] = sl.arenas[b][:, :, :, sl.lens[b]].reshape(sl.P, D)
        fresh.append(f)
    fresh_base = torch.tensor([f.data_ptr() + 2 * D for f in fresh], dtype=torch.int64, device=DEV)
    images1 = [torch.from_numpy(i).to(DEV) for i in sl.image0]
    kvq1 = torch.tensor([t.data_ptr() + GUARD for t in images1], dtype=torch.int64, device=DEV)
    outs = []
    for fresh_leg in (False, True):
        wsg = torch.full((words + 32,), SENT, dtype=torch.float32, device=DEV)
        out = (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
               torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
        args = (qh, ql, H * D, fresh_base if fresh_leg else sl.kv_base, sl.cap, sl.len, sl.livet, Sn, LAYER, H, Hkv, D, 1.0 / np.sqrt(D),
                nsplit, wsg[16:16 + words], out)
        if fresh_leg:
            n.attn_decode_slots_q8_fresh(*args, kvq1, sl.qcap, L)
        else:
            n.attn_decode_slots_q8(*args, sl.kvq_base, sl.qcap, L)
        torch.cuda.synchronize()
        assert torch.all(wsg[:16] == SENT) and torch.all(wsg[-16:] == SENT), "a guard word of the workspace was written"
        outs.append((out[0].cpu().view(torch.int16), out[1].cpu().view(torch.int16)))
    return outs[0], outs[1], [t.cpu().numpy() for t in images1]


@pytest.mark.parametrize("H,Hkv,nsplit", [(4, 4, 1), (4, 4, 4), (4, 2, 1), (4, 2, 4)])
def test_fresh_attention_equals_the_staging_entry_and_writes_no_image_byte(H, Hkv, nsplit):
    n = _n()
    rng = np.random.default_rng(H * 100 + Hkv * 10 + nsplit)
    lens = [0, 1, 255, 700, 1022, None, 512, 1024]                              # + dead, len = cap, len >= qcap
    caps = [1024] * 6 + [512, 2048]
    sl = Q8Slots(rng, lens, Hkv, QCAP, caps=caps)
    q = _q(rng, sl.S, H)
    parent, fresh, images1 = _attend_both(n, sl, q, H, nsplit)
    assert torch.equal(parent[0], fresh[0]) and torch.equal(parent[1], fresh[1]), "output planes differ from pc_attn_decode_slots_q8's"
    assert not torch.all(parent[0] == SENT16)
    staged = 0
    for b in range(sl.S):
        assert np.array_equal(images1[b], sl.image0[b]), f"slot {b}: the fresh entry wrote an image byte"
        staged += int(not np.array_equal(sl.images[b].cpu().numpy(), sl.image0[b]))
    assert staged == 5                                                           # (the parent staged row len of every running slot)


@pytest.mark.parametrize("H,Hkv,nsplit,m", [(4, 2, 4, 1022), (4, 4, 1, 255)])
def test_fresh_attention_is_slot_invariant_bit_for_bit(H, Hkv, nsplit, m):
    n = _n()
    rng = np.random.default_rng(m)
    own = rng.standard_normal((L, 2, Hkv, m + 1, D), dtype=F32).astype(np.float16)
    qrow = _q(rng, 1, H)[0]
    res = []
    for slot, others in ((0, None), (2, [300, 1000])):
        lens = [None] * S if others is None else list(others[:slot]) + [m] + list(others[slot:])
        lens[slot] = m
        rows = [None] * S
        rows[slot] = own
        sl = Q8Slots(rng, lens, Hkv, QCAP, rows=rows)
        q = _q(rng, S, H)
        q[slot] = qrow
        _, fresh, _ = _attend_both(n, sl, q, H, nsplit)
        res.append([n.from_act_frags(p.view(torch.float16).to(DEV), S)[slot].cpu().view(torch.int16) for p in fresh])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "output fragments differ"


def test_argument_errors_leave_the_outputs_untouched():
    n = _n()
    H, Hkv = 4, 2
    rng = np.random.default_rng(3)
    W = (H + 2 * Hkv) * D
    fr = Fresh(Hkv)
    qkv = torch.from_numpy(rng.standard_normal((S, W), dtype=F32)).to(DEV)
    cs = torch.zeros((S, D // 2, 2), dtype=torch.float32, device=DEV)
    qh = torch.full((S, H * D), SENT, dtype=torch.float16, device=DEV)
    ql = qh.clone()
    cap, ln, live = _i32([1024] * S), _i32([5, 6, 7]), _i32([1] * S)
    good = dict(qkv=qkv, ld=W, in_layout=1, q_hi=qh, q_lo=ql, q_ts=H * D, cs=cs, kv_base=fr.kv_base, cap=cap, length=ln, live=live, S=S,
                layer=LAYER, H=H, Hkv=Hkv, D=D, kvq_base=fr.kvq_base, qcap=QCAP, n_layers=L)
    for kw in (dict(D=64), dict(qcap=0), dict(layer=L), dict(n_layers=0), dict(in_layout=2), dict(S=17), dict(ld=W - 4), dict(q_ts=H * D + 4)):
        with pytest.raises(Exception, match="pc_rope_append_slots_q8"):
            n.rope_append_slots_q8(**{**good, **kw})
    words = n.attn_decode_slots_workspace_bytes(S, H, D, 2) // 4
    ws = torch.full((words,), SENT, dtype=torch.float32, device=DEV)
    out = (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
           torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
    agood = dict(q_hi=qh, q_lo=ql, q_ts=H * D, kv_base=fr.kv_base, cap=cap, length=ln, live=live, S=S, layer=LAYER, H=H, Hkv=Hkv, D=D,
                 softmax_scale=0.088, nsplit=2, workspace=ws, out_frag=out, kvq_base=fr.kvq_base, qcap=QCAP, n_layers=L)
    for kw in (dict(D=64), dict(qcap=0), dict(layer=L), dict(nsplit=33), dict(S=0), dict(workspace=ws[:-8]), dict(Hkv=3)):
        with pytest.raises(Exception, match="pc_attn_decode_slots_q8_fresh"):
            n.attn_decode_slots_q8_fresh(**{**agood, **kw})
    torch.cuda.synchronize()
    assert torch.all(qh == SENT) and torch.all(ql == SENT) and torch.all(ws == SENT) and torch.all(out[0] == SENT) and torch.all(out[1] == SENT)
    for b in range(S):
        assert torch.all(fr.bufs[b] == SENT) and np.array_equal(fr.images[b].cpu().numpy(), fr.image0)
    n.rope_append_slots_q8(**good)                                               # ... and the unmodified calls are accepted
    n.attn_decode_slots_q8_fresh(**agood)
    torch.cuda.synchronize()
    assert not torch.all(qh == SENT) and not torch.all(out[0] == SENT)
