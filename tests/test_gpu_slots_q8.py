"""The slot attention over int8 K / V images on the GPU (csrc/pc_slots_q8.hip): pc_attn_decode_slots_q8 through the
C-ABI against tests/slot_kv_q8_ref.py on the dequantised rows, the staged row bit for bit against tests/kv_q8_ref.py, everything
else of the images, their guards and the workspace guards untouched, slot invariance bit for bit, agreement with
pc_attn_decode_slots on rows on which the format is lossless, pc_kv_quant_q8_rows, and every argument error."""
import numpy as np
import pytest
import torch

from tests import kv_q8_ref as q8
from tests import slot_kv_q8_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATT_TOL = 2e-4          # tests/test_gpu_slots.py's bar for this kernel family, against the same kind of reference on identical inputs
SENT = 77.0             # sentinel of fp16 memory nothing may write
GUARD = 64              # guard bytes on both sides of every image
GB = 0xA5
D, L, LAYER, CAP = 128, 2, 1, 1024
F32 = np.float32


def _n():
    from promptcache_amd import _native
    _native.load()
    return _native


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _split16(x):
    hi = x.astype(np.float16)
    lo = (x - hi.astype(F32)).astype(np.float16)
    return hi, lo


class Q8Slots:
    """S slots: an fp16 arena [L][2][Hkv][cap][D] each (rows [0, len] random -- row len is the row "just appended" -- the rest a
    sentinel) and an int8 image of qcap rows per plane between guard bytes: rows [0, len) the quantised arena rows, rows at and
    behind len a NaN-scale pattern.  ``lens[b]`` None: a dead slot (live 0) that holds 9 rows.  ``rows[b]``: the slot's rows
    [L][2][Hkv][len + 1][D] fp16 instead of random ones."""

    def __init__(self, rng, lens, Hkv, qcap, caps=None, rows=None, lossless=False):
        self.S, self.Hkv, self.qcap, self.P = len(lens), Hkv, qcap, L * 2 * Hkv
        self.live = [0 if m is None else 1 for m in lens]
        self.lens = [9 if m is None else m for m in lens]
        self.caps = list(caps) if caps is not None else [CAP] * self.S
        self.arenas, self.images, self.image0, self.new16 = [], [], [], []
        nb = q8.image_bytes(self.P, qcap, D)
        for b, (m, cap) in enumerate(zip(self.lens, self.caps)):
            n_rows = min(m + 1, cap)
            if rows is not None and rows[b] is not None:
                kv16 = rows[b]
            elif lossless:
                kv16 = ref.lossless_rows(rng, (L, 2, Hkv, n_rows), D)[0]
            else:
                kv = rng.standard_normal((L, 2, Hkv, n_rows, D), dtype=F32)
                kv[:, 0] *= 0.7
                kv16 = kv.astype(np.float16)
            a = np.full((L, 2, Hkv, cap, D), SENT, dtype=np.float16)
            a[:, :, :, :n_rows] = kv16
            self.arenas.append(torch.from_numpy(a).to(DEV))
            self.new16.append(kv16[LAYER, :, :, m] if m < cap else None)       # [k|v][Hkv][D]
            codes = np.full((self.P, qcap, D), 0x55, dtype=np.int8)
            scale = np.full((self.P, qcap), np.nan, dtype=F32)
            keep = min(m, cap)
            c, s = q8.quantise(a[:, :, :, :keep].reshape(self.P, keep, D))
            codes[:, :keep], scale[:, :keep] = c, s
            img = np.concatenate([np.full(GUARD, GB, np.uint8), q8.pack(codes, scale), np.full(GUARD, GB, np.uint8)])
            assert img.size == nb + 2 * GUARD
            self.image0.append(img)
            self.images.append(torch.from_numpy(img).to(DEV))
        self.kv_base = torch.tensor([a.data_ptr() for a in self.arenas], dtype=torch.int64, device=DEV)
        self.kvq_base = torch.tensor([t.data_ptr() + GUARD for t in self.images], dtype=torch.int64, device=DEV)
        self.cap, self.len, self.livet = _i32(self.caps), _i32(self.lens), _i32(self.live)

    def image_planes(self, b):
        """(codes [L][2][Hkv][qcap][D], scale [L][2][Hkv][qcap]) of slot b as they are on the device now."""
        img = self.images[b].cpu().numpy()
        assert np.all(img[:GUARD] == GB) and np.all(img[-GUARD:] == GB), f"slot {b}: a guard of the image was written"
        c, s = q8.unpack(img[GUARD:-GUARD], self.P, self.qcap, D)
        return c.reshape(L, 2, self.Hkv, self.qcap, D), s.reshape(L, 2, self.Hkv, self.qcap)

    def expected_image(self, b, staged: bool):
        """Slot b's initial bytes, with row len of layer LAYER's planes replaced by the quantised new row where ``staged``."""
        img = self.image0[b].copy()
        if staged:
            c, s = q8.unpack(img[GUARD:-GUARD], self.P, self.qcap, D)
            c, s = c.reshape(L, 2, self.Hkv, self.qcap, D), s.reshape(L, 2, self.Hkv, self.qcap)
            c[LAYER, :, :, self.lens[b]], s[LAYER, :, :, self.lens[b]] = q8.quantise(self.new16[b])
        return img


def _attend(n, sl, q, H, nsplit, fp16_entry=False):
    """One pc_attn_decode_slots_q8 (or pc_attn_decode_slots) over ``sl`` with q [S][H][D] fp32 -> (out [S][H*D] fp32, hi, lo frags)."""
    S, Hkv = sl.S, sl.Hkv
    hi, lo = _split16(q.reshape(S, H * D))
    qh, ql = torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV)
    words = n.attn_decode_slots_workspace_bytes(S, H, D, nsplit) // 4
    wsg = torch.full((words + 32,), SENT, dtype=torch.float32, device=DEV)
    out = (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
           torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
    args = (qh, ql, H * D, sl.kv_base, sl.cap, sl.len, sl.livet, S, LAYER, H, Hkv, D, 1.0 / np.sqrt(D), nsplit, wsg[16:16 + words], out)
    if fp16_entry:
        n.attn_decode_slots(*args)
    else:
        n.attn_decode_slots_q8(*args, sl.kvq_base, sl.qcap, L)
    torch.cuda.synchronize()
    assert torch.all(wsg[:16] == SENT) and torch.all(wsg[-16:] == SENT), "a guard word of the workspace was written"
    got = (n.from_act_frags(out[0], S).float() + n.from_act_frags(out[1], S).float()).cpu().numpy()
    return got, out[0], out[1]


def _q(rng, S, H):
    return (rng.standard_normal((S, H, D), dtype=F32) * 0.5).astype(F32)


# live lens per split count (the issue's), then: a dead slot, a full slot (len = cap, left alone), len = cap - 1 (live), and a slot
# whose new K row holds an infinity (scale NaN, codes 0; its output is not compared)
LENS = {1: [0, 1, 255, 700], 4: [256, 257, 5, 1022]}
EXTRA = [None, CAP, CAP - 1, 3]
DEAD, FULL, LAST, INF = 4, 5, 6, 7


@pytest.mark.parametrize("H,Hkv,nsplit,qcap", [(4, 4, 1, 1024), (4, 4, 4, 1024), (4, 2, 1, 1024), (4, 2, 4, 1024), (4, 2, 4, 1536)])
def test_attention_and_staged_row_vs_the_references(H, Hkv, nsplit, qcap):
    n = _n()
    rng = np.random.default_rng(H * 100 + Hkv * 10 + nsplit + qcap)
    lens = LENS[nsplit] + EXTRA
    S = len(lens)
    rows = [None] * S
    inf_rows = rng.standard_normal((L, 2, Hkv, 4, D), dtype=F32).astype(np.float16)
    inf_rows[LAYER, 0, Hkv - 1, 3, 77] = np.inf
    rows[INF] = inf_rows
    sl = Q8Slots(rng, lens, Hkv, qcap, rows=rows)
    arenas0 = [a.clone() for a in sl.arenas]
    q = _q(rng, S, H)
    got, oh, _ = _attend(n, sl, q, H, nsplit)
    raw = n.from_act_frags(oh, S).cpu().numpy()
    worst = 0.0
    for b in range(S):
        assert torch.equal(sl.arenas[b].view(torch.int16), arenas0[b].view(torch.int16)), f"slot {b}: the fp16 arena was written"
        staged = b not in (DEAD, FULL)
        now = sl.images[b].cpu().numpy()
        want_img = sl.expected_image(b, staged)
        diff = np.flatnonzero(now != want_img)
        assert diff.size == 0, (f"slot {b} (len {sl.lens[b]}): {diff.size} image bytes differ from the initial image"
                                f"{' with the quantised row at len' if staged else ''}; first at byte {int(diff[0]) - GUARD}")
        if not staged:
            assert np.all(raw[b] == SENT), f"slot {b} (dead or full) was written"
            continue
        codes, scale = sl.image_planes(b)
        m = sl.lens[b]
        if b == INF:
            assert np.isnan(scale[LAYER, 0, Hkv - 1, m]) and not codes[LAYER, 0, Hkv - 1, m].any()
            assert np.isfinite(scale[LAYER, 1, :, m]).all() and np.isfinite(scale[LAYER, 0, :Hkv - 1, m]).all()
            continue
        want = ref.attend(q[b], codes[LAYER, 0, :, :m], scale[LAYER, 0, :, :m], codes[LAYER, 1, :, :m], scale[LAYER, 1, :, :m],
                          sl.new16[b][0], sl.new16[b][1]).reshape(H * D)
        err = float(np.abs(got[b] - want).max())
        worst = max(worst, err)
        print(f"[slots q8 H={H} Hkv={Hkv} nsplit={nsplit} qcap={qcap}] slot {b}: {m} + 1 keys, max|d| = {err:.2e}")
        assert np.isfinite(got[b]).all() and err < ATT_TOL, (b, m, err)
    print(f"[slots q8 H={H} Hkv={Hkv} nsplit={nsplit} qcap={qcap}] worst max|d| = {worst:.2e}")


@pytest.mark.parametrize("H,Hkv,nsplit,m", [(4, 4, 4, 1022), (4, 2, 1, 700), (4, 2, 4, 257)])
def test_kernel_is_slot_invariant_bit_for_bit(H, Hkv, nsplit, m):
    """A slot alone at index 2 of 8, and among seven busy slots at index 5: identical output fragments and image row."""
    n = _n()
    rng = np.random.default_rng(m)
    own = rng.standard_normal((L, 2, Hkv, m + 1, D), dtype=F32).astype(np.float16)
    qrow = _q(rng, 1, H)[0]
    res = []
    for slot, others in ((2, None), (5, [300, 1, 1000, 64, 777, 65, 900])):
        lens = [None] * 8 if others is None else list(others[:slot]) + [m] + list(others[slot:])
        lens[slot] = m
        rows = [None] * 8
        rows[slot] = own
        sl = Q8Slots(rng, lens, Hkv, 1024, rows=rows)
        q = _q(rng, 8, H)
        q[slot] = qrow
        _, oh, ol = _attend(n, sl, q, H, nsplit)
        codes, scale = sl.image_planes(slot)
        res.append((n.from_act_frags(oh, 8)[slot].clone().view(torch.int16), n.from_act_frags(ol, 8)[slot].clone().view(torch.int16),
                    codes[LAYER, :, :, m].copy(), scale[LAYER, :, :, m].copy().view(np.uint32)))
        assert np.array_equal(sl.images[slot].cpu().numpy(), sl.expected_image(slot, True))
    solo, crowd = res
    assert torch.equal(solo[0], crowd[0]) and torch.equal(solo[1], crowd[1]), "output fragments differ"
    assert np.array_equal(solo[2], crowd[2]) and np.array_equal(solo[3], crowd[3]), "the staged image row differs"


@pytest.mark.parametrize("H,Hkv,nsplit", [(4, 4, 1), (4, 2, 4)])
def test_lossless_rows_agree_with_the_fp16_entry(H, Hkv, nsplit):
    """On rows the format holds exactly, the image and the arena are the same numbers: the two entries differ by summation
    order only, each within ATT_TOL of the common reference."""
    n = _n()
    rng = np.random.default_rng(H + Hkv + nsplit)
    sl = Q8Slots(rng, LENS[nsplit], Hkv, 1024, lossless=True)
    q = _q(rng, sl.S, H)
    got8, _, _ = _attend(n, sl, q, H, nsplit)
    for b in range(sl.S):                                                # (the staged rows are exact too)
        assert np.array_equal(sl.images[b].cpu().numpy(), sl.expected_image(b, True))
    got16, _, _ = _attend(n, sl, q, H, nsplit, fp16_entry=True)
    err = float(np.abs(got8 - got16).max())
    print(f"[slots q8 lossless H={H} Hkv={Hkv} nsplit={nsplit}] max|q8 - fp16 entry| = {err:.2e}")
    assert np.isfinite(got8).all() and err < 2 * ATT_TOL


# ---- pc_kv_quant_q8_rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [0, 1, 77])
def test_kv_quant_q8_rows_between_two_plane_strides(n_rows):
    n = _n()
    rng = np.random.default_rng(n_rows)
    P, cap, qcap = 8, 1024, 1536
    src = (rng.standard_normal((P, cap, D), dtype=F32) * 3).astype(np.float16)
    if n_rows > 1:
        src[3, 5, 9] = np.inf
        src[2, 6] = 0
    nb = q8.image_bytes(P, qcap, D)
    codes0 = np.full((P, qcap, D), 0x55, dtype=np.int8)
    scale0 = np.full((P, qcap), np.nan, dtype=F32)
    img0 = np.concatenate([np.full(GUARD, GB, np.uint8), q8.pack(codes0, scale0), np.full(GUARD, GB, np.uint8)])
    img = torch.from_numpy(img0).to(DEV)
    n.kv_quant_q8_rows(torch.from_numpy(src).to(DEV), cap, n_rows, P, D, img[GUARD:GUARD + nb], qcap)
    torch.cuda.synchronize()
    want_c, want_s = codes0.copy(), scale0.copy()
    if n_rows:
        want_c[:, :n_rows], want_s[:, :n_rows] = q8.quantise(src[:, :n_rows])
    want = np.concatenate([img0[:GUARD], q8.pack(want_c, want_s), img0[-GUARD:]])
    assert np.array_equal(img.cpu().numpy(), want), "rows [0, n_rows) differ from the reference, or a byte outside them was written"


def test_kv_quant_q8_rows_with_equal_strides_is_kv_quant_q8():
    n = _n()
    rng = np.random.default_rng(3)
    P, rows = 6, 77
    src = torch.from_numpy((rng.standard_normal((P, rows, D), dtype=F32) * 2).astype(np.float16)).to(DEV)
    nb = q8.image_bytes(P, rows, D)
    a = torch.full((nb,), GB, dtype=torch.uint8, device=DEV)
    b = torch.full((nb,), GB, dtype=torch.uint8, device=DEV)
    n.kv_quant_q8(src, rows, P, D, a)
    n.kv_quant_q8_rows(src, rows, rows, P, D, b, rows)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    c, s = q8.quantise(src.cpu().numpy())
    assert np.array_equal(b.cpu().numpy(), q8.pack(c, s))


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_every_output_untouched():
    n = _n()
    rng = np.random.default_rng(11)
    H, Hkv, nsplit = 4, 2, 2
    sl = Q8Slots(rng, [5, 300], Hkv, 1024)
    S = sl.S
    hi, lo = _split16(_q(rng, S, H).reshape(S, H * D))
    qh, ql = torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV)
    ws = torch.full((n.attn_decode_slots_workspace_bytes(S, H, D, nsplit) // 4,), SENT, dtype=torch.float32, device=DEV)
    out = (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
           torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
    good = dict(q_hi=qh, q_lo=ql, q_ts=H * D, kv_base=sl.kv_base, cap=sl.cap, length=sl.len, live=sl.livet, S=S, layer=LAYER, H=H, Hkv=Hkv,
                D=D, softmax_scale=0.088, nsplit=nsplit, workspace=ws, out_frag=out, kvq_base=sl.kvq_base, qcap=1024, n_layers=L)
    null = torch.empty(0, dtype=torch.int32, device=DEV)                # data_ptr() == 0
    assert null.data_ptr() == 0
    cases = [dict(D=64), dict(H=3), dict(S=0), dict(S=17), dict(qcap=0), dict(nsplit=0), dict(nsplit=33), dict(workspace=ws[:-1]),
             dict(layer=L), dict(n_layers=0), dict(q_ts=H * D + 4), dict(kvq_base=null), dict(kv_base=null), dict(cap=null),
             dict(length=null), dict(live=null), dict(q_hi=null), dict(q_lo=null), dict(workspace=null), dict(out_frag=(null, out[1])),
             dict(out_frag=(out[0], null))]
    for kw in cases:
        with pytest.raises(RuntimeError, match="-1001"):
            n.attn_decode_slots_q8(**{**good, **kw})
    with pytest.raises(RuntimeError, match="-1001"):
        n.kv_quant_q8_rows(sl.arenas[0], CAP, 1025, sl.P, D, sl.images[0][GUARD:-GUARD], 1024)
    with pytest.raises(RuntimeError, match="-1001"):
        n.kv_quant_q8_rows(sl.arenas[0], CAP, 5, sl.P, 48, sl.images[0][GUARD:-GUARD], 1024)
    with pytest.raises(ValueError, match="too small"):
        n.kv_quant_q8_rows(sl.arenas[0], CAP, 5, sl.P, D, sl.images[0][GUARD:-GUARD - 4], 1024)
    torch.cuda.synchronize()
    assert torch.all(ws == SENT) and torch.all(out[0] == SENT) and torch.all(out[1] == SENT)
    for b in range(S):
        assert np.array_equal(sl.images[b].cpu().numpy(), sl.image0[b])
    n.attn_decode_slots_q8(**good)                                      # ... and the unmodified call is accepted
    torch.cuda.synchronize()
    assert not torch.any(n.from_act_frags(out[0], S) == SENT)
