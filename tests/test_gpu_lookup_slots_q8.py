"""The two entries of the prompt-lookup step over int8 K / V images on the GPU (csrc/pc_slots_q8.hip), through the
C-ABI.  pc_rope_append_slots_rows_q8: q planes and fp16 rows bit for bit against pc_rope_append_slots_rows into a scratch arena
(both ``fresh`` values, both layouts), image rows len + i bit for bit against tests/kv_q8_ref.py, every other byte of images,
fresh-row buffers, arenas and guards untouched; at k = 0, fresh = 1 every byte is pc_rope_append_slots_q8's.
pc_attn_verify_slots_q8: against tests/lookup_slots_q8_ref.py on the dequantised rows, fresh = 0 / 1 bit-equal, no image byte
written, slot invariance bit for bit, agreement with pc_attn_decode_slots_q8 at k = 0, and argument errors that leave every
output alone."""
import functools

import numpy as np
import pytest
import torch

from tests import kv_q8_ref as q8
from tests import lookup_slots_q8_ref as ref
from tests.test_gpu_slots_q8 import DEV, F32, GB, GUARD, LAYER, SENT, D, L, _i32, _n, _split16

pytestmark = pytest.mark.gpu
ATT_TOL = 2e-4          # the bar of the slot attention kernels' tests, same kind of reference on identical inputs
CROSS_TOL = 4e-4        # two kernels with different summation orders, each within ATT_TOL of the reference
S, CAP = 3, 1024
SENT16 = int(np.float16(SENT).view(np.int16))
DEAD = None
HEADS = [(4, 4), (4, 2), (8, 1)]          # (8, 1): 8 query heads per kv head -- two 16-column passes at k = 3, four at k = 7


def cases(k, qcap):
    """name -> (nsplit, [(len, cap)] x S).  nsplit 1: 0 / 1 / 63 / 64 / 700 and a dead slot; nsplit 4: 255 / 256 / 257, the last
    length with room (cap - k - 1), one row more (no room: untouched everywhere), a short slot whose projection holds an infinity,
    and a slot whose arena has room and whose image has not (untouched everywhere)."""
    return {
        "n1a": (1, [(0, CAP), (1, CAP), (63, CAP)]),
        "n1b": (1, [(64, CAP), (700, CAP), (DEAD, CAP)]),
        "n4a": (4, [(255, CAP), (256, CAP), (257, CAP)]),
        "n4b": (4, [(CAP - k - 1, CAP), (CAP - k, CAP), (5, CAP)]),
        "n4c": (4, [(qcap - k, 2048), (300, CAP), (DEAD, CAP)]),
    }


INF_CASE, INF_SLOT = "n4b", 2
bits = lambda t: t.cpu().view(torch.int16).numpy()


class Step:
    """One step over S slots, run through every entry under test once; everything the launches wrote, as numpy.

    Per slot: an fp16 arena [L][2][Hkv][cap][D] (rows [0, len) random, a sentinel behind) and an image of ``qcap`` rows per plane
    between guard bytes -- rows [0, len) the quantised arena rows, every row at and behind len in a NaN-scale pattern (codes 0x55,
    scales NaN).  The parent (pc_rope_append_slots_rows) appends into a copy of the arenas; leg 0 (fresh = 0) appends into arenas
    and images of its own, leg 1 (fresh = 1) into fresh-row buffers [P][k + 1][D] between guard rows and images of its own; then
    each leg's attention runs over what its append left."""

    def __init__(self, H, Hkv, k, qcap, name, layout=1, spec=None, seed=0, qkv_rows=None, attend=True):
        n = _n()
        self.H, self.Hkv, self.k, self.qcap, self.P = H, Hkv, k, qcap, L * 2 * Hkv
        self.nsplit, spec = cases(k, qcap)[name] if spec is None else spec
        rng = np.random.default_rng(seed + H * 1000 + Hkv * 100 + k * 10 + qcap)
        R, W, P = S * (k + 1), (H + 2 * Hkv) * D, self.P
        self.lens = [9 if m is DEAD else m for m, _ in spec]
        self.caps = [c for _, c in spec]
        self.live = [0 if m is DEAD else 1 for m, _ in spec]
        self.runs = [bool(lv) and m + k + 1 <= c and m + k + 1 <= qcap for lv, m, c in zip(self.live, self.lens, self.caps)]
        qkv = rng.standard_normal((R, W), dtype=F32)
        qkv[:, :H * D] *= 0.5
        if qkv_rows is not None:                          # (slot index, rows [k + 1][W], angles [k + 1][D / 2])
            qkv[qkv_rows[0] * (k + 1):(qkv_rows[0] + 1) * (k + 1)] = qkv_rows[1]
        if name == INF_CASE:
            qkv[INF_SLOT * (k + 1), (H + 2 * Hkv - 1) * D + 77] = np.inf          # V of the last kv head, draft row 0
        ang = rng.uniform(0, 6.28, (R, D // 2)).astype(F32)
        if qkv_rows is not None:
            ang[qkv_rows[0] * (k + 1):(qkv_rows[0] + 1) * (k + 1)] = qkv_rows[2]
        cs = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(F32)).to(DEV)
        qkv_t = torch.from_numpy(qkv).to(DEV)
        self.arena0, self.image0 = [], []
        for b, (m, c) in enumerate(zip(self.lens, self.caps)):
            a = np.full((L, 2, Hkv, c, D), SENT, dtype=np.float16)
            rows_rng = np.random.default_rng(m * 7 + 1) if qkv_rows is not None and b == qkv_rows[0] else rng
            kv = rows_rng.standard_normal((L, 2, Hkv, m, D), dtype=F32)
            kv[:, 0] *= 0.7
            a[:, :, :, :m] = kv.astype(np.float16)
            codes, scale = np.full((P, qcap, D), 0x55, dtype=np.int8), np.full((P, qcap), np.nan, dtype=F32)
            keep = min(m, qcap)
            codes[:, :keep], scale[:, :keep] = q8.quantise(a[:, :, :, :keep].reshape(P, keep, D))
            self.arena0.append(a)
            self.image0.append(np.concatenate([np.full(GUARD, GB, np.uint8), q8.pack(codes, scale), np.full(GUARD, GB, np.uint8)]))
        up = lambda xs: [torch.from_numpy(x).to(DEV) for x in xs]
        base = lambda ts, off=0: torch.tensor([t.data_ptr() + off for t in ts], dtype=torch.int64, device=DEV)
        cap_t, len_t, live_t = _i32(self.caps), _i32(self.lens), _i32(self.live)
        words = (cap_t, len_t, live_t)
        mk = lambda: torch.full((R, H * D), SENT, dtype=torch.float16, device=DEV)
        # the parent
        par = up(self.arena0)
        qh0, ql0 = mk(), mk()
        n.rope_append_slots_rows(qkv_t, W, layout, qh0, ql0, H * D, cs, base(par), *words, S, k, LAYER, H, Hkv, D)
        self.parent, self.q0 = [bits(a) for a in par], (bits(qh0), bits(ql0))
        # the two legs
        self.legs = []
        for fresh in (0, 1):
            images = up(self.image0)
            kvq = base(images, GUARD)
            if fresh:
                store = [torch.full((P * (k + 1) + 2, D), SENT, dtype=torch.float16, device=DEV) for _ in range(S)]
                kvb = base(store, 2 * D)
            else:
                store = up(self.arena0)
                kvb = base(store)
            qh, ql = mk(), mk()
            n.rope_append_slots_rows_q8(qkv_t, W, layout, qh, ql, H * D, cs, kvb, *words, S, k, LAYER, H, Hkv, D, kvq, qcap, L, fresh)
            torch.cuda.synchronize()
            leg = dict(q=(bits(qh), bits(ql)), store=[bits(t) for t in store], images=[t.cpu().numpy() for t in images])
            if attend:
                nw = n.attn_verify_slots_q8_workspace_bytes(S, k, H, D, self.nsplit) // 4
                wsg = torch.full((nw + 32,), SENT, dtype=torch.float32, device=DEV)
                mt = (R + 15) // 16
                out = tuple(torch.full((mt, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV) for _ in range(2))
                n.attn_verify_slots_q8(qh, ql, H * D, kvb, *words, S, k, LAYER, H, Hkv, D, 1.0 / np.sqrt(D), self.nsplit, wsg[16:16 + nw],
                                       out, kvq, qcap, L, fresh)
                torch.cuda.synchronize()
                assert torch.all(wsg[:16] == SENT) and torch.all(wsg[-16:] == SENT), "a guard word of the workspace was written"
                leg["out_bits"] = (bits(n.from_act_frags(out[0], R)), bits(n.from_act_frags(out[1], R)))
                leg["out"] = (n.from_act_frags(out[0], R).float() + n.from_act_frags(out[1], R).float()).cpu().numpy()
                leg["images_after"] = [t.cpu().numpy() for t in images]
                if k == 0 and fresh:                  # the one-token kernel over the same images and fresh rows
                    nw1 = n.attn_decode_slots_workspace_bytes(S, H, D, self.nsplit) // 4
                    ws1 = torch.empty(nw1, dtype=torch.float32, device=DEV)
                    out1 = tuple(torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV) for _ in range(2))
                    n.attn_decode_slots_q8_fresh(qh, ql, H * D, kvb, *words, S, LAYER, H, Hkv, D, 1.0 / np.sqrt(D), self.nsplit, ws1, out1,
                                                 kvq, qcap, L)
                    torch.cuda.synchronize()
                    leg["decode"] = (n.from_act_frags(out1[0], S).float() + n.from_act_frags(out1[1], S).float()).cpu().numpy()
            self.legs.append(leg)
        self.qkv_t, self.cs, self.words, self.layout = qkv_t, cs, words, layout

    def new16(self, b):
        """The fp16 rows the parent appended for slot b: [2][Hkv][k + 1][D]."""
        m = self.lens[b]
        return self.parent[b][LAYER, :, :, m:m + self.k + 1].view(np.float16)

    def expected_image(self, b):
        img = self.image0[b].copy()
        if self.runs[b]:
            m = self.lens[b]
            c, s = q8.unpack(img[GUARD:-GUARD], self.P, self.qcap, D)
            c, s = c.reshape(L, 2, self.Hkv, self.qcap, D), s.reshape(L, 2, self.Hkv, self.qcap)
            c[LAYER, :, :, m:m + self.k + 1], s[LAYER, :, :, m:m + self.k + 1] = q8.quantise(self.new16(b))
        return img


@functools.lru_cache(maxsize=4)
def step(H, Hkv, k, qcap, name, layout=1):
    return Step(H, Hkv, k, qcap, name, layout)


GRID = [(H, Hkv, k, 1024, name) for H, Hkv in HEADS for k in (0, 3, 7) for name in ("n1a", "n1b", "n4a", "n4b")] + \
       [(4, 2, k, qcap, name) for k in (3, 7) for qcap, name in ((1536, "n4a"), (1536, "n4b"), (1024, "n4c"), (1536, "n4c"))]


def check_append(st):
    k, Hkv, P = st.k, st.Hkv, st.P
    for fresh, leg in enumerate(st.legs):
        for b in range(S):
            m, rows = st.lens[b], slice(b * (k + 1), (b + 1) * (k + 1))
            what = f"fresh {fresh}, slot {b} (len {m})"
            img = leg["images"][b]
            diff = np.flatnonzero(img != st.expected_image(b))
            assert diff.size == 0, f"{what}: {diff.size} image bytes differ; first at byte {int(diff[0]) - GUARD}"
            store = leg["store"][b]
            if fresh:
                assert np.all(store[0] == SENT16) and np.all(store[-1] == SENT16), f"{what}: a guard row of the fresh-row buffer was written"
                store = store[1:-1].reshape(L, 2, Hkv, k + 1, D)
            if not st.runs[b]:
                assert np.all(leg["q"][0][rows] == SENT16) and np.all(leg["q"][1][rows] == SENT16), f"{what}: q rows of an idle slot were written"
                assert np.all(store == SENT16) if fresh else np.array_equal(store, st.arena0[b].view(np.int16)), f"{what}: fp16 rows written"
                continue
            assert np.array_equal(leg["q"][0][rows], st.q0[0][rows]) and np.array_equal(leg["q"][1][rows], st.q0[1][rows]), f"{what}: q planes"
            new = st.new16(b).view(np.int16)
            assert not np.all(new == SENT16)
            if fresh:
                assert np.array_equal(store[LAYER], new), f"{what}: fresh K / V rows differ from the parent's arena rows"
                assert np.all(np.delete(store, LAYER, axis=0) == SENT16), f"{what}: a fresh row of another layer was written"
            else:
                assert np.array_equal(store, st.parent[b]), f"{what}: the arena differs from the parent's"


@pytest.mark.parametrize("H,Hkv,k,qcap,name", GRID)
def test_append_vs_the_parent_and_the_quantiser(H, Hkv, k, qcap, name):
    st = step(H, Hkv, k, qcap, name)
    check_append(st)
    if name == INF_CASE:
        c, s = q8.unpack(st.legs[0]["images"][INF_SLOT][GUARD:-GUARD], st.P, qcap, D)
        c, s = c.reshape(L, 2, Hkv, qcap, D), s.reshape(L, 2, Hkv, qcap)
        m = st.lens[INF_SLOT]
        assert np.isnan(s[LAYER, 1, Hkv - 1, m]) and not c[LAYER, 1, Hkv - 1, m].any()
        assert np.isfinite(s[LAYER, 0, :, m:m + k + 1]).all() and np.isfinite(s[LAYER, 1, :, m + 1:m + k + 1]).all()


@pytest.mark.parametrize("H,Hkv,k,name", [(4, 2, 3, "n4a"), (8, 1, 7, "n1b"), (4, 4, 0, "n4b")])
def test_append_in_the_natural_layout(H, Hkv, k, name):
    check_append(Step(H, Hkv, k, 1024, name, layout=0, attend=False))


@pytest.mark.parametrize("H,Hkv,layout,name", [(4, 4, 1, "n1b"), (4, 2, 0, "n4b"), (8, 1, 1, "n4a")])
def test_append_at_k0_fresh_is_the_one_row_entry_byte_for_byte(H, Hkv, layout, name):
    n = _n()
    st = Step(H, Hkv, 0, 1024, name, layout=layout, attend=False)
    W, P = (H + 2 * Hkv) * D, st.P
    images = [torch.from_numpy(x).to(DEV) for x in st.image0]
    store = [torch.full((P + 2, D), SENT, dtype=torch.float16, device=DEV) for _ in range(S)]
    ptr = lambda ts, off: torch.tensor([t.data_ptr() + off for t in ts], dtype=torch.int64, device=DEV)
    qh = torch.full((S, H * D), SENT, dtype=torch.float16, device=DEV)
    ql = qh.clone()
    n.rope_append_slots_q8(st.qkv_t, W, layout, qh, ql, H * D, st.cs, ptr(store, 2 * D), *st.words, S, LAYER, H, Hkv, D, ptr(images, GUARD),
                           1024, L)
    torch.cuda.synchronize()
    leg = st.legs[1]
    assert np.array_equal(bits(qh), leg["q"][0]) and np.array_equal(bits(ql), leg["q"][1])
    assert any(st.runs) and not np.all(bits(qh) == SENT16)
    for b in range(S):
        assert np.array_equal(bits(store[b]), leg["store"][b]), f"slot {b}: fresh-row buffers differ"
        assert np.array_equal(images[b].cpu().numpy(), leg["images"][b]), f"slot {b}: images differ"


def reference(st, b):
    """tests/lookup_slots_q8_ref.py for slot b on the q planes and the image the append left -> [k + 1][H * D]."""
    k, H, Hkv, m = st.k, st.H, st.Hkv, st.lens[b]
    leg = st.legs[0]
    rows = slice(b * (k + 1), (b + 1) * (k + 1))
    q = (leg["q"][0][rows].view(np.float16).astype(F32) + leg["q"][1][rows].view(np.float16).astype(F32)).reshape(k + 1, H, D)
    c, s = q8.unpack(leg["images"][b][GUARD:-GUARD], st.P, st.qcap, D)
    c, s = c.reshape(L, 2, Hkv, st.qcap, D)[LAYER], s.reshape(L, 2, Hkv, st.qcap)[LAYER]
    new = st.new16(b)
    return ref.verify_attend_q8(q, c[0], s[0], c[1], s[1], new[0], new[1], m, k).reshape(k + 1, H * D)


WORST = {}


@pytest.mark.parametrize("H,Hkv,k,qcap,name", GRID)
def test_attention_vs_the_reference(H, Hkv, k, qcap, name):
    st = step(H, Hkv, k, qcap, name)
    a, f = st.legs
    assert np.array_equal(a["out_bits"][0], f["out_bits"][0]) and np.array_equal(a["out_bits"][1], f["out_bits"][1]), \
        "fresh = 0 and fresh = 1 differ on equal rows"
    for leg in st.legs:
        for b in range(S):
            assert np.array_equal(leg["images_after"][b], leg["images"][b]), f"slot {b}: the attention wrote an image byte"
    worst = 0.0
    for b in range(S):
        rows = slice(b * (k + 1), (b + 1) * (k + 1))
        if not st.runs[b]:
            # (a slot its cap word lets run and its image does not is out of contract: the merge launch, which asks the cap word
            # only, leaves undefined output rows for it -- as in pc_attn_decode_slots_q8; images, arenas and q planes are checked)
            if not (st.live[b] and st.lens[b] + k + 1 <= st.caps[b]):
                assert np.all(a["out_bits"][0][rows] == SENT16) and np.all(a["out_bits"][1][rows] == SENT16), f"slot {b}: rows of an idle slot"
            continue
        if name == INF_CASE and b == INF_SLOT:
            continue                                  # (its V holds an infinity and a NaN-scale row: not compared)
        want = reference(st, b)
        assert np.isfinite(a["out"][rows]).all(), f"slot {b}: a masked NaN-scale row reached the output"
        err = float(np.abs(a["out"][rows] - want).max())
        print(f"H {H} Hkv {Hkv} k {k} qcap {qcap} {name} slot {b} len {st.lens[b]}: max |d| = {err:.3e}")
        worst = max(worst, err)
        assert err < ATT_TOL, (b, st.lens[b], err)
    WORST[(H, Hkv, k, qcap, name)] = worst
    print(f"worst so far: {max(WORST.values()):.3e}")


@pytest.mark.parametrize("H,Hkv,name", [(h, g, name) for h, g in HEADS for name in ("n1a", "n1b", "n4a")])
def test_k0_agrees_with_the_one_token_kernel(H, Hkv, name):
    st = step(H, Hkv, 0, 1024, name)
    leg = st.legs[1]
    for b in range(S):
        if st.runs[b]:
            err = float(np.abs(leg["out"][b] - leg["decode"][b]).max())
            print(f"H {H} Hkv {Hkv} {name} slot {b} len {st.lens[b]}: max |verify_q8 - decode_q8| = {err:.3e}")
            assert err < CROSS_TOL, (b, err)


@pytest.mark.parametrize("H,Hkv,k,nsplit,m", [(4, 2, 3, 4, 257), (8, 1, 7, 1, 63), (4, 4, 3, 4, CAP - 4)])
def test_a_slot_alone_and_among_busy_slots_is_bit_equal(H, Hkv, k, nsplit, m):
    W = (H + 2 * Hkv) * D
    own = np.random.default_rng(11)
    rows, ang = own.standard_normal((k + 1, W), dtype=F32), own.uniform(0, 6.28, (k + 1, D // 2)).astype(F32)
    res = []
    for slot, spec in ((0, [(m, CAP), (DEAD, CAP), (DEAD, CAP)]), (2, [(33, CAP), (900, CAP), (m, CAP)])):
        st = Step(H, Hkv, k, 1024, "", spec=(nsplit, spec), seed=slot, qkv_rows=(slot, rows, ang))
        sl = slice(slot * (k + 1), (slot + 1) * (k + 1))
        res.append([st.legs[f]["out_bits"][p][sl] for f in (0, 1) for p in (0, 1)] + [st.legs[0]["q"][0][sl]])
    assert not np.all(res[0][0] == SENT16)
    for x, y in zip(*res):
        assert np.array_equal(x, y)


def test_argument_errors_leave_the_outputs_untouched():
    n = _n()
    H, Hkv, k = 4, 2, 3
    R, W, P = S * (k + 1), (H + 2 * Hkv) * D, L * 2 * Hkv
    rng = np.random.default_rng(3)
    img0 = np.full(q8.image_bytes(P, 1024, D), GB, np.uint8)
    images = [torch.from_numpy(img0).to(DEV) for _ in range(S)]
    store = [torch.full((P * (k + 1), D), SENT, dtype=torch.float16, device=DEV) for _ in range(S)]
    ptr = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)
    kvq, kvb = ptr(images), ptr(store)
    qkv = torch.from_numpy(rng.standard_normal((R, W), dtype=F32)).to(DEV)
    cs = torch.zeros((R, D // 2, 2), dtype=torch.float32, device=DEV)
    qh = torch.full((R, H * D), SENT, dtype=torch.float16, device=DEV)
    ql = qh.clone()
    cap, ln, live = _i32([1024] * S), _i32([5, 6, 7]), _i32([1] * S)
    good = dict(qkv=qkv, ld=W, in_layout=1, q_hi=qh, q_lo=ql, q_ts=H * D, cs=cs, kv_base=kvb, cap=cap, length=ln, live=live, S=S, k=k,
                layer=LAYER, H=H, Hkv=Hkv, D=D, kvq_base=kvq, qcap=1024, n_layers=L, fresh=True)
    for kw in (dict(D=64), dict(qcap=0), dict(layer=L), dict(layer=-1), dict(n_layers=0), dict(in_layout=2), dict(S=17), dict(S=0),
               dict(k=16), dict(k=-1), dict(S=16, k=4), dict(ld=W - 4), dict(q_ts=H * D + 4), dict(fresh=2), dict(H=0)):
        with pytest.raises(Exception, match="pc_rope_append_slots_rows_q8"):
            n.rope_append_slots_rows_q8(**{**good, **kw})
    nw = n.attn_verify_slots_q8_workspace_bytes(S, k, H, D, 2) // 4
    assert nw * 4 == n.attn_verify_slots_workspace_bytes(S, k, H, D, 3)          # one record more than the fp16 entry's
    ws = torch.full((nw,), SENT, dtype=torch.float32, device=DEV)
    out = tuple(torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV) for _ in range(2))
    agood = dict(q_hi=qh, q_lo=ql, q_ts=H * D, kv_base=kvb, cap=cap, length=ln, live=live, S=S, k=k, layer=LAYER, H=H, Hkv=Hkv, D=D,
                 softmax_scale=0.088, nsplit=2, workspace=ws, out_frag=out, kvq_base=kvq, qcap=1024, n_layers=L, fresh=True)
    short = ws[:n.attn_verify_slots_workspace_bytes(S, k, H, D, 2) // 4]         # (the fp16 entry's size: one record short)
    for kw in (dict(D=64), dict(qcap=0), dict(layer=L), dict(n_layers=0), dict(nsplit=33), dict(nsplit=0), dict(S=0), dict(S=17), dict(k=16),
               dict(S=16, k=4), dict(workspace=short), dict(workspace=ws[1:]), dict(Hkv=3), dict(q_ts=H * D - 8), dict(fresh=2)):
        with pytest.raises(Exception, match="pc_attn_verify_slots_q8"):
            n.attn_verify_slots_q8(**{**agood, **kw})
    torch.cuda.synchronize()
    assert torch.all(qh == SENT) and torch.all(ql == SENT) and torch.all(ws == SENT) and torch.all(out[0] == SENT) and torch.all(out[1] == SENT)
    for b in range(S):
        assert torch.all(store[b] == SENT) and np.array_equal(images[b].cpu().numpy(), img0)
    n.rope_append_slots_rows_q8(**good)                                          # ... and the unmodified calls are accepted
    n.attn_verify_slots_q8(**agood)
    torch.cuda.synchronize()
    assert not torch.all(qh == SENT) and not torch.all(out[0] == SENT)
