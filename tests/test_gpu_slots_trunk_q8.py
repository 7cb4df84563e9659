"""The shared-trunk slot attention over int8 K / V images on the GPU (csrc/pc_slots_q8.hip):
pc_attn_decode_slots_trunk_q8 through the C-ABI against tests/slot_trunk_q8_ref.py -- a member's own image rows [0, T) hold poison,
so a kernel that reads them cannot pass --, the staged row bit for bit against tests/kv_q8_ref.py, every other image byte, guard,
arena and dead slot untouched, a dead leader whose rows are still read, both tile shapes, bit identity with
pc_attn_decode_slots_q8 where nobody shares, invariance under the size of the group, agreement with pc_attn_decode_slots_trunk on
rows on which the format is lossless, and every argument error."""
import numpy as np
import pytest
import torch

from tests import kv_q8_ref as q8
from tests import slot_kv_q8_ref as ref
from tests import slot_trunk_q8_ref as tref
from tests.test_gpu_slots_q8 import ATT_TOL, CAP, DEV, GUARD, LAYER, SENT, D, L, Q8Slots, _i32, _n, _q, _split16

pytestmark = pytest.mark.gpu
F32 = np.float32


def shared_rows(b, lens, leader, trunk, qcap):
    """The predicate of the entry (slot_trunk_rows_q8; every slot here has an image), on the host."""
    g = leader[b]
    if not 0 <= g < len(lens):
        return 0
    T = trunk[g]
    return T if leader[g] == g and T > 0 and trunk[b] == T and T <= lens[b] and T <= qcap else 0


class TrunkSlots(Q8Slots):
    """``Q8Slots`` with leader / trunk words: a slot that names a leader holds the leader's fp16 rows [0, T) in its arena (T: its
    own trunk word), and -- where the entry's predicate gives it shared rows and it is not the leader itself -- POISON in rows
    [0, T) of its image: codes 0x55, scale NaN.  ``dead``: slots whose live word is 0 although they hold ``lens[b]`` rows."""

    def __init__(self, rng, lens, leader, trunk, Hkv, qcap, dead=(), lossless=False):
        S = len(lens)
        rows = []
        for b, m in enumerate(lens):
            if lossless:
                rows.append(ref.lossless_rows(rng, (L, 2, Hkv, m + 1), D)[0])
            else:
                kv = rng.standard_normal((L, 2, Hkv, m + 1, D), dtype=F32)
                kv[:, 0] *= 0.7
                rows.append(kv.astype(np.float16))
        for b in range(S):
            g, T = leader[b], trunk[b]
            if 0 <= g < S and g != b and 0 < T <= min(lens[b], lens[g]):
                rows[b][:, :, :, :T] = rows[g][:, :, :, :T]
        super().__init__(rng, lens, Hkv, qcap, rows=rows)
        self.leader_l, self.trunk_l = list(leader), list(trunk)
        self.leader, self.trunk = _i32(leader), _i32(trunk)
        self.T = [shared_rows(b, self.lens, leader, trunk, qcap) for b in range(S)]
        for b in range(S):
            if self.T[b] and leader[b] != b:
                img = self.image0[b]
                c, s = q8.unpack(img[GUARD:-GUARD], self.P, qcap, D)
                c, s = c.copy(), s.copy()
                c[:, :self.T[b]], s[:, :self.T[b]] = 0x55, np.nan
                img[GUARD:-GUARD] = q8.pack(c, s)
                self.images[b].copy_(torch.from_numpy(img))
        for b in dead:
            self.live[b] = 0
        self.livet = _i32(self.live)

    def planes0(self, b):
        """(codes [L][2][Hkv][qcap][D], scale [L][2][Hkv][qcap]) of slot b's INITIAL image."""
        c, s = q8.unpack(self.image0[b][GUARD:-GUARD], self.P, self.qcap, D)
        return c.reshape(L, 2, self.Hkv, self.qcap, D), s.reshape(L, 2, self.Hkv, self.qcap)

    def want(self, b, q):
        """The reference output of live slot b: [H * D] fp32."""
        m, T, g = self.lens[b], self.T[b], self.leader_l[b]
        oc, osc = self.planes0(b)
        lc, lsc = self.planes0(g) if T else (oc, osc)
        cut = lambda c, s, p, n: (c[LAYER, p, :, :n], s[LAYER, p, :, :n])
        return tref.attend(q, T, cut(lc, lsc, 0, max(T, 0)), cut(lc, lsc, 1, max(T, 0)), cut(oc, osc, 0, m), cut(oc, osc, 1, m),
                           self.new16[b][0], self.new16[b][1]).reshape(-1)


def _attend(n, sl, q, H, ns_own, ns_trunk, entry="trunk_q8"):
    """One launch of ``entry`` over ``sl`` with q [S][H][D] fp32 -> (out [S][H*D] fp32, hi, lo frags), guards checked."""
    S, Hkv = sl.S, sl.Hkv
    hi, lo = _split16(q.reshape(S, H * D))
    qh, ql = torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV)
    words = (n.attn_decode_slots_workspace_bytes(S, H, D, ns_own) if entry == "q8"
             else n.attn_decode_slots_trunk_workspace_bytes(S, H, D, ns_own, ns_trunk)) // 4
    wsg = torch.full((words + 32,), SENT, dtype=torch.float32, device=DEV)
    out = (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
           torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
    head = (qh, ql, H * D, sl.kv_base, sl.cap, sl.len, sl.livet)
    tail = (S, LAYER, H, Hkv, D, 1.0 / np.sqrt(D))
    if entry == "q8":
        n.attn_decode_slots_q8(*head, *tail, ns_own, wsg[16:16 + words], out, sl.kvq_base, sl.qcap, L)
    elif entry == "trunk_fp16":
        n.attn_decode_slots_trunk(*head, sl.leader, sl.trunk, *tail, ns_own, ns_trunk, wsg[16:16 + words], out)
    else:
        n.attn_decode_slots_trunk_q8(*head, sl.leader, sl.trunk, *tail, ns_own, ns_trunk, wsg[16:16 + words], out, sl.kvq_base, sl.qcap, L)
    torch.cuda.synchronize()
    assert torch.all(wsg[:16] == SENT) and torch.all(wsg[-16:] == SENT), "a guard word of the workspace was written"
    got = (n.from_act_frags(out[0], S).float() + n.from_act_frags(out[1], S).float()).cpu().numpy()
    return got, out[0], out[1]


def _check(n, sl, q, H, ns_own, ns_trunk, tag):
    """Every live slot against the reference; row len staged bit for bit; everything else untouched."""
    arenas0 = [a.clone() for a in sl.arenas]
    got, oh, _ = _attend(n, sl, q, H, ns_own, ns_trunk)
    raw = n.from_act_frags(oh, sl.S).cpu().numpy()
    worst = 0.0
    for b in range(sl.S):
        assert torch.equal(sl.arenas[b].view(torch.int16), arenas0[b].view(torch.int16)), f"slot {b}: the fp16 arena was written"
        staged = bool(sl.live[b]) and sl.lens[b] < sl.caps[b]
        now, want_img = sl.images[b].cpu().numpy(), sl.expected_image(b, staged)
        diff = np.flatnonzero(now != want_img)
        assert diff.size == 0, (f"slot {b} (len {sl.lens[b]}, T {sl.T[b]}): {diff.size} image bytes differ from the initial image"
                                f"{' with the quantised row at len' if staged else ''}; first at byte {int(diff[0]) - GUARD}")
        if not staged:
            assert np.all(raw[b] == SENT), f"slot {b} (dead) was written"
            continue
        err = float(np.abs(got[b] - sl.want(b, q[b])).max())
        worst = max(worst, err)
        print(f"[{tag}] slot {b}: leader {sl.leader_l[b]}, T {sl.T[b]}, {sl.lens[b]} + 1 keys, max|d| = {err:.2e}")
        assert np.isfinite(got[b]).all() and err < ATT_TOL, (b, sl.lens[b], sl.T[b], err)
    print(f"[{tag}] worst max|d| = {worst:.2e}")


# group A: slots 0, 2, 5 led by 0, T = 300 (no multiple of 16; slot 0 has T = len: no own image key); group B: slots 3, 4 led by 3,
# T = 7 (below one key tile; slot 4 has T = len); slot 1 on its own; slot 6 a dead member of group A; slot 7 names leader 0 with
# another trunk word: the plain attention over its own complete image
LENS = [300, 257, 301, 700, 7, 1022, 400, 500]
LEADER = [0, -1, 0, 3, 3, 0, 0, 0]
TRUNK = [300, 0, 300, 7, 7, 300, 300, 123]


@pytest.mark.parametrize("leader_dead", [False, True])
@pytest.mark.parametrize("H,Hkv,ns_own,ns_trunk,qcap", [(4, 4, 1, 1, 1024), (4, 4, 4, 4, 1024), (4, 2, 1, 4, 1024), (4, 2, 4, 1, 1536)])
def test_attention_and_staged_row_vs_the_references(H, Hkv, ns_own, ns_trunk, qcap, leader_dead):
    n = _n()
    rng = np.random.default_rng(H * 100 + Hkv * 10 + ns_own + 7 * ns_trunk + qcap)
    sl = TrunkSlots(rng, LENS, LEADER, TRUNK, Hkv, qcap, dead=(6, 0) if leader_dead else (6,))
    assert sl.T == [300, 0, 300, 7, 7, 300, 300, 0]
    _check(n, sl, _q(rng, sl.S, H), H, ns_own, ns_trunk,
           f"slots trunk q8 H={H} Hkv={Hkv} own={ns_own} trunk={ns_trunk} qcap={qcap}{' leader dead' if leader_dead else ''}")


@pytest.mark.parametrize("ns_own,ns_trunk", [(1, 1), (4, 2)])
def test_sixteen_slots_fill_two_tiles(ns_own, ns_trunk):
    """S = 16, H = 4, Hkv = 2: 32 columns, the two-tile instantiation.  Ten live members of group A: 20 columns, in both tiles."""
    n = _n()
    rng = np.random.default_rng(160 + ns_own)
    lens = [300, 640, 301, 70, 333, 1022, 400, 500, 300, 512, 317, 999, 801, 70, 71, 200]
    leader = [0, -1, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 3, -1]
    trunk = [300, 0, 300, 70, 300, 300, 300, 300, 300, 300, 300, 300, 300, 70, 70, 0]
    sl = TrunkSlots(rng, lens, leader, trunk, 2, 1024, dead=(6,))
    assert sum(1 for b in range(16) if sl.T[b] == 300 and sl.live[b]) == 10
    _check(n, sl, _q(rng, 16, 4), 4, ns_own, ns_trunk, f"slots trunk q8 S=16 own={ns_own} trunk={ns_trunk}")


@pytest.mark.parametrize("H,Hkv,nsplit", [(4, 4, 4), (4, 2, 1)])
def test_nobody_shares_is_the_plain_entry_bit_for_bit(H, Hkv, nsplit):
    """leader = -1 everywhere: both output planes and all images equal pc_attn_decode_slots_q8 at nsplit = nsplit_own."""
    n = _n()
    lens = [256, 257, 5, 1022, 0, 1, 700, CAP - 1]
    res = []
    for entry in ("q8", "trunk_q8"):
        rng = np.random.default_rng(H + Hkv + nsplit)                                    # the same slots and q twice
        sl = TrunkSlots(rng, lens, [-1] * 8, [0] * 8, Hkv, 1024, dead=(4,))
        q = _q(rng, 8, H)
        _, oh, ol = _attend(n, sl, q, H, nsplit, 3, entry)
        res.append((oh.clone().view(torch.int16), ol.clone().view(torch.int16), [t.clone() for t in sl.images]))
        for b in range(8):
            assert np.array_equal(sl.images[b].cpu().numpy(), sl.expected_image(b, b != 4))
    (h0, l0, im0), (h1, l1, im1) = res
    assert torch.equal(h0, h1) and torch.equal(l0, l1), "output planes differ from pc_attn_decode_slots_q8"
    assert all(torch.equal(a, b) for a, b in zip(im0, im1)), "an image differs from pc_attn_decode_slots_q8's"


@pytest.mark.parametrize("H,Hkv,ns_own,ns_trunk", [(4, 2, 4, 4), (4, 4, 1, 2)])
def test_a_member_does_not_depend_on_the_size_of_its_group(H, Hkv, ns_own, ns_trunk):
    """The same member with the same leader rows in a group of 2 at slots (0, 1) and in a group of 8 at slot 6: identical output
    fragments and staged row."""
    n = _n()
    T, m = 300, 777
    res = []
    for slot, lens in ((1, [T + 40, m, 3, 5, 9, 600, 64, 11]), (6, [T + 40, 900, T, 444, 1001, 301, m, 555])):
        rng = np.random.default_rng(42)                                                  # the leader's rows: the first drawn, both times
        leader = [0, 0] + [-1] * 6 if slot == 1 else [0] * 8
        trunk = [T, T] + [0] * 6 if slot == 1 else [T] * 8
        sl = TrunkSlots(rng, lens, leader, trunk, Hkv, 1024)
        mrng = np.random.default_rng(4242)                                               # the member's own rows and q, both times
        own = mrng.standard_normal((L, 2, Hkv, m + 1 - T, D), dtype=F32).astype(np.float16)
        a = sl.arenas[slot].cpu().numpy()
        a[:, :, :, T:m + 1] = own
        sl.arenas[slot].copy_(torch.from_numpy(a))
        c, s = q8.unpack(sl.image0[slot][GUARD:-GUARD], sl.P, sl.qcap, D)
        c, s = c.copy(), s.copy()
        c[:, T:m], s[:, T:m] = q8.quantise(a[:, :, :, T:m].reshape(sl.P, m - T, D))
        sl.image0[slot][GUARD:-GUARD] = q8.pack(c, s)
        sl.images[slot].copy_(torch.from_numpy(sl.image0[slot]))
        sl.new16[slot] = a[LAYER, :, :, m]
        q = _q(rng, 8, H)
        q[slot] = _q(mrng, 1, H)[0]
        got, oh, ol = _attend(n, sl, q, H, ns_own, ns_trunk)
        assert sl.T[slot] == T and np.abs(got[slot] - sl.want(slot, q[slot])).max() < ATT_TOL
        assert np.array_equal(sl.images[slot].cpu().numpy(), sl.expected_image(slot, True))
        codes, scale = sl.image_planes(slot)
        res.append((n.from_act_frags(oh, 8)[slot].clone().view(torch.int16), n.from_act_frags(ol, 8)[slot].clone().view(torch.int16),
                    codes[LAYER, :, :, m].copy(), scale[LAYER, :, :, m].copy().view(np.uint32)))
    small, large = res
    assert torch.equal(small[0], large[0]) and torch.equal(small[1], large[1]), "output fragments differ"
    assert np.array_equal(small[2], large[2]) and np.array_equal(small[3], large[3]), "the staged image row differs"


@pytest.mark.parametrize("H,Hkv,ns_own,ns_trunk", [(4, 4, 1, 1), (4, 2, 4, 4)])
def test_lossless_rows_agree_with_the_fp16_trunk_entry(H, Hkv, ns_own, ns_trunk):
    """On rows the format holds exactly, images and arenas are the same numbers: the entry and pc_attn_decode_slots_trunk differ by
    summation order only, each within ATT_TOL of the common reference."""
    n = _n()
    rng = np.random.default_rng(H + Hkv + ns_own + ns_trunk)
    sl = TrunkSlots(rng, LENS, LEADER, TRUNK, Hkv, 1024, dead=(6,), lossless=True)
    q = _q(rng, sl.S, H)
    got8, _, _ = _attend(n, sl, q, H, ns_own, ns_trunk)
    for b in range(sl.S):                                                                # (the staged rows are exact too)
        assert np.array_equal(sl.images[b].cpu().numpy(), sl.expected_image(b, b != 6))
    got16, _, _ = _attend(n, sl, q, H, ns_own, ns_trunk, "trunk_fp16")
    live = [b for b in range(sl.S) if b != 6]
    err = float(np.abs(got8[live] - got16[live]).max())
    print(f"[slots trunk q8 lossless H={H} Hkv={Hkv} own={ns_own} trunk={ns_trunk}] max|q8 - fp16 trunk entry| = {err:.2e}")
    assert np.isfinite(got8[live]).all() and err < 2 * ATT_TOL


def test_argument_errors_leave_every_output_untouched():
    n = _n()
    rng = np.random.default_rng(11)
    H, Hkv, ns_own, ns_trunk = 4, 2, 2, 2
    sl = TrunkSlots(rng, [300, 310], [0, 0], [300, 300], Hkv, 1024)
    S = sl.S
    hi, lo = _split16(_q(rng, S, H).reshape(S, H * D))
    qh, ql = torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV)
    ws = torch.full((n.attn_decode_slots_trunk_workspace_bytes(S, H, D, ns_own, ns_trunk) // 4,), SENT, dtype=torch.float32, device=DEV)
    out = (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
           torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
    good = dict(q_hi=qh, q_lo=ql, q_ts=H * D, kv_base=sl.kv_base, cap=sl.cap, length=sl.len, live=sl.livet, leader=sl.leader,
                trunk=sl.trunk, S=S, layer=LAYER, H=H, Hkv=Hkv, D=D, softmax_scale=0.088, nsplit_own=ns_own, nsplit_trunk=ns_trunk,
                workspace=ws, out_frag=out, kvq_base=sl.kvq_base, qcap=1024, n_layers=L)
    null = torch.empty(0, dtype=torch.int32, device=DEV)                # data_ptr() == 0
    assert null.data_ptr() == 0
    cases = [dict(D=64), dict(leader=null), dict(trunk=null), dict(kvq_base=null), dict(nsplit_trunk=0), dict(nsplit_trunk=33),
             dict(qcap=0), dict(layer=L), dict(workspace=ws[:-1]), dict(S=17),
             dict(nsplit_own=0), dict(nsplit_own=33), dict(H=3), dict(S=0), dict(n_layers=0), dict(kv_base=null), dict(live=null)]
    for kw in cases:
        with pytest.raises(RuntimeError, match="-1001"):
            n.attn_decode_slots_trunk_q8(**{**good, **kw})
    torch.cuda.synchronize()
    assert torch.all(ws == SENT) and torch.all(out[0] == SENT) and torch.all(out[1] == SENT)
    for b in range(S):
        assert np.array_equal(sl.images[b].cpu().numpy(), sl.image0[b])
    n.attn_decode_slots_trunk_q8(**good)                                # ... and the unmodified call is accepted
    torch.cuda.synchronize()
    assert not torch.any(n.from_act_frags(out[0], S) == SENT)
