"""The weight-streaming projections (pc_gemm: pc_gemm_skinny.h, pc_gemm_rows.hip, pc_gemm_ks.hip) pinned to EXACT sums and to
the split-precision floor.

Integer operands (tests/gemm_ref.py): every partial sum in any order is exact in fp32, so every comparison below is
``torch.equal`` against an int64 (or float64: equally exact here) reference -- one mis-summed, dropped or doubled k-step, one
lost lo-plane MFMA, one wrong tile or row shows as a failed bit comparison, not as noise under a tolerance.  The shapes select
the instantiations (tiles per workgroup 1 / 2 / 3 / 4 / 8 through N, block depths and tails through K, row regimes through M);
no environment override is used.  Activation planes carry NaN in the pad rows of their last row tile.

Gaussian operands: ``max |got - ref| <= floor16 / 32`` (gemm_ref.SPLIT_RULE), floor16 = what fp16 activations alone would
lose; both sides come from the reference alone (tests/test_gemm_ref_cpu.py derives the room).  Each case prints its measured
``err / floor16`` as a ``SPLIT_FLOOR`` line (collected in profiles/gemm_split_floor.json).
"""
import numpy as np
import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN32 = 0x7FC12345          # guard pattern of fp32 outputs (a NaN), compared as int32
NAN16 = 0x7DAD              # sentinel of fp16 arenas (a NaN), compared as int16


def _n():
    from promptcache_amd import _native
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(hi, lo6, tiles=None):
    """int64 [M][K] planes -> device fragment planes with NaN pad rows (``tiles``: row tiles to allocate, NaN behind M)."""
    M, K = hi.shape
    rows = M if tiles is None else 16 * tiles
    def one(v):
        full = np.full((rows, K), np.nan, dtype=np.float16)
        full[:M] = v
        return _dev(gr.pack_plane(full))
    return one(hi.astype(np.float16)), None if lo6 is None else one((lo6.astype(np.float64) * gr.LO_UNIT).astype(np.float16))


def _ref(hi, lo6, w_int, wd_chunks=None, k0=0, k1=None):
    """Exact fp32 [M][N] on the device.  Small problems: int64 on the host; large N: float64 on the device, 2048 weight rows at
    a time (every value is an integer multiple of 2^-6 far below 2^53: float64 is exact too)."""
    k1 = hi.shape[1] if k1 is None else k1
    if w_int.shape[0] * w_int.shape[1] <= (1 << 18):
        return _dev(gr.from_sum6(gr.exact_sum6(hi, lo6, w_int, k0, k1)))
    x6 = hi[:, k0:k1] * 64 + (0 if lo6 is None else lo6[:, k0:k1])
    xd = _dev(x6.astype(np.float64))
    out = [xd @ c[:, k0:k1].double().t() for c in wd_chunks]
    return (torch.cat(out, dim=1) * gr.LO_UNIT).float()


def _weight(N, K, seed, lim=2):
    n = _n()
    w_int = gr.exact_weight(N, K, seed, lim)
    w16 = _dev(w_int.astype(np.float16))
    return w_int, n.to_weight_frags(w16), list(torch.split(w16, 2048, dim=0))


def _ints(shape, seed, lim=8):
    return _dev(np.random.default_rng(seed).integers(-lim, lim + 1, size=shape).astype(np.float32))


# ---------------------------------------------------------------------------------------------------
# exact sums: plain store and residual add, one and two planes, <= 64 rows
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("units", list(gr.EXACT_UNITS))
@pytest.mark.parametrize("regime", list(gr.EXACT_ROWS))
def test_exact_store_and_add(regime, units):
    """One (row regime, tiles per workgroup) pair: every K / 32 in (1, 7, 9, 17, 33, 72) -- waves of the eight-way K split
    with nothing, one step, a tail shorter than any block depth, one block plus a tail, several blocks -- and every row count
    of the regime.  N / 16 = 3, 257, 514, 771, 1027 make choose_T return 1, 2, 3, 4, 8 and leave a last workgroup with clamped
    duplicate tiles (launch_T runs T = 4 in place of 8 for four row tiles)."""
    n = _n()
    N = 16 * units
    for ks in (gr.EXACT_KS_WIDEST if units == 1027 else gr.EXACT_KS):
        K = 32 * ks
        w_int, wf, wd = _weight(N, K, 100 + units)
        for M in gr.EXACT_ROWS[regime]:
            y0 = _ints((M, N), M + ks)
            for two in (True, False):
                hi, lo6 = gr.exact_planes(M, K, 200 + units, two)
                xh, xl = _planes(hi, lo6)
                ref = _ref(hi, lo6, w_int, wd)
                y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
                n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N)
                assert torch.equal(y, ref), ("store", M, N, K, two, int((y != ref).sum()))
                y2 = y0.clone()
                n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_ADD, y=y2, ldy=N)
                assert torch.equal(y2, y0 + ref), ("add", M, N, K, two, int((y2 != y0 + ref).sum()))


@pytest.mark.parametrize("N", gr.DEEP_N)
def test_exact_deep_block_residual_add(N):
    """launch_one's U = 16 block (one row tile, one weight tile per workgroup, residual add, M > 4, K / 32 >= 256): 32 or 33
    k-steps per wave = two blocks, two blocks plus a tail of one, and a last wave that holds less."""
    n = _n()
    for ks in gr.DEEP_KS:
        K = 32 * ks
        w_int, wf, wd = _weight(N, K, 300 + ks)
        for M in gr.DEEP_ROWS:
            y0 = _ints((M, N), M + ks)
            for two in (True, False):
                hi, lo6 = gr.exact_planes(M, K, 301, two)
                xh, xl = _planes(hi, lo6)
                ref = _ref(hi, lo6, w_int, wd)
                y = y0.clone()
                n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_ADD, y=y, ldy=N)
                assert torch.equal(y, y0 + ref), (M, N, K, two, int((y != y0 + ref).sum()))


# ---------------------------------------------------------------------------------------------------
# K slices: slabs, and the reduction inside the launch
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [5, 17, 33, 64])
def test_exact_k_slices_as_slabs(M):
    """Every slab equals the exact partial sum of its own K range (ceil(KS / kslices) k-steps per slice); with more slices than
    k-steps the slabs behind the end are exactly zero."""
    n = _n()
    for N in (48, 4112):
        for ks in gr.SLAB_KS:
            K = 32 * ks
            w_int, wf, wd = _weight(N, K, 400 + ks)
            hi, lo6 = gr.exact_planes(M, K, 401, True)
            xh, xl = _planes(hi, lo6)
            for S in gr.SLAB_SLICES:
                y = torch.full((S, M, N), float("nan"), dtype=torch.float32, device=DEV)
                n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N, kslices=S)
                for s, (k0, k1) in enumerate(gr.slice_ranges(ks, S)):
                    if k0 == k1:
                        assert bool((y[s] == 0).all()), ("empty slab", M, N, K, S, s)
                    else:
                        ref = _ref(hi, lo6, w_int, wd, 32 * k0, 32 * k1)
                        assert torch.equal(y[s], ref), (M, N, K, S, s, int((y[s] != ref).sum()))


@pytest.mark.parametrize("M", gr.KSRED_ROWS)
def test_exact_in_launch_k_reduction(M):
    """gemm_skinny_ks: scratch pre-filled with NaN, two launches without re-zeroing the counters; both bit-equal to the
    reference, counters all zero after each."""
    n = _n()
    for units in gr.KSRED_UNITS:
        N = 16 * units
        for ks in gr.KSRED_KS:
            K = 32 * ks
            w_int, wf, wd = _weight(N, K, 500 + ks)
            hi, lo6 = gr.exact_planes(M, K, 501, True)
            xh, xl = _planes(hi, lo6)
            ref = _ref(hi, lo6, w_int, wd)
            y0 = _ints((M, N), M + ks)
            for S in gr.KSRED_S:
                for T in gr.KSRED_T:
                    if M > 16 and T == 8:
                        continue
                    words = (2 if M > 16 else 1) * n.gemm_skinny_ks_scratch_bytes(N, S) // 4
                    scratch = torch.full((words,), float("nan"), dtype=torch.float32, device=DEV)
                    counters = torch.zeros((units + T - 1) // T, dtype=torch.int32, device=DEV)
                    for rep in range(2):
                        y = y0.clone()
                        n.gemm_skinny_ks(wf, xh, xl, M, N, K, y, N, S, T, scratch, counters)
                        assert torch.equal(y, y0 + ref), (M, N, K, S, T, rep, int((y != y0 + ref).sum()))
                        assert int(counters.abs().sum()) == 0, (M, N, K, S, T, rep)


# ---------------------------------------------------------------------------------------------------
# 65..512 rows
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", gr.ROWS_M)
def test_exact_rows_kernel(M):
    """gemm_rows_kernel: one and two row blocks, odd tile counts (the staging waves' row tile), a shorter second block; K ranges
    of one k-step, less than a stage, and ending inside a stage; kslices 1 and 3, store and add, one and two planes."""
    n = _n()
    for units in gr.ROWS_UNITS:
        N = 16 * units
        for ks in gr.ROWS_KS:
            K = 32 * ks
            w_int, wf, wd = _weight(N, K, 600 + ks)
            y0 = _ints((M, N), M + ks)
            for two in (True, False):
                hi, lo6 = gr.exact_planes(M, K, 601, two)
                xh, xl = _planes(hi, lo6)
                ref = _ref(hi, lo6, w_int, wd)
                y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
                n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N)
                assert torch.equal(y, ref), ("store", M, N, K, two, int((y != ref).sum()))
                y2 = y0.clone()
                n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_ADD, y=y2, ldy=N)
                assert torch.equal(y2, y0 + ref), ("add", M, N, K, two, int((y2 != y0 + ref).sum()))
                ys = torch.full((3, M, N), float("nan"), dtype=torch.float32, device=DEV)
                n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_STORE, y=ys, ldy=N, kslices=3)
                for s, (k0, k1) in enumerate(gr.slice_ranges(ks, 3)):
                    part = torch.zeros_like(ref) if k0 == k1 else _ref(hi, lo6, w_int, wd, 32 * k0, 32 * k1)
                    assert torch.equal(ys[s], part), ("slab", M, N, K, two, s, int((ys[s] != part).sum()))


# ---------------------------------------------------------------------------------------------------
# int8 weight image
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", gr.W8_ROWS)
def test_exact_int8_weight_image(M):
    """Codes in [-127, 127] (one +-127 per row), scales = exact powers of two that differ from row to row: store, add and three
    K slices (cut on k-step pairs) are exact."""
    n = _n()
    for N in (48, 4112):
        for k64 in gr.W8_K64:
            K = 64 * k64
            rng = np.random.default_rng([700, N, K])
            q = rng.integers(-gr.W8_CODE_MAX, gr.W8_CODE_MAX + 1, size=(N, K), dtype=np.int64)
            q[np.arange(N), rng.integers(0, K, size=N)] = np.where(np.arange(N) % 2 == 0, 127, -127)
            scale = (2.0 ** (np.arange(N) % 4)).astype(np.float32)
            wf8 = n.to_weight_frags_i8(_dev(q.astype(np.int8)))
            sc = _dev(scale)
            qd = list(torch.split(_dev(q.astype(np.float16)), 2048, dim=0))
            hi, lo6 = gr.exact_planes(M, K, 701, True)
            xh, xl = _planes(hi, lo6)
            ref = _ref(hi, lo6, q, qd) * sc[None, :]
            y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
            n.gemm_skinny(wf8, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N, wscale=sc)
            assert torch.equal(y, ref), ("store", M, N, K, int((y != ref).sum()))
            y0 = _ints((M, N), M + k64)
            y2 = y0.clone()
            n.gemm_skinny(wf8, xh, xl, M, N, K, n.EPI_ADD, y=y2, ldy=N, wscale=sc)
            assert torch.equal(y2, y0 + ref), ("add", M, N, K, int((y2 != y0 + ref).sum()))
            ys = torch.full((3, M, N), float("nan"), dtype=torch.float32, device=DEV)
            n.gemm_skinny(wf8, xh, xl, M, N, K, n.EPI_STORE, y=ys, ldy=N, kslices=3, wscale=sc)
            for s, (k0, k1) in enumerate(gr.slice_ranges(K // 32, 3, w8=True)):
                part = torch.zeros_like(ref) if k0 == k1 else _ref(hi, lo6, q, qd, 32 * k0, 32 * k1) * sc[None, :]
                assert torch.equal(ys[s], part), ("slab", M, N, K, s, int((ys[s] != part).sum()))


# ---------------------------------------------------------------------------------------------------
# q|k|v + RoPE epilogue
# ---------------------------------------------------------------------------------------------------

def _qkv_run(n, shape, hid, sin_one, kslices=1, live=None, seed=800):
    """One q|k|v launch on integer operands with the rotation table written directly: (cos, sin) = (1, 0) or (0, 1) in every
    entry.  Returns what the checks need.  ``live``: rows_dev value (rows >= live of the planes hold NaN)."""
    B, H, Hkv, D, q_len, past = shape
    T, W = B * q_len, (H + 2 * Hkv) * D
    cap = past + q_len + 2
    w_int = gr.exact_weight(W, hid, seed)
    w16 = _dev(w_int.astype(np.float16))
    wf = n.to_weight_frags(w16[n.qkv_rope_row_perm(H + 2 * Hkv, D).to(DEV)].contiguous())
    hi, lo6 = gr.exact_planes(T, hid, seed + 1, True)
    rows = T if live is None else min(live, T)
    xh, xl = _planes(hi[:rows], lo6[:rows], tiles=(T + 15) // 16)
    ref = _ref(hi, lo6, w_int, list(torch.split(w16, 2048, dim=0)))
    cs = torch.zeros((T, D // 2, 2), dtype=torch.float32, device=DEV)
    cs[..., 1 if sin_one else 0] = 1.0
    sent = lambda *s: torch.full(s, NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    arena, lo_rows = sent(B, 2, Hkv, cap, D), q_len + 2
    klo = sent(B, 2, Hkv, lo_rows, D)
    q, ql = sent(T, H * D), sent(T, H * D)
    scratch = torch.full((kslices, T, W), float("nan"), dtype=torch.float32, device=DEV) if kslices > 1 else None
    n.gemm_qkv_rope(wf, xh, xl, T, hid, cs, q, ql, H * D, arena[:, 0], arena[:, 1], 2 * Hkv * cap * D, cap * D, B, H, Hkv, D,
                    q_len, past, cap, kv_lo=(klo[:, 0], klo[:, 1], 2 * Hkv * lo_rows * D, lo_rows * D), lo_base=-1,
                    kslices=kslices, scratch=scratch,
                    rows_dev=None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return ref, q, ql, arena, klo


def _qkv_expect(ref, shape, sin_one):
    """Expected q [T][H][D], k and v [B][Hkv][q_len][D] (fp32, exact) from the exact sums ``ref`` [T][(H + 2 Hkv) D]."""
    B, H, Hkv, D, q_len, past = shape
    T = B * q_len
    def rot(x):                                  # x [..., D]: (cos, sin) = (0, 1): low half = -partner, high half = +partner
        return torch.cat([-x[..., D // 2:], x[..., :D // 2]], dim=-1) if sin_one else x
    qe = rot(ref[:, :H * D].reshape(T, H, D))
    ke = rot(ref[:, H * D:(H + Hkv) * D].reshape(B, q_len, Hkv, D)).permute(0, 2, 1, 3)
    ve = ref[:, (H + Hkv) * D:].reshape(B, q_len, Hkv, D).permute(0, 2, 1, 3)
    return qe, ke, ve


def _qkv_check(shape, hid, sin_one, kslices=1):
    n = _n()
    B, H, Hkv, D, q_len, past = shape
    T = B * q_len
    ref, q, ql, arena, klo = _qkv_run(n, shape, hid, sin_one, kslices)
    assert float(ref.abs().max()) <= 2048
    qe, ke, ve = _qkv_expect(ref, shape, sin_one)
    tag = (shape, hid, sin_one, kslices)
    assert torch.equal(q.float() + ql.float(), qe.reshape(T, H * D)), tag                 # q_hi + q_lo: the exact sums
    assert torch.equal(q, qe.reshape(T, H * D).half()), tag
    new = arena[:, :, :, past:past + q_len]
    assert torch.equal(new[:, 0], ke.half()) and torch.equal(new[:, 1], ve.half()), tag    # arena rows: fp16(sum); v unrotated
    assert torch.equal(new[:, 0].float() + klo[:, 0, :, :q_len].float(), ke), tag
    assert torch.equal(new[:, 1].float() + klo[:, 1, :, :q_len].float(), ve), tag
    a16, l16 = arena.view(torch.int16), klo.view(torch.int16)
    assert bool((a16[:, :, :, :past] == NAN16).all()) and bool((a16[:, :, :, past + q_len:] == NAN16).all()), tag
    assert bool((l16[:, :, :, q_len:] == NAN16).all()), tag


@pytest.mark.parametrize("hid", gr.QKV_HIDDEN)
@pytest.mark.parametrize("shape", gr.QKV_SHAPES)
def test_exact_qkv_rope_epilogue(shape, hid):
    """(cos, sin) = (1, 0): q_hi + q_lo are the exact sums, the arena rows fp16(sum).  (0, 1): every feature is plus or minus its
    rotary partner's exact sum, v unrotated.  Rows outside [past, past + q_len) and residual rows of other tokens keep their
    sentinel bits.  The 70-row case also runs with two K slices (qkv_rope_slabs_kernel)."""
    for sin_one in (False, True):
        _qkv_check(shape, hid, sin_one)
        if shape[0] * shape[4] > 64:
            _qkv_check(shape, hid, sin_one, kslices=2)


# ---------------------------------------------------------------------------------------------------
# output geometry: ldy > N, guard rows, rows_dev
# ---------------------------------------------------------------------------------------------------

def _guarded(rows, ldy):
    return torch.full(((rows + 2) * ldy,), NAN32, dtype=torch.int32, device=DEV)


def _guards_intact(buf, rows, N, ldy):
    g = buf.view(rows + 2, ldy)
    return bool((g[:rows, N:] == NAN32).all()) and bool((g[rows:] == NAN32).all())


@pytest.mark.parametrize("M", [5, 17, 33, 65])
def test_output_geometry_ldy_and_guards(M):
    """ldy = N + 4 and two guard rows behind the output: results exact, guard columns and rows untouched (int32 compare) under
    store, add, slabs and the in-launch reduction."""
    n = _n()
    N, ks = 80, 9
    K, ldy = 32 * ks, N + 4
    w_int, wf, wd = _weight(N, K, 900)
    hi, lo6 = gr.exact_planes(M, K, 901, True)
    xh, xl = _planes(hi, lo6)
    ref = _ref(hi, lo6, w_int, wd)
    y0 = _ints((M, N), 902)
    for epi in (n.EPI_STORE, n.EPI_ADD):
        buf = _guarded(M, ldy)
        yv = buf.view(torch.float32).view(M + 2, ldy)
        if epi == n.EPI_ADD:
            yv[:M, :N] = y0
        n.gemm_skinny(wf, xh, xl, M, N, K, epi, y=buf, ldy=ldy)
        assert torch.equal(yv[:M, :N], ref + y0 if epi == n.EPI_ADD else ref), (M, epi)
        assert _guards_intact(buf, M, N, ldy), (M, epi)
    S = 3
    buf = _guarded(S * M, ldy)
    n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_STORE, y=buf, ldy=ldy, kslices=S)
    yv = buf.view(torch.float32).view(S * M + 2, ldy)
    for s, (k0, k1) in enumerate(gr.slice_ranges(ks, S)):
        assert torch.equal(yv[s * M:(s + 1) * M, :N], _ref(hi, lo6, w_int, wd, 32 * k0, 32 * k1)), (M, "slab", s)
    assert _guards_intact(buf, S * M, N, ldy), (M, "slabs")
    if M <= 32:
        for S, T in ((3, 2), (2, 4)):
            scratch = torch.full(((2 if M > 16 else 1) * n.gemm_skinny_ks_scratch_bytes(N, S) // 4,), float("nan"), dtype=torch.float32, device=DEV)
            counters = torch.zeros((N // 16 + T - 1) // T, dtype=torch.int32, device=DEV)
            buf = _guarded(M, ldy)
            yv = buf.view(torch.float32).view(M + 2, ldy)
            yv[:M, :N] = y0
            n.gemm_skinny_ks(wf, xh, xl, M, N, K, buf, ldy, S, T, scratch, counters)
            assert torch.equal(yv[:M, :N], ref + y0) and _guards_intact(buf, M, N, ldy), (M, "ks", S, T)


@pytest.mark.parametrize("M", [16, 32, 64])
def test_rows_dev_limits_the_live_rows(M):
    """rows_dev (what every row-bucketed captured graph passes): rows < live are bit-equal to a launch with M = live and no
    rows_dev -- and to the exact sums -- while the plane rows >= live hold NaN; a value above M clamps to M; the guard rows
    behind M stay untouched.  Rows >= live of y are unspecified and not inspected."""
    n = _n()
    N, ks = 80, 9
    K = 32 * ks
    w_int, wf, wd = _weight(N, K, 1000)
    hi, lo6 = gr.exact_planes(M, K, 1001, True)
    y0 = _ints((M, N), 1002)
    for live in (1, M - 3, M, M + 5):
        rows = min(live, M)
        rd = torch.tensor([live], dtype=torch.int32, device=DEV)
        xh, xl = _planes(hi[:rows], lo6[:rows], tiles=M // 16)
        xh_b, xl_b = _planes(hi[:rows], lo6[:rows])
        ref = _ref(hi[:rows], lo6[:rows], w_int, wd)
        runs = [("store", lambda y, m, a, b, r: n.gemm_skinny(wf, a, b, m, N, K, n.EPI_STORE, y=y, ldy=N, rows_dev=r), False),
                ("add", lambda y, m, a, b, r: n.gemm_skinny(wf, a, b, m, N, K, n.EPI_ADD, y=y, ldy=N, rows_dev=r), True)]
        if M <= 32:
            def ks_run(y, m, a, b, r):
                scratch = torch.full(((2 if m > 16 else 1) * n.gemm_skinny_ks_scratch_bytes(N, 3) // 4,), float("nan"), dtype=torch.float32, device=DEV)
                n.gemm_skinny_ks(wf, a, b, m, N, K, y, N, 3, 2, scratch, torch.zeros(3, dtype=torch.int32, device=DEV), rows_dev=r)
            runs.append(("ks", ks_run, True))
        for name, run, adds in runs:
            buf = _guarded(M, N)
            ya = buf.view(torch.float32).view(M + 2, N)
            ya[:M] = y0
            run(buf, M, xh, xl, rd)
            yb = y0[:rows].clone()
            run(yb, rows, xh_b, xl_b, None)
            want = ref + y0[:rows] if adds else ref
            assert torch.equal(yb, want), (name, M, live, "plain launch")
            assert torch.equal(ya[:rows], yb), (name, M, live)
            assert bool((buf.view(M + 2, N)[M:] == NAN32).all()), (name, M, live, "guard rows")


@pytest.mark.parametrize("M", [16, 32, 64])
def test_rows_dev_under_the_qkv_epilogue(M):
    """The same under the q|k|v epilogue: q rows and arena rows of the tokens < live are exact, arena rows of tokens >= live are
    not inspected, the rows behind past + q_len and in front of past keep their sentinel bits."""
    n = _n()
    shape = (1, 2, 1, 64, M, 3)
    B, H, Hkv, D, q_len, past = shape
    for live in (1, M - 3, M, M + 5):
        rows = min(live, M)
        ref, q, ql, arena, klo = _qkv_run(n, shape, 96, False, live=live)
        qe, ke, ve = _qkv_expect(ref, shape, False)
        assert torch.equal(q[:rows].float() + ql[:rows].float(), qe.reshape(M, H * D)[:rows]), (M, live)
        new = arena[:, :, :, past:past + rows]
        assert torch.equal(new[:, 0], ke[:, :, :rows].half()) and torch.equal(new[:, 1], ve[:, :, :rows].half()), (M, live)
        assert torch.equal(new[:, 0].float() + klo[:, 0, :, :rows].float(), ke[:, :, :rows]), (M, live)
        a16 = arena.view(torch.int16)
        assert bool((a16[:, :, :, :past] == NAN16).all()) and bool((a16[:, :, :, past + q_len:] == NAN16).all()), (M, live)
        assert bool((klo.view(torch.int16)[:, :, :, q_len:] == NAN16).all()), (M, live)


# ---------------------------------------------------------------------------------------------------
# split precision: Gaussian operands against floor16 / 32
# ---------------------------------------------------------------------------------------------------

def _report(family, M, N, K, err, floor16):
    print(f"SPLIT_FLOOR family={family} M={M} N={N} K={K} err={err:.4e} floor16={floor16:.4e} ratio={err / floor16:.4e}")


def _floor_dev(x, wd):
    """gemm_ref.split_floor on the device (float64): large N."""
    ref = x.double() @ wd.t()
    return ref, float((x.half().double() @ wd.t() - ref).abs().max())


@pytest.mark.parametrize("family,M,N,K,extra", gr.SPLIT_STORE, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in gr.SPLIT_STORE])
def test_split_precision_store(family, M, N, K, extra):
    n = _n()
    assert K <= gr.SPLIT_K_MAX
    xn, wn = gr.gaussian_operands(M, N, K, 41)
    x, w = _dev(xn), _dev(wn)
    xh, xl = n.to_act_frags(x)
    sc = None
    if family == "w8":
        q, sc = n.quantize_rows_int8(w)
        wf, wd = n.to_weight_frags_i8(q), q.double() * sc.double()[:, None]
    else:
        wf, wd = n.to_weight_frags(w), w.double()
    if N <= 512:
        ref_np, floor16 = gr.split_floor(xn, wd.cpu().numpy())
        ref = _dev(ref_np)
    else:
        ref, floor16 = _floor_dev(x, wd)
    if family == "ks":
        S, T = extra["S"], extra["T"]
        scratch = torch.full((n.gemm_skinny_ks_scratch_bytes(N, S) // 4,), float("nan"), dtype=torch.float32, device=DEV)
        y = torch.zeros((M, N), dtype=torch.float32, device=DEV)
        n.gemm_skinny_ks(wf, xh, xl, M, N, K, y, N, S, T, scratch, torch.zeros((N // 16 + T - 1) // T, dtype=torch.int32, device=DEV))
        got = y.double()
    else:
        S = extra.get("kslices", 1)
        y = torch.full((S, M, N), float("nan"), dtype=torch.float32, device=DEV)
        n.gemm_skinny(wf, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N, kslices=S, wscale=sc)
        got = y.double().sum(0)
    err = float((got - ref).abs().max())
    _report(family, M, N, K, err, floor16)
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)


@pytest.mark.parametrize("M,N,K", gr.SPLIT_NORM)
def test_split_precision_norm_folded_source(M, N, K):
    """gemm_skinny_norm against fp64 RMSNorm followed by the product; floor16 is taken on fp16(normed x)."""
    n = _n()
    xn, wn = gr.gaussian_operands(M, N, K, 41, 3.0)
    gain = (1.0 + 0.2 * np.random.default_rng(5).standard_normal(K, dtype=np.float32)).astype(np.float16)
    eps = 1e-5
    normed = gr.rmsnorm64(xn, gain, eps)
    wd = wn.astype(np.float64)
    ref = normed @ wd.T
    floor16 = float(np.abs(normed.astype(np.float16).astype(np.float64) @ wd.T - ref).max())
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    n.gemm_skinny_norm(n.to_weight_frags(_dev(wn)), _dev(xn), _dev(gain), eps, M, N, K, n.EPI_STORE, y=y, ldy=N)
    err = float((y.double() - _dev(ref)).abs().max())
    _report("norm", M, N, K, err, floor16)
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)


@pytest.mark.parametrize("inter", gr.SPLIT_ACT_INTER)
@pytest.mark.parametrize("M", gr.SPLIT_ACT_ROWS)
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_split_precision_activation_epilogues(act, M, inter):
    """of_hi + of_lo against fp64 with floor16 = max |fp16(ref) - ref|; the planes are consistent bit for bit
    (of_hi == fp16(of_hi + of_lo formed in fp32)) and of_lo is non-zero in more than half of the elements."""
    n = _n()
    K = gr.SPLIT_ACT_K[inter]
    N = 2 * inter if act == "silu" else inter
    xn, wn = gr.gaussian_operands(M, N, K, 43)
    x, w = _dev(xn), _dev(wn)
    xh, xl = n.to_act_frags(x)
    mt = (M + 15) // 16
    oh = torch.zeros((mt, inter // 32, 64, 8), dtype=torch.float16, device=DEV)
    ol = torch.zeros_like(oh)
    n.gemm_skinny(n.to_weight_frags(w), xh, xl, M, N, K, n.EPI_SILU if act == "silu" else n.EPI_GELU, of_hi=oh, of_lo=ol)
    z = x.double() @ w.double().t()
    if act == "silu":
        g, u = z[:, :inter], z[:, inter:]
        ref = g / (1 + torch.exp(-g)) * u
    else:
        ref = 0.5 * z * (1 + torch.erf(z * 0.7071067811865476))
    floor16 = float((ref.half().double() - ref).abs().max())
    h, l = n.from_act_frags(oh, M), n.from_act_frags(ol, M)
    err = float((h.double() + l.double() - ref).abs().max())
    _report(act + ("_rows" if M > 64 else ""), M, N, K, err, floor16)
    # Plane consistency, bit for bit: of_hi is the fp16 rounding of of_hi + of_lo (formed in fp32, exact).  pc_split's pair
    # (hi = fp16(s), lo = fp16(s - hi)) allows exactly one exception: s - hi a hair inside half an ulp of hi rounds, as fp16, to
    # the half ulp itself, so hi + lo is an exact tie and round-to-even may name hi's neighbour (one element in a few thousand; more where of_lo is an fp16 subnormal).
    # Hence: of_lo never exceeds half an ulp of of_hi, and wherever the rounding of the sum is not of_hi, |of_lo| IS that half ulp.
    hf, lf = h.float(), l.float()
    half_ulp = torch.where(hf.abs() < 2.0 ** -14, torch.full_like(hf, 2.0 ** -25), torch.exp2(torch.frexp(hf).exponent.float() - 12))
    off = h != (hf + lf).half()
    print(f"PLANE_TIES {act} M={M} inter={inter}: {int(off.sum())} of {off.numel()} elements sit on an fp16 tie")
    assert bool((lf.abs() <= half_ulp).all()), "of_lo exceeds half an ulp of of_hi"
    assert bool((lf.abs()[off] == half_ulp[off]).all()), "of_hi is not a nearest fp16 of of_hi + of_lo"
    assert float((l != 0).float().mean()) > 0.5
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)
