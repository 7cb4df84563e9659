"""The many-row projections (pc_gemm_dense, pc_gemm_dense_ws, pc_gemm_dense_qkv_rope, pc_gemm_dense_a8; pc_gemm_dense.hip) pinned
to EXACT sums and to the split-precision floor.

Integer operands (tests/gemm_ref.py): every partial sum in any order is exact in fp32, so every comparison is ``torch.equal``
against an int64 (or float64: equally exact here) reference -- one mis-summed, dropped or doubled 16-deep slab, one lost lo-plane
MFMA, one K-tail chunk from the wrong place, one wrong weight row shows as a failed bit comparison, not as noise under a
tolerance.  The shapes select the instantiations (tests/dense_ref.py restates launch_dense_tile and launch_dense_splitk;
tests/test_dense_ref_cpu.py checks every table entry against it); no environment override is used.

Poison everywhere a correct kernel never reads or writes: activation planes and weights are views into wider buffers whose
columns K .. ld and rows behind M (behind N) hold NaN; y is a view with ldy > N and two guard rows in a NaN bit pattern compared as
int32; fp16 output planes, q planes and arenas carry a NaN sentinel compared as int16.  Guards and sentinels are checked after
every launch.

Gaussian operands: ``max |got - ref| <= floor16 / 32`` (gemm_ref.SPLIT_RULE); both sides come from the reference alone
(tests/test_dense_ref_cpu.py derives the room).  Each case prints its measured ``err / floor16`` as a ``SPLIT_FLOOR`` line
(collected in profiles/gemm_split_floor.json).
"""
import numpy as np
import pytest
import torch

from tests import dense_ref as dr
from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN32 = 0x7FC12345          # guard pattern of fp32 outputs and workspaces (a NaN), compared as int32
NAN16 = 0x7DAD              # sentinel of fp16 planes and arenas (a NaN), compared as int16
PAD = 24                    # poisoned columns behind K (three 16-byte chunks)


def _n():
    from promptcache_amd import _native
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(v):
    """fp16 [R][C] values -> a view [R][C] into a NaN buffer [R + 2][C + PAD]."""
    R, C = v.shape
    buf = torch.full((R + 2, C + PAD), float("nan"), dtype=torch.float16, device=DEV)
    buf[:R, :C] = _dev(v.astype(np.float16))
    return buf[:R, :C]


def _planes(hi, lo6):
    return _poisoned(hi), None if lo6 is None else _poisoned(lo6.astype(np.float64) * gr.LO_UNIT)


def _ref(hi, lo6, w_int, w):
    """Exact fp32 [M][N] on the device.  Small problems: int64 on the host; otherwise float64 on the device from the fp16 weight
    ``w`` already there (every value is an integer multiple of 2^-6 far below 2^53: float64 is exact too)."""
    if w_int.shape[0] * w_int.shape[1] <= (1 << 18):
        return _dev(gr.from_sum6(gr.exact_sum6(hi, lo6, w_int)))
    x6 = hi * 64 + (0 if lo6 is None else lo6)
    return ((_dev(x6.astype(np.float32)).double() @ w.double().t()) * gr.LO_UNIT).float()


class _Y:
    """fp32 output [M][N] as a view with ldy = N + 4 and two guard rows, all in the NAN32 pattern."""

    def __init__(self, M, N, base=None):
        self.M, self.N, self.ldy = M, N, N + 4
        self.buf = torch.full(((M + 2) * self.ldy,), NAN32, dtype=torch.int32, device=DEV)
        self.y = self.buf.view(torch.float32).view(M + 2, self.ldy)[:M, :N]
        if base is not None:
            self.y.copy_(base)

    def guards_intact(self):
        g = self.buf.view(self.M + 2, self.ldy)
        return bool((g[:self.M, self.N:] == NAN32).all()) and bool((g[self.M:] == NAN32).all())


class _Plane:
    """fp16 output [R][C] as a view with ld = C + 8 and two guard rows, all in the NAN16 sentinel."""

    def __init__(self, R, C):
        self.R, self.C = R, C
        self.buf = torch.full((R + 2, C + 8), NAN16, dtype=torch.int16, device=DEV)
        self.p = self.buf.view(torch.float16)[:R, :C]

    def guards_intact(self):
        return bool((self.buf[:self.R, self.C:] == NAN16).all()) and bool((self.buf[self.R:] == NAN16).all())


def _store_and_add(n, c, xh, xl, w, ref, seed, wscale=None, workspace=None):
    """One STORE and one ADD launch at case ``c``: results bit-equal, guard columns and rows intact."""
    tag = (c.M, c.N, c.K, xl is not None)
    out = _Y(c.M, c.N)
    n.gemm_dense(xh, xl, w, c.M, c.N, c.K, n.EPI_STORE, y=out.y, wscale=wscale, workspace=workspace)
    assert torch.equal(out.y, ref), ("store",) + tag + (int((out.y != ref).sum()),)
    assert out.guards_intact(), ("store guards",) + tag
    y0 = _dev(dr.base_ints(c.M, c.N, seed))
    out = _Y(c.M, c.N, y0)
    n.gemm_dense(xh, xl, w, c.M, c.N, c.K, n.EPI_ADD, y=out.y, wscale=wscale, workspace=workspace)
    assert torch.equal(out.y, y0 + ref), ("add",) + tag + (int((out.y != y0 + ref).sum()),)
    assert out.guards_intact(), ("add guards",) + tag


# ---------------------------------------------------------------------------------------------------
# a. store and add, both tiles, one and two planes
# ---------------------------------------------------------------------------------------------------

def _exact_case(c, seed):
    n = _n()
    w_int = gr.exact_weight(c.N, c.K, seed)
    w = _poisoned(w_int)
    for two in (True, False):
        hi, lo6 = gr.exact_planes(c.M, c.K, seed + 1, two)
        xh, xl = _planes(hi, lo6)
        _store_and_add(n, c, xh, xl, w, _ref(hi, lo6, w_int, w), seed + 2)


@pytest.mark.parametrize("M", list(dr.ROW_EDGE))
def test_exact_store_and_add_narrow_tile(M):
    """gemm_dense_kernel<4, STORE | ADD, TWO>: one row class against every ragged N (fewer than 8 panels; a panel count that is
    no multiple of 8) and every K / 8 class (tail only; no tail; one- and five-chunk tails at odd and even nk; a full pipeline)."""
    for c in dr.STORE_ADD_NARROW:
        if c.M == M:
            _exact_case(c, 100)


@pytest.mark.parametrize("c", dr.STORE_ADD_WIDE, ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_exact_store_and_add_wide_tile(c):
    """gemm_dense_kernel<2, STORE | ADD, TWO> without a workspace: the small shapes whose 128-wide grid needs two rounds of the 256
    CUs where the 256-wide one needs one."""
    _exact_case(c, 200)


# ---------------------------------------------------------------------------------------------------
# b. wscale
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", dr.WSCALE_CASES, ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_exact_weight_row_scales(c):
    """Per-row powers of two in 2^-2 .. 2^2: sum * wscale[n] is exact, under STORE and ADD, one and two planes."""
    n = _n()
    w_int = gr.exact_weight(c.N, c.K, 300)
    w = _poisoned(w_int)
    _, sc = dr.pow2_scales(c.N, 301, *dr.WSCALE_EXP)
    scd = _dev(sc)
    for two in (True, False):
        hi, lo6 = gr.exact_planes(c.M, c.K, 302, two)
        xh, xl = _planes(hi, lo6)
        _store_and_add(n, c, xh, xl, w, _ref(hi, lo6, w_int, w) * scd[None, :], 303, wscale=scd)


# ---------------------------------------------------------------------------------------------------
# c. split-K through pc_gemm_dense_ws
# ---------------------------------------------------------------------------------------------------

def _workspace(words):
    return torch.full((words,), NAN32, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("c", dr.SPLIT_CASES, ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_exact_split_k_with_workspace(c):
    """launch_dense<2, EPI_STORE> over K slices + dense_reduce_kernel<ADD>: bit-equal results; the slabs (the first
    slices * M * N floats of the workspace) finite, everything behind them untouched; a workspace one byte short runs the plain
    form: same bits, workspace untouched."""
    n = _n()
    used = c.kslices * c.M * c.N
    w_int = gr.exact_weight(c.N, c.K, 400)
    w = _poisoned(w_int)
    for two in (True, False):
        hi, lo6 = gr.exact_planes(c.M, c.K, 401, two)
        xh, xl = _planes(hi, lo6)
        ref = _ref(hi, lo6, w_int, w)
        y0 = _dev(dr.base_ints(c.M, c.N, 402))
        for epi, want in ((n.EPI_STORE, ref), (n.EPI_ADD, y0 + ref)):
            tag = (c.M, c.N, c.K, two, epi)
            ws = _workspace(used + 1024)
            out = _Y(c.M, c.N, y0 if epi == n.EPI_ADD else None)
            n.gemm_dense(xh, xl, w, c.M, c.N, c.K, epi, y=out.y, workspace=ws)
            assert torch.equal(out.y, want), tag + (int((out.y != want).sum()),)
            assert out.guards_intact(), tag
            assert bool(torch.isfinite(ws.view(torch.float32)[:used]).all()), tag + ("slabs",)
            assert bool((ws[used:] == NAN32).all()), tag + ("behind the slabs",)
            # the slabs are the exact partial sums of their K ranges, in slice order
            if two and epi == n.EPI_STORE:
                slabs, k0 = ws.view(torch.float32)[:used].view(c.kslices, c.M, c.N), 0
                for s, steps in enumerate(c.steps):
                    k1 = min(k0 + steps * dr.BK, c.K)
                    part = _dev(gr.from_sum6(gr.exact_sum6(hi, lo6, w_int, k0, k1)))
                    assert torch.equal(slabs[s], part), tag + ("slab", s)
                    k0 = k1
            ws = _workspace(used + 1024)
            out = _Y(c.M, c.N, y0 if epi == n.EPI_ADD else None)
            n.gemm_dense(xh, xl, w, c.M, c.N, c.K, epi, y=out.y, workspace=ws.view(torch.uint8)[:4 * used - 1])
            assert torch.equal(out.y, want) and out.guards_intact(), tag + ("one byte short",)
            assert bool((ws == NAN32).all()), tag + ("one byte short: workspace",)


@pytest.mark.parametrize("c,why", dr.SPLIT_REFUSED, ids=[w.replace(" ", "_") for _, w in dr.SPLIT_REFUSED])
def test_split_k_refused_leaves_the_workspace_untouched(c, why):
    n = _n()
    w_int = gr.exact_weight(c.N, c.K, 500)
    w = _poisoned(w_int)
    hi, lo6 = gr.exact_planes(c.M, c.K, 501, True)
    xh, xl = _planes(hi, lo6)
    ws = _workspace(8 * c.M * c.N + 1024)
    _store_and_add(n, c, xh, xl, w, _ref(hi, lo6, w_int, w), 502, workspace=ws)
    assert bool((ws == NAN32).all()), (why, c)


# ---------------------------------------------------------------------------------------------------
# d. SiLU and GELU epilogues, Gaussian operands
# ---------------------------------------------------------------------------------------------------

def _report(family, M, N, K, err, floor16):
    print(f"SPLIT_FLOOR family={family} M={M} N={N} K={K} err={err:.4e} floor16={floor16:.4e} ratio={err / floor16:.4e}")


@pytest.mark.parametrize("c", dr.ACT_CASES, ids=lambda c: f"{c.act}-{c.M}x{c.inter}x{c.K}-{'two' if c.two else 'one'}{'-wscale' if c.wscale else ''}")
def test_split_precision_activation_epilogues(c):
    """of_hi + of_lo against fp64 with floor16 = max |fp16(ref) - ref|; the planes are consistent bit for bit and of_lo is
    non-zero in more than half of the elements (as test_gpu_gemm_exact.py states it); sentinel columns and rows intact.  The
    one-plane form is held to its own reference: the activation of fp16(x) w^T."""
    n = _n()
    M, inter, K = c.M, c.inter, c.K
    N = dr.act_cols(c)
    assert K <= gr.SPLIT_K_MAX
    xn, wn = gr.gaussian_operands(M, N, K, 43)
    hi, lo = gr.split_planes(xn)
    xh, xl = _poisoned(hi), _poisoned(lo) if c.two else None
    w = _poisoned(wn)
    sc = _dev(dr.act_wscale(N)) if c.wscale else None
    oh, ol = _Plane(M, inter), _Plane(M, inter)
    n.gemm_dense(xh, xl, w, M, N, K, n.EPI_SILU if c.act == "silu" else n.EPI_GELU, out_hi=oh.p, out_lo=ol.p, wscale=sc)
    z = (_dev(xn).double() if c.two else xh.double()) @ w.double().t()
    if sc is not None:
        z = z * sc.double()[None, :]
    if c.act == "silu":
        g, u = z[:, :inter], z[:, inter:]
        ref = g / (1 + torch.exp(-g)) * u
    else:
        ref = 0.5 * z * (1 + torch.erf(z * 0.7071067811865476))
    floor16 = float((ref.half().double() - ref).abs().max())
    h, l = oh.p, ol.p
    err = float((h.double() + l.double() - ref).abs().max())
    _report(f"dense_{c.act}_{'wide' if c.tile == 256 else 'narrow'}", M, N, K, err, floor16)
    assert oh.guards_intact() and ol.guards_intact()
    # Plane consistency, bit for bit: of_hi is the fp16 rounding of of_hi + of_lo (formed in fp32, exact).  pc_split's pair
    # (hi = fp16(s), lo = fp16(s - hi)) allows exactly one exception: s - hi a hair inside half an ulp of hi rounds, as fp16, to
    # the half ulp itself, so hi + lo is an exact tie and round-to-even may name hi's neighbour.
    # Hence: of_lo never exceeds half an ulp of of_hi, and wherever the rounding of the sum is not of_hi, |of_lo| IS that half ulp.
    hf, lf = h.float(), l.float()
    half_ulp = torch.where(hf.abs() < 2.0 ** -14, torch.full_like(hf, 2.0 ** -25), torch.exp2(torch.frexp(hf).exponent.float() - 12))
    off = h != (hf + lf).half()
    print(f"PLANE_TIES {c.act} M={M} inter={inter}: {int(off.sum())} of {off.numel()} elements sit on an fp16 tie")
    assert bool((lf.abs() <= half_ulp).all()), "of_lo exceeds half an ulp of of_hi"
    assert bool((lf.abs()[off] == half_ulp[off]).all()), "of_hi is not a nearest fp16 of of_hi + of_lo"
    assert float((l != 0).float().mean()) > 0.5
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)


# ---------------------------------------------------------------------------------------------------
# e. q|k|v + RoPE epilogue
# ---------------------------------------------------------------------------------------------------

def _sent(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(torch.float16)


@pytest.mark.parametrize("c", dr.ROPE_CASES, ids=lambda c: f"B{c.B}-H{c.H}-Hkv{c.Hkv}-q{c.q_len}-K{c.K}")
def test_exact_qkv_rope_epilogue(c):
    """The rotation table varies per (row, feature pair) over (1, 0), (0, 1), (-1, 0), (0, -1), (0.5, 0.5): a wrong table row or
    column, a wrong weight-row-to-LDS-row map, a wrong head, batch row or arena row shows as a failed bit comparison."""
    n = _n()
    B, H, Hkv, q_len, K = c.B, c.H, c.Hkv, c.q_len, c.K
    T, W = dr.rope_dims(c)
    pasts = list(c.past) if isinstance(c.past, tuple) else [c.past] * B
    cap = max(pasts) + q_len + 2
    w_int = gr.exact_weight(W, K, 600)
    w = _poisoned(w_int)
    hi, lo6 = gr.exact_planes(T, K, 601, c.two)
    xh, xl = _planes(hi, lo6)
    sums = _ref(hi, lo6, w_int, w).double().cpu().numpy()
    cs_np = dr.rotation_table(T)
    e = dr.rope_expect(sums, cs_np, H, Hkv)                                       # [T][heads][128] float64, exact
    qe = _dev(e[:, :H].reshape(T, H * 128).astype(np.float32))
    ke = _dev(e[:, H:H + Hkv].reshape(B, q_len, Hkv, 128).transpose(0, 2, 1, 3).astype(np.float32))
    ve = _dev(e[:, H + Hkv:].reshape(B, q_len, Hkv, 128).transpose(0, 2, 1, 3).astype(np.float32))
    q_ts = H * 128 + 8
    q, ql = _sent(T + 2, q_ts), _sent(T + 2, q_ts)
    arena = _sent(B, 2, Hkv, cap, 128)
    lo_rows = cap - c.lo_row0
    klo = _sent(B, 2, Hkv, lo_rows, 128)
    kv_lo = (klo[:, 0], klo[:, 1], 2 * Hkv * lo_rows * 128, lo_rows * 128, c.lo_row0) if c.kv_lo else None
    past_lens = _dev(np.asarray(pasts, dtype=np.int32)) if isinstance(c.past, tuple) else None
    n.gemm_dense_qkv_rope(xh, xl, w, K, _dev(cs_np), q, ql if c.q_lo else None, q_ts, arena[:, 0], arena[:, 1], 2 * Hkv * cap * 128,
                          cap * 128, B, H, Hkv, 128, q_len, max(pasts), cap, kv_lo=kv_lo, past_lens=past_lens)
    torch.cuda.synchronize()
    tag = tuple(c[:-1])
    qv = q[:T, :H * 128]
    assert torch.equal(qv, qe.half()), tag + ("q_hi", int((qv != qe.half()).sum()))
    q16, ql16 = q.view(torch.int16), ql.view(torch.int16)
    assert bool((q16[:T, H * 128:] == NAN16).all()) and bool((q16[T:] == NAN16).all()), tag + ("q sentinels",)
    if c.q_lo:
        assert torch.equal(qv.float() + ql[:T, :H * 128].float(), qe), tag + ("q_hi + q_lo",)
        assert bool((ql16[:T, H * 128:] == NAN16).all()) and bool((ql16[T:] == NAN16).all()), tag + ("q_lo sentinels",)
    else:
        assert bool((ql16 == NAN16).all()), tag + ("q_lo absent",)
    a16, l16 = arena.view(torch.int16), klo.view(torch.int16)
    for b, past in enumerate(pasts):
        new = arena[b, :, :, past:past + q_len]
        assert torch.equal(new[0], ke[b].half()) and torch.equal(new[1], ve[b].half()), tag + ("arena rows", b)
        assert bool((a16[b, :, :, :past] == NAN16).all()) and bool((a16[b, :, :, past + q_len:] == NAN16).all()), tag + ("arena sentinels", b)
        if c.kv_lo:
            r0 = past - c.lo_row0
            nl = klo[b, :, :, r0:r0 + q_len]
            assert torch.equal(new[0].float() + nl[0].float(), ke[b]) and torch.equal(new[1].float() + nl[1].float(), ve[b]), tag + ("arena + lo", b)
            assert bool((l16[b, :, :, :r0] == NAN16).all()) and bool((l16[b, :, :, r0 + q_len:] == NAN16).all()), tag + ("lo sentinels", b)
    if not c.kv_lo:
        assert bool((l16 == NAN16).all()), tag + ("k_lo / v_lo absent",)


# ---------------------------------------------------------------------------------------------------
# f. LLM.int8 form
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", dr.A8_CASES, ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_exact_a8_codes_scales_and_corr(c):
    """sum * w_scale[n] * x_scale[m] + corr[m][n], bit-equal under STORE and ADD; with *corr_has = 0 a corr full of NaN is
    ignored.  corr is a view with ldc > N into a NaN buffer."""
    n = _n()
    M, N, K = c.M, c.N, c.K
    q, w_int, we, xe, corr = dr.a8_operands(M, N, K, 700)
    plain, with_corr = dr.a8_expect(q, w_int, we, xe, corr)
    xq, w = _poisoned(q), _poisoned(w_int)
    wsc, xsc = _dev(np.exp2(we).astype(np.float32)), _dev(np.exp2(xe).astype(np.float32))
    cbuf = torch.full((M + 2, N + 4), float("nan"), dtype=torch.float32, device=DEV)
    cv = cbuf[:M, :N]
    y0 = _dev(dr.base_ints(M, N, 701))
    for has in (1, 0):
        if has:
            cv.copy_(_dev(corr.astype(np.float32)))
        else:
            cbuf.fill_(float("nan"))
        flag = torch.tensor([has], dtype=torch.int32, device=DEV)
        ref = _dev((with_corr if has else plain).astype(np.float32))
        out = _Y(M, N)
        n.gemm_dense_a8(xq, w, wsc, xsc, cv, flag, M, N, K, n.EPI_STORE, y=out.y)
        assert torch.equal(out.y, ref) and out.guards_intact(), ("store", M, N, K, has, int((out.y != ref).sum()))
        out = _Y(M, N, y0)
        n.gemm_dense_a8(xq, w, wsc, xsc, cv, flag, M, N, K, n.EPI_ADD, y=out.y)
        assert torch.equal(out.y, y0 + ref) and out.guards_intact(), ("add", M, N, K, has, int((out.y != y0 + ref).sum()))


# ---------------------------------------------------------------------------------------------------
# g. split precision of the plain product: Gaussian operands against floor16 / 32
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", dr.SPLIT_FLOOR, ids=lambda c: f"{c.family}-{c.M}x{c.N}x{c.K}")
def test_split_precision_plain_product(c):
    n = _n()
    M, N, K = c.M, c.N, c.K
    assert K <= gr.SPLIT_K_MAX
    xn, wn = gr.gaussian_operands(M, N, K, 41)
    hi, lo = gr.split_planes(xn)
    xh, xl = _poisoned(hi), None if c.form == "one" else _poisoned(lo)
    w = _poisoned(wn)
    if N <= 512:
        ref_np, floor16 = gr.split_floor(xn, wn)
        ref = _dev(ref_np)
    else:
        x = _dev(xn)
        ref = x.double() @ w.double().t()
        floor16 = float((x.half().double() @ w.double().t() - ref).abs().max())
    if c.form == "one":                                               # its own reference: fp16(x) w^T
        ref = xh.double() @ w.double().t()
    base = None
    if c.form == "add":
        base = _dev(np.random.default_rng(1).standard_normal((M, N)).astype(np.float32))
        ref = ref + base.double()
    ws = _workspace(8 * M * N) if c.form == "ws" else None
    out = _Y(M, N, base)
    n.gemm_dense(xh, xl, w, M, N, K, n.EPI_ADD if c.form == "add" else n.EPI_STORE, y=out.y, workspace=ws)
    err = float((out.y.double() - ref).abs().max())
    _report(c.family, M, N, K, err, floor16)
    assert out.guards_intact()
    if ws is not None:                                                # the split form ran: two slabs of finite partial sums
        used = dr.plan(M, N, K, dr.EPI_STORE, ws_bytes=4 * ws.numel()).kslices * M * N
        assert used >= 2 * M * N and bool(torch.isfinite(ws.view(torch.float32)[:used]).all()) and bool((ws[used:] == NAN32).all())
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)
