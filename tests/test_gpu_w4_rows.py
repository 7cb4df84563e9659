"""pc_gemm_w4_rows (csrc/pc_gemm_w4_rows.hip): the 1..64-row projections over the MXFP4 weight images of pc_gemm_w4.

* Exact sums: integer operands (tests/mxfp4_ref.exact_weight against tests/gemm_ref.exact_planes; the headroom argument of
  tests/test_mxfp4_cpu.py holds per K slice too: a slice's sum is a sub-sum) -- ``torch.equal`` against the integer reference, the
  sum of the slabs and every slab against the sum over its own quads, NaN in the pad rows of the last row tile, NaN-pattern guards
  behind N, behind the last slab and in a slab behind ``kslices``.
* A slice without a quad stores zeros.
* Bit-equality with pc_gemm_w4 (the reference is that kernel): row r of a 64-row launch against the one-row launch of row r.
* Row independence across M, split-precision floor (``max |got - ref| <= floor16 / 32``, both sides from the reference), guards.
"""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_ref as gr
from tests import mxfp4_ref as mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN32 = 0x7FC12345
ROWS = (17, 32, 33, 48, 64)
SLICES = (1, 2, 4)


def _n():
    from promptcache_amd import _native
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(hi, lo):
    """fp16 [M][K] planes -> device fragment planes [ceil(M/16)][K/32][64][8], NaN in the pad rows of the last row tile."""
    return _dev(gr.pack_plane(hi.astype(np.float16))), _dev(gr.pack_plane(lo.astype(np.float16)))


@functools.lru_cache(maxsize=2)
def _exact_case(units, K):
    """Weight images, 64 integer rows (a launch of M rows takes the first M) and the exact references: for every ``kslices`` the
    per-slab sums over the slab's own quads, (64 hi + lo6) . (2 W')^T scaled by 2^-7 once.  The products run in float64 on
    integers whose sums stay far below 2^53 -- bit for bit the int64 sum -- and are checked to be integers below 2^24 units."""
    N = 16 * units
    codes, exps, w2 = mx.exact_weight(N, K, 900 + units)
    ci, si = _n().to_weight_frags_w4(_dev(codes), _dev(exps))
    hi, lo6 = gr.exact_planes(64, K, 901 + units, True)
    x7 = (hi * 64 + lo6).astype(np.float64)
    wd = w2.astype(np.float64)
    refs = {}
    for ks in SLICES:
        slabs = []
        for q0, q1 in gr.slice_ranges(K // 128, ks):
            s = x7[:, q0 * 128:q1 * 128] @ wd[:, q0 * 128:q1 * 128].T if q1 > q0 else np.zeros((64, N))
            assert np.abs(s).max(initial=0) < 2.0 ** 24 and np.array_equal(s, s.astype(np.int64))
            slabs.append(_dev((s.astype(np.int64).astype(np.float64) * 2.0 ** -7).astype(np.float32)))
        refs[ks] = slabs
    return ci, si, hi, lo6, refs


# ---------------------------------------------------------------------------------------------------
# exact sums
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [128, 384, 1152, 2560])      # K / 128 = 1, 3, 9, 20: empty waves and slices, one quad each, tails
@pytest.mark.parametrize("units", [1, 3, 257])             # one workgroup with clamped duplicate tiles, ..., 65 workgroups
def test_exact_store_slabs(units, K):
    n = _n()
    N, ldy = 16 * units, 16 * units + 4
    ci, si, hi, lo6, refs = _exact_case(units, K)
    for M in ROWS:
        xh, xl = _planes(hi[:M], lo6[:M].astype(np.float64) * gr.LO_UNIT)
        for ks in SLICES:
            buf = torch.full(((ks + 1) * M * ldy + 2 * ldy,), NAN32, dtype=torch.int32, device=DEV)
            n.gemm_w4_rows(ci, si, xh, xl, M, N, K, n.EPI_STORE, y=buf, ldy=ldy, kslices=ks)
            body = buf[:(ks + 1) * M * ldy].view(ks + 1, M, ldy)
            got = body[:ks, :, :N].contiguous().view(torch.float32)
            total = torch.zeros((M, N), dtype=torch.float32, device=DEV)
            want = torch.zeros((M, N), dtype=torch.float32, device=DEV)
            for s in range(ks):
                ref = refs[ks][s][:M]
                assert torch.equal(got[s], ref), ("slab", s, M, N, K, ks, int((got[s] != ref).sum()))
                total += got[s]
                want += ref
            assert torch.equal(total, want) and torch.equal(want, sum(r[:M] for r in refs[1])), ("sum", M, N, K, ks)
            assert bool((body[:ks, :, N:] == NAN32).all()), ("guard behind N", M, N, K, ks)
            assert bool((body[ks] == NAN32).all()), ("slab behind kslices", M, N, K, ks)
            assert bool((buf[(ks + 1) * M * ldy:] == NAN32).all()), ("guard behind the slabs", M, N, K, ks)


def test_empty_slices_store_zeros():
    """K = 128 is one quad: with kslices = 4 the slices 1..3 own nothing and must still write their slabs (pc_rmsnorm_frag adds
    every slab)."""
    n = _n()
    units, K, M = 3, 128, 33
    N = 16 * units
    ci, si, hi, lo6, refs = _exact_case(units, K)
    xh, xl = _planes(hi[:M], lo6[:M].astype(np.float64) * gr.LO_UNIT)
    y = torch.full((4, M, N), float("nan"), dtype=torch.float32, device=DEV)
    n.gemm_w4_rows(ci, si, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N, kslices=4)
    assert torch.equal(y[0], refs[1][0][:M])
    assert bool((y[1:] == 0).all())


# ---------------------------------------------------------------------------------------------------
# the same bits as pc_gemm_w4, row by row; row independence across M
# ---------------------------------------------------------------------------------------------------

EQ_ROWS = (0, 15, 16, 37, 63)


@pytest.mark.parametrize("K", [1152, 2560])
def test_store_rows_are_bit_equal_to_pc_gemm_w4(K):
    n = _n()
    M, N = 64, 1040                                     # 65 tiles: the last workgroup holds clamped duplicates
    xn, wn = gr.gaussian_operands(M, N, K, 81)
    ci, si = n.to_weight_frags_w4(*n.quantize_mxfp4(_dev(wn)))
    xh, xl = n.to_act_frags(_dev(xn))
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    n.gemm_w4_rows(ci, si, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N)
    for r in EQ_ROWS:
        h1, l1 = n.to_act_frags(_dev(xn[r:r + 1]))
        y1 = torch.full((1, N), float("nan"), dtype=torch.float32, device=DEV)
        n.gemm_w4(ci, si, 1, N, K, n.EPI_STORE, xf_hi=h1, xf_lo=l1, y=y1, ldy=N)
        assert torch.equal(y1[0], y[r]), (r, int((y1[0] != y[r]).sum()))


def test_silu_rows_are_bit_equal_to_pc_gemm_w4():
    n = _n()
    M, inter, K = 64, 544, 1152                         # 34 gate/up pairs: 17 workgroups
    N = 2 * inter
    xn, wn = gr.gaussian_operands(M, N, K, 83)
    ci, si = n.to_weight_frags_w4(*n.quantize_mxfp4(_dev(wn)))
    xh, xl = n.to_act_frags(_dev(xn))
    oh = torch.zeros((4, inter // 32, 64, 8), dtype=torch.float16, device=DEV)
    ol = torch.zeros_like(oh)
    n.gemm_w4_rows(ci, si, xh, xl, M, N, K, n.EPI_SILU, of_hi=oh, of_lo=ol)
    gh, gl = n.from_act_frags(oh, M), n.from_act_frags(ol, M)
    assert float((gl != 0).float().mean()) > 0.5
    for r in EQ_ROWS:
        h1, l1 = n.to_act_frags(_dev(xn[r:r + 1]))
        o1h = torch.zeros((1, inter // 32, 64, 8), dtype=torch.float16, device=DEV)
        o1l = torch.zeros_like(o1h)
        n.gemm_w4(ci, si, 1, N, K, n.EPI_SILU, xf_hi=h1, xf_lo=l1, of_hi=o1h, of_lo=o1l)
        assert torch.equal(n.from_act_frags(o1h, 1)[0], gh[r]) and torch.equal(n.from_act_frags(o1l, 1)[0], gl[r]), r


@pytest.mark.parametrize("ks", SLICES)
def test_rows_do_not_depend_on_m(ks):
    """Rows 0..16 of the 64-row launch against the 17-row launch of the same rows, slab by slab (Gaussian operands: the sums are
    not exact, so equality means the same summation order)."""
    n = _n()
    N, K = 272, 1152
    xn, wn = gr.gaussian_operands(64, N, K, 85)
    ci, si = n.to_weight_frags_w4(*n.quantize_mxfp4(_dev(wn)))
    out = {}
    for M in (64, 17):
        xh, xl = n.to_act_frags(_dev(xn[:M]))
        y = torch.full((ks, M, N), float("nan"), dtype=torch.float32, device=DEV)
        n.gemm_w4_rows(ci, si, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N, kslices=ks)
        out[M] = y
    assert not bool(torch.isnan(out[64]).any())
    assert torch.equal(out[64][:, :17], out[17]), int((out[64][:, :17] != out[17]).sum())


# ---------------------------------------------------------------------------------------------------
# split precision: Gaussian operands against floor16 / 32
# ---------------------------------------------------------------------------------------------------

def _report(family, M, N, K, err, floor16):
    print(f"SPLIT_FLOOR family=w4_rows_{family} M={M} N={N} K={K} err={err:.4e} floor16={floor16:.4e} ratio={err / floor16:.4e}")


def _gauss(M, N, K, seed):
    xn, wn = gr.gaussian_operands(M, N, K, seed)
    codes, exps = mx.quantize(wn)
    return xn, mx.dequantize(codes, exps), _n().to_weight_frags_w4(_dev(codes), _dev(exps))


@pytest.mark.parametrize("M,K", [(17, 384), (64, 2560)])
def test_split_precision_store(M, K):
    n = _n()
    N = 80
    xn, wd, (ci, si) = _gauss(M, N, K, 91)
    ref, floor16 = gr.split_floor(xn, wd)
    xh, xl = n.to_act_frags(_dev(xn))
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    n.gemm_w4_rows(ci, si, xh, xl, M, N, K, n.EPI_STORE, y=y, ldy=N)
    err = float((y.double() - _dev(ref)).abs().max())
    _report("store", M, N, K, err, floor16)
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)


@pytest.mark.parametrize("M", [17, 64])
@pytest.mark.parametrize("inter", [32, 96])
def test_split_precision_silu_epilogue(inter, M):
    """of_hi + of_lo against fp64 with floor16 = max |fp16(ref) - ref| and the planes' consistency, as
    tests/test_gpu_w4.py::test_split_precision_silu_epilogue states them; inter / 16 = 2 and 6: one and three pairs, two per
    workgroup."""
    n = _n()
    N, K = 2 * inter, 256
    mt = (M + 15) // 16
    xn, wd, (ci, si) = _gauss(M, N, K, 93)
    oh = torch.zeros((mt, inter // 32, 64, 8), dtype=torch.float16, device=DEV)
    ol = torch.zeros_like(oh)
    z = _dev(xn).double() @ _dev(wd).t()
    xh, xl = n.to_act_frags(_dev(xn))
    n.gemm_w4_rows(ci, si, xh, xl, M, N, K, n.EPI_SILU, of_hi=oh, of_lo=ol)
    g, u = z[:, :inter], z[:, inter:]
    ref = g / (1 + torch.exp(-g)) * u
    floor16 = float((ref.half().double() - ref).abs().max())
    h, l = n.from_act_frags(oh, M), n.from_act_frags(ol, M)
    err = float((h.double() + l.double() - ref).abs().max())
    _report("silu", M, N, K, err, floor16)
    hf, lf = h.float(), l.float()
    half_ulp = torch.where(hf.abs() < 2.0 ** -14, torch.full_like(hf, 2.0 ** -25), torch.exp2(torch.frexp(hf).exponent.float() - 12))
    off = h != (hf + lf).half()
    assert bool((lf.abs() <= half_ulp).all()), "of_lo exceeds half an ulp of of_hi"
    assert bool((lf.abs()[off] == half_ulp[off]).all()), "of_hi is not a nearest fp16 of of_hi + of_lo"
    assert float((l != 0).float().mean()) > 0.5
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)
    full = n.from_act_frags(oh, 16 * mt)                # pad rows of the output planes are never written
    assert bool((full[M:] == 0).all())


# ---------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing():
    n = _n()
    N, K = 64, 128
    codes, exps, _ = mx.exact_weight(N, K, 950)
    ci, si = n.to_weight_frags_w4(_dev(codes), _dev(exps))
    xh, xl = n.to_act_frags(torch.zeros((80, K), device=DEV))
    y = torch.full((9, 80, N), float("nan"), dtype=torch.float32, device=DEV)
    oh = torch.full((5, N // 64, 64, 8), float("nan"), dtype=torch.float16, device=DEV)
    ol = oh.clone()
    cases = (dict(M=0), dict(M=65), dict(K=96), dict(kslices=0), dict(kslices=9), dict(epi=n.EPI_SILU, kslices=2), dict(ci=None),
             dict(si=None), dict(struct_bytes=8), dict(epi=n.EPI_ADD))
    for kw in cases:
        a = dict(ci=ci, si=si, M=32, K=K, kslices=1, epi=n.EPI_STORE, struct_bytes=None)
        a.update(kw)
        with pytest.raises(RuntimeError, match="code -1001"):
            n.gemm_w4_rows(a["ci"], a["si"], xh, xl, a["M"], N, a["K"], a["epi"], y=y, ldy=N, of_hi=oh, of_lo=ol,
                           kslices=a["kslices"], struct_bytes=a["struct_bytes"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(oh).all()) and bool(torch.isnan(ol).all())
