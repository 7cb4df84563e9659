"""pc_gemm_w4 (csrc/pc_gemm_w4.hip): the <= 16-row projections over MXFP4 weight images.

* Conversion probe: every code under every block exponent, one-hot activation rows -- the output IS the dequantised weight,
  bit for bit.  Settles the nibble order, the scale operand and the absence of fp16 flushing.
* Exact sums: integer operands (tests/mxfp4_ref.exact_weight against tests/gemm_ref.exact_planes; the headroom is re-derived in
  tests/test_mxfp4_cpu.py): ``torch.equal`` against the int64 sum, NaN in the pad rows, guards behind the outputs, rows_dev.
* Split-precision floor (Gaussian operands, ``max |got - ref| <= floor16 / 32``, both sides from the reference alone): plain
  store, the norm-folded source, the SiLU epilogue -- the way tests/test_gpu_gemm_exact.py holds pc_gemm.
* Row independence: row r of a 16-row launch is bit-equal to the one-row launch of that row.
"""
import numpy as np
import pytest
import torch

from tests import gemm_ref as gr
from tests import mxfp4_ref as mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN32 = 0x7FC12345


def _n():
    from promptcache_amd import _native
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _images(codes, exps):
    return _n().to_weight_frags_w4(_dev(codes), _dev(exps))


def _planes(hi, lo, tiles=1):
    """fp16 [M][K] planes -> device fragment planes, NaN in the pad rows."""
    def one(v):
        full = np.full((16 * tiles, v.shape[1]), np.nan, dtype=np.float16)
        full[:v.shape[0]] = v
        return _dev(gr.pack_plane(full))
    return one(hi), one(lo)


def _int_planes(M, K, seed):
    hi, lo6 = gr.exact_planes(M, K, seed, True)
    return hi, lo6, _planes(hi.astype(np.float16), (lo6.astype(np.float64) * gr.LO_UNIT).astype(np.float16))


def _ref(hi, lo6, w2):
    """Exact fp32 [M][N]: (64 hi + lo6) . (2 W')^T in int64, scaled by 2^-7 once."""
    return _dev((((hi * 64 + lo6) @ w2.T).astype(np.float64) * 2.0 ** -7).astype(np.float32))


def _guarded(rows, ldy):
    return torch.full(((rows + 2) * ldy,), NAN32, dtype=torch.int32, device=DEV)


def _guards_intact(buf, rows, N, ldy):
    g = buf.view(rows + 2, ldy)
    return bool((g[:rows, N:] == NAN32).all()) and bool((g[rows:] == NAN32).all())


def _ints(shape, seed, lim=8):
    return _dev(np.random.default_rng(seed).integers(-lim, lim + 1, size=shape).astype(np.float32))


# ---------------------------------------------------------------------------------------------------
# conversion probe
# ---------------------------------------------------------------------------------------------------

def test_conversion_probe_every_code_under_every_exponent():
    """K = 128, N = 432: row n has block exponent n // 16 - 13 in every block and every block holds all 16 codes, rotated by the
    row and the block.  M = 16 one-hot rows, eight launches cover the 128 features: y[m][n] == W'[n][k_m] bit for bit (the sum
    has one non-zero term)."""
    n = _n()
    N, K, M = 432, 128, 16
    rows = np.arange(N)[:, None]
    nib = ((np.arange(K)[None, :] + 3 * rows + 5 * (np.arange(K)[None, :] // 32)) % 16).astype(np.uint8)
    n2 = nib.reshape(N, K // 2, 2)
    codes = (n2[:, :, 0] | (n2[:, :, 1] << 4)).astype(np.uint8)
    exps = np.repeat((rows // 16 - 13 + 127).astype(np.uint8), K // 32, axis=1)
    wd = mx.dequantize(codes, exps)
    assert np.array_equal(wd.astype(np.float16).astype(np.float64), wd) and np.abs(wd[wd != 0]).min() == 2.0 ** -14
    assert np.array_equal(_n().dequantize_mxfp4(_dev(codes), _dev(exps)).cpu().numpy().astype(np.float64), wd)
    ci, si = _images(codes, exps)
    want = _dev(wd.astype(np.float32))
    seen = torch.zeros((N, K), dtype=torch.bool, device=DEV)
    for i in range(K // M):
        hi = np.zeros((M, K), dtype=np.float16)
        hi[np.arange(M), M * i + np.arange(M)] = 1.0
        xh, xl = _planes(hi, np.zeros_like(hi))
        y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
        n.gemm_w4(ci, si, M, N, K, n.EPI_STORE, xf_hi=xh, xf_lo=xl, y=y, ldy=N)
        ref = want[:, M * i:M * (i + 1)].t().contiguous()
        bad = (y != ref)
        assert not bool(bad.any()), (i, int(bad.sum()), y[bad][:4].tolist(), ref[bad][:4].tolist())
        seen[:, M * i:M * (i + 1)] = True
    assert bool(seen.all())


# ---------------------------------------------------------------------------------------------------
# exact sums
# ---------------------------------------------------------------------------------------------------

EXACT_ROWS = (1, 5, 12, 16)
EXACT_K = (128, 384, 1152, 2560)      # K / 128 = 1, 3, 9, 20: waves with nothing, one quad each, a tail, blocks + tail


@pytest.mark.parametrize("units", [1, 3, 9, 257, 515])
def test_exact_store_and_add(units):
    """N / 16 = 1, 3, 9 (one tile per workgroup), 257 (two, the last workgroup with a clamped duplicate), 515 (four under the
    store epilogue; K = 128 and 1152 there: one quad in one wave, and full blocks with a tail): STORE and ADD are torch.equal to the int64 reference for every row count and K."""
    n = _n()
    N = 16 * units
    for K in (EXACT_K if units != 515 else (128, 1152)):
        codes, exps, w2 = mx.exact_weight(N, K, 300 + units)
        ci, si = _images(codes, exps)
        for M in EXACT_ROWS:
            hi, lo6, (xh, xl) = _int_planes(M, K, 400 + units)
            ref = _ref(hi, lo6, w2)
            y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
            n.gemm_w4(ci, si, M, N, K, n.EPI_STORE, xf_hi=xh, xf_lo=xl, y=y, ldy=N)
            assert torch.equal(y, ref), ("store", M, N, K, int((y != ref).sum()))
            y0 = _ints((M, N), M + K)
            y2 = y0.clone()
            n.gemm_w4(ci, si, M, N, K, n.EPI_ADD, xf_hi=xh, xf_lo=xl, y=y2, ldy=N)
            assert torch.equal(y2, y0 + ref), ("add", M, N, K, int((y2 != y0 + ref).sum()))


@pytest.mark.parametrize("M", [5, 16])
def test_output_geometry_ldy_and_guards(M):
    n = _n()
    N, K, ldy = 144, 384, 148
    codes, exps, w2 = mx.exact_weight(N, K, 500)
    ci, si = _images(codes, exps)
    hi, lo6, (xh, xl) = _int_planes(M, K, 501)
    ref = _ref(hi, lo6, w2)
    y0 = _ints((M, N), 502)
    for epi in (n.EPI_STORE, n.EPI_ADD):
        buf = _guarded(M, ldy)
        yv = buf.view(torch.float32).view(M + 2, ldy)
        if epi == n.EPI_ADD:
            yv[:M, :N] = y0
        n.gemm_w4(ci, si, M, N, K, epi, xf_hi=xh, xf_lo=xl, y=buf, ldy=ldy)
        assert torch.equal(yv[:M, :N], ref + y0 if epi == n.EPI_ADD else ref), (M, epi)
        assert _guards_intact(buf, M, N, ldy), (M, epi)


def test_rows_dev_limits_the_live_rows():
    """Rows < live are bit-equal to the exact sums while the plane rows >= live hold NaN; a value above M clamps to M; the guard
    rows behind M stay untouched."""
    n = _n()
    M, N, K = 16, 144, 384
    codes, exps, w2 = mx.exact_weight(N, K, 600)
    ci, si = _images(codes, exps)
    hi, lo6 = gr.exact_planes(M, K, 601, True)
    y0 = _ints((M, N), 602)
    for live in (1, 13, 16, 21):
        rows = min(live, M)
        rd = torch.tensor([live], dtype=torch.int32, device=DEV)
        xh, xl = _planes(hi[:rows].astype(np.float16), (lo6[:rows].astype(np.float64) * gr.LO_UNIT).astype(np.float16))
        ref = _ref(hi[:rows], lo6[:rows], w2)
        for epi in (n.EPI_STORE, n.EPI_ADD):
            buf = _guarded(M, N)
            ya = buf.view(torch.float32).view(M + 2, N)
            ya[:M] = y0
            n.gemm_w4(ci, si, M, N, K, epi, xf_hi=xh, xf_lo=xl, y=buf, ldy=N, rows_dev=rd)
            assert torch.equal(ya[:rows], ref + y0[:rows] if epi == n.EPI_ADD else ref), (live, epi)
            assert bool((buf.view(M + 2, N)[M:] == NAN32).all()), (live, epi)


@pytest.mark.parametrize("epi_name", ["store", "add"])
def test_row_independence(epi_name):
    """Row r of an M = 16 launch is bit-equal to the M = 1 launch of that row (Gaussian operands: the sums are NOT exact, so
    equality means the same summation order)."""
    n = _n()
    N, K = 4112, 1152                                   # two tiles per workgroup, a K tail
    epi = n.EPI_STORE if epi_name == "store" else n.EPI_ADD
    xn, wn = gr.gaussian_operands(16, N, K, 71)
    ci, si = n.to_weight_frags_w4(*n.quantize_mxfp4(_dev(wn)))
    y0 = torch.randn((16, N), dtype=torch.float32, device=DEV)
    xh, xl = n.to_act_frags(_dev(xn))
    y = y0.clone()
    n.gemm_w4(ci, si, 16, N, K, epi, xf_hi=xh, xf_lo=xl, y=y, ldy=N)
    for r in (0, 7, 15):
        h1, l1 = n.to_act_frags(_dev(xn[r:r + 1]))
        y1 = y0[r:r + 1].clone()
        n.gemm_w4(ci, si, 1, N, K, epi, xf_hi=h1, xf_lo=l1, y=y1, ldy=N)
        assert torch.equal(y1[0], y[r]), (r, int((y1[0] != y[r]).sum()))


# ---------------------------------------------------------------------------------------------------
# split precision: Gaussian operands against floor16 / 32
# ---------------------------------------------------------------------------------------------------

def _report(family, M, N, K, err, floor16):
    print(f"SPLIT_FLOOR family=w4_{family} M={M} N={N} K={K} err={err:.4e} floor16={floor16:.4e} ratio={err / floor16:.4e}")


def _gauss(M, N, K, seed, x_scale=1.0):
    """x fp32 [M][K], W' float64 [N][K] (the restatement's dequantised weight) and the device images of the same codes.  (Above
    2^22 weights the codes come from the device quantiser, which tests/test_mxfp4_cpu.py holds bit-equal to the restatement.)"""
    xn, wn = gr.gaussian_operands(M, N, K, seed, x_scale)
    if N * K > (1 << 22):
        codes, exps = (t.cpu().numpy() for t in _n().quantize_mxfp4(_dev(wn)))
    else:
        codes, exps = mx.quantize(wn)
    return xn, mx.dequantize(codes, exps), _images(codes, exps)


@pytest.mark.parametrize("K", [128, 512, 1024])
@pytest.mark.parametrize("M", [1, 12, 16])
def test_split_precision_store(M, K):
    n = _n()
    N = 80
    assert K <= gr.SPLIT_K_MAX
    xn, wd, (ci, si) = _gauss(M, N, K, 41)
    ref, floor16 = gr.split_floor(xn, wd)
    xh, xl = n.to_act_frags(_dev(xn))
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    n.gemm_w4(ci, si, M, N, K, n.EPI_STORE, xf_hi=xh, xf_lo=xl, y=y, ldy=N)
    err = float((y.double() - _dev(ref)).abs().max())
    _report("store", M, N, K, err, floor16)
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)


@pytest.mark.parametrize("M,N,K", [(1, 48, 128), (12, 80, 1024), (16, 4112, 512), (5, 8240, 128), (12, 8240, 512)])
def test_split_precision_norm_folded_source(M, N, K):
    """The norm source against fp64 RMSNorm followed by the product; floor16 is taken on fp16(normed x).  N / 16 = 3, 5, 257, 515:
    one, two and four tiles per workgroup."""
    n = _n()
    xn, wd, (ci, si) = _gauss(M, N, K, 43, 3.0)
    gain = (1.0 + 0.2 * np.random.default_rng(5).standard_normal(K, dtype=np.float32)).astype(np.float16)
    eps = 1e-5
    normed = gr.rmsnorm64(xn, gain, eps)
    ref = normed @ wd.T
    floor16 = float(np.abs(normed.astype(np.float16).astype(np.float64) @ wd.T - ref).max())
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    n.gemm_w4(ci, si, M, N, K, n.EPI_STORE, x=_dev(xn), norm_weight=_dev(gain), eps=eps, y=y, ldy=N)
    err = float((y.double() - _dev(ref)).abs().max())
    _report("norm", M, N, K, err, floor16)
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,inter,K", [(3, 64, 256), (12, 4128, 128), (16, 8256, 128), (12, 8224, 512)])
def test_split_precision_silu_epilogue(M, inter, K, norm):
    """of_hi + of_lo against fp64 with floor16 = max |fp16(ref) - ref|, from the planes or the norm source (inter / 16 = 4, 258,
    516, 514 at K = 512: one, two and three pairs per workgroup under the norm source), and the planes' consistency as
    tests/test_gpu_gemm_exact.py states it."""
    n = _n()
    N = 2 * inter
    xn, wd, (ci, si) = _gauss(M, N, K, 47)
    oh = torch.zeros((1, inter // 32, 64, 8), dtype=torch.float16, device=DEV)
    ol = torch.zeros_like(oh)
    if norm:
        gain = (1.0 + 0.2 * np.random.default_rng(6).standard_normal(K, dtype=np.float32)).astype(np.float16)
        z = _dev(gr.rmsnorm64(xn, gain, 1e-5)) @ _dev(wd).t()
        n.gemm_w4(ci, si, M, N, K, n.EPI_SILU, x=_dev(xn), norm_weight=_dev(gain), eps=1e-5, of_hi=oh, of_lo=ol)
    else:
        z = _dev(xn).double() @ _dev(wd).t()
        xh, xl = n.to_act_frags(_dev(xn))
        n.gemm_w4(ci, si, M, N, K, n.EPI_SILU, xf_hi=xh, xf_lo=xl, of_hi=oh, of_lo=ol)
    g, u = z[:, :inter], z[:, inter:]
    ref = g / (1 + torch.exp(-g)) * u
    floor16 = float((ref.half().double() - ref).abs().max())
    h, l = n.from_act_frags(oh, M), n.from_act_frags(ol, M)
    err = float((h.double() + l.double() - ref).abs().max())
    _report("silu_norm" if norm else "silu", M, N, K, err, floor16)
    hf, lf = h.float(), l.float()
    half_ulp = torch.where(hf.abs() < 2.0 ** -14, torch.full_like(hf, 2.0 ** -25), torch.exp2(torch.frexp(hf).exponent.float() - 12))
    off = h != (hf + lf).half()
    assert bool((lf.abs() <= half_ulp).all()), "of_lo exceeds half an ulp of of_hi"
    assert bool((lf.abs()[off] == half_ulp[off]).all()), "of_hi is not a nearest fp16 of of_hi + of_lo"
    assert float((l != 0).float().mean()) > 0.5
    assert err <= floor16 / gr.SPLIT_RULE, (err / floor16)
    # pad rows of the output planes are never written
    full = n.from_act_frags(oh, 16)
    assert bool((full[M:] == 0).all())


# ---------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing():
    n = _n()
    N, K = 48, 128
    codes, exps, _ = mx.exact_weight(N, K, 700)
    ci, si = _images(codes, exps)
    xh, xl = n.to_act_frags(torch.zeros((32, K), device=DEV))
    y = torch.full((32, N), float("nan"), dtype=torch.float32, device=DEV)
    for kw in (dict(M=17), dict(K=96), dict(ci=None), dict(si=None)):
        a = dict(ci=ci, si=si, M=16, K=K)
        a.update(kw)
        with pytest.raises(RuntimeError, match="code -1001"):
            n.gemm_w4(a["ci"], a["si"], a["M"], N, a["K"], n.EPI_STORE, xf_hi=xh, xf_lo=xl, y=y, ldy=N)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ---------------------------------------------------------------------------------------------------
# pc_rope_append_ex behind the plain q|k|v store: residual row offsets read on the device
# ---------------------------------------------------------------------------------------------------

def test_rope_append_ex_reads_the_residual_row_offset_from_the_device():
    """lo_row0 = -1 (this pass's rows) and -2 (past_len_dev[1], a tail's base) against the host forms, bit for bit -- also when the
    host's past_len is not the device's (a captured graph replayed at another past length); nothing else is written."""
    n = _n()
    B, H, Hkv, D, q_len, past, cap, base = 1, 4, 2, 64, 5, 7, 32, 3
    W = (H + 2 * Hkv) * D
    qkv = torch.randn((q_len, W), dtype=torch.float32, device=DEV)
    cs = torch.empty((q_len, D // 2, 2), dtype=torch.float32, device=DEV)
    n.rope_table(torch.arange(40, 40 + q_len, dtype=torch.int32, device=DEV), 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=DEV).float() / D)), cs, q_len, D)

    def run(lo_row0, host_past, words, rows):
        arena = torch.full((2, B, Hkv, cap, D), 77.0, dtype=torch.float16, device=DEV)
        lo = torch.full((2, B, Hkv, rows, D), 77.0, dtype=torch.float16, device=DEV)
        q = torch.full((q_len, H * D), 77.0, dtype=torch.float16, device=DEV)
        ql = torch.full_like(q, 77.0)
        pd = None if words is None else torch.tensor(words, dtype=torch.int32, device=DEV)
        n.rope_append(qkv, q_len * W, W, q, q_len * H * D, H * D, qkv[:, H * D:], qkv[:, (H + Hkv) * D:], q_len * W, W, arena[0], arena[1],
                      Hkv * cap * D, cap * D, cs, B, H, Hkv, D, q_len, host_past, cap, True, past_len_dev=pd, q_out_lo=ql,
                      kv_lo=(lo[0], lo[1], Hkv * rows * D, rows * D, lo_row0))
        return [t.view(torch.int16) for t in (q, ql, arena, lo)]

    own = run(past, past, None, q_len + 2)                       # host form: compact rows of this pass
    assert bool((own[3][:, :, :, q_len:] == own[3][0, 0, 0, q_len, 0]).all()) and bool((own[3][:, :, :, :q_len] != own[3][0, 0, 0, q_len, 0]).any())
    for host_past, words in ((past, [past, 0, q_len]), (2, [past, 0, q_len])):
        got = run(-1, host_past, words, q_len + 2)
        assert all(torch.equal(a, b) for a, b in zip(own, got)), (host_past, "lo_row0 = -1")
    rows = past - base + q_len + 2
    tail = run(base, past, None, rows)                           # host form: a tail that started at key `base`
    for host_past in (past, 4):
        got = run(-2, host_past, [past, base, q_len], rows)
        assert all(torch.equal(a, b) for a, b in zip(tail, got)), (host_past, "lo_row0 = -2")
    with pytest.raises(RuntimeError, match="code -1001"):
        run(-2, past, None, rows)                                # -2 needs the device words
    with pytest.raises(RuntimeError, match="code -1001"):
        run(-3, past, [past, base, q_len], rows)
