"""pc_w4_expand (csrc/pc_w4_expand.hip): the fp16 weight W' from the two MXFP4 images of pc_gemm_w4, as the fragment image of
``_native.to_weight_frags`` or row-major.

* Bit equality on quantiser output (``torch.equal`` on int16 views against ``to_weight_frags(W')`` / ``W'``), blocks at the
  exponent clamps -13 / +13 and all-zero blocks included; row-major with ``ld_out = K`` and ``K + 8``, pad columns untouched.
* Every code under every exponent byte 114..140 against tests/mxfp4_ref (by value: code 8 is -0, which the quantiser never emits).
* ``row_perm``: the q|k|v permutation of pc_gemm_qkv_rope and a random one.
* NaN-pattern guards in front of and behind the output; argument errors leave the output untouched.
"""
import functools

import numpy as np
import pytest
import torch

from tests import mxfp4_ref as mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 0x7E55                  # an fp16 NaN pattern
NG = 64                         # guard halves on either side of the output (128 B: the output stays 16-byte aligned)


def _n():
    from promptcache_amd import _native
    return _native


@functools.lru_cache(maxsize=16)
def _case(units, K, seed=0):
    """Gaussian weights, every 5th block pushed to the upper exponent clamp, every 7th to the lower, every 11th zero:
    (code image, scale image, W' fp16 [N][K])."""
    n = _n()
    N = 16 * units
    g = torch.Generator().manual_seed(100 + 7 * units + K + seed)
    w = torch.randn((N, K // 32, 32), generator=g)
    b = torch.arange(N * (K // 32)).view(N, K // 32)
    w[b % 5 == 1] *= 2.0 ** 15            # block exponent 13 or 14 before the clamp: elements saturate
    w[b % 7 == 2] *= 2.0 ** -14           # -15 or -16 before the clamp: elements survive as small codes
    w[b % 11 == 3] = 0.0
    codes, exps = n.quantize_mxfp4(w.view(N, K).to(DEV))
    e = set(exps.unique().tolist())
    assert {127 - 13, 127 + 13} <= e and bool((codes.view(N, K // 32, 16) == 0).all(dim=2).any())
    ci, si = n.to_weight_frags_w4(codes, exps)
    return ci, si, n.dequantize_mxfp4(codes, exps)


def _guarded(numel):
    buf = torch.full((numel + 2 * NG,), GUARD, dtype=torch.int16, device=DEV)
    return buf, buf[NG:NG + numel]


def _guards_intact(buf, numel):
    return bool((buf[:NG] == GUARD).all()) and bool((buf[NG + numel:] == GUARD).all())


def _frag(ci, si, N, K, row_perm=None):
    n = _n()
    buf, out = _guarded(N * K)
    n.w4_expand(ci, si, out, N, K, n.W4_EXPAND_FRAG, row_perm=row_perm)
    torch.cuda.synchronize()
    assert _guards_intact(buf, N * K)
    return out.view(N // 16, K // 32, 4, 16, 8)


@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("units", [1, 3, 257])
def test_bit_equal_to_the_dequantised_weight(units, K):
    n = _n()
    N = 16 * units
    ci, si, wp = _case(units, K)
    got = _frag(ci, si, N, K)
    assert torch.equal(got, n.to_weight_frags(wp).view(torch.int16))
    for ld in (K, K + 8):
        buf, out = _guarded(N * ld)
        n.w4_expand(ci, si, out, N, K, n.W4_EXPAND_ROWMAJOR, ld_out=ld)
        torch.cuda.synchronize()
        assert _guards_intact(buf, N * ld)
        rows = out.view(N, ld)
        assert torch.equal(rows[:, :K], wp.view(torch.int16))
        assert bool((rows[:, K:] == GUARD).all())


def test_every_code_under_every_exponent():
    """16 codes x the 27 exponent bytes 114..140, every code at every position of a lane's eight values; images packed element
    by element from the layout's definition (tests/mxfp4_ref.pack_images), values from tests/mxfp4_ref.dequantize."""
    n = _n()
    N, K = 16, 896                                              # 28 blocks per row: bytes 114..140, then 127 once more
    r, k = np.arange(N)[:, None], np.arange(K)[None, :]
    nib = ((k + 3 * r) % 16).astype(np.uint8)                  # a block of 32 holds every code twice, rotated per row
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    exps = np.broadcast_to(np.where(np.arange(28) < 27, 114 + np.arange(28), 127).astype(np.uint8), (N, 28)).copy()
    seen = {(int(c), 114 + b) for b in range(27) for c in np.unique(nib[:, 32 * b:32 * b + 32])}
    assert len(seen) == 16 * 27
    ci, si = mx.pack_images(codes, exps)
    ci, si = torch.from_numpy(ci).to(DEV), torch.from_numpy(si).to(DEV)
    ref = mx.dequantize(codes, exps)
    assert np.array_equal(ref.astype(np.float16).astype(np.float64), ref)
    ref = torch.from_numpy(ref.astype(np.float32)).to(DEV)
    buf, out = _guarded(N * K)
    n.w4_expand(ci, si, out, N, K, n.W4_EXPAND_ROWMAJOR, ld_out=K)
    torch.cuda.synchronize()
    assert _guards_intact(buf, N * K)
    got = out.view(torch.float16).view(N, K).float()
    assert bool((got == ref).all())                              # by value: -0 == 0
    fr = _frag(ci, si, N, K).view(torch.float16).float()
    assert bool((fr == n.to_weight_frags(ref).view(1, K // 32, 4, 16, 8)).all())


@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2)])
def test_qkv_rope_row_perm(H, Hkv):
    n = _n()
    N, K = (H + 2 * Hkv) * 128, 384
    ci, si, wp = _case(N // 16, K, seed=1)
    perm = n.qkv_rope_row_perm(H + 2 * Hkv, 128).to(DEV)
    got = _frag(ci, si, N, K, row_perm=perm.to(torch.int32).contiguous())
    assert torch.equal(got, n.to_weight_frags(wp[perm].contiguous()).view(torch.int16))


def test_random_row_perm_both_layouts():
    n = _n()
    N, K = 48, 384
    ci, si, wp = _case(3, K)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(4)).to(DEV)
    p32 = perm.to(torch.int32).contiguous()
    assert torch.equal(_frag(ci, si, N, K, row_perm=p32), n.to_weight_frags(wp[perm].contiguous()).view(torch.int16))
    buf, out = _guarded(N * (K + 8))
    n.w4_expand(ci, si, out, N, K, n.W4_EXPAND_ROWMAJOR, ld_out=K + 8, row_perm=p32)
    torch.cuda.synchronize()
    assert _guards_intact(buf, N * (K + 8))
    assert torch.equal(out.view(N, K + 8)[:, :K], wp[perm].view(torch.int16))


def test_argument_errors_leave_the_output_untouched():
    n = _n()
    N, K = 48, 384
    ci, si, _ = _case(3, K)
    buf, out = _guarded(N * (K + 8))
    F, R = n.W4_EXPAND_FRAG, n.W4_EXPAND_ROWMAJOR
    bad = [dict(N=N + 8, K=K, layout=F), dict(N=N, K=K + 32, layout=F), dict(N=N, K=K, layout=2), dict(N=N, K=K, layout=-1),
           dict(N=N, K=K, layout=R, ld_out=K - 8), dict(N=N, K=K, layout=R, ld_out=K + 4), dict(N=N, K=K, layout=R, ld_out=0),
           dict(N=N, K=K, layout=F, struct_bytes=8), dict(N=0, K=K, layout=F), dict(N=N, K=0, layout=F)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="-1001"):
            n.w4_expand(ci, si, out, **kw)
    for c, s, o in ((None, si, out), (ci, None, out), (ci, si, None), (ci.data_ptr() + 8, si, out), (ci, si.data_ptr() + 4, out),
                    (ci, si, out.data_ptr() + 2)):
        with pytest.raises(RuntimeError, match="-1001"):
            n.w4_expand(c, s, o, N, K, F)
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
