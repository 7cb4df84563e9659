"""MXFP4 weights on the host (no GPU): the quantiser against the numpy restatement (tests/mxfp4_ref.py) bit for bit, the
exactness of dequantisation, the two images pc_gemm_w4 reads, the headroom of the integer operands tests/test_gpu_w4.py uses,
the args struct against the C compiler and the kernels of csrc/pc_gemm_w4.hip in the built library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import gemm_ref as gr
from tests import mxfp4_ref as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n():
    from promptcache_amd import _native
    return _native


def _quant(w):
    c, e = _n().quantize_mxfp4(torch.from_numpy(np.ascontiguousarray(w)))
    return c.numpy(), e.numpy()


def _same(w):
    c, e = _quant(w)
    cr, er = mx.quantize(w)
    assert c.dtype == np.uint8 and e.dtype == np.uint8 and c.shape == cr.shape and e.shape == er.shape
    assert np.array_equal(e, er), "block exponents differ"
    assert np.array_equal(c, cr), int((c != cr).sum())
    return c, e


@pytest.mark.parametrize("sigma", [0.02, 0.05, 1.0])
def test_quantiser_equals_the_restatement_on_gaussian_rows(sigma):
    w = (sigma * np.random.default_rng(7).standard_normal((48, 512), dtype=np.float32)).astype(np.float16)
    c, e = _same(w)
    assert len(np.unique(e)) > 1 and len(np.unique(c)) > 100          # (the draw exercises several exponents and all codes)


def _block(vals, fill=0.0):
    b = np.full(32, fill, dtype=np.float32)
    b[:len(vals)] = vals
    return b


def test_hand_made_blocks():
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=np.float32)
    tie_codes = [0, 2, 2, 4, 4, 6, 6]                                   # the even code of each pair of neighbours
    blocks, want_e, want_first = [], [], []
    blocks.append(_block([])); want_e.append(0); want_first.append([0])                        # all zero
    blocks.append(_block([4.0, -4.0])); want_e.append(0); want_first.append([6, 14])           # amax a power of two: v = 4
    for ex in (-3, 0, 5):                                                                      # exact ties, amax = 6 * 2^ex
        blocks.append(_block(np.concatenate(([6.0], ties, -ties)) * 2.0 ** ex)); want_e.append(ex)
        want_first.append([7] + tie_codes + [c + 8 if c else 0 for c in tie_codes])
    # |v| in (6, 8): amax = 7.5 keeps e = 0 (floor(log2 7.5) = 2), saturates to code 7
    blocks.append(_block([7.5, -6.5, 7.99])); want_e.append(0); want_first.append([7, 15, 7])
    # a negative value that rounds to zero is code 0, never 8
    blocks.append(_block([4.0, -0.2, -0.25, -0.26])); want_e.append(0); want_first.append([6, 0, 0, 9])
    # exponent clamps: amax below 2^-11 (e = -13) and above 2^16 (e = 13, saturating)
    blocks.append(_block([2.0 ** -13, -(2.0 ** -14), 2.0 ** -15])); want_e.append(-13); want_first.append([2, 9, 0])
    blocks.append(_block([2.0 ** 17, -(2.0 ** 15), 2.0 ** 13])); want_e.append(13); want_first.append([7, 14, 2])
    w = np.stack(blocks).astype(np.float32)
    c, e = _same(w)
    assert list(e[:, 0].astype(int) - 127) == want_e
    codes = np.stack((c & 15, c >> 4), axis=2).reshape(len(blocks), 32)
    for i, first in enumerate(want_first):
        assert list(codes[i, :len(first)]) == first, (i, list(codes[i, :len(first)]), first)
    assert not (codes == 8).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_weights_are_refused(bad):
    w = np.ones((16, 128), dtype=np.float32)
    w[3, 77] = bad
    with pytest.raises(ValueError):
        _quant(w)
    with pytest.raises(ValueError):
        mx.quantize(w)


@pytest.mark.parametrize("sigma", [0.02, 0.05, 1.0])
def test_dequantisation_is_fp16_exact_and_the_quantiser_idempotent(sigma):
    n = _n()
    w = (sigma * np.random.default_rng(11).standard_normal((32, 256), dtype=np.float32)).astype(np.float16)
    c, e = n.quantize_mxfp4(torch.from_numpy(w))
    d = n.dequantize_mxfp4(c, e)
    ref = mx.dequantize(c.numpy(), e.numpy())
    assert d.dtype == torch.float16 and np.array_equal(d.numpy().astype(np.float64), ref)      # nothing lost in fp16
    assert np.array_equal(ref.astype(np.float16).astype(np.float64), ref)
    a = np.abs(ref[ref != 0])
    assert a.min() >= 2.0 ** -14                                                               # normals only
    c2, e2 = n.quantize_mxfp4(d)
    assert torch.equal(c2, c) and torch.equal(e2, e)
    rel = np.sqrt(((ref - w.astype(np.float64)) ** 2).mean() / (w.astype(np.float64) ** 2).mean())
    print(f"MXFP4_RMS sigma={sigma} rel_rms={rel:.4f}")
    assert 0.05 < rel < 0.2


def test_image_round_trip_on_an_asymmetric_matrix():
    n = _n()
    rng = np.random.default_rng(3)
    N, K = 48, 384
    codes = rng.integers(0, 256, size=(N, K // 2), dtype=np.uint8)
    exps = rng.integers(114, 141, size=(N, K // 32), dtype=np.uint8)
    ci, si = n.to_weight_frags_w4(torch.from_numpy(codes), torch.from_numpy(exps))
    assert tuple(ci.shape) == (N // 16, K // 128, 64, 16) and ci.is_contiguous() and si.is_contiguous()
    cr, sr = mx.pack_images(codes, exps)
    assert np.array_equal(ci.numpy(), cr) and np.array_equal(si.numpy().reshape(sr.shape), sr)
    c2, e2 = n.from_weight_frags_w4(ci, si)
    assert np.array_equal(c2.numpy(), codes) and np.array_equal(e2.numpy(), exps)
    with pytest.raises(ValueError):
        n.to_weight_frags_w4(torch.from_numpy(codes[:, :48]), torch.from_numpy(exps[:, :3]))   # K = 96


def test_headroom_of_the_integer_operands():
    """2 W' is an integer of magnitude <= 24, 2^6 (hi + lo) one of magnitude <= 128: every product is a multiple of 2^-7 and
    every partial sum over at most K terms stays below 24 * 128 * K units -- below 2^23 up to K = 2560, so every fp32 addition
    in any order is exact and the only correct result is the int64 one."""
    K = 2560
    assert 24 * 128 * K < 2 ** 23 <= 24 * 128 * (K + 256)
    codes, exps, w2 = mx.exact_weight(32, K, 1)
    assert np.array_equal(mx.quantize(mx.dequantize(codes, exps))[0], codes)      # a fixed point of the quantiser
    assert np.abs(w2).max() == 24 and np.array_equal(w2 * 0.5, mx.dequantize(codes, exps))
    hi, lo6 = gr.exact_planes(16, K, 2, True)
    x6 = hi * 64 + lo6
    assert np.abs(x6).max() <= 128
    worst = (np.abs(x6) @ np.abs(w2).T).max()
    assert worst < 2 ** 23
    # fp32, one term after the other, planes interleaved: equal to the int64 sum
    wd = (w2 * 0.5).astype(np.float16)
    got = gr.fp32_k_order((hi.astype(np.float16), (lo6 * gr.LO_UNIT).astype(np.float16)), wd[:, :640])[:, :]
    ref = ((x6[:, :640] @ w2[:, :640].T).astype(np.float64) * 2.0 ** -7).astype(np.float32)
    assert np.array_equal(got, ref)


def test_w4_args_layout_matches_the_header(tmp_path):
    n = _n()
    cls, st = n.GemmW4Args, "pc_gemm_w4_args"
    assert cls._fields_[0][0] == "struct_bytes"
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {',
            f'  printf("{st} %zu\\n", sizeof({st}));']
    for f, _ in cls._fields_:
        body.append(f'  printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    body += ['  return 0;', '}']
    src = tmp_path / "layout_w4.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout_w4"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got[st]) == ctypes.sizeof(cls)
    for name, _ in cls._fields_:
        assert int(got[f"{st}.{name}"]) == getattr(cls, name).offset, name
    assert "pc_gemm_w4" in n.SIGNATURES


def test_the_w4_kernels_are_in_the_library():
    from promptcache_amd import codeobj
    n = _n()
    names = [r["demangled"] for r in codeobj.kernels(n.lib_path()) if "gemm_w4_kernel" in r["demangled"]]
    assert 1 <= len(names) <= 14, names
    for must in ("gemm_w4_kernel<1, 0, false>", "gemm_w4_kernel<1, 1, false>", "gemm_w4_kernel<1, 2, false>",
                 "gemm_w4_kernel<4, 0, true>", "gemm_w4_kernel<3, 2, true>"):
        assert any(must in x for x in names), must


def test_argument_errors_need_no_gpu():
    """M = 17, K = 96 and null images return PC_ERR_ARG before anything is launched."""
    n = _n()
    lib = n.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf) & ~15
    def call(**kw):
        a = n.GemmW4Args()
        a.struct_bytes = ctypes.sizeof(n.GemmW4Args)
        base = dict(epilogue=n.EPI_STORE, codes=p + 16, scales=p + 16, xf_hi=p + 16, xf_lo=p + 16, M=16, N=16, K=128, y=p + 16, ldy=16)
        base.update(kw)
        for k, v in base.items():
            setattr(a, k, v)
        return lib.pc_gemm_w4(ctypes.byref(a), None)
    assert call(M=17) == -1001 and b"M=17" in lib.pc_last_error_string()
    assert call(K=96) == -1001
    assert call(codes=None) == -1001 and call(scales=None) == -1001
    assert call(epilogue=n.EPI_QKV_ROPE) == -1001
    a = n.GemmW4Args()
    assert lib.pc_gemm_w4(ctypes.byref(a), None) == -1001                 # struct_bytes = 0: ABI mismatch
