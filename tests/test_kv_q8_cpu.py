"""CPU-side checks of the int8 module KV store: the numpy restatement's derived error bound and edge rows, the image layout,
the engine's ``module_kv`` knob, and the C-ABI of the two new entry points (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import kv_q8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(rng, n, D, mag, outliers=True):
    x = (rng.standard_normal((n, D)) * mag).astype(np.float16)
    if outliers:
        with np.errstate(over="ignore"):
            x[::7, 3] = (x[::7, 3].astype(np.float32) * 20).clip(-65504, 65504).astype(np.float16)
    return x


def _check_bound(x):
    """|deq - x| <= scale/2 * (1 + 2^-20) + ulp_fp16(deq)/2, element by element.  Derivation: x * inv and code * scale are each one
    fp32 rounding away from exact (relative 2^-24 each, inv and scale one more each: the 2^-20 factor is generous), rintf moves the
    product by at most 1/2, i.e. scale/2 in the value, and the final fp16 rounding adds at most half a spacing at the result."""
    c, s = R.quantise(x)
    y = R.dequant(c, s)
    assert np.abs(c.astype(np.int32)).max(initial=0) <= 127
    err = np.abs(y.astype(np.float64) - x.astype(np.float64))
    bound = s.astype(np.float64)[..., None] / 2 * (1 + 2.0 ** -20) + R.ulp_fp16(y) / 2
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return c, s, y


@pytest.mark.parametrize("D", [64, 128])
def test_restatement_error_bound_over_magnitudes(D):
    rng = np.random.default_rng(D)
    worst = 0.0
    for mag in (1e-7, 1e-4, 1.0, 30.0, 500.0):
        x = _rows(rng, 20000, D, mag)
        c, s, y = _check_bound(x)
        # a row's largest element takes code +-127
        ax = np.abs(x.astype(np.float32))
        top = ax.argmax(axis=-1)
        live = ax.max(axis=-1) > 0
        assert (np.abs(c[np.arange(len(x)), top].astype(np.int32))[live] == 127).all()
        err = np.abs(y.astype(np.float64) - x.astype(np.float64))
        bound = s.astype(np.float64)[..., None] / 2 * (1 + 2.0 ** -20) + R.ulp_fp16(y) / 2
        worst = max(worst, float((err[live] / bound[live]).max()))
    print(f"D={D}: worst error / bound = {worst:.5f}")


@pytest.mark.parametrize("D", [64, 128])
def test_edge_rows(D):
    sub = np.float16(2.0 ** -24)                                  # the smallest fp16 subnormal
    zero = np.zeros((3, D), np.float16)
    c, s, y = _check_bound(zero)
    assert not c.any() and not s.any() and not y.any()
    one_sub = np.zeros((4, D), np.float16)
    one_sub[0, 0], one_sub[1, D - 1], one_sub[2, 5], one_sub[3, :] = sub, -sub, sub, sub
    c, s, y = _check_bound(one_sub)
    assert c[0, 0] == 127 and c[1, D - 1] == -127 and (c[3] == 127).all()
    assert np.array_equal(y.view(np.uint16), one_sub.view(np.uint16))      # one level: reproduced exactly
    big = np.zeros((3, D), np.float16)
    big[0, :] = 65504
    big[1, 0], big[1, 1] = 65504, -65504
    big[2, 0], big[2, 1:] = 65504, np.float16(1.0)
    c, s, y = _check_bound(big)
    assert np.isfinite(y.astype(np.float32)).all() and y[0, 0] == np.float16(65504) and y[1, 1] == np.float16(-65504)
    assert c[0, 0] == 127 and c[1, 1] == -127


def test_non_finite_rows_dequantise_to_nan():
    x = np.ones((4, 128), np.float16)
    x[0, 7] = np.nan
    x[1, 0] = np.inf
    x[2, 127] = -np.inf
    c, s = R.quantise(x)
    y = R.dequant(c, s)
    assert np.isnan(s[:3]).all() and not c[:3].any() and np.isnan(y[:3].astype(np.float32)).all()
    assert s[3] == np.float32(1.0) / np.float32(127.0) and (c[3] == 127).all() and np.isfinite(y[3].astype(np.float32)).all()


@pytest.mark.parametrize("P,n,D", [(4, 1, 128), (2, 1, 64), (64, 7, 128), (12, 1000, 64), (2048, 3, 128), (6, 33, 16)])
def test_image_size_and_scale_offset(P, n, D):
    rng = np.random.default_rng(P * 1000 + n)
    x = _rows(rng, P * n, D, 1.0).reshape(P, n, D)
    c, s = R.quantise(x)
    img = R.pack(c, s)
    assert img.dtype == np.uint8 and img.size == R.image_bytes(P, n, D) == P * n * (D + 4)
    assert R.scale_offset(P, n, D) == P * n * D and R.scale_offset(P, n, D) % 16 == 0
    assert np.array_equal(img[:P * n * D].view(np.int8).reshape(P, n, D), c)
    assert np.array_equal(img[P * n * D:].view(np.uint32), s.reshape(-1).view(np.uint32))
    c2, s2 = R.unpack(img, P, n, D)
    assert np.array_equal(c2, c) and np.array_equal(s2.view(np.uint32), s.view(np.uint32))
    assert np.array_equal(R.quantise_store(x), img)
    from promptcache_amd import _native
    assert _native.kv_q8_image_bytes(n, P, D) == img.size
    # against the fp16 store: exactly (D + 4) / 2D
    assert img.size * 2 * D == x.nbytes * (D + 4)


class _NoModelLM(H.TokOnlyLM):
    device = "cpu"
    use_full_position_ids = False

    def get_cache_shape(self):
        return 1, 1, 16


def test_engine_module_kv_knob(monkeypatch):
    from promptcache_amd import CacheEngine
    monkeypatch.delenv("PC_MODULE_KV", raising=False)
    assert CacheEngine(16, _NoModelLM(), target_device="cpu").module_kv == "fp16"
    assert CacheEngine(16, _NoModelLM(), target_device="cpu", module_kv="int8").module_kv == "int8"
    with pytest.raises(ValueError, match="module_kv"):
        CacheEngine(16, _NoModelLM(), target_device="cpu", module_kv="fp8")
    monkeypatch.setenv("PC_MODULE_KV", "int8")
    assert CacheEngine(16, _NoModelLM(), target_device="cpu").module_kv == "int8"
    assert CacheEngine(16, _NoModelLM(), target_device="cpu", module_kv="fp16").module_kv == "fp16"     # the argument wins
    monkeypatch.setenv("PC_MODULE_KV", "fp8")
    with pytest.raises(ValueError, match="module_kv"):
        CacheEngine(16, _NoModelLM(), target_device="cpu")
    # a schema that is not encoded holds no module KV in either format
    monkeypatch.setenv("PC_MODULE_KV", "int8")
    eng = CacheEngine(16, _NoModelLM(), target_device="cpu")
    assert eng.module_bytes() == {}


def test_abi_of_the_int8_store_entry_points():
    from promptcache_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "promptcache_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.lib_path())
    for name in ("pc_kv_quant_q8", "pc_kv_gather_q8"):
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/promptcache_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    lib = _native.load()
    # argument errors are answered without a GPU
    assert lib.pc_kv_gather_q8(None, 1, None, 1, 1, 128, 16, None) == -1001
    assert b"null pointer" in lib.pc_last_error_string()
    assert lib.pc_kv_gather_q8(None, 1, None, 1, 1, 96, 16, None) == -1001
    assert b"head_dim" in lib.pc_last_error_string()
    assert lib.pc_kv_quant_q8(None, 4, 2, 128, None, None) == -1001
    assert lib.pc_kv_quant_q8(None, 0, 2, 128, None, None) == 0                 # nothing to do
    seg = (_native.KvSeg * 1)(_native.KvSeg(4096, 10, 8))
    dst = ctypes.c_void_p(4096)
    assert lib.pc_kv_gather_q8(seg, 1, dst, 1, 1, 128, 16, None) == -1002       # rows 10..17 do not fit 16: nothing is launched
    assert b"exceeds max_ctx" in lib.pc_last_error_string()


def test_the_new_kernels_are_in_the_library_and_lean():
    from promptcache_amd import codeobj
    rows = {r["demangled"]: r for r in codeobj.kernels(_native_path())}
    for must in ("kv_gather_q8_kernel", "kv_quant_q8_kernel"):
        hit = [r for n, r in rows.items() if must in n]
        assert 1 <= len(hit) <= 3, (must, len(hit))          # the gather: one instantiation per head dim (32, 64, 128)
        for r in hit:
            assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128 and r["lds"] == 0, r


def _native_path():
    from promptcache_amd import _native
    return _native.lib_path()
