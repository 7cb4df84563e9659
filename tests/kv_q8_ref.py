"""numpy restatement of the int8 module KV store (csrc/pc_kv_q8.hip: pc_kv_quant_q8, pc_kv_gather_q8).  Test infrastructure only.

One segment of ``n`` rows, ``P = L * 2 * Hkv`` planes, head dim ``D`` is one contiguous byte image::

    int8  codes [P][n][D]      plane p = (layer * 2 + k|v) * Hkv + head
    fp32  scale [P][n]         starts at byte P*n*D

A (plane, row) of D fp16 values x is quantised with every step in fp32, round to nearest even::

    s = max|x|;  inv = 127.0f / s (0 when s == 0);  code = (int8) rintf(x * inv);  scale = s / 127.0f
    deq = fp16_rn((float) code * scale)

A row that holds a NaN or an infinity stores scale = NaN and codes 0, and dequantises to NaN."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

_F127 = np.float32(127.0)


def quantise(x16: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """fp16 ``[..., D]`` -> (int8 codes ``[..., D]``, fp32 scale ``[...]``)."""
    assert x16.dtype == np.float16
    x = x16.astype(np.float32)
    ax = np.abs(x)
    bad = ~np.isfinite(ax).all(axis=-1)
    s = np.where(bad, np.float32(0), np.max(np.where(np.isfinite(ax), ax, np.float32(0)), axis=-1)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.where(s > 0, _F127 / np.where(s > 0, s, np.float32(1)), np.float32(0)).astype(np.float32)
        prod = (np.where(bad[..., None], np.float32(0), x) * inv[..., None]).astype(np.float32)
    codes = np.rint(prod).astype(np.int32).astype(np.int8)
    scale = (s / _F127).astype(np.float32)
    scale = np.where(bad, np.float32(np.nan), scale).astype(np.float32)
    return codes, scale


def dequant(codes: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """(int8 ``[..., D]``, fp32 ``[...]``) -> fp16 ``[..., D]``: the fp32 product, then one rounding to fp16."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (codes.astype(np.float32) * scale[..., None].astype(np.float32)).astype(np.float32).astype(np.float16)


def image_bytes(P: int, n: int, D: int) -> int:
    return P * n * (D + 4)


def scale_offset(P: int, n: int, D: int) -> int:
    return P * n * D


def pack(codes: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """codes ``[P, n, D]`` int8 + scale ``[P, n]`` fp32 -> the uint8 image."""
    P, n, D = codes.shape
    assert scale.shape == (P, n) and codes.dtype == np.int8 and scale.dtype == np.float32
    return np.concatenate([np.ascontiguousarray(codes).view(np.uint8).reshape(-1),
                           np.ascontiguousarray(scale).view(np.uint8).reshape(-1)])


def unpack(image: np.ndarray, P: int, n: int, D: int) -> Tuple[np.ndarray, np.ndarray]:
    image = np.ascontiguousarray(image).view(np.uint8).reshape(-1)
    assert image.size == image_bytes(P, n, D), (image.size, P, n, D)
    off = scale_offset(P, n, D)
    return image[:off].view(np.int8).reshape(P, n, D), image[off:].view(np.float32).reshape(P, n)


def quantise_store(store16: np.ndarray) -> np.ndarray:
    """fp16 segment store ``[L, 2, Hkv, n, D]`` (or ``[P, n, D]``) -> image."""
    n, D = store16.shape[-2:]
    c, s = quantise(store16.reshape(-1, n, D))
    return pack(c, s)


def dequant_image(image: np.ndarray, L: int, Hkv: int, n: int, D: int) -> np.ndarray:
    """image -> fp16 ``[L, 2, Hkv, n, D]``."""
    c, s = unpack(image, L * 2 * Hkv, n, D)
    return dequant(c, s).reshape(L, 2, Hkv, n, D)


def gather(arena: np.ndarray, images: Sequence[np.ndarray], lens: Sequence[int], dst_rows: Sequence[int]) -> np.ndarray:
    """What pc_kv_gather_q8 leaves in the staged buffer ``[L, 2, Hkv, cap, D]`` (fp16, returned as a copy)."""
    out = arena.copy()
    L, _, Hkv, _, D = out.shape
    for img, n, r in zip(images, lens, dst_rows):
        if n:
            out[:, :, :, r:r + n] = dequant_image(img, L, Hkv, n, D)
    return out


def ulp_fp16(y: np.ndarray) -> np.ndarray:
    """Spacing of fp16 at |y| (float64): 2^(e - 10) with e the exponent of |y|, 2^-24 over the subnormals and at zero."""
    a = np.abs(y.astype(np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)
