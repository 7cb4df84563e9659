"""Numpy reference of the slot attention over int8 K / V images (csrc/pc_slots_q8.hip: pc_attn_decode_slots_q8).  Test
infrastructure only.

A slot attends over ``len`` image rows -- an element is ``float32(code) * scale``, the fp32 product with no fp16 rounding -- plus
the row that was just appended, exact from the fp16 arena; the launch also quantises that row into image row ``len`` with the
pinned arithmetic of ``tests/kv_q8_ref.quantise``."""
from typing import Tuple

import numpy as np

from tests import kv_q8_ref as q8
from tests import slots_ref

F32 = np.float32


def dequant32(codes: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """(int8 ``[..., D]``, fp32 ``[...]``) -> fp32 ``[..., D]``: the fp32 product, not rounded to fp16."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (codes.astype(F32) * scale[..., None].astype(F32)).astype(F32)


def attend(q: np.ndarray, codes_k: np.ndarray, scale_k: np.ndarray, codes_v: np.ndarray, scale_v: np.ndarray, k_new16: np.ndarray,
           v_new16: np.ndarray) -> np.ndarray:
    """One slot.  q ``[H][D]`` (RoPE applied, fp32), codes ``[Hkv][len][D]`` int8 and scales ``[Hkv][len]`` fp32 of the image rows
    in front of the new one, ``k_new16`` / ``v_new16`` ``[Hkv][D]`` fp16: the row just appended.  -> ``[H][D]`` fp32:
    ``slots_ref.attend_slot`` over the dequantised rows followed by the exact new row."""
    assert k_new16.dtype == np.float16 and v_new16.dtype == np.float16
    k = np.concatenate([dequant32(codes_k, scale_k), k_new16.astype(F32)[:, None, :]], axis=1)
    v = np.concatenate([dequant32(codes_v, scale_v), v_new16.astype(F32)[:, None, :]], axis=1)
    return slots_ref.attend_slot(q, k, v)


def append(image: Tuple[np.ndarray, np.ndarray], row16: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``image`` = (codes ``[..., n, D]``, scale ``[..., n]``), ``row16`` fp16 ``[..., D]`` -> the image with the quantised row
    behind its last one (``kv_q8_ref.quantise``)."""
    codes, scale = image
    c, s = q8.quantise(row16)
    return np.concatenate([codes, c[..., None, :]], axis=-2), np.concatenate([scale, s[..., None]], axis=-1)


def lossless_rows(rng, shape, D: int = 128) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Rows on which the format is lossless: integer codes with a +-127 in every row, times a power-of-two scale.
    -> (fp16 rows ``shape + (D,)``, int8 codes, fp32 scales); every value ``code * scale`` is exact in fp16 (|code| <= 127 has 7
    bits, the scales are 2^-9 .. 2^-4, so the smallest spacing 2^-9 is a normal fp16's)."""
    codes = rng.integers(-127, 128, size=tuple(shape) + (D,)).astype(np.int8)
    flat = codes.reshape(-1, D)
    where = rng.integers(0, D, size=flat.shape[0])
    flat[np.arange(flat.shape[0]), where] = np.where(rng.integers(0, 2, size=flat.shape[0]) == 0, -127, 127).astype(np.int8)
    scale = np.ldexp(F32(1.0), rng.integers(-9, -3, size=tuple(shape))).astype(F32)
    rows = (codes.astype(F32) * scale[..., None]).astype(np.float16)
    assert np.array_equal(rows.astype(F32), codes.astype(F32) * scale[..., None])
    return rows, codes, scale
