"""Numpy restatement of the MXFP4 weight format (OCP MX: 32-element blocks, E8M0 scale, FP4 E2M1 elements) as this project
fixes it; no GPU, no torch.  ``promptcache_amd`` must not import this module: ``_native.quantize_mxfp4`` is held bit-equal to it.

* Block: 32 consecutive input features k of one output row n.
* Block exponent: ``e = clamp(floor(log2(amax)) - 2, -13, 13)``; an all-zero block has ``e = 0``.  E8M0 byte ``e + 127``.
* Element: ``v = w * 2^-e`` (exact), rounded to the nearest value of the E2M1 grid with ties to the even CODE; ``|v| > 6``
  saturates to 6; anything that rounds to zero is code 0000, never 1000.  Code bits ``s e e m``: codes 0..7 are
  0, .5, 1, 1.5, 2, 3, 4, 6.
* A NaN or an infinity raises ``ValueError``.
* Packing: two codes per byte, the low nibble is the lower feature index.
"""
from __future__ import annotations

import numpy as np

BLOCK = 32
EXP_MIN, EXP_MAX = -13, 13
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float64)


def block_exponents(w):
    """int [N][K/32]: the clamped block exponents of a finite weight [N][K]."""
    w = np.asarray(w, dtype=np.float64)
    N, K = w.shape
    assert K % BLOCK == 0, K
    amax = np.abs(w.reshape(N, K // BLOCK, BLOCK)).max(axis=2)
    e = np.zeros(amax.shape, dtype=np.int64)
    nz = amax > 0
    # floor(log2(a)) without a logarithm: a = m * 2^x with m in [0.5, 1)
    e[nz] = np.clip(np.frexp(amax[nz])[1] - 1 - 2, EXP_MIN, EXP_MAX)
    return e


def round_e2m1(v):
    """Codes 0..15 of the scaled elements ``v`` (any shape): nearest grid value by distance, a tie to the even code."""
    v = np.asarray(v, dtype=np.float64)
    a = np.minimum(np.abs(v), 6.0)
    dist = np.abs(a[..., None] - GRID)                  # [..., 8]; exact: multiples of 2^-k far inside float64
    best = dist.min(axis=-1, keepdims=True)
    cand = dist == best                                 # one code, or two neighbours on a tie
    even = cand & (np.arange(8) % 2 == 0)
    code = np.where(cand.sum(axis=-1) > 1, even.argmax(axis=-1), cand.argmax(axis=-1))
    return (code + 8 * ((v < 0) & (code > 0))).astype(np.uint8)


def quantize(w):
    """``(codes uint8 [N][K/2], exps uint8 [N][K/32])`` of a weight [N][K] (any float dtype)."""
    w = np.asarray(w)
    if not np.isfinite(w.astype(np.float64)).all():
        raise ValueError("mxfp4: the weight holds a NaN or an infinity")
    w = w.astype(np.float64)
    N, K = w.shape
    e = block_exponents(w)
    v = w.reshape(N, K // BLOCK, BLOCK) * np.exp2(-e.astype(np.float64))[:, :, None]
    c = round_e2m1(v).reshape(N, K // 2, 2)
    return (c[:, :, 0] | (c[:, :, 1] << 4)).astype(np.uint8), (e + 127).astype(np.uint8)


def dequantize(codes, exps):
    """float64 [N][K] (every value is exact in fp16: ``.astype(np.float16)`` loses nothing)."""
    codes, exps = np.asarray(codes), np.asarray(exps)
    N, K = codes.shape[0], 2 * codes.shape[1]
    nib = np.stack((codes & 15, codes >> 4), axis=2).reshape(N, K)
    val = np.where(nib >= 8, -GRID[nib & 7], GRID[nib & 7])
    scale = np.exp2(exps.astype(np.float64) - 127.0)
    return (val.reshape(N, K // BLOCK, BLOCK) * scale[:, :, None]).reshape(N, K)


def pack_images(codes, exps):
    """The two images ``pc_gemm_w4`` reads, element by element from the layout's definition (slow, for small matrices):
    codes [N/16][K/128][64][16], scales [N/16][K/128][16][4]."""
    N, K = codes.shape[0], 2 * codes.shape[1]
    assert N % 16 == 0 and K % 128 == 0
    ci = np.zeros((N // 16, K // 128, 64, 16), dtype=np.uint8)
    si = np.zeros((N // 16, K // 128, 16, 4), dtype=np.uint8)
    for t in range(N // 16):
        for s in range(K // 128):
            for m in range(16):
                for j in range(4):
                    si[t, s, m, j] = exps[16 * t + m, 4 * s + j]
                    for g in range(4):
                        k0 = 128 * s + 32 * j + 8 * g
                        ci[t, s, 16 * g + m, 4 * j:4 * j + 4] = codes[16 * t + m, k0 // 2:k0 // 2 + 4]
    return ci, si


def exact_weight(N, K, seed):
    """codes uniform over the 15 distinct values, block exponents in {0, 1}: W' = multiples of 0.5 up to 12.
    Returns (codes [N][K/2], exps [N][K/32], w2 int64 [N][K] = 2 W')."""
    rng = np.random.default_rng([seed, N, K, 4])
    nib = rng.integers(0, 15, size=(N, K), dtype=np.int64)
    nib = np.where(nib >= 8, nib + 1, nib).astype(np.uint8)               # 8 (-0) is never produced by the quantiser
    exps = (127 + rng.integers(0, 2, size=(N, K // 32))).astype(np.uint8)
    n2 = nib.reshape(N, K // 2, 2)
    codes = (n2[:, :, 0] | (n2[:, :, 1] << 4)).astype(np.uint8)
    w2 = np.rint(2.0 * dequantize(codes, exps)).astype(np.int64)
    return codes, exps, w2
