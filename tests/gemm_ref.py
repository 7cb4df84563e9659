"""References for the weight-streaming projections (pc_gemm): numpy only, no GPU.

Two kinds of operands:

* INTEGER operands (``exact_operands``): an fp16 weight of integers in [-2, 2], a hi plane of integers in [-2, 2] and a lo
  plane of {-1, 0, 1} * 2^-6, with ``|hi + lo| <= 2`` in every element.  Every product ``w * (hi + lo)`` is a multiple of
  2^-6 of magnitude <= 4, so every partial sum over at most K terms -- in any order and any grouping -- is a multiple of 2^-6
  below ``4 K``: with ``4 K 2^6 < 2^23`` (K <= 8448 leaves two bits to spare) it has at most 23 significant bits, every
  fp32 addition and every MFMA accumulation is exact, and the only correct output is BIT-EQUAL to the int64 reference.  The
  planes are built directly: the kernels' contract is ``sum_k (hi + lo) * w``, so hi and lo need not be the split of anything.

* GAUSSIAN operands with the split-precision floor (``split_floor``): ``floor16 = max |fp16(x) w^T - ref|`` is what a kernel
  that had only fp16 activations would lose.  The acceptance rule of the split-precision tests is
  ``max |got - ref| <= floor16 / SPLIT_RULE`` (SPLIT_RULE = 32): an fp32 accumulation in plain k order sits a few hundred times
  below floor16, the loss of the lo plane of ONE k-step of ONE row only a few times (tests/test_gemm_ref_cpu.py re-derives
  both for every shape below).  The rule separates the two only up to K = 1056; longer K uses integer operands.
"""
from __future__ import annotations

import numpy as np

LO_BITS = 6
LO_UNIT = 2.0 ** -LO_BITS
SPLIT_RULE = 32.0
SPLIT_K_MAX = 1056

# ---------------------------------------------------------------------------------------------------
# shape tables shared by tests/test_gemm_ref_cpu.py (headroom, sensitivity, room around the rule) and
# tests/test_gpu_gemm_exact.py (the launches)
# ---------------------------------------------------------------------------------------------------

# rows per row regime (launch_skinny_mt1 / mt2 / mt4; 33 and 48 rows: three row tiles in the four-tile kernel)
EXACT_ROWS = {"mt1": (1, 5, 16), "mt2": (17, 32), "mt4": (33, 48, 49, 64)}
# N / 16 -> tiles per workgroup choose_T picks (1, 2, 3, 4, 8); every one leaves a last workgroup with clamped duplicate tiles.
# (launch_T caps T at 6 for four row tiles -- i.e. the T = 8 choice runs the T = 4 instantiation there -- and at 8 / MT tiles
# for int8 weight images.)
EXACT_UNITS = {3: 1, 257: 2, 514: 3, 771: 4, 1027: 8}
# K / 32: with 1 and 7 some waves of the eight-way K split hold nothing; 9 and 17: one or two k-steps plus an empty tail wave;
# 33: a tail shorter than every block depth; 72: full blocks (9 k-steps per wave: U = 8 + tail 1, U = 4: 2 blocks + 1, ...)
EXACT_KS = (1, 7, 9, 17, 33, 72)
EXACT_KS_WIDEST = (1, 7, 9)                  # N = 16432: keep the weight image at a few MB
# the U = 16 block of launch_one (one row tile, one weight tile, residual add, M > 4, K / 32 >= 256)
DEEP_ROWS, DEEP_N, DEEP_KS = (5, 16), (16, 48), (256, 257, 263)
SLAB_SLICES, SLAB_KS = (2, 3, 16), (2, 9, 33)
KSRED_ROWS, KSRED_S, KSRED_T, KSRED_UNITS, KSRED_KS = (1, 12, 16, 17, 32), (1, 2, 3, 8), (1, 2, 4, 8), (5, 8), (3, 9, 33)
ROWS_M, ROWS_UNITS, ROWS_KS = (65, 97, 130, 257, 289, 336, 385, 512), (3, 7), (1, 3, 7, 10)
# int8 weight image: codes up to 127 against hi in [-2, 2]: 127 * 2 * K * 2^6 < 2^23 holds up to K = 512, so the K / 64 = 17 the
# table would like is shrunk to 8
W8_ROWS, W8_K64 = (1, 16, 33, 64), (1, 5, 8)
W8_CODE_MAX = 127
# (B, H, Hkv, D, q_len, past)
QKV_SHAPES = ((1, 2, 2, 64, 1, 3), (2, 4, 2, 128, 5, 7), (1, 4, 1, 32, 17, 0), (1, 2, 2, 128, 40, 9), (1, 2, 1, 64, 70, 2))
QKV_HIDDEN = (32, 288)

# split-precision cases: (family, M, N, K, extra).  K in {32, 288, 544, 1056}; the int8 image needs K % 64 == 0, hence 576.
SPLIT_STORE = (
    ("skinny_mt1", 1, 48, 32, {}), ("skinny_mt1", 12, 48, 544, {}), ("skinny_mt2", 26, 48, 1056, {}), ("skinny_mt4", 50, 48, 288, {}),
    ("skinny_T8", 12, 16432, 288, {}),
    ("slabs", 20, 80, 1056, {"kslices": 3}), ("ks", 12, 80, 544, {"S": 2, "T": 2}), ("rows", 130, 112, 544, {}),
    ("w8", 33, 64, 576, {}),
)
SPLIT_NORM = ((1, 48, 288), (16, 80, 1056), (17, 48, 544), (32, 80, 32))
SPLIT_ACT_ROWS, SPLIT_ACT_INTER, SPLIT_ACT_K = (3, 20, 50, 130), (64, 8256), {64: 288, 8256: 32}


def exact_k_values():
    """Every K the integer-operand GPU tests use with the fp16 weight image."""
    ks = set(EXACT_KS) | set(DEEP_KS) | set(SLAB_KS) | set(KSRED_KS) | set(ROWS_KS) | {h // 32 for h in QKV_HIDDEN}
    return sorted(32 * k for k in ks)


# ---------------------------------------------------------------------------------------------------
# integer operands
# ---------------------------------------------------------------------------------------------------

def exact_weight(N, K, seed, lim=2):
    """int64 [N][K] of integers in [-lim, lim] (the fp16 weight is ``.astype(np.float16)``, exact)."""
    return np.random.default_rng([seed, N, K, 1]).integers(-lim, lim + 1, size=(N, K), dtype=np.int64)


def exact_planes(M, K, seed, two):
    """(hi, lo6) int64 [M][K]: hi in [-2, 2]; lo6 in {-1, 0, 1} (units of 2^-6) with |64 hi + lo6| <= 128, or None."""
    rng = np.random.default_rng([seed, M, K, 2])
    hi = rng.integers(-2, 3, size=(M, K), dtype=np.int64)
    if not two:
        return hi, None
    lo6 = rng.integers(-1, 2, size=(M, K), dtype=np.int64)
    lo6 = np.where(hi == 2, np.minimum(lo6, 0), np.where(hi == -2, np.maximum(lo6, 0), lo6))
    return hi, lo6


def exact_sum6(hi, lo6, w, k0=0, k1=None):
    """int64 [M][N]: 2^6 * sum over features k0 <= k < k1 of (hi + lo) * w."""
    k1 = hi.shape[1] if k1 is None else k1
    x6 = hi[:, k0:k1] << LO_BITS
    if lo6 is not None:
        x6 = x6 + lo6[:, k0:k1]
    return x6 @ w[:, k0:k1].T


def from_sum6(s6):
    """The int64 sums, scaled back by 2^-6 and converted ONCE (exact below 2^24 units)."""
    return (s6.astype(np.float64) * LO_UNIT).astype(np.float32)


def exact_operands(M, N, K, seed, two, want_ref=True):
    """fp16 weight [N][K], hi and lo planes as fp16 [M][K] (lo None for the one-plane form), fp32 reference [M][N]."""
    w = exact_weight(N, K, seed)
    hi, lo6 = exact_planes(M, K, seed, two)
    ref = from_sum6(exact_sum6(hi, lo6, w)) if want_ref else None
    lo = None if lo6 is None else (lo6.astype(np.float64) * LO_UNIT).astype(np.float16)
    return w.astype(np.float16), hi.astype(np.float16), lo, ref


def pack_plane(x, pad=np.nan):
    """[M][K] -> the activation fragment layout Xf[ceil(M/16)][K/32][64][8] (lane 16 g + m of k-step s holds row 16 mt + m,
    features 32 s + 8 g .. + 7); the pad rows M .. 16 ceil(M/16) - 1 of the last row tile are filled with ``pad``."""
    M, K = x.shape
    assert K % 32 == 0
    mt = (M + 15) // 16
    xp = np.full((mt * 16, K), pad, dtype=np.float16)
    xp[:M] = x
    return np.ascontiguousarray(xp.reshape(mt, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(mt, K // 32, 64, 8)


def unpack_plane(f, M):
    """Inverse of ``pack_plane`` (rows < M)."""
    mt, ks = f.shape[0], f.shape[1]
    return f.reshape(mt, ks, 4, 16, 8).transpose(0, 3, 1, 2, 4).reshape(mt * 16, ks * 32)[:M]


def slice_ranges(KS, kslices, w8=False):
    """K-step range [k0, k1) of every K slice as wave_k_range / gemm_rows_kernel cut it: ceil(KS / kslices) k-steps per slice
    (rounded up to a k-step pair for the int8 image); slices behind the end are empty (k0 == k1)."""
    ksq = (KS + kslices - 1) // kslices
    if w8:
        ksq = (ksq + 1) & ~1
    out = []
    for s in range(kslices):
        k0 = min(s * ksq, KS)
        out.append((k0, min(k0 + ksq, KS)))
    return out


def fp32_k_order(x_planes, w):
    """sum_k in fp32, one feature after the other in k order, planes interleaved (the worst realistic order): [M][N] fp32."""
    acc = np.zeros((x_planes[0].shape[0], w.shape[0]), dtype=np.float32)
    wt = np.ascontiguousarray(w.T.astype(np.float32))
    xs = [p.astype(np.float32) for p in x_planes]
    for k in range(w.shape[1]):
        for p in xs:
            acc += p[:, k:k + 1] * wt[k:k + 1, :]           # fp32 product (exact for fp16 operands), fp32 add
    return acc


# ---------------------------------------------------------------------------------------------------
# Gaussian operands and the split-precision floor
# ---------------------------------------------------------------------------------------------------

def gaussian_operands(M, N, K, seed, x_scale=1.0):
    """x fp32 [M][K] ~ x_scale N(0, 1), w fp16 [N][K] ~ 0.05 N(0, 1): the inputs of the tolerance tests in test_gpu_kernels.py."""
    rng = np.random.default_rng([seed, M, N, K])
    w = (0.05 * rng.standard_normal((N, K), dtype=np.float32)).astype(np.float16)
    x = (x_scale * rng.standard_normal((M, K), dtype=np.float32)).astype(np.float32)
    return x, w


def split_planes(x):
    """hi = fp16(x), lo = fp16(x - hi) (what to_act_frags and pc_split produce)."""
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_floor(x, w):
    """fp64 ``ref = x w^T`` and ``floor16 = max |fp16(x) w^T - ref|`` (w: fp16 weight, or the fp64 dequantised int8 weight)."""
    wd = w.astype(np.float64)
    ref = x.astype(np.float64) @ wd.T
    floor16 = float(np.abs(x.astype(np.float16).astype(np.float64) @ wd.T - ref).max())
    return ref, floor16


def lost_lo_step(x, w, mode=np.median, depth=32):
    """max |error| when the lo plane of ONE k-step of ONE row is lost, reduced over all (row, k-step) choices by ``mode``.
    ``depth``: features per k-step (32: a k-step of the weight-streaming kernels; 16: one slab of the 32x32x16 MFMA of
    pc_gemm_dense, where a K that is no multiple of it ends in a shorter slab -- zero-filled here as in the kernel)."""
    _, lo = split_planes(x)
    M, K = x.shape
    steps = (K + depth - 1) // depth
    lo3 = np.zeros((M, steps * depth))
    lo3[:, :K] = lo
    lo3 = lo3.reshape(M, steps, depth)
    w3 = np.zeros((w.shape[0], steps * depth))
    w3[:, :K] = w
    w3 = w3.reshape(w.shape[0], steps, depth)
    worst = np.empty((M, steps))
    for s in range(steps):
        worst[:, s] = np.abs(lo3[:, s] @ w3[:, s].T).max(axis=1)
    return float(mode(worst))


def rmsnorm64(x, gain, eps):
    xd = x.astype(np.float64)
    return xd / np.sqrt((xd * xd).mean(axis=1, keepdims=True) + eps) * gain.astype(np.float64)
