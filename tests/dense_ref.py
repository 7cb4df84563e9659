"""References for the many-row projections (pc_gemm_dense, pc_gemm_dense_ws, pc_gemm_dense_qkv_rope, pc_gemm_dense_a8;
prompt-cache_amd/csrc/pc_gemm_dense.hip): numpy only, no GPU.  The operand generators and the split-precision rule are those of
tests/gemm_ref.py; this file adds

* a restatement of the host-side choices of the kernel file -- which tile width ``launch_dense_tile`` picks and when
  ``launch_dense_splitk`` cuts K -- so that the shape tables below can say which of the 20 ``gemm_dense_kernel<WM, EPI, TWO>``
  instantiations (and which ``dense_reduce_kernel``) a launch runs WITHOUT an environment override (PC_DENSE_BN / PC_DENSE_KS are
  read once per process: the shapes select),
* the shape tables of tests/test_gpu_dense_exact.py, every entry annotated with the instantiation it selects and the edge it is
  there for (tests/test_dense_ref_cpu.py checks the annotations against the restatement, the headroom of the integer operands and
  the room on both sides of the ``floor16 / 32`` rule),
* integer operands for the LLM.int8 form (pc_gemm_dense_a8) and a rotation table that varies per (row, feature pair).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import gemm_ref as gr

BM, BK = 128, 64                                                 # pc_gemm_dense.hip:54
EPI_STORE, EPI_ADD, EPI_SILU, EPI_ROPE, EPI_GELU = 0, 1, 2, 3, 4   # pc_gemm_dense.hip:56
EPI_NAMES = {EPI_STORE: "STORE", EPI_ADD: "ADD", EPI_SILU: "SILU", EPI_ROPE: "ROPE", EPI_GELU: "GELU"}

# (tile 128 | 256, K slices asked for, K-steps per slice, slabs written to the workspace: 0 = the plain form)
Plan = namedtuple("Plan", "tile kslices kper slabs")


def ceil_div(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------
# the host-side choices, restated line by line
# ---------------------------------------------------------------------------------------------------

def select_tile(M, cols):
    """launch_dense_tile (pc_gemm_dense.hip:882-893) without PC_DENSE_BN.  ``cols``: N; 2 * inter under SiLU (:888 ``nfeat * 2``);
    (H + 2 Hkv) * 128 under RoPE (:1014 sets p.N to it)."""
    mb = ceil_div(M, BM)                                                             # :889
    b256, b128 = mb * ceil_div(cols, 256), mb * ceil_div(cols, 128)                  # :890
    # :891   b256 <= 512 && 0.62f * ceil(b128 / 256) < 1.0f * ceil(b256 / 256), in float32 as the source has it
    narrow = b256 <= 512 and bool(np.float32(0.62) * np.float32(ceil_div(b128, 256)) < np.float32(1.0) * np.float32(ceil_div(b256, 256)))
    return 128 if narrow else 256                                                    # :892  launch_dense<4, EPI> : launch_dense<2, EPI>


def split_slices(M, N, K, epi, ws_bytes, xscale=False):
    """launch_dense_splitk (pc_gemm_dense.hip:854-879) without PC_DENSE_KS / PC_DENSE_BN: (tile, kslices) or None when the plain
    form runs.  The ``narrow`` branch (:864) needs 256 / b256 < 2 and 256 / b128 >= 2; b128 >= b256, so it never holds: every
    split-K launch is launch_dense<2, EPI_STORE> plus dense_reduce_kernel."""
    if ws_bytes <= 0 or xscale or epi not in (EPI_STORE, EPI_ADD):                   # :858
        return None
    nkt, mb = ceil_div(K, BK), ceil_div(M, BM)                                       # :859
    b256, b128 = mb * ceil_div(N, 256), mb * ceil_div(N, 128)                        # :861
    narrow, ks = False, 256 // b256                                                  # :862-863
    if ks < 2 and 256 // b128 >= 2:                                                  # :864
        narrow, ks = True, 256 // b128
    ks = min(ks, 8)                                                                  # :865
    while ks > 1 and nkt // ks < 8:                                                  # :866  keep >= 8 K-steps per slice
        ks -= 1
    if ks < 2 or ks * M * N * 4 > ws_bytes:                                          # :867
        return None
    return (128 if narrow else 256), ks                                              # :870


def plan(M, cols, K, epi, ws_bytes=0, xscale=False):
    """(M, cols, K, epilogue, workspace bytes) -> Plan.  gemm_dense_impl (:949-955) tries the split form first, then the tile rule."""
    nkt = ceil_div(K, BK)                                                            # launch_dense :819
    sp = split_slices(M, cols, K, epi, ws_bytes, xscale)
    if sp is None:
        return Plan(select_tile(M, cols), 1, nkt, 0)                                 # :820 kper = ceil(nkt / 1); grid.y = 1 (:821)
    tile, ks = sp
    kper = ceil_div(nkt, ks)                                                         # :820
    return Plan(tile, ks, kper, ceil_div(nkt, kper))                                 # :821 grid.y, :872 nslab


def slice_steps(K, kper):
    """K-steps of every slice (gemm_dense_kernel :114-116: t0 = blockIdx.y * kper, nk = min(kper, nkt - t0))."""
    nkt = ceil_div(K, BK)
    return [min(kper, nkt - t0) for t0 in range(0, nkt, kper)]


def kernels(p, epi, two):
    """The kernel instantiations a launch with plan ``p`` runs: ("gemm", WM, EPI, TWO) (launch_dense :845-846: TWO = x_lo given)
    and, for the split form, ("reduce", ADD) (:875-876) behind a STORE main kernel (:870)."""
    wm = 4 if p.tile == 128 else 2                                                   # BN = 64 * (8 / WM), :96
    if p.slabs:
        return {("gemm", wm, EPI_STORE, bool(two)), ("reduce", epi == EPI_ADD)}
    return {("gemm", wm, epi, bool(two))}


ALL_KERNELS = {("gemm", wm, epi, two) for wm in (2, 4) for epi in EPI_NAMES for two in (False, True)} | {("reduce", False), ("reduce", True)}


def grid_panels(M, cols, epi, tile):
    """(mb, nb, workgroups launched per K slice) -- launch_dense :816-821; workgroups with ni >= nb return at once (:112)."""
    units = ceil_div(cols // 2, tile // 2) if epi == EPI_SILU else ceil_div(cols, tile)    # :816
    mb = ceil_div(M, BM)
    return mb, units, 8 * mb * ceil_div(units, 8)


# ---------------------------------------------------------------------------------------------------
# shape tables: integer operands
# ---------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "M N K tile edge")

ROW_EDGE = {1: "a single row (every staged activation row clamps to row 0)", 127: "one M-block, one row short",
            130: "a 2-row second M-block", 257: "three M-blocks, one row in the last", 300: "three M-blocks, 44 rows in the last"}
K_EDGE = {8: "one chunk: nk = 1, the K tail only", 64: "nk = 1, no tail, stage(1) skipped", 72: "nk = 2 with a one-chunk tail",
          136: "odd nk = 3, one-chunk tail: the tail lands in buffer 0 (double-buffer parity)",
          168: "odd nk = 3 with a five-chunk tail (XOR-permuted chunk positions on both sides of kchunks)",
          200: "nk = 4, one-chunk tail in buffer 1", 520: "a full pipeline (nk = 9) plus a one-chunk tail"}
NARROW_N = {132: "nb = 2 < 8: six of every eight workgroups return at ni >= nb", 1156: "nb = 10: not a multiple of 8"}

# narrow tile (gemm_dense_kernel<4, STORE | ADD, TWO>): every (M, N, K) class against every other
STORE_ADD_NARROW = tuple(Case(M, N, K, 128, f"{ROW_EDGE[M]}; {NARROW_N[N]}; {K_EDGE[K]}")
                         for M in ROW_EDGE for N in NARROW_N for K in K_EDGE)
# wide tile (gemm_dense_kernel<2, STORE | ADD, TWO>) without a workspace: 0.62 * ceil(b128 / 256) >= ceil(b256 / 256)
STORE_ADD_WIDE = tuple(
    [Case(300, 10884, K, 256, f"b256 = 129, b128 = 258; nb = 43: not a multiple of 8; {K_EDGE[K]}") for K in K_EDGE] + [
        Case(257, 10884, 168, 256, f"b256 = 129; {ROW_EDGE[257]}; {K_EDGE[168]}"),
        Case(130, 16644, 72, 256, f"b256 = 132, b128 = 262; nb = 66; {ROW_EDGE[130]}"),
        Case(1030, 3588, 136, 256, "b256 = 135, b128 = 261: nine M-blocks, nb = 15"),
        Case(16390, 132, 72, 256, "b256 = 129, b128 = 258 from 129 M-blocks; nb = 1 < 8: seven of every eight workgroups return"),
        Case(1, 32772, 72, 256, f"b256 = 129, b128 = 257; {ROW_EDGE[1]}"),
        Case(127, 32772, 136, 256, f"b256 = 129, b128 = 257; {ROW_EDGE[127]}"),
    ])
# per-row weight scales 2^-2 .. 2^2 (the epilogue's wscale multiply), both tiles
WSCALE_CASES = (Case(130, 260, 136, 128, "wscale, narrow, ragged N (nb = 3)"), Case(300, 1156, 72, 128, "wscale, narrow, three M-blocks"),
                Case(300, 10884, 72, 256, "wscale, wide, last panel holds 132 of 256 columns"))
WSCALE_EXP = (-2, 2)

# split-K through pc_gemm_dense_ws: (M, N, K, kslices, kper, K-steps per slice, edge); all launch_dense<2, EPI_STORE> + reduce
SplitCase = namedtuple("SplitCase", "M N K kslices kper steps edge")
SPLIT_CASES = (
    SplitCase(130, 260, 1096, 2, 9, (9, 9), "2 slices of 9 K-steps, the K tail (one chunk) ends the last; nb = 2"),
    SplitCase(130, 132, 2056, 4, 9, (9, 9, 9, 6), "4 slices of 9, 9, 9 and 6 K-steps with a tail; nb = 1"),
    SplitCase(257, 132, 1096, 2, 9, (9, 9), "three M-blocks"),
)
# shapes launch_dense_splitk refuses although a workspace is there: (case, why)
SPLIT_REFUSED = ((Case(130, 260, 520, 128, "nkt = 9: nkt / ks < 8 for every ks >= 2 -> plain narrow form"), "too few K-steps"),
                 (Case(300, 10884, 72, 256, "b256 = 129 > 128: 256 / b256 < 2 -> plain wide form"), "full grid"))

# pc_gemm_dense_qkv_rope, D = 128: (B, H, Hkv, q_len, past | past_lens, K, lo_row0, q_lo, kv_lo, two, tile, edge)
RopeCase = namedtuple("RopeCase", "B H Hkv q_len past K lo_row0 q_lo kv_lo two tile edge")
ROPE_CASES = (
    RopeCase(1, 2, 1, 130, 3, 72, 3, True, True, True, 128, "B = 1, 4 heads, Hkv < H, residual rows start at the past (lo_row0 = past)"),
    RopeCase(3, 4, 2, 50, (0, 7, 3), 136, 0, True, True, True, 128, "B = 3, past_lens differ, batch boundaries at rows 50 and 100 of M-block 0"),
    RopeCase(1, 8, 2, 127, 5, 200, 2, True, True, False, 128, "12 heads, one activation plane, 0 < lo_row0 < past"),
    RopeCase(2, 3, 1, 65, 0, 8, 0, False, False, True, 128, "5 heads (odd), q_lo and k_lo / v_lo absent, K = 8, batch boundary at row 65"),
    RopeCase(3, 100, 16, 50, (4, 0, 9), 72, 0, True, True, True, 256, "wide: 132 heads, two per panel, M = 150, past_lens"),
    RopeCase(1, 65, 11, 257, 1, 72, 1, True, True, False, 256, "wide: 87 heads (the last panel holds one), three M-blocks, one plane"),
)
ROT_CHOICES = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.5, 0.5))

# pc_gemm_dense_a8: activation codes in [-127, 127], weight codes in [-2, 2], scales 2^-1 .. 2^1, corr in [-8, 8]
A8_CODE_MAX, A8_W_MAX, A8_EXP, A8_CORR_MAX, BASE_MAX = 127, 2, (-1, 1), 8, 8
A8_CASES = (Case(130, 260, 72, 128, "a8 narrow: ragged M and N, one-chunk K tail"), Case(1, 132, 136, 128, "a8 narrow: a single row, odd nk"),
            Case(300, 10884, 136, 256, "a8 wide: three M-blocks, nb = 43, K tail"))


def exact_cases():
    """Every (M, N, K) the integer-operand launches of pc_gemm_dense / _ws use with the operands of gemm_ref.exact_*."""
    out = [(c.M, c.N, c.K) for c in STORE_ADD_NARROW + STORE_ADD_WIDE + WSCALE_CASES]
    out += [(c.M, c.N, c.K) for c in SPLIT_CASES] + [(c.M, c.N, c.K) for c, _ in SPLIT_REFUSED]
    return out


def rope_dims(c):
    """(M, cols) of a RopeCase."""
    return c.B * c.q_len, (c.H + 2 * c.Hkv) * 128


# ---------------------------------------------------------------------------------------------------
# shape tables: Gaussian operands (K <= gemm_ref.SPLIT_K_MAX)
# ---------------------------------------------------------------------------------------------------

# (family, M, N, K, tile, form): form = store | ws (split-K with a workspace) | add (on a Gaussian base) | one (x_lo absent)
SplitFloorCase = namedtuple("SplitFloorCase", "family M N K tile form")
SPLIT_FLOOR = (
    SplitFloorCase("dense_narrow", 130, 136, 72, 128, "store"),
    SplitFloorCase("dense_narrow", 130, 136, 520, 128, "store"),
    SplitFloorCase("dense_wide", 300, 10884, 72, 256, "store"),
    SplitFloorCase("dense_splitk", 130, 132, 1040, 256, "ws"),      # nkt = 17: the smallest K class with nkt / 2 >= 8 is 961 .. 1024
    SplitFloorCase("dense_add", 257, 264, 1040, 128, "add"),
    SplitFloorCase("dense_one_plane", 130, 136, 520, 128, "one"),
)
# (act, M, inter, K, tile, two, wscale): N = 2 * inter under SiLU, inter under GELU
ActCase = namedtuple("ActCase", "act M inter K tile two wscale")
ACT_CASES = (
    ActCase("silu", 45, 172, 520, 128, True, False), ActCase("silu", 45, 172, 520, 128, True, True), ActCase("silu", 130, 300, 72, 128, False, False),
    ActCase("silu", 300, 5444, 72, 256, True, False), ActCase("silu", 257, 5508, 136, 256, False, False),
    ActCase("gelu", 45, 172, 520, 128, True, False), ActCase("gelu", 130, 300, 72, 128, False, False),
    ActCase("gelu", 300, 10884, 72, 256, True, False), ActCase("gelu", 257, 11012, 136, 256, False, False),
)


def act_cols(c):
    return 2 * c.inter if c.act == "silu" else c.inter


def act_wscale(n):
    """Per-row weight scales in [0.5, 1.5) for the activation cases that carry one."""
    return (0.5 + np.random.default_rng(2).random(n)).astype(np.float32)


def launches():
    """(Plan, epilogue, planes) of EVERY launch tests/test_gpu_dense_exact.py makes, in no particular order: what the kernel names
    recorded in profiles/dense_exact_kernel_stats.txt are counted against."""
    out, sa = [], (EPI_STORE, EPI_ADD)
    for c in STORE_ADD_NARROW + STORE_ADD_WIDE + WSCALE_CASES:
        out += [(plan(c.M, c.N, c.K, epi), epi, two) for epi in sa for two in (True, False)]
    for c in SPLIT_CASES:                                             # with room for the slabs, then one byte short of it
        need = c.kslices * c.M * c.N * 4
        out += [(plan(c.M, c.N, c.K, epi, ws_bytes=b), epi, two) for epi in sa for two in (True, False) for b in (need, need - 1)]
    for c, _ in SPLIT_REFUSED:
        out += [(plan(c.M, c.N, c.K, epi, ws_bytes=1 << 30), epi, True) for epi in sa]
    for c in ROPE_CASES:
        out.append((plan(*rope_dims(c), c.K, EPI_ROPE), EPI_ROPE, c.two))
    for c in A8_CASES:                                                # *corr_has = 1 and 0
        out += [(plan(c.M, c.N, c.K, epi, xscale=True), epi, False) for epi in sa] * 2
    for c in ACT_CASES:
        epi = EPI_SILU if c.act == "silu" else EPI_GELU
        out.append((plan(c.M, act_cols(c), c.K, epi), epi, c.two))
    for c in SPLIT_FLOOR:
        epi = EPI_ADD if c.form == "add" else EPI_STORE
        out.append((plan(c.M, c.N, c.K, epi, ws_bytes=32 * c.M * c.N if c.form == "ws" else 0), epi, c.form != "one"))
    return out


# ---------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------

def pow2_scales(n, seed, lo, hi):
    """(exponents int64 [n], fp32 2^exponent): powers of two that differ from row to row, both ends present."""
    e = np.random.default_rng([seed, n, 7]).integers(lo, hi + 1, size=n, dtype=np.int64)
    e[0], e[-1] = hi, lo
    return e, np.exp2(e.astype(np.float64)).astype(np.float32)


def base_ints(M, N, seed, lim=BASE_MAX):
    """The y an ADD launch starts from: integers in [-lim, lim] as fp32."""
    return np.random.default_rng([seed, M, N, 3]).integers(-lim, lim + 1, size=(M, N)).astype(np.float32)


def a8_operands(M, N, K, seed):
    """LLM.int8 operands: activation codes int64 [M][K] in [-127, 127] (every row holds a +-127), weight codes int64 [N][K] in
    [-2, 2], exponents of the power-of-two w_scale [N] and x_scale [M], integer corr int64 [M][N]."""
    rng = np.random.default_rng([seed, M, N, K, 4])
    q = rng.integers(-A8_CODE_MAX, A8_CODE_MAX + 1, size=(M, K), dtype=np.int64)
    q[np.arange(M), rng.integers(0, K, size=M)] = np.where(np.arange(M) % 2 == 0, A8_CODE_MAX, -A8_CODE_MAX)
    w = gr.exact_weight(N, K, seed, A8_W_MAX)
    we, _ = pow2_scales(N, seed, *A8_EXP)
    xe, _ = pow2_scales(M, seed + 1, *A8_EXP)
    corr = rng.integers(-A8_CORR_MAX, A8_CORR_MAX + 1, size=(M, N), dtype=np.int64)
    return q, w, we, xe, corr


def a8_expect(q, w, we, xe, corr):
    """float64 [M][N]: sum * w_scale[n] * x_scale[m] without and with corr (exact: integers times powers of two)."""
    s = (q @ w.T).astype(np.float64) * np.exp2(we.astype(np.float64))[None, :] * np.exp2(xe.astype(np.float64))[:, None]
    return s, s + corr.astype(np.float64)


def rotation_table(T, half=64):
    """fp32 [T][half][2] (cos, sin): a fixed function of (row t, feature pair j) into ROT_CHOICES that varies along both."""
    t, j = np.arange(T, dtype=np.int64)[:, None], np.arange(half, dtype=np.int64)[None, :]
    idx = (3 * t + 7 * j + (t * j) // 5 + (t // 50)) % len(ROT_CHOICES)
    return np.asarray(ROT_CHOICES, dtype=np.float32)[idx]


def rope_expect(sums, cs, H, Hkv):
    """float64 [T][H + 2 Hkv][128]: q and k heads rotated (llama rotate_half: feature d pairs with d + 64,
    lo' = lo cos - hi sin, hi' = hi cos + lo sin), v heads as they are.  ``sums`` [T][(H + 2 Hkv) * 128] exact projection sums."""
    T = sums.shape[0]
    x = sums.astype(np.float64).reshape(T, H + 2 * Hkv, 2, 64)
    c, s = cs[:, None, :, 0].astype(np.float64), cs[:, None, :, 1].astype(np.float64)
    out = x.copy()
    r = H + Hkv
    out[:, :r, 0] = x[:, :r, 0] * c - x[:, :r, 1] * s
    out[:, :r, 1] = x[:, :r, 1] * c + x[:, :r, 0] * s
    return out.reshape(T, H + 2 * Hkv, 128)


def split_is_exact(v):
    """True where fp16(v) + fp16(v - fp16(v)) == v (what q_hi + q_lo and arena + residual plane can hold)."""
    hi = v.astype(np.float16).astype(np.float64)
    return hi + (v - hi).astype(np.float16).astype(np.float64) == v
