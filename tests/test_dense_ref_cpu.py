"""The references of tests/test_gpu_dense_exact.py, checked without a GPU: for every shape the GPU tests launch,
* the integer operands (weight scales, ADD base values, LLM.int8 codes and the rotated q|k|v sums included) leave the headroom
  that makes every fp32 partial sum exact,
* the shape lands, under the restatement of launch_dense_tile / launch_dense_splitk in tests/dense_ref.py, on the tile width,
  plane count, epilogue and split it is annotated with, and the tables together reach all 20 gemm_dense_kernel instantiations
  and both dense_reduce_kernels,
* and the Gaussian shapes leave room on BOTH sides of the ``floor16 / 32`` rule (a lost lo plane of one 16-deep slab of one
  row: the MFMA of pc_gemm_dense is 32x32x16)."""
import numpy as np
import pytest

from tests import dense_ref as dr
from tests import gemm_ref as gr


# ---------------------------------------------------------------------------------------------------
# headroom
# ---------------------------------------------------------------------------------------------------

def test_exactness_headroom_of_every_integer_shape():
    # products w (hi + lo) are multiples of 2^-6 of magnitude <= 4 (gemm_ref.exact_planes keeps |hi + lo| <= 2): every partial sum
    # over at most K of them, in any grouping, is a multiple of 2^-6 below 4 K, exact in fp32 while 4 K 2^6 < 2^23 -- with the
    # ADD base (integers up to BASE_MAX) on top
    for M, N, K in dr.exact_cases():
        assert (4 * K + dr.BASE_MAX) * 2 ** gr.LO_BITS < 2 ** 23, (M, N, K)
    # wscale: the sum times 2^e, e in [-2, 2]: a multiple of 2^-8 below 16 K, plus the base
    lo, hi = dr.WSCALE_EXP
    for c in dr.WSCALE_CASES:
        assert (4 * c.K * 2 ** hi + dr.BASE_MAX) * 2 ** (gr.LO_BITS - lo) < 2 ** 23, c
    # the split-K slabs are partial sums (exact as above); dense_reduce_kernel adds them and the base in slice order: the same bound
    for c in dr.SPLIT_CASES:
        assert (4 * c.K + dr.BASE_MAX) * 2 ** gr.LO_BITS < 2 ** 23, c
    # LLM.int8: |code_x code_w| <= 127 * 2 per term; times w_scale x_scale in [2^-2, 2^2] (exact), plus corr, plus the base
    e_lo, e_hi = dr.A8_EXP
    for c in dr.A8_CASES:
        assert dr.A8_CODE_MAX * dr.A8_W_MAX * c.K < 2 ** 23, c                        # the integer accumulator itself
        top = dr.A8_CODE_MAX * dr.A8_W_MAX * c.K * 4 ** e_hi + dr.A8_CORR_MAX + dr.BASE_MAX
        assert top * 4 ** (-e_lo) < 2 ** 23, c                                        # in units of 2^(2 e_lo)
    # ... and the generated operands keep what the bounds assume
    hi_, lo6 = gr.exact_planes(300, 2056, 3, True)
    assert np.abs(64 * hi_ + lo6).max() <= 128 and set(np.unique(lo6)) == {-1, 0, 1} and set(np.unique(hi_)) == {-2, -1, 0, 1, 2}
    assert np.abs(gr.exact_sum6(hi_, lo6, gr.exact_weight(132, 2056, 3))).max() < 2 ** 23
    assert float(np.abs(dr.base_ints(300, 132, 1)).max()) == dr.BASE_MAX


@pytest.mark.parametrize("c", dr.A8_CASES[:2], ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_a8_operands_are_exact_in_fp32(c):
    q, w, we, xe, corr = dr.a8_operands(c.M, c.N, c.K, 1300)
    assert np.abs(q).max() == dr.A8_CODE_MAX and (np.abs(q).max(axis=1) == dr.A8_CODE_MAX).all() and np.abs(w).max() == dr.A8_W_MAX
    assert we.min() == dr.A8_EXP[0] and we.max() == dr.A8_EXP[1] and np.abs(corr).max() == dr.A8_CORR_MAX
    assert dr.A8_EXP[0] <= xe.min() and xe.max() <= dr.A8_EXP[1] and (c.M == 1 or (xe.min(), xe.max()) == dr.A8_EXP)
    plain, with_corr = dr.a8_expect(q, w, we, xe, corr)
    for v in (plain, with_corr, with_corr + dr.base_ints(c.M, c.N, 5)):
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    # the epilogue's own order in fp32: (sum * w_scale) * x_scale + corr
    s32 = (q @ w.T).astype(np.float32) * np.exp2(we).astype(np.float32)[None, :]
    s32 = s32 * np.exp2(xe).astype(np.float32)[:, None] + corr.astype(np.float32)
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), with_corr)


@pytest.mark.parametrize("c", dr.ROPE_CASES, ids=lambda c: f"B{c.B}-H{c.H}-Hkv{c.Hkv}-q{c.q_len}-K{c.K}")
def test_rotated_sums_are_exact_and_fit_the_output_planes(c):
    """The rotation table holds all five (cos, sin) choices and varies along rows and feature pairs; the rotated sums are
    multiples of 2^-7 far below 2^23 units (the epilogue's fp32 multiply-adds are exact in either order, fused or not), and
    every one of them is held exactly by an fp16 hi plane plus an fp16 residual plane."""
    M, cols = dr.rope_dims(c)
    cs = dr.rotation_table(M)
    assert cs.shape == (M, 64, 2) and cs.dtype == np.float32
    seen = {tuple(v) for v in cs.reshape(-1, 2)}
    assert seen == set(dr.ROT_CHOICES)
    assert (cs[1:] != cs[:-1]).any(axis=(1, 2)).all() and (cs[:, 1:] != cs[:, :-1]).any(axis=(0, 2)).all()
    assert 2 * 4 * c.K * 2 ** (gr.LO_BITS + 1) < 2 ** 23
    heads = min(c.H + 2 * c.Hkv, 6)                                  # (more heads only repeat the same bound)
    H = min(c.H, heads - 2)
    Hkv = (heads - H) // 2
    w = gr.exact_weight((H + 2 * Hkv) * 128, c.K, 1200)
    hi, lo6 = gr.exact_planes(M, c.K, 1201, c.two)
    sums = gr.exact_sum6(hi, lo6, w).astype(np.float64) * gr.LO_UNIT
    e = dr.rope_expect(sums, cs, H, Hkv)
    assert np.array_equal(np.rint(e * 128), e * 128) and np.abs(e).max() <= 2 * 4 * c.K
    assert dr.split_is_exact(e).all()
    # fp32 evaluation in the kernel's form
    x = sums.astype(np.float32).reshape(M, H + 2 * Hkv, 2, 64)
    cc, ss = cs[:, None, :, 0], cs[:, None, :, 1]
    a = x[:, :H + Hkv, 0] * cc - x[:, :H + Hkv, 1] * ss
    assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), e.reshape(M, -1, 2, 64)[:, :H + Hkv, 0])
    # v heads are not rotated, q and k heads are (somewhere)
    assert np.array_equal(e[:, H + Hkv:].reshape(M, -1), sums[:, (H + Hkv) * 128:])
    assert (e[:, :H + Hkv].reshape(M, -1) != sums[:, :(H + Hkv) * 128]).any()


def test_fp32_accumulation_in_slab_order_is_bit_equal_to_the_int64_reference():
    """The dense kernel's grouping: 16-deep slabs, hi plane then lo plane, K slices summed apart and added in slice order."""
    for c in (dr.STORE_ADD_NARROW[5], dr.SPLIT_CASES[1]):
        M, N, K = min(c.M, 20), min(c.N, 64), c.K
        w, hi, lo, ref = gr.exact_operands(M, N, K, 5, True)
        tot = np.zeros_like(ref)
        for k0 in range(0, K, 9 * dr.BK):
            part = np.zeros_like(ref)
            for s0 in range(k0, min(k0 + 9 * dr.BK, K), 16):
                for p in (hi, lo):
                    part += p[:, s0:s0 + 16].astype(np.float32) @ w[:, s0:s0 + 16].astype(np.float32).T
            tot += part
        assert tot.dtype == np.float32 and np.array_equal(tot.view(np.int32), ref.view(np.int32))


def test_integer_operands_are_dense_enough_to_fail():
    """Mutants of the reference at the dense kernel's granularity differ from it in every row they touch: the lo plane of one
    16-deep slab lost, one slab counted twice, and the first chunk behind K read as if it were the last chunk in front of it."""
    for K in dr.K_EDGE:
        for M in (1, 130):
            N = 132
            w = gr.exact_weight(N, K, 9)
            hi, lo6 = gr.exact_planes(M, K, 9, True)
            ref = gr.exact_sum6(hi, lo6, w)
            slabs = list(range(0, K, 16))
            for s0 in sorted({slabs[0], slabs[len(slabs) // 2], slabs[-1]}):
                s1 = min(s0 + 16, K)
                lo_m = lo6.copy(); lo_m[:, s0:s1] = 0
                hit = (gr.exact_sum6(hi, lo_m, w) != ref).any(axis=1)
                # (an 8-feature half slab at the end of K: a row's eight lo terms are all zero once in some hundred rows)
                assert hit.all() if s1 - s0 == 16 else hit.mean() > 0.95, (M, K, s0, "lo slab lost")
                assert (ref + gr.exact_sum6(hi, lo6, w, s0, s1) != ref).any(axis=1).all(), (M, K, s0, "slab twice")
            if K > 8:
                again = ref + gr.exact_sum6(hi, lo6, w, K - 8, K)
                assert (again != ref).any(axis=1).all(), (M, K, "chunk behind K = the chunk in front of it")


# ---------------------------------------------------------------------------------------------------
# selection and coverage
# ---------------------------------------------------------------------------------------------------

def test_every_table_entry_selects_what_it_is_annotated_with():
    for c in dr.STORE_ADD_NARROW + dr.STORE_ADD_WIDE + dr.WSCALE_CASES:
        for epi in (dr.EPI_STORE, dr.EPI_ADD):
            assert dr.plan(c.M, c.N, c.K, epi) == dr.Plan(c.tile, 1, dr.ceil_div(c.K, 64), 0), c
        assert c.N % 4 == 0 and c.N % 128 != 0 and c.K % 8 == 0, c                  # ragged N
    for c in dr.SPLIT_CASES:
        need = c.kslices * c.M * c.N * 4
        for epi in (dr.EPI_STORE, dr.EPI_ADD):
            p = dr.plan(c.M, c.N, c.K, epi, ws_bytes=need)
            assert p == dr.Plan(256, c.kslices, c.kper, len(c.steps)) and tuple(dr.slice_steps(c.K, p.kper)) == c.steps, c
            assert dr.plan(c.M, c.N, c.K, epi, ws_bytes=need - 1).slabs == 0, c       # one byte short: the plain form
            assert dr.plan(c.M, c.N, c.K, epi, ws_bytes=need, xscale=True).slabs == 0, c
        assert c.K % 64 != 0, c                                                      # the K tail ends the last slice
    for (c, _), big in zip(dr.SPLIT_REFUSED, (1 << 30, 1 << 30)):
        assert dr.plan(c.M, c.N, c.K, dr.EPI_STORE, ws_bytes=big) == dr.Plan(c.tile, 1, dr.ceil_div(c.K, 64), 0), c
    for c in dr.ROPE_CASES:
        assert dr.plan(*dr.rope_dims(c), c.K, dr.EPI_ROPE).tile == c.tile, c
        assert c.Hkv < c.H and (c.lo_row0 == 0 if isinstance(c.past, tuple) else c.lo_row0 <= c.past), c
    for c in dr.A8_CASES:
        assert dr.plan(c.M, c.N, c.K, dr.EPI_ADD, ws_bytes=1 << 30, xscale=True) == dr.Plan(c.tile, 1, dr.ceil_div(c.K, 64), 0), c
    for c in dr.ACT_CASES:
        assert dr.plan(c.M, dr.act_cols(c), c.K, dr.EPI_SILU if c.act == "silu" else dr.EPI_GELU).tile == c.tile, c
        assert c.inter % 4 == 0 and c.inter % 32 != 0 and c.K <= gr.SPLIT_K_MAX, c
    for c in dr.SPLIT_FLOOR:
        p = dr.plan(c.M, c.N, c.K, dr.EPI_ADD if c.form == "add" else dr.EPI_STORE, ws_bytes=(1 << 24) if c.form == "ws" else 0)
        assert p.tile == c.tile and (p.slabs >= 2) == (c.form == "ws") and c.K <= gr.SPLIT_K_MAX, c


def test_grid_edges_named_in_the_tables_exist():
    """Both tiles see a grid with fewer than 8 panels and one whose panel count is no multiple of 8 (workgroups that return at
    ni >= nb), and every K / 8 class is there."""
    for table, tile in ((dr.STORE_ADD_NARROW, 128), (dr.STORE_ADD_WIDE + tuple(dr.Case(c.M, c.N, c.K, 256, c.edge) for c in dr.SPLIT_CASES), 256)):
        nbs = {dr.grid_panels(c.M, c.N, dr.EPI_STORE, tile)[1] for c in table}
        assert any(nb < 8 for nb in nbs) and any(nb > 8 and nb % 8 for nb in nbs), (tile, nbs)
        ks = {c.K for c in table}
        assert {8, 64, 72} <= ks and any(dr.ceil_div(k, 64) % 2 == 1 and 8 < k % 64 for k in ks) and any(k > 512 and k % 64 for k in ks), (tile, ks)
    assert {c.M for c in dr.STORE_ADD_NARROW} == {1, 127, 130, 257, 300}


def test_the_tables_reach_all_22_kernels():
    seen = set()
    for p, epi, two in dr.launches():
        seen |= dr.kernels(p, epi, two)
    assert len(dr.ALL_KERNELS) == 22 and seen == dr.ALL_KERNELS, sorted(dr.ALL_KERNELS - seen)


def test_recorded_kernel_names_and_call_counts_match_the_restatement():
    """profiles/dense_exact_kernel_stats.txt (one profiler run of tests/test_gpu_dense_exact.py on the GPU) names all 22 kernels,
    and every one was called exactly as often as the restatement predicts for the launches of that file.  After a change of the
    tables or of the launch rules in pc_gemm_dense.hip the profile is recorded again."""
    import collections
    import csv
    import os
    import re
    want = collections.Counter()
    for p, epi, two in dr.launches():
        want.update(dr.kernels(p, epi, two))
    got = collections.Counter()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dense_exact_kernel_stats.txt")
    with open(path) as f:
        for row in csv.reader(line for line in f if not line.startswith("#")):
            m = re.search(r"gemm_dense_kernel<(\d), (\d), (true|false), false, false>", row[0])
            if m:
                got[("gemm", int(m[1]), int(m[2]), m[3] == "true")] += int(row[1])
            m = re.search(r"dense_reduce_kernel<(true|false)>", row[0])
            if m:
                got[("reduce", m[1] == "true")] += int(row[1])
    assert set(got) == dr.ALL_KERNELS, sorted(dr.ALL_KERNELS - set(got))
    assert got == want, sorted((k, want[k], got[k]) for k in want if want[k] != got[k])


def test_the_narrow_split_k_branch_is_unreachable():
    """launch_dense_splitk's ``narrow`` needs 256 / b256 < 2 and 256 / b128 >= 2 with b128 >= b256: never, whatever the shape."""
    for M in (1, 100, 129, 300, 1000, 4096, 16384, 40000):
        for N in (4, 128, 132, 256, 260, 1156, 4096, 16644, 32772):
            sp = dr.split_slices(M, N, 1 << 16, dr.EPI_STORE, 1 << 40)
            assert sp is None or sp[0] == 256, (M, N)


# ---------------------------------------------------------------------------------------------------
# room around the rule
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", dr.SPLIT_FLOOR, ids=lambda c: f"{c.family}-{c.M}x{c.N}x{c.K}")
def test_room_on_both_sides_of_the_split_rule(c):
    """An honest fp32 accumulation (plain k order, hi and lo interleaved; the Gaussian base added last for the ADD case) sits at
    least 2x below ``floor16 / 32``; losing the lo plane of one 16-deep slab of one row (the median choice) at least 2x above."""
    assert c.K <= gr.SPLIT_K_MAX
    N = min(c.N, 512)                                                 # (N only widens the maxima: 512 columns do)
    x, w = gr.gaussian_operands(c.M, N, c.K, 41)
    ref, floor16 = gr.split_floor(x, w)
    hi, lo = gr.split_planes(x)
    if c.form == "one":                                               # its own reference: fp16(x) w^T
        ref = hi.astype(np.float64) @ w.astype(np.float64).T
        got = gr.fp32_k_order([hi], w)
    else:
        got = gr.fp32_k_order([hi, lo], w)
    if c.form == "add":
        base = np.random.default_rng(1).standard_normal((c.M, N)).astype(np.float32)
        got, ref = got + base, ref + base.astype(np.float64)
    honest = float(np.abs(got.astype(np.float64) - ref).max())
    faulty = gr.lost_lo_step(x, w, depth=16)
    bar = floor16 / gr.SPLIT_RULE
    print(f"{c.family} M={c.M} N={N} K={c.K}: honest = {honest:.3e}, rule = {bar:.3e}, lost slab (median) = {faulty:.3e}")
    assert got.dtype == np.float32 and honest * 2 <= bar, (floor16 / honest)
    if c.form != "one":                                               # (no lo plane to lose)
        assert faulty >= 2 * bar, (floor16 / faulty)


def _act64(z, act, inter):
    if act == "silu":
        g, u = z[:, :inter], z[:, inter:]
        return g / (1 + np.exp(-g)) * u
    from math import erf
    return 0.5 * z * (1 + np.vectorize(erf)(z * 0.7071067811865476))


@pytest.mark.parametrize("c", dr.ACT_CASES, ids=lambda c: f"{c.act}-{c.M}x{c.inter}x{c.K}-{'two' if c.two else 'one'}{'-ws' if c.wscale else ''}")
def test_room_on_both_sides_of_the_rule_for_the_activation_epilogues(c):
    """SiLU(g) * u and GELU evaluated in fp32 from fp32 sums sit at least 2x below ``max |fp16(ref) - ref| / 32``; with two planes,
    the same evaluation on sums that lost the lo plane of one 16-deep slab of one row (the median choice) sits at least 2x above."""
    inter = min(c.inter, 128)                                         # (more columns only widen the maxima)
    N = 2 * inter if c.act == "silu" else inter
    M = min(c.M, 64)
    x, w = gr.gaussian_operands(M, N, c.K, 43)
    sc = dr.act_wscale(N) if c.wscale else np.ones(N, dtype=np.float32)
    hi, lo = gr.split_planes(x)
    xs = x if c.two else hi
    z64 = (xs.astype(np.float64) @ w.astype(np.float64).T) * sc.astype(np.float64)
    ref = _act64(z64, c.act, inter)
    floor16 = float(np.abs(ref.astype(np.float16).astype(np.float64) - ref).max())
    bar = floor16 / gr.SPLIT_RULE
    z32 = gr.fp32_k_order([hi, lo] if c.two else [hi], w) * sc[None, :]
    if c.act == "silu":
        got = (z32[:, :inter] / (np.float32(1) + np.exp(-z32[:, :inter]))) * z32[:, inter:]
    else:
        got = _act64(z32.astype(np.float64), c.act, inter)            # (erf in fp32 is not in numpy: the sums carry the error)
    honest = float(np.abs(got.astype(np.float64) - ref).max())
    assert honest * 2 <= bar, (honest, bar)
    if not c.two:
        return
    worst = []
    lo64, w64 = lo.astype(np.float64), w.astype(np.float64)
    for s0 in range(0, c.K, 16):
        dz = (lo64[:, s0:s0 + 16] @ w64[:, s0:s0 + 16].T) * sc.astype(np.float64)
        worst.append(np.abs(_act64(z64 - dz, c.act, inter) - ref).max(axis=1))
    faulty = float(np.median(np.stack(worst)))
    print(f"{c.act} M={M} inter={inter} K={c.K}: honest = {honest:.3e}, rule = {bar:.3e}, lost slab (median) = {faulty:.3e}")
    assert faulty >= 2 * bar, (faulty, bar)
