"""The references of tests/test_gpu_gemm_exact.py, checked without a GPU: for every shape the GPU tests launch,
* the integer operands leave the headroom that makes every fp32 partial sum exact,
* they are dense enough that a mis-summed k-step shows in every row it touches,
* and the Gaussian shapes leave room on BOTH sides of the ``floor16 / 32`` rule."""
import numpy as np
import pytest

from tests import gemm_ref as gr


def test_exactness_headroom_of_every_integer_shape():
    # |w (hi + lo)| <= 4 in every term (exact_planes keeps |hi + lo| <= 2), in units of 2^-6
    for K in gr.exact_k_values():
        assert 4 * K * 2 ** gr.LO_BITS < 2 ** 23, K
    for k64 in gr.W8_K64:                                    # int8 codes up to 127 against |hi + lo| <= 2
        assert gr.W8_CODE_MAX * 2 * (64 * k64) * 2 ** gr.LO_BITS < 2 ** 23, k64
    # the q|k|v sums stay inside fp16's range of exactly rounded values the test relies on
    assert all(4 * h <= 2048 for h in gr.QKV_HIDDEN)
    hi, lo6 = gr.exact_planes(64, 8416, 3, True)
    assert np.abs(64 * hi + lo6).max() <= 128 and set(np.unique(lo6)) == {-1, 0, 1} and set(np.unique(hi)) == {-2, -1, 0, 1, 2}
    w = gr.exact_weight(48, 8416, 3)
    assert np.abs(gr.exact_sum6(hi, lo6, w)).max() < 2 ** 23


@pytest.mark.parametrize("M,N,K,two", [(5, 48, 32, True), (17, 48, 288, True), (33, 48, 2304, False), (16, 16, 8416, True),
                                       (64, 112, 320, True)])
def test_fp32_accumulation_in_k_order_is_bit_equal_to_the_int64_reference(M, N, K, two):
    w, hi, lo, ref = gr.exact_operands(M, N, K, 5, two)
    got = gr.fp32_k_order([hi] if lo is None else [hi, lo], w)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), ref.view(np.int32))
    # ... and in another grouping: eight K shares summed separately, then added
    parts = [gr.fp32_k_order([p[:, c::8] for p in ([hi] if lo is None else [hi, lo])], w[:, c::8]) for c in range(8)]
    tot = np.zeros_like(ref)
    for p in parts:
        tot += p
    assert np.array_equal(tot.view(np.int32), ref.view(np.int32))


def test_plane_packer_round_trip_and_pad_rows():
    _, hi, _, _ = gr.exact_operands(21, 16, 96, 7, True, want_ref=False)
    f = gr.pack_plane(hi)
    assert f.shape == (2, 3, 64, 8)
    assert np.array_equal(gr.unpack_plane(f, 21), hi)
    full = gr.unpack_plane(f, 32)
    assert np.isnan(full[21:].astype(np.float32)).all()
    # lane 16 g + m of k-step s: row 16 mt + m, features 32 s + 8 g .. + 7
    assert np.array_equal(f[1, 2, 16 * 3 + 4], hi[16 + 4, 64 + 24:64 + 32])


def _shapes_for_sensitivity():
    out = []
    for rows in gr.EXACT_ROWS.values():
        out += [(M, 48, 32 * ks) for M in rows for ks in gr.EXACT_KS]
    out += [(M, N, 32 * ks) for M in gr.DEEP_ROWS for N in gr.DEEP_N for ks in gr.DEEP_KS]
    out += [(M, 48, 32 * ks) for M in gr.ROWS_M[:3] for ks in gr.ROWS_KS]
    return out


def test_integer_operands_are_dense_enough_to_fail():
    """Three mutants of the reference differ from it in at least one element of every row they touch."""
    for M, N, K in _shapes_for_sensitivity():
        w = gr.exact_weight(N, K, 9)
        hi, lo6 = gr.exact_planes(M, K, 9, True)
        ref = gr.exact_sum6(hi, lo6, w)
        KS = K // 32
        for s in sorted({0, KS // 2, KS - 1}):
            k0, k1 = 32 * s, 32 * s + 32
            # (1) one k-step's lo terms removed, in every row
            lo_m = lo6.copy(); lo_m[:, k0:k1] = 0
            assert (gr.exact_sum6(hi, lo_m, w) != ref).any(axis=1).all(), (M, N, K, s, "lo removed")
            # (2) one k-step counted twice
            twice = ref + gr.exact_sum6(hi, lo6, w, k0, k1)
            assert (twice != ref).any(axis=1).all(), (M, N, K, s, "k-step twice")
        if KS >= 2:
            # (3) the activations of two k-steps of one row exchanged (each then meets the other's weights)
            for row in sorted({0, M - 1}):
                hi_m, lo_m = hi.copy(), lo6.copy()
                for p in (hi_m, lo_m):
                    p[row, 0:32], p[row, K - 32:K] = p[row, K - 32:K].copy(), p[row, 0:32].copy()
                d = gr.exact_sum6(hi_m, lo_m, w) != ref
                assert d[row].any() and not np.delete(d, row, axis=0).any(), (M, N, K, row, "k-steps exchanged")


def test_slice_ranges_partition_k():
    for KS in set(gr.SLAB_KS) | set(gr.ROWS_KS) | set(gr.KSRED_KS):
        for S in set(gr.SLAB_SLICES) | set(gr.KSRED_S):
            r = gr.slice_ranges(KS, S)
            assert len(r) == S and r[0][0] == 0 and max(b for _, b in r) == KS
            assert all(a <= b for a, b in r) and all(r[i][1] == r[i + 1][0] or r[i + 1][0] == KS for i in range(S - 1))
    assert gr.slice_ranges(2, 16)[2:] == [(2, 2)] * 14
    assert gr.slice_ranges(10, 3, w8=True) == [(0, 4), (4, 8), (8, 10)] and gr.slice_ranges(2, 3, w8=True) == [(0, 2), (2, 2), (2, 2)]


def _split_cases():
    out = [(fam, M, min(N, 512), K, 1.0) for fam, M, N, K, _ in gr.SPLIT_STORE]      # (N only widens the maxima: 512 columns do)
    out += [("norm", M, N, K, 3.0) for M, N, K in gr.SPLIT_NORM]
    return out


@pytest.mark.parametrize("fam,M,N,K,xs", _split_cases())
def test_room_on_both_sides_of_the_split_rule(fam, M, N, K, xs):
    """An honest fp32 accumulation (plain k order, hi and lo interleaved) sits at least 2x below ``floor16 / 32``; losing the
    lo plane of one k-step of one row (the median choice) sits at least 2x above it."""
    assert K <= gr.SPLIT_K_MAX
    x, w = gr.gaussian_operands(M, N, K, 41, xs)
    wd = w
    if fam == "norm":
        gain = (1.0 + 0.2 * np.random.default_rng(5).standard_normal(K, dtype=np.float32)).astype(np.float16)
        x = gr.rmsnorm64(x, gain, 1e-5).astype(np.float32)
    if fam == "w8":
        amax = np.abs(w.astype(np.float32)).max(axis=1)
        q = np.clip(np.rint(w.astype(np.float32) * (127.0 / amax)[:, None]), -127, 127)
        wd = q.astype(np.float64) * (amax.astype(np.float64) / 127.0)[:, None]
    ref, floor16 = gr.split_floor(x, wd)
    hi, lo = gr.split_planes(x)
    honest = float(np.abs(gr.fp32_k_order([hi, lo], wd.astype(np.float32)).astype(np.float64) - ref).max())
    faulty = gr.lost_lo_step(x, wd)
    bar = floor16 / gr.SPLIT_RULE
    print(f"{fam} M={M} N={N} K={K}: floor16/honest = {floor16 / honest:.0f}, floor16/faulty = {floor16 / faulty:.1f}")
    assert honest * 2 <= bar, (floor16 / honest)
    assert faulty >= 2 * bar, (floor16 / faulty)


@pytest.mark.parametrize("inter", gr.SPLIT_ACT_INTER)
def test_room_under_the_split_rule_for_the_activation_epilogues(inter):
    """SiLU(g) * u and GELU evaluated in fp32 from fp32 sums sit at least 2x below ``max |fp16(ref) - ref| / 32``."""
    K, M = gr.SPLIT_ACT_K[inter], 20
    x, w = gr.gaussian_operands(M, 2 * min(inter, 256), K, 43)
    hi, lo = gr.split_planes(x)
    gu64 = x.astype(np.float64) @ w.astype(np.float64).T
    gu32 = gr.fp32_k_order([hi, lo], w)
    h = gu64.shape[1] // 2
    ref = gu64[:, :h] / (1 + np.exp(-gu64[:, :h])) * gu64[:, h:]
    got = (gu32[:, :h] / (np.float32(1) + np.exp(-gu32[:, :h]))) * gu32[:, h:]
    floor16 = float(np.abs(ref.astype(np.float16).astype(np.float64) - ref).max())
    assert got.dtype == np.float32 and float(np.abs(got - ref).max()) * 2 <= floor16 / gr.SPLIT_RULE
