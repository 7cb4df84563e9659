"""CPU checks of tests/attn_ref.py: the float64 attention against the oracle and a brute-force loop, the census expectation and
the headroom that makes the GPU threshold of tests/test_gpu_attn_pins.py decisive, and -- from the fp16-rounded operands
themselves -- that every score profile has the running-max property it is named for."""
import numpy as np
import pytest

from oracle import llama_oracle as orc
from tests import attn_ref as ar

ROUTE_IDS = [r.name for r in ar.ROUTES]


def test_attention64_matches_the_oracle_on_gaussian_operands():
    rng = np.random.default_rng(1)
    B, T, H, Hkv, D, past = 2, 9, 4, 2, 32, 11
    q = rng.standard_normal((B, T, H, D)).astype(np.float32)
    k = rng.standard_normal((B, Hkv, past + T, D)).astype(np.float32)
    v = rng.standard_normal((B, Hkv, past + T, D)).astype(np.float32)
    ref = orc.attention_core(q.transpose(0, 2, 1, 3), k, v, past, H // Hkv).transpose(0, 2, 1, 3).reshape(B, T, H * D)
    got = ar.attention64(q, k, v, past)
    # the oracle's softmax is float32
    np.testing.assert_allclose(got, ref, atol=2e-6, rtol=0)


def test_attention64_matches_a_per_row_loop_with_a_ragged_prefix():
    rng = np.random.default_rng(2)
    B, T, H, Hkv, D = 3, 5, 4, 2, 16
    pres, P = [3, 0, 7], 8
    q = rng.standard_normal((B, T, H, D))
    own_k, own_v = rng.standard_normal((B, Hkv, T + 2, D)), rng.standard_normal((B, Hkv, T + 2, D))     # (slack rows: never read)
    pk, pv = rng.standard_normal((Hkv, P, D)), rng.standard_normal((Hkv, P, D))
    got = ar.attention64(q, own_k, own_v, pres, prefix=(pk, pv))
    for b, pre in enumerate(pres):
        keys = np.concatenate([pk[:, :pre], own_k[b, :, :T]], axis=1)
        vals = np.concatenate([pv[:, :pre], own_v[b, :, :T]], axis=1)
        np.testing.assert_allclose(got[b], ar.attention_loop(q[b], keys, vals, pre), atol=1e-13, rtol=0)
        # ... and the same keys laid out as one arena per batch row
        one = ar.attention64(q[b:b + 1], keys[None], vals[None], pre)
        np.testing.assert_allclose(got[b], one[0], atol=1e-13, rtol=0)


def test_route_table_is_what_the_issue_lists():
    shapes = {(r.kind, r.B, r.H, r.Hkv, r.D, r.q_len, r.past, r.lo_mode) for r in ar.ROUTES}
    for want in [("plain64", 1, 4, 2, 128, 130, 100, "none"), ("plain64", 2, 4, 4, 64, 200, 77, "none"), ("plain64", 1, 2, 1, 128, 456, 0, "none"),
                 ("hp64", 1, 4, 2, 128, 50, 700, "none"), ("hp64", 1, 4, 4, 64, 64, 0, "none"), ("hp64", 1, 4, 4, 64, 64, 1, "none"),
                 ("rows32", 1, 8, 8, 128, 70, 600, "none"), ("rows32", 2, 64, 64, 64, 130, 3, "none"),
                 ("ring", 1, 8, 4, 128, 130, 77, "own"), ("ring", 1, 8, 4, 128, 65, 1200, "own"), ("ring", 1, 8, 4, 128, 128, 128, "all"),
                 ("ring", 1, 8, 4, 128, 200, 0, "all"), ("ring", 1, 8, 4, 128, 300, 513, "none"),
                 ("ring_prefix", 3, 4, 2, 128, 150, (37, 300, 128), "all"),
                 ("wide", 1, 4, 2, 128, 128, 640, "own"), ("wide", 1, 4, 2, 128, 130, 1000, "own"), ("wide", 1, 4, 2, 128, 259, 700, "own"),
                 ("wide", 1, 4, 2, 128, 300, 515, "own")]:
        assert want in shapes, want
    assert all(max(ar.pasts(r)) + r.q_len <= 1500 for r in ar.ROUTES)
    assert {ar.ROUTE[n].kind for n in ar.PROFILE_ROUTES} == {"plain64", "hp64", "rows32", "ring", "wide"}


@pytest.mark.parametrize("name", ROUTE_IDS)
@pytest.mark.parametrize("design", ["zero", "equal"])
def test_census_expectation_and_headroom(name, design):
    r = ar.ROUTE[name]
    ops = ar.census_operands(r, design)
    count, n = ar.census_counts(r, ops)
    assert (count.sum(axis=-1) == n[:, :, None]).all()
    ref = ar.reference(r, ops).reshape(r.B, r.q_len, r.H, r.D)
    want = np.repeat(count, r.H // r.Hkv, axis=2) / n[:, :, None, None]
    assert np.abs(ref - want).max() <= 1e-12
    # what makes abs(got * n - count) <= 0.25 decisive: fp16 output rounding of a correct kernel stays below 0.05 ...
    assert count.max() * 2.0 ** -11 <= 0.05
    # ... and one key too many moves its own column of got * n by n (count + 1) / (n + 1) - count = (n - count) / (n + 1), one too
    # few by (n - count) / (n - 1): above 0.9 for every row with at least 40 visible keys (every case has such rows; the shorter
    # rows of the no-past cases still move by more than 0.25 from n = 2 on: (n - 1) / (n + 1) >= 1 / 3)
    big = n >= 40
    assert big.any()
    worst = ((n[:, :, None, None] - count) / (n[:, :, None, None] + 1.0))[big].min()
    assert worst > 0.9, worst
    few = (n >= 2) & ~big
    if few.any():
        assert ((n[:, :, None, None] - count) / (n[:, :, None, None] + 1.0))[few].min() > 0.25
    if design == "equal":
        s = ar.scores_log2(r, ops) if r.kind != "ring_prefix" else None
        if s is not None:
            fin = np.where(np.isfinite(s), s, np.nan)
            assert np.nanmax(np.nanmax(fin, axis=-1) - np.nanmin(fin, axis=-1)) < 1e-9      # equal along the key axis
            assert np.nanstd(fin[:, :, 0]) > 0.1                                            # ... and different per row


def _rows_seeing(r, key):
    return np.arange(r.q_len) >= key - r.past


@pytest.mark.parametrize("rname", ar.PROFILE_ROUTES)
@pytest.mark.parametrize("first", [0, 32])
@pytest.mark.parametrize("pname", ar.PROFILES)
def test_profiles_have_their_running_max_property(pname, first, rname):
    r = ar.ROUTE[rname]
    ops = ar.profile_operands(pname, r)
    for key in ("q", "k", "v"):
        assert ops[key].dtype == np.float16 and np.isfinite(ops[key].astype(np.float64)).all()
    s = ar.scores_log2(r, ops)                                       # [H, T, S]
    tm = ar.tile_maxima(s, first)                                    # [H, T, ntiles]
    edges = ([0] if first else []) + list(range(first, s.shape[-1], ar.TK))
    tile_of = lambda key: int(np.searchsorted(edges, key, side="right") - 1)      # noqa: E731
    _, rows, marks = ar.profile_levels(pname, r.past, r.q_len)
    on = ar.online_rises(tm)
    if pname in ("late_spike", "own_spike"):
        t = tile_of(marks[0])
        assert t >= 1
        see = _rows_seeing(r, marks[0])
        assert see.sum() >= 16 and (on[:, see, t - 1] >= 20).all()
        if pname == "late_spike":
            assert r.past - ar.TK <= marks[0] < r.past and see.all()
        else:
            assert (~see).sum() >= 16 and np.nanmax(np.where(np.isfinite(on[:, ~see]), on[:, ~see], np.nan)) < 4
    elif pname == "early_spike":
        assert tile_of(0) == 0
        later = np.where(np.isfinite(tm[..., 1:]), tm[..., 1:], -1e9).max(axis=-1)
        assert (tm[..., 0] - later >= 20).all()
    elif pname == "row_spike":
        t = tile_of(marks[0])
        groups = {i // 16 for i in rows}
        assert len(groups) == 3 and 0 in groups and (r.q_len - 1) // 16 in groups
        fin = np.where(np.isfinite(on), on, -1e9).max(axis=-1)       # [H, T]: the largest rise of each row
        for g in groups:
            members = np.arange(16 * g, min(16 * g + 16, r.q_len))
            jumped = (fin[:, members] >= 16)
            assert (jumped.sum(axis=1) == 1).all()
            assert (on[:, [i for i in rows if i // 16 == g], t - 1] >= 16).all()
            assert (fin[:, members][~jumped] < 4).all()
    elif pname in ("stairs_up", "threshold"):
        de = ar.deferred_rises(tm)
        assert ((de > 5) & (de < 7.9)).any(axis=-1).all()
        assert ((de > 8.1) & (de < 12)).any(axis=-1).all()
        if pname == "stairs_up":      # P stays below 2^12 under the deferral: no rise the kernel does not follow reaches it
            assert de[np.isfinite(de)].max() < 12
    elif pname == "stairs_down":
        assert on[np.isfinite(on)].max() < 1
        assert (tm[..., 0] - np.where(np.isfinite(tm), tm, 1e9).min(axis=-1) > 2 * ar.STAIR - 1).all()      # ... while the maxima fall


def test_fp16_p_loss_is_far_below_the_plain_tolerance():
    """The plain routes are held to atol 4e-3: what fp16 P alone costs on the profiles (reference arithmetic) stays below it."""
    for rname in ("plain64-130-400", "rows32-70-600"):
        for pname in ar.PROFILES:
            assert ar.fp16_p_loss(ar.ROUTE[rname], ar.profile_operands(pname, ar.ROUTE[rname])) < 1e-3
