"""References for the many-row attention kernels (attn_fwd_kernel plain and HP, attn_fwd32_kernel, attn_ring_kernel,
attn_wide_kernel + own-rows ring partial + attn_combine_kernel; prompt-cache_amd/csrc/pc_attn*.hip): numpy only, no GPU.

* ``attention64``: float64 softmax attention under the index-order causal mask (row i sees keys < past + i + 1), GQA by head
  repetition, optionally behind a shared prefix of per-batch-row length.
* the ROUTES of tests/test_gpu_attn_pins.py, each with the dispatch rule that selects it (pc_attn.hip ``use_rows32`` /
  ``choose_nsplit``, pc_attn_ring.hip ``ring_eligible`` / ``ring_nsplit``, pc_attn_wide.hip ``wide_eligible`` / ``wide_nsplit``).
* census operands: one-hot V and scores that are equal along the key axis, so that every visible key weighs exactly 1 / n_i and
  the output times n_i is an integer count per column: one key too many or too few moves a column by ~1.
* score profiles that drive the running-max paths: a Gaussian background at scale 0.5 plus a rank-one part along feature 0
  (q[..., 0] = PROFILE_A for the rows that take part, k[j, 0] = level_j / unit(D)), so that the score of key j in log2 units is
  level_j + a background of about +-1.5.  Feature 0 of the background (and of every lo plane) is zero: no cross-talk.

Where the steps sit.  Every kernel here walks 64-key tiles.  The wide kernel's tiles are absolute (key0 = 64 t) and its slices at
the test shapes are two or three tiles long starting at a multiple of 128 keys (wide_nsplit: ceil(past / 64) / 2 slices), so a
step ON a multiple of 128 would always fall between two slices and never reach a running max.  The stairs therefore step at ODD
multiples of 64 (64, 192, 320, ...: between the two tiles of a slice, between tiles of any tiling from key 0, inside a tile of a
tiling from key 32), with the third step moved to key 37 of its tile (293) for the in-tile case.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

LOG2E = 1.4426950408889634
TK = 64                      # pc_attn_common.h: keys per LDS tile
DEFER_LOG2 = 8.0             # pc_attn_wide.hip kDeferLog2
PROFILE_A = 4.0              # q[..., 0] of the rows that take part in a profile
SPIKE = 30.0                 # log2 units
ROW_SPIKE = 24.0
STAIR = 5.75                 # "about 6": two steps (11.5) stay inside the (8.1, 12) window of the CPU check
# Q's background scale.  Between two tiles the maxima of a scale-0.5 background differ by up to ~0.8 log2 units over the rows of a
# case, which would carry a 7.5 step across the 7.9 / 8.1 windows of the CPU check (and 2 x STAIR across 12): the three profiles
# whose steps are measured against kDeferLog2 scale Q's background by 1/4 (differences <= ~0.2); the spikes keep 0.5.
Q_BG = {"stairs_up": 0.125, "stairs_down": 0.125, "threshold": 0.125}
PROFILES = ("late_spike", "early_spike", "own_spike", "row_spike", "stairs_up", "threshold", "stairs_down")

# kind: plain64 = attn_fwd_kernel<D, false>, hp64 = attn_fwd_kernel<D, true> (q_lo given; PC_ATTN_NO_RING=1 at D = 128, where the
# ring kernel would take >= 33 such rows), rows32 = attn_fwd32_kernel, ring, ring_prefix, wide.
# past: int, or the prefix lengths of the batch rows (ring_prefix).  lo_mode: residual K / V planes "none" | "own" | "all".
# splits: whether the launch writes split-KV partials (tests/test_gpu_attn_pins.py::test_splits_really_ran holds it to that).
Route = namedtuple("Route", "name kind B H Hkv D q_len past lo_mode splits rule")

ROUTES = (
    # use_rows32: q_len > 64 and (B H ceil(q / 128) >= 256 or kv >= 8 q) -- all false below -> the 64-row kernel; no q_lo -> plain.
    # choose_nsplit: ns = (320 + base / 2) / base with base = B H ceil(q / 64), capped by kv / 128 (two tiles per split)
    Route("plain64-130-100", "plain64", 1, 4, 2, 128, 130, 100, "none", False, "base 12 -> 27, kv / 128 = 1 -> 1 split"),
    Route("plain64-d64-200-77", "plain64", 2, 4, 4, 64, 200, 77, "none", True, "base 32 -> 10, kv / 128 = 2 -> 2 splits"),
    Route("plain64-456-0", "plain64", 1, 2, 1, 128, 456, 0, "none", True, "base 16 -> 20, kv / 128 = 3 -> 3 splits"),
    # (added for the profiles: the table's plain routes have at most 100 staged keys)  kv = 530 >= 4 q: the cost rule, 3 splits
    Route("plain64-130-400", "plain64", 1, 4, 2, 128, 130, 400, "none", True, "kv 530 < 8 q = 1040 -> 64-row; cost rule -> 3 splits"),
    # q_len <= 64: the HP form whatever the planes; q_lo given.  kv = 750 >= 4 q: cost rule over T = 12 tiles -> 4 splits + merge
    Route("hp64-50-700", "hp64", 1, 4, 2, 128, 50, 700, "none", True, "q <= 64 -> HP; cost rule -> 4 splits"),
    Route("hp64-d64-64-0", "hp64", 1, 4, 4, 64, 64, 0, "none", False, "kv / 128 = 0 -> 1 split"),
    Route("hp64-d64-64-1", "hp64", 1, 4, 4, 64, 64, 1, "none", False, "kv = 65: kv / 128 = 0 -> 1 split, a one-key second tile"),
    Route("rows32-70-600", "rows32", 1, 8, 8, 128, 70, 600, "none", True, "kv 670 >= 8 q = 560 -> 32-row; cost rule -> 4 splits"),
    Route("rows32-d64-130-3", "rows32", 2, 64, 64, 64, 130, 3, "none", False, "B H ceil(130 / 128) = 256 -> 32-row; base 256 -> 1 split"),
    # ring_eligible: D = 128, q_lo, q_len >= 33, no ALiBi / tail / small.  ring_nsplit minimises rounds (stages + 1) + merge
    Route("ring-130-77-own", "ring", 1, 8, 4, 128, 130, 77, "own", False, "units 16, 207 keys: 2 stages -> 1 split"),
    Route("ring-65-1200-own", "ring", 1, 8, 4, 128, 65, 1200, "own", True, "units 8, 1265 keys -> 5 splits"),
    Route("ring-128-128-all", "ring", 1, 8, 4, 128, 128, 128, "all", False, "units 8, 256 keys -> 1 split"),
    Route("ring-200-0-all", "ring", 1, 8, 4, 128, 200, 0, "all", False, "units 16, 200 keys -> 1 split"),
    Route("ring-300-513-none", "ring", 1, 8, 4, 128, 300, 513, "none", True, "units 24, 813 keys -> 7 splits"),
    Route("ring-prefix", "ring_prefix", 3, 4, 2, 128, 150, (37, 300, 128), "all", False, "units 24, 450 keys -> 1 split"),
    # wide_eligible: ring_eligible, B = 1, past >= PC_ATTN_WIDE_MIN (256 here), q_len >= 128, residual planes with lo_row0 < 0.
    # wide_nsplit = min(256 / H, ceil(past / 64) / 2, 15) slices + the own-rows partial; R = ceil(groups per q-block / 8)
    Route("wide-128-640-R1", "wide", 1, 4, 2, 128, 128, 640, "own", True, "8 groups: R = 1; 5 slices of 2 tiles + own"),
    Route("wide-130-1000-R2", "wide", 1, 4, 2, 128, 130, 1000, "own", True, "9 groups: R = 2; 8 slices of 2 tiles, the last tile partial"),
    Route("wide-259-700-R3", "wide", 1, 4, 2, 128, 259, 700, "own", True, "17 groups: R = 3; 5 slices of 3 / 3 / 3 / 2 tiles"),
    Route("wide-300-515-2blk", "wide", 1, 4, 2, 128, 300, 515, "own", True, "19 groups: two q-blocks of 10 + 9, R = 2; 4 slices"),
)
ROUTE = {r.name: r for r in ROUTES}
N_TRUNK = 320                # rows of the shared prefix planes (ring_prefix)
WIDE_MIN = "256"             # PC_ATTN_WIDE_MIN of the wide routes

# one route of each kernel for the running-max profiles (+ all three wide R values, + a second ring route: ragged last group)
PROFILE_ROUTES = ("plain64-130-400", "hp64-50-700", "rows32-70-600", "ring-65-1200-own", "ring-300-513-none",
                  "wide-128-640-R1", "wide-130-1000-R2", "wide-259-700-R3")


def pasts(r):
    return list(r.past) if isinstance(r.past, tuple) else [r.past] * r.B


def split_precision(r):
    return r.kind not in ("plain64", "rows32")


# ---------------------------------------------------------------------------------------------------
# float64 attention
# ---------------------------------------------------------------------------------------------------

def attention64(q, k, v, past_per_row, prefix=None):
    """q [B, T, H, D]; k, v [B, Hkv, rows, D]; past_per_row: int or one per batch row.  Without ``prefix`` batch row b attends to
    k[b, :, :past_b + T]; with ``prefix = (pk, pv)`` ([Hkv, P, D]) to pk[:, :past_b] followed by k[b, :, :T].  Row i sees keys
    < past_b + i + 1.  Returns float64 [B, T, H * D]."""
    q = np.asarray(q, dtype=np.float64)
    B, T, H, D = q.shape
    pl = [int(past_per_row)] * B if np.ndim(past_per_row) == 0 else [int(x) for x in past_per_row]
    out = np.empty((B, T, H * D), dtype=np.float64)
    for b in range(B):
        if prefix is None:
            kk, vv = np.asarray(k[b], dtype=np.float64)[:, :pl[b] + T], np.asarray(v[b], dtype=np.float64)[:, :pl[b] + T]
        else:
            kk = np.concatenate([np.asarray(prefix[0], dtype=np.float64)[:, :pl[b]], np.asarray(k[b], dtype=np.float64)[:, :T]], axis=1)
            vv = np.concatenate([np.asarray(prefix[1], dtype=np.float64)[:, :pl[b]], np.asarray(v[b], dtype=np.float64)[:, :T]], axis=1)
        rep = H // kk.shape[0]
        kk, vv = np.repeat(kk, rep, axis=0), np.repeat(vv, rep, axis=0)
        s = np.einsum("thd,hsd->hts", q[b], kk) / np.sqrt(D)
        vis = np.arange(pl[b] + T)[None, :] <= (pl[b] + np.arange(T))[:, None]
        s = np.where(vis[None], s, -np.inf)
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        out[b] = np.einsum("hts,hsd->thd", p, vv).reshape(T, H * D)
    return out


def attention_loop(q, keys, values, past):
    """Brute force, one (row, head) at a time: q [T, H, D], keys / values [Hkv, S, D] (the visible sequence of ONE batch row)."""
    T, H, D = q.shape
    rep = H // keys.shape[0]
    out = np.zeros((T, H, D))
    for i in range(T):
        nvis = past + i + 1
        for h in range(H):
            s = np.array([float(np.dot(q[i, h].astype(np.float64), keys[h // rep, j].astype(np.float64))) for j in range(nvis)]) / np.sqrt(D)
            w = np.exp(s - s.max())
            w /= w.sum()
            for j in range(nvis):
                out[i, h] += w[j] * values[h // rep, j].astype(np.float64)
    return out.reshape(T, H * D)


# ---------------------------------------------------------------------------------------------------
# operands: a dict of numpy arrays in the launch's own layout
#   q, q_lo [B, T, H, D] fp16 (q_lo None on the plain routes)
#   k, v [B, Hkv, S, D] fp16 valid rows (ring_prefix: the batch rows' OWN rows, S = T), k_lo, v_lo the same shape or None --
#   zero where the route's lo_mode carries no residual row
#   trunk_k, trunk_v, trunk_k_lo, trunk_v_lo [Hkv, N_TRUNK, D] (ring_prefix only)
# ---------------------------------------------------------------------------------------------------

def _f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def _lo_rows(r):
    """Key rows [lo, hi) of the launch's own K / V arrays that have a residual row."""
    if r.kind == "ring_prefix":
        return 0, r.q_len
    S = r.past + r.q_len
    return {"none": (0, 0), "own": (r.past, S), "all": (0, S)}[r.lo_mode]


def census_v(Hkv, S, D, b, j0=0):
    """V [Hkv, S, D] fp16: row (h, j) is one-hot at column (j0 + j + 7 h + 3 b) % D."""
    v = np.zeros((Hkv, S, D), dtype=np.float16)
    h, j = np.meshgrid(np.arange(Hkv), np.arange(S), indexing="ij")
    v[h, j, (j0 + j + 7 * h + 3 * b) % D] = 1.0
    return v


def census_operands(r, design, seed=0):
    """design "zero": Q = 0 (every score is 0).  "equal": Q Gaussian, every key row of a kv head equal to one Gaussian vector
    (scores equal along the key axis, different per row).  Residual K / V planes are zero; q_lo is zero / small Gaussian."""
    assert design in ("zero", "equal")
    rng = np.random.default_rng([seed, ROUTES.index(r), design == "equal"])
    B, T, H, Hkv, D = r.B, r.q_len, r.H, r.Hkv, r.D
    hp = split_precision(r)
    S = T if r.kind == "ring_prefix" else r.past + T
    ops = {}
    if design == "zero":
        ops["q"] = np.zeros((B, T, H, D), dtype=np.float16)
        ops["q_lo"] = np.zeros((B, T, H, D), dtype=np.float16) if hp else None
        kvec = np.zeros((Hkv, D), dtype=np.float16)
    else:
        ops["q"] = _f16(rng.standard_normal((B, T, H, D)))
        ops["q_lo"] = _f16(2.0 ** -12 * rng.standard_normal((B, T, H, D))) if hp else None
        kvec = _f16(rng.standard_normal((Hkv, D)))
    if design == "zero":      # K is irrelevant to the scores: Gaussian, so that a wrong row would at least be a different one
        ops["k"] = _f16(rng.standard_normal((B, Hkv, S, D)))
    else:
        ops["k"] = np.broadcast_to(kvec[None, :, None, :], (B, Hkv, S, D)).copy()
    lo0, lo1 = _lo_rows(r)
    has_lo = lo1 > lo0
    ops["k_lo"] = np.zeros((B, Hkv, S, D), dtype=np.float16) if has_lo else None
    ops["v_lo"] = np.zeros((B, Hkv, S, D), dtype=np.float16) if has_lo else None
    if r.kind == "ring_prefix":
        ops["v"] = np.stack([census_v(Hkv, T, D, b, j0=r.past[b]) for b in range(B)])
        ops["trunk_k"] = (_f16(rng.standard_normal((Hkv, N_TRUNK, D))) if design == "zero"
                          else np.broadcast_to(kvec[:, None, :], (Hkv, N_TRUNK, D)).copy())
        ops["trunk_v"] = census_v(Hkv, N_TRUNK, D, 0)
        ops["trunk_k_lo"] = np.zeros((Hkv, N_TRUNK, D), dtype=np.float16)
        ops["trunk_v_lo"] = np.zeros((Hkv, N_TRUNK, D), dtype=np.float16)
    else:
        ops["v"] = np.stack([census_v(Hkv, S, D, b) for b in range(B)])
    return ops


def effective(r, ops):
    """(q, k, v, prefix | None) in float64, hi + lo planes: what ``attention64`` takes."""
    q = ops["q"].astype(np.float64) + (ops["q_lo"].astype(np.float64) if ops["q_lo"] is not None else 0.0)
    k, v = ops["k"].astype(np.float64), ops["v"].astype(np.float64)
    if ops["k_lo"] is not None:
        k, v = k + ops["k_lo"].astype(np.float64), v + ops["v_lo"].astype(np.float64)
    prefix = None
    if r.kind == "ring_prefix":
        prefix = (ops["trunk_k"].astype(np.float64) + ops["trunk_k_lo"].astype(np.float64),
                  ops["trunk_v"].astype(np.float64) + ops["trunk_v_lo"].astype(np.float64))
    return q, k, v, prefix


def reference(r, ops):
    q, k, v, prefix = effective(r, ops)
    return attention64(q, k, v, pasts(r), prefix)


def _v_seq(r, ops, b):
    """The one-hot V rows batch row b can see, in key order: [Hkv, past_b + T, D]."""
    past, T = pasts(r)[b], r.q_len
    if r.kind == "ring_prefix":
        return np.concatenate([ops["trunk_v"][:, :past], ops["v"][b][:, :T]], axis=1)
    return ops["v"][b][:, :past + T]


def census_counts(r, ops):
    """(count int64 [B, T, Hkv, D], n int64 [B, T]): count[b, i, h, c] = visible keys of row i whose one-hot V row of kv head h
    sits in column c; n[b, i] = past_b + i + 1 visible keys.  Integer arithmetic on the V planes themselves."""
    B, T = r.B, r.q_len
    count = np.empty((B, T, r.Hkv, r.D), dtype=np.int64)
    n = np.empty((B, T), dtype=np.int64)
    for b, past in enumerate(pasts(r)):
        seq = _v_seq(r, ops, b)
        assert np.isin(seq, (0.0, 1.0)).all() and (seq.sum(axis=-1) == 1).all()
        cum = np.cumsum(seq.astype(np.int64), axis=1)                  # [Hkv, S, D]
        count[b] = cum[:, past:past + T].transpose(1, 0, 2)
        n[b] = past + np.arange(T) + 1
    return count, n


def census_keys(r, ops, b, hkv, col, n_vis):
    """The keys of batch row b (numbered along its visible sequence) whose V row of kv head hkv is one-hot at ``col``:
    (those a row with n_vis visible keys sees, those it does not).  A count that is one too high names a key of the second
    list, one too low a key of the first."""
    js = np.flatnonzero(_v_seq(r, ops, b)[hkv, :, col] == 1.0)
    return js[js < n_vis].tolist(), js[js >= n_vis].tolist()


# ---------------------------------------------------------------------------------------------------
# score profiles
# ---------------------------------------------------------------------------------------------------

def unit(D):
    """log2 units of score per unit of k[j, 0] for a row with q[..., 0] = PROFILE_A."""
    return PROFILE_A * LOG2E / np.sqrt(D)


def stair_boundaries(S):
    """Odd multiples of 64 below S, the third one moved to key 37 of its tile (module docstring)."""
    bs = list(range(TK, S, 2 * TK))
    if len(bs) >= 3:
        bs[2] = bs[2] - TK + 37          # 320 -> 293
    return bs


def mid_tile_key(past):
    """The staged key at offset 37 of a 64-key tile (counted from key 0) among the last 64 staged keys."""
    j = (past - 1) - ((past - 1 - 37) % TK)
    assert past - TK <= j < past and j % TK == 37
    return j


def spike_rows(T):
    """row_spike: one row in the first 16-row group, one in a group a wave owns second (group 9 of the wide kernel's wave 1 when
    there are that many rows, else group 1: the second half of the 32-row kernel's wave 0), one in the last group."""
    return (3, 149 if T > 160 else 21, T - 1)


def profile_levels(name, past, T):
    """(level float64 [S] in log2 units along the key axis, rows that take part (None = all), the keys the profile is about)."""
    S = past + T
    lv = np.zeros(S)
    rows, marks = None, []
    if name == "late_spike":
        marks = [mid_tile_key(past)]
        lv[marks[0]] = SPIKE
    elif name == "early_spike":
        marks = [0]
        lv[0] = SPIKE
    elif name == "own_spike":
        marks = [past + min(37, T // 2)]
        lv[marks[0]] = SPIKE
    elif name == "row_spike":
        marks = [mid_tile_key(past)]
        lv[marks[0]] = ROW_SPIKE
        rows = spike_rows(T)
    elif name in ("stairs_up", "stairs_down"):
        marks = stair_boundaries(S)
        for b in marks:
            lv[b:] += STAIR if name == "stairs_up" else -STAIR
        if name == "stairs_down":
            lv -= lv.min()                 # (start high, end at 0: the same span of k[j, 0] as stairs_up)
    elif name == "threshold":
        # per 64-key tile (from key 0): 0, 7.5, 0, 8.5, 0, 7.5, ... -- the second tile of a two-tile slice rises by 7.5 (deferred,
        # P up to 2^7.5) or by 8.5 (moved); a walk over all tiles defers at tile 1 and moves at tile 3
        t = np.arange(S) // TK
        lv = np.where(t % 4 == 1, 7.5, np.where(t % 4 == 3, 8.5, 0.0))
        marks = list(range(TK, S, TK))
    else:
        raise ValueError(name)
    return lv, rows, marks


def profile_operands(name, r, seed=0):
    """fp16 Q (+ lo plane on split-precision routes), K, V (+ residual planes by the route's lo_mode) for one profile on route r."""
    assert r.kind != "ring_prefix" and r.B == 1
    rng = np.random.default_rng([seed, ROUTES.index(r), PROFILES.index(name)])
    B, T, H, Hkv, D, past = r.B, r.q_len, r.H, r.Hkv, r.D, r.past
    S = past + T
    hp = split_precision(r)
    lv, rows, _ = profile_levels(name, past, T)

    def g(shape, scale):
        a = scale * rng.standard_normal(shape)
        a[..., 0] = 0.0
        return _f16(a)

    ops = {"q": g((B, T, H, D), Q_BG.get(name, 0.5)), "q_lo": g((B, T, H, D), 2.0 ** -12) if hp else None,
           "k": g((B, Hkv, S, D), 0.5), "v": _f16(0.5 * rng.standard_normal((B, Hkv, S, D)))}
    if rows is None:
        ops["q"][..., 0] = PROFILE_A
    else:
        ops["q"][:, list(rows), :, 0] = PROFILE_A
    ops["k"][..., 0] = _f16(lv / unit(D))[None, None, :]
    lo0, lo1 = _lo_rows(r)
    ops["k_lo"] = ops["v_lo"] = None
    if lo1 > lo0:
        ops["k_lo"], ops["v_lo"] = np.zeros((B, Hkv, S, D), dtype=np.float16), np.zeros((B, Hkv, S, D), dtype=np.float16)
        ops["k_lo"][:, :, lo0:lo1] = g((B, Hkv, lo1 - lo0, D), 2.0 ** -12)
        ops["v_lo"][:, :, lo0:lo1] = _f16(2.0 ** -12 * rng.standard_normal((B, Hkv, lo1 - lo0, D)))
    return ops


def scores_log2(r, ops, b=0):
    """float64 [H, T, S]: q . k / sqrt(D) * log2 e of the operands themselves (hi + lo), masked keys at -inf."""
    q, k, _, _ = effective(r, ops)
    T, past = r.q_len, pasts(r)[b]
    kk = np.repeat(k[b][:, :past + T], r.H // r.Hkv, axis=0)
    s = np.einsum("thd,hsd->hts", q[b], kk) / np.sqrt(r.D) * LOG2E
    vis = np.arange(past + T)[None, :] <= (past + np.arange(T))[:, None]
    return np.where(vis[None], s, -np.inf)


def tile_maxima(s, first=0):
    """Per-row maxima over 64-key tiles counted from key ``first`` (a shorter tile [0, first) in front when first > 0):
    [..., ntiles]; a tile without a visible key is -inf."""
    S = s.shape[-1]
    edges = ([0] if first else []) + list(range(first, S, TK)) + [S]
    return np.stack([s[..., a:b].max(axis=-1) for a, b in zip(edges[:-1], edges[1:])], axis=-1)


def deferred_rises(tm):
    """The rule of pc_attn_wide.hip soft_core restated: ``moved = (mx - m_run) > kDeferLog2``; the running max moves only then.
    Returns the rises [..., ntiles - 1] of every tile after the first over the running max the kernel HOLDS at that tile
    (tiles with no visible key: -inf)."""
    held = tm[..., 0].copy()
    out = []
    for t in range(1, tm.shape[-1]):
        rise = tm[..., t] - held
        out.append(rise)
        held = np.where(rise > DEFER_LOG2, tm[..., t], held)
    return np.stack(out, axis=-1)


def online_rises(tm):
    """Rises of every tile after the first over the running max of an ordinary online softmax (moved = m_new > m_run)."""
    run = np.maximum.accumulate(tm, axis=-1)
    return tm[..., 1:] - run[..., :-1]


def fp16_p_loss(r, ops):
    """max |attention with P rounded to fp16 (relative to the row maximum, as the plain kernels form it) - attention64|: what
    the reference alone loses to fp16 P on these operands."""
    q, k, v, _ = effective(r, ops)
    s = scores_log2(r, ops)
    p = np.exp2(s - s.max(axis=-1, keepdims=True))
    p16 = p.astype(np.float16).astype(np.float64)
    vv = np.repeat(v[0][:, :s.shape[-1]], r.H // r.Hkv, axis=0)
    o16 = np.einsum("hts,hsd->thd", p16, vv) / p.sum(axis=-1).T[..., None]
    o = np.einsum("hts,hsd->thd", p, vv) / p.sum(axis=-1).T[..., None]
    return float(np.abs(o16 - o).max())
