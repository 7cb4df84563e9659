"""numpy restatement of the token-control rule (csrc/pc_logit_ctl.hip, pc_logit_adjust).  Test infrastructure only.

Per row, in this order -- bit level, every step in float32:
  1. a[j] = x[j]
  2. for each table entry (ids distinct; an id outside [0, V) is skipped), a[id] = x[id] + bias: one fp32 add, so x + (-inf) = -inf
  3. with an allow-list, every j not in it: a[j] = -inf
  4. while the row's token number g is below min_new_tokens, a[stop] = -inf for the stop ids
A NaN in x stays NaN unless step 3 or 4 writes over it."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

BIAS_MAX = 64
STOP_MAX = 8
NINF = np.float32(-np.inf)


def adjust(x: np.ndarray, bias: Sequence = (), allowed: Optional[Sequence[int]] = None, stop_ids: Sequence[int] = (),
           hold_stops: bool = False) -> np.ndarray:
    """The adjusted copy of one fp32 row.  ``bias``: ``[(id, value), ...]``; ``hold_stops``: the row's token number is below
    ``min_new_tokens``."""
    x = np.asarray(x, dtype=np.float32)
    V = x.size
    a = x.copy()
    with np.errstate(invalid="ignore"):
        for i, v in bias:
            if 0 <= int(i) < V:
                a[int(i)] = x[int(i)] + np.float32(v)
    if allowed is not None:
        keep = np.zeros(V, dtype=bool)
        ids = np.asarray([i for i in allowed if 0 <= int(i) < V], dtype=np.int64)
        keep[ids] = True
        a[~keep] = NINF
    if hold_stops:
        for i in stop_ids:
            if 0 <= int(i) < V:
                a[int(i)] = NINF
    return a


def adjust_controls(x: np.ndarray, controls, generated: int) -> np.ndarray:
    """``adjust`` under a ``modes.TokenControls`` (None: the row) for generated token number ``generated`` (0: the prefill's)."""
    if controls is None:
        return np.asarray(x, dtype=np.float32).copy()
    return adjust(x, controls.bias, controls.allowed, controls.stop_ids, generated < controls.min_new_tokens)


def adjust_slots(x: np.ndarray, rows_per_slot: int, blocks: Sequence[dict], lens: Optional[Sequence[int]] = None) -> np.ndarray:
    """``pc_logit_adjust`` over ``[S * rows_per_slot][V]`` rows: ``blocks[b]`` = ``dict(bias=, allowed=, stop_ids=, stop_free_len=,
    n_bias=)`` as the device block holds them (``n_bias`` clamped into 0..64 and defaulting to ``len(bias)``); row ``(b, i)`` holds
    the stop ids back while ``lens[b] + i < stop_free_len`` (``lens`` None reads as 0)."""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty_like(x)
    for r in range(x.shape[0]):
        b, i = divmod(r, rows_per_slot)
        blk = blocks[b]
        bias = list(blk.get("bias", ()))
        nb = min(max(int(blk.get("n_bias", len(bias))), 0), BIAS_MAX)
        hold = (0 if lens is None else int(lens[b])) + i < int(blk.get("stop_free_len", 0))
        out[r] = adjust(x[r], bias[:nb], blk.get("allowed"), blk.get("stop_ids", ()), hold)
    return out


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Bitwise equality of two fp32 arrays, NaN positions compared as positions."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(gn, wn)) and \
        bool(np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


def allowed_bits(allowed: Sequence[int], V: int) -> np.ndarray:
    """uint32 ``[ceil(V / 32)]`` with the bit of every allowed id inside the vocabulary set."""
    bits = np.zeros((V + 31) // 32, dtype=np.uint32)
    for i in allowed:
        if 0 <= int(i) < V:
            bits[int(i) >> 5] |= np.uint32(1) << np.uint32(int(i) & 31)
    return bits
