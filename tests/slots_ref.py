"""Numpy reference of the batched decode over slots (csrc/pc_slots.hip, pc_sample_advance_slots): ragged one-row attention per
slot in fp32, written from the definition of ``oracle.llama_oracle.attention_core`` (softmax(q k^T / sqrt(D)) v, query heads
broadcast over their kv head; no mask for a single query row), and the advance rule on top of ``tests/sample_ref.py``."""
from typing import List, Optional, Sequence

import numpy as np

from tests import sample_ref as sr

F32 = np.float32


def attend_slot(q: np.ndarray, k: np.ndarray, v: np.ndarray) -> np.ndarray:
    """One slot.  q [H][D] (RoPE applied), k / v [Hkv][n][D]: the slot's n keys, its own row included.  -> [H][D] fp32."""
    H, D = q.shape
    rep = H // k.shape[0]
    out = np.empty((H, D), dtype=F32)
    for h in range(H):
        kk, vv = k[h // rep].astype(F32), v[h // rep].astype(F32)
        s = (kk @ q[h].astype(F32)) / F32(np.sqrt(D))
        e = np.exp((s - s.max()).astype(F32))
        out[h] = (e / e.sum(dtype=F32)).astype(F32) @ vv
    return out


def attend_slots(q: np.ndarray, keys: Sequence[Optional[np.ndarray]], values: Sequence[Optional[np.ndarray]]) -> List[Optional[np.ndarray]]:
    """Ragged batch: ``keys[b]`` None = idle slot (no output)."""
    return [None if k is None else attend_slot(q[b], k, v) for b, (k, v) in enumerate(zip(keys, values))]


def advance_slot(state: dict, logits: np.ndarray, history: set, T: float, rp: float, top_p: float, top_k: int, stop_ids: Sequence[int]):
    """pc_sample_advance_slots for one slot.  ``state``: ids, pos, len, cap, live, budget, ctr, seed (ints), mutated in place;
    ``history``: the set of ids the penalty sees, the drawn token is added.  -> (token | None, margin, processed row | None)."""
    if not state["live"]:
        return None, np.inf, None
    if state["len"] >= state["cap"]:
        state["live"] = 0
        return None, np.inf, None
    tok, margin, proc = sr.draw(logits, sorted(history), T, rp, top_p, top_k, state["seed"], state["ctr"])
    state["ids"] = tok
    state["pos"] += 1
    state["len"] += 1
    state["ctr"] += 1
    state["budget"] -= 1
    history.add(tok)
    if tok in stop_ids or state["budget"] <= 0 or state["len"] + 1 >= state["cap"]:
        state["live"] = 0
    return tok, margin, proc
