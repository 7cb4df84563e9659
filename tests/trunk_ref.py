"""Numpy reference of the shared-trunk decode attention (csrc/pc_slots.hip, pc_attn_decode_slots_trunk): one query row over a
TRUNK of keys (read from the group leader's arena) and the slot's OWN keys, each part reduced to the partial record the kernels
leave -- unnormalised sum, maximum and denominator in the log2 domain -- and merged as the merge launch merges them, trunk first."""
from typing import Sequence, Tuple

import numpy as np

F32 = np.float32
LOG2E = F32(1.4426950408889634)
NEG_BIG = F32(-1.0e30)


def partial(q: np.ndarray, k: np.ndarray, v: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """q [H][D] fp32, k / v [Hkv][n][D] -> (num [H][D], m [H], den [H]): sum_j 2^(s_j - m) v_j, m = max_j s_j, sum_j 2^(s_j - m)
    with s = q.k / sqrt(D) * log2(e).  n = 0: (0, -1e30, 0), the record of a split without keys."""
    H, D = q.shape
    rep = H // k.shape[0]
    num, m, den = np.zeros((H, D), F32), np.full(H, NEG_BIG, F32), np.zeros(H, F32)
    if k.shape[1] == 0:
        return num, m, den
    scale = F32(1.0 / np.sqrt(D)) * LOG2E
    for h in range(H):
        kk, vv = k[h // rep].astype(F32), v[h // rep].astype(F32)
        s = (kk @ q[h].astype(F32)) * scale
        m[h] = s.max()
        e = np.exp2((s - m[h]).astype(F32)).astype(F32)
        den[h] = e.sum(dtype=F32)
        num[h] = e @ vv
    return num, m, den


def merge(parts: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]]) -> np.ndarray:
    """The merge launch: records in key order, weights 2^(m_i - max m), fp32."""
    ms = np.max(np.stack([p[1] for p in parts]), axis=0)
    num = np.zeros_like(parts[0][0])
    den = np.zeros_like(parts[0][2])
    for pn, pm, pd in parts:
        w = np.exp2((pm - ms).astype(F32)).astype(F32)
        den = (den + w * pd).astype(F32)
        num = (num + w[:, None] * pn).astype(F32)
    return (num / den[:, None]).astype(F32)


def attend_trunk(q: np.ndarray, k_trunk: np.ndarray, v_trunk: np.ndarray, k_own: np.ndarray, v_own: np.ndarray) -> np.ndarray:
    """One slot of a group: trunk keys [Hkv][T][D] (the LEADER's rows), own keys [Hkv][n - T][D].  -> [H][D] fp32."""
    return merge([partial(q, k_trunk, v_trunk), partial(q, k_own, v_own)])


def attend_f64(q: np.ndarray, k: np.ndarray, v: np.ndarray) -> np.ndarray:
    """softmax(q k^T / sqrt(D)) v in float64 over all keys."""
    H, D = q.shape
    rep = H // k.shape[0]
    out = np.empty((H, D), np.float64)
    for h in range(H):
        s = k[h // rep].astype(np.float64) @ q[h].astype(np.float64) / np.sqrt(D)
        e = np.exp(s - s.max())
        out[h] = (e / e.sum()) @ v[h // rep].astype(np.float64)
    return out
