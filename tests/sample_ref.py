"""numpy restatement of the device sampler's draw (csrc/pc_sample.hip, pc_sample_advance).  Test infrastructure only.

The chain itself is the oracle's (``oracle.sampling_oracle.process_logits``: the reference's generation_engine.py:32-42); this
module adds what the kernel does after it: Philox4x32-10 keyed by the 64-bit seed with counter (i >> 2, step, 0, 0), the
uniform u_i = ((word[i & 3] >> 8) + 0.5) * 2^-24, the Gumbel-max draw argmax_i (x_i - log(-log u_i)) over the kept tokens, and
the greedy rule (temperature < 1e-5 or top_p < 1e-8: argmax of the processed row, the lowest index among equal maxima)."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from oracle.sampling_oracle import is_greedy, process_logits

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter: np.ndarray, key: Tuple[int, int]) -> np.ndarray:
    """Philox4x32-10 of counters [N, 4] (uint32) under key (k0, k1) -> [N, 4] uint32."""
    c = [np.asarray(counter, dtype=np.uint64)[:, j].copy() for j in range(4)]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(_W0)) & _MASK
        k1 = (k1 + np.uint64(_W1)) & _MASK
    return np.stack(c, axis=1).astype(np.uint32)


def uniforms(V: int, seed: int, step: int) -> np.ndarray:
    """u_i in (0, 1) for tokens 0..V-1 at one (seed, step), float64 (exact)."""
    g = np.arange((V + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((g.size, 4), dtype=np.uint64)
    ctr[:, 0] = g
    ctr[:, 1] = step & 0xFFFFFFFF
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)[:V]
    return ((words >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def scores(processed: np.ndarray, seed: int, step: int, greedy: bool) -> np.ndarray:
    """Per-token draw scores (float64): -inf for filtered tokens; x for greedy, x - log(-log u) otherwise."""
    x = np.asarray(processed, dtype=np.float32).astype(np.float64)
    x = np.where(np.isnan(x), -np.inf, x)
    if greedy:
        return x
    u = uniforms(x.size, seed, step)
    return np.where(np.isfinite(x) | (x > 0), x - np.log(-np.log(u)), -np.inf)


def draw(logits: np.ndarray, history: Optional[Sequence[int]], temperature: float, repetition_penalty: float, top_p: float,
         top_k: int, seed: int, step: int) -> Tuple[int, float, np.ndarray]:
    """-> (token, margin between the best and second-best score, processed row).  margin = inf when one token is kept."""
    x = np.asarray(logits, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(-np.inf), x)
    proc = process_logits(x, history if history is not None else [], temperature, repetition_penalty, top_p, top_k)
    s = scores(proc, seed, step, is_greedy(temperature, top_p))
    if not np.any(s > -np.inf):
        return 0, np.inf, proc
    tok = int(np.argmax(s))                       # the lowest index among equal maxima
    rest = np.delete(s, tok)
    second = rest.max() if rest.size else -np.inf
    return tok, float(s[tok] - second), proc
