"""numpy restatement of the device sampler's draw (csrc/pc_sample.hip, pc_sample_advance).  Test infrastructure only.

The chain itself is the oracle's (``oracle.sampling_oracle.process_logits``: the reference's generation_engine.py:32-42); this
module adds what the kernel does after it: Philox4x32-10 keyed by the 64-bit seed with counter (i >> 2, step, 0, 0), the
uniform u_i = ((word[i & 3] >> 8) + 0.5) * 2^-24, the Gumbel-max draw argmax_i (x_i - log(-log u_i)) over the kept tokens, and
the greedy rule (temperature < 1e-5 or top_p < 1e-8: argmax of the processed row, the lowest index among equal maxima)."""
from __future__ import annotations

import os
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


# ---- tests/golden/sampling_chain_vocab.npz (oracle/gen_golden.py sampling_vocab_goldens) ----------------------------------
# A row is int16 codes x 2^exp2 (exact in fp32), with four sentinel codes; a case is one row, a parameter set, a history (bits
# over the vocabulary) and the reference's kept set (bits in rank_order of the row: a prefix, whatever the row, packs to nothing).
CODE_NINF, CODE_NAN, CODE_NEGZERO, CODE_PINF = -32768, -32767, -32766, 32767
VOCAB_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_chain_vocab.npz")


def decode_vocab_row(codes: np.ndarray, exp2: int) -> np.ndarray:
    x = codes.astype(np.float32) * np.float32(2.0 ** int(exp2))
    x[codes == CODE_NINF] = -np.inf
    x[codes == CODE_PINF] = np.inf
    x[codes == CODE_NAN] = np.nan
    x[codes == CODE_NEGZERO] = -0.0
    return x


def rank_order(x: np.ndarray) -> np.ndarray:
    """Token ids in top-p rank order: value descending, the higher index first among equal values (-0 == +0), NaN ahead of
    everything (torch's ascending sort puts it last)."""
    nan = np.isnan(x)
    v = np.where(nan, np.inf, x).astype(np.float64)
    return np.lexsort((-np.arange(x.size), -v, -nan.astype(np.int8)))


def vocab_cases(path: str = VOCAB_GOLD):
    """-> dicts: row, family, logits (fp32 [V]), history (int64 ids), T, rp, top_p, top_k, kept (bool [V], the reference's)."""
    z = np.load(path, allow_pickle=False)
    V = z["vocab"].astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(V)])
    rows = [decode_vocab_row(z["codes"][row_off[i]:row_off[i + 1]], z["exp2"][i]) for i in range(V.size)]
    orders = {}
    hb, kb = z["history_bits"], z["kept_bits"]
    off = 0
    for c, r in enumerate(z["case_row"]):
        v, x, nb = int(V[r]), rows[r], (int(V[r]) + 7) // 8
        hist = np.nonzero(np.unpackbits(hb[off:off + nb], count=v))[0]
        if r not in orders:
            orders[r] = rank_order(x)
        kept = np.zeros(v, dtype=bool)
        kept[orders[r]] = np.unpackbits(kb[off:off + nb], count=v).astype(bool)
        off += nb
        t, rp, tp, tk = z["params"][c]
        yield dict(row=int(r), family=str(z["family"][r]), logits=x, history=hist, T=float(t), rp=float(rp), top_p=float(tp),
                   top_k=int(tk), kept=kept)
    assert off == hb.size == kb.size


def tie_canonical(pre: np.ndarray, kept: np.ndarray) -> np.ndarray:
    """``kept`` with the kept count of every value moved to that value's highest indices (-0 == +0, NaN one value).  The
    reference's top-p sort is not stable, so which tokens of a tie run it keeps is unspecified; how many is not (equal values
    add equal mass).  The device and the oracle keep the highest indices: this is the reference's set in that reading."""
    v = np.where(np.isnan(pre), np.inf, pre).astype(np.float64) + 0.0
    order = np.lexsort((-np.arange(v.size), -v))                 # value descending, index descending
    sv = v[order]
    new = np.r_[True, sv[1:] != sv[:-1]]
    gid = np.cumsum(new) - 1
    starts = np.nonzero(new)[0]
    count = np.bincount(gid, weights=kept[order].astype(np.float64)).astype(np.int64)
    out = np.zeros_like(kept)
    out[order] = (np.arange(v.size) - starts[gid]) < count[gid]
    return out
