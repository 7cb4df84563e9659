"""numpy restatement of the sampled prompt-lookup verify step (csrc/pc_sample.hip, pc_lookup_verify_sample) and a host model of
``SampleLookupLoop``.  Test infrastructure only.

The draw of one row is ``tests/sample_ref.draw`` (the oracle's chain + Philox / Gumbel-max); this module adds the rule around it
(include/promptcache_hip.h): row i <= ndraft is drawn at Philox step ``draws + i`` under the history ``bits + ids[1..i]``, the
longest prefix of draws that equal their drafts is accepted, one more token is emitted, and the state advances by that many."""
from __future__ import annotations

from functools import lru_cache
from typing import Callable, List, Sequence, Tuple

import numpy as np

from tests import lookup_ref as lr
from tests import sample_ref as sr


def history_bits(ids, V: int) -> np.ndarray:
    """uint32 [ceil(V / 32)] with the bit of every id in ``ids`` set (ids outside the vocabulary ignored)."""
    bits = np.zeros((V + 31) // 32, dtype=np.uint32)
    for t in ids:
        t = int(t)
        if 0 <= t < V:
            bits[t >> 5] |= np.uint32(1 << (t & 31))
    return bits


def bits_ids(bits: np.ndarray, V: int) -> List[int]:
    b = np.unpackbits(np.asarray(bits, dtype=np.uint32).view(np.uint8), bitorder="little")[:V]
    return [int(i) for i in np.flatnonzero(b)]


@lru_cache(maxsize=1 << 16)
def _draw(row: bytes, history: Tuple[int, ...], params, seed: int, step: int):
    """sample_ref.draw, remembered: the rows a speculative step accepts are the very draws of the one-token generation (the set
    of history ids is what the penalty sees, so it is the key)."""
    T, rp, top_p, top_k = params
    return sr.draw(np.frombuffer(row, dtype=np.float32), list(history), T, rp, top_p, top_k, seed, step)


def draw(logits_row, history, params, seed: int, step: int):
    """-> (token, score margin, processed row) of one row under the history ids ``history`` (sample_ref.draw)."""
    row = np.ascontiguousarray(logits_row, dtype=np.float32)
    if row.size > 4096:                                # (a real vocabulary: nothing repeats, and the key would be the row)
        T, rp, top_p, top_k = params
        return sr.draw(row, list(history), T, rp, top_p, top_k, seed, step)
    return _draw(row.tobytes(), tuple(sorted({int(t) for t in history})), tuple(params), int(seed), int(step))


def verify_sample(logits, st, ring_cap: int, params: Tuple[float, float, float, int], seed: int):
    """pc_lookup_verify_sample on ``logits [rows][vocab]`` and the state ``st`` -- ``lookup_ref.verify``'s dict (hist, hist_len[1], ids,
    pos, past, ndraft[1], budget[1], ring [ring_cap][rows+1], ctr[1]) plus ``bits`` (uint32 history bitmap) and ``draws[1]`` --
    under ``params = (temperature, repetition_penalty, top_p, top_k)`` -> ``(new state, info)``: every state word (deep copy;
    the scratch words are not modelled), and ``info`` = dict(tokens: the draw of every row i <= ndraft, margins: its score
    margin (best minus second best, float64), processed: its processed row, acc, emit)."""
    st = {k_: np.array(v, copy=True) for k_, v in st.items()}
    logits = np.asarray(logits, dtype=np.float32)
    rows, V = logits.shape
    nd = min(max(int(st["ndraft"][0]), 0), rows - 1)
    d = int(st["draws"][0])
    base = bits_ids(st["bits"], V)
    t, margins, processed = [], [], []
    for i in range(nd + 1):
        history = base + [int(x) for x in st["ids"][1:1 + i] if 0 <= int(x) < V]
        tok, margin, proc = draw(logits[i], history, params, seed, d + i)
        t.append(tok)
        margins.append(margin)
        processed.append(proc)
    acc = 0
    while acc < nd and t[acc] == int(st["ids"][1 + acc]):
        acc += 1
    L = int(st["hist_len"][0])
    emit = min(acc + 1, int(st["budget"][0]), max(0, st["hist"].size - L) if L >= 0 else 0)
    emit = max(emit, 0)
    c = int(st["ctr"][0])
    rec = st["ring"].reshape(ring_cap, rows + 1)[c % ring_cap]
    rec[0] = emit
    rec[1:1 + emit] = t[:emit]
    st["ctr"][0] = c + 1
    if emit > 0:
        st["hist"][L:L + emit] = t[:emit]
        st["hist_len"][0] = L + emit
        st["ids"][0] = t[emit - 1]
        st["pos"][0] += emit
        st["past"][0] += emit
        st["budget"][0] -= emit
        st["draws"][0] = d + emit
        st["bits"] |= history_bits(t[:emit], V)
    return st, dict(tokens=t, margins=margins, processed=processed, acc=acc, emit=emit)


def sequential(model: Callable[[Sequence[int]], np.ndarray], prefix: Sequence[int], first_token: int, n: int, params, seed: int,
               history_ids: Sequence[int]) -> List[int]:
    """The one-token sampled loop (SampleLoop) on the host model ``model`` (prefix of tokens -> logits of the next): ``n`` tokens
    behind ``first_token``, token number j drawn at Philox step j under the history ``history_ids`` + the tokens drawn so far
    (``history_ids`` holds ``first_token``, as in GenerationEngine)."""
    seq, hist, out = [int(t) for t in prefix] + [int(first_token)], [int(t) for t in history_ids], []
    for j in range(1, n + 1):
        tok, _, _ = draw(model(seq), hist, params, seed, j)
        out.append(tok)
        seq.append(tok)
        hist.append(tok)
    return out


def simulate(model: Callable[[Sequence[int]], np.ndarray], prefix: Sequence[int], first_token: int, corpus: Sequence[int], k: int,
             max_new: int, params, seed: int, history_ids: Sequence[int], nmax: int = 3, surplus: int = 0, ring_cap: int = 4):
    """SampleLookupLoop on the host model: draft (lookup_ref.draft_state) -> the k + 1 rows of logits ``model`` gives for the fed
    token and the drafts -> verify_sample, until ``max_new`` tokens are out, then ``surplus`` more steps (budget 0).
    -> (per-step token lists, final state, per-step states)."""
    V = int(np.asarray(model(list(prefix) + [int(first_token)])).size)
    h0 = [int(t) for t in corpus] + [int(first_token)]
    st = dict(hist=np.zeros(len(h0) + max_new, dtype=np.int32), hist_len=np.array([len(h0)], dtype=np.int32),
              ids=np.full(k + 1, int(first_token), dtype=np.int64), pos=np.full(k + 1, len(prefix), dtype=np.int32),
              past=np.array([len(prefix), 0], dtype=np.int32), ndraft=np.zeros(1, dtype=np.int32),
              budget=np.array([max_new], dtype=np.int32), ring=np.zeros((ring_cap, k + 2), dtype=np.int32),
              ctr=np.zeros(1, dtype=np.int32), bits=history_bits(history_ids, V), draws=np.ones(1, dtype=np.int32))
    st["hist"][:len(h0)] = h0
    seq = [int(t) for t in prefix]                     # the tokens in front of the fed one
    steps, states, got, extra = [], [], 0, 0
    while got < max_new or extra < surplus:
        if got >= max_new:
            extra += 1
        ids, pos, m = lr.draft_state(st["hist"], st["hist_len"][0], st["ids"], st["pos"], k, nmax)
        st["ids"], st["pos"], st["ndraft"][0] = ids, pos, m
        rows = [model(seq + [int(t) for t in ids[:i + 1]]) for i in range(k + 1)]
        c = int(st["ctr"][0])
        st, info = verify_sample(np.stack(rows), st, ring_cap, params, seed)
        rec = st["ring"].reshape(ring_cap, k + 2)[c % ring_cap]
        toks = [int(t) for t in rec[1:1 + int(rec[0])]]
        assert got >= max_new or toks, "a step with budget left emits at least one token"
        seq += [int(ids[0])] + toks[:-1] if toks else []
        steps.append(toks)
        states.append(st)
        got += len(toks)
    return steps, st, states

