"""numpy restatement of the prompt-lookup step's two device kernels (csrc/pc_lookup.hip) and a host model of the loop.

The rules are fully determined (include/promptcache_hip.h), so these are exact references: the GPU tests compare every word."""
import numpy as np


def draft(h, L, k, nmax=3):
    """pc_lookup_draft on the history ``h[0:L]`` -> ``(drafts, m)``: ``drafts`` are the k ids of rows 1..k (the m real drafts, then
    pads that repeat the fed token ``h[L-1]``), ``m`` = ndraft.  The suffix lengths n = min(nmax, L-1) .. 1 are tried longest
    first; of the positions j in [0, L-n-1] with h[j:j+n] == h[L-n:L] the largest is taken."""
    h = [int(t) for t in h[:L]]
    fed = h[L - 1] if L >= 1 else 0
    for n in range(min(nmax, L - 1), 0, -1):
        suf = h[L - n:L]
        for j in range(L - n - 1, -1, -1):
            if h[j:j + n] == suf:
                m = min(k, L - (j + n))
                return h[j + n:j + n + m] + [fed] * (k - m), m
    return [fed] * k, 0


def draft_state(hist, hist_len, ids, pos, k, nmax=3):
    """The kernel's effect on its state words: -> (ids, pos, ndraft) after the launch (copies; words beyond k + 1 untouched)."""
    ids, pos = np.array(ids, dtype=np.int64), np.array(pos, dtype=np.int32)
    L = int(hist_len)
    d, m = draft(hist, L, k, nmax)
    for i in range(k):
        ids[1 + i] = d[i] if i < m else ids[0]
        pos[1 + i] = pos[0] + 1 + i
    return ids, pos, m


def argmax_rows(logits):
    """Per-row argmax, lowest index among equal maxima; a row without any value above -inf gives 0."""
    out = []
    for row in np.asarray(logits, dtype=np.float32):
        best, bi = -np.inf, 0
        with np.errstate(invalid="ignore"):
            ok = row > -np.inf                       # (NaN compares false, as on the device)
        if ok.any():
            mx = row[ok].max()
            bi = int(np.flatnonzero(ok & (row == mx))[0])
        out.append(bi)
    return out


def verify(logits, st, ring_cap):
    """pc_lookup_verify on ``logits [rows][vocab]`` and the state ``st`` (dict of numpy arrays: hist, hist_len[1], ids, pos, past,
    ndraft[1], budget[1], ring [ring_cap][rows+1], ctr[1]) -> the new state (deep copy)."""
    st = {k_: np.array(v, copy=True) for k_, v in st.items()}
    rows = len(logits)
    a = argmax_rows(logits)
    nd = min(max(int(st["ndraft"][0]), 0), rows - 1)
    acc = 0
    while acc < nd and a[acc] == int(st["ids"][1 + acc]):
        acc += 1
    emit = min(acc + 1, int(st["budget"][0]))
    c = int(st["ctr"][0])
    rec = st["ring"].reshape(ring_cap, rows + 1)[c % ring_cap]
    rec[0] = emit
    rec[1:1 + emit] = a[:emit]
    st["ctr"][0] = c + 1
    if emit > 0:
        L = int(st["hist_len"][0])
        st["hist"][L:L + emit] = a[:emit]
        st["hist_len"][0] = L + emit
        st["ids"][0] = a[emit - 1]
        st["pos"][0] += emit
        st["past"][0] += emit
        st["budget"][0] -= emit
    return st


def simulate(corpus, first_token, T, k, nmax=3):
    """Per-step emit counts of the loop when the model's greedy continuation of ``first_token`` is the known sequence ``T``
    (row i of a step answers T[p + i] as long as the drafts before it were right): history = corpus ++ [first_token], budget =
    len(T).  Runs until all of T is emitted."""
    h = [int(t) for t in corpus] + [int(first_token)]
    T = [int(t) for t in T]
    p, counts = 0, []
    while p < len(T):
        d, m = draft(h, len(h), k, nmax)
        acc = 0
        while acc < m and p + acc < len(T) and d[acc] == T[p + acc]:
            acc += 1
        emit = min(acc + 1, len(T) - p)
        h += T[p:p + emit]
        p += emit
        counts.append(emit)
    return counts
