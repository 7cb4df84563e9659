"""numpy restatement of the batched prompt-lookup step (csrc/pc_lookup_slots.hip, the *_slots entries of csrc/pc_lookup.hip) and a
host model of the loop.  Built on tests/lookup_ref.py; imports nothing of the product.

A slot RUNS when it is live and ``0 <= len`` and ``len + k + 1 <= cap``.  The draft / rope / attention launches leave a slot that
does not run alone; the verify launch gives it an empty ring record (its counter keeps pace with the replays) and switches it off."""
import numpy as np

from tests import lookup_ref as lr


def runs(st, b, k):
    return bool(st["live"][b] != 0 and 0 <= st["len"][b] and st["len"][b] + k + 1 <= st["cap"][b])


def _copy(st):
    return {k_: np.array(v, copy=True) for k_, v in st.items()}


def draft_slots(st, k, nmax=3):
    """pc_lookup_draft_slots on the state ``st`` (dict of numpy arrays: hist [S][hist_cap], hist_len [S], ids [S][k+1], pos [S][k+1],
    ndraft [S], cap / len / live [S], ...) -> the new state (deep copy)."""
    st = _copy(st)
    for b in range(len(st["live"])):
        if not runs(st, b, k):
            continue
        st["ids"][b], st["pos"][b], st["ndraft"][b] = lr.draft_state(st["hist"][b], st["hist_len"][b], st["ids"][b], st["pos"][b], k, nmax)
    return st


def verify_slots(logits, st, k, ring_cap):
    """pc_lookup_verify_slots on ``logits [S * (k + 1)][vocab]`` and ``st`` (draft_slots' arrays plus budget [S], stop_ids [S][8],
    ring [S][ring_cap][k + 2], ctr [S]) -> (new state, row argmax)."""
    st = _copy(st)
    S, rows = len(st["live"]), k + 1
    a_all = lr.argmax_rows(logits)
    ring = st["ring"].reshape(S, ring_cap, rows + 1)
    for b in range(S):
        c = int(st["ctr"][b])
        rec = ring[b, c % ring_cap]
        st["ctr"][b] = c + 1
        if not runs(st, b, k):
            rec[0] = 0
            st["live"][b] = 0
            continue
        a = a_all[b * rows:(b + 1) * rows]
        nd = min(max(int(st["ndraft"][b]), 0), k)
        acc = 0
        while acc < nd and a[acc] == int(st["ids"][b][1 + acc]):
            acc += 1
        bud = int(st["budget"][b])
        L = int(st["hist_len"][b])
        emit = max(min(acc + 1, bud, st["hist"].shape[1] - L), 0)
        stops = set(int(t) for t in st["stop_ids"][b])
        stopped = False
        for i in range(emit):
            if a[i] in stops:
                emit, stopped = i + 1, True
                break
        rec[0] = emit
        rec[1:1 + emit] = a[:emit]
        if emit > 0:
            st["hist"][b][L:L + emit] = a[:emit]
            st["hist_len"][b] = L + emit
            st["ids"][b][0] = a[emit - 1]
            st["pos"][b][0] += emit
            st["len"][b] += emit
            st["budget"][b] = bud - emit
        if stopped or bud - emit <= 0 or st["len"][b] + k + 1 > st["cap"][b]:
            st["live"][b] = 0
    return st, np.array(a_all, dtype=np.int32)


def verify_attend(q, K, V, length, k):
    """The causal k + 1-row attention of one slot in float64: q [k+1][H][D], K / V [Hkv][>= length + k + 1][D] (rows length..length+k
    are this step's own) -> [k+1][H][D]; row i sees keys [0, length + i]."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    R, H, D = q.shape
    G = H // K.shape[0]
    out = np.zeros((R, H, D))
    for i in range(R):
        nk = length + i + 1
        for h in range(H):
            s = K[h // G, :nk] @ q[i, h] / np.sqrt(D)
            p = np.exp(s - s.max())
            out[i, h] = (p / p.sum()) @ V[h // G, :nk]
    return out


def simulate_slots(corpora, first_tokens, Ts, k, nmax=3, stop_ids=()):
    """Per-step emit counts per sequence when sequence j's greedy continuation of ``first_tokens[j]`` is the known ``Ts[j]`` (budget
    len(Ts[j])): -> list over steps of lists over sequences (0 once a sequence is over), until every sequence is over."""
    stops = set(int(t) for t in stop_ids)
    hs = [[int(t) for t in c] + [int(f)] for c, f in zip(corpora, first_tokens)]
    Ts = [[int(t) for t in T] for T in Ts]
    p, alive, steps = [0] * len(Ts), [len(T) > 0 for T in Ts], []
    while any(alive):
        row = []
        for j, T in enumerate(Ts):
            if not alive[j]:
                row.append(0)
                continue
            d, m = lr.draft(hs[j], len(hs[j]), k, nmax)
            acc = 0
            while acc < m and p[j] + acc < len(T) and d[acc] == T[p[j] + acc]:
                acc += 1
            emit = min(acc + 1, len(T) - p[j])
            for i in range(emit):
                if T[p[j] + i] in stops:
                    emit, alive[j] = i + 1, False
                    break
            hs[j] += T[p[j]:p[j] + emit]
            p[j] += emit
            if p[j] >= len(T):
                alive[j] = False
            row.append(emit)
        steps.append(row)
    return steps
