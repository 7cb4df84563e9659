"""numpy restatement of the per-slot sampled prompt-lookup verify step (csrc/pc_sample.hip, pc_lookup_verify_slots_each), a host
model of continuous admission into the lookup slot loop (``LookupSlotLoop(each=True)``), and the inputs of the GPU cases.  Test
infrastructure only; imports nothing of the product.

The rule per slot is ``tests/lookup_sample_ref.verify_sample`` -- row i <= ndraft drawn at Philox step ``draws + i`` under the
history ``bits + ids[1..i]``, the longest agreeing prefix plus one token -- with what ``tests/lookup_slots_ref.verify_slots`` adds
for slots: the EMPTY record and ``ctr += 1`` of a slot that does not run, the cut behind the first emitted stop id, ``len`` in the
place of ``past`` and the ``live`` rule."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import lookup_ref as lr
from tests import lookup_sample_ref as lsr
from tests import lookup_slots_ref as lsl

GREEDY = (0.0, 1.0, 1.0, -1)
SAMPLED = (0.7, 1.1, 0.9, 40)
WIDE = (1.0, 1.0, 0.95, -1)
GREEDY_RP = (0.0, 1.3, 1.0, -1)
MARGIN = 1e-4           # tests/test_gpu_sample.py: draws are compared where the reference's decision is no near-tie


def _copy(st):
    return {k_: np.array(v, copy=True) for k_, v in st.items()}


def verify_slots_each(logits, st, k: int, ring_cap: int, params: Sequence[Tuple], seeds: Sequence[int],
                      force: Optional[Dict[Tuple[int, int], int]] = None):
    """pc_lookup_verify_slots_each on ``logits [S * (k + 1)][vocab]`` and ``st`` -- ``lookup_slots_ref.verify_slots``' arrays plus
    ``bits`` uint32 [S][ceil(vocab / 32)] and ``draws`` [S] -- under ``params[b]`` = (temperature, repetition_penalty, top_p, top_k)
    and ``seeds[b]`` -> ``(new state, info)``: every state word (deep copy; the scratch words are not modelled) and ``info[b]`` =
    None for a slot that did not run, else dict(tokens, margins, acc, emit) of ``lookup_sample_ref.verify_sample`` (emit behind the
    stop cut).  ``force[(b, i)]``: take that token as the draw of row i of slot b (a test follows the device through a near-tie)."""
    st = _copy(st)
    logits = np.asarray(logits, dtype=np.float32)
    S, rows = len(st["live"]), k + 1
    ring = st["ring"].reshape(S, ring_cap, rows + 1)
    infos: List[Optional[dict]] = []
    for b in range(S):
        c = int(st["ctr"][b])
        if not lsl.runs(st, b, k):
            ring[b, c % ring_cap][0] = 0
            st["ctr"][b] = c + 1
            st["live"][b] = 0
            infos.append(None)
            continue
        bud = int(st["budget"][b])

        def one(budget):
            s1 = dict(hist=st["hist"][b], hist_len=st["hist_len"][b:b + 1], ids=st["ids"][b], pos=st["pos"][b],
                      past=np.array([st["len"][b], 0], dtype=np.int32), ndraft=st["ndraft"][b:b + 1],
                      budget=np.array([budget], dtype=np.int32), ring=np.zeros((1, rows + 1), dtype=np.int32),
                      ctr=np.zeros(1, dtype=np.int32), bits=st["bits"][b], draws=st["draws"][b:b + 1])
            if force:
                return _verify_forced(logits[b * rows:(b + 1) * rows], s1, params[b], seeds[b], {i: t for (bb, i), t in force.items() if bb == b})
            return lsr.verify_sample(logits[b * rows:(b + 1) * rows], s1, 1, params[b], seeds[b])
        new, info = one(bud)
        stops = set(int(t) for t in st["stop_ids"][b] if t >= 0)
        stopped = False
        for i in range(info["emit"]):
            if info["tokens"][i] in stops:                       # the stop id itself is emitted, nothing behind it
                stopped = True
                if i + 1 < info["emit"]:
                    new, info = one(i + 1)
                break
        emit = info["emit"]
        ring[b, c % ring_cap][:1 + emit] = new["ring"][0][:1 + emit]
        st["ctr"][b] = c + 1
        st["hist"][b], st["hist_len"][b], st["ids"][b], st["pos"][b] = new["hist"], new["hist_len"][0], new["ids"], new["pos"]
        st["len"][b] = new["past"][0]
        st["budget"][b] = bud - emit
        st["bits"][b], st["draws"][b] = new["bits"], new["draws"][0]
        if stopped or bud - emit <= 0 or st["len"][b] + k + 1 > st["cap"][b]:
            st["live"][b] = 0
        infos.append(info)
    return st, infos


def _verify_forced(logits, s1, params, seed, forced: Dict[int, int]):
    """``lookup_sample_ref.verify_sample`` with the draws of the rows in ``forced`` replaced: the accept rule is re-run on the forced
    tokens by handing verify_sample rows whose draw is the forced token whatever the parameters (one-hot rows, plain argmax)."""
    if not forced:
        return lsr.verify_sample(logits, s1, 1, params, seed)
    _, info = lsr.verify_sample(logits, s1, 1, params, seed)
    toks = [forced.get(i, t) for i, t in enumerate(info["tokens"])]
    onehot = np.full(logits.shape, -1.0, dtype=np.float32)
    for i, t in enumerate(toks):
        onehot[i, t] = 1.0
    new, inf2 = lsr.verify_sample(onehot, s1, 1, (0.0, 1.0, 1.0, 0), seed)
    inf2["margins"] = info["margins"]
    return new, inf2


# ---- admission: the history a sequence enters with --------------------------------------------------------------------------------
def fit_history(corpus: Sequence[int], token: int, max_new: int, hist_cap: int) -> List[int]:
    """The history of a sequence admitted with ``corpus`` and fed ``token``: ``corpus ++ [token]`` with the OLDEST corpus ids dropped
    until ``hist_len + max_new <= hist_cap``; ValueError when ``max_new + 1`` alone does not fit."""
    if max_new + 1 > hist_cap:
        raise ValueError("max_new + 1 exceeds the history capacity")
    keep = hist_cap - max_new - 1
    c = [int(t) for t in corpus]
    return (c[len(c) - keep:] if keep < len(c) else c) + [int(token)] if keep > 0 else [int(token)]


def new_state(S: int, k: int, V: int, hist_cap: int, ring_cap: int):
    hw = (V + 31) // 32
    z = lambda shape, dt=np.int32: np.zeros(shape, dtype=dt)
    return dict(hist=z((S, hist_cap)), hist_len=z(S), ids=z((S, k + 1), np.int64), pos=z((S, k + 1)), ndraft=z(S), cap=z(S), len=z(S),
                live=z(S), budget=z(S), stop_ids=np.full((S, 8), -1, dtype=np.int32), ring=z((S, ring_cap, k + 2)), ctr=z(S),
                bits=z((S, hw), np.uint32), draws=z(S))


def arm(st, s: int, k: int, V: int, hist: Sequence[int], position: int, length: int, cap: int, budget: int, counter: int,
        history_ids: Sequence[int], stop_ids: Sequence[int]) -> None:
    """pc_lookup_slot_arm on the numpy state: every word of slot ``s``, nothing of another slot."""
    st["hist"][s, :len(hist)] = hist
    st["hist_len"][s] = len(hist)
    st["ids"][s, 0], st["pos"][s, 0], st["ndraft"][s] = hist[-1], position, 0
    st["cap"][s], st["len"][s], st["budget"][s], st["ctr"][s], st["draws"][s] = cap, length, budget, counter, 1
    st["stop_ids"][s] = -1
    st["stop_ids"][s, :len(stop_ids)] = list(stop_ids)
    st["bits"][s] = lsr.history_bits(history_ids, V)
    st["live"][s] = 1


def simulate_serve(model: Callable[[Sequence[int]], np.ndarray], requests: List[dict], S: int, k: int, hist_cap: int, nmax: int = 3,
                   ring_cap: int = 4):
    """Continuous admission on the host model ``model`` (prefix of tokens -> logits of the next).  ``requests[r]`` = dict(prefix,
    first, corpus, max_new, params, seed, history_ids, stop_ids): the sequence feeds ``first`` behind ``prefix`` and may emit
    ``max_new`` tokens.  Requests take the lowest free slot in order, at replay 0 or as soon as a slot's sequence is over; every
    replay is draft_slots -> the rows ``model`` gives -> verify_slots_each.  -> (per-step token lists per request, dict(draws, bits) per
    request at its end, replays)."""
    V = int(np.asarray(model(list(requests[0]["prefix"]) + [int(requests[0]["first"])])).size)
    st = new_state(S, k, V, hist_cap, ring_cap)
    params, seeds = [GREEDY] * S, [0] * S
    slot_req: List[Optional[int]] = [None] * S
    seq: List[List[int]] = [[] for _ in range(S)]        # the tokens in front of the fed one
    out = {r: [] for r in range(len(requests))}
    end: Dict[int, dict] = {}
    nxt, n = 0, 0
    while True:
        for s in range(S):
            if slot_req[s] is None and nxt < len(requests):
                q = requests[nxt]
                hist = fit_history(q["corpus"], q["first"], q["max_new"], hist_cap)
                n0 = len(q["prefix"])
                arm(st, s, k, V, hist, n0, n0, n0 + q["max_new"] + k + 2, q["max_new"], n, q["history_ids"], q["stop_ids"])
                params[s], seeds[s] = q["params"], q["seed"]
                slot_req[s], seq[s] = nxt, [int(t) for t in q["prefix"]]
                nxt += 1
        if all(r is None for r in slot_req):
            return out, end, n
        st = lsl.draft_slots(st, k, nmax)
        R1 = k + 1
        logits = np.zeros((S * R1, V), dtype=np.float32)
        for s in range(S):
            if slot_req[s] is not None and lsl.runs(st, s, k):
                for i in range(R1):
                    logits[s * R1 + i] = model(seq[s] + [int(t) for t in st["ids"][s][:i + 1]])
        fed = st["ids"][:, 0].copy()
        st, _ = verify_slots_each(logits, st, k, ring_cap, params, seeds)
        assert all(int(c) == n + 1 for c in st["ctr"][[s for s in range(S) if slot_req[s] is not None]]), "record c belongs to replay c"
        for s in range(S):
            r = slot_req[s]
            if r is None:
                continue
            rec = st["ring"][s, n % ring_cap]
            toks = [int(t) for t in rec[1:1 + int(rec[0])]]
            out[r].append(toks)
            seq[s] += [int(fed[s])] + toks[:-1] if toks else []
            if not st["live"][s]:
                end[r] = dict(draws=int(st["draws"][s]), bits=st["bits"][s].copy())
                slot_req[s] = None
        n += 1


# ---- the mixed case of the GPU test (tests/test_gpu_lookup_serve.py) and of its CPU condition --------------------------------------
# S = 6, k = 3: slot 0 plain greedy with a stop id in the middle of an accepted run; slot 1 sampled, three right drafts; slot 2
# idle; slot 3 live without room for a step's rows; slot 4 sampled with a budget that cuts the step; slot 5 greedy with a penalty,
# one right draft and a wrong one.  Two steps: the second runs on what the first left (slots 0, 3 and 4 are off by then).
EACH_S, EACH_K, EACH_RING, EACH_HIST_CAP, EACH_STEPS = 6, 3, 4, 64, 2
EACH_PARAMS = [GREEDY, SAMPLED, GREEDY, SAMPLED, WIDE, GREEDY_RP]
EACH_LIVE = [1, 1, 0, 1, 1, 1]
EACH_LENS = [40, 43, 46, 77, 52, 55]
EACH_CAPS = [900, 900, 900, 80, 900, 900]             # slot 3: len + k + 1 > cap
EACH_BUDGET = [9, 9, 9, 9, 2, 9]
EACH_DRAWS = [1, 5, 1, 8, 11, 3]
EACH_CTR = 7
EACH_PLAN = [[(3, 3), (3, 3), None, None, (3, 3), (1, 2)],      # per step and slot: (right drafts, drafts)
             [None, (1, 3), None, None, None, (2, 2)]]
# rng seeds per vocabulary size, picked on the CPU (test_lookup_serve_cpu.test_each_case_seeds_leave_three_quarters_comparable runs
# the reference alone): at least 3/4 of the live sampled (slot, row) pairs have a margin above MARGIN
EACH_RNG_SEED = {1001: 21, 32000: 22}


def each_case(V: int):
    """-> (state before step 0, seeds, logits per step): drafts are written per step by ``each_drafts``."""
    rng = np.random.default_rng(EACH_RNG_SEED[V])
    S, k = EACH_S, EACH_K
    st = new_state(S, k, V, EACH_HIST_CAP, EACH_RING)
    for b in range(S):
        h = rng.integers(b * (V // S), (b + 1) * (V // S), 20).astype(np.int32)
        st["hist"][b, :20], st["hist_len"][b] = h, 20
        st["ids"][b, 0], st["pos"][b, 0] = h[-1], 100 + b
        st["bits"][b] = lsr.history_bits(h, V)
    st["ring"][:] = -7
    for name, vals in (("cap", EACH_CAPS), ("len", EACH_LENS), ("live", EACH_LIVE), ("budget", EACH_BUDGET), ("draws", EACH_DRAWS)):
        st[name][:] = vals
    st["ctr"][:] = EACH_CTR
    for b in range(S):
        st["stop_ids"][b, 0] = (7 * b + 5) % V
    seeds = [int(s) for s in rng.integers(0, 2 ** 62, S)]
    logits = [(rng.standard_normal((S * (k + 1), V)) * 2.0).astype(np.float32) for _ in range(EACH_STEPS)]
    return st, seeds, logits


def each_drafts(st, logits, seeds, plan) -> None:
    """The draft stage of one step, made up: slot b gets ``plan[b] = (right, total)`` drafts -- the first ``right`` are the
    reference's own draws of rows 0.., the next one is wrong -- written to ids[b][1..] / pos / ndraft in place.  At step 0 slot 0's
    stop row also gets the draw of its row 1: a stop id in the middle of an accepted run."""
    k, V = EACH_K, logits.shape[1]
    for b, pl in enumerate(plan):
        st["pos"][b, 1:] = st["pos"][b, 0] + np.arange(1, k + 1)
        if pl is None:
            st["ids"][b, 1:], st["ndraft"][b] = st["ids"][b, 0], 0
            continue
        right, total = pl
        base = lsr.bits_ids(st["bits"][b], V)
        drafts: List[int] = []
        for i in range(total):
            tok, _, _ = lsr.draw(logits[b * (k + 1) + i], base + drafts, EACH_PARAMS[b], seeds[b], int(st["draws"][b]) + i)
            drafts.append(int(tok) if i < right else (int(tok) + 1) % V)
        st["ids"][b, 1:1 + total], st["ids"][b, 1 + total:], st["ndraft"][b] = drafts, st["ids"][b, 0], total
        if b == 0 and right >= 2:
            st["stop_ids"][0, 1] = drafts[1]


def each_reference_margins(V: int):
    """The reference alone over the case: margins of the live sampled (slot, row) pairs (params other than plain greedy)."""
    st, seeds, logits = each_case(V)
    margins = []
    for step in range(EACH_STEPS):
        each_drafts(st, logits[step], seeds, EACH_PLAN[step])
        st, infos = verify_slots_each(logits[step], st, EACH_K, EACH_RING, EACH_PARAMS, seeds)
        for b, info in enumerate(infos):
            if info is not None and EACH_PARAMS[b] != GREEDY:
                margins += [float(m) for m in info["margins"]]
    return margins


def lookup_arm_block_bytes(native, hist_words: int, hist_ids: Sequence[int], **f) -> bytearray:
    """A pc_lookup_slot_arm block as bytes: ``f`` = fields of pc_lookup_slot_arm_block (params: a 4-tuple, stop_ids: a list, bits:
    uint32 words), then the bitmap, then the history ids."""
    import ctypes
    buf = bytearray(native.lookup_slot_arm_bytes(hist_words, len(hist_ids)))
    b = native.LookupSlotArmBlock.from_buffer(buf)
    for name in ("slot", "cap", "kv_base", "len", "pos", "id", "leader", "trunk", "budget", "counter", "seed"):
        setattr(b, name, int(f[name]))
    b.hist_words, b.hist_len = hist_words, len(hist_ids)
    b.params = native.SampleParams.from_buffer_copy(native.sample_params_bytes(*f["params"], 0))
    for j in range(8):
        b.stop_ids[j] = int(f["stop_ids"][j]) if j < len(f["stop_ids"]) else -1
    del b
    n0 = ctypes.sizeof(native.LookupSlotArmBlock)
    buf[n0:n0 + 4 * hist_words] = np.asarray(f["bits"], dtype=np.uint32).tobytes()
    n1 = n0 + ((4 * hist_words + 7) & ~7)
    buf[n1:n1 + 4 * len(hist_ids)] = np.asarray(hist_ids, dtype=np.int32).tobytes()
    return buf
