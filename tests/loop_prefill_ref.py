"""numpy restatement of the FORCED ROWS of the lookup step over slots (csrc/pc_lookup_common.h: lookup_draft_forced_rule,
lookup_accept_forced_rule; the entries pc_lookup_slot_arm_prompt, pc_lookup_draft_slots_prompt, pc_lookup_verify_slots_prompt) and
the inputs of the GPU cases.  Test infrastructure only; built on tests/lookup_serve_ref.py, imports nothing of the product.

The state is ``lookup_serve_ref.new_state``'s plus ``forced`` int32 [S]: the prompt tokens still to be fed behind ``ids[b][0]``.
A running slot with ``forced[b] = R > 0`` has ``hist[L - 1] = ids[b][0]`` and ``hist[L .. L + R)`` = the tokens to feed
(``L = hist_len[b]``).  Per step: the draft feeds ``m = min(k, R)`` of them; for ``R > k`` nothing is drawn, the record is EMPTY and
the slot moves on by ``k + 1`` rows; for ``R <= k`` row ``R`` alone is drawn -- as a sequence's first token: under the bitmap as it
stands at Philox step ``draws[b]`` -- and from there on every word of the slot but ``ctr`` is what ``arm`` leaves behind a serial
prefill that drew the same token.  A slot with ``forced[b] = 0`` and a slot that does not run are ``lookup_serve_ref``'s."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import lookup_sample_ref as lsr
from tests import lookup_serve_ref as lsv
from tests import lookup_slots_ref as lsl

GREEDY, SAMPLED, WIDE, GREEDY_RP, MARGIN = lsv.GREEDY, lsv.SAMPLED, lsv.WIDE, lsv.GREEDY_RP, lsv.MARGIN
WORDS = ("hist", "hist_len", "ids0", "pos0", "len", "budget", "draws", "bits", "stop_ids")     # what the equivalence compares


def new_state(S: int, k: int, V: int, hist_cap: int, ring_cap: int):
    st = lsv.new_state(S, k, V, hist_cap, ring_cap)
    st["forced"] = np.zeros(S, dtype=np.int32)
    return st


def fit_prompt_history(corpus: Sequence[int], ids: Sequence[int], max_new: int, hist_cap: int) -> List[int]:
    """The history of a sequence admitted with its question ``ids`` still to be fed: ``corpus ++ ids``, the whole question kept and
    the OLDEST corpus ids dropped until ``len + max_new <= hist_cap``; ValueError when ``len(ids) + max_new`` alone does not fit."""
    q = len(ids)
    if q + max_new > hist_cap:
        raise ValueError("the question and max_new exceed the history capacity")
    keep = hist_cap - max_new - q
    c = [int(t) for t in corpus]
    return (c[len(c) - keep:] if keep < len(c) else c) + [int(t) for t in ids] if keep > 0 else [int(t) for t in ids]


def arm_prompt(st, s: int, k: int, V: int, hist: Sequence[int], n_forced: int, position: int, length: int, cap: int, budget: int,
               counter: int, history_ids: Sequence[int], stop_ids: Sequence[int]) -> None:
    """pc_lookup_slot_arm_prompt on the numpy state: ``hist`` runs through the last question token, the last ``n_forced`` of its ids
    are still to be fed, ``position`` / ``length`` are those of the first question token and of the staged rows."""
    assert 0 <= n_forced < len(hist)
    lsv.arm(st, s, k, V, hist, position, length, cap, budget, counter, history_ids, stop_ids)
    st["hist_len"][s] = len(hist) - n_forced
    st["ids"][s, 0] = hist[len(hist) - n_forced - 1]
    st["forced"][s], st["draws"][s] = n_forced, 0


def draft_slots_prompt(st, k: int, nmax: int = 3):
    """pc_lookup_draft_slots_prompt -> the new state (deep copy)."""
    forced = st["forced"]
    new = lsl.draft_slots({n: v for n, v in st.items() if n != "forced"}, k, nmax)
    new["forced"] = forced.copy()
    for b in range(len(st["live"])):
        R = int(forced[b])
        if R <= 0 or not lsl.runs(st, b, k):
            continue
        L, m = int(st["hist_len"][b]), min(k, R)
        ids, pos = st["ids"][b].copy(), st["pos"][b].copy()
        ids[1:] = ids[0]
        ids[1:1 + m] = st["hist"][b][L:L + m]
        pos[1:] = pos[0] + np.arange(1, k + 1)
        new["ids"][b], new["pos"][b], new["ndraft"][b] = ids, pos, m
    return new


def verify_slots_prompt(logits, st, k: int, ring_cap: int, params: Sequence[Tuple], seeds: Sequence[int],
                        force: Optional[Dict[Tuple[int, int], int]] = None):
    """pc_lookup_verify_slots_prompt -> ``(new state, info)``: ``lookup_serve_ref.verify_slots_each`` for the slots without forced
    rows and for those that do not run; for a running slot with forced rows ``info[b]`` = dict(forced=R, emit=0 | 1, tokens,
    margins) -- the draw of row R and its float64 score margin where the question ends.  ``force[(b, i)]``: as there."""
    logits = np.asarray(logits, dtype=np.float32)
    S, rows = len(st["live"]), k + 1
    V = logits.shape[1]
    mine = [b for b in range(S) if int(st["forced"][b]) > 0 and lsl.runs(st, b, k)]
    # (the other slots: the parent rule on a state in which the forced slots do not run)
    rest = {n: np.array(v, copy=True) for n, v in st.items() if n != "forced"}
    for b in mine:
        rest["live"][b] = 0
    new, infos = lsv.verify_slots_each(logits, rest, k, ring_cap, params, seeds, force)
    new["forced"] = st["forced"].copy()
    ring = new["ring"].reshape(S, ring_cap, rows + 1)
    for b in mine:
        for w in ("live", "ctr"):
            new[w][b] = st[w][b]
        ring[b, int(st["ctr"][b]) % ring_cap] = st["ring"].reshape(S, ring_cap, rows + 1)[b, int(st["ctr"][b]) % ring_cap]
        R, L, c = int(st["forced"][b]), int(st["hist_len"][b]), int(st["ctr"][b])
        rec = ring[b, c % ring_cap]
        new["ctr"][b] = c + 1
        if R > k:
            rec[0] = 0
            new["hist_len"][b] = L + k + 1
            new["ids"][b][0] = st["hist"][b][L + k]
            new["pos"][b][0] += k + 1
            new["len"][b] += k + 1
            new["forced"][b] = R - k - 1
            infos[b] = dict(forced=R, emit=0, tokens=[], margins=[])
            continue
        m = R
        g, margin, _ = lsr.draw(logits[b * rows + m], lsr.bits_ids(st["bits"][b], V), params[b], seeds[b], int(st["draws"][b]))
        if force and (b, m) in force:
            g = force[(b, m)]
        g, bud = int(g), int(st["budget"][b])
        rec[0], rec[1] = 1, g
        new["hist"][b][L + m] = g
        new["hist_len"][b] = L + m + 1
        new["ids"][b][0] = g
        new["pos"][b][0] += m + 1
        new["len"][b] += m + 1
        new["forced"][b] = 0
        new["budget"][b] = bud - 1
        new["draws"][b] = 1
        new["bits"][b][g >> 5] |= np.uint32(1 << (g & 31))
        if g in set(int(t) for t in st["stop_ids"][b]) or bud - 1 <= 0 or int(new["len"][b]) + k + 1 > int(st["cap"][b]):
            new["live"][b] = 0
        infos[b] = dict(forced=R, emit=1, tokens=[g], margins=[float(margin)])
    return new, infos


def words(st, b: int, k: int) -> dict:
    """The words of slot ``b`` the equivalence with the serial arm is stated on (``WORDS``): everything but ``ctr``, the ring, the
    draft rows 1.. and ``ndraft`` -- which the next draft rewrites -- with the history cut at ``hist_len``."""
    L = int(st["hist_len"][b])
    return dict(hist=st["hist"][b][:L].tolist(), hist_len=L, ids0=int(st["ids"][b][0]), pos0=int(st["pos"][b][0]), len=int(st["len"][b]),
                budget=int(st["budget"][b]), draws=int(st["draws"][b]), bits=st["bits"][b].tolist(), stop_ids=st["stop_ids"][b].tolist(),
                live=int(st["live"][b]), forced=int(st["forced"][b]))


def serial_words(S: int, k: int, V: int, hist_cap: int, s: int, corpus: Sequence[int], question: Sequence[int], g: int, position0: int,
                 staged: int, cap: int, max_new: int, history_ids: Sequence[int], stop_ids: Sequence[int]) -> dict:
    """What today's flow leaves in slot ``s``: a serial prefill of ``question`` over ``staged`` rows drew ``g``; the sequence is armed
    (``lookup_serve_ref.arm``) feeding ``g`` at ``position0 + q`` over ``staged + q`` rows with ``max_new - 1`` tokens to go."""
    q = len(question)
    st = new_state(S, k, V, hist_cap, 4)
    hist = lsv.fit_history(list(corpus) + [int(t) for t in question], g, max_new - 1, hist_cap)
    lsv.arm(st, s, k, V, hist, position0 + q, staged + q, cap, max_new - 1, 0, list(history_ids) + [g], stop_ids)
    w = words(st, s, k)
    # the device's own stop rules act on g in the in-loop flow; the serial flow never arms a sequence that ended with its first token
    w["live"] = int(not (g in set(stop_ids) or max_new - 1 <= 0 or staged + q + k + 1 > cap))
    return w


def feed_question(S: int, k: int, V: int, hist_cap: int, s: int, corpus: Sequence[int], question: Sequence[int], position0: int,
                  staged: int, cap: int, max_new: int, params: Tuple, seed: int, history_ids: Sequence[int], stop_ids: Sequence[int],
                  row_logits, ring_cap: int = 4):
    """The in-loop flow on the reference alone: slot ``s`` is armed with ``question`` still to be fed and stepped until its first
    token is out (or it stops running).  ``row_logits(prefix ids) -> logits`` of the row that ends the prefix.  -> (state, steps,
    first token | None)."""
    st = new_state(S, k, V, hist_cap, ring_cap)
    hist = fit_prompt_history(corpus, question, max_new, hist_cap)
    arm_prompt(st, s, k, V, hist, len(question) - 1, position0, staged, cap, max_new, 0, history_ids, stop_ids)
    prm, seeds = [GREEDY] * S, [0] * S
    prm[s], seeds[s] = params, seed
    fed: List[int] = []
    steps = 0
    while st["live"][s] and lsl.runs(st, s, k):          # (forced rows that run out at a step's end leave the last token to an ordinary step)
        st = draft_slots_prompt(st, k)
        logits = np.zeros((S * (k + 1), V), dtype=np.float32)
        for i in range(k + 1):
            logits[s * (k + 1) + i] = row_logits(fed + [int(t) for t in st["ids"][s][:i + 1]])
        nd = int(st["ndraft"][s])
        fed += [int(t) for t in st["ids"][s][:nd + 1]]
        st, infos = verify_slots_prompt(logits, st, k, ring_cap, prm, seeds)
        steps += 1
        if infos[s] is not None and infos[s]["emit"]:
            return st, steps, infos[s]["tokens"][0]
    return st, steps, None


# ---- the case of tests/test_gpu_loop_prefill.py ----------------------------------------------------------------------------------
# S = 3: slot 0 is fed a question of q tokens, slot 1 decodes (drafts made up as in lookup_serve_ref.each_drafts), slot 2 is idle.
CASE_S, CASE_RING, CASE_HIST_CAP = 3, 4, 96
CASE_RNG_SEED = {1001: 31, 32000: 32}


def case(V: int, k: int, params0: Tuple, q: int):
    """-> (state before step 0, params, seeds, logits per step, steps): slot 0 armed by ``arm_prompt`` with ``q`` question tokens
    behind a corpus of 12 ids, slot 1 a decoding slot with 20 ids of history, slot 2 idle with stale words."""
    rng = np.random.default_rng(CASE_RNG_SEED[V] + 7 * k + q)
    S = CASE_S
    st = new_state(S, k, V, CASE_HIST_CAP, CASE_RING)
    params = [params0, SAMPLED if params0 == GREEDY else GREEDY, WIDE]
    seeds = [int(s) for s in rng.integers(0, 2 ** 62, S)]
    for b in (1, 2):
        h = rng.integers(b * (V // S), (b + 1) * (V // S), 20).astype(np.int32)
        lsv.arm(st, b, k, V, h.tolist(), 100 + b, 40 + b, 900, 50, 5, h.tolist(), [(7 * b + 5) % V])
    st["live"][2], st["draws"][1] = 0, 4
    corpus = rng.integers(0, V // S, 12).tolist()
    question = rng.integers(0, V // S, q).tolist()
    hist = fit_prompt_history(corpus, question, 9, CASE_HIST_CAP)
    arm_prompt(st, 0, k, V, hist, q - 1, 200, 64, 900, 9, 5, corpus[:5] + question, [3])
    st["ring"][:] = -7
    steps = -(-q // (k + 1)) + 2                    # the prefill, then two decoding steps of the slot
    logits = [(rng.standard_normal((S * (k + 1), V)) * 2.0).astype(np.float32) for _ in range(steps)]
    return st, params, seeds, logits, steps


def case_drafts(st, logits, params, seeds, k: int, right: int, total: int) -> None:
    """The draft stage of a decoding slot, made up (``lookup_serve_ref.each_drafts``' recipe): every running slot WITHOUT forced
    rows gets ``total`` drafts of which the first ``right`` are the reference's own draws -- written in place behind the real draft
    launch, which a GPU test runs first for the slots with forced rows."""
    V = logits.shape[1]
    for b in range(len(st["live"])):
        if not lsl.runs(st, b, k) or int(st["forced"][b]) > 0:
            continue
        st["pos"][b, 1:] = st["pos"][b, 0] + np.arange(1, k + 1)
        base = lsr.bits_ids(st["bits"][b], V)
        drafts: List[int] = []
        for i in range(min(total, k)):
            tok, _, _ = lsr.draw(logits[b * (k + 1) + i], base + drafts, params[b], seeds[b], int(st["draws"][b]) + i)
            drafts.append(int(tok) if i < right else (int(tok) + 1) % V)
        st["ids"][b, 1:], st["ndraft"][b] = st["ids"][b, 0], len(drafts)
        st["ids"][b, 1:1 + len(drafts)] = drafts


def case_reference_margins(V: int, k: int, params0: Tuple, q: int):
    """The reference alone over ``case``: the float64 score margins of the sampled rows it draws (params other than plain greedy)."""
    st, params, seeds, logits, steps = case(V, k, params0, q)
    margins: List[float] = []
    for step in range(steps):
        st = draft_slots_prompt(st, k)
        case_drafts(st, logits[step], params, seeds, k, 2, 3)
        st, infos = verify_slots_prompt(logits[step], st, k, CASE_RING, params, seeds)
        for b, info in enumerate(infos):
            if info is not None and params[b] != GREEDY:
                margins += [float(m) for m in info["margins"]]
    return margins
