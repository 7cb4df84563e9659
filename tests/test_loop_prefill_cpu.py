"""Prefill inside the lookup step, the parts that need no GPU: the forced-row rule (tests/loop_prefill_ref.py) on a toy
model against the serial arm, its reduction to tests/lookup_serve_ref.py with no forced rows, the history an in-loop admission
keeps, ``check_loop_prefill`` / ``serve_plan(loop_prefill=True)``, the C-ABI of the three entries and ``serve(loop_prefill=True)``
over a scripted loop."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import lookup_sample_ref as lsr
from tests import lookup_serve_ref as lsv
from tests import lookup_slots_ref as lsl
from tests import loop_prefill_ref as ref
from tests.test_lookup_sample_cpu import PREFIX, V, toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pc_lookup_slot_arm_prompt", "pc_lookup_draft_slots_prompt", "pc_lookup_verify_slots_prompt")
S, HIST_CAP, STAGED, POS0 = 3, 64, len(PREFIX), 40
CORPUS = [0, 1, 2, 3, 4, 5, 0, 2, 4]                       # ids below 11, the last token of every question: see _question
QKINDS = {"1": lambda k: 1, "k": lambda k: k, "k+1": lambda k: k + 1, "k+2": lambda k: k + 2, "2(k+1)+1": lambda k: 2 * (k + 1) + 1}


def _question(q, seed=0):
    """q ids; the last one occurs nowhere else.  Where q = 1 mod (k + 1) the forced rows run out at a step's end and the last token
    is fed by an ORDINARY step (forced = 0, draws = 0), which would draft behind a token it finds in its history: here it finds
    none, so that step too emits the first token alone and the words can be compared with the serial arm's."""
    return np.random.default_rng(seed).integers(0, 11, q - 1).tolist() + [11]


def _feed(k, question, params, max_new=9, cap=200, stop_ids=(), seed=77, s=1):
    history = PREFIX + question
    return ref.feed_question(S, k, V, HIST_CAP, s, CORPUS, question, POS0, STAGED, cap, max_new, params, seed, history, list(stop_ids),
                             lambda fed: toy_model(PREFIX + fed))


def _serial(k, question, params, max_new=9, cap=200, stop_ids=(), seed=77, s=1):
    history = PREFIX + question
    g = int(lsr.draw(toy_model(PREFIX + question), history, params, seed, 0)[0])
    return g, ref.serial_words(S, k, V, HIST_CAP, s, CORPUS, question, g, POS0, STAGED, cap, max_new, history, list(stop_ids))


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [ref.GREEDY, (0.7, 1.3, 0.9, 4), ref.GREEDY_RP], ids=["greedy", "chain", "greedy_rp"])
@pytest.mark.parametrize("kind", list(QKINDS))
def test_a_question_fed_through_the_rows_leaves_the_words_of_the_serial_arm(kind, params):
    """q tokens at k = 1, 3, 7: ceil(q / (k + 1)) steps, EMPTY records until the last, and then every word but ctr is what
    pc_lookup_slot_arm writes behind a serial prefill that drew the same first token -- so the words are the same at every k."""
    for k in (1, 3, 7):
        q = QKINDS[kind](k)
        question = _question(q, seed=q)
        st, steps, g = _feed(k, question, params)
        want_g, want = _serial(k, question, params)
        assert steps == -(-q // (k + 1)) and g == want_g, (k, q)
        got = ref.words(st, 1, k)
        assert got["forced"] == 0 and got == want, (k, q)
        ring = st["ring"][1]
        assert [int(r[0]) for r in ring[:steps]] == [0] * (steps - 1) + [1] and int(ring[steps - 1][1]) == g
        assert int(st["ctr"][1]) == steps and st["ctr"][0] == steps and st["live"][0] == 0       # (an idle neighbour keeps pace)


def test_forced_rows_step_by_step():
    """k = 3, q = 6: step 0 feeds t_0..t_3 and draws nothing, step 1 feeds t_4, t_5 and a pad row and draws row 1."""
    k, question = 3, [6, 7, 8, 9, 10, 11]
    st = ref.new_state(S, k, V, HIST_CAP, 4)
    hist = ref.fit_prompt_history(CORPUS, question, 9, HIST_CAP)
    ref.arm_prompt(st, 0, k, V, hist, 5, POS0, STAGED, 200, 9, 3, PREFIX + question, [])
    L = len(CORPUS) + 1
    assert int(st["hist_len"][0]) == L and int(st["forced"][0]) == 5 and int(st["draws"][0]) == 0 and int(st["ids"][0, 0]) == 6
    st = ref.draft_slots_prompt(st, k)
    assert st["ids"][0].tolist() == [6, 7, 8, 9] and st["pos"][0].tolist() == [40, 41, 42, 43] and int(st["ndraft"][0]) == 3
    logits = np.zeros((S * 4, V), dtype=np.float32)
    logits[:, 2] = 5.0
    bits = st["bits"].copy()
    st, info = ref.verify_slots_prompt(logits, st, k, 4, [ref.GREEDY] * S, [0] * S)
    assert info[0] == dict(forced=5, emit=0, tokens=[], margins=[])
    assert (int(st["hist_len"][0]), int(st["ids"][0, 0]), int(st["pos"][0, 0]), int(st["len"][0]), int(st["forced"][0])) == \
        (L + 4, 10, 44, STAGED + 4, 1)
    assert int(st["budget"][0]) == 9 and int(st["draws"][0]) == 0 and np.array_equal(st["bits"], bits) and int(st["ctr"][0]) == 4
    assert int(st["ring"][0, 3, 0]) == 0 and int(st["live"][0]) == 1
    st = ref.draft_slots_prompt(st, k)
    assert st["ids"][0].tolist() == [10, 11, 10, 10] and int(st["ndraft"][0]) == 1 and st["pos"][0].tolist() == [44, 45, 46, 47]
    logits[1, 4] = 9.0                                       # row 1 ends the question; rows 0, 2, 3 would say 2
    st, info = ref.verify_slots_prompt(logits, st, k, 4, [ref.GREEDY] * S, [0] * S)
    assert info[0]["tokens"] == [4] and info[0]["emit"] == 1
    assert (int(st["hist_len"][0]), int(st["ids"][0, 0]), int(st["pos"][0, 0]), int(st["len"][0]), int(st["forced"][0])) == \
        (L + 6, 4, 46, STAGED + 6, 0)
    assert st["hist"][0, L + 4:L + 6].tolist() == [11, 4] and int(st["budget"][0]) == 8 and int(st["draws"][0]) == 1
    assert lsr.bits_ids(st["bits"][0], V) == sorted(set(PREFIX + question + [4])) and st["ring"][0, 0].tolist()[:2] == [1, 4]


def test_without_forced_rows_the_reference_is_the_parents():
    for Vv in lsv.EACH_RNG_SEED:
        st0, seeds, logits = lsv.each_case(Vv)
        lsv.each_drafts(st0, logits[0], seeds, lsv.EACH_PLAN[0])
        mine = dict(st0, forced=np.zeros(lsv.EACH_S, dtype=np.int32))
        a, ia = lsv.verify_slots_each(logits[0], st0, lsv.EACH_K, lsv.EACH_RING, lsv.EACH_PARAMS, seeds)
        b, ib = ref.verify_slots_prompt(logits[0], mine, lsv.EACH_K, lsv.EACH_RING, lsv.EACH_PARAMS, seeds)
        assert all(np.array_equal(a[w], b[w]) for w in a) and not b["forced"].any()
        assert [None if i is None else i["tokens"] for i in ia] == [None if i is None else i["tokens"] for i in ib]
        da, db = lsl.draft_slots(st0, lsv.EACH_K), ref.draft_slots_prompt(mine, lsv.EACH_K)
        assert all(np.array_equal(da[w], db[w]) for w in da)


def test_budget_one_a_stop_id_and_a_slot_without_room():
    k, question = 3, _question(5, seed=3)
    # budget 1: the first token is the last -- emitted, the slot is off, the words still the serial arm's
    st, steps, g = _feed(k, question, ref.GREEDY, max_new=1)
    want_g, want = _serial(k, question, ref.GREEDY, max_new=1)
    got = ref.words(st, 1, k)
    assert g == want_g and got["forced"] == 0 and got == want and got["live"] == 0 and got["budget"] == 0
    # the first token is a stop id: emitted, the slot is off
    st, steps, g2 = _feed(k, question, ref.GREEDY, stop_ids=[g])
    got = ref.words(st, 1, k)
    assert g2 == g and got["live"] == 0 and got["budget"] == 8 and int(st["ring"][1, steps - 1, 0]) == 1
    assert got["forced"] == 0 and got == _serial(k, question, ref.GREEDY, stop_ids=[g])[1]
    # no room for the steps behind the question: the question is fed, the first token is out, the slot is off (len + k + 1 > cap)
    st, steps, g3 = _feed(k, question, ref.GREEDY, cap=STAGED + 5 + k)
    assert g3 == g and ref.words(st, 1, k)["live"] == 0 and int(st["len"][1]) == STAGED + 5
    # no room for a step of the question itself: the slot does not run -- EMPTY record, live = 0, every other word as it was
    st = ref.new_state(S, k, V, HIST_CAP, 4)
    hist = ref.fit_prompt_history(CORPUS, question, 9, HIST_CAP)
    ref.arm_prompt(st, 1, k, V, hist, 4, POS0, STAGED, STAGED + k, 9, 0, PREFIX + question, [])
    before = ref.words(st, 1, k)
    st2 = ref.draft_slots_prompt(st, k)
    assert all(np.array_equal(st[w], st2[w]) for w in st)
    st2, info = ref.verify_slots_prompt(np.zeros((S * 4, V), dtype=np.float32), st2, k, 4, [ref.GREEDY] * S, [0] * S)
    after = ref.words(st2, 1, k)
    assert info[1] is None and after.pop("live") == 0 and before.pop("live") == 1 and after == before and after["forced"] == 4
    assert int(st2["ring"][1, 0, 0]) == 0 and int(st2["ctr"][1]) == 1


def test_case_seeds_leave_three_quarters_comparable():
    """The condition tests/test_gpu_loop_prefill.py relies on, met by the reference alone: in every case at least 3/4 of the sampled
    rows have a float64 score margin above 1e-4."""
    for Vv in ref.CASE_RNG_SEED:
        for k in (1, 3, 7):
            for params0 in (ref.GREEDY, ref.SAMPLED):
                m = [x for q in (k + 3, k + 2) for x in ref.case_reference_margins(Vv, k, params0, q)]
                assert m and 4 * sum(x > ref.MARGIN for x in m) >= 3 * len(m), (Vv, k, params0, sorted(m)[:4])


# ---- the history ---------------------------------------------------------------------------------------------------------------------
def test_the_whole_question_stays_in_the_history_and_equals_the_serial_admission():
    from promptcache_amd.model.llama_hip import lookup_admit_history, lookup_prompt_history
    for fit in (ref.fit_prompt_history, lookup_prompt_history):
        assert fit([1, 2, 3], [7, 8], 4, 16) == [1, 2, 3, 7, 8]
        assert fit(list(range(20)), [7, 8], 4, 16) == list(range(10, 20)) + [7, 8]        # 10 corpus ids + 2 + 4 new = 16
        assert fit(list(range(20)), [7, 8], 14, 16) == [7, 8] and fit([], [7], 15, 16) == [7]
        with pytest.raises(ValueError):
            fit([1], [7, 8], 15, 16)
    rng = np.random.default_rng(1)
    for _ in range(200):
        c, q = rng.integers(0, 50, int(rng.integers(0, 40))).tolist(), rng.integers(0, 50, int(rng.integers(1, 9))).tolist()
        mn, cap = int(rng.integers(1, 12)), int(rng.integers(21, 40))
        h = lookup_prompt_history(c, q, mn, cap)
        assert h == ref.fit_prompt_history(c, q, mn, cap) and len(h) + mn <= cap and h[len(h) - len(q):] == q
        # behind the first token g it is the history a serial prefill of the question is admitted with
        assert h + [99] == lookup_admit_history(c + q, 99, mn - 1, cap)


# ---- check_loop_prefill, serve_plan ---------------------------------------------------------------------------------------------------
def _engine(hf):
    from promptcache_amd.generation_engine import GenerationEngine
    lm = types.SimpleNamespace(hf_model=hf, use_full_position_ids=False, decode=lambda ids: " ".join(map(str, ids)), device="cpu")
    ge = GenerationEngine(lm)
    ge.device_greedy_loop = ge.device_sample_loop = True
    return ge


def test_check_loop_prefill_names_the_conflict():
    from promptcache_amd.model.llama_hip import check_loop_prefill
    check_loop_prefill(False, 0, "int8")
    check_loop_prefill(True, 3)
    check_loop_prefill(True, 15, "fp16")
    with pytest.raises(ValueError, match="lookup is off"):
        check_loop_prefill(True, 0)
    with pytest.raises(ValueError, match="no lookup step"):
        check_loop_prefill(True, 0, "fp16", "the model has no lookup step")
    with pytest.raises(ValueError, match="int8"):
        check_loop_prefill(True, 3, "int8")


def test_serve_plan_names_the_mode_and_serve_refuses_before_anything_is_allocated(monkeypatch):
    full = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True, lookup_slot_loop=None, lookup_available=lambda: True,
                                 lookup_slot_q8_available=lambda: True, D=128)
    no_step = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True, lookup_slot_loop=None, lookup_available=lambda: False)
    ge = _engine(full)
    for args in ((), (3, 4), (7, 16), (40, 4)):
        assert ge.serve_plan(*args) == ge.serve_plan(*args, loop_prefill=False)
    ok, why = ge.serve_plan(3, 4, loop_prefill=True)
    assert ok and why.startswith(ge.serve_plan(3, 4)[1]) and "loop_prefill=True" in why and "prefilled inside" in why
    for bad, word in ((dict(lookup=0, slots=4), "lookup is off"), (dict(lookup=7, slots=16), "64"),
                      (dict(lookup=3, slots=4, slot_kv="int8"), "int8")):
        with pytest.raises(ValueError, match=word):
            ge.serve_plan(loop_prefill=True, **bad)
    with pytest.raises(ValueError, match="no lookup step"):
        _engine(no_step).serve_plan(3, 4, loop_prefill=True)

    def process(*a, **kw):
        raise AssertionError("serve asked the cache engine for something")
    ce = types.SimpleNamespace(process=process, slots=4, max_ctx_length=4096)
    for kw, word in ((dict(lookup=0), "lookup is off"), (dict(lookup=3, slot_kv="int8"), "int8")):
        with pytest.raises(ValueError, match=word):
            next(ge.serve(ce, iter([1]), None, loop_prefill=True, **kw))
    monkeypatch.setenv("PC_SERVE_LOOP_PREFILL", "1")
    with pytest.raises(ValueError, match="lookup is off"):
        next(ge.serve(ce, iter([1]), None))
    with pytest.raises(ValueError, match="no batched decode loop|does not run"):
        next(_engine(None).serve(ce, iter([1]), None, lookup=3))


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    from promptcache_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "promptcache_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.lib_path())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _native.SIGNATURES, name
    # each entry is its parent plus `forced` (and n_forced): the argument lists say so
    sig = _native.SIGNATURES
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    d, v, a = (sig[n][1] for n in ("pc_lookup_draft_slots", "pc_lookup_verify_slots_each", "pc_lookup_slot_arm"))
    assert sig["pc_lookup_draft_slots_prompt"] == (ctypes.c_int, d[:9] + [vp] + d[9:])
    assert sig["pc_lookup_verify_slots_prompt"] == (ctypes.c_int, v[:24] + [vp] + v[24:])
    assert sig["pc_lookup_slot_arm_prompt"] == (ctypes.c_int, a[:3] + [vp, i32] + a[3:])


def test_the_structs_did_not_change(tmp_path):
    """pc_lookup_slot_arm_block / pc_lookup_slot_state are the parent's: sizes and offsets of the ctypes mirrors against gcc."""
    import subprocess
    from promptcache_amd import _native
    structs = (("pc_lookup_slot_arm_block", _native.LookupSlotArmBlock, 120), ("pc_lookup_slot_state", _native.LookupSlotState, 144))
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {']
    for st, cls, _ in structs:
        body.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        body += [f'  printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    body += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    for st, cls, size in structs:
        assert int(got[st]) == ctypes.sizeof(cls) == size, st
        for name, _ in cls._fields_:
            assert int(got[f"{st}.{name}"]) == getattr(cls, name).offset, (st, name)


def test_entries_reject_bad_arguments_without_a_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)

    def draft(S=4, k=3, nmax=3, hist_cap=64, hist=p, forced=p):
        return lib.pc_lookup_draft_slots_prompt(hist, p, hist_cap, p, p, p, p, p, p, forced, S, k, nmax, None)
    for bad in (dict(S=0), dict(S=17), dict(k=0), dict(k=16), dict(S=8, k=8), dict(nmax=0), dict(nmax=9), dict(hist_cap=0),
                dict(hist_cap=1 << 24), dict(hist=None), dict(forced=None)):
        assert draft(**bad) == -1001, bad
        assert b"pc_lookup_draft_slots_prompt" in lib.pc_last_error_string()

    def verify(S=4, k=3, V=1001, ldl=1001, logits=p, params=p, ring_cap=16, hist_cap=64, forced=p):
        return lib.pc_lookup_verify_slots_prompt(logits, ldl, V, S, k, params, p, p, p, p, p, p, p, hist_cap, p, p, p, p, p, p, p, p, p, p,
                                                 forced, ring_cap, None)
    for bad in (dict(S=0), dict(S=17), dict(k=0), dict(k=16), dict(S=8, k=8), dict(V=0), dict(V=1 << 24, ldl=1 << 24), dict(ldl=1000),
                dict(logits=p + 2), dict(params=p + 4), dict(ring_cap=0), dict(hist_cap=0), dict(logits=None), dict(forced=None)):
        assert verify(**bad) == -1001, bad
        assert b"pc_lookup_verify_slots_prompt" in lib.pc_last_error_string()
    state = _native.LookupSlotState(*([p] * len(_native.LookupSlotState._fields_)))
    hw = 32

    def arm(S=4, k=3, hist_cap=64, slot=1, words=hw, hist_len=5, nbytes=None, pad=0, st=state, forced=p, n_forced=2):
        raw = (ctypes.c_uint64 * 64)()
        b = _native.LookupSlotArmBlock.from_address(ctypes.addressof(raw) + pad)
        b.slot, b.hist_words, b.hist_len = slot, words, hist_len
        nb = _native.lookup_slot_arm_bytes(words, max(hist_len, 0)) if nbytes is None else nbytes
        return lib.pc_lookup_slot_arm_prompt(ctypes.addressof(raw) + pad, nb, ctypes.byref(st), forced, n_forced, S, k, hist_cap, None)
    null = _native.LookupSlotState(*([p] * 17 + [None]))
    for bad in (dict(S=0), dict(S=17), dict(k=0), dict(S=8, k=8), dict(hist_cap=0), dict(slot=-1), dict(slot=4), dict(words=0),
                dict(hist_len=0), dict(hist_len=65), dict(nbytes=8), dict(pad=4), dict(st=null), dict(forced=None), dict(n_forced=-1),
                dict(n_forced=5), dict(n_forced=6)):
        assert arm(**bad) == -1001, bad
        assert b"pc_lookup_slot_arm_prompt" in lib.pc_last_error_string()
    assert lib.pc_lookup_slot_arm_prompt(None, 8, ctypes.byref(state), p, 0, 4, 3, 64, None) == -1001


# ---- serve(loop_prefill=True) over a scripted loop -------------------------------------------------------------------------------------
class _FakePromptLoop:
    """``LookupSlotLoop(each=True, prompt_rows=True)``'s protocol on the host: sequence j's tokens are ``1000 * tag + 0, + 1, ...``;
    a sequence admitted by ``admit`` already has its token 0 and gives ``width`` per replay from its start, one admitted by
    ``admit_prompt`` gives nothing for ``ceil(q / (k + 1)) - 1`` replays, then token 0 alone, then ``width`` per replay."""

    prompt_rows, hist_cap, nsplit_trunk = True, 8192, 0

    def __init__(self, k, width):
        self.k, self.width, self.n = k, width, 0
        self._start, self._max_new, self._tag, self._pre, self.idx, self.calls = [], [], [], [], [], []
        self.retired, self.closed = {}, None

    def enqueue(self):
        self.n += 1
        return self.n - 1

    def elapsed_ms(self, i):
        assert i < self.n
        return 1.0

    def first_step(self, j):
        return self._start[j] + max(self._pre[j] - 1, 0)

    def prefill_replays(self, j):
        return self._pre[j]

    def tokens(self, j, i):
        assert i < self.n, "the host asked for a replay it never enqueued"
        tag, mn = self._tag[j], self._max_new[j]
        if self._pre[j]:
            s = i - self.first_step(j)
            if s < 0:
                return []
            lo, hi = (0, 1) if s == 0 else (1 + (s - 1) * self.width, 1 + s * self.width)
            return [1000 * tag + t for t in range(lo, min(hi, mn))]
        s = i - self._start[j]
        return [] if s < 0 else [1000 * tag + 1 + t for t in range(s * self.width, min((s + 1) * self.width, mn))]

    def kill(self, j):
        raise AssertionError("nothing ends on the host here")

    def _enter(self, slot, tag, max_new, pre):
        assert not [j for j in range(len(self._tag)) if self.idx[j] == slot and j not in self.retired], "the slot's sequence was not retired"
        self._start.append(self.n); self._max_new.append(max_new); self._tag.append(tag); self._pre.append(pre); self.idx.append(slot)
        return len(self._tag) - 1

    def admit(self, slot, past, token, position, max_new, params, seed, history, stop_ids, corpus, trunk=None):
        self.calls.append(("admit", past.tag, position))
        return self._enter(slot, past.tag, max_new, 0)                   # (max_new: the tokens BEHIND the first)

    def admit_prompt(self, slot, past, ids, position0, max_new, params, seed, history, stop_ids, corpus, trunk=None, decode_gap=0):
        self.calls.append(("admit_prompt", past.tag, list(ids), position0, max_new, decode_gap, list(corpus)))
        return self._enter(slot, past.tag, max_new, -(-len(ids) // (self.k + 1)))

    def retire(self, j, consumed):
        self.retired[j] = consumed

    def close(self, consumed):
        self.closed = dict(consumed)


def _fake_serve(slots, reqs, lookup, width, questions, **kw):
    import torch
    made, built = [], []

    def lookup_slot_loop(pasts, tokens, positions, max_new, k, corpora, **kws):
        built.append(kws)
        loop = _FakePromptLoop(k, width)
        for j, s in enumerate(kws["slot_index"]):
            loop.admit(s, pasts[j], tokens[j], positions[j], max_new[j], kws["params"][j], kws["seeds"][j], kws["histories"][j],
                       kws["stop_ids"][j], corpora[j])
        made.append(loop)
        return loop
    hf = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True, lookup_slot_loop=lookup_slot_loop,
                               lookup_available=lambda: True)
    ge = _engine(hf)
    prefills = []

    def forward(ids, positions, past):
        prefills.append(past.tag)
        logits = torch.zeros((1, len(ids), 64000))
        logits[0, -1, 1000 * past.tag] = 1.0
        return logits, past, 1.0
    ge._forward = forward

    def process(prompt, slot=0, return_full_position_ids=False):
        ids, pos = questions[prompt]
        arena = types.SimpleNamespace(layout=[], B=1, materialize=lambda: None)
        return list(ids), list(pos), 0.0, types.SimpleNamespace(tag=prompt, arena=arena)
    ce = types.SimpleNamespace(process=process, slots=slots, max_ctx_length=4096)
    outs = {}
    for r, o in ge.serve(ce, iter(reqs), None, stream_interval=1, lookup=lookup, **kw):
        outs.setdefault(r, []).append(o)
    return ge, made, built, prefills, outs


def test_serve_prefills_admitted_requests_inside_the_loop():
    from promptcache_amd.generation_engine import GenerationParameters as G
    k = 3
    # tags 1..6; 5 has non-contiguous positions, 6 a question of 1 mod (k + 1) tokens: both take the serial path
    questions = {1: ([11, 12], [50, 51]), 2: ([21], [50]), 3: (list(range(30, 40)), list(range(50, 60))), 4: ([41, 42, 43, 44], [7, 8, 9, 10]),
                 5: ([51, 52, 53], [50, 51, 60]), 6: ([61, 62, 63, 64, 65], [50, 51, 52, 53, 54])}
    max_new = {1: 6, 2: 9, 3: 7, 4: 1, 5: 5, 6: 4}
    reqs = [(t, G(temperature=0.0, max_new_tokens=max_new[t])) for t in (1, 2, 3, 4, 5, 6)]
    ge, made, built, prefills, outs = _fake_serve(2, reqs, k, 4, questions, loop_prefill=True)
    loop = made[0]
    assert len(made) == 1 and built[0]["prompt_rows"] is True
    want = {r: [1000 * t + j for j in range(max_new[t])] for r, t in enumerate((1, 2, 3, 4, 5, 6))}
    assert {r: list(t) for r, t in ge.last_serve_tokens.items()} == want
    # the first fill (1, 2) and the requests the mode does not take (5, 6) were prefilled by a forward of their own
    assert prefills == [1, 2, 5, 6]
    prompts = [c for c in loop.calls if c[0] == "admit_prompt"]
    assert [(c[1], c[2], c[3], c[4], c[5]) for c in prompts] == [(3, list(range(30, 40)), 50, 7, 1), (4, [41, 42, 43, 44], 7, 1, 1)]
    assert all(c[6] == [] for c in prompts)                              # (the corpus in front of the question: the staged ids)
    st = ge.last_serve_stats
    assert st["loop_prefills"] == 2 and st["step_prefills"] == 4 and st["requests"] == 6
    assert st["tokens"] == sum(len(w) - 1 for w in want.values()) + 2    # (the first tokens of 3 and 4 came from the loop)
    for j in range(6):
        assert loop.retired[j] == len(want[j]) - 1, j                    # tokens behind the first, however it was prefilled
    assert loop.closed == {}
    # the first token of request 3 (index 2) came out of the ring: its time to first token is wall time, set at that read
    assert outs[2][0].new_text == "3000" and outs[2][0].elapsed_time > 0.0 and outs[3][0].new_text == "4000"


def test_mode_off_is_todays_serve(monkeypatch):
    from promptcache_amd.generation_engine import GenerationParameters as G
    monkeypatch.delenv("PC_SERVE_LOOP_PREFILL", raising=False)
    questions = {t: ([10 * t, 10 * t + 1], [50, 51]) for t in (1, 2, 3)}
    reqs = [(t, G(temperature=0.0, max_new_tokens=5)) for t in (1, 2, 3)]
    ge, made, built, prefills, _ = _fake_serve(2, reqs, 3, 4, questions)
    assert "prompt_rows" not in built[0] and prefills == [1, 2, 3] and not [c for c in made[0].calls if c[0] == "admit_prompt"]
    assert set(ge.last_serve_stats) == {"replays", "rows", "live_rows", "requests", "tokens", "steps"}
