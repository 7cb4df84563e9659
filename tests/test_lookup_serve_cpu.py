"""Prompt-lookup drafts under continuous batching, the parts that need no GPU: the per-slot verify rule (tests/lookup_serve_ref.py,
the restatement of pc_lookup_verify_slots_each) in a toy-model simulation of continuous admission against the one-token sampled
generation of every request, the C-ABI of the two new entries, the layout of their structs, the history a sequence is admitted
with, ``serve_plan(lookup)``'s decision table and ``serve(lookup=k)`` over a scripted lookup loop."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import lookup_sample_ref as lsr
from tests import lookup_serve_ref as ref
from tests.test_lookup_sample_cpu import PREFIX, V, toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pc_lookup_verify_slots_each", "pc_lookup_slot_arm")
TOY = [(0.0, 1.0, 1.0, 0), (0.7, 1.3, 0.9, 4), (1.0, 1.0, 1.0, 0), (0.0, 1.2, 1.0, 0)]     # plain greedy, a chain, T = 1, greedy + penalty
MAX_NEW = [5, 12, 20, 9, 16, 7, 11]
HIST_CAP = 48


# ---- the rule: continuous admission on a toy model -------------------------------------------------------------------------------
def _requests(k):
    """7 requests: mixed parameter sets, budgets that cut a step in the middle (every draft of an "answer" corpus is right, so a
    step would yield k + 1 tokens), stop ids inside accepted runs (requests 1 and 4), a corpus longer than the history buffer
    (request 5: its oldest ids are dropped) and one with nothing to copy (request 2)."""
    reqs, want = [], []
    for r, max_new in enumerate(MAX_NEW):
        p, seed = TOY[r % 4], 4000 + r
        prefix = PREFIX[r % 5:] + PREFIX[:r % 5]
        first = int(np.random.default_rng(r).integers(0, V))
        T = lsr.sequential(toy_model, prefix, first, max_new, p, seed, prefix + [first])
        stops = [T[5]] if r in (1, 4) else []
        cut = next((i + 1 for i, t in enumerate(T) if t in stops), len(T))
        rng = np.random.default_rng(100 + r)
        corpus = {2: [], 5: rng.integers(0, V, 60).tolist() + [first] + T}.get(r, [first] + T)
        reqs.append(dict(prefix=prefix, first=first, corpus=corpus, max_new=max_new, params=p, seed=seed, history_ids=prefix + [first],
                         stop_ids=stops))
        want.append(T[:cut])
    return reqs, want


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_continuous_admission_is_the_one_token_generation_of_every_request(S, k):
    reqs, want = _requests(k)
    steps, end, replays = ref.simulate_serve(toy_model, reqs, S, k, HIST_CAP)
    total = 0
    for r, q in enumerate(reqs):
        got = [t for s in steps[r] for t in s]
        assert got == want[r], (S, k, r)
        assert all(len(s) <= k + 1 for s in steps[r]) and all(len(s) >= 1 for s in steps[r][:-1])
        assert end[r]["draws"] == 1 + len(got), (S, k, r)
        assert np.array_equal(end[r]["bits"], lsr.history_bits(q["history_ids"] + got, V)), (S, k, r)
        total += len(got)
    # conditions on the input: a stop id cut an accepted run behind its first token, a budget cut a step, steps were saved
    if k >= 3:
        assert len(steps[1][-1]) >= 2 or len(steps[4][-1]) >= 2
        assert any(len(want[r]) == MAX_NEW[r] and 1 <= len(steps[r][-1]) < k + 1 and len(steps[r]) > 1 for r in (0, 3, 6))
    assert replays < total


def test_a_stop_id_in_the_middle_of_an_accepted_run_and_an_idle_slot():
    """A made case: slot 0 accepts three drafts, the second emitted token is a stop id; slot 1 is idle; slot 2 has no room."""
    S, k, Vv = 3, 3, 12
    st = ref.new_state(S, k, Vv, 16, 2)
    for b in range(S):
        ref.arm(st, b, k, Vv, [1, 2], 10, 20, 100, 9, 4, [1, 2], [])
    st["live"][1], st["cap"][2] = 0, 23                               # slot 2: 20 + 4 > 23
    st["ids"][0, 1:], st["ndraft"][0] = [5, 6, 7], 3
    st["stop_ids"][0, 3] = 6
    logits = np.zeros((S * 4, Vv), dtype=np.float32)
    for i, t in enumerate((5, 6, 7, 8)):
        logits[i, t] = 9.0
    new, infos = ref.verify_slots_each(logits, st, k, 2, [ref.GREEDY] * S, [0] * S)
    assert infos[0]["acc"] == 3 and infos[0]["emit"] == 2 and infos[1] is None and infos[2] is None
    assert new["ring"][0, 0].tolist() == [2, 5, 6, 0, 0] and new["live"].tolist() == [0, 0, 0]
    assert int(new["draws"][0]) == 3 and int(new["len"][0]) == 22 and int(new["budget"][0]) == 7 and int(new["ids"][0, 0]) == 6
    assert lsr.bits_ids(new["bits"][0], Vv) == [1, 2, 5, 6] and new["hist"][0, :4].tolist() == [1, 2, 5, 6]
    assert new["ctr"].tolist() == [5, 5, 5] and int(new["ring"][1, 0, 0]) == 0 and int(new["ring"][2, 0, 0]) == 0
    for w in ("hist", "hist_len", "ids", "pos", "len", "budget", "bits", "draws"):
        assert np.array_equal(new[w][1:], st[w][1:]), w              # a slot that does not run keeps every other word


def test_each_case_seeds_leave_three_quarters_comparable():
    """The condition tests/test_gpu_lookup_serve.py relies on, met by the reference alone: at least 3/4 of the live sampled (slot,
    row) pairs of the mixed case have a float64 score margin above 1e-4."""
    for Vv in ref.EACH_RNG_SEED:
        m = ref.each_reference_margins(Vv)
        assert len(m) == 18 and 4 * sum(x > ref.MARGIN for x in m) >= 3 * len(m), (Vv, sorted(m)[:6])


# ---- admission: the history --------------------------------------------------------------------------------------------------
def test_admission_drops_the_oldest_corpus_ids_and_refuses_a_budget_that_cannot_fit():
    from promptcache_amd.model.llama_hip import lookup_admit_history
    for fit in (ref.fit_history, lookup_admit_history):
        assert fit([1, 2, 3], 9, 4, 16) == [1, 2, 3, 9]
        assert fit(list(range(20)), 9, 4, 16) == list(range(9, 20)) + [9]           # 11 corpus ids + the token + 4 new = 16
        assert fit(list(range(20)), 9, 15, 16) == [9] and fit([], 9, 15, 16) == [9]
        with pytest.raises(ValueError):
            fit([1], 9, 16, 16)
    rng = np.random.default_rng(0)
    for _ in range(200):
        c, mn, cap = rng.integers(0, 50, int(rng.integers(0, 40))).tolist(), int(rng.integers(1, 20)), int(rng.integers(21, 40))
        h = lookup_admit_history(c, 7, mn, cap)
        assert h == ref.fit_history(c, 7, mn, cap) and len(h) + mn <= cap and h[-1] == 7 and (c + [7])[-len(h):] == h


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    from promptcache_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "promptcache_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.lib_path())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _native.SIGNATURES, name


def test_lookup_slot_arm_structs_match_the_header(tmp_path):
    """The method of test_abi_symbols.test_struct_layouts_match_the_header for the two structs of pc_lookup_slot_arm."""
    import subprocess
    from promptcache_amd import _native
    structs = (("pc_lookup_slot_arm_block", _native.LookupSlotArmBlock), ("pc_lookup_slot_state", _native.LookupSlotState))
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {']
    for st, cls in structs:
        body.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        body += [f'  printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    body += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    for st, cls in structs:
        assert int(got[st]) == ctypes.sizeof(cls) and ctypes.sizeof(cls) % 8 == 0, st
        for name, _ in cls._fields_:
            assert int(got[f"{st}.{name}"]) == getattr(cls, name).offset, (st, name)


def test_entries_reject_bad_arguments_without_a_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)

    def verify(S=4, k=3, V=1001, ldl=1001, logits=p, params=p, ring_cap=16, hist_cap=64):
        return lib.pc_lookup_verify_slots_each(logits, ldl, V, S, k, params, p, p, p, p, p, p, p, hist_cap, p, p, p, p, p, p, p, p, p, p,
                                               ring_cap, None)
    for bad in (dict(S=0), dict(S=17), dict(k=0), dict(k=16), dict(S=8, k=8), dict(V=0), dict(V=1 << 24, ldl=1 << 24), dict(ldl=1000),
                dict(logits=p + 2), dict(params=p + 4), dict(ring_cap=0), dict(hist_cap=0), dict(logits=None)):
        assert verify(**bad) == -1001, bad
        assert b"pc_lookup_verify_slots_each" in lib.pc_last_error_string()
    state = _native.LookupSlotState(*([p] * len(_native.LookupSlotState._fields_)))
    hw = 32

    def arm(S=4, k=3, hist_cap=64, slot=1, words=hw, hist_len=5, nbytes=None, pad=0, st=state):
        raw = (ctypes.c_uint64 * 64)()
        b = _native.LookupSlotArmBlock.from_address(ctypes.addressof(raw) + pad)
        b.slot, b.hist_words, b.hist_len = slot, words, hist_len
        nb = _native.lookup_slot_arm_bytes(words, max(hist_len, 0)) if nbytes is None else nbytes
        return lib.pc_lookup_slot_arm(ctypes.addressof(raw) + pad, nb, ctypes.byref(st), S, k, hist_cap, None)
    null = _native.LookupSlotState(*([p] * 17 + [None]))
    for bad in (dict(S=0), dict(S=17), dict(k=0), dict(S=8, k=8), dict(hist_cap=0), dict(slot=-1), dict(slot=4), dict(words=0),
                dict(hist_len=0), dict(hist_len=65), dict(nbytes=8), dict(pad=4), dict(st=null)):
        assert arm(**bad) == -1001, bad
        assert b"pc_lookup_slot_arm" in lib.pc_last_error_string()
    assert lib.pc_lookup_slot_arm(None, 8, ctypes.byref(state), 4, 3, 64, None) == -1001
    assert _native.lookup_slot_arm_bytes(3, 5) == ctypes.sizeof(_native.LookupSlotArmBlock) + 16 + 24


# ---- serve_plan(lookup) and serve(lookup=k) over a scripted model -----------------------------------------------------------------
def _engine(hf):
    from promptcache_amd.generation_engine import GenerationEngine
    lm = types.SimpleNamespace(hf_model=hf, use_full_position_ids=False, decode=lambda ids: " ".join(map(str, ids)), device="cpu")
    ge = GenerationEngine(lm)
    ge.device_greedy_loop = ge.device_sample_loop = True
    return ge


def test_serve_plan_says_which_form_runs():
    full = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True, lookup_slot_loop=None, lookup_available=lambda: True)
    plain = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True)
    no_step = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True, lookup_slot_loop=None, lookup_available=lambda: False)
    assert _engine(full).serve_plan() == _engine(full).serve_plan(0) and _engine(full).serve_plan()[0]
    ok, why = _engine(full).serve_plan(3, slots=4)
    assert ok and "lookup" in why and "k = 3" in why
    ok, why = _engine(full).serve_plan(40, slots=4)
    assert ok and "k = 15" in why                                       # k above 15 is taken as 15
    for ge, S, word in ((_engine(plain), 4, "no lookup step"), (_engine(no_step), 4, "no lookup step"), (_engine(full), 16, "64")):
        ok, why = ge.serve_plan(7, slots=S)
        assert ok and "one token per replay" in why and word in why, why
    assert not _engine(None).serve_plan(3, slots=4)[0]


class _FakeLookupLoop:
    """``LookupSlotLoop(each=True)``'s protocol on the host: sequence j's tokens are ``1000 * tag + 1, + 2, ...``, ``width`` per
    replay (the drafts are always right), until its budget or a stop id."""

    def __init__(self, k, width):
        self.k, self.width, self.n, self.nsplit_trunk = k, width, 0, 0
        self._start, self._max_new, self._stops, self._tag, self._killed, self.idx, self.corpora = [], [], [], [], [], [], []
        self.retired, self.closed = {}, None

    def enqueue(self):
        self.n += 1
        return self.n - 1

    def elapsed_ms(self, i):
        assert i < self.n
        return 1.0

    def tokens(self, j, i):
        assert i < self.n, "the host asked for a replay it never enqueued"
        s = i - self._start[j]
        if s < 0 or (self._killed[j] is not None and i >= self._killed[j]):
            return []
        out = []
        for t in range(s * self.width, min((s + 1) * self.width, self._max_new[j])):
            if any(1000 * self._tag[j] + u + 1 in self._stops[j] for u in range(t)):
                break
            out.append(1000 * self._tag[j] + t + 1)
        return out

    def kill(self, j):
        self._killed[j] = self.n

    def admit(self, slot, past, token, position, max_new, params, seed, history, stop_ids, corpus, trunk=None):
        assert not [j for j in range(len(self._tag)) if self.idx[j] == slot and j not in self.retired], "the slot's sequence was not retired"
        self._start.append(self.n); self._max_new.append(max_new); self._stops.append(set(stop_ids)); self._tag.append(past.tag)
        self._killed.append(None); self.idx.append(slot); self.corpora.append(list(corpus))
        return len(self._tag) - 1

    def retire(self, j, consumed):
        self.retired[j] = consumed

    def close(self, consumed):
        self.closed = dict(consumed)


def _fake_serve(slots, reqs, lookup, width, stream_interval=1, abandon_after=None):
    import torch
    made = []

    def lookup_slot_loop(pasts, tokens, positions, max_new, k, corpora, **kw):
        assert kw["each"] and kw["max_keys"] == 4096 and kw["slots"] == slots and len(kw["params"]) == len(pasts)
        loop = _FakeLookupLoop(k, width)
        for j, s in enumerate(kw["slot_index"]):
            loop.admit(s, pasts[j], tokens[j], positions[j], max_new[j], kw["params"][j], kw["seeds"][j], kw["histories"][j],
                       kw["stop_ids"][j], corpora[j])
        made.append(loop)
        return loop

    def slot_loop(*a, **kw):
        raise AssertionError("serve(lookup=k) built the one-token loop")
    hf = types.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True, lookup_slot_loop=lookup_slot_loop,
                               lookup_available=lambda: True)
    ge = _engine(hf)

    def forward(ids, positions, past):
        logits = torch.zeros((1, len(ids), 8000))
        logits[0, -1, 1000 * past.tag] = 1.0
        return logits, past, 1.0
    ge._forward = forward

    def process(prompt, slot=0, return_full_position_ids=False):
        return [prompt], [10 + prompt], 0.0, types.SimpleNamespace(tag=prompt, arena=types.SimpleNamespace(layout=[], B=1))
    ce = types.SimpleNamespace(process=process, slots=slots, max_ctx_length=4096)
    outs = {}
    gen = ge.serve(ce, iter(reqs), None, stream_interval=stream_interval, lookup=lookup)
    for n, (r, o) in enumerate(gen):
        outs.setdefault(r, []).append(o)
        if abandon_after is not None and n + 1 >= abandon_after:
            gen.close()
            break
    return ge, made, outs


def test_serve_with_lookup_reads_several_tokens_per_replay_and_retires_with_tokens():
    from promptcache_amd.generation_engine import GenerationParameters as G
    max_new = [6, 13, 9, 4, 11]
    reqs = [(r + 1, G(temperature=0.0, max_new_tokens=mn, stop_token_ids=[3005] if r == 2 else [])) for r, mn in enumerate(max_new)]
    ge, made, outs = _fake_serve(2, reqs, 3, 4)
    loop = made[0]
    assert len(made) == 1 and loop.k == 3
    toks = ge.last_serve_tokens
    want = {r: [1000 * (r + 1) + j for j in range(mn)] for r, mn in enumerate(max_new)}
    want[2] = want[2][:6]                                                # 3000 .. 3005: the stop id, inside a replay's tokens
    assert {r: list(t) for r, t in toks.items()} == want
    for j in range(5):                                                   # retired with the TOKENS the loop gave, not the replays
        assert loop.retired[j] == len(want[j]) - 1, j
    assert loop.corpora[0] == [1] and loop.closed == {}
    st = ge.last_serve_stats
    assert st["tokens"] == sum(len(w) - 1 for w in want.values()) and st["steps"] == st["replays"] == loop.n and st["steps"] < st["tokens"]
    assert [o.new_text for o in outs[3]][-1] == " ".join(map(str, want[3]))
    # the look-ahead rule: a replay is enqueued ahead only while the step in flight cannot exhaust a budget (room > k + 1), so a
    # single short sequence never costs a replay behind its last token
    ge1, made1, _ = _fake_serve(2, [(1, G(temperature=0.0, max_new_tokens=9))], 3, 4)
    assert made1[0].n == 2                                              # 8 tokens in the loop, 4 per replay
    # abandoned: close() gets the tokens consumed so far of the sequences still running
    ge2, made2, _ = _fake_serve(2, [(1, G(temperature=0.0, max_new_tokens=30)), (2, G(temperature=0.0, max_new_tokens=30))], 3, 4, abandon_after=8)
    assert made2[0].closed == {0: 4, 1: 4} and made2[0].retired == {}      # (two first tokens, then replay 0's tokens of both)


def test_serve_without_lookup_and_with_too_many_rows_builds_todays_loop():
    from promptcache_amd.generation_engine import GenerationParameters as G
    from tests.test_serve_cpu import _FakeLoop
    made = []

    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, slots=None, slot_index=None, each=False,
                  max_keys=None, trunks=None):
        made.append(_FakeLoop([p.tag for p in pasts], max_new, stop_ids, slot_index))
        return made[-1]

    def lookup_slot_loop(*a, **kw):
        raise AssertionError("the lookup loop was built")
    hf = types.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True, lookup_slot_loop=lookup_slot_loop,
                               lookup_available=lambda: True)
    import torch
    for slots, lookup in ((2, 0), (2, None), (16, 7)):
        ge = _engine(hf)

        def forward(ids, positions, past):
            logits = torch.zeros((1, len(ids), 8000))
            logits[0, -1, 1000 * past.tag] = 1.0
            return logits, past, 1.0
        ge._forward = forward
        ce = types.SimpleNamespace(process=lambda prompt, slot=0: ([prompt], [10 + prompt], 0.0, types.SimpleNamespace(tag=prompt)),
                                   slots=slots, max_ctx_length=4096)
        reqs = [(r + 1, G(temperature=0.0, max_new_tokens=5)) for r in range(3)]
        list(ge.serve(ce, reqs, lookup=lookup))
        assert {r: list(t) for r, t in ge.last_serve_tokens.items()} == {r: [1000 * (r + 1) + j for j in range(5)] for r in range(3)}
        assert sorted(ge.last_serve_stats) == ["live_rows", "replays", "requests", "rows"]
