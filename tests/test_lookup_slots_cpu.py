"""Host-side checks of the batched prompt-lookup step: tests/lookup_slots_ref.py against tests/lookup_ref.py, the stop-id and
arena-room rules, and the fallbacks of ``LlamaHIP.lookup_slot_loop`` / ``GenerationEngine.generate_batch(lookup=k)`` that need no GPU."""
import types

import numpy as np
import pytest

from tests import lookup_ref as lr
from tests import lookup_slots_ref as ref

RING_CAP = 4


def _state(S, k, hist_rows, cap=200, length=50, budget=40):
    hc = 64
    st = dict(hist=np.zeros((S, hc), dtype=np.int32), hist_len=np.zeros(S, dtype=np.int32), ids=np.full((S, k + 1), -7, dtype=np.int64),
              pos=np.full((S, k + 1), -9, dtype=np.int32), ndraft=np.full(S, -1, dtype=np.int32),
              budget=np.full(S, budget, dtype=np.int32), stop_ids=np.full((S, 8), -1, dtype=np.int32),
              ring=np.full((S, RING_CAP, k + 2), -5, dtype=np.int32), ctr=np.arange(S, dtype=np.int32) + 2,
              len=np.full(S, length, dtype=np.int32), cap=np.full(S, cap, dtype=np.int32), live=np.ones(S, dtype=np.int32))
    for b, h in enumerate(hist_rows):
        st["hist"][b, :len(h)] = h
        st["hist_len"][b] = len(h)
        st["ids"][b, 0] = h[-1]
        st["pos"][b, 0] = 100 + b
    return st


def _logits(am, V=64):
    x = np.zeros((len(am), V), dtype=np.float32)
    for i, a in enumerate(am):
        x[i, a] = 10.0
    return x


@pytest.mark.parametrize("k", [1, 3, 7])
def test_one_slot_is_the_b1_reference(k):
    rng = np.random.default_rng(k)
    for trial in range(20):
        h = rng.integers(0, 4, size=int(rng.integers(2, 40))).tolist()
        st = _state(1, k, [h], budget=int(rng.integers(0, 6)))
        d = ref.draft_slots(st, k)
        ids, pos, m = lr.draft_state(st["hist"][0], st["hist_len"][0], st["ids"][0], st["pos"][0], k)
        assert np.array_equal(d["ids"][0], ids) and np.array_equal(d["pos"][0], pos) and d["ndraft"][0] == m
        am = [int(ids[1 + i]) if i < trial % (k + 1) else 60 - i for i in range(k + 1)]
        x = _logits(am)
        got, a = ref.verify_slots(x, d, k, RING_CAP)
        one = dict(hist=d["hist"][0], hist_len=d["hist_len"], ids=d["ids"][0], pos=d["pos"][0], past=np.array([d["len"][0], 0], np.int32),
                   ndraft=d["ndraft"], budget=d["budget"], ring=d["ring"][0], ctr=d["ctr"])
        want = lr.verify(x, one, RING_CAP)
        assert a.tolist() == am
        for name in ("hist_len", "ndraft", "budget", "ctr"):
            assert np.array_equal(got[name], want[name]), name
        assert np.array_equal(got["hist"][0], want["hist"]) and np.array_equal(got["ids"][0], want["ids"])
        assert np.array_equal(got["pos"][0], want["pos"]) and np.array_equal(got["ring"][0], want["ring"])
        assert got["len"][0] == want["past"][0]
        assert got["live"][0] == (1 if got["budget"][0] > 0 else 0)


def test_a_stop_id_inside_an_accepted_run_cuts_the_record_and_clears_live():
    k = 7
    h = list(range(10, 22)) + [10, 11]                     # suffix 10 11 -> drafts 12 13 14 15 16 17 18
    st = ref.draft_slots(_state(2, k, [h, h]), k)
    assert st["ndraft"].tolist() == [k, k] and st["ids"][0, 1:].tolist() == list(range(12, 19))
    st["stop_ids"][0, 5] = 14                              # slot 0 only
    am = list(range(12, 19)) + [40]                        # the model agrees with every draft, then says 40
    got, _ = ref.verify_slots(_logits(am + am), st, k, RING_CAP)
    r0, r1 = got["ring"][0, 2], got["ring"][1, 3]
    assert r0[:4].tolist() == [3, 12, 13, 14] and got["live"][0] == 0 and got["len"][0] == 53 and got["budget"][0] == 37
    assert got["ids"][0, 0] == 14 and got["pos"][0, 0] == 103 and got["hist_len"][0] == len(h) + 3
    assert r1.tolist() == [8] + am and got["live"][1] == 1 and got["len"][1] == 58
    # the next step: slot 0 is idle -- an empty record, nothing else
    nxt, _ = ref.verify_slots(_logits(am + am), ref.draft_slots(got, k), k, RING_CAP)
    assert nxt["ring"][0, 3, 0] == 0 and nxt["ctr"][0] == got["ctr"][0] + 1
    for name in ("hist", "hist_len", "ids", "pos", "len", "budget", "ndraft"):
        assert np.array_equal(nxt[name][0], got[name][0]), name


def test_a_slot_without_room_for_a_steps_rows_is_skipped_and_switched_off():
    k = 3
    h = [5, 6, 7, 5, 6]
    st = _state(2, k, [h, h], cap=53, length=50)           # 50 + 4 > 53
    st["cap"][1] = 54                                      # slot 1 fits exactly
    d = ref.draft_slots(st, k)
    assert d["ndraft"].tolist() == [-1, 3] and np.array_equal(d["ids"][0], st["ids"][0])
    got, _ = ref.verify_slots(_logits([7, 5, 6, 9] * 2), d, k, RING_CAP)
    assert got["live"].tolist() == [0, 0] and got["ring"][0, 2, 0] == 0 and got["len"][0] == 50 and got["budget"][0] == 40
    assert got["ring"][1, 3].tolist() == [4, 7, 5, 6, 9] and got["len"][1] == 54       # emitted, then no room for another step: off


def test_verify_attend_is_causal_inside_the_draft_rows():
    rng = np.random.default_rng(3)
    k, H, Hkv, D, m = 3, 4, 2, 16, 9
    q = rng.standard_normal((k + 1, H, D))
    K, V = rng.standard_normal((Hkv, m + k + 2, D)), rng.standard_normal((Hkv, m + k + 2, D))
    a = ref.verify_attend(q, K, V, m, k)
    K2, V2 = K.copy(), V.copy()
    K2[:, m + 2:], V2[:, m + 2:] = 1e4, 1e4                # rows 0 and 1 see keys [0, m] and [0, m + 1] only
    b = ref.verify_attend(q, K2, V2, m, k)
    assert np.array_equal(a[:2], b[:2]) and not np.allclose(a[2:], b[2:])
    one = ref.verify_attend(q[:1], K, V, m, 0)
    assert np.allclose(one[0], a[0], atol=1e-12)


def test_simulate_slots_is_simulate_per_sequence_and_stops_at_a_stop_id():
    T = [3, 4, 5, 6, 3, 4, 5, 6, 9, 9, 2, 1]
    corp = [[], [3, 4, 5, 6, 3, 4, 5, 6, 9], [3, 4, 0]]
    steps = ref.simulate_slots(corp, [7, 7, 7], [T, T, T], 3)
    for j, c in enumerate(corp):
        assert [s[j] for s in steps if s[j]] == lr.simulate(c, 7, T, 3), j
    assert len(lr.simulate(corp[1], 7, T, 3)) < len(T)
    cut = ref.simulate_slots(corp[:2], [7, 7], [T, T], 3, stop_ids=[9])
    assert all(sum(s[j] for s in cut) == T.index(9) + 1 for j in range(2))


# ---- fallbacks that need no GPU ---------------------------------------------------------------------------------------------
def test_lookup_slot_loop_refuses_more_than_64_rows_and_models_without_the_step():
    from promptcache_amd.model.llama_hip import LlamaHIP
    m = object.__new__(LlamaHIP)
    m.slot_loop_available = lambda: True
    m.lookup_available = lambda: True
    pasts = [object()] * 8
    assert m.lookup_slot_loop(pasts, [1] * 8, [5] * 8, 10, 8, [[]] * 8) is None          # 8 x 9 rows
    assert m.lookup_slot_loop(pasts[:5], [1] * 5, [5] * 5, 10, 8, [[]] * 5) is None      # 5 sequences take 8 slots: 8 x 9 rows
    assert m.lookup_slot_loop(pasts[:3], [1] * 3, [5] * 3, 10, 15, [[]] * 3, slots=8) is None
    assert m.lookup_slot_loop(pasts[:2], [1] * 2, [5] * 2, 10, 0, [[]] * 2) is None
    m.lookup_available = lambda: False
    assert m.lookup_slot_loop(pasts[:1], [1], [5], 10, 3, [[]]) is None


class _FakeHF:
    """A model with the batched loop's interface whose lookup loop is unavailable: counts what generate_batch asks for."""

    def __init__(self, with_lookup):
        self.asked = []
        if with_lookup:
            self.lookup_slot_loop = self._lookup

    def slot_loop_available(self):
        return True

    def _lookup(self, *a, **kw):
        self.asked.append("lookup")
        return None

    def slot_loop(self, *a, **kw):
        self.asked.append("slots")
        return None


def _fake_engine(with_lookup=True):
    import torch
    from promptcache_amd.generation_engine import GenerationEngine
    hf = _FakeHF(with_lookup)
    lm = types.SimpleNamespace(hf_model=hf, use_full_position_ids=False, decode=lambda ids: " ".join(map(str, ids)), device="cpu")
    ge = GenerationEngine(lm, lookup=7)

    def forward(ids, positions, past):                     # (the real one times the call with device events)
        logits = torch.zeros((1, len(ids), 16))
        logits[0, -1, 5] = 1.0
        return logits, past, 0.0
    ge._forward = forward
    return ge, hf


def _requests(n):
    arena = lambda: types.SimpleNamespace(B=1, layout=[])
    return [([1, 2, 3], [0, 1, 2], types.SimpleNamespace(arena=arena())) for _ in range(n)]


def test_generate_batch_rejects_lookup_with_share_trunk():
    from promptcache_amd.generation_engine import GenerationParameters
    ge, hf = _fake_engine()
    params = GenerationParameters(temperature=0.0, max_new_tokens=4)
    with pytest.raises(ValueError):
        next(ge.generate_batch(_requests(2), params, lookup=3, share_trunk=True))
    assert hf.asked == []


def test_generate_batch_falls_back_to_the_slot_loop(monkeypatch):
    """A refused lookup loop (no library, too many rows, no lookup step) and sampled params lead to today's ``slot_loop`` call; with
    lookup off -- the default, whatever the engine-level ``lookup`` says -- the lookup loop is not even asked for."""
    from promptcache_amd.generation_engine import GenerationParameters
    greedy = GenerationParameters(temperature=0.0, max_new_tokens=4)
    sampled = GenerationParameters(temperature=0.8, top_p=0.9, max_new_tokens=4)
    monkeypatch.delenv("PC_SLOT_LOOKUP", raising=False)

    def asked(params, with_lookup=True, **kw):
        ge, hf = _fake_engine(with_lookup)
        if not params.greedy:
            hf.sample_token = lambda *a: 5
        with pytest.raises(RuntimeError, match="refused a batched decode loop"):       # (the fake's slot_loop gives None too)
            list(ge.generate_batch(_requests(2), params, **kw))
        return hf.asked

    assert asked(greedy, lookup=3) == ["lookup", "slots"]
    assert asked(greedy, with_lookup=False, lookup=3) == ["slots"]
    assert asked(sampled, lookup=3) == ["slots"]
    assert asked(greedy) == ["slots"]                                            # engine lookup=7 is not consulted
    assert asked(greedy, lookup=0) == ["slots"]
    monkeypatch.setenv("PC_SLOT_LOOKUP", "3")
    assert asked(greedy) == ["lookup", "slots"]
