"""CPU checks of the prompt-lookup reference (tests/lookup_ref.py) on hand-written cases, and of the host pieces of the feature
that need no GPU (the ABI table, the engine's corpus rule)."""
import numpy as np

from tests import lookup_ref as lr


def test_no_match_gives_no_drafts_and_pads_repeat_the_fed_token():
    assert lr.draft([5, 6, 7, 8], 4, 3) == ([8, 8, 8], 0)


def test_a_match_only_at_n_1():
    # suffix (9, 4): "9 4" and "x 9 4" occur nowhere earlier; "4" does, at j = 1 -> followers 7, 9, 4
    assert lr.draft([3, 4, 7, 9, 4], 5, 3) == ([7, 9, 4], 3)
    assert lr.draft([3, 4, 7, 9, 4], 5, 2) == ([7, 9], 2)


def test_of_two_matches_the_later_one_wins():
    h = [1, 2, 3, 50, 1, 2, 3, 60, 61, 1, 2, 3]
    assert lr.draft(h, len(h), 2) == ([60, 61], 2)
    # ... and the longer suffix wins over a later match of a shorter one: "2 3" at j = 6 would give 70
    h = [1, 2, 3, 50, 51, 9, 2, 3, 70, 1, 2, 3]
    assert lr.draft(h, len(h), 2) == ([50, 51], 2)
    assert lr.draft(h, len(h), 2, nmax=2) == ([70, 1], 2)


def test_followers_run_out_before_k():
    h = [7, 8, 9, 1, 7, 8]
    # "7 8" at j = 0 -> followers 9, 1, 7, 8 (4 of them); k = 7 -> 3 pads of the fed token
    assert lr.draft(h, len(h), 7) == ([9, 1, 7, 8, 8, 8, 8], 4)
    h = [4, 4]
    assert lr.draft(h, 2, 3) == ([4, 4, 4], 1)           # one follower: the fed token itself


def test_a_history_of_one_token():
    assert lr.draft([11], 1, 3) == ([11, 11, 11], 0)


def test_self_overlapping_suffix():
    # "a a a" matches at j = 0 (the range excludes the suffix itself, not an overlap with it); one follower
    assert lr.draft([2, 2, 2, 2], 4, 3) == ([2, 2, 2], 1)
    assert lr.draft([2, 2, 2, 2, 2, 2], 6, 2) == ([2, 2], 1)


def test_only_the_first_L_entries_count():
    h = [1, 2, 3, 1, 2, 3, 1, 2]
    assert lr.draft(h, 5, 2) == ([3, 1], 2)              # history 1 2 3 1 2: "1 2" at j = 0


def test_simulate_on_a_periodic_sequence_gives_ceil_counts():
    S = [10, 11, 12, 13, 14] * 8
    corpus, first, T = S[:5], S[5], S[6:30]
    # step 1: only "10" (n = 1) occurs earlier, followers 11 12 13 -> 4 tokens; from then on "x y z" matches one period back
    assert lr.simulate(corpus, first, T, 3) == [4] * 6
    assert lr.simulate(corpus, first, T[:23], 3) == [4] * 5 + [3]
    assert lr.simulate(corpus, first, T, 1) == [2] * 12
    # no corpus, nothing repeats: one token per step
    assert lr.simulate([], 99, list(range(100, 110)), 7) == [1] * 10
    # the period (5) bounds the followers of the most recent match: k = 7 still copies 5 per step
    assert lr.simulate(corpus, first, T, 7)[:3] == [6, 6, 6]


def test_verify_accepts_the_agreeing_prefix_and_never_a_pad():
    V, k = 16, 3

    def logits(am):
        x = np.zeros((len(am), V), dtype=np.float32)
        for i, a in enumerate(am):
            x[i, a] = 1.0
        return x

    def state(ids, nd, budget, ctr=0, L=2):
        return dict(hist=np.array([1, 2] + [0] * 10, dtype=np.int32), hist_len=np.array([L], dtype=np.int32),
                    ids=np.array(ids, dtype=np.int64), pos=np.array([20, 21, 22, 23], dtype=np.int32),
                    past=np.array([30, 0], dtype=np.int32), ndraft=np.array([nd], dtype=np.int32),
                    budget=np.array([budget], dtype=np.int32), ring=np.full((4, k + 2), -1, dtype=np.int32),
                    ctr=np.array([ctr], dtype=np.int32))

    s = lr.verify(logits([5, 6, 7, 8]), state([2, 5, 6, 9], 3, 10), 4)          # two drafts right, the third wrong
    assert list(s["ring"][0]) == [3, 5, 6, 7, -1] and s["ids"][0] == 7 and s["pos"][0] == 23 and s["past"][0] == 33
    assert s["budget"][0] == 7 and s["hist_len"][0] == 5 and list(s["hist"][:5]) == [1, 2, 5, 6, 7] and s["ctr"][0] == 1
    s = lr.verify(logits([5, 2, 2, 2]), state([2, 5, 2, 2], 1, 10), 4)          # ndraft = 1: rows 2, 3 are pads that "agree"
    assert list(s["ring"][0]) == [2, 5, 2, -1, -1]
    s = lr.verify(logits([5, 6, 7, 8]), state([2, 5, 6, 7], 3, 2, ctr=7), 4)    # the budget cuts the step; the ring wraps
    assert list(s["ring"][3]) == [2, 5, 6, -1, -1] and s["budget"][0] == 0 and s["ctr"][0] == 8
    s0 = state([2, 5, 6, 7], 3, 0)
    s = lr.verify(logits([5, 6, 7, 8]), s0, 4)                                  # no budget: an empty record, nothing else
    assert s["ring"][0][0] == 0 and s["ctr"][0] == 1
    for name in ("hist", "hist_len", "ids", "pos", "past", "budget"):
        assert np.array_equal(s[name], s0[name]), name
    x = logits([5])
    x[0, 3] = 1.0                                                               # a tie: the lowest index wins
    assert lr.argmax_rows(x) == [3]


def test_abi_table_carries_the_two_entries():
    from promptcache_amd import _native
    assert "pc_lookup_draft" in _native.SIGNATURES and "pc_lookup_verify" in _native.SIGNATURES
    lib = _native.load()
    assert lib.pc_lookup_draft(None, None, 1, None, None, None, 3, 3, None) == -1001
    assert lib.pc_lookup_verify(None, 16, 16, 1, None, None, None, 1, None, None, None, None, None, None, None, 4, None) == -1001


def test_engine_corpus_is_the_staged_ids_in_row_order_then_the_prompt():
    from promptcache_amd.generation_engine import GenerationEngine

    class Seq:
        def __init__(self, ids):
            self._ids = ids

        def token_ids(self):
            return self._ids

    class Arena:
        layout = [(Seq([1, 2, 3]), 3, "fp16"), (object(), 4, "fp16"), (Seq([7, 8]), 3, "fp16"), (Seq([9]), 1)]

    class Cache:
        arena = Arena()

    # the run without ids and the run whose ids do not cover its rows contribute nothing
    assert GenerationEngine._lookup_corpus(Cache(), [40, 41]) == [1, 2, 3, 9, 40, 41]
    assert GenerationEngine._lookup_corpus(None, [40]) == [40]
