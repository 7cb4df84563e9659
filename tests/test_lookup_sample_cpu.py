"""The sampled prompt-lookup rule (tests/lookup_sample_ref.py, the restatement of pc_lookup_verify_sample) on the CPU: a
speculative generation is the one-token sampled generation token for token, whatever the drafts were, and the state words keep
their books."""
import numpy as np
import pytest

from tests import lookup_sample_ref as lsr

V, N_NEW, SEEDS = 12, 40, 50
PARAMS = {"T1": (1.0, 1.0, 1.0, 0), "chain": (0.7, 1.3, 0.9, 4), "greedy_rp": (0.0, 1.2, 1.0, 0)}
PREFIX = [3, 1, 4, 1, 5]
_TABLE = np.random.default_rng(2024).normal(0.0, 2.0, size=(V, V, V, V)).astype(np.float32)


def toy_model(seq):
    """Logits: a fixed pseudo-random function of the last 3 tokens."""
    a, b, c = (int(t) for t in seq[-3:])
    return _TABLE[a, b, c]


def _first(seed):
    return int(np.random.default_rng(seed).integers(0, V))


@pytest.fixture(scope="module")
def answers():
    """(parameter set, seed) -> (first token, the one-token sampled generation of N_NEW tokens)."""
    out = {}
    for name, p in PARAMS.items():
        for seed in range(SEEDS):
            first = _first(seed)
            out[name, seed] = (first, lsr.sequential(toy_model, PREFIX, first, N_NEW, p, 1000 + seed, PREFIX + [first]))
    return out


def _corpora(first, T, seed):
    rng = np.random.default_rng(7 * seed + 1)
    changed = [first] + list(T)
    for j in (1 + 9, 1 + 23):
        changed[j] = (changed[j] + 1 + int(rng.integers(0, V - 1))) % V
    return {"empty": [], "answer": [first] + list(T), "changed": changed, "random": rng.integers(0, V, size=60).tolist()}


@pytest.mark.parametrize("name", list(PARAMS))
def test_speculative_generation_is_the_one_token_generation(answers, name):
    p = PARAMS[name]
    saved = 0
    for seed in range(SEEDS):
        first, T = answers[name, seed]
        ks = (1, 3, 7, 15) if seed < 4 else ((1, 3, 7, 15)[seed & 3],)    # every k on 4 seeds, one k in turn on the rest
        for cname, corpus in _corpora(first, T, seed).items():
            for k in ks:
                # budgets that cut a step in the middle: three on 4 seeds, a second one where whole steps are accepted on the rest
                for max_new in ((N_NEW, N_NEW - 3, 5) if seed < 4 else (N_NEW, 11 + seed % 7) if cname == "answer" else (N_NEW,)):
                    steps, st, _ = lsr.simulate(toy_model, PREFIX, first, corpus, k, max_new, p, 1000 + seed, PREFIX + [first])
                    got = [t for s in steps for t in s]
                    assert got == T[:max_new], (name, seed, cname, k, max_new)
                    assert all(1 <= len(s) <= k + 1 for s in steps)
                    if cname == "answer" and max_new == N_NEW:
                        # (a condition on the input: with the answer to copy from, steps must be saved)
                        assert len(steps) < N_NEW, (name, seed, k)
                        saved += N_NEW - len(steps)
    assert saved > 0


@pytest.mark.parametrize("name", list(PARAMS))
def test_state_bookkeeping(answers, name):
    p = PARAMS[name]
    for seed in (0, 1, 2):
        first, T = answers[name, seed]
        hist_ids = PREFIX + [first]
        for k in (3, 7):
            max_new = 17
            steps, st, states = lsr.simulate(toy_model, PREFIX, first, [first] + T, k, max_new, p, 1000 + seed, hist_ids, surplus=3)
            emitted = [t for s in steps for t in s]
            assert emitted == T[:max_new] and [len(s) for s in steps[-3:]] == [0, 0, 0]
            assert int(st["draws"][0]) == 1 + len(emitted)
            assert np.array_equal(st["bits"], lsr.history_bits(hist_ids + emitted, V))
            assert int(st["budget"][0]) == 0 and int(st["past"][0]) == len(PREFIX) + max_new
            assert int(st["hist_len"][0]) == 1 + len(T) + 1 + max_new
            # surplus steps: nothing but the empty record (and the draft stage's rows 1..k, which the verify stage does not own)
            last = states[-4]
            for a in states[-3:]:
                for w in ("hist", "hist_len", "past", "budget", "bits", "draws"):
                    assert np.array_equal(a[w], last[w]), w
                assert int(a["ids"][0]) == int(last["ids"][0]) and int(a["pos"][0]) == int(last["pos"][0])
            assert int(st["ctr"][0]) == len(steps)
            assert int(st["ring"].reshape(4, k + 2)[(len(steps) - 1) % 4][0]) == 0


def test_a_draft_changes_the_next_rows_history():
    """The rule's one subtlety, on a made case: row 1 is drawn under the penalty of draft 1, as the one-token loop would."""
    rows = np.zeros((2, V), dtype=np.float32)
    rows[0, 5] = 9.0                       # row 0 draws 5 (greedy)
    rows[1, 5], rows[1, 2] = 4.0, 3.0      # row 1: 5 leads, unless 5 is penalised (4.0 / 2.0 < 3.0)
    st = dict(hist=np.zeros(8, dtype=np.int32), hist_len=np.array([1], dtype=np.int32), ids=np.array([0, 5], dtype=np.int64),
              pos=np.array([10, 11], dtype=np.int32), past=np.array([10, 0], dtype=np.int32), ndraft=np.array([1], dtype=np.int32),
              budget=np.array([9], dtype=np.int32), ring=np.zeros((4, 3), dtype=np.int32), ctr=np.zeros(1, dtype=np.int32),
              bits=lsr.history_bits([0], V), draws=np.ones(1, dtype=np.int32))
    new, info = lsr.verify_sample(rows, st, 4, (0.0, 2.0, 1.0, 0), 0)
    assert info["tokens"] == [5, 2] and info["acc"] == 1 and info["emit"] == 2
    assert new["ring"][0].tolist() == [2, 5, 2] and int(new["draws"][0]) == 3
    assert lsr.bits_ids(new["bits"], V) == [0, 2, 5]
