"""Forced rows on the GPU, no model: pc_lookup_draft_slots_prompt / pc_lookup_verify_slots_prompt word for word
against tests/loop_prefill_ref.py over a question's steps with a decoding and an idle neighbour, against the existing entries with
no forced rows, pc_lookup_slot_arm_prompt word for word with guards behind every array, and argument errors that leave the outputs
alone."""
import gc

import numpy as np
import pytest
import torch

from tests import lookup_sample_ref as lsr
from tests import lookup_serve_ref as lsv
from tests import loop_prefill_ref as ref
from tests.test_gpu_lookup_serve import SLOT_WORDS, _each_words, _pinned, _sentinel_state, _verify_each
from tests.test_gpu_slots import _n

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORDS = SLOT_WORDS + ("draws", "forced")


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The caching allocator hands this module's blocks back when it ends: tests that count ``torch.cuda.memory_allocated``
    see an unsplit remainder of a cached block of another module's size as bytes nobody owns."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _draft_prompt(n, d, k, nmax=3):
    S = d["ids"].shape[0]
    n.lookup_draft_slots_prompt(d["hist"], d["hist_len"], d["ids"], d["pos"], d["ndraft"], d["cap"], d["len"], d["live"], d["forced"],
                                S, k, nmax)


def _verify_prompt(n, logits, ldl, V, d, ring_cap):
    S, k = d["ids"].shape[0], d["ids"].shape[1] - 1
    n.lookup_verify_slots_prompt(logits, ldl, V, S, k, d["params"], d["seeds"], d["bits"], d["row_bits"], d["draws"], d["row_token"],
                                 d["hist"], d["hist_len"], d["ids"], d["pos"], d["len"], d["cap"], d["live"], d["ndraft"], d["budget"],
                                 d["stop_ids"], d["ring"], d["ctr"], d["forced"], ring_cap)


def _same(dev, want, names, what):
    for name in names:
        got = dev[name].cpu().numpy()
        assert np.array_equal(got, want[name]), (what, name, got, want[name])
    assert np.array_equal(dev["bits"].cpu().numpy().view(np.uint32), want["bits"]), (what, "bits")


# ---- 1. a question's steps against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("params0", [ref.GREEDY, ref.SAMPLED], ids=["greedy", "sampled"])
@pytest.mark.parametrize("V", [1001, 32000])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_forced_steps_equal_the_reference(k, V, params0):
    """S = 3: slot 0 is fed its question, slot 1 decodes with made-up drafts (two right, then a wrong one), slot 2 is idle.  Two
    question lengths: q = k + 3 (a full step, then the step that ends the question in row 1) and q = k + 2 (the forced rows run out
    at the end of a step: an ordinary step with draws = 0 feeds the last token).  Every state word and ring record after every
    draft and every verify launch; a sampled draw is compared where the reference's float64 score margin exceeds 1e-4, and
    followed on the device's token otherwise."""
    n = _n()
    S, ring_cap = ref.CASE_S, ref.CASE_RING
    pairs = checked = 0
    for q in (k + 3, k + 2):
        st, params, seeds, logits, steps = ref.case(V, k, params0, q)
        dev = _each_words(n, st, V, params, seeds)
        first = None
        for step in range(steps):
            what = (q, step)
            # the draft launch: forced rows for slot 0 while its question lasts, the n-gram search for slot 1, nothing for slot 2
            _draft_prompt(n, dev, k)
            torch.cuda.synchronize()
            st = ref.draft_slots_prompt(st, k)
            _same(dev, st, WORDS, what + ("draft",))
            forced_now = int(st["forced"][0])
            ref.case_drafts(st, logits[step], params, seeds, k, 2, 3)
            for name in ("ids", "pos", "ndraft"):
                dev[name].copy_(torch.from_numpy(st[name]))
            buf = torch.full((S * (k + 1), V + 4), 7.0, dtype=torch.float32, device=DEV)          # (row stride V + 4)
            x = buf[:, :V]
            x.copy_(torch.from_numpy(logits[step]))
            dev["row_token"].fill_(-1)
            _verify_prompt(n, x, V + 4, V, dev, ring_cap)
            torch.cuda.synchronize()
            row_token = dev["row_token"].cpu().numpy().reshape(S, k + 1)
            want, infos = ref.verify_slots_prompt(logits[step], st, k, ring_cap, params, seeds)
            force = {}
            for b, info in enumerate(infos):
                if info is None:
                    assert np.all(row_token[b] == -1), what + (b,)
                    continue
                R = info.get("forced", 0)
                rows = ([R] if info["emit"] else []) if R else list(range(len(info["tokens"])))
                assert [i for i in range(k + 1) if row_token[b, i] != -1] == rows, what + (b, row_token[b])   # nothing else was drawn
                for i, tok, margin in zip(rows, info["tokens"], info["margins"]):
                    got = int(row_token[b, i])
                    sampled = params[b] != ref.GREEDY
                    pairs += sampled
                    if margin > ref.MARGIN:
                        assert got == tok, what + (b, i, got, tok, margin)
                        checked += sampled
                    elif got != tok:
                        force[(b, i)] = got
            if force:
                want, infos = ref.verify_slots_prompt(logits[step], st, k, ring_cap, params, seeds, force=force)
            _same(dev, want, WORDS, what + ("verify",))
            if forced_now and first is None and infos[0]["emit"]:
                first = step
                assert forced_now <= k and int(want["draws"][0]) == 1 and int(want["forced"][0]) == 0
            st = want
        assert st["ctr"].tolist() == [5 + steps] * S and not st["live"][2]
        if q == k + 3:
            assert first == 1, first                            # R = k + 2 > k: an EMPTY record; then R = 1: row 1 ends the question
            assert int(st["len"][0]) >= 64 + q and int(st["pos"][0, 0]) - 200 == int(st["len"][0]) - 64
    print(f"[forced rows k={k} V={V}] sampled rows {pairs}, compared outright {checked}")
    # (a condition on the inputs, met by the reference alone: test_loop_prefill_cpu.test_case_seeds_leave_three_quarters_comparable)
    assert pairs > 0 and 4 * checked >= 3 * pairs, (checked, pairs)


# ---- 2. no forced rows: the existing entries, word for word ---------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1001, 32000])
def test_without_forced_rows_the_entries_are_the_existing_ones(V):
    n = _n()
    S, k = lsv.EACH_S, lsv.EACH_K
    st, seeds, logits = lsv.each_case(V)
    st["ids"][:, 1:], st["pos"][:, 1:], st["ndraft"][:] = -7, -9, -1                      # (what only the draft launch writes)
    a = _each_words(n, st, V, lsv.EACH_PARAMS, seeds)
    b = _each_words(n, dict(st, forced=np.zeros(S, dtype=np.int32)), V, lsv.EACH_PARAMS, seeds)
    for step in range(lsv.EACH_STEPS):
        n.lookup_draft_slots(a["hist"], a["hist_len"], a["ids"], a["pos"], a["ndraft"], a["cap"], a["len"], a["live"], S, k, 3)
        _draft_prompt(n, b, k)
        x = torch.from_numpy(logits[step]).to(DEV)
        _verify_each(n, x, V, V, a, lsv.EACH_RING)
        _verify_prompt(n, x, V, V, b, lsv.EACH_RING)
        torch.cuda.synchronize()
        for name in SLOT_WORDS + ("draws", "bits", "row_token"):
            assert torch.equal(a[name], b[name]), (step, name)
        assert not b["forced"].any()
    assert int(a["ctr"][0]) == lsv.EACH_CTR + 2


# ---- 3. pc_lookup_slot_arm_prompt ---------------------------------------------------------------------------------------------------
def test_arm_prompt_writes_one_slot_word_for_word():
    """Every array holds one slot more than the entry is told (S + 1 rows, S = 4): the row behind the last slot is a guard.  The
    armed slot is the last one, so whatever ran past its words would land in the guard."""
    n = _n()
    S, k, V, hist_cap = 4, 3, 1001, 40
    hw = (V + 31) // 32
    rng = np.random.default_rng(4)
    st, handle = _sentinel_state(n, S + 1, k, V, hist_cap)
    forced = torch.full((S + 1,), 127, dtype=torch.int32, device=DEV)
    arena = torch.zeros(8, dtype=torch.float16, device=DEV)
    bit_ids = sorted(set(int(t) for t in rng.integers(0, V, 40)))
    corpus, question = [int(t) for t in rng.integers(0, V, 8)], [int(t) for t in rng.integers(0, V, 7)]
    hist_ids = corpus + question                                          # (an odd count: the last 64-bit word is half used)
    seed = int(rng.integers(0, 2 ** 62))
    nbytes = n.lookup_slot_arm_bytes(hw, len(hist_ids))
    for n_forced in (len(question) - 1, 0):
        fed = hist_ids[len(hist_ids) - n_forced - 1]                      # the token the slot feeds first: t_0, or the last id
        f = dict(slot=S - 1, cap=900, kv_base=arena.data_ptr(), len=40, pos=77, id=fed, leader=-1, trunk=0, budget=6, counter=12,
                 seed=seed, params=ref.SAMPLED, stop_ids=[5, 6, 7], bits=lsr.history_bits(bit_ids, V))
        host = _pinned(lsv.lookup_arm_block_bytes(n, hw, hist_ids, **f))
        st["live"].zero_()
        before = {name: v.cpu().clone() for name, v in st.items()}
        before["forced"] = forced.cpu().clone()
        n.lookup_slot_arm_prompt(host, nbytes, handle, forced, n_forced, S, k, hist_cap)
        torch.cuda.synchronize()
        after = {name: v.cpu().clone() for name, v in st.items()}
        after["forced"] = forced.cpu().clone()
        s = S - 1
        want = ref.new_state(S + 1, k, V, hist_cap, 4)
        ref.arm_prompt(want, s, k, V, hist_ids, n_forced, 77, 40, 900, 6, 12, bit_ids, [5, 6, 7])
        for name in ("cap", "len", "live", "ndraft", "budget", "hist_len", "ctr", "draws", "forced"):
            assert int(after[name][s]) == int(want[name][s]), (n_forced, name)
        assert (int(after["hist_len"][s]), int(after["forced"][s]), int(after["draws"][s])) == (len(hist_ids) - n_forced, n_forced, 0)
        assert int(after["kv_base"][s]) == arena.data_ptr() and int(after["seeds"][s]) == seed
        assert (int(after["leader"][s]), int(after["trunk"][s])) == (-1, 0)
        assert after["ids"][s].tolist() == [fed, 115, 115, 115] and int(want["ids"][s, 0]) == fed
        assert after["pos"][s].tolist() == [77, 114, 114, 114]
        assert bytes(after["params"][24 * s:24 * s + 24].numpy()) == n.sample_params_bytes(*ref.SAMPLED, 0)
        assert after["stop_ids"][s].tolist() == [5, 6, 7, -1, -1, -1, -1, -1]
        assert np.array_equal(after["bits"][s].numpy().view(np.uint32), want["bits"][s])
        assert after["hist"][s].tolist() == hist_ids + [126] * (hist_cap - len(hist_ids))          # all ids, the question included
        for name in after:                                               # every word of every other slot and of the guard row
            keep = [b for b in range(S + 1) if b != s]
            assert torch.equal(after[name].view(S + 1, -1)[keep], before[name].view(S + 1, -1)[keep]), (n_forced, name)
    # n_forced = 0 armed a slot that the existing step moves: the first token is drawn at step 0 (draws was armed 0)
    x = (rng.standard_normal(((S + 1) * (k + 1), V)) * 2.0).astype(np.float32)
    tok, margin, _ = lsr.draw(x[(S - 1) * (k + 1)], bit_ids, ref.SAMPLED, seed, 0)
    assert margin > ref.MARGIN, "pick another rng seed: the reference's draw is a near-tie"
    ring = torch.full((S + 1, 16, k + 2), -1, dtype=torch.int32, device=DEV)
    row_bits = torch.zeros((S + 1) * (k + 1) * hw, dtype=torch.int32, device=DEV)
    row_token = torch.zeros((S + 1) * (k + 1), dtype=torch.int32, device=DEV)
    n.lookup_verify_slots_prompt(torch.from_numpy(x).to(DEV), V, V, S, k, st["params"], st["seeds"], st["bits"], row_bits, st["draws"],
                                 row_token, st["hist"][:S], st["hist_len"], st["ids"], st["pos"], st["len"], st["cap"], st["live"],
                                 st["ndraft"], st["budget"], st["stop_ids"], ring, st["ctr"], forced, 16)
    torch.cuda.synchronize()
    assert ring[S - 1, 12].tolist()[:2] == [1, tok] and int(st["draws"][S - 1]) == 1 and int(st["budget"][S - 1]) == 5


# ---- 4. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched():
    n = _n()
    V, k, q = 1001, 3, 6
    st, params, seeds, logits, _ = ref.case(V, k, ref.SAMPLED, q)
    dev = _each_words(n, st, V, params, seeds)
    before = {name: v.clone() for name, v in dev.items()}
    x = torch.from_numpy(logits[0]).to(DEV)
    S = ref.CASE_S
    with pytest.raises(RuntimeError, match="pc_lookup_draft_slots_prompt"):
        n.lookup_draft_slots_prompt(dev["hist"], dev["hist_len"], dev["ids"], dev["pos"], dev["ndraft"], dev["cap"], dev["len"], dev["live"],
                                    None, S, k, 3)
    with pytest.raises(RuntimeError, match="pc_lookup_draft_slots_prompt"):
        n.lookup_draft_slots_prompt(dev["hist"], dev["hist_len"], dev["ids"], dev["pos"], dev["ndraft"], dev["cap"], dev["len"], dev["live"],
                                    dev["forced"], S, k, 9)
    for bad in (dict(forced=None), dict(ring_cap=0), dict(ldl=V - 1)):
        d = dict(dev, **{w: v for w, v in bad.items() if w == "forced"})
        with pytest.raises(RuntimeError, match="pc_lookup_verify_slots_prompt"):
            _verify_prompt(n, x, bad.get("ldl", V), V, d, bad.get("ring_cap", ref.CASE_RING))
    hw = (V + 31) // 32
    sent, handle = _sentinel_state(n, S, k, V, 40)
    forced = torch.full((S,), 127, dtype=torch.int32, device=DEV)
    sent_before = {name: v.clone() for name, v in sent.items()}
    f = dict(slot=1, cap=900, kv_base=0, len=40, pos=77, id=3, leader=-1, trunk=0, budget=6, counter=0, seed=1, params=ref.GREEDY,
             stop_ids=[], bits=np.zeros(hw, dtype=np.uint32))
    host = _pinned(lsv.lookup_arm_block_bytes(n, hw, [1, 2, 3], **f))
    nb = n.lookup_slot_arm_bytes(hw, 3)
    for kw in (dict(forced=None, n_forced=1), dict(n_forced=3), dict(n_forced=-1), dict(nbytes=nb - 8), dict(S=1)):
        with pytest.raises(RuntimeError, match="pc_lookup_slot_arm_prompt"):
            n.lookup_slot_arm_prompt(host, kw.get("nbytes", nb), handle, kw.get("forced", forced), kw.get("n_forced", 1), kw.get("S", S), k, 40)
    torch.cuda.synchronize()
    for name, v in before.items():
        assert torch.equal(dev[name], v), name
    for name, v in sent_before.items():
        assert torch.equal(sent[name], v), name
    assert forced.tolist() == [127] * S
