"""Helpers of tests/test_serve_cpu.py and tests/test_gpu_serve.py: the per-slot reference of pc_sample_advance_slots_each (on top of
tests/slots_ref.py), the layout of the cases of the per-slot advance test, and the device words of both kernels."""
import ctypes

import numpy as np

from tests import slots_ref as ref

GREEDY = (0.0, 1.0, 1.0, -1)
SAMPLED = (0.7, 1.1, 0.9, 40)
WIDE = (1.0, 1.0, 0.95, -1)
MARGIN = 1e-4           # tests/test_gpu_sample.py: draws are compared where the reference's own decision is not a near-tie

# the per-slot advance case (S = 8): slots alternate greedy / sampled, slot 5 takes the third chain; slots 2 and 6 are idle, slot 7
# holds a full arena; draws != counters everywhere
EACH_S = 8
EACH_PARAMS = [GREEDY, SAMPLED, GREEDY, SAMPLED, GREEDY, WIDE, GREEDY, SAMPLED]
EACH_LIVE = [1, 1, 0, 1, 1, 1, 0, 1]
EACH_LENS = [50, 53, 56, 59, 62, 65, 68, 80]
EACH_CAPS = [1000, 1000, 1000, 1000, 1000, 1000, 1000, 80]          # slot 7: len == cap
EACH_CTR, EACH_BUDGET, EACH_STEPS = 3, 4, 6
EACH_DRAWS = [10 + 3 * b for b in range(EACH_S)]
# rng seeds per vocabulary size, picked on the CPU (test_serve_cpu.test_each_case_seeds_leave_three_quarters_comparable runs the
# reference alone): at least 3/4 of the live sampled (slot, step) pairs have a margin above MARGIN
EACH_RNG_SEED = {1001: 11, 32000: 12}


def advance_each(state: dict, logits, history: set, prm, stop_row):
    """pc_sample_advance_slots_each for one slot: tests/slots_ref.advance_slot with that slot's parameters and stop row, the
    random stream counted by ``state["draws"]`` and ``state["ctr"]`` left to the ring.  -> (token | None, margin, processed)."""
    tmp = dict(state, ctr=state["draws"])
    tok, margin, proc = ref.advance_slot(tmp, logits, history, *prm, tuple(int(t) for t in stop_row if t >= 0))
    for f in ("ids", "pos", "len", "live", "budget"):
        state[f] = tmp[f]
    if tok is not None:
        state["draws"] += 1
        state["ctr"] += 1
    return tok, margin, proc


def each_case(V: int):
    """Inputs of the per-slot advance case at vocabulary ``V``: (rng, histories, seeds, first logits, stop rows)."""
    rng = np.random.default_rng(EACH_RNG_SEED[V])
    S = EACH_S
    hists = [set(int(t) for t in rng.integers(b * (V // S), (b + 1) * (V // S), 30)) for b in range(S)]
    seeds = [int(s) for s in rng.integers(0, 2 ** 62, S)]
    x0 = (rng.standard_normal((S, V)) * 2.0).astype(np.float32)
    # slot 3's stop row holds the token the reference draws for slot 3 at step 0 (it ends exactly that slot); the other rows hold
    # ids of their own
    st3 = dict(ids=0, pos=0, len=1, cap=9, live=1, budget=9, ctr=0, draws=EACH_DRAWS[3], seed=seeds[3])
    stop3 = advance_each(st3, x0[3], set(hists[3]), EACH_PARAMS[3], ())[0]
    stops = np.full((S, 8), -1, dtype=np.int32)
    for b in range(S):
        stops[b, 0] = (stop3 + 1 + b) % V
        stops[b, 1] = (7 * b + 5) % V
    stops[3, 2] = stop3
    return rng, hists, seeds, x0, stops


def each_states(seeds):
    return [dict(ids=-5, pos=100, len=EACH_LENS[b], cap=EACH_CAPS[b], live=EACH_LIVE[b], budget=EACH_BUDGET, ctr=EACH_CTR,
                 draws=EACH_DRAWS[b], seed=seeds[b]) for b in range(EACH_S)]


def each_reference_margins(V: int):
    """The reference alone over the case (it follows its own tokens): margins of the live sampled (slot, step) pairs."""
    rng, hists, seeds, x0, stops = each_case(V)
    want, whist = each_states(seeds), [set(h) for h in hists]
    margins = []
    for step in range(EACH_STEPS):
        x = x0 if step == 0 else (rng.standard_normal((EACH_S, V)) * 2.0).astype(np.float32)
        for b in range(EACH_S):
            tok, margin, _ = advance_each(want[b], x[b], whist[b], EACH_PARAMS[b], stops[b])
            if tok is not None and EACH_PARAMS[b] != GREEDY:
                margins.append(float(margin))
    return margins


def arm_block_bytes(native, hist_words, **f) -> bytearray:
    """A pc_slot_arm block as bytes: ``f`` = fields of pc_slot_arm_block (params: a 4-tuple, stop_ids: a list, hist: uint32 words)."""
    buf = bytearray(native.slot_arm_bytes(hist_words))
    b = native.SlotArmBlock.from_buffer(buf)
    for name in ("slot", "cap", "kv_base", "len", "pos", "id", "leader", "trunk", "budget", "counter", "draws", "seed"):
        setattr(b, name, int(f[name]))
    b.hist_words = hist_words
    b.params = native.SampleParams.from_buffer_copy(native.sample_params_bytes(*f["params"], 0))
    for j in range(8):
        b.stop_ids[j] = int(f["stop_ids"][j]) if j < len(f["stop_ids"]) else -1
    del b
    n0 = ctypes.sizeof(native.SlotArmBlock)
    buf[n0:n0 + 4 * hist_words] = np.asarray(f["hist"], dtype=np.uint32).tobytes()
    return buf
