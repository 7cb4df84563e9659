"""The host side ``SlotLoop`` and ``LookupSlotLoop`` share, the parts that need no GPU: the bytes of the two arm blocks against
``struct.pack`` images laid out from include/promptcache_hip.h, the trunk table check, the ``sampled`` predicate and the surface
``GenerationEngine`` and the factories rely on."""
import inspect
import struct
import types

import numpy as np
import pytest

# pc_slot_arm_block / pc_lookup_slot_arm_block of include/promptcache_hip.h, field for field (no padding: every field sits on its
# natural alignment).  The two differ in the pair of words before the seed only.
HEAD = "<iiQiiq" + "iiii"                      # slot cap kv_base len pos id | leader trunk budget counter
TAIL = "Q" + "fffiQ" + "8i"                    # seed | pc_sample_params {temperature repetition_penalty top_p top_k seed} | stop_ids
HEADER_BYTES = 120
SENTINEL = 0xCD

SAMPLED = types.SimpleNamespace(temperature=0.7, repetition_penalty=1.2, top_p=0.9, top_k=40, greedy=False)
GREEDY = types.SimpleNamespace(temperature=0.0, repetition_penalty=1.0, top_p=1.0, top_k=0, greedy=True)
PARAMS = {"sampled": (SAMPLED, (0.7, 1.2, 0.9, 40, 0)), "greedy": (GREEDY, (0.0, 1.0, 1.0, -1, 0))}
FIELDS = dict(slot=3, cap=4096, kv_base=0x7F12_3456_7000, len=777, pos=801, id=31999, leader=1, trunk=256, budget=64, counter=1030)
STOPS = {0: [], 3: [2, 13, 29871], 8: [2, 5, 7, 11, 13, 17, 19, 23]}
SEED = 2 ** 63 + 2 ** 40 + 12345                # above 2^63: the block carries its low 63 bits


def _bitmap(ids, vocab):
    words = [0] * ((vocab + 31) // 32)
    for t in ids:
        if 0 <= t < vocab:
            words[t >> 5] |= 1 << (t & 31)
    return struct.pack("<%dI" % len(words), *words)


def _expected(kind, extra, hist_words, params_words, stops, bitmap, hist_ids=()):
    pair = (extra["draws"], hist_words) if kind == "slot" else (hist_words, extra["hist_len"])
    f = FIELDS
    head = struct.pack(HEAD + "ii" + TAIL, f["slot"], f["cap"], f["kv_base"], f["len"], f["pos"], f["id"], f["leader"], f["trunk"],
                       f["budget"], f["counter"], *pair, SEED & (2 ** 63 - 1), *params_words, *(stops + [-1] * (8 - len(stops))))
    assert len(head) == HEADER_BYTES
    pad = bytes([SENTINEL]) * (-len(bitmap) % 8)            # the filler leaves the pad alone
    return head + bitmap + pad + struct.pack("<%di" % len(hist_ids), *hist_ids)


@pytest.mark.parametrize("hist_words", [5, 4])
@pytest.mark.parametrize("nstop", [0, 3, 8])
@pytest.mark.parametrize("mode", ["sampled", "greedy"])
@pytest.mark.parametrize("kind", ["slot", "lookup"])
def test_arm_block_bytes(kind, mode, nstop, hist_words):
    from promptcache_amd import _native
    from promptcache_amd.model.llama_hip import _fill_arm_block
    vocab = 32 * hist_words - 7                   # (the last word is partly used)
    params, params_words = PARAMS[mode]
    history = [0, 31, 32, vocab - 1, vocab, -4, 63, 63, 70]          # ids outside the vocabulary are ignored
    hist_ids = [9, 8, 7, 6, 5] if kind == "lookup" else []           # odd length
    header = _native.SlotArmBlock if kind == "slot" else _native.LookupSlotArmBlock
    extra = {"draws": 1} if kind == "slot" else {"hist_len": len(hist_ids)}
    arr = np.full(HEADER_BYTES + 4 * hist_words + 4 + 4 * len(hist_ids) + 16, SENTINEL, dtype=np.uint8)
    off = _fill_arm_block(arr, header, dict(FIELDS, **extra), SEED, params, STOPS[nstop], history, vocab)
    assert off == HEADER_BYTES + (4 * hist_words + 7) // 8 * 8
    if kind == "lookup":                          # what the lookup leaf does behind the filler
        arr[off:off + 4 * len(hist_ids)].view(np.int32)[:] = hist_ids
    bitmap = _bitmap(history, vocab) if mode == "sampled" else bytes(4 * hist_words)
    want = _expected(kind, extra, hist_words, params_words, STOPS[nstop], bitmap, hist_ids)
    assert arr[:len(want)].tobytes() == want
    assert (arr[len(want):] == SENTINEL).all()     # nothing written behind the block
    # the native byte counts are the filler's offsets
    assert _native.slot_arm_bytes(hist_words) == off
    assert _native.lookup_slot_arm_bytes(hist_words, len(hist_ids)) == off + (4 * len(hist_ids) + 7) // 8 * 8


def test_arm_block_of_a_greedy_stream_with_a_penalty_is_sampled():
    from promptcache_amd import _native
    from promptcache_amd.model.llama_hip import _fill_arm_block
    params = types.SimpleNamespace(temperature=0.0, repetition_penalty=1.1, top_p=1.0, top_k=0, greedy=True)
    arr = np.zeros(HEADER_BYTES + 16, dtype=np.uint8)
    _fill_arm_block(arr, _native.SlotArmBlock, dict(FIELDS, draws=1), 7, params, [], [1, 33], 128)
    want = _expected("slot", {"draws": 1}, 4, (0.0, 1.1, 1.0, -1, 0), [], _bitmap([1, 33], 128))
    assert arr.tobytes()[8 * 7 + 8:] == want[8 * 7 + 8:]            # everything behind the seed
    assert struct.unpack_from("<Q", arr, 56)[0] == 7


def test_slot_trunks_table():
    from promptcache_amd.model.llama_hip import _slot_trunks
    assert _slot_trunks(None, [300, 400, 5]) == [(None, 0)] * 3
    # the (leader, T) tables of tests/test_trunk_cpu.py, over arenas that hold the rows
    two_groups = [(0, 400), (1, 300), (None, 0), (0, 400), (None, 0), (1, 300), (1, 300)]
    lengths = [410, 385, 77, 410, 0, 385, 305]
    assert _slot_trunks(two_groups, lengths) == two_groups
    assert _slot_trunks([(0, 300)] * 3, [300, 350, 350]) == [(0, 300)] * 3
    assert _slot_trunks([(np.int64(0), np.int32(300)), (0, 300)], [350, 350]) == [(0, 300), (0, 300)]
    with pytest.raises(AssertionError):            # a leader that does not lead itself
        _slot_trunks([(None, 0), (0, 300)], [350, 350])
    with pytest.raises(AssertionError):            # ... or leads itself over other rows
        _slot_trunks([(0, 299), (0, 300)], [350, 350])
    with pytest.raises(AssertionError):            # T above the member's length
        _slot_trunks([(0, 300), (0, 300)], [350, 299])
    with pytest.raises(AssertionError):            # T above the leader's length
        _slot_trunks([(0, 300), (0, 300)], [299, 350])
    with pytest.raises(AssertionError):
        _slot_trunks([(0, 0), (0, 0)], [350, 350])


def test_is_sampled():
    from promptcache_amd.model.llama_hip import _is_sampled
    P = lambda greedy, rp: types.SimpleNamespace(greedy=greedy, repetition_penalty=rp)
    assert _is_sampled(None) is False
    assert _is_sampled(P(True, 1.0)) is False
    assert _is_sampled(P(True, 1.1)) is True
    assert _is_sampled(P(False, 1.0)) is True


def test_class_surface():
    from promptcache_amd.model.llama_hip import LookupSlotLoop, SlotLoop, _SlotLoopHost
    assert SlotLoop.__bases__ == (_SlotLoopHost,) and LookupSlotLoop.__bases__ == (_SlotLoopHost,)
    # generation_engine._reader tells the two apart by ``tokens``
    assert hasattr(SlotLoop, "token") and not hasattr(SlotLoop, "tokens")
    assert hasattr(LookupSlotLoop, "tokens") and not hasattr(LookupSlotLoop, "token")
    assert list(inspect.signature(SlotLoop.__init__).parameters) == [
        "self", "model", "arenas", "tokens", "positions", "max_new", "params", "seeds", "histories", "stop_ids", "slots", "slot_index",
        "trunks", "each", "max_keys"]
    assert list(inspect.signature(LookupSlotLoop.__init__).parameters) == [
        "self", "model", "arenas", "tokens", "positions", "max_new", "k", "corpora", "nmax", "stop_ids", "slots", "max_keys", "trunks",
        "each", "slot_index", "params", "seeds", "histories", "hist_cap"]
    for cls in (SlotLoop, LookupSlotLoop):
        for name in ("admit", "retire", "enqueue", "elapsed_ms", "kill", "close"):
            assert callable(getattr(cls, name)), (cls, name)
    assert (SlotLoop.RING, SlotLoop.MAX_SLOTS, LookupSlotLoop.RING, LookupSlotLoop.MAX_ROWS) == (1024, 16, 1024, 64)
