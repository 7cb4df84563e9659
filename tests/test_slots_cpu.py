"""Batched decode over slots, the parts that need no GPU: the numpy reference against the oracle's attention, the C-ABI
declarations, ``CacheEngine(slots=...)`` argument checks and ``generate_batch``'s fallback decision table."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import llama_oracle as orc
from tests import slots_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pc_rope_append_slots", "pc_attn_decode_slots", "pc_attn_decode_slots_workspace_bytes", "pc_sample_advance_slots")


@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 128), (4, 2, 128), (8, 1, 64)])
def test_reference_equals_attention_core_slot_by_slot(H, Hkv, D):
    rng = np.random.default_rng(H * 100 + Hkv)
    lens = [1, 2, 64, 65, 300]
    q = rng.standard_normal((len(lens) + 1, H, D)).astype(np.float32)
    keys = [(0.7 * rng.standard_normal((Hkv, n, D))).astype(np.float16) for n in lens] + [None]
    vals = [rng.standard_normal((Hkv, n, D)).astype(np.float16) for n in lens] + [None]
    got = ref.attend_slots(q, keys, vals)
    assert got[-1] is None
    for b, n in enumerate(lens):
        want = orc.attention_core(q[b][None, :, None, :], keys[b][None].astype(np.float32), vals[b][None].astype(np.float32),
                                  n - 1, H // Hkv)[0, :, 0, :]
        assert np.abs(got[b] - want).max() < 2e-6, (b, n)


def test_reference_advance_rule():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(64).astype(np.float32)
    top = int(np.argmax(x))
    st = dict(ids=0, pos=10, len=5, cap=100, live=1, budget=2, ctr=0, seed=1)
    tok, _, _ = ref.advance_slot(st, x, set(), 0.0, 1.0, 1.0, -1, ())
    assert tok == top and (st["pos"], st["len"], st["ctr"], st["budget"], st["live"]) == (11, 6, 1, 1, 1)
    ref.advance_slot(st, x, set(), 0.0, 1.0, 1.0, -1, ())
    assert st["live"] == 0 and st["budget"] == 0                         # budget used up
    before = dict(st)
    assert ref.advance_slot(st, x, set(), 0.0, 1.0, 1.0, -1, ())[0] is None and st == before     # idle: nothing moves
    st = dict(ids=0, pos=10, len=5, cap=100, live=1, budget=9, ctr=0, seed=1)
    ref.advance_slot(st, x, set(), 0.0, 1.0, 1.0, -1, (top,))
    assert st["live"] == 0                                               # stop id
    st = dict(ids=0, pos=10, len=97, cap=100, live=1, budget=9, ctr=0, seed=1)
    ref.advance_slot(st, x, set(), 0.0, 1.0, 1.0, -1, ())
    assert st["len"] == 98 and st["live"] == 1
    ref.advance_slot(st, x, set(), 0.0, 1.0, 1.0, -1, ())
    assert st["len"] == 99 and st["live"] == 0                           # the next row would be the arena's last
    st = dict(ids=7, pos=10, len=100, cap=100, live=1, budget=9, ctr=4, seed=1)
    assert ref.advance_slot(st, x, set(), 0.0, 1.0, 1.0, -1, ())[0] is None
    assert (st["ids"], st["len"], st["ctr"], st["live"]) == (7, 100, 4, 0)    # a full arena only goes idle


def test_header_declares_and_library_exports_the_slot_entries():
    from promptcache_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "promptcache_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.lib_path())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _native.SIGNATURES, name


def test_slot_entries_reject_bad_arguments_without_a_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    assert lib.pc_attn_decode_slots_workspace_bytes(8, 32, 128, 4) == 8 * 32 * 4 * 130 * 4
    assert lib.pc_attn_decode_slots_workspace_bytes(0, 32, 128, 4) == 0
    assert lib.pc_rope_append_slots(None, 0, 0, None, None, 0, None, None, None, None, None, 17, 0, 4, 4, 128, None) == -1001
    assert b"S <= 16" in lib.pc_last_error_string()
    assert lib.pc_attn_decode_slots(None, None, 0, None, None, None, None, 8, 0, 4, 4, 96, 0.1, 4, None, 0, None, None, None) == -1001
    assert b"head_dim 64 or 128" in lib.pc_last_error_string()
    assert lib.pc_attn_decode_slots(None, None, 0, None, None, None, None, 8, 0, 4, 4, 128, 0.1, 33, None, 0, None, None, None) == -1001
    assert b"nsplit" in lib.pc_last_error_string()
    assert lib.pc_sample_advance_slots(None, 0, 10, None, None, None, None, None, None, None, None, None, None, None, None, 4, 8,
                                       None, None) == -1001


class _FakeLM:
    device = "cpu"
    use_full_position_ids = False

    def get_cache_shape(self):
        return 2, 4, 128


@pytest.mark.parametrize("bad", [0, -1, 17, 2.0, "2", True, None])
def test_cache_engine_rejects_bad_slot_counts(bad):
    from promptcache_amd import CacheEngine
    with pytest.raises(ValueError, match="slots"):
        CacheEngine(64, _FakeLM(), target_device="cpu", slots=bad)


def test_cache_engine_slots_are_separate_buffers_allocated_on_first_use():
    from promptcache_amd import CacheEngine
    eng = CacheEngine(64, _FakeLM(), target_device="cpu", slots=3)
    assert eng.slots == 3 and eng.slot_cache(0) is eng.prompt_cache
    assert eng._slot_caches == [None, None, None]
    a = eng.slot_cache(2)
    assert a is eng.slot_cache(2) and a is not eng.prompt_cache and eng._slot_caches[1] is None
    assert a.arena.buf.data_ptr() != eng.prompt_cache.arena.buf.data_ptr()
    assert a.arena.buf.shape == eng.prompt_cache.arena.buf.shape and a.defer_gather == eng.prompt_cache.defer_gather
    for bad in (-1, 3, 1.0, None, True):
        with pytest.raises(ValueError, match="slot"):
            eng.slot_cache(bad)
    a.length = a.arena.length = 7
    eng.remove_all_schemas()
    assert a.length == 0 and eng.prompt_cache.length == 0
    assert CacheEngine(64, _FakeLM(), target_device="cpu").slots == 1


def _engine(hf=None, full=False):
    from promptcache_amd.generation_engine import GenerationEngine
    lm = types.SimpleNamespace(hf_model=hf, use_full_position_ids=full)
    return GenerationEngine(lm)


def test_generate_batch_fallback_decision_table():
    from promptcache_amd.generation_engine import GenerationParameters
    ok = types.SimpleNamespace(slot_loop=lambda *a, **k: None, slot_loop_available=lambda: True)
    no = types.SimpleNamespace(slot_loop=lambda *a, **k: None, slot_loop_available=lambda: False)      # Falcon, int8, PC_DECODE_TAIL=1
    greedy = GenerationParameters(temperature=0.0, max_new_tokens=8)
    sampled = GenerationParameters(temperature=0.7, top_p=0.9, max_new_tokens=8)
    assert _engine(ok).batch_plan(4, greedy)[0] and _engine(ok).batch_plan(16, sampled)[0] and _engine(ok).batch_plan(1, greedy)[0]
    assert not _engine(ok).batch_plan(17, greedy)[0]
    assert not _engine(ok).batch_plan(0, greedy)[0]
    assert not _engine(ok, full=True).batch_plan(4, greedy)[0]                       # MPT
    assert not _engine(no).batch_plan(4, greedy)[0]
    assert not _engine(types.SimpleNamespace()).batch_plan(4, greedy)[0]             # a model without the entry
    assert not _engine(None).batch_plan(4, greedy)[0]
    e = _engine(ok)
    e.device_greedy_loop = False                                                      # PC_DEVICE_GREEDY=0
    assert not e.batch_plan(4, greedy)[0] and e.batch_plan(4, sampled)[0]
    e = _engine(ok)
    e.device_sample_loop = False                                                      # PC_DEVICE_SAMPLE=0
    assert e.batch_plan(4, greedy)[0] and not e.batch_plan(4, sampled)[0]
    assert not e.batch_plan(4, GenerationParameters(temperature=0.0, repetition_penalty=1.2))[0]   # greedy with a penalty: sampled loop
    assert not _engine(ok).batch_plan(4, GenerationParameters(temperature=0.0, stop_token_ids=list(range(9))))[0]
    assert not _engine(ok).batch_plan(4, GenerationParameters(temperature=0.0, max_new_tokens=1))[0]


def test_models_say_whether_they_host_a_slot_loop():
    from promptcache_amd.model.falcon_hip import FalconHIP
    from promptcache_amd.model.llama_hip import LlamaHIP, SlotLoop
    from promptcache_amd.model.mpt_hip import MptHIP
    assert LlamaHIP.supports_slot_loop and not FalconHIP.supports_slot_loop and not MptHIP.supports_slot_loop
    assert SlotLoop.MAX_SLOTS == 16
