"""Shared-trunk batched decode, the parts that need no GPU: the two-part numpy reference against the one-part one and float64,
``common_trunks``' grouping table, the C-ABI declarations and argument checks, ``generate_batch``'s new parameter and the
staged-layout record ``PromptCache.update`` keeps on its arena."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from tests import slots_ref
from tests import trunk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pc_attn_decode_slots_trunk", "pc_attn_decode_slots_trunk_workspace_bytes")
REF_TOL = 2e-6


@pytest.mark.parametrize("n,T", [(8259, 8000), (1738, 1725), (300, 256), (66, 64), (1738, 1)])
def test_two_part_reference_equals_the_one_part_reference_and_float64(n, T):
    rng = np.random.default_rng(n * 7 + T)
    H, Hkv, D = 4, 2, 128
    q = rng.standard_normal((H, D)).astype(np.float32)
    k = (0.7 * rng.standard_normal((Hkv, n, D))).astype(np.float16)
    v = rng.standard_normal((Hkv, n, D)).astype(np.float16)
    got = ref.attend_trunk(q, k[:, :T], v[:, :T], k[:, T:], v[:, T:])
    e1 = float(np.abs(got - slots_ref.attend_slot(q, k, v)).max())
    e2 = float(np.abs(got - ref.attend_f64(q, k, v)).max())
    print(f"[trunk_ref n={n} T={T}] vs attend_slot {e1:.2e}, vs float64 {e2:.2e}")
    assert e1 < REF_TOL and e2 < REF_TOL, (n, T, e1, e2)


def test_a_split_without_keys_has_no_weight_in_the_merge():
    rng = np.random.default_rng(1)
    q = rng.standard_normal((2, 64)).astype(np.float32)
    k = rng.standard_normal((2, 9, 64)).astype(np.float16)
    v = rng.standard_normal((2, 9, 64)).astype(np.float16)
    a = ref.merge([ref.partial(q, k, v)])
    b = ref.merge([ref.partial(q, k[:, :0], v[:, :0]), ref.partial(q, k, v)])
    assert np.array_equal(a, b)


def test_common_trunks_table():
    from promptcache_amd.model.kv_arena import common_trunks
    sys_, intro, a, b, c, other = (object() for _ in range(6))
    L = lambda *runs: list(runs)
    # disjoint schemas
    assert common_trunks([L((sys_, 300)), L((other, 300))], 256) == [(None, 0), (None, 0)]
    # a common run cut by a differing second module
    assert common_trunks([L((sys_, 300), (a, 50), (c, 9)), L((sys_, 300), (b, 50), (c, 9))], 256) == [(0, 300), (0, 300)]
    # identical prompts
    assert common_trunks([L((sys_, 300), (a, 50))] * 3, 256) == [(0, 350)] * 3
    # a group of one
    assert common_trunks([L((sys_, 300), (a, 50))], 1) == [(None, 0)]
    # T below min_rows, and the same batch with a lower bar
    lay = [L((sys_, 100), (a, 50)), L((sys_, 100), (b, 50))]
    assert common_trunks(lay, 256) == [(None, 0), (None, 0)]
    assert common_trunks(lay, 100) == [(0, 100), (0, 100)]
    # two groups in one batch, an unrelated sequence and an empty arena between them; the leader is the lowest index
    lay = [L((other, 400), (a, 10)), L((sys_, 300), (intro, 80), (a, 5)), L((c, 77)), L((other, 400), (b, 10)), L(),
           L((sys_, 300), (intro, 80), (b, 5)), L((sys_, 300), (a, 5))]
    assert common_trunks(lay, 256) == [(0, 400), (1, 300), (None, 0), (0, 400), (None, 0), (1, 300), (1, 300)]
    # the same rows under another identity, or the same identity with other row counts, are not shared
    assert common_trunks([L((sys_, 300)), L((sys_, 299))], 1) == [(None, 0), (None, 0)]
    # a member that is a prefix of the others bounds T
    assert common_trunks([L((sys_, 300)), L((sys_, 300), (a, 50)), L((sys_, 300), (a, 50))], 256) == [(0, 300)] * 3


def test_min_rows_default_and_environment(monkeypatch):
    from promptcache_amd.model import kv_arena
    monkeypatch.delenv("PC_SLOT_TRUNK_MIN", raising=False)
    assert kv_arena.slot_trunk_min_rows() == 256
    s = object()
    lay = [[(s, 255)], [(s, 255)]]
    assert kv_arena.common_trunks(lay) == [(None, 0)] * 2
    monkeypatch.setenv("PC_SLOT_TRUNK_MIN", "128")
    assert kv_arena.common_trunks(lay) == [(0, 255)] * 2


def test_header_declares_and_library_exports_the_trunk_entries():
    from promptcache_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "promptcache_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.lib_path())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _native.SIGNATURES, name
    assert callable(_native.attn_decode_slots_trunk) and callable(_native.attn_decode_slots_trunk_workspace_bytes)


def test_trunk_entry_rejects_bad_arguments_without_a_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    assert lib.pc_attn_decode_slots_trunk_workspace_bytes(8, 32, 128, 4, 2) == 8 * 32 * 6 * 130 * 4
    assert lib.pc_attn_decode_slots_trunk_workspace_bytes(8, 32, 128, 0, 2) == 0
    assert lib.pc_attn_decode_slots_trunk_workspace_bytes(8, 32, 128, 4, 0) == 0

    def call(S=8, H=4, Hkv=4, D=128, ns_own=4, ns_trunk=2, ptr=None, q_ts=512, ws=None, ws_bytes=0):
        return lib.pc_attn_decode_slots_trunk(ptr, ptr, q_ts, ptr, ptr, ptr, ptr, ptr, ptr, S, 0, H, Hkv, D, 0.1, ns_own, ns_trunk,
                                              ws, ws_bytes, ptr, ptr, None)
    assert call(S=17) == -1001 and b"S <= 16" in lib.pc_last_error_string()
    assert call(D=96) == -1001 and b"head_dim 64 or 128" in lib.pc_last_error_string()
    assert call(H=6, Hkv=4) == -1001
    for kw in (dict(ns_own=0), dict(ns_own=33), dict(ns_trunk=0), dict(ns_trunk=33)):
        assert call(**kw) == -1001 and b"[1, 32]" in lib.pc_last_error_string(), kw
    assert call() == -1001 and b"null pointer" in lib.pc_last_error_string()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 63) & ~63
    assert call(ptr=p, ws=p, q_ts=4) == -1001 and b"alignment" in lib.pc_last_error_string()
    assert call(ptr=p + 2, ws=p) == -1001 and b"alignment" in lib.pc_last_error_string()
    assert call(ptr=p, ws=p, ws_bytes=64) == -1001 and b"workspace" in lib.pc_last_error_string()
    need = lib.pc_attn_decode_slots_trunk_workspace_bytes(8, 4, 128, 4, 2)
    assert call(ptr=p, ws=p + 4, ws_bytes=need) == -1001 and b"workspace" in lib.pc_last_error_string()


def test_generate_batch_and_slot_loop_accept_share_trunk(monkeypatch):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    from promptcache_amd.model.llama_hip import LlamaHIP, SlotLoop
    sig = inspect.signature(GenerationEngine.generate_batch)
    assert sig.parameters["share_trunk"].default is None
    assert list(sig.parameters)[:4] == ["self", "requests", "params", "stream_interval"]
    sl = inspect.signature(LlamaHIP.slot_loop)
    assert sl.parameters["share_trunk"].default is False and sl.parameters["min_trunk"].default is None
    assert "trunks" in inspect.signature(SlotLoop.__init__).parameters
    # a model without a batched loop: the sequences run through generate() whatever share_trunk says
    seen = []
    ge = GenerationEngine(types.SimpleNamespace(hf_model=None, use_full_position_ids=False))
    monkeypatch.setattr(ge, "generate", lambda *a, **k: seen.append(a[0]) or iter(["out"]))
    params = GenerationParameters(temperature=0.0, max_new_tokens=4)
    assert list(ge.generate_batch([([1, 2], [0, 1], None)], params, share_trunk=True)) == [(0, "out")]
    assert seen == [[1, 2]]


def test_prompt_cache_update_and_reset_maintain_the_recorded_layout(monkeypatch):
    from promptcache_amd import _native
    from promptcache_amd.cache_engine import PromptCache
    monkeypatch.setattr(_native, "kv_gather", lambda *a, **k: None)

    class Entry:
        q8_shape = None
        device_store = None
        format = "fp16"

        def __init__(self, rows, used):
            self.token_sequence, self.rows, self.usage_counter = object(), rows, used
            self.store = types.SimpleNamespace(data_ptr=lambda: 0)

        def __len__(self):
            return self.rows
    pc = PromptCache(64, 2, 2, 64, "cpu")
    assert pc.arena.layout == []
    a, b, c = Entry(10, 5), Entry(7, 9), Entry(3, 1)
    pc.update([a, b, c])                                         # most-used first
    assert [(run[0] is e.token_sequence, run[1]) for run, e in zip(pc.arena.layout, (b, a, c))] == [(True, 7), (True, 10), (True, 3)]
    assert sum(run[1] for run in pc.arena.layout) == len(pc) == 20
    pc.update([b, c])
    assert [run[1] for run in pc.arena.layout] == [7, 3] and pc.arena.layout[0][0] is b.token_sequence
    # rows gathered from another store format are other bytes: a kept run keeps the format it was staged under, a new one does not
    b.format = c.format = "int8"
    b.q8_shape = c.q8_shape = a.q8_shape = (1, 1, 1)
    monkeypatch.setattr(_native, "kv_gather_q8", lambda *a, **k: None)
    a.format = "int8"
    pc.update([b, a])
    assert [run[1:] for run in pc.arena.layout] == [(7, "fp16"), (10, "int8")]
    from promptcache_amd.model.kv_arena import common_trunks
    other = [(b.token_sequence, 7, "int8"), (a.token_sequence, 10, "int8")]
    assert common_trunks([pc.arena.layout, other], 1) == [(None, 0), (None, 0)]
    assert common_trunks([other, list(other)], 1) == [(0, 17), (0, 17)]
    assert pc.arena.grown(128).layout == pc.arena.layout
    pc.reset()
    assert pc.arena.layout == [] and len(pc) == 0
