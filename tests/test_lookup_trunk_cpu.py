"""Shared-trunk attention of the batched prompt-lookup step, the parts that need no GPU: the two-part numpy reference against the
one-part one and float64, the C-ABI declarations and argument checks, ``lookup_slot_loop``'s new parameters and
``generate_batch(lookup=k, share_trunk=True)`` on a model that offers the step."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from tests import lookup_slots_ref as lsr
from tests import lookup_trunk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pc_attn_verify_slots_trunk", "pc_attn_verify_slots_trunk_workspace_bytes")
REF_TOL = 2e-6          # fp32 partials against float64 at <= 1 753 keys: tests/test_trunk_cpu.py's bar (set there for 8 259 keys)


@pytest.mark.parametrize("k", [1, 15])
@pytest.mark.parametrize("length,T", [(1738, 1725), (300, 256), (66, 65), (65, 65), (70, 1)])
def test_two_part_reference_equals_the_one_part_reference_and_float64(length, T, k):
    rng = np.random.default_rng(length * 31 + T * 7 + k)
    H, Hkv, D = 4, 2, 128
    n = length + k + 1
    q = rng.standard_normal((k + 1, H, D)).astype(np.float32)
    K = (0.7 * rng.standard_normal((Hkv, n, D))).astype(np.float16)
    V = rng.standard_normal((Hkv, n, D)).astype(np.float16)
    got = ref.verify_attend_trunk(q, K[:, :T], V[:, :T], K[:, T:], V[:, T:], length, k)
    one = lsr.verify_attend(q, K, V, length, k)
    e1 = float(np.abs(got - one).max())
    f64 = np.empty_like(one)                                  # an evaluation of its own: all scores of a row at once
    for i in range(k + 1):
        nk = length + i + 1
        Kx, Vx = np.repeat(K[:, :nk].astype(np.float64), H // Hkv, 0), np.repeat(V[:, :nk].astype(np.float64), H // Hkv, 0)
        s = np.einsum("hnd,hd->hn", Kx, q[i].astype(np.float64)) / np.sqrt(D)
        p = np.exp(s - s.max(1, keepdims=True))
        f64[i] = np.einsum("hn,hnd->hd", p / p.sum(1, keepdims=True), Vx)
    e2 = float(np.abs(got - f64).max())
    print(f"[lookup_trunk_ref len={length} T={T} k={k}] vs verify_attend {e1:.2e}, vs float64 {e2:.2e}")
    assert e1 < REF_TOL and e2 < REF_TOL, (length, T, k, e1, e2)


def test_header_declares_and_library_exports_the_trunk_verify_entries():
    from promptcache_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "promptcache_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.lib_path())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _native.SIGNATURES, name
    assert callable(_native.attn_verify_slots_trunk) and callable(_native.attn_verify_slots_trunk_workspace_bytes)


def test_trunk_verify_entry_rejects_bad_arguments_without_a_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    wsb = lib.pc_attn_verify_slots_trunk_workspace_bytes
    assert wsb(8, 3, 32, 128, 4, 2) == 8 * 4 * 32 * 6 * 130 * 4
    assert wsb(8, 3, 32, 128, 0, 2) == 0 and wsb(8, 3, 32, 128, 4, 0) == 0

    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 63) & ~63

    def call(S=4, k=3, H=4, Hkv=4, D=128, ns_own=4, ns_trunk=2, ptr=p, leader=0, q_ts=512, ws=p, ws_bytes=1 << 40):
        return lib.pc_attn_verify_slots_trunk(ptr, ptr, q_ts, ptr, ptr, ptr, ptr, ptr if leader == 0 else leader, ptr, S, k, 0, H, Hkv,
                                              D, 0.1, ns_own, ns_trunk, ws, ws_bytes, ptr, ptr, None)
    assert call(S=16, k=4) == -1001 and b"S * (k + 1) <= 64" in lib.pc_last_error_string()           # 80 rows
    assert call(S=1, k=16) == -1001 and b"k <= 15" in lib.pc_last_error_string()
    assert call(S=17, k=1) == -1001
    assert call(D=96) == -1001 and b"head_dim 64 or 128" in lib.pc_last_error_string()
    assert call(H=6, Hkv=4) == -1001
    for kw in (dict(ns_own=0), dict(ns_own=33), dict(ns_trunk=0), dict(ns_trunk=33)):
        assert call(**kw) == -1001 and b"[1, 32]" in lib.pc_last_error_string(), kw
    assert call(leader=None) == -1001 and b"null pointer" in lib.pc_last_error_string()
    assert call(ptr=None) == -1001 and b"null pointer" in lib.pc_last_error_string()
    assert call(q_ts=4) == -1001 and b"alignment" in lib.pc_last_error_string()
    need = wsb(4, 3, 4, 128, 4, 2)
    assert call(ws_bytes=need - 1) == -1001 and b"workspace" in lib.pc_last_error_string()
    assert call(ws=p + 4, ws_bytes=need) == -1001 and b"workspace" in lib.pc_last_error_string()


def test_lookup_slot_loop_accepts_the_trunk_parameters_and_still_refuses():
    from promptcache_amd.model.llama_hip import LlamaHIP, LookupSlotLoop
    sig = inspect.signature(LlamaHIP.lookup_slot_loop).parameters
    assert sig["share_trunk"].default is False and sig["min_trunk"].default is None and sig["trunks"].default is None
    assert "trunks" in inspect.signature(LookupSlotLoop.__init__).parameters
    m = object.__new__(LlamaHIP)
    m.slot_loop_available = lambda: True
    m.lookup_available = lambda: True
    assert m.lookup_trunk_available() is True
    pasts = [object()] * 8
    kw = dict(share_trunk=True, min_trunk=1)
    assert m.lookup_slot_loop(pasts, [1] * 8, [5] * 8, 10, 8, [[]] * 8, **kw) is None          # 8 x 9 rows
    assert m.lookup_slot_loop(pasts[:5], [1] * 5, [5] * 5, 10, 8, [[]] * 5, **kw) is None      # 5 sequences take 8 slots: 8 x 9 rows
    assert m.lookup_slot_loop(pasts[:3], [1] * 3, [5] * 3, 10, 15, [[]] * 3, slots=8, **kw) is None
    assert m.lookup_slot_loop(pasts[:2], [1] * 2, [5] * 2, 10, 0, [[]] * 2, trunks=[(0, 5), (0, 5)]) is None
    m.lookup_available = lambda: False
    assert m.lookup_trunk_available() is False
    assert m.lookup_slot_loop(pasts[:1], [1], [5], 10, 3, [[]], **kw) is None


class _FakeHF:
    """A model with the batched loops' interface that offers the shared-trunk lookup step: records what generate_batch asks for."""

    def __init__(self, offers=True):
        self.asked = []
        self.offers = offers

    def slot_loop_available(self):
        return True

    def lookup_trunk_available(self):
        return self.offers

    def lookup_slot_loop(self, *a, **kw):
        self.asked.append(("lookup", kw.get("share_trunk")))
        return None

    def slot_loop(self, *a, **kw):
        self.asked.append(("slots", kw.get("share_trunk")))
        return None


def _fake_engine(offers=True):
    import torch
    from promptcache_amd.generation_engine import GenerationEngine
    hf = _FakeHF(offers)
    lm = types.SimpleNamespace(hf_model=hf, use_full_position_ids=False, decode=lambda ids: " ".join(map(str, ids)), device="cpu")
    ge = GenerationEngine(lm)

    def forward(ids, positions, past):
        logits = torch.zeros((1, len(ids), 16))
        logits[0, -1, 5] = 1.0
        return logits, past, 0.0
    ge._forward = forward
    return ge, hf


def _requests(n):
    arena = lambda: types.SimpleNamespace(B=1, layout=[])
    return [([1, 2, 3], [0, 1, 2], types.SimpleNamespace(arena=arena())) for _ in range(n)]


def test_generate_batch_asks_for_the_shared_lookup_loop_where_the_model_offers_it(monkeypatch):
    from promptcache_amd.generation_engine import GenerationParameters
    params = GenerationParameters(temperature=0.0, max_new_tokens=4)
    ge, hf = _fake_engine()
    # (the fake refuses both loops: what is checked is that no ValueError comes and what was asked, in which order)
    with pytest.raises(RuntimeError, match="refused a batched decode loop"):
        list(ge.generate_batch(_requests(2), params, lookup=3, share_trunk=True))
    assert hf.asked == [("lookup", True), ("slots", True)]
    # the environment knobs follow the same rule
    monkeypatch.setenv("PC_SLOT_TRUNK", "1")
    monkeypatch.setenv("PC_SLOT_LOOKUP", "3")
    ge, hf = _fake_engine()
    with pytest.raises(RuntimeError, match="refused a batched decode loop"):
        list(ge.generate_batch(_requests(2), params))
    assert hf.asked == [("lookup", True), ("slots", True)]
    # a model whose step is not available, and a batch that no device loop decodes: ValueError before anything is asked
    ge, hf = _fake_engine(offers=False)
    with pytest.raises(ValueError):
        next(ge.generate_batch(_requests(2), params))
    assert hf.asked == []
    ge, hf = _fake_engine()
    with pytest.raises(ValueError):
        next(ge.generate_batch(_requests(17), params))
    assert hf.asked == []
    # without share_trunk nothing changes
    monkeypatch.delenv("PC_SLOT_TRUNK")
    ge, hf = _fake_engine()
    with pytest.raises(RuntimeError):
        list(ge.generate_batch(_requests(2), params))
    assert hf.asked == [("lookup", False), ("slots", False)]
