"""CPU side of prompt-lookup drafts over int8 K / V images: the numpy reference of the step
(tests/lookup_slots_q8_ref.py) against ``lookup_slots_ref.verify_attend`` on rows on which the format is lossless, and on lossy
rows the property the mode stands on -- a draft row sees the step's earlier rows QUANTISED and its own row exact; the refusals of
``check_slot_kv`` with and without ``lookup_q8``, of ``serve`` / ``generate_batch`` / ``lookup_slot_loop``; the plans' strings; and
the argument errors of ``pc_rope_append_slots_rows_q8`` / ``pc_attn_verify_slots_q8`` that are answered before anything touches a
device (tests/test_slot_kv_only_cpu.py is the pattern)."""
import ctypes
import re

import numpy as np
import pytest

from tests import kv_q8_ref as q8
from tests import lookup_slots_q8_ref as ref
from tests import lookup_slots_ref as lsr
from tests.slot_kv_q8_ref import dequant32, lossless_rows
from tests.test_slot_kv_q8_cpu import _engine, _Hf

F32 = np.float32
D = 128


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,n,k", [(4, 4, 0, 0), (4, 2, 1, 3), (4, 2, 77, 7), (8, 1, 300, 3)])
def test_reference_equals_verify_attend_on_lossless_rows(H, Hkv, n, k):
    rng = np.random.default_rng(H * 100 + n + k)
    rows, codes, scale = lossless_rows(rng, (2, Hkv, n + k + 1), D)           # [k|v][Hkv][n + k + 1][D]
    q = (rng.standard_normal((k + 1, H, D)) * 0.5).astype(F32)
    got = ref.verify_attend_q8(q, codes[0], scale[0], codes[1], scale[1], rows[0][:, n:], rows[1][:, n:], n, k)
    want = lsr.verify_attend(q, rows[0], rows[1], n, k)
    assert got.shape == want.shape == (k + 1, H, D)
    assert float(np.abs(got - want).max()) < 1e-6


def test_a_draft_row_sees_earlier_rows_of_its_step_quantised_and_its_own_exact():
    rng = np.random.default_rng(9)
    H, Hkv, n, k = 4, 2, 20, 3
    img16, codes, scale = lossless_rows(rng, (2, Hkv, n), D)                  # the image in front of the step: exact
    new = (rng.standard_normal((2, Hkv, k + 1, D)) * 8).astype(np.float16)    # the step's rows: lossy, and as large as the image's
    nc, ns = q8.quantise(new)
    deq = dequant32(nc, ns)
    assert float(np.abs(deq - new.astype(F32)).max()) > 1e-3                  # (on the inputs: quantising them loses something)
    q = (rng.standard_normal((k + 1, H, D)) * 2.0).astype(F32)
    got = ref.verify_attend_q8(q, codes[0], scale[0], codes[1], scale[1], new[0], new[1], n, k)
    for i in range(k + 1):
        # row i, spelled out: image rows, the step's rows 0 .. i - 1 dequantised, row i as it is
        K = np.concatenate([img16[0].astype(F32), deq[0][:, :i], new[0][:, i:i + 1].astype(F32)], axis=1)
        V = np.concatenate([img16[1].astype(F32), deq[1][:, :i], new[1][:, i:i + 1].astype(F32)], axis=1)
        want = lsr.verify_attend(q[i:i + 1], K, V, n + i, 0)[0]
        assert float(np.abs(got[i] - want).max()) < 1e-12, i
    # ... which is neither "every fresh row exact" nor "every fresh row quantised" from row 1 on
    exact = lsr.verify_attend(q, np.concatenate([img16[0], new[0]], axis=1), np.concatenate([img16[1], new[1]], axis=1), n, k)
    allq = lsr.verify_attend(q, np.concatenate([img16[0].astype(F32), deq[0]], axis=1),
                             np.concatenate([img16[1].astype(F32), deq[1]], axis=1), n, k)
    assert float(np.abs(got[0] - exact[0]).max()) < 1e-12                     # row 0 has no earlier row of the step
    for i in range(1, k + 1):
        assert float(np.abs(got[i] - exact[i]).max()) > 1e-5 and float(np.abs(got[i] - allq[i]).max()) > 1e-5, i


def test_the_step_is_the_one_token_loop_whatever_the_step_boundaries():
    """Six tokens in one step (k = 5), or as 2 + 4, or one by one: the same outputs, because every row past the boundary has
    been quantised either way."""
    rng = np.random.default_rng(4)
    H, Hkv, n, T = 4, 2, 11, 6
    _, codes, scale = lossless_rows(rng, (2, Hkv, n), D)
    new = rng.standard_normal((2, Hkv, T, D)).astype(np.float16)
    q = rng.standard_normal((T, H, D)).astype(F32)

    def run(cuts):
        c, s, out, at = codes, scale, [], 0
        for m in cuts:                                                         # a step of m rows, then its rows join the image
            out.append(ref.verify_attend_q8(q[at:at + m], c[0], s[0], c[1], s[1], new[0][:, at:at + m], new[1][:, at:at + m], n + at, m - 1))
            nc, ns = q8.quantise(new[:, :, at:at + m])
            c, s = np.concatenate([c, nc], axis=2), np.concatenate([s, ns], axis=2)
            at += m
        return np.concatenate(out)
    whole = run([6])
    assert np.array_equal(whole, run([2, 4])) and np.array_equal(whole, run([1] * 6))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_check_slot_kv_with_and_without_lookup_q8():
    from promptcache_amd.model.llama_hip import check_slot_kv
    for kw in (dict(), dict(lookup_q8=False)):
        with pytest.raises(ValueError, match="lookup > 0 exclude each other"):
            check_slot_kv("int8", lookup=3, head_dim=128, **kw)
    assert check_slot_kv("int8", lookup=3, head_dim=128, lookup_q8=True) is None
    assert check_slot_kv("int8", lookup=0, lookup_q8=True) is None and check_slot_kv("fp16", lookup=3, lookup_q8=True) is None
    # the keyword lifts that one refusal only
    for kw, word in ((dict(share_trunk=True), "share_trunk"), (dict(head_dim=64), "head_dim"), (dict(no_loop="x"), "does not have"),
                     (dict(not_batched="y"), "is not: y")):
        with pytest.raises(ValueError, match=word):
            check_slot_kv("int8", lookup=3, lookup_q8=True, **kw)


class _HfLookup(_Hf):
    """A model stub with the lookup step; ``q8``: whether it says ``lookup_slot_q8_available``."""

    def __init__(self, q8_step):
        super().__init__()
        if q8_step is not None:
            self.lookup_slot_q8_available = lambda: q8_step

    def lookup_available(self):
        return True

    def lookup_slot_loop(self, *a, **k):
        raise AssertionError("no request: no loop is built")


class _Slots:
    slots = 2
    max_ctx_length = 2048


def test_serve_takes_the_mode_where_the_model_has_the_step_and_generate_batch_keeps_refusing(monkeypatch):
    from promptcache_amd.generation_engine import GenerationParameters
    for name in ("PC_SLOT_KV", "PC_SLOT_KEEP_ARENAS", "PC_SERVE_LOOKUP", "PC_SLOT_LOOKUP", "PC_SLOT_TRUNK"):
        monkeypatch.delenv(name, raising=False)
    params = GenerationParameters(temperature=0.0, max_new_tokens=8)
    reqs = [([1, 2], [0, 1], object())] * 2
    for hf in (_Hf(), _HfLookup(None), _HfLookup(False)):                     # no such method, or it says no
        with pytest.raises(ValueError, match="lookup > 0 exclude each other"):
            next(_engine(hf).serve(None, [], params, slot_kv="int8", lookup=2))
    ge = _engine(_HfLookup(True))
    for kw in (dict(), dict(keep_arenas=False), dict(keep_arenas=True)):
        assert list(ge.serve(_Slots(), [], params, slot_kv="int8", lookup=2, **kw)) == []
    monkeypatch.setenv("PC_SLOT_KV", "int8")                                  # the environment asks for the same mode
    monkeypatch.setenv("PC_SERVE_LOOKUP", "3")
    monkeypatch.setenv("PC_SLOT_KEEP_ARENAS", "0")
    assert list(ge.serve(_Slots(), [], params)) == []
    with pytest.raises(ValueError, match="lookup > 0 exclude each other"):
        next(_engine(_Hf()).serve(None, [], params))
    for name in ("PC_SLOT_KV", "PC_SERVE_LOOKUP", "PC_SLOT_KEEP_ARENAS"):
        monkeypatch.delenv(name)
    # the other refusals stand
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.serve(None, [], params, slot_kv="int8", lookup=2, share_trunk=True))
    with pytest.raises(ValueError, match="needs slot_kv='int8'"):
        next(ge.serve(None, [], params, lookup=2, keep_arenas=False))
    # generate_batch: its callers hand in live arenas, and the combination stays refused there
    with pytest.raises(ValueError, match="lookup > 0 exclude each other"):
        next(ge.generate_batch(reqs, params, slot_kv="int8", lookup=3))
    with pytest.raises(ValueError, match="generate_batch.*nothing to save"):
        next(ge.generate_batch(reqs, params, lookup=3, keep_arenas=False))


def test_lookup_slot_loop_refuses_before_anything_is_built():
    from promptcache_amd.model.llama_hip import LlamaHIP

    class M:
        D = 128
        slot_loop_available = lambda self: True
        lookup_available = lambda self: (_ for _ in ()).throw(AssertionError("the refusal comes first"))
        lookup_slot_q8_available = lambda self: True

    with pytest.raises(ValueError, match="share_trunk"):
        LlamaHIP.lookup_slot_loop(M(), [], [], [], 4, 3, [], kv="int8", share_trunk=True)
    with pytest.raises(ValueError, match="share_trunk"):
        LlamaHIP.lookup_slot_loop(M(), [], [], [], 4, 3, [], kv="int8", trunks=[(None, 0)])
    with pytest.raises(ValueError, match="needs slot_kv='int8'"):
        LlamaHIP.lookup_slot_loop(M(), [], [], [], 4, 3, [], keep_arenas=False)
    with pytest.raises(ValueError, match="must be one of"):
        LlamaHIP.lookup_slot_loop(M(), [], [], [], 4, 3, [], kv="fp8")
    no = M()
    no.lookup_slot_q8_available = lambda: False
    with pytest.raises(ValueError, match="lookup > 0 exclude each other"):
        LlamaHIP.lookup_slot_loop(no, [], [], [], 4, 3, [], kv="int8")
    hd64 = M()
    hd64.D = 64
    with pytest.raises(ValueError, match="head_dim"):
        LlamaHIP.lookup_slot_loop(hd64, [], [], [], 4, 3, [], kv="int8")


def test_loop_classes_share_the_host_side():
    from promptcache_amd.model import llama_hip as lh
    assert lh.LookupSlotLoopQ8.kv == "int8" and issubclass(lh.LookupSlotLoopQ8Only, lh.LookupSlotLoopQ8)
    assert issubclass(lh.LookupSlotLoopQ8, lh.LookupSlotLoop) and lh.LookupSlotLoop.kv == "fp16"
    # one _quantise_entry / _image_rows for the loops whose images follow the sequences, one seat for the loops without arenas
    assert lh.LookupSlotLoopQ8._quantise_entry is lh.SlotLoopQ8Only._quantise_entry is lh.LookupSlotLoopQ8Only._quantise_entry
    assert lh.LookupSlotLoopQ8Only._seat is lh.SlotLoopQ8Only._seat and lh.LookupSlotLoopQ8Only._prepared is lh.SlotLoopQ8Only._prepared
    assert lh.SlotLoopQ8._quantise_entry is lh._SlotLoopHost._quantise_entry
    assert lh.LookupSlotLoop.slot_kv_bytes is lh.SlotLoop.slot_kv_bytes

    class A:
        def __init__(self, length):
            self.length = length
    for cls, k in ((lh.SlotLoopQ8Only, 0), (lh.LookupSlotLoopQ8, 3), (lh.LookupSlotLoopQ8Only, 7)):
        loop = cls.__new__(cls)
        loop.k = k
        assert loop._image_rows([A(100), A(40)], [5, 90], None) == 40 + 90 + k + 2
        assert loop._image_rows([A(100), A(40)], [5, 90], 2048) == 2048


def test_plans_name_every_mode_and_are_unchanged_without_the_arguments(monkeypatch):
    for name in ("PC_SLOT_KV", "PC_SLOT_KEEP_ARENAS"):
        monkeypatch.delenv(name, raising=False)
    ge = _engine(_HfLookup(True))
    look = ge.serve_plan(3, 4)
    assert look == (True, "one device loop with prompt-lookup drafts (lookup, k = 3): up to k + 1 tokens per sequence and replay, "
                          "new prompts admitted as slots free up")
    q8p = ge.serve_plan(3, 4, slot_kv="int8")
    assert q8p == (True, look[1] + ", K/V read from int8 images (slot_kv='int8')")
    only = ge.serve_plan(3, 4, slot_kv="int8", keep_arenas=False)
    assert only[0] and only[1].startswith(q8p[1]) and "keep_arenas=False" in only[1]
    for word in ("lookup, k = 3", "slot_kv='int8'", "keep_arenas=False"):
        assert word in only[1]
    # where the 64 rows do not fit the one-token loop runs, over images all the same
    wide = ge.serve_plan(7, 16, slot_kv="int8", keep_arenas=False)
    assert wide[0] and "one token per replay" in wide[1] and "64 rows" in wide[1] and "slot_kv='int8'" in wide[1]
    assert ge.serve_plan(3, 4, slot_kv="fp16") == look and ge.serve_plan(3, 4, keep_arenas=False) == look


# ---- argument errors of the entry points -----------------------------------------------------------------------------------------
A = 0x10000          # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch


def test_entries_are_declared_and_mirrored():
    from promptcache_amd import _native
    lib = _native.load()
    rt, at = _native.SIGNATURES["pc_rope_append_slots_rows_q8"]
    parent = _native.SIGNATURES["pc_rope_append_slots_rows"][1]
    assert rt is ctypes.c_int and at[:len(parent) - 1] == parent[:-1] and len(at) == len(parent) + 4
    rt, at = _native.SIGNATURES["pc_attn_verify_slots_q8"]
    parent = _native.SIGNATURES["pc_attn_verify_slots"][1]
    assert rt is ctypes.c_int and at[:len(parent) - 1] == parent[:-1] and len(at) == len(parent) + 4
    for name in ("pc_rope_append_slots_rows_q8", "pc_attn_verify_slots_q8", "pc_attn_verify_slots_q8_workspace_bytes"):
        assert hasattr(lib, name) and callable(getattr(_native, name[3:]))
    # one record more per (row, head) than the fp16 entry
    assert _native.attn_verify_slots_q8_workspace_bytes(3, 3, 4, 128, 2) == _native.attn_verify_slots_workspace_bytes(3, 3, 4, 128, 3)
    assert _native.attn_verify_slots_q8_workspace_bytes(0, 3, 4, 128, 2) == 0


WS = 4 * 4 * 4 * 3 * 130 * 4       # S (k + 1) H (nsplit + 1) (D + 2) floats


@pytest.mark.parametrize("kw,word", [
    (dict(D=64), "head_dim must be 128"), (dict(D=32), "head_dim must be 128"), (dict(H=4, Hkv=3), "multiple of Hkv"),
    (dict(q_hi=None), "null"), (dict(q_lo=None), "null"), (dict(kv_base=None), "null"), (dict(cap=None), "null"), (dict(len=None), "null"),
    (dict(live=None), "null"), (dict(ws=None), "null"), (dict(of_hi=None), "null"), (dict(of_lo=None), "null"),
    (dict(kvq_base=None), "null"), (dict(S=0), "1 <= S <= 16"), (dict(S=17), "1 <= S <= 16"), (dict(k=-1), "0 <= k <= 15"),
    (dict(k=16), "0 <= k <= 15"), (dict(S=16, k=4), r"S \* \(k \+ 1\) <= 64"), (dict(qcap=0), "qcap"), (dict(qcap=-5), "qcap"),
    (dict(n_layers=0), "n_layers"), (dict(layer=2, n_layers=2), "n_layers"), (dict(layer=-1), "1 <= S <= 16"),
    (dict(nsplit=0), r"\[1, 32\]"), (dict(nsplit=33), r"\[1, 32\]"), (dict(ws_bytes=WS - 4), "workspace"),
    (dict(ws_bytes=4 * 4 * 4 * 2 * 130 * 4), "workspace"),                     # (pc_attn_verify_slots' size: the exact record is missing)
    (dict(ws=A + 8), "workspace"), (dict(q_ts=516), "alignment"), (dict(q_ts=504), "alignment"), (dict(q_hi=A + 8), "alignment"),
    (dict(fresh=2), "fresh"), (dict(fresh=-1), "fresh"),
])
def test_attn_verify_slots_q8_argument_errors_need_no_gpu(kw, word):
    from promptcache_amd import _native
    lib = _native.load()
    f = dict(q_hi=A, q_lo=A, q_ts=512, kv_base=A, cap=A, len=A, live=A, S=4, k=3, layer=1, H=4, Hkv=2, D=128, nsplit=2, ws=A,
             ws_bytes=WS, of_hi=A, of_lo=A, kvq_base=A, qcap=1024, n_layers=2, fresh=0)
    f.update(kw)
    rc = lib.pc_attn_verify_slots_q8(f["q_hi"], f["q_lo"], f["q_ts"], f["kv_base"], f["cap"], f["len"], f["live"], f["S"], f["k"],
                                     f["layer"], f["H"], f["Hkv"], f["D"], 0.088, f["nsplit"], f["ws"], f["ws_bytes"], f["of_hi"],
                                     f["of_lo"], f["kvq_base"], f["qcap"], f["n_layers"], f["fresh"], None)
    assert rc == -1001, rc
    msg = lib.pc_last_error_string().decode()
    assert "pc_attn_verify_slots_q8" in msg and re.search(word, msg), msg


@pytest.mark.parametrize("kw,word", [
    (dict(D=64), "head_dim must be 128"), (dict(D=256), "head_dim must be 128"), (dict(D=0), "head_dim must be 128"),
    (dict(S=0), "1 <= S <= 16"), (dict(S=17), "1 <= S <= 16"), (dict(k=-1), "0 <= k <= 15"), (dict(k=16), "0 <= k <= 15"),
    (dict(S=16, k=4), "S * (k + 1) <= 64"), (dict(S=8, k=8), "S * (k + 1) <= 64"), (dict(layer=-1), "bad sizes"), (dict(H=0), "bad sizes"),
    (dict(Hkv=0), "bad sizes"),
    (dict(qkv=None), "null"), (dict(q_hi=None), "null"), (dict(q_lo=None), "null"), (dict(cs=None), "null"), (dict(kv_base=None), "null"),
    (dict(cap=None), "null"), (dict(len=None), "null"), (dict(live=None), "null"), (dict(kvq_base=None), "null"),
    (dict(in_layout=2), "in_layout"), (dict(in_layout=-1), "in_layout"), (dict(fresh=2), "fresh"), (dict(fresh=-1), "fresh"),
    (dict(qcap=0), "qcap"), (dict(qcap=-1), "qcap"), (dict(n_layers=0), "n_layers"), (dict(layer=2), "n_layers"), (dict(layer=7), "n_layers"),
    (dict(ld=1020), "alignment"), (dict(ld=1026), "alignment"), (dict(q_ts=516), "alignment"), (dict(qkv=A + 4), "alignment"),
    (dict(q_hi=A + 8), "alignment"), (dict(q_lo=A + 2), "alignment"),
])
def test_rope_append_slots_rows_q8_argument_errors_need_no_gpu(kw, word):
    from promptcache_amd import _native
    lib = _native.load()
    f = dict(qkv=A, ld=1024, in_layout=1, q_hi=A, q_lo=A, q_ts=512, cs=A, kv_base=A, cap=A, len=A, live=A, S=4, k=3, layer=1, H=4, Hkv=2,
             D=128, kvq_base=A, qcap=1024, n_layers=2, fresh=1)
    f.update(kw)
    rc = lib.pc_rope_append_slots_rows_q8(f["qkv"], f["ld"], f["in_layout"], f["q_hi"], f["q_lo"], f["q_ts"], f["cs"], f["kv_base"], f["cap"],
                                          f["len"], f["live"], f["S"], f["k"], f["layer"], f["H"], f["Hkv"], f["D"], f["kvq_base"],
                                          f["qcap"], f["n_layers"], f["fresh"], None)
    assert rc == -1001, rc
    msg = lib.pc_last_error_string().decode()
    assert "pc_rope_append_slots_rows_q8" in msg and word in msg, msg
