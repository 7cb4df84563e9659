"""CPU side of the int8-only slot residency (``keep_arenas=False``): the refusals of ``check_slot_keep_arenas`` and of
the engine's ``keep_arenas`` argument, the plans' strings, and the argument errors of ``pc_rope_append_slots_q8`` /
``pc_attn_decode_slots_q8_fresh`` that are answered before anything touches a device (tests/test_slot_kv_q8_cpu.py is the pattern)."""
import ctypes
import re

import pytest

from tests.test_slot_kv_q8_cpu import _engine, _Hf


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_check_slot_keep_arenas_refusals():
    from promptcache_amd.model.llama_hip import check_slot_keep_arenas, parse_keep_arenas
    for ok in ((True, "fp16"), (True, "int8"), (False, "int8")):
        assert check_slot_keep_arenas(*ok) is None
    assert check_slot_keep_arenas(True, "fp16", generate_batch=True) is None
    with pytest.raises(ValueError, match="needs slot_kv='int8'"):
        check_slot_keep_arenas(False, "fp16")
    for kv in ("fp16", "int8"):
        with pytest.raises(ValueError, match="generate_batch.*nothing to save"):
            check_slot_keep_arenas(False, kv, generate_batch=True)
    assert parse_keep_arenas(None) and parse_keep_arenas("") and parse_keep_arenas("1") and not parse_keep_arenas("0")
    with pytest.raises(ValueError, match="PC_SLOT_KEEP_ARENAS"):
        parse_keep_arenas("no")


def test_engine_refuses_the_mode_before_anything_is_asked_of_the_model(monkeypatch):
    from promptcache_amd.generation_engine import GenerationParameters
    monkeypatch.delenv("PC_SLOT_KV", raising=False)
    monkeypatch.delenv("PC_SLOT_KEEP_ARENAS", raising=False)
    params = GenerationParameters(temperature=0.0, max_new_tokens=8)
    ge = _engine(_Hf())
    reqs = [([1, 2], [0, 1], object())] * 2
    # without the images the arenas are all a slot has
    with pytest.raises(ValueError, match="needs slot_kv='int8'"):
        next(ge.serve(None, [], params, keep_arenas=False))
    with pytest.raises(ValueError, match="needs slot_kv='int8'"):
        next(ge.serve(None, [], params, slot_kv="fp16", keep_arenas=False))
    # generate_batch: N live arenas come in
    with pytest.raises(ValueError, match="generate_batch.*nothing to save"):
        next(ge.generate_batch(reqs, params, keep_arenas=False))
    # wherever check_slot_kv refuses int8, with its words
    with pytest.raises(ValueError, match="lookup"):
        next(ge.serve(None, [], params, slot_kv="int8", keep_arenas=False, lookup=2))
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.serve(None, [], params, slot_kv="int8", keep_arenas=False, share_trunk=True))
    with pytest.raises(ValueError, match="batch-1 arena"):
        next(ge.generate_batch(reqs, params, slot_kv="int8", keep_arenas=False))
    none = _engine(_Hf(available=False))
    with pytest.raises(ValueError, match="no batched decode loop"):
        next(none.serve(None, [], params, slot_kv="int8", keep_arenas=False))
    hd64 = _Hf()
    hd64.D = 64
    with pytest.raises(ValueError, match="head_dim"):
        next(_engine(hd64).serve(None, [], params, slot_kv="int8", keep_arenas=False))
    # the environment asks for the same refusal; generate_batch does not read it
    monkeypatch.setenv("PC_SLOT_KEEP_ARENAS", "0")
    with pytest.raises(ValueError, match="needs slot_kv='int8'"):
        next(ge.serve(None, [], params))
    with pytest.raises(ValueError, match="batch-1 arena"):
        next(ge.generate_batch(reqs, params, slot_kv="int8"))
    monkeypatch.setenv("PC_SLOT_KEEP_ARENAS", "2")
    with pytest.raises(ValueError, match="PC_SLOT_KEEP_ARENAS"):
        next(ge.serve(None, [], params, slot_kv="int8"))


def test_slot_loop_refuses_the_mode_without_int8():
    from promptcache_amd.model.llama_hip import LlamaHIP

    class M:
        D = 128
        slot_loop_available = lambda self: True
        _slot_loop_front = lambda self, *a: (_ for _ in ()).throw(AssertionError("the refusal comes first"))
    with pytest.raises(ValueError, match="needs slot_kv='int8'"):
        LlamaHIP.slot_loop(M(), [], [], [], 4, keep_arenas=False)
    with pytest.raises(ValueError, match="share_trunk"):
        LlamaHIP.slot_loop(M(), [], [], [], 4, kv="int8", keep_arenas=False, share_trunk=True)


def test_plans_name_the_mode_and_are_unchanged_without_the_argument(monkeypatch):
    from promptcache_amd.generation_engine import GenerationParameters
    monkeypatch.delenv("PC_SLOT_KV", raising=False)
    monkeypatch.delenv("PC_SLOT_KEEP_ARENAS", raising=False)
    params = GenerationParameters(temperature=0.0, max_new_tokens=8)
    ge = _engine(_Hf())
    assert ge.batch_plan(4, params) == (True, "one device loop over all sequences")
    assert ge.batch_plan(4, params, slot_kv="int8") == (True, "one device loop over all sequences, K/V read from int8 images (slot_kv='int8')")
    assert ge.serve_plan() == (True, "one device loop, new prompts admitted as slots free up")
    q8 = ge.serve_plan(slot_kv="int8")
    assert q8 == (True, "one device loop, new prompts admitted as slots free up, K/V read from int8 images (slot_kv='int8')")
    assert ge.serve_plan(slot_kv="int8", keep_arenas=True) == q8 and ge.serve_plan(keep_arenas=True) == ge.serve_plan()
    only = ge.serve_plan(slot_kv="int8", keep_arenas=False)
    assert only[0] and only[1].startswith(q8[1]) and "keep_arenas=False" in only[1] and "one shared arena" in only[1]
    monkeypatch.setenv("PC_SLOT_KEEP_ARENAS", "0")              # (the strings follow the argument only)
    assert ge.serve_plan(slot_kv="int8") == q8
    no = _engine(_Hf(available=False))
    assert no.serve_plan(slot_kv="int8", keep_arenas=False) == no.serve_plan()


# ---- argument errors of the entry points -------------------------------------------------------------------------------------
A = 0x10000          # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch


def test_entries_are_declared_and_mirrored():
    from promptcache_amd import _native
    lib = _native.load()
    rt, at = _native.SIGNATURES["pc_attn_decode_slots_q8_fresh"]
    assert rt is ctypes.c_int and at == _native.SIGNATURES["pc_attn_decode_slots_q8"][1]
    rt, at = _native.SIGNATURES["pc_rope_append_slots_q8"]
    parent = _native.SIGNATURES["pc_rope_append_slots"][1]
    assert rt is ctypes.c_int and at[:len(parent) - 1] == parent[:-1] and len(at) == len(parent) + 3
    for name in ("pc_attn_decode_slots_q8_fresh", "pc_rope_append_slots_q8"):
        assert hasattr(lib, name) and callable(getattr(_native, name[3:]))


@pytest.mark.parametrize("kw,word", [
    (dict(D=64), "head_dim must be 128"), (dict(D=32), "head_dim must be 128"), (dict(H=4, Hkv=3), "multiple of Hkv"),
    (dict(q_hi=None), "null"), (dict(q_lo=None), "null"), (dict(kv_base=None), "null"), (dict(cap=None), "null"), (dict(len=None), "null"),
    (dict(live=None), "null"), (dict(ws=None), "null"), (dict(of_hi=None), "null"), (dict(of_lo=None), "null"),
    (dict(kvq_base=None), "null"), (dict(S=0), "1 <= S <= 16"), (dict(S=17), "1 <= S <= 16"), (dict(qcap=0), "qcap"),
    (dict(qcap=-5), "qcap"), (dict(n_layers=0), "n_layers"), (dict(layer=2, n_layers=2), "n_layers"), (dict(layer=-1), "1 <= S <= 16"),
    (dict(nsplit=0), r"\[1, 32\]"), (dict(nsplit=33), r"\[1, 32\]"), (dict(ws_bytes=4 * 4 * 2 * 130 * 4 - 4), "workspace"),
    (dict(q_ts=516), "alignment"),
])
def test_attn_decode_slots_q8_fresh_argument_errors_need_no_gpu(kw, word):
    from promptcache_amd import _native
    lib = _native.load()
    f = dict(q_hi=A, q_lo=A, q_ts=512, kv_base=A, cap=A, len=A, live=A, S=4, layer=1, H=4, Hkv=2, D=128, nsplit=2, ws=A,
             ws_bytes=4 * 4 * 2 * 130 * 4, of_hi=A, of_lo=A, kvq_base=A, qcap=1024, n_layers=2)
    f.update(kw)
    rc = lib.pc_attn_decode_slots_q8_fresh(f["q_hi"], f["q_lo"], f["q_ts"], f["kv_base"], f["cap"], f["len"], f["live"], f["S"],
                                           f["layer"], f["H"], f["Hkv"], f["D"], 0.088, f["nsplit"], f["ws"], f["ws_bytes"], f["of_hi"],
                                           f["of_lo"], f["kvq_base"], f["qcap"], f["n_layers"], None)
    assert rc == -1001, rc
    msg = lib.pc_last_error_string().decode()
    assert "pc_attn_decode_slots_q8_fresh" in msg and re.search(word, msg), msg


@pytest.mark.parametrize("kw,word", [
    (dict(D=64), "head_dim must be 128"), (dict(D=256), "head_dim must be 128"), (dict(D=0), "head_dim must be 128"),
    (dict(S=0), "1 <= S <= 16"), (dict(S=17), "1 <= S <= 16"), (dict(layer=-1), "bad sizes"), (dict(H=0), "bad sizes"),
    (dict(Hkv=0), "bad sizes"),
    (dict(qkv=None), "null"), (dict(q_hi=None), "null"), (dict(q_lo=None), "null"), (dict(cs=None), "null"), (dict(kv_base=None), "null"),
    (dict(cap=None), "null"), (dict(len=None), "null"), (dict(live=None), "null"), (dict(kvq_base=None), "null"),
    (dict(in_layout=2), "in_layout"), (dict(in_layout=-1), "in_layout"),
    (dict(qcap=0), "qcap"), (dict(qcap=-1), "qcap"), (dict(n_layers=0), "n_layers"), (dict(layer=2), "n_layers"), (dict(layer=7), "n_layers"),
    (dict(ld=1020), "alignment"), (dict(ld=1026), "alignment"), (dict(q_ts=516), "alignment"), (dict(qkv=A + 4), "alignment"),
    (dict(q_hi=A + 8), "alignment"), (dict(q_lo=A + 2), "alignment"),
])
def test_rope_append_slots_q8_argument_errors_need_no_gpu(kw, word):
    from promptcache_amd import _native
    lib = _native.load()
    f = dict(qkv=A, ld=1024, in_layout=1, q_hi=A, q_lo=A, q_ts=512, cs=A, kv_base=A, cap=A, len=A, live=A, S=4, layer=1, H=4, Hkv=2,
             D=128, kvq_base=A, qcap=1024, n_layers=2)
    f.update(kw)
    rc = lib.pc_rope_append_slots_q8(f["qkv"], f["ld"], f["in_layout"], f["q_hi"], f["q_lo"], f["q_ts"], f["cs"], f["kv_base"], f["cap"],
                                     f["len"], f["live"], f["S"], f["layer"], f["H"], f["Hkv"], f["D"], f["kvq_base"], f["qcap"],
                                     f["n_layers"], None)
    assert rc == -1001, rc
    msg = lib.pc_last_error_string().decode()
    assert "pc_rope_append_slots_q8" in msg and word in msg, msg
