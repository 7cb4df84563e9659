"""CPU side of the int8 slot K/V mode: the numpy reference of pc_attn_decode_slots_q8 on rows on which the format
is lossless, the refusals of ``check_slot_kv`` and of the engine's ``slot_kv`` argument, and the argument errors of the two new
entry points that are answered before anything touches a device (tests/test_w4_expand_abi_cpu.py is the pattern)."""
import ctypes

import numpy as np
import pytest

from tests import kv_q8_ref as q8
from tests import slot_kv_q8_ref as ref
from tests import slots_ref

F32 = np.float32


# ---- the reference on lossless rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,n", [(4, 4, 0), (4, 2, 1), (4, 2, 77), (8, 1, 300)])
def test_reference_equals_attend_slot_on_lossless_rows(H, Hkv, n):
    rng = np.random.default_rng(H * 100 + n)
    D = 128
    rows, codes, scale = ref.lossless_rows(rng, (2, Hkv, n + 1), D)           # [k|v][Hkv][n + 1][D]
    q = (rng.standard_normal((H, D)) * 0.5).astype(F32)
    got = ref.attend(q, codes[0][:, :n], scale[0][:, :n], codes[1][:, :n], scale[1][:, :n], rows[0][:, n], rows[1][:, n])
    want = slots_ref.attend_slot(q, rows[0], rows[1])
    err = float(np.abs(got - want).max())
    print(f"[slot_kv_q8_ref H={H} Hkv={Hkv} n={n}] max|d| vs attend_slot on the fp16 rows = {err:.2e}")
    assert err <= 1e-6


def test_quantise_is_exact_on_lossless_rows_and_append_places_the_row():
    rng = np.random.default_rng(5)
    rows, codes, scale = ref.lossless_rows(rng, (3, 40), 128)
    c, s = q8.quantise(rows)
    assert np.array_equal(c, codes) and np.array_equal(s.view(np.uint32), scale.view(np.uint32))
    image = (codes[:, :39], scale[:, :39])
    c2, s2 = ref.append(image, rows[:, 39])
    assert c2.shape == (3, 40, 128) and np.array_equal(c2, codes) and np.array_equal(s2.view(np.uint32), scale.view(np.uint32))
    bad = rows[:, 0].copy()
    bad[1, 17] = np.inf
    c3, s3 = ref.append(image, bad)
    assert np.isnan(s3[1, 39]) and not c3[1, 39].any() and np.array_equal(c3[0, 39], codes[0, 0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_check_slot_kv_refusals():
    from promptcache_amd.model.llama_hip import check_slot_kv
    for ok in (dict(kv="fp16"), dict(kv="fp16", share_trunk=True, lookup=3, head_dim=64, no_loop="x", not_batched="y"),
               dict(kv="int8"), dict(kv="int8", head_dim=128)):
        assert check_slot_kv(**ok) is None
    for kw, word in [(dict(kv="fp8"), "must be one of"), (dict(kv=None), "must be one of"),
                     (dict(kv="int8", share_trunk=True), "share_trunk"), (dict(kv="int8", lookup=3), "lookup"),
                     (dict(kv="int8", head_dim=64), "head_dim"),
                     (dict(kv="int8", no_loop="architecture, int8 weights or PC_DECODE_TAIL=1"), "PC_DECODE_TAIL=1"),
                     (dict(kv="int8", not_batched="more than 16 requests"), "more than 16 requests")]:
        with pytest.raises(ValueError, match=word):
            check_slot_kv(**kw)


class _Hf:
    D = 128

    def __init__(self, available=True):
        self.available = available

    def slot_loop_available(self):
        return self.available

    def slot_loop(self, *a, **k):
        raise AssertionError("the refusal comes before anything is asked of the model")


class _Lm:
    use_full_position_ids = False

    def __init__(self, hf):
        self.hf_model = hf


def _engine(hf):
    from promptcache_amd.generation_engine import GenerationEngine
    ge = GenerationEngine.__new__(GenerationEngine)
    ge.lm, ge.device_greedy_loop, ge.device_sample_loop, ge.lookup, ge.lookup_sampled = _Lm(hf), True, True, 0, False
    return ge


def test_engine_refuses_int8_where_the_loop_cannot_run_it_and_plans_report_the_mode(monkeypatch):
    from promptcache_amd.generation_engine import GenerationParameters
    monkeypatch.delenv("PC_SLOT_KV", raising=False)
    params = GenerationParameters(temperature=0.0, max_new_tokens=8)
    ge = _engine(_Hf())
    plain = ge.batch_plan(4, params)
    assert plain == (True, "one device loop over all sequences") and ge.batch_plan(4, params, slot_kv="fp16") == plain
    assert ge.batch_plan(4, params, slot_kv="int8") == (True, plain[1] + ", K/V read from int8 images (slot_kv='int8')")
    assert ge.batch_plan(17, params, slot_kv="int8") == ge.batch_plan(17, params)
    assert ge.serve_plan() == ge.serve_plan(slot_kv="fp16") and "int8" not in ge.serve_plan()[1]
    assert ge.serve_plan(slot_kv="int8")[1].endswith("K/V read from int8 images (slot_kv='int8')")
    monkeypatch.setenv("PC_SLOT_KV", "int8")
    assert "int8" in ge.batch_plan(4, params)[1] and "int8" in ge.serve_plan()[1]
    monkeypatch.delenv("PC_SLOT_KV")
    reqs = [([1, 2], [0, 1], object())] * 2
    for kw, word in [(dict(slot_kv="int8", share_trunk=True), "share_trunk"), (dict(slot_kv="int8", lookup=3), "lookup"),
                     (dict(slot_kv="fp8"), "must be one of"), (dict(slot_kv="int8"), "batch-1 arena")]:
        with pytest.raises(ValueError, match=word):
            next(ge.generate_batch(reqs, params, **kw))
    with pytest.raises(ValueError, match="more than 16 requests"):
        next(ge.generate_batch(reqs * 9, params, slot_kv="int8"))
    with pytest.raises(ValueError, match="lookup"):
        next(ge.serve(None, [], params, slot_kv="int8", lookup=2))
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.serve(None, [], params, slot_kv="int8", share_trunk=True))
    none = _engine(_Hf(available=False))                       # Falcon / MPT / load_in_8bit / PC_DECODE_TAIL=1
    with pytest.raises(ValueError, match="no batched decode loop"):
        next(none.generate_batch(reqs, params, slot_kv="int8"))
    with pytest.raises(ValueError, match="no batched decode loop"):
        next(none.serve(None, [], params, slot_kv="int8"))
    monkeypatch.setenv("PC_SLOT_KV", "int8")                    # the environment asks for the same refusals
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.generate_batch(reqs, params, share_trunk=True))


# ---- argument errors of the entry points -------------------------------------------------------------------------------------
A = 0x10000          # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch


def test_entries_are_declared_and_mirrored():
    from promptcache_amd import _native
    lib = _native.load()
    rt, at = _native.SIGNATURES["pc_kv_quant_q8_rows"]
    assert rt is ctypes.c_int and len(at) == 8 and hasattr(lib, "pc_kv_quant_q8_rows") and callable(_native.kv_quant_q8_rows)
    rt, at = _native.SIGNATURES["pc_attn_decode_slots_q8"]
    assert rt is ctypes.c_int and len(at) == len(_native.SIGNATURES["pc_attn_decode_slots"][1]) + 3
    assert hasattr(lib, "pc_attn_decode_slots_q8") and callable(_native.attn_decode_slots_q8)


@pytest.mark.parametrize("kw,word", [
    (dict(n_rows=-1), "bad sizes"), (dict(n_planes=0), "bad sizes"), (dict(src_plane_rows=76), "bad sizes"),
    (dict(dst_plane_rows=76), "bad sizes"), (dict(n_rows=0, src_plane_rows=0, dst_plane_rows=0), "bad sizes"),
    (dict(head_dim=48), "head_dim"), (dict(head_dim=256), "head_dim"),
    (dict(src=None), "null"), (dict(dst=None), "null"), (dict(src=A + 8), "aligned"), (dict(dst=A + 4), "aligned"),
])
def test_kv_quant_q8_rows_argument_errors_need_no_gpu(kw, word):
    from promptcache_amd import _native
    lib = _native.load()
    f = dict(src=A, src_plane_rows=1024, n_rows=77, n_planes=8, head_dim=128, dst=A, dst_plane_rows=1536)
    f.update(kw)
    rc = lib.pc_kv_quant_q8_rows(f["src"], f["src_plane_rows"], f["n_rows"], f["n_planes"], f["head_dim"], f["dst"], f["dst_plane_rows"],
                                 None)
    assert rc == -1001, rc
    msg = lib.pc_last_error_string().decode()
    assert "pc_kv_quant_q8_rows" in msg and word in msg, msg


def test_kv_quant_q8_rows_of_no_rows_is_a_no_op():
    from promptcache_amd import _native
    assert _native.load().pc_kv_quant_q8_rows(None, 1024, 0, 8, 128, None, 1536, None) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(D=64), "head_dim must be 128"), (dict(D=32), "head_dim must be 128"), (dict(H=4, Hkv=3), "multiple of Hkv"),
    (dict(q_hi=None), "null"), (dict(q_lo=None), "null"), (dict(kv_base=None), "null"), (dict(cap=None), "null"), (dict(len=None), "null"),
    (dict(live=None), "null"), (dict(ws=None), "null"), (dict(of_hi=None), "null"), (dict(of_lo=None), "null"),
    (dict(kvq_base=None), "null"), (dict(S=0), "1 <= S <= 16"), (dict(S=17), "1 <= S <= 16"), (dict(qcap=0), "qcap"),
    (dict(qcap=-5), "qcap"), (dict(n_layers=0), "n_layers"), (dict(layer=2, n_layers=2), "n_layers"), (dict(layer=-1), "1 <= S <= 16"),
    (dict(nsplit=0), r"\[1, 32\]"), (dict(nsplit=33), r"\[1, 32\]"), (dict(ws_bytes=4 * 4 * 2 * 130 * 4 - 4), "workspace"),
    (dict(q_ts=516), "alignment"),
])
def test_attn_decode_slots_q8_argument_errors_need_no_gpu(kw, word):
    import re
    from promptcache_amd import _native
    lib = _native.load()
    f = dict(q_hi=A, q_lo=A, q_ts=512, kv_base=A, cap=A, len=A, live=A, S=4, layer=1, H=4, Hkv=2, D=128, nsplit=2, ws=A,
             ws_bytes=4 * 4 * 2 * 130 * 4, of_hi=A, of_lo=A, kvq_base=A, qcap=1024, n_layers=2)
    f.update(kw)
    assert lib.pc_attn_decode_slots_workspace_bytes(4, 4, 128, 2) == 4 * 4 * 2 * 130 * 4
    rc = lib.pc_attn_decode_slots_q8(f["q_hi"], f["q_lo"], f["q_ts"], f["kv_base"], f["cap"], f["len"], f["live"], f["S"], f["layer"],
                                     f["H"], f["Hkv"], f["D"], 0.088, f["nsplit"], f["ws"], f["ws_bytes"], f["of_hi"], f["of_lo"],
                                     f["kvq_base"], f["qcap"], f["n_layers"], None)
    assert rc == -1001, rc
    msg = lib.pc_last_error_string().decode()
    assert "pc_attn_decode_slots_q8" in msg and re.search(word, msg), msg
