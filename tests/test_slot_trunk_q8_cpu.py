"""CPU side of the shared-trunk attention over int8 K/V images: the numpy reference of
pc_attn_decode_slots_trunk_q8 (tests/slot_trunk_q8_ref.py), the invariant the mode rests on -- the quantiser is row-local, so equal
fp16 rows give equal image rows --, the one resolution of the pair ``slot_kv="int8"`` x ``share_trunk`` in ``modes.py``, and the
refusals that are answered before anything is built."""
import numpy as np
import pytest

from tests import kv_q8_ref as q8
from tests import slot_kv_q8_ref as ref
from tests import slot_trunk_q8_ref as tref
from tests.test_slot_kv_q8_cpu import _engine, _Hf

F32 = np.float32
D = 128
OLD_TEXT = ("slot_kv='int8' and share_trunk exclude each other (the shared-trunk attention reads the leader's fp16 "
            "arena; int8 images under share_trunk are not implemented)")
ENV = ("PC_SLOT_KV", "PC_SLOT_TRUNK", "PC_SLOT_KEEP_ARENAS", "PC_SERVE_LOOKUP", "PC_SLOT_LOOKUP", "PC_SERVE_LOOP_PREFILL",
       "PC_SERVE_LOGPROBS")


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,T,n", [(4, 4, 7, 7), (4, 2, 300, 301), (4, 2, 5, 77), (8, 1, 64, 200)])
def test_reference_equals_the_unshared_reference_where_the_trunk_rows_are_equal(H, Hkv, T, n):
    """Member rows [0, T) = leader rows [0, T): the concatenation IS the member's image, so the result is
    ``slot_kv_q8_ref.attend`` on the member's image alone, bit for bit -- and the member's own rows [0, T) do not enter."""
    rng = np.random.default_rng(H * 1000 + T + n)
    kv = (rng.standard_normal((2, Hkv, n + 1, D)) * 1.5).astype(np.float16)           # [k|v][Hkv][n + 1][D]; row n is the new one
    codes, scale = q8.quantise(kv[:, :, :n])
    lead_rows = np.concatenate([kv[:, :, :T], rng.standard_normal((2, Hkv, 9, D)).astype(np.float16)], axis=2)   # leader: T + 9 rows
    lc, ls = q8.quantise(lead_rows)
    q = (rng.standard_normal((H, D)) * 0.5).astype(F32)
    want = ref.attend(q, codes[0], scale[0], codes[1], scale[1], kv[0][:, n], kv[1][:, n])
    got = tref.attend(q, T, (lc[0], ls[0]), (lc[1], ls[1]), (codes[0], scale[0]), (codes[1], scale[1]), kv[0][:, n], kv[1][:, n])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    poisoned_c, poisoned_s = codes.copy(), scale.copy()
    poisoned_c[:, :, :T], poisoned_s[:, :, :T] = 0x55, np.nan                           # the member's own trunk rows are never read
    again = tref.attend(q, T, (lc[0], ls[0]), (lc[1], ls[1]), (poisoned_c[0], poisoned_s[0]), (poisoned_c[1], poisoned_s[1]),
                        kv[0][:, n], kv[1][:, n])
    assert np.array_equal(again.view(np.uint32), want.view(np.uint32))
    alone = tref.attend(q, 0, (lc[0], ls[0]), (lc[1], ls[1]), (codes[0], scale[0]), (codes[1], scale[1]), kv[0][:, n], kv[1][:, n])
    assert np.array_equal(alone.view(np.uint32), want.view(np.uint32))                  # T = 0: the slot on its own


def test_quantise_is_row_local():
    """The same fp16 row between different neighbours, at another row index and in another plane count: the same codes and scale."""
    rng = np.random.default_rng(9)
    row = (rng.standard_normal(D) * 3).astype(np.float16)
    a = (rng.standard_normal((3, 40, D)) * 0.01).astype(np.float16)                   # tiny neighbours
    b = (rng.standard_normal((5, 17, D)) * 100).astype(np.float16)                    # huge neighbours
    a[1, 7], b[4, 16] = row, row
    (ca, sa), (cb, sb), (c1, s1) = q8.quantise(a), q8.quantise(b), q8.quantise(row[None])
    assert np.array_equal(ca[1, 7], cb[4, 16]) and np.array_equal(ca[1, 7], c1[0])
    assert sa[1, 7].view(np.uint32) == sb[4, 16].view(np.uint32) == s1[0].view(np.uint32)
    # ... so equal leading rows give equal leading image rows, whatever follows them
    lead = (rng.standard_normal((4, 30, D))).astype(np.float16)
    member = np.concatenate([lead[:, :21], rng.standard_normal((4, 50, D)).astype(np.float16)], axis=1)
    (cl, sl), (cm, sm) = q8.quantise(lead), q8.quantise(member)
    assert np.array_equal(cl[:, :21], cm[:, :21]) and np.array_equal(sl[:, :21].view(np.uint32), sm[:, :21].view(np.uint32))


# ---- modes -----------------------------------------------------------------------------------------------------------------------
def test_check_slot_kv_with_and_without_trunk_q8():
    from promptcache_amd.modes import check_slot_kv
    for kw in (dict(), dict(trunk_q8=False)):
        with pytest.raises(ValueError) as e:
            check_slot_kv("int8", share_trunk=True, head_dim=128, **kw)
        assert str(e.value) == OLD_TEXT                                                 # the old text, unchanged
    assert check_slot_kv("int8", share_trunk=True, lookup=0, head_dim=128, trunk_q8=True) is None
    assert check_slot_kv("int8", trunk_q8=True) is None and check_slot_kv("fp16", share_trunk=True, lookup=3, trunk_q8=True) is None
    for lq8 in (False, True):                                                           # with lookup: no shared-trunk form
        with pytest.raises(ValueError, match="share_trunk") as e:
            check_slot_kv("int8", share_trunk=True, lookup=3, head_dim=128, trunk_q8=True, lookup_q8=lq8)
        assert "lookup" in str(e.value) and str(e.value) != OLD_TEXT
    # the keyword lifts that one refusal only
    for kw, word in ((dict(head_dim=64), "head_dim"), (dict(no_loop="x"), "does not have"), (dict(not_batched="y"), "is not: y")):
        with pytest.raises(ValueError, match=word):
            check_slot_kv("int8", share_trunk=True, trunk_q8=True, **kw)
    with pytest.raises(ValueError, match="lookup > 0 exclude each other"):
        check_slot_kv("int8", lookup=3, trunk_q8=True)


def test_resolve_serve_takes_the_pair_and_resolve_batch_never_does(monkeypatch):
    from promptcache_amd import modes
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    assert modes.Capabilities().trunk_q8 is False
    assert modes.Capabilities(None, None, False, False, False, False, 128, True).trunk_q8 is True   # appended: the last field
    yes = modes.Capabilities(trunk_q8=True, head_dim=128, lookup=True, lookup_loop=True, lookup_q8=True, lookup_trunk=True)
    no = modes.Capabilities(trunk_q8=False, head_dim=128, lookup=True, lookup_loop=True, lookup_q8=True, lookup_trunk=True)
    m = modes.resolve_serve(yes, 4, slot_kv="int8", share_trunk=True)
    assert (m.batched, m.share_trunk, m.slot_kv, m.drafts, m.keep_arenas) == (True, True, "int8", 0, True)
    assert m == modes.Modes(True, m.base, share_trunk=True, slot_kv="int8")
    assert m.loop_kwargs(one_token=True) == {"kv": "int8"}
    with pytest.raises(ValueError) as e:
        modes.resolve_serve(no, 4, slot_kv="int8", share_trunk=True)
    assert str(e.value) == OLD_TEXT
    with pytest.raises(ValueError, match="share_trunk") as e:
        modes.resolve_serve(yes, 4, slot_kv="int8", share_trunk=True, lookup=3)
    assert "lookup" in str(e.value)
    with pytest.raises(ValueError, match="keep_arenas=False") as e:
        modes.resolve_serve(yes, 4, slot_kv="int8", share_trunk=True, keep_arenas=False)
    assert "share_trunk" in str(e.value)
    assert modes.resolve_serve(yes, 4, slot_kv="int8", keep_arenas=False).keep_arenas is False      # (without sharing: as before)
    for caps in (yes, no):
        with pytest.raises(ValueError) as e:
            modes.resolve_batch(caps, 4, slot_kv="int8", share_trunk=True)
        assert str(e.value) == OLD_TEXT
    # the environment spelling gives the same results
    env = {"PC_SLOT_KV": "int8", "PC_SLOT_TRUNK": "1"}
    assert modes.resolve_serve(yes, 4, env=env) == m
    with pytest.raises(ValueError, match="exclude each other"):
        modes.resolve_serve(no, 4, env=env)
    with pytest.raises(ValueError, match="keep_arenas=False"):
        modes.resolve_serve(yes, 4, env={**env, "PC_SLOT_KEEP_ARENAS": "0"})
    with pytest.raises(ValueError, match="share_trunk"):
        modes.resolve_serve(yes, 4, env={**env, "PC_SERVE_LOOKUP": "2"})
    with pytest.raises(ValueError, match="exclude each other"):
        modes.resolve_batch(yes, 4, env=env)
    assert modes.resolve_serve(yes, 4, env={}) == modes.resolve_serve(no, 4, env={})                # mode off: nothing moves


class _HfTrunk(_Hf):
    """A model stub that says it has the shared-trunk attention over images."""

    def __init__(self, says=True):
        super().__init__()
        self.slot_trunk_q8_available = lambda: says


class _Slots:
    slots = 2
    max_ctx_length = 2048


def test_serve_takes_the_pair_where_the_model_has_the_step(monkeypatch):
    from promptcache_amd.generation_engine import GenerationParameters
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    params = GenerationParameters(temperature=0.0, max_new_tokens=8)
    reqs = [([1, 2], [0, 1], object())] * 2
    ge = _engine(_HfTrunk())
    assert ge._capabilities(True, True).trunk_q8 is True and _engine(_Hf())._capabilities(True, True).trunk_q8 is False
    assert list(ge.serve(_Slots(), [], params, slot_kv="int8", share_trunk=True)) == []
    for hf in (_Hf(), _HfTrunk(False)):                                                 # no such method, or it says no
        with pytest.raises(ValueError) as e:
            next(_engine(hf).serve(_Slots(), [], params, slot_kv="int8", share_trunk=True))
        assert str(e.value) == OLD_TEXT
    with pytest.raises(ValueError, match="keep_arenas=False.*share_trunk"):
        next(ge.serve(_Slots(), [], params, slot_kv="int8", share_trunk=True, keep_arenas=False))
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.serve(_Slots(), [], params, slot_kv="int8", share_trunk=True, lookup=2))
    with pytest.raises(ValueError) as e:                                                # generate_batch stays refused
        next(ge.generate_batch(reqs, params, slot_kv="int8", share_trunk=True))
    assert str(e.value) == OLD_TEXT
    monkeypatch.setenv("PC_SLOT_KV", "int8")                                            # the environment asks for the same mode
    monkeypatch.setenv("PC_SLOT_TRUNK", "1")
    assert list(ge.serve(_Slots(), [], params)) == []
    with pytest.raises(ValueError, match="exclude each other"):
        next(_engine(_Hf()).serve(_Slots(), [], params))
    with pytest.raises(ValueError, match="exclude each other"):
        next(ge.generate_batch(reqs, params))
    monkeypatch.setenv("PC_SLOT_KEEP_ARENAS", "0")
    with pytest.raises(ValueError, match="keep_arenas=False"):
        next(ge.serve(_Slots(), [], params))


def test_slot_loop_refuses_the_pair_without_each_before_anything_is_built():
    from promptcache_amd.model.llama_hip import LlamaHIP

    class M:
        D = 128
        slot_loop_available = lambda self: True
        slot_trunk_q8_available = lambda self: True
        _slot_loop_front = lambda self, *a: (_ for _ in ()).throw(AssertionError("the refusal comes first"))

    for kw in (dict(share_trunk=True), dict(trunks=[(None, 0)]), dict(share_trunk=True, each=False)):
        with pytest.raises(ValueError) as e:
            LlamaHIP.slot_loop(M(), [], [], [], 4, kv="int8", **kw)
        assert str(e.value) == OLD_TEXT
    with pytest.raises(ValueError, match="keep_arenas=False.*share_trunk"):
        LlamaHIP.slot_loop(M(), [], [], [], 4, kv="int8", share_trunk=True, each=True, keep_arenas=False)
    with pytest.raises(AssertionError, match="the refusal comes first"):               # each=True: the pair passes the checks
        LlamaHIP.slot_loop(M(), [], [], [], 4, kv="int8", share_trunk=True, each=True)
    no = M()
    no.slot_trunk_q8_available = lambda: False
    with pytest.raises(ValueError) as e:
        LlamaHIP.slot_loop(no, [], [], [], 4, kv="int8", share_trunk=True, each=True)
    assert str(e.value) == OLD_TEXT
    hd64 = M()
    hd64.D = 64
    with pytest.raises(ValueError, match="head_dim"):
        LlamaHIP.slot_loop(hd64, [], [], [], 4, kv="int8", share_trunk=True, each=True)


def test_the_entry_is_declared_and_mirrored():
    import ctypes
    from promptcache_amd import _native
    lib = _native.load()
    rt, at = _native.SIGNATURES["pc_attn_decode_slots_trunk_q8"]
    assert rt is ctypes.c_int and len(at) == len(_native.SIGNATURES["pc_attn_decode_slots_trunk"][1]) + 3
    assert hasattr(lib, "pc_attn_decode_slots_trunk_q8") and callable(_native.attn_decode_slots_trunk_q8)
