"""Token controls without a GPU: the numpy rule of tests/logit_ctl_ref.py against transformers' own processors,
``GenerationParameters`` validation (one test per ``ValueError``), ``modes`` resolution, the engine over scripted loops, ``serve``'s
admission errors, the ctypes mirror of ``pc_logit_ctl`` against gcc and pc_logit_adjust's argument errors."""
import ctypes
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import logit_ctl_ref as ref
from tests.test_engine_trace_cpu import _MultiTokenLoop, _OneTokenLoop, _cache, _engine
from tests.test_serve_cpu import _FakeLoop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(**kw):
    from promptcache_amd.generation_engine import GenerationParameters
    kw.setdefault("temperature", 0.0)
    return GenerationParameters(**kw)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_reference_rule_order_and_bits():
    x = np.array([0.5, -1.25, np.nan, -np.inf, 3.0, 1e30, 2.0, 7.0], dtype=np.float32)
    a = ref.adjust(x, bias=[(0, 1.5), (2, 1.0), (3, 5.0), (4, -np.inf), (5, 1e30), (9, 1.0), (-1, 1.0)])
    assert a[0] == np.float32(2.0) and np.isnan(a[2]) and a[3] == -np.inf and a[4] == -np.inf and a[5] == np.float32(1e30) + np.float32(1e30)
    assert ref.same_bits(a[[1, 6, 7]], x[[1, 6, 7]])
    # the allow-list comes behind the bias (a biased id outside it stays -inf, a NaN outside it becomes -inf), the stop ids last
    a = ref.adjust(x, bias=[(0, 100.0), (6, 1.0)], allowed=[6, 7, 2], stop_ids=[7, -1, 50], hold_stops=True)
    assert a.tolist()[:2] == [-np.inf, -np.inf] and np.isnan(a[2]) and a[6] == 3.0 and a[7] == -np.inf
    assert ref.adjust(x, allowed=[6, 7], stop_ids=[7], hold_stops=False)[7] == 7.0
    assert ref.adjust(x, allowed=[1])[2] == -np.inf
    # one float32 add: the sum is rounded once, to float32
    y = np.array([1.0], dtype=np.float32)
    assert ref.adjust(y, bias=[(0, 2.0 ** -30)])[0] == np.float32(1.0)
    assert ref.same_bits(np.array([np.nan, 1.0], np.float32), np.array([np.nan, 1.0], np.float32))
    assert not ref.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert ref.allowed_bits([0, 31, 32, 64, 99], 65).tolist() == [0x80000001, 1, 1]
    # the slot form: the block's n_bias is clamped, the boundary is len + i < stop_free_len
    rows = np.tile(np.arange(4, dtype=np.float32), (4, 1))
    out = ref.adjust_slots(rows, 2, [dict(bias=[(0, 1.0)], n_bias=1000, stop_ids=[3], stop_free_len=6), dict(bias=[(0, 1.0)], n_bias=-1)], [5, 0])
    assert out[:, 0].tolist() == [1.0, 1.0, 0.0, 0.0] and out[:, 3].tolist() == [-np.inf, 3.0, 3.0, 3.0]


@pytest.mark.parametrize("V", [9, 65, 2048])
def test_reference_against_transformers_processors(V):
    lp = pytest.importorskip("transformers.generation.logits_process")
    g = np.random.default_rng(V)
    for trial in range(4):
        x = (g.standard_normal(V) * 4).astype(np.float32)
        ids = g.permutation(V)[:min(8, V - 2)].tolist()
        bias = [(i, float(np.float32(v))) for i, v in zip(ids, g.standard_normal(len(ids)) * 3)]
        scores = torch.from_numpy(x.copy())[None, :]
        prompt = torch.zeros((1, 5), dtype=torch.long)
        # logit_bias: single-token sequences of SequenceBiasLogitsProcessor
        try:
            proc = lp.SequenceBiasLogitsProcessor([[[i], v] for i, v in bias])
        except (TypeError, ValueError):
            proc = lp.SequenceBiasLogitsProcessor({(i,): v for i, v in bias})
        want = proc(prompt, scores.clone())[0].numpy()
        assert ref.same_bits(ref.adjust(x, bias=bias), want)
        # bans: SuppressTokensLogitsProcessor
        want = lp.SuppressTokensLogitsProcessor(ids[:3])(prompt, scores.clone())[0].numpy()
        assert ref.same_bits(ref.adjust(x, bias=[(i, -np.inf) for i in ids[:3]]), want)
        # an allow-list: the complement suppressed
        allow = sorted(ids[:4])
        want = lp.SuppressTokensLogitsProcessor([j for j in range(V) if j not in allow])(prompt, scores.clone())[0].numpy()
        assert ref.same_bits(ref.adjust(x, allowed=allow), want)
        # min_new_tokens at g = min_new - 1 (held back) and g = min_new (free): g tokens were generated behind the 5-token prompt
        stops, min_new = ids[:2], 3
        from promptcache_amd.modes import token_controls
        ctl = token_controls(min_new_tokens=min_new, stop_token_ids=stops)
        mn = lp.MinNewTokensLengthLogitsProcessor(5, min_new, stops)
        for gen in (min_new - 1, min_new):
            want = mn(torch.zeros((1, 5 + gen), dtype=torch.long), scores.clone())[0].numpy()
            assert ref.same_bits(ref.adjust_controls(x, ctl, gen), want)
        assert (ref.adjust_controls(x, ctl, min_new - 1)[stops] == -np.inf).all() and ref.same_bits(ref.adjust_controls(x, ctl, min_new), x)


# ---- GenerationParameters: one test per ValueError --------------------------------------------------------------------------------
def test_defaults_are_off_and_the_merge():
    from promptcache_amd.modes import LOGIT_BIAS_MAX, LOGIT_STOP_MAX, TokenControls
    p = _params()
    assert (p.logit_bias, p.banned_token_ids, p.allowed_token_ids, p.min_new_tokens, p.token_controls) == (None, None, None, 0, None)
    assert _params(logit_bias={}, banned_token_ids=[], min_new_tokens=5).token_controls is None      # no stop id to hold back: vacuous
    assert (LOGIT_BIAS_MAX, LOGIT_STOP_MAX) == (64, 8)
    c = _params(logit_bias={7: 1.5, 3: -2, 9: -math.inf}, banned_token_ids=[7, 11], allowed_token_ids=[5, 3, 5, 40],
                min_new_tokens=4, stop_token_ids=[2, 40, 2]).token_controls
    assert c == TokenControls(((3, -2.0), (7, -math.inf), (9, -math.inf), (11, -math.inf)), (3, 5, 40), 4, (2, 40))      # a ban wins
    assert c.max_id() == 40
    assert _params(min_new_tokens=0, stop_token_ids=[2]).token_controls is None
    assert _params(logit_bias={i: 0.5 for i in range(32)}, banned_token_ids=list(range(16, 64))).token_controls is not None   # 64 distinct


def test_value_error_bias_plus_inf():
    with pytest.raises(ValueError, match=r"logit_bias\[4\].*finite, or -inf"):
        _params(logit_bias={4: math.inf})


def test_value_error_bias_nan():
    with pytest.raises(ValueError, match=r"logit_bias\[4\].*finite, or -inf"):
        _params(logit_bias={4: float("nan")})


def test_value_error_more_than_64_ids():
    with pytest.raises(ValueError, match="65 distinct ids, more than LOGIT_BIAS_MAX = 64"):
        _params(logit_bias={i: 1.0 for i in range(40)}, banned_token_ids=list(range(30, 65)))


def test_value_error_more_than_8_stop_ids_with_min_new():
    with pytest.raises(ValueError, match="at most 8 stop token ids"):
        _params(stop_token_ids=list(range(9)), min_new_tokens=2)
    assert _params(stop_token_ids=list(range(9)), min_new_tokens=0).token_controls is None


def test_value_error_ids():
    for kw in (dict(logit_bias={-1: 1.0}), dict(banned_token_ids=[2.5]), dict(allowed_token_ids=[True]), dict(banned_token_ids=["7"])):
        with pytest.raises(ValueError, match="non-negative integers"):
            _params(**kw)
    with pytest.raises(ValueError, match="min_new_tokens must be a non-negative integer"):
        _params(min_new_tokens=-1)
    # in range once the vocabulary is known: at the first use
    from promptcache_amd.modes import check_token_controls
    c = _params(logit_bias={5000: 1.0}).token_controls
    assert check_token_controls(c, vocab=5001) is c and check_token_controls(None, loop_prefill=True) is None
    with pytest.raises(ValueError, match=r"id 5000, outside the vocabulary \[0, 5000\)"):
        check_token_controls(c, vocab=5000)


def test_value_error_nothing_left_to_draw():
    with pytest.raises(ValueError, match="no token that can be drawn"):
        _params(allowed_token_ids=[])
    with pytest.raises(ValueError, match="no token that can be drawn"):
        _params(allowed_token_ids=[3, 4], banned_token_ids=[4, 3])
    with pytest.raises(ValueError, match="minus the stop ids while min_new_tokens > 0"):
        _params(allowed_token_ids=[3, 4], banned_token_ids=[4], stop_token_ids=[3], min_new_tokens=1)
    assert _params(allowed_token_ids=[3, 4], banned_token_ids=[4], stop_token_ids=[3]).token_controls is not None
    from promptcache_amd.modes import check_token_controls
    with pytest.raises(ValueError, match="no token that can be drawn"):
        check_token_controls(_params(banned_token_ids=[0, 1]).token_controls, vocab=2)


def test_value_error_loop_prefill_and_check_token_controls():
    from promptcache_amd.modes import check_token_controls
    c = _params(banned_token_ids=[1]).token_controls
    with pytest.raises(ValueError, match="loop_prefill=True and token controls.*forced question rows"):
        check_token_controls(c, loop_prefill=True)
    with pytest.raises(ValueError, match="at most 8 stop token ids, not 9"):
        check_token_controls(_params(stop_token_ids=[1], min_new_tokens=2).token_controls, n_stop_ids=9)


# ---- modes ------------------------------------------------------------------------------------------------------------------------
def test_resolve_serve_off_is_the_parents_record(monkeypatch):
    from promptcache_amd.modes import Capabilities, Modes, resolve_batch, resolve_serve
    full = Capabilities(lookup_loop=True, lookup=True, lookup_q8=True, lookup_trunk=True, head_dim=128)
    m = resolve_serve(full, 4, env={})
    assert m.token_controls is False and m == Modes(True, "one device loop, new prompts admitted as slots free up")
    assert m.loop_kwargs() == {} == m.loop_kwargs(one_token=True) and "token_controls" not in m.reason()
    assert resolve_serve(full, 4, env={}, token_controls=False) == m and resolve_serve(full, 4, env={"PC_SERVE_TOKEN_CONTROLS": "0"}) == m
    # keyword-only: the positional order of the constructor is what it was, logprobs its last positional field
    assert Modes(True, "x", False, 0, 0, None, "fp16", True, False, 3).logprobs == 3
    with pytest.raises(TypeError):
        Modes(True, "x", False, 0, 0, None, "fp16", True, False, 3, True)
    assert Modes(True, "x", token_controls=True).token_controls and Modes(True, "x") != Modes(True, "x", token_controls=True)
    on = resolve_serve(full, 4, lookup=3, slot_kv="int8", env={}, token_controls=True, logprobs=1)
    assert on.token_controls and on.loop_kwargs() == {"kv": "int8", "logprobs": 1, "token_controls": True} == on.loop_kwargs(one_token=True)
    assert on.reason().endswith("applied in front of the draw (token_controls=True)")
    assert resolve_serve(full, 4, env={"PC_SERVE_TOKEN_CONTROLS": "1"}).token_controls
    assert not resolve_serve(full, 4, env={"PC_SERVE_TOKEN_CONTROLS": "1"}, token_controls=False).token_controls
    with pytest.raises(ValueError, match="PC_SERVE_TOKEN_CONTROLS must be 0 or 1"):
        resolve_serve(full, 4, env={"PC_SERVE_TOKEN_CONTROLS": "yes"})
    with pytest.raises(ValueError, match="loop_prefill=True and token controls"):
        resolve_serve(full, 4, lookup=3, loop_prefill=True, env={}, token_controls=True)
    assert not resolve_batch(full, 4, env={"PC_SERVE_TOKEN_CONTROLS": "1"}).token_controls          # (serve's switch)
    # a loop that is not batched says nothing about the node
    assert "token_controls" not in resolve_serve(Capabilities(not_batched="PC_DEVICE_GREEDY=0"), 4, env={}, token_controls=True).reason()


def test_serve_plan_names_the_mode():
    log = []
    hf = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True)
    ge = _engine(log, hf, {})
    assert ge.serve_plan() == ge.serve_plan(token_controls=False)
    batched, why = ge.serve_plan(token_controls=True)
    assert batched and why.endswith("(token_controls=True)") and why.startswith(ge.serve_plan()[1])


# ---- the engine over scripted loops -----------------------------------------------------------------------------------------------
def _hf(log, make_loop, multi=False):
    """A model with the single-sequence loop factories and the eager call, restated with the numpy rule."""
    def factory(*a, **kw):
        log.append(["loop", sorted(kw), kw.get("token_controls")])
        return make_loop()

    def adjust_logits(row, controls, generated):
        log.append(["adjust_logits", generated])
        return torch.from_numpy(ref.adjust_controls(row.numpy(), controls, generated))
    hf = types.SimpleNamespace(greedy_loop=factory, sample_loop=factory, can_loop=lambda past: True, adjust_logits=adjust_logits,
                               config=types.SimpleNamespace(vocab_size=8192))
    if multi:
        hf.lookup_loop, hf.lookup_available = factory, lambda: True
    return hf


def test_generate_first_token_goes_through_the_eager_call_and_the_loop_gets_the_controls():
    log = []
    ge = _engine(log, _hf(log, lambda: _OneTokenLoop(log, [11, 12, 13])), {None: [[(10, 2.0), (20, 1.0)]]})
    p = _params(max_new_tokens=4, banned_token_ids=[10])
    outs = list(ge.generate([7, 8], [0, 1], p, None, stream_interval=1))
    assert outs[-1].new_text == "20 11 12 13"                             # the ban moved the first token to the runner-up
    assert ["adjust_logits", 0] in log and ["loop", ["token_controls"], p.token_controls] in log
    # off: nothing new is handed to the loop, the eager call is not made
    log = []
    ge = _engine(log, _hf(log, lambda: _OneTokenLoop(log, [11, 12, 13])), {None: [[(10, 2.0), (20, 1.0)]]})
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=4), None, stream_interval=1))
    assert outs[-1].new_text == "10 11 12 13" and ["loop", [], None] in log and not any(e[0] == "adjust_logits" for e in log)
    # the lookup loop takes them too
    log = []
    ge = _engine(log, _hf(log, lambda: _MultiTokenLoop(log, [[21, 22], [23]], 3), multi=True), {None: [[(10, 2.0), (20, 1.0)]]}, lookup=3)
    p = _params(max_new_tokens=4, allowed_token_ids=[20, 21, 22, 23])
    outs = list(ge.generate([7, 8], [0, 1], p, None, stream_interval=1))
    assert outs[-1].new_text == "20 21 22 23" and ["loop", ["token_controls"], p.token_controls] in log


def test_host_steps_take_the_eager_call_per_token_with_the_token_number():
    log = []
    hf = types.SimpleNamespace(adjust_logits=_hf(log, None).adjust_logits, config=types.SimpleNamespace(vocab_size=8192))
    rows = [[(30, 3.0), (40, 2.0)], [(30, 3.0), (41, 2.0)], [(30, 3.0), (42, 2.0)], [(30, 3.0), (43, 2.0)]]
    ge = _engine(log, hf, {None: rows})
    # token 30 is a stop id held back for the generated tokens 0 and 1: it is drawn as number 2, and ends the generation
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=4, stop_token_ids=[30], min_new_tokens=2), None, stream_interval=1))
    assert outs[-1].new_text == "40 41 30" and [e for e in log if e[0] == "adjust_logits"] == [["adjust_logits", g] for g in range(3)]
    ge = _engine([], types.SimpleNamespace(), {None: rows})               # a model without the call: an error, not a fallback
    with pytest.raises(RuntimeError, match="adjust_logits"):
        list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=2, banned_token_ids=[30]), None))
    with pytest.raises(ValueError, match=r"outside the vocabulary \[0, 8192\)"):
        list(_engine([], hf, {None: rows}).generate([7, 8], [0, 1], _params(max_new_tokens=2, banned_token_ids=[8192]), None))


class _FakeLoopCtl(_FakeLoop):
    """tests/test_serve_cpu._FakeLoop whose ``admit`` takes the request's controls."""
    admitted = []

    def admit(self, slot, past, token, position, max_new, params, seed, history, stop_ids, trunk=None, controls=None):
        _FakeLoopCtl.admitted.append((past.tag, controls))
        return super().admit(slot, past, token, position, max_new, params, seed, history, stop_ids, trunk=trunk)


def _fake_serve(reqs, **serve_kw):
    made = []

    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, slots=None, slot_index=None, each=False,
                  max_keys=None, trunks=None, **kw):
        made.append(kw)
        return (_FakeLoopCtl if "token_controls" in kw else _FakeLoop)([p.tag for p in pasts], max_new, stop_ids, slot_index)
    log = []
    hf = types.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True, adjust_logits=_hf(log, None).adjust_logits,
                               config=types.SimpleNamespace(vocab_size=8192))
    ge = _engine(log, hf, {r + 1: [[(1000 * (r + 1), 2.0), (1000 * (r + 1) + 500, 1.0)]] for r in range(len(reqs))})
    ce = types.SimpleNamespace(process=lambda prompt, slot=0, return_full_position_ids=False: ([prompt], [10 + prompt], 0.0, _cache(prompt)),
                               slots=2, max_ctx_length=4096)
    outs = {}
    for index, out in ge.serve(ce, iter(reqs), None, stream_interval=1, share_trunk=False, **serve_kw):
        outs.setdefault(index, []).append(out)
    return outs, made, ge, log


def test_serve_over_a_fake_loop_hands_every_request_its_own_block(monkeypatch):
    monkeypatch.delenv("PC_SERVE_TOKEN_CONTROLS", raising=False)
    kws = [dict(banned_token_ids=[1000]), {}, dict(allowed_token_ids=[3500, 3001, 3002, 3003]), {}]
    reqs = [(r + 1, _params(max_new_tokens=3, **kw)) for r, kw in enumerate(kws)]
    _FakeLoopCtl.admitted = []
    outs, made, ge, log = _fake_serve(reqs, token_controls=True)
    # the first fill builds the loop with one block (or None) per sequence; later requests bring theirs through admit
    assert made == [{"token_controls": [reqs[0][1].token_controls, None]}]
    assert _FakeLoopCtl.admitted == [(3, reqs[2][1].token_controls), (4, None)]
    assert [ge.last_serve_tokens[r][0] for r in range(4)] == [1500, 2000, 3500, 4000]      # first tokens under each request's controls
    assert [e for e in log if e[0] == "adjust_logits"] == [["adjust_logits", 0]] * 2      # ... through the eager call, where asked
    # off: the model is handed nothing new
    plain = [(r + 1, _params(max_new_tokens=3)) for r in range(4)]
    outs, made, ge, log = _fake_serve(plain)
    assert made == [{}] and not any(e[0] == "adjust_logits" for e in log)
    monkeypatch.setenv("PC_SERVE_TOKEN_CONTROLS", "1")
    outs, made, ge, log = _fake_serve(plain)
    assert made == [{"token_controls": [None, None]}]


def test_serve_admission_errors(monkeypatch):
    monkeypatch.delenv("PC_SERVE_TOKEN_CONTROLS", raising=False)
    with pytest.raises(ValueError, match=r"carries token controls.*call serve\(token_controls=True\).*PC_SERVE_TOKEN_CONTROLS=1"):
        _fake_serve([(1, _params(max_new_tokens=3)), (2, _params(max_new_tokens=3, min_new_tokens=2, stop_token_ids=[5]))])
    # a refused request is refused before it is processed or prefilled
    log, seen = [], []
    ge = _engine(log, types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True), {})
    ce = types.SimpleNamespace(process=lambda prompt, slot=0, return_full_position_ids=False: seen.append(prompt), slots=2, max_ctx_length=4096)
    with pytest.raises(ValueError, match=r"serve\(token_controls=True\)"):
        list(ge.serve(ce, iter([(1, _params(logit_bias={3: 1.0}))]), None, share_trunk=False))
    assert seen == [] and log == []
    hf = types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True, lookup_slot_loop=None, lookup_available=lambda: True)
    with pytest.raises(ValueError, match="loop_prefill=True and token controls"):
        list(_engine([], hf, {}).serve(ce, iter([(1, _params(logit_bias={3: 1.0}))]), None, share_trunk=False, lookup=3, loop_prefill=True))
    with pytest.raises(ValueError, match="loop_prefill=True and token controls"):
        list(_engine([], hf, {}).serve(ce, iter([(1, _params())]), None, share_trunk=False, lookup=3, loop_prefill=True, token_controls=True))
    assert seen == []


# ---- the struct mirror and the C entry ---------------------------------------------------------------------------------------------
def test_struct_mirror_of_pc_logit_ctl_matches_the_header(tmp_path):
    from promptcache_amd import _native
    cls = _native.LogitCtl
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {',
            '  printf("size %zu\\n", sizeof(pc_logit_ctl));']
    body += [f'  printf("{f} %zu\\n", offsetof(pc_logit_ctl, {f}));' for f, _ in cls._fields_]
    body += ['  printf("PC_LOGIT_BIAS_MAX %d\\n", PC_LOGIT_BIAS_MAX);', '  printf("PC_LOGIT_STOP_MAX %d\\n", PC_LOGIT_STOP_MAX);', '  return 0;', '}']
    src = tmp_path / "ctl.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "ctl"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 16 + 4 * 8 + 4 * 64 + 4 * 64
    for name, _ in cls._fields_:
        assert int(got[name]) == getattr(cls, name).offset, name
    from promptcache_amd import modes
    assert int(got["PC_LOGIT_BIAS_MAX"]) == _native.LOGIT_BIAS_MAX == modes.LOGIT_BIAS_MAX == ref.BIAS_MAX
    assert int(got["PC_LOGIT_STOP_MAX"]) == _native.LOGIT_STOP_MAX == modes.LOGIT_STOP_MAX == ref.STOP_MAX
    # the image helper: the neutral block, and a full one
    neutral = cls.from_buffer_copy(_native.logit_ctl_bytes())
    assert (neutral.n_bias, neutral.use_allowed, neutral.stop_free_len, list(neutral.stop_ids)) == (0, 0, 0, [-1] * 8)
    b = cls.from_buffer_copy(_native.logit_ctl_bytes([(5, 1.5), (9, -math.inf)], True, 77, [3, 4]))
    assert (b.n_bias, b.use_allowed, b.stop_free_len, list(b.stop_ids)[:3], list(b.bias_id)[:2], b.bias[0], b.bias[1]) == \
        (2, 1, 77, [3, 4, -1], [5, 9], 1.5, -math.inf)


def test_argument_errors_need_no_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    one = ctypes.c_void_p((base + 15) & ~15)
    two = ctypes.c_void_p(one.value + 2048)
    good = dict(logits=one, ldl=64, vocab=64, S=2, rps=2, ctl=one, allowed=None, len=None, out=two, ldo=64)

    def call(**kw):
        a = {**good, **kw}
        return lib.pc_logit_adjust(a["logits"], a["ldl"], a["vocab"], a["S"], a["rps"], a["ctl"], a["allowed"], a["len"], a["out"], a["ldo"], None)
    for bad in (dict(logits=None), dict(ctl=None), dict(out=None), dict(S=0), dict(rps=0), dict(rps=17), dict(S=33), dict(S=65, rps=1),
                dict(vocab=0), dict(vocab=1 << 24, ldl=1 << 24, ldo=1 << 24), dict(ldl=63), dict(ldo=60), dict(ldo=66),
                dict(logits=ctypes.c_void_p(one.value + 2)), dict(out=ctypes.c_void_p(two.value + 4)), dict(out=one),
                dict(allowed=ctypes.c_void_p(one.value + 1)), dict(len=ctypes.c_void_p(one.value + 2))):
        assert call(**bad) == -1001, bad
        assert b"pc_logit_adjust" in lib.pc_last_error_string()
    assert "pc_logit_adjust" in _native.SIGNATURES
    src = open(os.path.join(ROOT, "include", "promptcache_hip.h")).read()
    contract = src[src.index("pc_logit_adjust:"):src.index("#define PC_LOGIT_BIAS_MAX")]
    assert "writes out of place" in contract and "No state, no counter, no atomic" in contract
