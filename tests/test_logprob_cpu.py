"""Per-token log-probabilities without a GPU: the float64 reference of tests/logprob_ref.py against torch, the float32
restatement of the kernel's arithmetic on every row the GPU test uses, ``modes.check_logprobs`` / ``resolve_serve(logprobs=...)``,
the token-stream rule and the two pumps over scripted loops, ``serve``'s admission errors, and pc_token_logprobs' argument errors."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import logprob_ref as ref
from tests.test_engine_trace_cpu import _LookupSlotLoop, _MultiTokenLoop, _OneTokenLoop, _cache, _engine
from tests.test_serve_cpu import _FakeLoop

GPU_VOCABS = (9, 33, 1000, 1027, 32000, 128256)       # tests/test_gpu_logprob.py


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [9, 33, 1000, 32000])
def test_reference_against_torch(V):
    rng = np.random.default_rng(V)
    for j in range(4):
        x = (rng.standard_normal(V) * (1.0 + 3 * j)).astype(np.float32)
        if j == 3:
            x[rng.random(V) < 0.2] = -np.inf
            x[0] = 0.5
        want = torch.log_softmax(torch.from_numpy(x.astype(np.float64)), dim=-1).numpy()
        got = ref.log_softmax(x)
        fin = np.isfinite(want)
        assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.abs(got[fin] - want[fin]).max() < 1e-12
        fx = x[np.isfinite(x)]
        if len(np.unique(fx)) == len(fx):                                # tie-free: torch.topk has one answer
            n = min(8, len(fx) - 1)
            top = torch.topk(torch.from_numpy(x.astype(np.float64)), n).indices.numpy()
            assert np.array_equal(ref.order(x)[:n], top)
            ids, lp = ref.record(x, int(top[0]), n)
            assert ids[0] == ids[1] == top[0] and lp[0] == lp[1] and np.all(np.diff(lp[1:]) <= 0)


def test_reference_conventions():
    x = np.array([1.0, np.nan, 3.0, 3.0, -np.inf, 1.0, 3.0], dtype=np.float32)
    assert ref.order(x).tolist() == [2, 3, 6, 0, 5, 1, 4]                # value descending, index ascending; NaN ranks as -inf
    ids, lp = ref.record(x, 6, 6)
    assert ids.tolist() == [6, 2, 3, 6, 0, 5, 1] and lp[0] == lp[1] == lp[3] and np.isneginf(lp[6])
    assert abs(np.exp(lp[1:6]).sum() - 1.0) < 1e-12                       # -inf and NaN contribute nothing
    ids, lp = ref.record(x, 7, 2)                                        # out of range: NaN in entry 0, the rest right
    assert ids.tolist() == [-1, 2, 3] and np.isnan(lp[0]) and np.isfinite(lp[1:]).all()
    for dead in (np.full(5, -np.inf), np.full(5, np.nan), np.array([0.0, np.inf, 1.0])):
        ids, lp = ref.record(dead.astype(np.float32), 1, 3)
        assert ids.tolist() == [-1] * 4 and np.isnan(lp).all()
    ids, lp = ref.records(np.stack([x, x]), [0, 2], 1)
    assert ids.tolist() == [[0, 2], [2, 2]] and lp.shape == (2, 2)


@pytest.mark.parametrize("V", GPU_VOCABS)
def test_float32_restatement_stays_within_the_tolerance_on_the_gpu_tests_rows(V):
    """The inputs are fair: the kernel's sums in float32 stay within the bound on every row kind, and no row hides a dropped element
    (losing the spike, the maximum of the range row or one element of the constant row moves the result by far more than 2e-4, or
    changes an id)."""
    worst = 0.0
    for name, x in ref.case_rows(V).items():
        assert np.nanmax(np.abs(np.where(np.isinf(x), 0, x))) <= 64
        want, got = ref.log_softmax(x), ref.log_softmax_f32(x)
        if name == "nothing_finite":
            assert np.isnan(want).all() and np.isnan(got).all()
            continue
        fin = np.isfinite(want)
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), name
        worst = max(worst, float(np.abs(got[fin].astype(np.float64) - want[fin]).max()))
        if name.startswith("spike@"):
            p = int(name.split("@")[1])
            lost = ref.log_softmax(np.delete(x, p))
            # log(e^20 + V - 1) - log(V - 1): above 10 up to V = e^10 = 22 026, 8.2 at V = 128 256 -- 40 000 tolerances
            assert abs(lost[0 if p else 1] - want[0 if p else 1]) > (10 if V <= 22026 else 8)
        toks = ref.case_tokens(x, min(8, V - 1))
        assert toks[0] == ref.order(x)[0] and toks[2] == V - 1 and toks[3] == V and toks[4] == -1
        assert toks[1] not in ref.order(x)[:min(8, V - 1)].tolist()
    assert worst <= ref.TOL, worst
    assert V - 1 in ref.spike_positions(V) and 0 in ref.spike_positions(V) and len(ref.spike_positions(V)) == min(10, V)


# ---- modes ------------------------------------------------------------------------------------------------------------------------
def test_check_logprobs_and_resolve_serve():
    from promptcache_amd.modes import LOGPROBS_MAX_TOP, Capabilities, Modes, check_logprobs, resolve_batch, resolve_serve
    assert LOGPROBS_MAX_TOP == 8 == ref.MAX_TOP
    assert check_logprobs(None) is None and check_logprobs(None, loop_prefill=True) is None
    assert [check_logprobs(n) for n in range(9)] == list(range(9))
    for bad in (-1, 9, 2.0, "3", True):
        with pytest.raises(ValueError, match=r"None or an integer in 0\.\.8"):
            check_logprobs(bad)
    with pytest.raises(ValueError, match="loop_prefill=True and logprobs exclude each other.*first token.*forced row"):
        check_logprobs(0, loop_prefill=True)
    full = Capabilities(lookup_loop=True, lookup=True, lookup_q8=True, lookup_trunk=True, head_dim=128)
    # defaults off: nothing new is handed to a model
    m = resolve_serve(full, 4, env={})
    assert m.logprobs is None and m.loop_kwargs() == {} and m.loop_kwargs(one_token=True) == {} and "logprobs" not in m.reason()
    assert Modes(True, "x").logprobs is None and Modes.__dataclass_fields__["logprobs"] is list(Modes.__dataclass_fields__.values())[-1]
    # the environment is read only where the argument is None
    env = {"PC_SERVE_LOGPROBS": "5"}
    assert resolve_serve(full, 4, env=env).logprobs == 5 and resolve_serve(full, 4, env=env, logprobs=2).logprobs == 2
    assert resolve_serve(full, 4, env={"PC_SERVE_LOGPROBS": ""}).logprobs is None
    m = resolve_serve(full, 4, lookup=3, slot_kv="int8", keep_arenas=False, env={}, logprobs=0)
    assert m.loop_kwargs() == {"kv": "int8", "keep_arenas": False, "logprobs": 0} == m.loop_kwargs(one_token=True)
    assert m.reason().endswith("per-token log-probabilities with up to 0 alternatives (logprobs=0)")
    for env_bad in ("9", "-1", "x"):
        with pytest.raises(ValueError, match="PC_SERVE_LOGPROBS"):
            resolve_serve(full, 4, env={"PC_SERVE_LOGPROBS": env_bad})
    with pytest.raises(ValueError, match="0..8"):
        resolve_serve(full, 4, env={}, logprobs=9)
    # the refusal comes behind loop_prefill's own, and names the reason
    with pytest.raises(ValueError, match="lookup is off"):
        resolve_serve(full, 4, loop_prefill=True, env={}, logprobs=1)
    with pytest.raises(ValueError, match="forced row"):
        resolve_serve(full, 4, lookup=3, loop_prefill=True, env={}, logprobs=1)
    with pytest.raises(ValueError, match="forced row"):
        resolve_serve(full, 4, lookup=3, env={"PC_SERVE_LOOP_PREFILL": "1", "PC_SERVE_LOGPROBS": "1"})
    assert resolve_serve(full, 4, lookup=3, loop_prefill=True, env={}).loop_kwargs() == {"prompt_rows": True}
    assert resolve_batch(full, 4, env={"PC_SERVE_LOGPROBS": "3"}).logprobs is None        # (serve's variable, serve's mode)


def test_parameters_and_output_fields():
    import promptcache_amd
    from promptcache_amd.generation_engine import GenerationParameters, Output, TokenLogprob
    assert promptcache_amd.TokenLogprob is TokenLogprob and promptcache_amd.Output is Output
    assert GenerationParameters().logprobs is None and GenerationParameters(logprobs=0).logprobs == 0
    for bad in (-1, 9, 1.5, "2"):
        with pytest.raises(ValueError, match="GenerationParameters.logprobs"):
            GenerationParameters(logprobs=bad)
    out = Output("a b", "b", 2.0, 1.0)                                   # positional construction keeps working
    assert out.logprobs is None and list(Output.__dataclass_fields__)[-1] == "logprobs"
    r = TokenLogprob(5, -0.25, [(5, -0.25), (7, -2.0)])
    assert (r.token, r.logprob, r.top) == (5, -0.25, [(5, -0.25), (7, -2.0)]) and TokenLogprob(1, -1.0).top == []


# ---- the token-stream rule and the pumps over scripted loops ----------------------------------------------------------------------
def _rec(token, n=8):
    return (token, -token / 1e4, [(token + a, -1.0 - a) for a in range(n)])


class _OneTokenLP(_OneTokenLoop):
    def logprobs(self, i):
        self.log.append(["logprobs", i])
        return [_rec(self.toks[i])]


class _MultiTokenLP(_MultiTokenLoop):
    def logprobs(self, i):
        self.log.append(["logprobs", i])
        return [_rec(t) for t in self.toks[i]]


class _LookupSlotLP(_LookupSlotLoop):
    def logprobs(self, j, i):
        self.log.append(["logprobs", j, i])
        return [_rec(t) for t in self.steps[i][j]]


def _params(**kw):
    from promptcache_amd.generation_engine import GenerationParameters
    kw.setdefault("temperature", 0.0)
    return GenerationParameters(**kw)


def _hf(log, make_loop, multi=False):
    """A model with one single-sequence loop factory (handed ``logprobs`` only when asked) and the eager call."""
    def factory(*a, **kw):
        log.append(["loop", sorted(kw)])
        return make_loop()

    def token_logprobs(rows, tokens, n):
        log.append(["token_logprobs", list(tokens), n])
        return [_rec(t, n) for t in tokens]
    hf = types.SimpleNamespace(greedy_loop=factory, sample_loop=factory, can_loop=lambda past: True, token_logprobs=token_logprobs)
    if multi:
        hf.lookup_loop, hf.lookup_available = factory, lambda: True
    return hf


def _aligned(out, tokens, n):
    assert [r.token for r in out.logprobs] == tokens
    assert all(r.logprob == -r.token / 1e4 and r.top == _rec(r.token, n)[2] for r in out.logprobs)


def test_generate_one_token_steps_records_align_and_are_cumulative():
    log = []
    ge = _engine(log, _hf(log, lambda: _OneTokenLP(log, [11, 12, 13, 14, 15])), {None: [10]})
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=6, logprobs=2), None, stream_interval=1))
    assert [len(o.logprobs) for o in outs] == [1, 2, 3, 4, 5, 6]
    _aligned(outs[-1], [10, 11, 12, 13, 14, 15], 2)                      # the loop ranks 8, the request keeps its 2
    assert outs[2].logprobs == outs[-1].logprobs[:3] and outs[2].logprobs is not outs[-1].logprobs
    assert ["token_logprobs", [10], 2] in log and ["loop", ["logprobs"]] in log and ["logprobs", 0] in log
    # off: no accessor is called, the loop is handed nothing new, Output.logprobs is None
    log2 = []
    ge = _engine(log2, _hf(log2, lambda: _OneTokenLoop(log2, [11, 12, 13])), {None: [10]})       # (a loop without the accessor)
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=4), None, stream_interval=1))
    assert len(outs) == 4 and all(o.logprobs is None for o in outs)
    assert ["loop", []] in log2 and not any(e[0] in ("logprobs", "token_logprobs") for e in log2)


def test_generate_multi_token_steps_a_stop_id_cuts_a_step_short_and_a_stop_string_cuts_the_text_only():
    steps = [[21, 22, 23], [24], [25, 26, 27, 28]]
    log = []
    ge = _engine(log, _hf(log, lambda: _MultiTokenLP(log, steps, 3), multi=True), {None: [20]}, lookup=3)
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=9, logprobs=1), None, stream_interval=1))
    _aligned(outs[-1], [20, 21, 22, 23, 24, 25, 26, 27, 28], 1)
    log = []
    ge = _engine(log, _hf(log, lambda: _MultiTokenLP(log, steps, 3), multi=True), {None: [20]}, lookup=3)
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=9, stop_token_ids=[26], logprobs=0), None, stream_interval=2))
    _aligned(outs[-1], [20, 21, 22, 23, 24, 25, 26], 0)                  # the stop id included, the rest of its step dropped
    log = []
    ge = _engine(log, _hf(log, lambda: _MultiTokenLP(log, steps, 3), multi=True), {None: [20]}, lookup=3)
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=9, stop_str=["23 24"], logprobs=3), None, stream_interval=1))
    assert outs[-1].new_text == "20 21 22 "
    _aligned(outs[-1], [20, 21, 22, 23, 24], 3)                          # a stop string cuts the text, not the list


def test_host_steps_take_the_eager_call_per_token():
    log = []
    ge = _engine(log, types.SimpleNamespace(token_logprobs=_hf(log, None).token_logprobs), {None: [30, 31, 32]})
    outs = list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=3, logprobs=4), None, stream_interval=1))
    _aligned(outs[-1], [30, 31, 32], 4)
    assert [e for e in log if e[0] == "token_logprobs"] == [["token_logprobs", [t], 4] for t in (30, 31, 32)]
    ge = _engine([], types.SimpleNamespace(), {None: [30]})              # a model without the call: an error, not a fallback
    with pytest.raises(RuntimeError, match="token_logprobs"):
        list(ge.generate([7, 8], [0, 1], _params(max_new_tokens=2, logprobs=0), None))
    with pytest.raises(ValueError, match="GenerationParameters.logprobs"):
        p = _params(max_new_tokens=2)
        p.logprobs = 12                                                  # (set behind the constructor's check)
        list(ge.generate([7, 8], [0, 1], p, None))


def test_pump_slots_asks_only_for_streams_that_want_them():
    from promptcache_amd.generation_engine import GenerationEngine, _Stream
    render = lambda ids, new, stops: (" ".join(map(str, ids)), " ".join(map(str, new)), False, False)
    steps = [[[41, 42], [51]], [[43], [52, 53, 54]], [[], [55]]]
    log = []
    loop = _LookupSlotLP(log, steps, 3)
    a = _Stream(render, _params(max_new_tokens=4, logprobs=1), 1, [1], 5, index=0)
    b = _Stream(render, _params(max_new_tokens=6), 1, [2], 5, index=1)
    for st, first in ((a, 40), (b, 50)):
        st.emit(first, _rec(first) if st.lps is not None else None)
    outs = {}
    for index, out in GenerationEngine._pump_slots(loop, [a, b]):
        outs[index] = out
    _aligned(outs[0], [40, 41, 42, 43], 1)
    assert outs[1].logprobs is None and outs[1].new_text == "50 51 52 53 54 55"
    assert [e for e in log if e[0] == "logprobs"] == [["logprobs", 0, 0], ["logprobs", 0, 1]]
    # a loop without the accessor still serves streams that do not ask
    b2 = _Stream(render, _params(max_new_tokens=3), 1, [2], 5, index=0)
    b2.emit(50)
    got = [o.new_text for _, o in GenerationEngine._pump_slots(_LookupSlotLoop([], [[[51, 52]]], 3), [b2])]
    assert got[-1] == "50 51 52"
    # a stream that asks and gets no record is an error, not a silent None
    c = _Stream(render, _params(max_new_tokens=3, logprobs=0), 1, [2], 5)
    with pytest.raises(RuntimeError, match="without its log-probabilities"):
        c.emit(9)


class _FakeLoopLP(_FakeLoop):
    """tests/test_serve_cpu._FakeLoop with the accessor, ranking ``n`` alternatives."""
    asked = []

    def logprobs(self, k, i):
        t = self.token(k, i)
        _FakeLoopLP.asked.append((k, i))
        return [] if t is None else [_rec(t, self.n_lp)]


def _fake_serve(reqs, **serve_kw):
    made = []

    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, slots=None, slot_index=None, each=False,
                  max_keys=None, trunks=None, **kw):
        made.append(kw)
        loop = (_FakeLoopLP if "logprobs" in kw else _FakeLoop)([p.tag for p in pasts], max_new, stop_ids, slot_index)
        loop.n_lp = kw.get("logprobs")
        return loop
    log = []
    hf = types.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True, token_logprobs=_hf(log, None).token_logprobs)
    ge = _engine(log, hf, {r + 1: [1000 * (r + 1)] for r in range(len(reqs))})
    ce = types.SimpleNamespace(process=lambda prompt, slot=0, return_full_position_ids=False: ([prompt], [10 + prompt], 0.0, _cache(prompt)),
                               slots=2, max_ctx_length=4096)
    outs = {}
    for index, out in ge.serve(ce, iter(reqs), None, stream_interval=1, share_trunk=False, **serve_kw):
        outs.setdefault(index, []).append(out)
    return outs, made, ge, log


def test_serve_over_a_fake_loop_hands_out_what_each_request_asked_for(monkeypatch):
    monkeypatch.delenv("PC_SERVE_LOGPROBS", raising=False)
    asks, budgets = [3, None, 0, 3, None], [4, 6, 3, 2, 5]
    reqs = [(r + 1, _params(max_new_tokens=b, logprobs=a)) for r, (a, b) in enumerate(zip(asks, budgets))]
    _FakeLoopLP.asked = []
    outs, made, ge, log = _fake_serve(reqs, logprobs=3)
    assert made == [{"logprobs": 3}]
    for r, (a, b) in enumerate(zip(asks, budgets)):
        toks = [1000 * (r + 1) + j for j in range(b)]
        assert ge.last_serve_tokens[r] == toks
        if a is None:
            assert all(o.logprobs is None for o in outs[r])
        else:
            _aligned(outs[r][-1], toks, a)
            assert [len(o.logprobs) for o in outs[r]] == list(range(1, b + 1))
    assert [e[1:] for e in log if e[0] == "token_logprobs"] == [[[1000], 3], [[3000], 0], [[4000], 3]]     # first tokens, asked for only
    # off: the model is handed nothing new and no loop is asked
    plain = [(r + 1, _params(max_new_tokens=b)) for r, b in enumerate(budgets)]
    outs, made, ge, log = _fake_serve(plain)
    assert made == [{}] and all(o.logprobs is None for os_ in outs.values() for o in os_)
    monkeypatch.setenv("PC_SERVE_LOGPROBS", "2")
    outs, made, ge, log = _fake_serve(plain)
    assert made == [{"logprobs": 2}] and all(o.logprobs is None for os_ in outs.values() for o in os_)


def test_serve_admission_errors(monkeypatch):
    monkeypatch.delenv("PC_SERVE_LOGPROBS", raising=False)
    ok = (1, _params(max_new_tokens=3, logprobs=1))
    with pytest.raises(ValueError, match=r"asks for logprobs=4.*ranks 3 alternatives.*serve\(logprobs=n\) with n >= 4"):
        _fake_serve([ok, (2, _params(max_new_tokens=3, logprobs=4))], logprobs=3)
    with pytest.raises(ValueError, match=r"asks for logprobs=0.*carries no log-probability node.*serve\(logprobs=n\)"):
        _fake_serve([(1, _params(max_new_tokens=3, logprobs=0))])
    with pytest.raises(ValueError, match="0..8"):
        _fake_serve([ok], logprobs=11)
    outs, made, ge, log = _fake_serve([ok, (2, _params(max_new_tokens=3, logprobs=4))], logprobs=4)
    assert [len(r.top) for r in outs[0][-1].logprobs] == [1, 1, 1] and [len(r.top) for r in outs[1][-1].logprobs] == [4, 4, 4]
    # a refused request is refused before it is processed or prefilled
    log, seen = [], []
    ce_process = lambda prompt, slot=0, return_full_position_ids=False: seen.append(prompt)
    ge = _engine(log, types.SimpleNamespace(slot_loop=None, slot_loop_available=lambda: True), {})
    ce = types.SimpleNamespace(process=ce_process, slots=2, max_ctx_length=4096)
    with pytest.raises(ValueError, match=r"serve\(logprobs="):
        list(ge.serve(ce, iter([(1, _params(logprobs=2))]), None, share_trunk=False, logprobs=1))
    assert seen == [] and log == []


# ---- the C entry's argument errors need no GPU ------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    buf = (ctypes.c_float * 64)()
    one = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(one.value + 2)
    good = dict(logits=one, ldl=16, vocab=16, rows=2, tok64=one, tok32=None, stride=1, top_n=8, ids=one, lp=one)

    def call(**kw):
        a = {**good, **kw}
        return lib.pc_token_logprobs(a["logits"], a["ldl"], a["vocab"], a["rows"], a["tok64"], a["tok32"], a["stride"], a["top_n"],
                                     a["ids"], a["lp"], None)
    for bad in (dict(logits=None), dict(ids=None), dict(lp=None), dict(tok64=None), dict(tok32=one), dict(rows=0), dict(rows=65),
                dict(top_n=-1), dict(top_n=9), dict(vocab=8, ldl=8), dict(vocab=1 << 24, ldl=1 << 24), dict(ldl=15), dict(stride=0),
                dict(logits=odd), dict(tok64=ctypes.c_void_p(one.value + 4)), dict(ids=odd), dict(lp=odd)):
        assert call(**bad) == -1001, bad
        assert b"pc_token_logprobs" in lib.pc_last_error_string()
    assert _native.LOGPROBS_MAX_TOP == 8 and "pc_token_logprobs" in _native.SIGNATURES
    src = open(_native.lib_path().replace("promptcache_amd/libpromptcache_hip.so", "../include/promptcache_hip.h")).read()
    assert "#define PC_LOGPROBS_MAX_TOP 8" in src
    contract = src[src.index("pc_token_logprobs:"):src.index("#define PC_LOGPROBS_MAX_TOP")]
    assert "BEFORE temperature, repetition penalty, top-p and top-k" in contract
