"""Token controls end to end on the GPU: the ``pc_logit_adjust`` node in front of every device loop's draw, the eager
call, and ``generate`` / ``generate_batch`` / ``serve``.

The truth of a token is the CPU chain applied to the loop's OWN raw logits row of that step, read back with one replay enqueued at
a time: the rule of tests/logit_ctl_ref.py, then the existing sampling reference (tests/sample_ref.py ``draw``: the oracle's chain,
Philox, Gumbel-max, "lowest index among equal maxima").  Greedy tokens are exact.  A sampled draw races fp32 scores on the device
against float64 ones here, so -- as in tests/test_gpu_sample.py -- it is compared where the reference's own margin between the best
and the second-best score exceeds 1e-4, and most steps must be that clear.  Two PATHS (``serve`` against ``generate``) are compared
the way tests/test_gpu_logprob_model.py compares them: greedy tokens equal."""
import pytest
import torch

from tests import logit_ctl_ref as ref
from tests import logprob_ref
from tests import sample_ref as sr
from tests import trunk_helpers as th

pytestmark = pytest.mark.gpu
DEV = th.DEV
N_NEW = 12
MARGIN = 1e-4
SAMPLED = dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40)


@pytest.fixture(scope="module")
def mid():
    shape, w16, lm, eng, prompts = th.mid_setup(3, 9, 4, th.PICKS)
    assert lm.hf_model.slot_loop_available() and lm.hf_model.lookup_available() and lm.hf_model.D == 128
    return lm, eng, prompts


def _params(**kw):
    from promptcache_amd.generation_engine import GenerationParameters
    kw.setdefault("stop_token_ids", [])
    return GenerationParameters(max_new_tokens=N_NEW, stop_str=[], **kw)


def _ctl(stop=(), **kw):
    from promptcache_amd.modes import token_controls
    return token_controls(stop_token_ids=list(stop), vocab=2048, **kw)


def _fresh(lm, eng, prompt, slot, ctl=None, params=None, seed=0):
    """A fresh prefill of ``prompt`` in ``slot`` -> (past, first token drawn under ``ctl``, its position, history ids)."""
    ids, pos, out = th.prefill(lm, eng, prompt, slot)
    row = lm.hf_model.adjust_logits(out.logits[0, -1], ctl, 0)
    first = int(torch.argmax(row)) if params is None else lm.hf_model.sample_token(row, params, seed, list(ids))
    return out.past_key_values, first, max(pos) + 2, list(ids) + [first]


def _new_at(t, start):
    """The first index >= ``start`` whose token the run had not emitted before (a condition on the inputs: it must exist early
    enough for the controls built on it to bite)."""
    i = next(i for i in range(start, len(t)) if t[i] not in t[:i])
    assert i <= start + 2, (t, start)
    return i


class _Chain:
    """The reference chain over the rows a loop hands back: ``check(row, token, g, hist, step)`` counts clear and unclear draws."""

    def __init__(self, ctl, params=None, seed=0):
        self.ctl, self.seed, self.sure, self.unsure = ctl, seed, 0, 0
        self.p = (0.0, 1.0, 1.0, -1) if params is None else (params.temperature, params.repetition_penalty, params.top_p, params.top_k)
        self.greedy = params is None

    def check(self, row, token, g, hist, what):
        a = ref.adjust_controls(row, self.ctl, g)
        want, margin, _ = sr.draw(a, hist, *self.p, self.seed, g)          # (token number g is drawn at Philox step g)
        if self.greedy or margin > MARGIN:
            assert int(token) == want, (what, g, token, want, margin)
            self.sure += 1
        else:
            self.unsure += 1

    def done(self):
        print(f"[logit ctl model] chain: {self.sure} tokens equal the reference's, {self.unsure} draws within {MARGIN} not compared")
        assert self.sure >= 3 * self.unsure and self.sure > 0, (self.sure, self.unsure)


# ---- the single-sequence loops ----------------------------------------------------------------------------------------------------
def _loop_run(lm, eng, prompt, ctl, sampled, mention=True, logprobs=None):
    m = lm.hf_model
    params = _params(**SAMPLED) if sampled else None
    past, first, pos, hist = _fresh(lm, eng, prompt, 0, ctl, params, 77)
    kw = {"token_controls": ctl} if mention else {}
    if logprobs is not None:
        kw["logprobs"] = logprobs
    loop = m.sample_loop(past, first, pos, N_NEW, params, 77, hist, **kw) if sampled else m.greedy_loop(past, first, pos, N_NEW, **kw)
    chain = _Chain(ctl, params, 77)
    toks, recs, rows = [first], [], []
    for i in range(N_NEW - 1):
        loop.enqueue()
        t = loop.token(i)
        rows.append(loop._last_ent[1].reshape(-1).float().cpu().numpy())
        chain.check(rows[-1], t, i + 1, hist + toks[1:], "loop")
        toks.append(t)
        if logprobs is not None:
            recs += loop.logprobs(i)
    loop.close(N_NEW - 3)
    chain.done()
    return toks, loop.arena.length, set(m._graphs), recs, rows


@pytest.mark.parametrize("sampled", [False, True])
def test_greedy_and_sample_loop(mid, sampled):
    lm, eng, prompts = mid
    base = set(lm.hf_model._graphs)
    t0, len0, keys0, _, _ = _loop_run(lm, eng, prompts[0], None, sampled, mention=False)
    t1, len1, keys1, _, _ = _loop_run(lm, eng, prompts[0], None, sampled)
    assert (t1, len1, keys1) == (t0, len0, keys0) and not any("ctl" in k for k in keys0 - base)      # empty controls: the parent's run
    assert _ctl() is None and _ctl(logit_bias={}, banned_token_ids=[], min_new_tokens=4) is None
    # a ban on the token of step 3 (the first new one from there): the same prefix, and the token never appears
    b = _new_at(t0, 3)
    t2, len2, keys2, _, _ = _loop_run(lm, eng, prompts[0], _ctl(banned_token_ids=[t0[b]]), sampled)
    assert keys2 > keys0 and all(k[-1] == "ctl" for k in keys2 - keys0) and len2 == len0
    if not sampled:
        assert t2[:b] == t0[:b] and t0[b] not in t2
    # an allow-list of three tokens, a bias on one of them and one on a token outside it
    allow = sorted(set(t0))[:3]
    assert len(allow) == 3
    t3, _, keys3, _, _ = _loop_run(lm, eng, prompts[0], _ctl(allowed_token_ids=allow, logit_bias={allow[0]: 2.0, 5: 30.0}), sampled)
    assert set(t3) <= set(allow) and keys3 == keys2                                                   # one graph serves every block
    # min_new_tokens = 6 over the token of step 2: held back for the generated tokens 0..5
    s2 = _new_at(t0, 2)
    t4, _, _, _, _ = _loop_run(lm, eng, prompts[0], _ctl(stop=[t0[s2]], min_new_tokens=6), sampled)
    assert t0[s2] not in t4[:6] and (sampled or (t4[:s2] == t0[:s2] and t4 != t0))


def test_logprobs_stay_the_raw_rows_under_a_ban(mid):
    lm, eng, prompts = mid
    t0 = _loop_run(lm, eng, prompts[0], None, False, mention=False)[0]
    b = _new_at(t0, 3)
    toks, _, _, recs, rows = _loop_run(lm, eng, prompts[0], _ctl(banned_token_ids=[t0[b]]), False, logprobs=2)
    assert len(recs) == len(rows) == N_NEW - 1
    worst, seen = 0.0, False
    for rec, x, t in zip(recs, rows, toks[1:]):
        ids, lp = logprob_ref.record(x, int(t), 2)
        assert rec[0] == int(t) == ids[0] and [a for a, _ in rec[2]] == ids[1:].tolist()
        worst = max([worst, abs(rec[1] - lp[0])] + [abs(b - w) for (_, b), w in zip(rec[2], lp[1:])])
        seen = seen or t0[b] in ids[1:].tolist()
    assert worst <= logprob_ref.TOL and seen                       # the banned token is still the raw row's most likely one at its step


@pytest.mark.parametrize("sampled", [False, True])
def test_lookup_loops_with_the_boundary_inside_a_step(mid, sampled):
    from promptcache_amd.model.llama_hip import LookupLoop, SampleLookupLoop
    lm, eng, prompts = mid
    m = lm.hf_model
    k = 3
    params = _params(**SAMPLED) if sampled else None
    more = dict(params=params, seed=77) if sampled else {}

    def run(corpus, ctl, mention=True):
        past, first, pos, hist = _fresh(lm, eng, prompts[1], 1, ctl, params, 77)
        kw = {"token_controls": ctl} if mention else {}
        loop = m.lookup_loop(past, first, pos, N_NEW - 1, k, [first] + corpus, **more, **(dict(history_ids=hist) if sampled else {}), **kw)
        assert type(loop) is (SampleLookupLoop if sampled else LookupLoop)
        chain = _Chain(ctl, params, 77)
        toks, steps = [first], []
        while len(toks) < N_NEW:
            i = loop.enqueue()
            got = loop.tokens(i)
            rows = m._lookup_graph(loop)[1].reshape(k + 1, -1)[:len(got)].float().cpu().numpy()
            for r, t in enumerate(got):
                chain.check(rows[r], t, len(toks), hist + toks[1:], "lookup")
                toks.append(t)
            steps.append(got)
        loop.close(N_NEW - 3)
        chain.done()
        return toks, steps, loop.arena.length, set(m._graphs)

    t0, _, len0, keys0 = run([], None, mention=False)
    t1, _, len1, keys1 = run([], None)
    assert (t1, len1, keys1) == (t0, len0, keys0)
    allow = sorted(set(t0))[:3]
    ta, _, _, keys_a = run(t0[1:], _ctl(allowed_token_ids=allow))
    assert set(ta) <= set(allow) and all(key[-1] == "ctl" for key in keys_a - keys0) and keys_a > keys0
    # min_new_tokens = 6 over the token of step 2, on a corpus that holds the controlled answer: every draft is right, a step
    # emits k + 1 = 4 tokens, and the boundary between token numbers 5 and 6 falls between two rows of one step
    s2 = _new_at(t0, 2)
    ctl = _ctl(stop=[t0[s2]], min_new_tokens=6)
    tc = run([], ctl)[0]
    tm, steps, _, _ = run(tc[1:], ctl)
    assert tm == tc and t0[s2] not in tm[:6] and (sampled or tm != t0)
    g0 = 1
    inside = False
    for s in steps:
        inside = inside or (g0 < 6 <= g0 + len(s) - 1)
        g0 += len(s)
    assert inside, steps


# ---- the batched loops ------------------------------------------------------------------------------------------------------------
def _slot_run(lm, eng, prompts, ctls, mention=True, **kw):
    """SlotLoop over S = 3 slots: sequences in slots 0 and 2, slot 1 idle; ``ctls``: one ``TokenControls`` (or None) per sequence."""
    m = lm.hf_model
    fr = [_fresh(lm, eng, prompts[j], s, c) for (j, s), c in zip(((0, 0), (2, 2)), ctls or [None, None])]
    more = {"token_controls": ctls} if mention else {}
    loop = m.slot_loop([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], N_NEW, stop_ids=[], slots=3, slot_index=[0, 2], **kw, **more)
    chains = [_Chain(c) for c in (ctls or [None, None])]
    toks = [[f[1]] for f in fr]
    for i in range(N_NEW - 1):
        loop.enqueue()
        for j in range(2):
            t = loop.token(j, i)
            chains[j].check(loop.logits[loop.idx[j]].float().cpu().numpy(), t, i + 1, [], f"slot sequence {j}")
            toks[j].append(t)
    loop.close([N_NEW - 1, N_NEW - 1])
    for c in chains:
        c.done()
    return toks, [getattr(a, "length", None) for a in loop.arenas], set(m._graphs), type(loop).__name__


@pytest.mark.parametrize("kv", [dict(), dict(kv="int8"), dict(kv="int8", keep_arenas=False)])
def test_slot_loop_with_a_block_per_slot(mid, kv):
    lm, eng, prompts = mid
    t0, len0, keys0, name = _slot_run(lm, eng, prompts, None, mention=False, **kv)
    t1, len1, keys1, _ = _slot_run(lm, eng, prompts, None, **kv)
    assert (t1, len1, keys1) == (t0, len0, keys0)
    allow = sorted(set(t0[0]))[:3]
    ctls = [_ctl(allowed_token_ids=allow, banned_token_ids=[allow[2]], stop=[allow[0]], min_new_tokens=4), None]
    t2, len2, keys2, _ = _slot_run(lm, eng, prompts, ctls, **kv)
    assert set(t2[0]) <= set(allow[:2]) and allow[0] not in t2[0][:4] and t2[1] == t0[1] and len2 == len0      # slot 2 is untouched
    assert keys2 > keys0 and all(k[-1] == "ctl" for k in keys2 - keys0), name
    # the blocks swapped: each sequence follows its own
    b = _new_at(t0[1], 3)
    t3 = _slot_run(lm, eng, prompts, [None, _ctl(banned_token_ids=[t0[1][b]])], **kv)[0]
    assert t3[0] == t0[0] and t3[1][:b] == t0[1][:b] and t0[1][b] not in t3[1]


def test_lookup_slot_loop_with_the_boundary_inside_a_step(mid):
    lm, eng, prompts = mid
    m = lm.hf_model
    k = 3

    def run(corpora, ctls, mention=True, **kw):
        fr = [_fresh(lm, eng, prompts[j], j, c) for j, c in zip(range(2), ctls or [None, None])]
        cs = [[f[1]] + c for f, c in zip(fr, corpora)]
        more = {"token_controls": ctls} if mention else {}
        loop = m.lookup_slot_loop([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], N_NEW - 1, k, cs, slots=2, **kw, **more)
        chains = [_Chain(c) for c in (ctls or [None, None])]
        toks, steps = [[f[1]] for f in fr], [[], []]
        while any(len(t) < N_NEW for t in toks):
            i = loop.enqueue()
            for j in range(2):
                got = loop.tokens(j, i)
                r0 = loop.idx[j] * (k + 1)
                rows = loop.logits[r0:r0 + len(got)].float().cpu().numpy()
                for r, t in enumerate(got):
                    chains[j].check(rows[r], t, len(toks[j]), [], f"lookup slot sequence {j}")
                    toks[j].append(t)
                steps[j].append(got)
        loop.close([N_NEW - 1, N_NEW - 1])
        for c in chains:
            c.done()
        return toks, steps, [a.length for a in loop.arenas], set(m._graphs)

    t0, _, len0, keys0 = run([[], []], None, mention=False)
    t1, _, len1, keys1 = run([[], []], None)
    assert (t1, len1, keys1) == (t0, len0, keys0)
    allow = sorted(set(t0[0]))[:3]
    s2 = _new_at(t0[1], 2)
    ctls = [_ctl(allowed_token_ids=allow), _ctl(stop=[t0[1][s2]], min_new_tokens=6)]
    tc, _, _, keys_c = run([[], []], ctls)
    assert set(tc[0]) <= set(allow) and t0[1][s2] not in tc[1][:6] and tc[1] != t0[1] and keys_c > keys0 and all(key[-1] == "ctl" for key in keys_c - keys0)
    tm, steps, _, _ = run([t[1:] for t in tc], ctls)               # every draft right: steps of k + 1 tokens
    assert tm == tc
    g0, inside = 1, False
    for s in steps[1]:
        inside = inside or (g0 < 6 <= g0 + len(s) - 1)
        g0 += len(s)
    assert inside, steps[1]
    tq = run([[], []], ctls, kv="int8")[0]                         # ... and over int8 images the allow-list holds (chain checked above)
    assert set(tq[0]) <= set(allow)
    with pytest.raises(ValueError, match="loop_prefill=True and token controls"):
        m.lookup_slot_loop([], [], [], N_NEW, k, [], each=True, prompt_rows=True, token_controls=True)


# ---- the engine -------------------------------------------------------------------------------------------------------------------
def test_generate_and_generate_batch(mid):
    from promptcache_amd import GenerationEngine
    lm, eng, prompts = mid

    def ids_of(ge, params, prompt=prompts[0]):
        """The generated ids: read from the log-probability records (``logprobs=0`` adds a node behind the draw, nothing else)."""
        ids, pos, _, cache = eng.process(prompt)
        outs = list(ge.generate(ids, pos, params, cache))
        return [r.token for r in outs[-1].logprobs]

    ge = GenerationEngine(lm)
    t0 = ids_of(ge, _params(temperature=0.0, logprobs=0))
    assert len(t0) == N_NEW
    b = _new_at(t0, 3)
    tb = ids_of(ge, _params(temperature=0.0, logprobs=0, banned_token_ids=[t0[b]]))
    assert tb[:b] == t0[:b] and t0[b] not in tb and len(tb) == N_NEW
    allow = sorted(set(t0))[:3]
    for engine, kw in ((ge, dict(temperature=0.0)), (ge, SAMPLED), (GenerationEngine(lm, lookup=3), dict(temperature=0.0)),
                       (GenerationEngine(lm, lookup=3, lookup_sampled=True), SAMPLED)):
        torch.manual_seed(3)
        ta = ids_of(engine, _params(logprobs=0, allowed_token_ids=allow, **kw))
        assert len(ta) == N_NEW and set(ta) <= set(allow), (kw, ta)
    # min_new_tokens: the stop id is the token of step 2; without it the run ends there, with it at least 6 tokens come out
    s2 = _new_at(t0, 2)
    stop = t0[s2]
    for engine in (ge, GenerationEngine(lm, lookup=3)):
        cut = ids_of(engine, _params(temperature=0.0, logprobs=0, stop_token_ids=[stop]))
        assert cut == t0[:s2 + 1]
        tm = ids_of(engine, _params(temperature=0.0, logprobs=0, stop_token_ids=[stop], min_new_tokens=6))
        assert len(tm) >= 6 and stop not in tm[:6] and tm[:s2] == t0[:s2] and (stop not in tm or tm.index(stop) == len(tm) - 1)
    # the host-stepped path gives the device loop's tokens
    host = GenerationEngine(lm)
    host.device_greedy_loop = host.device_sample_loop = False
    assert ids_of(host, _params(temperature=0.0, logprobs=0, banned_token_ids=[t0[b]]))[:b] == t0[:b]
    th_ = ids_of(host, _params(temperature=0.0, logprobs=0, allowed_token_ids=allow))
    assert set(th_) <= set(allow) and len(th_) == N_NEW
    # generate_batch: one parameter set, every slot the same block
    for kw in ({}, dict(lookup=3), dict(slot_kv="int8")):
        reqs = [eng.process(p, slot=j) for j, p in enumerate(prompts[:3])]
        outs = th.collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], _params(temperature=0.0, logprobs=0, allowed_token_ids=allow), **kw))
        for j in range(3):
            tj = [r.token for r in outs[j][-1].logprobs]
            assert len(tj) == N_NEW and set(tj) <= set(allow), (kw, j, tj)
            if "slot_kv" not in kw:                # (int8 images: the format's logits, not generate's)
                assert tj == ids_of(ge, _params(temperature=0.0, logprobs=0, allowed_token_ids=allow), prompts[j])


def _schema_text(lm):
    from promptcache_amd import synth
    sp, _ = synth.persona_like("deep", system_len=60, intro_len=20, traits=th.TRAITS, question_len=8, seed=6, pick=(0, 1))
    return lm.get_formatter()(sp)


@pytest.mark.parametrize("mode", [dict(), dict(lookup=3), dict(slot_kv="int8")])
def test_serve(mid, mode):
    """2 slots, 6 requests: two with different controls and four without share the loop; the later ones re-arm the slots the
    controlled ones held."""
    from promptcache_amd import CacheEngine, GenerationEngine
    from promptcache_amd.generation_engine import GenerationParameters
    lm, _, prompts = mid
    eng = CacheEngine(2048, lm, slots=2)
    eng.add_schema(_schema_text(lm))
    ge = GenerationEngine(lm)
    budgets = [7, 12, 9, 6, 8, 5]
    ps = [prompts[i % 4] for i in range(6)]

    def reqs(extra):
        return [(p, GenerationParameters(temperature=0.0, max_new_tokens=b, **e)) for p, b, e in zip(ps, budgets, extra)]

    off = th.collect(ge.serve(eng, iter(reqs([{}] * 6)), **mode))
    toks_off = {r: list(v) for r, v in ge.last_serve_tokens.items()}
    keys_off = set(lm.hf_model._graphs)
    assert [o[-1].new_text for o in off.values()]
    # the mode on and nobody asking: the same tokens through the neutral blocks
    th.collect(ge.serve(eng, iter(reqs([{}] * 6)), token_controls=True, **mode))
    assert {r: list(v) for r, v in ge.last_serve_tokens.items()} == toks_off
    assert all(k[-1] == "ctl" for k in set(lm.hf_model._graphs) - keys_off) and set(lm.hf_model._graphs) > keys_off
    allow = sorted(set(toks_off[0]))[:3]
    s2 = _new_at(toks_off[1], 2)
    b = _new_at(toks_off[1], s2 + 1)
    stop, ban = toks_off[1][s2], toks_off[1][b]
    extra = [dict(allowed_token_ids=allow), dict(banned_token_ids=[ban], stop_token_ids=[stop], min_new_tokens=6), {}, {}, {}, {}]
    th.collect(ge.serve(eng, iter(reqs(extra)), token_controls=True, **mode))
    toks = {r: list(v) for r, v in ge.last_serve_tokens.items()}
    assert set(toks[0]) <= set(allow) and len(toks[0]) == budgets[0]
    assert len(toks[1]) >= 6 and stop not in toks[1][:6] and ban not in toks[1] and toks[1][:s2] == toks_off[1][:s2]
    for r in range(2, 6):                          # no trace of a predecessor's block in a re-armed slot
        assert toks[r] == toks_off[r], r
    if "slot_kv" not in mode:                      # each controlled request against its own generate (int8: another format's logits)
        for r in range(2):
            ids, pos, _, cache = eng.process(ps[r])
            solo = list(ge.generate(ids, pos, GenerationParameters(temperature=0.0, max_new_tokens=budgets[r], logprobs=0, **extra[r]), cache))
            assert [x.token for x in solo[-1].logprobs] == toks[r], r


def test_falcon_host_stepped_allow_list():
    from promptcache_amd import CacheEngine, GenerationEngine, Prompt, synth
    from promptcache_amd.generation_engine import GenerationParameters
    from promptcache_amd.model import Falcon
    from promptcache_amd.model.config import FALCON_SHAPES
    from promptcache_amd.model.weights import make_falcon_weights_np
    shape = FALCON_SHAPES["falcon-mid"]
    lm = Falcon(name="falcon-mid", shape=shape, weights=make_falcon_weights_np(shape, 3, 2.0), device=DEV)
    eng = CacheEngine(1024, lm)
    sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=th.TRAITS, question_len=8, seed=6, pick=(0, 1))
    eng.add_schema(lm.get_formatter()(sp))
    prompt = Prompt(pp, [lm.get_formatter()])
    ge = GenerationEngine(lm)
    ge.device_greedy_loop = ge.device_sample_loop = False          # one forward per token on the host
    out = {}
    for name, kw in (("free", {}), ("allow", dict(allowed_token_ids=[11, 400, 1999])), ("ban", None)):
        if kw is None:
            kw = dict(banned_token_ids=[out["free"][2]])
        ids, pos, _, cache = eng.process(prompt)
        outs = list(ge.generate(ids, pos, GenerationParameters(temperature=0.0, max_new_tokens=6, logprobs=0, **kw), cache))
        out[name] = [r.token for r in outs[-1].logprobs]
    assert len(out["allow"]) == 6 and set(out["allow"]) <= {11, 400, 1999}
    assert out["ban"][:2] == out["free"][:2] and out["free"][2] not in out["ban"]


def test_value_errors(mid):
    from promptcache_amd import CacheEngine, GenerationEngine
    from promptcache_amd.generation_engine import GenerationParameters
    lm, _, prompts = mid
    eng = CacheEngine(2048, lm, slots=2)
    eng.add_schema(_schema_text(lm))
    ge = GenerationEngine(lm)
    ask = lambda **kw: [(prompts[0], GenerationParameters(temperature=0.0, max_new_tokens=4, **kw))]
    with pytest.raises(ValueError, match=r"call serve\(token_controls=True\)"):
        list(ge.serve(eng, iter(ask(banned_token_ids=[3]))))
    with pytest.raises(ValueError, match="loop_prefill=True and token controls"):
        list(ge.serve(eng, iter(ask(banned_token_ids=[3])), lookup=3, loop_prefill=True))
    with pytest.raises(ValueError, match="loop_prefill=True and token controls"):
        list(ge.serve(eng, iter(ask()), lookup=3, loop_prefill=True, token_controls=True))
    with pytest.raises(ValueError, match="at most 8 stop token ids"):
        ask(stop_token_ids=list(range(10, 19)), min_new_tokens=2)
    with pytest.raises(ValueError, match=r"outside the vocabulary \[0, 2048\)"):
        list(ge.serve(eng, iter(ask(logit_bias={2048: 1.0})), token_controls=True))
    assert lm.hf_model._live_loop is None
    out = th.collect(ge.serve(eng, iter(ask(allowed_token_ids=[7, 8])), token_controls=True))          # ... and the engine serves afterwards
    assert out[0][-1].new_text is not None and set(ge.last_serve_tokens[0]) <= {7, 8}
