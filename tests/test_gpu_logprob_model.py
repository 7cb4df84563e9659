"""Per-token log-probabilities end to end on the GPU: the node behind every device loop's last stage, the eager call,
and ``generate`` / ``generate_batch`` / ``serve``.

The truth of a record is the float64 log-softmax (tests/logprob_ref.py) of the loop's OWN logits row, read back with one replay
enqueued at a time: the slot loops expose ``loop.logits``, the single-sequence graph entries hold their output row.  Tokens and
alternative ids are exact, log-probabilities within 2e-4 (the kernel's bound, tests/test_gpu_logprob.py).  With ``logprobs=n``
against ``None`` every loop form gives the same tokens bit for bit and the same arena lengths, and with ``None`` the graph keys are
the ones of a run that never mentions the argument.

Where two PATHS are compared (device loop against host steps, ``serve`` against ``generate``) their logits may differ by the
project's parity bar d = 1e-2 (tests/test_gpu_engine.py); a log-probability x_j - m - log s then moves by at most 2 d, so records of
the same token are compared at 2 * 1e-2 + 2 * 2e-4."""
import math

import pytest
import torch

from tests import logprob_ref as ref
from tests import trunk_helpers as th

pytestmark = pytest.mark.gpu
DEV = th.DEV
TOL = ref.TOL
PATH_TOL = 2 * 1e-2 + 2 * TOL
N_NEW = 14
SAMPLED = dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40)


@pytest.fixture(scope="module")
def mid():
    shape, w16, lm, eng, prompts = th.mid_setup(3, 9, 4, th.PICKS)
    assert lm.hf_model.slot_loop_available() and lm.hf_model.lookup_available() and lm.hf_model.D == 128
    return lm, eng, prompts


def _fresh(lm, eng, prompt, slot, params=None, seed=0):
    """A fresh prefill of ``prompt`` in ``slot`` -> (past, first token, its position, history ids, the prefill's last row)."""
    ids, pos, out = th.prefill(lm, eng, prompt, slot)
    row = out.logits[0, -1]
    first = int(torch.argmax(row)) if params is None else lm.hf_model.sample_token(row, params, seed, list(ids))
    return out.past_key_values, first, max(pos) + 2, list(ids) + [first], row


def _check(recs, rows, tokens, n, what):
    """``recs`` (one per token) against the float64 truth of ``rows`` (fp32, one per token)."""
    assert len(recs) == len(tokens) == len(rows), (what, len(recs), len(tokens), len(rows))
    worst = 0.0
    for rec, x, t in zip(recs, rows, tokens):
        ids, lp = ref.record(x, int(t), n)
        assert rec[0] == int(t) == ids[0], (what, rec[0], t)
        assert [a for a, _ in rec[2]] == ids[1:].tolist(), (what, rec[2], ids)
        worst = max([worst, abs(rec[1] - lp[0])] + [abs(b - w) for (_, b), w in zip(rec[2], lp[1:])])
    print(f"[logprob model] {what}: max |lp - float64| = {worst:.3e} over {len(recs)} tokens")
    assert worst <= TOL, (what, worst)


def _params(**kw):
    from promptcache_amd.generation_engine import GenerationParameters
    return GenerationParameters(max_new_tokens=N_NEW, stop_token_ids=[], stop_str=[], **kw)


# ---- the single-sequence loops ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampled", [False, True])
def test_greedy_and_sample_loop(mid, sampled):
    lm, eng, prompts = mid
    m = lm.hf_model
    params = _params(**SAMPLED) if sampled else None

    def run(n_lp, mention=True):
        past, first, pos, hist, _ = _fresh(lm, eng, prompts[0], 0, params, 77)
        kw = {"logprobs": n_lp} if mention else {}
        loop = m.sample_loop(past, first, pos, N_NEW, params, 77, hist, **kw) if sampled else m.greedy_loop(past, first, pos, N_NEW, **kw)
        toks, recs, rows = [], [], []
        for i in range(N_NEW):
            loop.enqueue()
            toks.append(loop.token(i))
            if n_lp is not None:
                recs += loop.logprobs(i)
                rows.append(loop._last_ent[1].reshape(-1).float().cpu().numpy())
        loop.close(N_NEW - 3)
        return toks, recs, rows, loop.arena.length, set(m._graphs)

    base = set(m._graphs)                                              # (the model is shared with the tests in front)
    t0, _, _, len0, keys0 = run(None, mention=False)
    t1, _, _, len1, keys1 = run(None)
    assert (t1, len1, keys1) == (t0, len0, keys0)                      # None: the keys of a run that never mentions the argument
    assert keys0 > base and not any("logprobs" in k for k in keys0 - base)
    for n in (0, 3):
        t2, recs, rows, len2, keys2 = run(n)
        assert (t2, len2) == (t0, len0)
        assert keys2 > keys1 and all(k[-2:] == ("logprobs", n) for k in keys2 - keys1)
        keys1 = keys2
        _check(recs, rows, t2, n, f"{'SampleLoop' if sampled else 'GreedyLoop'} n={n}")
        if not sampled and n:
            assert all(r[0] == r[2][0][0] and r[1] == r[2][0][1] for r in recs)      # greedy: the token is the first alternative


@pytest.mark.parametrize("sampled", [False, True])
def test_lookup_loops(mid, sampled):
    """k = 3 on a corpus that holds the answer with two tokens changed: some drafts are accepted, some rejected."""
    from promptcache_amd.model.llama_hip import LookupLoop, SampleLookupLoop
    lm, eng, prompts = mid
    m = lm.hf_model
    k, n = 3, 3
    params = _params(**SAMPLED) if sampled else None
    more = dict(params=params, seed=77) if sampled else {}

    def run(corpus, **kw):
        past, first, pos, hist, _ = _fresh(lm, eng, prompts[1], 1, params, 77)
        loop = m.lookup_loop(past, first, pos, N_NEW, k, [first] + corpus, **more, **(dict(history_ids=hist) if sampled else {}), **kw)
        assert type(loop) is (SampleLookupLoop if sampled else LookupLoop)
        steps, recs, rows = [], [], []
        while sum(map(len, steps)) < N_NEW:
            i = loop.enqueue()
            toks = loop.tokens(i)
            steps.append(toks)
            if kw.get("logprobs") is not None:
                recs.append(loop.logprobs(i))
                rows.append(m._lookup_graph(loop)[1].reshape(k + 1, -1)[:len(toks)].float().cpu().numpy())
        loop.close(N_NEW - 2)
        return steps, recs, rows, loop.arena.length, set(m._graphs)

    corpus = [t for s in run([])[0] for t in s]
    corpus[4] = (corpus[4] + 1) % 2048 or 3
    corpus[9] = (corpus[9] + 1) % 2048 or 3
    s0, _, _, len0, keys0 = run(corpus)
    T = [t for s in s0 for t in s]
    assert len(T) == N_NEW and any(len(s) > 1 for s in s0) and len(s0) > math.ceil(N_NEW / (k + 1))
    if not sampled:
        assert T[:4] + T[5:9] + T[10:] == corpus[:4] + corpus[5:9] + corpus[10:]
    s1, _, _, len1, keys1 = run(corpus, logprobs=None)
    assert (s1, len1, keys1) == (s0, len0, keys0)
    s2, recs, rows, len2, keys2 = run(corpus, logprobs=n)
    assert (s2, len2) == (s0, len0) and keys2 > keys0 and all("logprobs" in key for key in keys2 - keys0)
    assert [len(r) for r in recs] == [len(s) for s in s2]
    _check([r for rs in recs for r in rs], [x for xs in rows for x in xs], T, n, "SampleLookupLoop" if sampled else "LookupLoop")


# ---- the batched loops ------------------------------------------------------------------------------------------------------------
def _slot_run(lm, eng, prompts, n_lp, mention=True, **kw):
    """SlotLoop over S = 3 slots: sequences in slots 0 and 2, slot 1 idle, sequence 0 stopped early by a stop id."""
    m = lm.hf_model
    fr = [_fresh(lm, eng, prompts[j], s) for j, s in ((0, 0), (2, 2))]
    stop = kw.pop("stop")
    lp = {"logprobs": n_lp} if mention else {}
    loop = m.slot_loop([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], N_NEW, stop_ids=stop, slots=3, slot_index=[0, 2], **kw, **lp)
    toks, recs, rows = [[], []], [[], []], [[], []]
    for i in range(N_NEW):
        loop.enqueue()
        for j in range(2):
            t = loop.token(j, i)
            if n_lp is not None:
                r = loop.logprobs(j, i)
                assert len(r) == (t is not None)
                recs[j] += r
            if t is not None:
                toks[j].append(t)
                rows[j].append(loop.logits[loop.idx[j]].float().cpu().numpy())
    loop.close([len(t) for t in toks])
    lens = [getattr(a, "length", None) for a in loop.arenas]
    return toks, recs, rows, lens, set(m._graphs), type(loop).__name__


def test_slot_loop_with_an_idle_slot_and_an_early_stop(mid):
    lm, eng, prompts = mid
    base = set(lm.hf_model._graphs)
    t_free = _slot_run(lm, eng, prompts, None, mention=False, stop=[])[0]
    # (a condition on the inputs: a token that sequence 0 meets first in the middle of its run and sequence 1 never does)
    cut = next(i for i in range(2, N_NEW - 1) if t_free[0][i] not in t_free[0][:i] and t_free[0][i] not in t_free[1])
    stop = [t_free[0][cut]]
    t0, _, _, len0, keys0, _ = _slot_run(lm, eng, prompts, None, mention=False, stop=stop)
    assert len(t0[0]) == cut + 1 < N_NEW and len(t0[1]) == N_NEW
    t1, _, _, len1, keys1, _ = _slot_run(lm, eng, prompts, None, stop=stop)
    assert (t1, len1, keys1) == (t0, len0, keys0) and not any("logprobs" in k for k in keys0 - base)
    t2, recs, rows, len2, keys2, _ = _slot_run(lm, eng, prompts, 4, stop=stop)
    assert (t2, len2) == (t0, len0) and keys2 > keys0 and all("logprobs" in k for k in keys2 - keys0)
    for j in range(2):
        _check(recs[j], rows[j], t2[j], 4, f"SlotLoop sequence {j}")


@pytest.mark.parametrize("keep", [True, False])
def test_slot_loop_over_int8_images(mid, keep):
    lm, eng, prompts = mid
    kw = dict(kv="int8", stop=[]) if keep else dict(kv="int8", keep_arenas=False, stop=[])
    t0, _, _, len0, keys0, name = _slot_run(lm, eng, prompts, None, mention=False, **dict(kw))
    assert name == ("SlotLoopQ8" if keep else "SlotLoopQ8Only")
    t2, recs, rows, len2, keys2, _ = _slot_run(lm, eng, prompts, 2, **dict(kw))
    assert (t2, len2) == (t0, len0) and all("logprobs" in k for k in keys2 - keys0) and keys2 > keys0
    for j in range(2):
        _check(recs[j], rows[j], t2[j], 2, f"{name} sequence {j}")


def test_lookup_slot_loop(mid):
    """S = 2, k = 3; per sequence a corpus that holds its answer with one token changed."""
    lm, eng, prompts = mid
    m = lm.hf_model
    k, n = 3, 3

    def run(corpora, **kw):
        fr = [_fresh(lm, eng, prompts[j], j) for j in range(2)]
        cs = [[f[1]] + c for f, c in zip(fr, corpora)]
        loop = m.lookup_slot_loop([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], N_NEW, k, cs, slots=2, **kw)
        steps, recs, rows = [[], []], [[], []], [[], []]
        while any(sum(map(len, s)) < N_NEW for s in steps):
            i = loop.enqueue()
            for j in range(2):
                toks = loop.tokens(j, i)
                steps[j].append(toks)
                if kw.get("logprobs") is not None:
                    recs[j] += loop.logprobs(j, i)
                    r0 = loop.idx[j] * (k + 1)
                    rows[j] += list(loop.logits[r0:r0 + len(toks)].float().cpu().numpy())
        loop.close([N_NEW - 1, N_NEW - 4])
        return steps, recs, rows, [a.length for a in loop.arenas], set(m._graphs)

    T = [[t for s in seq for t in s] for seq in run([[], []])[0]]
    corpora = [list(t) for t in T]
    for c in corpora:
        c[6] = (c[6] + 1) % 2048 or 3
    s0, _, _, len0, keys0 = run(corpora)
    assert [[t for s in seq for t in s] for seq in s0] == T and any(len(s) > 1 for seq in s0 for s in seq)
    s1, _, _, len1, keys1 = run(corpora, logprobs=None)
    assert (s1, len1, keys1) == (s0, len0, keys0)
    s2, recs, rows, len2, keys2 = run(corpora, logprobs=n)
    assert (s2, len2) == (s0, len0) and keys2 > keys0 and all("logprobs" in key for key in keys2 - keys0)
    for j in range(2):
        _check(recs[j], rows[j], T[j], n, f"LookupSlotLoop sequence {j}")
    with pytest.raises(ValueError, match="forced row"):
        m.lookup_slot_loop([], [], [], N_NEW, k, [], each=True, prompt_rows=True, logprobs=1)


# ---- the engine -------------------------------------------------------------------------------------------------------------------
def _same_path(a, b, what, tol=PATH_TOL):
    """Two record lists of the same tokens from two paths: tokens equal, log-probabilities of the same ids within ``tol``."""
    assert [r.token for r in a] == [r.token for r in b], what
    worst = 0.0
    for x, y in zip(a, b):
        worst = max(worst, abs(x.logprob - y.logprob))
        ty = dict(y.top)
        worst = max([worst] + [abs(lp - ty[i]) for i, lp in x.top if i in ty])
    print(f"[logprob model] {what}: max |lp - lp'| = {worst:.3e}")
    assert worst <= tol, (what, worst)


def _spy(m, monkeypatch):
    """Record every eager ``token_logprobs`` call of model ``m``: (rows fp32, tokens, n, records)."""
    calls, real = [], m.token_logprobs

    def spy(rows, tokens, n):
        out = real(rows, tokens, n)
        calls.append((rows.reshape(-1, rows.shape[-1]).float().cpu().numpy(), list(tokens), n, out))
        return out
    monkeypatch.setattr(m, "token_logprobs", spy)
    return calls


def test_generate_device_loops_against_host_steps(mid, monkeypatch):
    from promptcache_amd import GenerationEngine, TokenLogprob
    lm, eng, prompts = mid
    calls = _spy(lm.hf_model, monkeypatch)

    def run(ge, params):
        ids, pos, _, cache = eng.process(prompts[0])
        return list(ge.generate(ids, pos, params, cache))

    for name, kw, lookup in (("greedy", dict(temperature=0.0), 0), ("sampled", SAMPLED, 0), ("lookup", dict(temperature=0.0), 3)):
        off = run(GenerationEngine(lm, lookup=lookup), _params(**kw)) if name != "sampled" else None
        torch.manual_seed(3)
        del calls[:]
        outs = run(GenerationEngine(lm, lookup=lookup), _params(logprobs=2, **kw))
        assert len(calls) == 1                                                        # the first token alone came through the eager call
        _check(calls[0][3], calls[0][0], calls[0][1], 2, f"generate {name}: first token")
        lps = outs[-1].logprobs
        assert len(lps) == N_NEW and all(isinstance(r, TokenLogprob) and len(r.top) == 2 for r in lps)
        assert [len(o.logprobs) for o in outs] == sorted(len(o.logprobs) for o in outs) and outs[0].logprobs[0] == lps[0]    # cumulative
        assert lm.decode([r.token for r in lps]) == outs[-1].new_text
        if off is not None:
            assert [o.new_text for o in off] == [o.new_text for o in outs] and all(o.logprobs is None for o in off)
        host = GenerationEngine(lm)
        host.device_greedy_loop = host.device_sample_loop = False
        torch.manual_seed(3)
        del calls[:]
        stepped = run(host, _params(logprobs=2, **kw))
        assert len(calls) == N_NEW
        for rows, toks, n, recs in calls:
            _check(recs, rows, toks, n, f"generate {name}: host step")
        if name != "sampled":                      # (the host's sampler is torch's, another random stream: other tokens)
            _same_path(lps, stepped[-1].logprobs, f"generate {name}: device loop against host steps")
    # a stop id ends the list with the stop token; max_new_tokens=1 gives the first token's record alone
    stop = lps[5].token
    cut = [r.token for r in lps].index(stop)
    from promptcache_amd.generation_engine import GenerationParameters
    outs = run(GenerationEngine(lm, lookup=3), GenerationParameters(temperature=0.0, max_new_tokens=N_NEW, stop_token_ids=[stop], logprobs=0))
    assert [r.token for r in outs[-1].logprobs] == [r.token for r in lps[:cut + 1]] and all(r.top == [] for r in outs[-1].logprobs)
    outs = run(GenerationEngine(lm), GenerationParameters(temperature=0.0, max_new_tokens=1, logprobs=8))
    assert len(outs) == 1 and len(outs[0].logprobs) == 1 and len(outs[0].logprobs[0].top) == 8


def test_generate_covers_falcon(monkeypatch):
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
    calls = _spy(lm.hf_model, monkeypatch)
    ge = GenerationEngine(lm)
    texts = {}
    for n in (None, 3):
        ids, pos, _, cache = eng.process(prompt)
        texts[n] = list(ge.generate(ids, pos, GenerationParameters(temperature=0.0, max_new_tokens=6, logprobs=n), cache))
    assert [o.new_text for o in texts[None]] == [o.new_text for o in texts[3]] and texts[None][-1].logprobs is None
    lps = texts[3][-1].logprobs
    assert len(lps) == 6 and all(len(r.top) == 3 and r.token == r.top[0][0] for r in lps)
    # every record is the float64 truth of the row the model handed over (device loop or host steps: whatever Falcon decodes with)
    eager = [rec for rows, toks, n, recs in calls for rec in recs]
    for rows, toks, n, recs in calls:
        _check(recs, rows, toks, n, "Falcon: eager call")
    assert len(eager) >= 1 and (eager[0][0], eager[0][1]) == (lps[0].token, lps[0].logprob)


def test_generate_batch(mid):
    from promptcache_amd import GenerationEngine
    lm, eng, prompts = mid
    ge = GenerationEngine(lm)

    def batch(params, **kw):
        reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts[:3])]
        return th.collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, **kw))

    for kw in ({}, dict(lookup=3)):
        off, on = batch(_params(temperature=0.0), **kw), batch(_params(temperature=0.0, logprobs=2), **kw)
        for k in range(3):
            assert [o.new_text for o in off[k]] == [o.new_text for o in on[k]] and off[k][-1].logprobs is None
            lps = on[k][-1].logprobs
            assert len(lps) == N_NEW and all(len(r.top) == 2 and (r.token, r.logprob) == r.top[0] for r in lps)
            ids, pos, _, cache = eng.process(prompts[k])
            solo = list(ge.generate(ids, pos, _params(temperature=0.0, logprobs=2), cache))
            _same_path(lps, solo[-1].logprobs, f"generate_batch {kw} sequence {k} against generate")


@pytest.mark.parametrize("mode", [dict(), dict(lookup=3), dict(slot_kv="int8")])
def test_serve(mid, mode):
    """2 slots, 5 requests asking for 0, 3 or no alternatives: a request with None comes back with ``Output.logprobs is None``."""
    from promptcache_amd import CacheEngine, GenerationEngine
    from promptcache_amd.generation_engine import GenerationParameters
    lm, _, prompts = mid
    eng = CacheEngine(2048, lm, slots=2)
    eng.add_schema(_schema_text(lm))
    ge = GenerationEngine(lm)
    asks = [3, None, 0, 3, None]
    budgets = [6, 11, 9, 5, 8]
    ps = [prompts[i % 4] for i in range(5)]

    def reqs(with_lp):
        return [(p, GenerationParameters(temperature=0.0, max_new_tokens=b, logprobs=a if with_lp else None)) for p, b, a in zip(ps, budgets, asks)]

    off = th.collect(ge.serve(eng, iter(reqs(False)), **mode))
    toks_off = {k: list(v) for k, v in ge.last_serve_tokens.items()}
    keys_off = set(lm.hf_model._graphs)
    on = th.collect(ge.serve(eng, iter(reqs(True)), logprobs=3, **mode))
    assert {k: list(v) for k, v in ge.last_serve_tokens.items()} == toks_off                   # the same tokens, bit for bit
    assert all(k[-2:] == ("logprobs", 3) for k in set(lm.hf_model._graphs) - keys_off)
    for r, ask in enumerate(asks):
        assert [o.new_text for o in on[r]] == [o.new_text for o in off[r]] and all(o.logprobs is None for o in off[r])
        lps = on[r][-1].logprobs
        if ask is None:
            assert all(o.logprobs is None for o in on[r])
            continue
        assert [x.token for x in lps] == toks_off[r] and all(len(x.top) == ask for x in lps)
        assert all(x.logprob <= 0.0 and math.isfinite(x.logprob) for x in lps)
        if ask:
            assert all((x.token, x.logprob) == x.top[0] and x.top[0][1] >= x.top[1][1] >= x.top[2][1] for x in lps)
        if "slot_kv" not in mode:                  # (int8 images: the format's logits, not generate's)
            ids, pos, _, cache = eng.process(ps[r])
            solo = list(ge.generate(ids, pos, GenerationParameters(temperature=0.0, max_new_tokens=budgets[r], logprobs=ask), cache))
            _same_path(lps, solo[-1].logprobs, f"serve {mode} request {r} against generate")


def _schema_text(lm):
    from promptcache_amd import synth
    sp, _ = synth.persona_like("deep", system_len=60, intro_len=20, traits=th.TRAITS, question_len=8, seed=6, pick=(0, 1))
    return lm.get_formatter()(sp)


def test_serve_admission_errors_and_the_loop_prefill_refusal(mid):
    from promptcache_amd import CacheEngine, GenerationEngine
    from promptcache_amd.generation_engine import GenerationParameters
    lm, _, prompts = mid
    eng = CacheEngine(2048, lm, slots=2)
    eng.add_schema(_schema_text(lm))
    ge = GenerationEngine(lm)
    ask = lambda n: [(prompts[0], GenerationParameters(temperature=0.0, max_new_tokens=4, logprobs=n))]
    with pytest.raises(ValueError, match=r"serve\(logprobs=n\) with n >= 5"):
        list(ge.serve(eng, iter(ask(5)), logprobs=3))
    with pytest.raises(ValueError, match=r"carries no log-probability node: call serve\(logprobs=n\)"):
        list(ge.serve(eng, iter(ask(0))))
    with pytest.raises(ValueError, match="forced row"):
        list(ge.serve(eng, iter(ask(1)), lookup=3, loop_prefill=True, logprobs=1))
    with pytest.raises(ValueError, match="0..8"):
        list(ge.serve(eng, iter(ask(None)), logprobs=9))
    assert lm.hf_model._live_loop is None
    out = th.collect(ge.serve(eng, iter(ask(1)), logprobs=1))          # ... and the engine serves afterwards
    assert len(out[0][-1].logprobs) == 4
