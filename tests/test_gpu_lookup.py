"""Prompt-lookup speculative decoding on the GPU: the two kernels of csrc/pc_lookup.hip against the numpy restatement
(tests/lookup_ref.py), word for word, and ``LookupLoop`` / ``GenerationEngine(lookup=k)`` against the stepped mode, the host
model of the loop, ``GreedyLoop`` and the numpy oracle."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import lookup_ref as lr

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-2          # the project's parity bar
DEV = "cuda:0"


# ---- pc_lookup_draft ---------------------------------------------------------------------------------------------------------
def _check_draft(h, L, k, nmax=3):
    from promptcache_amd import _native
    h = np.asarray(h, dtype=np.int32)
    hist = torch.from_numpy(h.copy()).to(DEV)
    ids0 = np.full(20, -7, dtype=np.int64)
    pos0 = np.full(20, -9, dtype=np.int32)
    ids0[0], pos0[0] = (h[L - 1] if L >= 1 else 3), 1000
    ids, pos = torch.from_numpy(ids0.copy()).to(DEV), torch.from_numpy(pos0.copy()).to(DEV)
    nd = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    hl = torch.tensor([L], dtype=torch.int32, device=DEV)
    _native.lookup_draft(hist, hl, ids, pos, nd, k, nmax)
    want_ids, want_pos, want_m = lr.draft_state(h, L, ids0, pos0, k, nmax)
    assert int(nd[0]) == want_m, (L, k, int(nd[0]), want_m)
    assert np.array_equal(ids.cpu().numpy(), want_ids), (L, k)          # (all 20 words: those beyond k + 1 are untouched)
    assert np.array_equal(pos.cpu().numpy(), want_pos), (L, k)
    assert np.array_equal(hist.cpu().numpy(), h) and int(hl[0]) == L
    return want_m


@pytest.mark.parametrize("k", [1, 7, 15])
def test_draft_equals_the_reference(k):
    rng = np.random.default_rng(40 + k)
    some = 0
    for L in (1, 2, 5, 300, 4097):
        dense = rng.integers(0, 5, size=L + 40)                        # 5 symbols: matches everywhere
        some += _check_draft(dense, L, k)
        _check_draft(dense, L, k, nmax=1)
        _check_draft(dense, L, k, nmax=8)
        sparse = rng.permutation(32000)[:L + 40]                       # all different: no match at any n
        assert _check_draft(sparse, L, k) == 0
    assert some > 0
    # the winning (largest) j in the last workgroup-stride of a 4097-token history, an earlier copy of the suffix far in front
    L = 4097
    h = rng.permutation(32000)[:L + 8]
    h[L - 3:L] = (31001, 31002, 31003)
    h[10:13] = (31001, 31002, 31003)
    h[L - 9:L - 6] = (31001, 31002, 31003)                             # followers h[L-6 .. L): six of them
    assert _check_draft(h, L, k) == min(k, 6)
    h[L - 9] = 5                                                       # ... now only "31002 31003" there: the n = 3 match in front wins
    assert _check_draft(h, L, k) == k


# ---- pc_lookup_verify --------------------------------------------------------------------------------------------------------
RING_CAP = 4


def _verify_case(V, rows, am, ids, nd, budget, ctr, tie=None, misalign=1):
    """One launch against lr.verify: logits whose row i has its maximum at am[i] (``tie``: (row, lower index) of a second,
    equal maximum)."""
    from promptcache_amd import _native
    k = rows - 1
    rng = np.random.default_rng(V + 31 * rows + 7 * budget + nd)
    x = rng.standard_normal((rows, V)).astype(np.float32)
    want_am = list(am)
    for i, a in enumerate(am):
        x[i, a] = 10.0
    if tie is not None:
        x[tie[0], tie[1]] = 10.0
        want_am[tie[0]] = min(tie[1], am[tie[0]])
    assert lr.argmax_rows(x) == want_am
    flat = torch.zeros(rows * V + 4, dtype=torch.float32, device=DEV)
    flat[misalign:misalign + rows * V] = torch.from_numpy(x.reshape(-1)).to(DEV)      # base 4-byte aligned only
    logits = flat[misalign:misalign + rows * V].view(rows, V)
    L = 5
    st = dict(hist=np.array([9, 8, 7, 6, int(ids[0])] + [-3] * 27, dtype=np.int32), hist_len=np.array([L], dtype=np.int32),
              ids=np.array(list(ids) + [-7] * (20 - len(ids)), dtype=np.int64),
              pos=np.array([100 + i for i in range(rows)] + [-9] * (20 - rows), dtype=np.int32),
              past=np.array([60, 17], dtype=np.int32), ndraft=np.array([nd], dtype=np.int32),
              budget=np.array([budget], dtype=np.int32), ring=np.full((RING_CAP, rows + 1), -5, dtype=np.int32),
              ctr=np.array([ctr], dtype=np.int32))
    dev = {n: torch.from_numpy(v.copy()).to(DEV) for n, v in st.items()}
    amax = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    _native.lookup_verify(logits, V, V, rows, amax, dev["hist"], dev["hist_len"], dev["ids"], dev["pos"], dev["past"], dev["ndraft"],
                          dev["budget"], dev["ring"], dev["ctr"], RING_CAP)
    want = lr.verify(x, st, RING_CAP)
    assert amax[:rows].tolist() == want_am
    for name in st:
        assert np.array_equal(dev[name].cpu().numpy(), want[name]), (name, V, rows, nd, budget, dev[name].cpu().numpy(), want[name])
    return int(want["ring"][ctr % RING_CAP][0])


@pytest.mark.parametrize("V", [32000, 32003])
@pytest.mark.parametrize("rows", [1, 2, 8, 16])
def test_verify_equals_the_reference(V, rows):
    k = rows - 1
    fed = 77
    drafts = [1000 + 3 * i for i in range(k)]
    bonus = [V - 1 - i for i in range(rows)]                                  # what the model says where it disagrees (last columns)

    def am_for(acc, nd):
        """argmax per row: agrees with the first ``acc`` drafts, then its own tokens."""
        return [drafts[i] if i < acc else bonus[i] for i in range(rows)]

    if k == 0:
        for budget in (0, 1, 5):
            assert _verify_case(V, 1, [V - 2], [fed], 0, budget, 2) == min(1, budget)
        _verify_case(V, 1, [500], [fed], 0, 3, RING_CAP - 1, tie=(0, 17))    # tie: the lowest index; counter at the ring's end
        return
    nd = k
    for acc in sorted({0, min(1, nd), nd}):
        for budget in sorted({0, 1, max(acc, 1), acc + 5}):
            got = _verify_case(V, rows, am_for(acc, nd), [fed] + drafts, nd, budget, 1)
            assert got == min(acc + 1, budget)
    # ndraft < k: the pad rows repeat the fed token, and the model "agrees" with a pad (its argmax there IS the fed token):
    # a pad must never be accepted
    nd = k // 2
    am = [drafts[i] if i < nd else fed for i in range(rows)]
    ids = [fed] + drafts[:nd] + [fed] * (k - nd)
    assert _verify_case(V, rows, am, ids, nd, 40, 0) == nd + 1
    # a tie of two maxima in one row: the lowest index wins -- and decides acceptance (draft 0 is the lower index)
    am = am_for(k, k)
    assert _verify_case(V, rows, [V - 5] + am[1:], [fed] + drafts, k, 40, 0, tie=(0, drafts[0])) == k + 1
    # the ring wraps: counter = ring_cap - 1 writes the last record, the next one the first
    _verify_case(V, rows, am_for(1, k), [fed] + drafts, k, 9, RING_CAP - 1)
    _verify_case(V, rows, am_for(1, k), [fed] + drafts, k, 9, RING_CAP, misalign=3)


@pytest.mark.parametrize("V", [32000, 32016])
def test_one_row_verify_is_greedy_advance(V):
    from promptcache_amd import _native
    x = torch.randn(V, device=DEV)
    x[V - 3] = 9.0
    x[41] = 9.0                                                              # a tie: both kernels take index 41
    a = dict(ids=torch.tensor([5], dtype=torch.int64, device=DEV), pos=torch.tensor([70], dtype=torch.int32, device=DEV),
             past=torch.tensor([33, 4], dtype=torch.int32, device=DEV), ring=torch.zeros(8, dtype=torch.int32, device=DEV),
             ctr=torch.tensor([2], dtype=torch.int32, device=DEV))
    b = {n: v.clone() for n, v in a.items()}
    b["ring"] = torch.zeros(8 * 2, dtype=torch.int32, device=DEV)
    _native.greedy_advance(x, V, a["ids"], a["pos"], a["past"], a["ring"], a["ctr"])
    hist = torch.zeros(8, dtype=torch.int32, device=DEV)
    hl = torch.tensor([1], dtype=torch.int32, device=DEV)
    _native.lookup_verify(x.view(1, V), V, V, 1, torch.zeros(16, dtype=torch.int32, device=DEV), hist, hl, b["ids"], b["pos"], b["past"],
                          torch.zeros(1, dtype=torch.int32, device=DEV), torch.tensor([3], dtype=torch.int32, device=DEV), b["ring"],
                          b["ctr"], 8)
    assert int(a["ids"][0]) == 41
    for n in ("ids", "pos", "past", "ctr"):
        assert torch.equal(a[n], b[n]), n
    assert b["ring"].view(8, 2)[2].tolist() == [1, int(a["ring"][2])]


# ---- LookupLoop --------------------------------------------------------------------------------------------------------------
SHAPE, W_SEED, W_SCALE, CTX_LEN, N_NEW = "mid_gqa", 108, 3.0, 40, 24


@pytest.fixture(scope="module")
def model():
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    shape = SHAPES[SHAPE]
    w16 = make_weights_np(shape, W_SEED, W_SCALE)
    lm = Llama2(name="lk", shape=shape, weights=w16, device=DEV)
    ctx = np.random.default_rng(W_SEED).integers(3, shape.vocab_size, size=CTX_LEN).tolist()
    return lm, shape, w16, ctx


def _prefill(lm, ctx):
    out = lm(input_ids=torch.tensor([ctx]), position_ids=torch.tensor([list(range(len(ctx)))]), use_cache=True)
    return out.past_key_values, int(out.logits[0, -1].argmax())


def _run(lm, ctx, corpus, k, max_new, device_loop, extra=0, keep_logits=False):
    """One lookup generation of ``max_new`` tokens behind a fresh prefill of ``ctx`` -> (first token, per-step token lists, loop,
    per-step logits)."""
    past, first = _prefill(lm, ctx)
    loop = lm.hf_model.lookup_loop(past, first, len(ctx), max_new, k, corpus)
    loop.device_loop = device_loop
    steps, logits, got = [], [], 0
    while got < max_new:
        i = loop.enqueue()
        t = loop.tokens(i)
        assert 1 <= len(t) <= k + 1
        if keep_logits:
            logits.append(loop.logits[0, :len(t)].float().cpu().numpy())
        steps.append(t)
        got += len(t)
    for _ in range(extra):
        steps.append(loop.tokens(loop.enqueue()))
    return first, steps, loop, logits


@pytest.fixture(scope="module")
def reference_run(model):
    """T: the greedy continuation (N_NEW tokens behind the first), from the stepped mode with nothing to copy from but itself."""
    lm, shape, w16, ctx = model
    first, steps, loop, logits = _run(lm, ctx, [], 3, N_NEW, False, keep_logits=True)
    loop.close(N_NEW)
    T = [t for s in steps for t in s]
    assert len(T) == N_NEW
    return first, T, steps, logits


@pytest.mark.parametrize("k", [3, 7])
def test_device_loop_equals_the_stepped_mode(model, k):
    from promptcache_amd.model.llama_hip import LookupLoop
    lm, shape, w16, ctx = model
    kv = {}
    for dev_loop in (True, False):
        first, steps, loop, _ = _run(lm, ctx, ctx, k, N_NEW, dev_loop)
        assert isinstance(loop, LookupLoop) and loop.len0 == CTX_LEN
        loop.close(N_NEW)
        a = loop.arena
        assert a.length == CTX_LEN + N_NEW
        kv[dev_loop] = (first, steps, a.buf[:, :, :, :, CTX_LEN:CTX_LEN + N_NEW].clone())
    assert kv[True][0] == kv[False][0] and kv[True][1] == kv[False][1]        # tokens and per-step counts
    assert torch.equal(kv[True][2], kv[False][2])                              # K / V rows of every layer, bit for bit
    assert lm.hf_model._live_loop is None


def test_acceptance_follows_the_host_model(model, reference_run):
    lm, shape, w16, ctx = model
    first, T, steps0, _ = reference_run
    k = 7
    full = ctx[-8:] + [first] + T                   # the context tail, then the answer itself: every draft is right
    wrong = list(full)
    wrong[8 + 1 + 6] = (wrong[8 + 1 + 6] + 1) % shape.vocab_size or 3
    wrong[8 + 1 + 15] = (wrong[8 + 1 + 15] + 1) % shape.vocab_size or 3
    # (a condition on the inputs, not on the code: the full corpus must actually save steps)
    assert len(lr.simulate(full, first, T, k)) < len(T)
    assert [len(s) for s in steps0] == lr.simulate([], first, T, 3)
    for corpus in ([], full, wrong):
        f, steps, loop, _ = _run(lm, ctx, corpus, k, N_NEW, True)
        loop.close(N_NEW)
        assert f == first and [t for s in steps for t in s] == T
        assert [len(s) for s in steps] == lr.simulate(corpus, first, T, k), corpus is full


def test_budget_and_memory_safety(model, reference_run):
    from promptcache_amd.model.llama_hip import GreedyLoop
    lm, shape, w16, ctx = model
    m = lm.hf_model
    first, T, _, _ = reference_run
    k, max_new = 3, 10
    past, f = _prefill(lm, ctx)
    assert f == first
    loop = m.lookup_loop(past, first, len(ctx), max_new, k, ctx[-8:] + [first] + T)
    a = loop.arena
    lo = CTX_LEN + max_new + k + 1
    assert a.cap >= lo + 1
    with torch.inference_mode():
        a.buf[:, :, :, :, lo:] = 0.5
    before = a.buf[:, :, :, :, lo:].clone()
    need = len(lr.simulate(ctx[-8:] + [first] + T, first, T[:max_new], k))
    steps = [loop.tokens(loop.enqueue()) for _ in range(need + 6)]
    assert sum(map(len, steps)) == max_new and [t for s in steps for t in s] == T[:max_new]
    assert all(len(s) > 0 for s in steps[:need]) and all(len(s) == 0 for s in steps[need:])
    torch.cuda.synchronize()
    assert torch.equal(a.buf[:, :, :, :, lo:], before)                         # nothing behind the rows the budget allows
    consumed = 7
    loop.close(consumed)
    assert a.length == CTX_LEN + consumed and m._live_loop is None
    nxt, p = T[consumed - 1], CTX_LEN + consumed
    got = lm(input_ids=torch.tensor([[nxt]]), position_ids=torch.tensor([[p]]), past_key_values=a.views(), use_cache=True).logits[0, -1]
    # the same state after a GreedyLoop of the same tokens
    past, f = _prefill(lm, ctx)
    g = m.greedy_loop(past, first, len(ctx), max_new)
    assert type(g) is GreedyLoop
    toks = [g.token(g.enqueue()) for _ in range(consumed)]
    assert toks == T[:consumed]
    g.close(consumed)
    ref = lm(input_ids=torch.tensor([[nxt]]), position_ids=torch.tensor([[p]]), past_key_values=g.arena.views(), use_cache=True).logits[0, -1]
    d = float((got - ref).abs().max())
    print(f"logits behind a lookup loop vs behind a greedy loop: max |d| = {d:.2e}")
    assert d < LOGIT_TOL


def test_lookup_logits_and_tokens_against_the_oracle(model, reference_run):
    """Teacher-forced through the numpy oracle: every emitted position's logits within the parity bar, every token the oracle's
    argmax.  The weight seed was chosen (on the CPU, beforehand) so that the oracle's own top-2 margin exceeds 2e-2 -- twice the
    bar: each of two logits may move by 1e-2 -- at EVERY position; the test re-checks that on its inputs."""
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    lm, shape, w16, ctx = model
    first, T, steps, logits = reference_run
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=lm.hf_model.inv_freq_cpu.numpy())
    oracle = LlamaOracle(cfg, {n: v.astype(np.float32) for n, v in w16.items()})
    dev_rows = np.concatenate(logits, axis=0)
    assert dev_rows.shape[0] == N_NEW
    with H.oracle_blas():
        olog, present = oracle.forward(np.array([ctx]), np.arange(len(ctx))[None])
        assert int(np.argmax(olog[0, -1])) == first
        top = np.sort(olog[0, -1])[-2:]
        margin, worst, fed = float(top[1] - top[0]), 0.0, first
        for i in range(N_NEW):
            olog, present = oracle.forward(np.array([[fed]]), np.array([[len(ctx) + i]]), past=present)
            row = olog[0, -1]
            top = np.sort(row)[-2:]
            margin = min(margin, float(top[1] - top[0]))
            worst = max(worst, float(np.abs(dev_rows[i] - row).max()))
            assert int(np.argmax(row)) == T[i], i
            fed = T[i]
    print(f"lookup steps vs oracle: max |dlogit| = {worst:.2e}; oracle top-2 margin >= {margin:.3f}")
    assert margin > 2e-2
    assert worst < LOGIT_TOL


# ---- GenerationEngine(lookup=k) ----------------------------------------------------------------------------------------------
def test_engine_takes_the_lookup_loop_for_plain_greedy_only():
    from promptcache_amd import GenerationEngine, GenerationParameters, Prompt
    from promptcache_amd.model.llama_hip import GreedyLoop, LookupLoop, SampleLoop
    from tests.test_gpu_engine import build_product
    g = H.load_case("mid_trip")              # (the golden `trip` schema on a shape whose decode runs the device loops)
    lm, eng = build_product(g)
    assert lm.hf_model.lookup_available()
    prompt = Prompt(str(g["prompt_text"]), [lm.get_formatter()])
    want = lm.decode(g["greedy"].tolist())

    def run(lookup, params):
        ids, pos, _, cache = eng.process(prompt)
        kinds, outs = set(), []
        for o in GenerationEngine(lm, lookup=lookup).generate(ids, pos, params, cache, stream_interval=1):
            outs.append(o)
            if lm.hf_model._live_loop is not None:
                kinds.add(type(lm.hf_model._live_loop))
        assert lm.hf_model._live_loop is None
        return outs, kinds

    greedy = GenerationParameters(temperature=0.0, max_new_tokens=len(g["greedy"]), stop_token_ids=[], stop_str=[])
    outs, kinds = run(7, greedy)
    assert outs[-1].new_text == want and kinds == {LookupLoop}
    assert len(outs) == len(g["greedy"])                                       # one Output per token, as without lookup
    outs, kinds = run(0, greedy)
    assert outs[-1].new_text == want and kinds == {GreedyLoop}
    # a stop id in the middle of the answer: the tokens of the step behind it are dropped, the arena ends at the consumed row
    stop = int(g["greedy"][2])
    cut = g["greedy"].tolist().index(stop)
    assert 0 < cut < len(g["greedy"]) - 1
    outs, kinds = run(7, GenerationParameters(temperature=0.0, max_new_tokens=len(g["greedy"]), stop_token_ids=[stop], stop_str=[]))
    assert outs[-1].new_text == lm.decode(g["greedy"].tolist()[:cut + 1])
    sampled = GenerationParameters(temperature=0.8, top_p=0.9, max_new_tokens=6, stop_token_ids=[], stop_str=[])
    _, kinds = run(7, sampled)
    assert kinds == {SampleLoop}
