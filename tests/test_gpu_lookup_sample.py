"""Sampled prompt-lookup speculative decoding on the GPU: ``pc_lookup_verify_sample`` (csrc/pc_sample.hip) against its numpy
restatement (tests/lookup_sample_ref.py) word for word and against its two degenerate forms (``pc_sample_advance``,
``pc_lookup_verify``) bit for bit; ``SampleLookupLoop`` against the stepped mode, the host model of the step, ``SampleLoop`` and the
numpy oracle; ``GenerationEngine(lookup=k, lookup_sampled=True)``."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import lookup_sample_ref as lsr
from tests import sample_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_TOL = 1e-2          # the project's parity bar
MARGIN = 1e-4             # test_gpu_sample.py's bar for the fp32 (device) vs float64 (reference) Gumbel race
RING_CAP = 4
PARAM_SETS = ((1.0, 1.0, 0.95, 0), (0.8, 1.1, 0.9, 50), (0.0, 1.2, 1.0, 0))
LDL_PAD, MISALIGN = 5, 1  # row stride V + 5, base one float behind a 256-byte boundary: 4- but not 16-byte aligned


# ---- pc_lookup_verify_sample against the reference -----------------------------------------------------------------------------
def _params_dev(params, seed):
    from promptcache_amd import _native
    T, rp, tp, tk = params
    return torch.frombuffer(bytearray(_native.sample_params_bytes(T, rp, tp, tk if tk > 0 else -1, seed)), dtype=torch.uint8).to(DEV)


def _device_rows(x, ldl):
    rows, V = x.shape
    flat = torch.full((rows * ldl + 8,), 7.0, dtype=torch.float32, device=DEV)
    view = flat[MISALIGN:MISALIGN + rows * ldl].view(rows, ldl)
    view[:, :V] = torch.from_numpy(x).to(DEV)
    assert view.data_ptr() % 16 == 4
    return view


def _state(V, rows, fed, drafts, nd, budget, ctr, base_hist, draws, hist_room=27):
    L = 5
    return dict(hist=np.array([9, 8, 7, 6, int(fed)] + [-3] * hist_room, dtype=np.int32), hist_len=np.array([L], dtype=np.int32),
                ids=np.array([fed] + list(drafts) + [-7] * (20 - rows), dtype=np.int64),
                pos=np.array([100 + i for i in range(rows)] + [-9] * (20 - rows), dtype=np.int32),
                past=np.array([60, 17], dtype=np.int32), ndraft=np.array([nd], dtype=np.int32),
                budget=np.array([budget], dtype=np.int32), ring=np.full((RING_CAP, rows + 1), -5, dtype=np.int32),
                ctr=np.array([ctr], dtype=np.int32), bits=lsr.history_bits(list(base_hist) + [fed], V),
                draws=np.array([draws], dtype=np.int32))


def _launch(x, st, params, seed, want_processed=True):
    """One pc_lookup_verify_sample on device copies of ``st`` -> (state after, row tokens, processed rows)."""
    from promptcache_amd import _native
    rows, V = x.shape
    hw = (V + 31) // 32
    dev = {n: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v.copy()).to(DEV) for n, v in st.items()}
    row_bits = torch.full((rows * hw,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)      # scratch arrives dirty
    row_token = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    proc = torch.full((rows, V), float("nan"), dtype=torch.float32, device=DEV) if want_processed else None
    _native.lookup_verify_sample(_device_rows(x, V + LDL_PAD), V + LDL_PAD, V, rows, _params_dev(params, seed), dev["bits"], row_bits,
                                 dev["draws"], row_token, dev["hist"], dev["hist_len"], dev["ids"], dev["pos"], dev["past"],
                                 dev["ndraft"], dev["budget"], dev["ring"], dev["ctr"], RING_CAP, proc)
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy() for n, t in dev.items()}
    got["bits"] = got["bits"].view(np.uint32)
    return got, row_token.cpu().numpy(), None if proc is None else proc.cpu().numpy()


class _Tally:
    def __init__(self):
        self.cases = self.skipped = 0
        self.min_margin = np.inf


def _check(x, st, params, seed, tally, tag, processed=False):
    """Launch + reference on the same words; every word compared where every deciding draw (rows 0 .. acc) is above MARGIN.
    -> the reference's info, or None for a skipped case."""
    want, info = lsr.verify_sample(x, st, RING_CAP, params, seed)
    got, row_token, proc = _launch(x, st, params, seed, processed)
    rows, V = x.shape
    nd = min(max(int(st["ndraft"][0]), 0), rows - 1)
    deciding = info["margins"][:min(info["acc"], nd) + 1]
    tally.cases += 1
    tally.min_margin = min(tally.min_margin, min(deciding))
    if min(deciding) <= MARGIN:
        tally.skipped += 1
        return None
    for name in want:
        assert np.array_equal(got[name], want[name]), (tag, name, got[name][:24], want[name][:24])
    for i in range(nd + 1):
        if info["margins"][i] > MARGIN:
            assert int(row_token[i]) == info["tokens"][i], (tag, "row token", i)
    if processed:
        T, rp, tp, tk = params
        from tests.test_gpu_sample import _check_kept
        base = lsr.bits_ids(st["bits"], V)
        for i in range(nd + 1):
            history = base + [int(t) for t in st["ids"][1:1 + i]]
            ref = info["processed"][i]
            # kept values bit-equal, kept set equal -- with top-p on: up to the reference's own fp32 softmax error at the cut
            # (test_gpu_sample._check_kept, the bar pc_sample_advance's processed row is held to)
            _check_kept((tag, "processed row", i), x[i], history, T, rp, tp, tk, ref != -np.inf, proc[i])
    return info


def _true_draws(x, base_hist, fed, params, seed, d0):
    """The sequential draws of the rows: t[i] at step d0 + i under base_hist + fed + t[0..i)."""
    T, rp, tp, tk = params
    hist, out = list(base_hist) + [fed], []
    for i in range(x.shape[0]):
        tok, _, _ = sr.draw(x[i], hist, T, rp, tp, tk, seed, d0 + i)
        out.append(tok)
        hist.append(tok)
    return out


def _drafts_for(true, acc, k, V):
    """Drafts that agree with the first ``acc`` sequential draws and differ at draft ``acc`` (the later ones stay right)."""
    d = list(true[:k])
    if acc < k:
        d[acc] = (d[acc] + 1) % V
    return d


@pytest.mark.parametrize("V", [1000, 4099, 32000])
@pytest.mark.parametrize("rows", [1, 2, 8, 16])
def test_verify_sample_equals_the_reference(V, rows):
    k = rows - 1
    rng = np.random.default_rng(1000 * rows + V)
    tally = _Tally()
    fed, d0 = 77, 7
    for pi, params in enumerate(PARAM_SETS):
        seed = 40 + 3 * pi + rows
        x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
        base = rng.integers(0, V, 40).tolist()
        # (rows 1.. are drawn under the drafts in front of them: with wrong drafts behind ``acc`` the later "true" tokens are
        # not what the rows draw, but nothing behind the first miss decides anything)
        true = _true_draws(x, base, fed, params, seed, d0)
        if k == 0:
            for budget in (0, 1, 5):
                info = _check(x, _state(V, 1, fed, [], 0, budget, 2, base, d0), params, seed, tally, (V, rows, pi, budget), processed=budget == 5)
                assert info is None or info["emit"] == min(1, budget)
            continue
        for acc in sorted({0, k // 2, k}):
            for budget in sorted({0, 1, max(acc, 1), acc + 5}):
                st = _state(V, rows, fed, _drafts_for(true, acc, k, V), k, budget, 1, base, d0)
                info = _check(x, st, params, seed, tally, (V, rows, pi, acc, budget), processed=(acc == k and budget == acc + 5))
                if info is not None:
                    assert info["acc"] == acc and info["emit"] == min(acc + 1, budget), (V, rows, pi, acc, budget, info["acc"])
        # ndraft = 0 on a k + 1-row step: one token, whatever rows 1..k hold
        info = _check(x, _state(V, rows, fed, true[:k], 0, 9, 0, base, d0), params, seed, tally, (V, rows, pi, "nd0"))
        assert info is None or info["emit"] == 1
        # ndraft < k, the pad rows holding the very tokens that would be drawn there: a pad is never accepted
        nd = k // 2
        info = _check(x, _state(V, rows, fed, true[:k], nd, 40, 0, base, d0), params, seed, tally, (V, rows, pi, "pads"), processed=True)
        assert info is None or (info["acc"] == nd and info["emit"] == nd + 1)
        # the ring wraps (ring_cap = 4, counter = 6 -> record 2; counter = 3 -> the last record)
        _check(x, _state(V, rows, fed, _drafts_for(true, 1, k, V), k, 9, 6, base, d0), params, seed, tally, (V, rows, pi, "wrap6"))
        _check(x, _state(V, rows, fed, _drafts_for(true, 1, k, V), k, 9, RING_CAP - 1, base, d0), params, seed, tally, (V, rows, pi, "wrap3"))
        # the history one word short of what emit needs: emit is clamped to the room
        st = _state(V, rows, fed, true[:k], k, 40, 0, base, d0, hist_room=k)
        info = _check(x, st, params, seed, tally, (V, rows, pi, "clamp"))
        assert info is None or (info["acc"] == k and info["emit"] == k)
        # a draft token whose bit is already set: row 0 made to draw a token of the history (its logit far above the rest)
        y = x.copy()
        y[0, base[3]] = 60.0
        t2 = _true_draws(y, base, fed, params, seed, d0)
        assert t2[0] == base[3]
        info = _check(y, _state(V, rows, fed, t2[:k], k, 40, 0, base, d0), params, seed, tally, (V, rows, pi, "bit set"))
        assert info is None or info["acc"] == k
    # a draft whose penalty changes the next row's draw (greedy, rp = 2): made so on the host and asserted there
    params, seed = (0.0, 2.0, 1.0, 0), 5
    x = (rng.standard_normal((rows, V)) * 0.3).astype(np.float32)                # (every other logit below 2)
    assert x.max() < 2.0
    a, b = 11, V - 2
    base = [t for t in rng.integers(0, V, 40).tolist() if t not in (a, b, fed)]
    x[0, a] = 9.0
    if k >= 1:
        x[1, a], x[1, b] = 4.0, 3.0
        assert sr.draw(x[1], base + [fed], *params, seed, d0 + 1)[0] == a and sr.draw(x[1], base + [fed, a], *params, seed, d0 + 1)[0] == b
        true = _true_draws(x, base, fed, params, seed, d0)
        assert true[:2] == [a, b]
        info = _check(x, _state(V, rows, fed, true[:k], k, 40, 0, base, d0), params, seed, tally, (V, rows, "penalty"))
        assert info is not None and info["tokens"][:2] == [a, b] and info["acc"] == k
    print(f"[verify_sample] V={V} rows={rows}: {tally.cases} cases, {tally.skipped} skipped, smallest deciding margin {tally.min_margin:.3g}")
    assert tally.cases > 0 and tally.skipped * 100 <= tally.cases, (tally.cases, tally.skipped)


# ---- degenerate forms, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 4099, 32000])
def test_one_row_is_sample_advance(V):
    """rows = 1, ndraft = 0: token, ids, pos, past_len, bitmap and processed row are pc_sample_advance's at counter = draws."""
    from promptcache_amd import _native
    from promptcache_amd.model.llama_hip import _history_bits
    rng = np.random.default_rng(V)
    for pi, params in enumerate(PARAM_SETS):
        seed, d0 = 900 + pi, 13 + pi
        x = (rng.standard_normal((1, V)) * 3).astype(np.float32)
        base = rng.integers(0, V, 40).tolist()
        row = _device_rows(x, V + LDL_PAD)
        pd = _params_dev(params, seed)
        a = dict(ids=torch.tensor([5], dtype=torch.int64, device=DEV), pos=torch.tensor([70], dtype=torch.int32, device=DEV),
                 past=torch.tensor([33, 4], dtype=torch.int32, device=DEV), bits=_history_bits(base, V).to(DEV))
        b = {n: v.clone() for n, v in a.items()}
        ring_a, ctr_a = torch.zeros(64, dtype=torch.int32, device=DEV), torch.tensor([d0], dtype=torch.int32, device=DEV)
        proc_a, proc_b = (torch.full((V,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
        _native.sample_advance(row[0, :V], V, pd, a["bits"], a["ids"], a["pos"], a["past"], ring_a, ctr_a, proc_a)
        hw = (V + 31) // 32
        ring_b = torch.zeros(RING_CAP * 2, dtype=torch.int32, device=DEV)
        draws = torch.tensor([d0], dtype=torch.int32, device=DEV)
        _native.lookup_verify_sample(row, V + LDL_PAD, V, 1, pd, b["bits"], torch.zeros(hw, dtype=torch.int32, device=DEV), draws,
                                     torch.zeros(16, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV),
                                     torch.tensor([1], dtype=torch.int32, device=DEV), b["ids"], b["pos"], b["past"],
                                     torch.zeros(1, dtype=torch.int32, device=DEV), torch.tensor([3], dtype=torch.int32, device=DEV),
                                     ring_b, torch.zeros(1, dtype=torch.int32, device=DEV), RING_CAP, proc_b.view(1, V))
        torch.cuda.synchronize()
        for n in a:
            assert torch.equal(a[n], b[n]), (V, pi, n)
        assert ring_b[:2].tolist() == [1, int(a["ids"][0])] and int(draws[0]) == d0 + 1 == int(ctr_a[0])
        assert torch.equal(proc_a.view(torch.int32), proc_b.view(torch.int32)), (V, pi)


@pytest.mark.parametrize("rows", [1, 8])
def test_greedy_block_is_lookup_verify(rows):
    """A greedy parameter block with rp = 1: every word pc_lookup_verify writes is equal."""
    from promptcache_amd import _native
    V, k = 32000, rows - 1
    rng = np.random.default_rng(rows)
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    am = x.argmax(axis=1).tolist()
    for acc, budget in ((0, 9), (k // 2, 9), (k, 9), (k, max(k - 1, 0)), (k, 0)):
        drafts = _drafts_for(am, acc, k, V)
        st = _state(V, rows, 77, drafts, k, budget, 2, [1, 2, 3], 4)
        got, _, _ = _launch(x, st, (0.0, 1.0, 1.0, 0), 0, want_processed=False)
        dev = {n: torch.from_numpy(st[n].copy()).to(DEV) for n in ("hist", "hist_len", "ids", "pos", "past", "ndraft", "budget", "ring", "ctr")}
        amax = torch.zeros(16, dtype=torch.int32, device=DEV)
        _native.lookup_verify(_device_rows(x, V + LDL_PAD), V + LDL_PAD, V, rows, amax, dev["hist"], dev["hist_len"], dev["ids"], dev["pos"],
                              dev["past"], dev["ndraft"], dev["budget"], dev["ring"], dev["ctr"], RING_CAP)
        torch.cuda.synchronize()
        for n, t in dev.items():
            assert np.array_equal(got[n], t.cpu().numpy()), (rows, acc, budget, n)
        assert int(got["ring"][2 % RING_CAP][0]) == min(acc + 1, budget)


def test_argument_checks():
    from promptcache_amd import _native
    V = 64
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=DEV)
    x = torch.zeros(17 * V, dtype=torch.float32, device=DEV)
    args = lambda rows, vocab=V: (x, vocab, vocab, rows, _params_dev((1.0, 1.0, 1.0, 0), 0), z(2), z(64), z(1), z(32), z(8), z(1),
                                  z(20, torch.int64), z(20), z(2), z(1), z(1), z(RING_CAP * 18), z(1), RING_CAP)
    for rows in (0, 17):
        with pytest.raises(RuntimeError, match="1 <= rows <= 16"):
            _native.lookup_verify_sample(*args(rows))
    with pytest.raises(RuntimeError, match="null pointer"):
        a = list(args(1))
        lib = _native.load()
        rc = lib.pc_lookup_verify_sample(a[0].data_ptr(), V, V, 1, 0, a[5].data_ptr(), a[6].data_ptr(), a[7].data_ptr(), a[8].data_ptr(),
                                         a[9].data_ptr(), a[10].data_ptr(), 8, a[11].data_ptr(), a[12].data_ptr(), a[13].data_ptr(),
                                         a[14].data_ptr(), a[15].data_ptr(), a[16].data_ptr(), a[17].data_ptr(), RING_CAP, 0,
                                         _native.current_stream())
        _native.check(rc, "pc_lookup_verify_sample")
    with pytest.raises(RuntimeError, match="2\\^24"):
        lib = _native.load()
        a = list(args(1))
        rc = lib.pc_lookup_verify_sample(a[0].data_ptr(), 1 << 24, 1 << 24, 1, a[4].data_ptr(), a[5].data_ptr(), a[6].data_ptr(),
                                         a[7].data_ptr(), a[8].data_ptr(), a[9].data_ptr(), a[10].data_ptr(), 8, a[11].data_ptr(),
                                         a[12].data_ptr(), a[13].data_ptr(), a[14].data_ptr(), a[15].data_ptr(), a[16].data_ptr(),
                                         a[17].data_ptr(), RING_CAP, 0, _native.current_stream())
        _native.check(rc, "pc_lookup_verify_sample")


# ---- SampleLookupLoop ----------------------------------------------------------------------------------------------------------------
# (the mid_gqa shape and fixture recipe of tests/test_gpu_lookup.py)
SHAPE, W_SEED, W_SCALE, CTX_LEN, N_NEW = "mid_gqa", 108, 3.0, 40, 24
# The filters are off in the loop tests: a token at the top-p boundary may flip under the 1e-2 logit noise between two forward
# shapes; they are covered on identical logits above.  DRAW_SEED was chosen on the CPU (LlamaOracle + sample_ref.draw) so that
# the oracle's score margin exceeds 2 * LOGIT_TOL / T at every position (0.088 at its smallest); the oracle test re-checks it.
LOOP_PARAMS, DRAW_SEED = (0.8, 1.1, 1.0, 0), 1


def _gen_params(params, max_new=N_NEW + 1, stop=()):
    from promptcache_amd import GenerationParameters
    T, rp, tp, tk = params
    return GenerationParameters(temperature=T, repetition_penalty=rp, top_p=tp, top_k=tk if tk > 0 else -1, max_new_tokens=max_new,
                                stop_token_ids=list(stop), stop_str=[])


@pytest.fixture(scope="module")
def model():
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    shape = SHAPES[SHAPE]
    w16 = make_weights_np(shape, W_SEED, W_SCALE)
    lm = Llama2(name="lks", shape=shape, weights=w16, device=DEV)
    ctx = np.random.default_rng(W_SEED).integers(3, shape.vocab_size, size=CTX_LEN).tolist()
    return lm, shape, w16, ctx


def _prefill(lm, ctx, params=LOOP_PARAMS, seed=DRAW_SEED):
    """-> (past, first token: drawn from the prefill's last row at step 0, as GenerationEngine draws it)."""
    out = lm(input_ids=torch.tensor([ctx]), position_ids=torch.tensor([list(range(len(ctx)))]), use_cache=True)
    first = lm.hf_model.sample_token(out.logits[0, -1], _gen_params(params), seed, ctx)
    return out.past_key_values, first


def _run(lm, ctx, corpus, k, max_new, device_loop, extra=0, keep=False, params=LOOP_PARAMS, seed=DRAW_SEED):
    """One sampled lookup generation of ``max_new`` tokens behind a fresh prefill -> (first token, per-step token lists, loop,
    per-step (logits [k+1][V], state words before the verify stage... taken by the stepped mode only))."""
    from promptcache_amd.model.llama_hip import SampleLookupLoop
    past, first = _prefill(lm, ctx, params, seed)
    loop = lm.hf_model.lookup_loop(past, first, len(ctx), max_new, k, corpus, params=_gen_params(params), seed=seed,
                                   history_ids=ctx + [first])
    assert type(loop) is SampleLookupLoop
    loop.device_loop = device_loop
    steps, kept, got = [], [], 0
    while got < max_new:
        i = loop.enqueue()
        t = loop.tokens(i)
        assert 1 <= len(t) <= k + 1
        if keep:
            kept.append(_snapshot(loop))
        steps.append(t)
        got += len(t)
    for _ in range(extra):
        steps.append(loop.tokens(loop.enqueue()))
    return first, steps, loop, kept


def _snapshot(loop):
    """The stepped mode's logits of the step just run and the state words behind it."""
    st = loop.st
    snap = {n: st[n].cpu().numpy().copy() for n in ("ids", "pos", "past", "ndraft", "budget", "ctr", "hist_len", "draws")}
    snap["bits"] = st["bits"].cpu().numpy().view(np.uint32).copy()
    snap["hist"] = st["hist"].cpu().numpy().copy()
    snap["ring"] = loop.ring.cpu().numpy().copy()
    snap["logits"] = loop.logits[0, :loop.k + 1].float().cpu().numpy().copy()
    return snap


@pytest.fixture(scope="module")
def reference_run(model):
    """The one-token sampled generation (SampleLoop): first token + N_NEW tokens, same seed and parameters."""
    from promptcache_amd.model.llama_hip import SampleLoop
    lm, shape, w16, ctx = model
    past, first = _prefill(lm, ctx)
    loop = lm.hf_model.sample_loop(past, first, len(ctx), N_NEW + 1, _gen_params(LOOP_PARAMS), DRAW_SEED, ctx + [first])
    assert type(loop) is SampleLoop
    T = [loop.token(loop.enqueue()) for _ in range(N_NEW)]
    loop.close(N_NEW)
    return first, T


@pytest.mark.parametrize("k", [3, 7])
def test_device_loop_equals_the_stepped_mode(model, reference_run, k):
    lm, shape, w16, ctx = model
    first, T = reference_run
    kv = {}
    for dev_loop in (True, False):
        f, steps, loop, _ = _run(lm, ctx, ctx[-8:] + [first] + T, k, N_NEW, dev_loop)
        assert loop.len0 == CTX_LEN
        loop.close(N_NEW)
        a = loop.arena
        assert a.length == CTX_LEN + N_NEW
        kv[dev_loop] = (f, steps, a.buf[:, :, :, :, CTX_LEN:CTX_LEN + N_NEW].clone())
    assert kv[True][0] == kv[False][0] and kv[True][1] == kv[False][1]        # tokens and per-step counts
    assert torch.equal(kv[True][2], kv[False][2])                              # K / V rows of every layer, bit for bit
    assert len(kv[True][1]) < N_NEW                                            # (the corpus is the answer: steps were saved)
    assert lm.hf_model._live_loop is None


def test_every_step_follows_the_host_model(model, reference_run):
    """Stepped mode: every step's record, draws, budget and past equal verify_sample run on that very step's logits; the three
    corpora give the same tokens, and the step counts are the simulation's."""
    from tests import lookup_ref as lr
    lm, shape, w16, ctx = model
    first, T = reference_run
    k, V = 7, shape.vocab_size
    full = ctx[-8:] + [first] + T
    wrong = list(full)
    wrong[8 + 1 + 6] = (wrong[8 + 1 + 6] + 1) % V or 3
    wrong[8 + 1 + 15] = (wrong[8 + 1 + 15] + 1) % V or 3
    assert len(lr.simulate(full, first, T, k)) < len(T)          # (a condition on the inputs: the full corpus saves steps)
    low = 0
    for corpus in ([], full, wrong):
        f, steps, loop, kept = _run(lm, ctx, corpus, k, N_NEW, False, keep=True)
        loop.close(N_NEW)
        assert f == first and [t for s in steps for t in s] == T, corpus is full
        assert [len(s) for s in steps] == lr.simulate(corpus, first, T, k), corpus is full
        # the state before step j's verify stage: the words after step j - 1 (the initial ones for j = 0) + step j's drafts
        hist0 = [int(t) for t in corpus] + [first]
        before = dict(hist=np.zeros(kept[0]["hist"].size, dtype=np.int32), hist_len=np.array([len(hist0)], dtype=np.int32),
                      ids=np.full(16, first, dtype=np.int64), pos=np.full(16, CTX_LEN, dtype=np.int32),
                      past=np.array([CTX_LEN, 0], dtype=np.int32), ndraft=np.zeros(1, dtype=np.int32),
                      budget=np.array([N_NEW], dtype=np.int32), ring=np.zeros((loop.RING, k + 2), dtype=np.int32),
                      ctr=np.zeros(1, dtype=np.int32), bits=lsr.history_bits(ctx + [first], V), draws=np.ones(1, dtype=np.int32))
        before["hist"][:len(hist0)] = hist0
        for j, snap in enumerate(kept):
            ids, pos, m = lr.draft_state(before["hist"], before["hist_len"][0], before["ids"], before["pos"], k)
            st = dict(before, ids=ids[:k + 1], pos=pos[:k + 1], ndraft=np.array([m], dtype=np.int32), past=before["past"][:2])
            want, info = lsr.verify_sample(snap["logits"], st, loop.RING, LOOP_PARAMS, DRAW_SEED)
            if min(info["margins"][:info["acc"] + 1]) <= MARGIN:
                low += 1
                break                                            # (the words behind a race this close are not the reference's to call)
            assert int(snap["ndraft"][0]) == m
            assert snap["ring"][j].tolist()[:1 + info["emit"]] == [info["emit"]] + info["tokens"][:info["emit"]] == \
                want["ring"].reshape(loop.RING, k + 2)[j].tolist()[:1 + info["emit"]], (j, corpus is full)
            for name in ("draws", "budget", "ctr", "hist_len"):
                assert int(snap[name][0]) == int(want[name][0]), (j, name)
            assert int(snap["past"][0]) == int(want["past"][0]) and int(snap["ids"][0]) == int(want["ids"][0])
            assert np.array_equal(snap["bits"], want["bits"]), j
            assert np.array_equal(snap["hist"][:int(want["hist_len"][0])], want["hist"][:int(want["hist_len"][0])]), j
            before = dict(want, ids=np.concatenate([want["ids"], np.full(16 - k - 1, first, dtype=np.int64)]),
                          pos=np.concatenate([want["pos"], np.full(16 - k - 1, CTX_LEN, dtype=np.int32)]))
    assert low == 0, low


def test_tokens_are_the_sample_loops_and_logits_the_oracles(model, reference_run):
    """Against SampleLoop (same seed and parameters) the N_NEW tokens are equal; teacher-forced through the numpy oracle, every
    emitted position's logits are within the parity bar and every token is the oracle's draw, whose score margin exceeds
    2 * LOGIT_TOL / T at EVERY position (each of two scores may move by LOGIT_TOL / T) -- re-checked here on the inputs."""
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    lm, shape, w16, ctx = model
    first, T = reference_run
    Tm, rp, tp, tk = LOOP_PARAMS
    f, steps, loop, kept = _run(lm, ctx, ctx[-8:] + [first] + T, 3, N_NEW, False, keep=True)
    loop.close(N_NEW)
    assert f == first and [t for s in steps for t in s] == T
    dev_rows = np.concatenate([snap["logits"][:len(s)] for snap, s in zip(kept, steps)], axis=0)
    assert dev_rows.shape[0] == N_NEW
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=lm.hf_model.inv_freq_cpu.numpy())
    oracle = LlamaOracle(cfg, {n: v.astype(np.float32) for n, v in w16.items()})
    with H.oracle_blas():
        olog, present = oracle.forward(np.array([ctx]), np.arange(len(ctx))[None])
        tok, margin, _ = sr.draw(olog[0, -1], ctx, Tm, rp, tp, tk, DRAW_SEED, 0)
        assert tok == first
        worst, fed, hist = 0.0, first, ctx + [first]
        for i in range(N_NEW):
            olog, present = oracle.forward(np.array([[fed]]), np.array([[len(ctx) + i]]), past=present)
            row = olog[0, -1]
            tok, mg, _ = sr.draw(row, hist, Tm, rp, tp, tk, DRAW_SEED, 1 + i)
            margin = min(margin, mg)
            worst = max(worst, float(np.abs(dev_rows[i] - row).max()))
            assert tok == T[i], i
            fed = T[i]
            hist.append(fed)
    print(f"sampled lookup steps vs oracle: max |dlogit| = {worst:.2e}; oracle score margin >= {margin:.3f}")
    assert margin > 2 * LOGIT_TOL / Tm
    assert worst < LOGIT_TOL


def test_budget_and_memory_safety(model, reference_run):
    from tests import lookup_ref as lr
    lm, shape, w16, ctx = model
    m = lm.hf_model
    first, T = reference_run
    k, max_new = 3, 10
    corpus = ctx[-8:] + [first] + T
    past, f = _prefill(lm, ctx)
    assert f == first
    loop = m.lookup_loop(past, first, len(ctx), max_new, k, corpus, params=_gen_params(LOOP_PARAMS), seed=DRAW_SEED,
                         history_ids=ctx + [first])
    a = loop.arena
    lo = CTX_LEN + max_new + k + 1
    assert a.cap >= lo + 1
    with torch.inference_mode():
        a.buf[:, :, :, :, lo:] = 0.5
    before = a.buf[:, :, :, :, lo:].clone()
    need = len(lr.simulate(corpus, first, T[:max_new], k))
    steps = [loop.tokens(loop.enqueue()) for _ in range(need)]
    torch.cuda.synchronize()
    draws, bits = int(loop.st["draws"][0]), loop.st["bits"].clone()
    assert draws == 1 + max_new
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), lsr.history_bits(ctx + [first] + T[:max_new], shape.vocab_size))
    steps += [loop.tokens(loop.enqueue()) for _ in range(6)]                     # six surplus replays
    assert sum(map(len, steps)) == max_new and [t for s in steps for t in s] == T[:max_new]
    assert all(len(s) > 0 for s in steps[:need]) and all(len(s) == 0 for s in steps[need:])
    torch.cuda.synchronize()
    assert torch.equal(a.buf[:, :, :, :, lo:], before)                         # nothing behind the rows the budget allows
    assert int(loop.st["draws"][0]) == draws and torch.equal(loop.st["bits"], bits)
    assert int(loop.st["past"][0]) == CTX_LEN + max_new and int(loop.st["budget"][0]) == 0
    consumed = 7
    loop.close(consumed)
    assert a.length == CTX_LEN + consumed and m._live_loop is None


# ---- GenerationEngine(lookup=k, lookup_sampled=True) ---------------------------------------------------------------------------
# torch.manual_seed(ENGINE_SEED): chosen on the CPU (the oracle's cached prefill + sample_ref.draw) so that the oracle's score
# margin exceeds 2 * LOGIT_TOL / T at each of the ENGINE_NEW positions of the golden `mid_trip` case under LOOP_PARAMS
ENGINE_SEED, ENGINE_NEW = 1, 12


def test_engine_switch():
    from promptcache_amd import GenerationEngine, GenerationParameters, Prompt
    from promptcache_amd.model.llama_hip import LookupLoop, SampleLookupLoop, SampleLoop
    from tests.test_gpu_engine import build_product
    g = H.load_case("mid_trip")
    lm, eng = build_product(g)
    hf = lm.hf_model
    assert hf.lookup_available()
    prompt = Prompt(str(g["prompt_text"]), [lm.get_formatter()])
    made = []

    class Rec(GenerationEngine):
        """Records the emitted ids; ``answer``: appended to what a lookup generation may copy from (a random-weight model does
        not quote its prompt, and the steps below are to carry several tokens)."""
        answer = []

        def _render(self, output_ids, new_ids, stop_strs):
            self.ids = list(new_ids)
            return super()._render(output_ids, new_ids, stop_strs)

        @staticmethod
        def _lookup_corpus(cache, token_ids):
            return GenerationEngine._lookup_corpus(cache, token_ids) + Rec.answer

    orig = hf.lookup_loop

    def spy(*a, **k):
        loop = orig(*a, **k)
        made.append(loop)
        return loop

    def run(params, seed=ENGINE_SEED, **kw):
        ids, pos, _, cache = eng.process(prompt)
        torch.manual_seed(seed)
        e = Rec(lm, **kw)
        kinds, outs = set(), []
        for o in e.generate(ids, pos, params, cache, stream_interval=1):
            outs.append(o)
            if hf._live_loop is not None:
                kinds.add(type(hf._live_loop))
        assert hf._live_loop is None
        return outs, kinds, e.ids

    hf.lookup_loop = spy
    try:
        sampled = _gen_params(LOOP_PARAMS, ENGINE_NEW)
        want_outs, kinds, want_ids = run(sampled, lookup=7, lookup_sampled=False)
        assert kinds == {SampleLoop} and len(want_ids) == ENGINE_NEW and not made
        Rec.answer = list(want_ids)
        outs, kinds, ids = run(sampled, lookup=7, lookup_sampled=True)
        assert kinds == {SampleLookupLoop} and len(made) == 1
        assert ids == want_ids and outs[-1].new_text == want_outs[-1].new_text and outs[-1].text == want_outs[-1].text
        assert len(outs) == len(want_outs)                                      # one Output per token, as without lookup
        assert made[0].n < ENGINE_NEW - 1                                       # (the answer was there to copy: steps were saved)
        _, kinds, _ = run(sampled, lookup=0, lookup_sampled=True)
        assert kinds == {SampleLoop}
        n_graphs = sum(1 for key in hf._graphs if key[:2] == ("loop", "lookup") and key[-1] == "sample")
        # greedy with a penalty takes the sampled lookup loop too -- through the graph the sampled request captured
        pen = GenerationParameters(temperature=0.0, repetition_penalty=1.2, max_new_tokens=ENGINE_NEW, stop_token_ids=[], stop_str=[])
        Rec.answer = []
        _, kinds, pen_ids = run(pen, lookup=7, lookup_sampled=True)
        assert kinds == {SampleLookupLoop}
        assert sum(1 for key in hf._graphs if key[:2] == ("loop", "lookup") and key[-1] == "sample") == n_graphs >= 1
        _, kinds, pen_want = run(pen, lookup=7, lookup_sampled=False)
        assert kinds == {SampleLoop}
        print(f"greedy with a penalty, lookup vs one-token loop: {pen_ids} / {pen_want}")
        # plain greedy keeps LookupLoop
        greedy = GenerationParameters(temperature=0.0, max_new_tokens=len(g["greedy"]), stop_token_ids=[], stop_str=[])
        outs, kinds, _ = run(greedy, lookup=7, lookup_sampled=True)
        assert kinds == {LookupLoop} and outs[-1].new_text == lm.decode(g["greedy"].tolist())
        # a stop id in the middle of a step: the rest of the step is dropped and the arena ends at the consumed row
        Rec.answer = list(want_ids)
        stop = want_ids[4]
        cut = want_ids.index(stop)
        del made[:]
        outs, kinds, ids = run(_gen_params(LOOP_PARAMS, ENGINE_NEW, stop=[stop]), lookup=7, lookup_sampled=True)
        assert kinds == {SampleLookupLoop} and ids == want_ids[:cut + 1]
        assert outs[-1].new_text == lm.decode(want_ids[:cut + 1])
        loop = made[0]
        produced = [t for i in range(loop.n) for t in loop.tokens(i)]
        assert produced[:cut] == want_ids[1:cut + 1] and len(produced) > cut     # (the step went on behind the stop id)
        assert loop.arena.length == loop.len0 + cut and hf._live_loop is None
    finally:
        del hf.lookup_loop
