"""The device sampler (csrc/pc_sample.hip, pc_sample_advance) and the sampled decode loop (model/llama_hip.py SampleLoop) on the
GPU: the processed row against the REFERENCE's chain (tests/golden/sampling_chain.npz), the draw against its numpy restatement
(tests/sample_ref.py), the distribution of draws, the loop-state contract, and generate() end to end."""
import os
from collections import Counter

import numpy as np
import pytest
import torch

from oracle import sampling_oracle as so
from tests import sample_ref as sr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_chain.npz")
MARGIN = 1e-4
PARAM_SETS = ((1.0, 1.0, 0.95, -1), (0.7, 1.1, 0.9, 40), (1.3, 1.0, 1.0, -1), (0.0, 1.3, 1.0, -1), (0.8, 1.2, 0.5, 5),
              (0.9, 1.0, 0.999, 1000), (2.0, 1.0, 0.3, -1), (0.6, 1.0, 1.0, 1))


class _State:
    """Device words of one eager pc_sample_advance (the loop state's layout)."""

    def __init__(self, V, history=(), step=0, ring=64):
        from promptcache_amd.model.llama_hip import _history_bits
        self.V = V
        self.ids = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.pos = torch.full((1,), 100, dtype=torch.int32, device="cuda")
        self.past = torch.full((2,), 50, dtype=torch.int32, device="cuda")
        self.ring = torch.full((ring,), -1, dtype=torch.int32, device="cuda")
        self.ctr = torch.full((1,), step, dtype=torch.int32, device="cuda")
        self.hist = _history_bits(history, V).cuda()
        self.params = torch.zeros(24, dtype=torch.uint8, device="cuda")

    def set_params(self, T, rp, tp, tk, seed):
        from promptcache_amd import _native
        self.params.copy_(torch.frombuffer(bytearray(_native.sample_params_bytes(T, rp, tp, tk, seed)), dtype=torch.uint8))

    def advance(self, row, processed=None):
        from promptcache_amd import _native
        _native.sample_advance(row, self.V, self.params, self.hist, self.ids, self.pos, self.past, self.ring, self.ctr, processed)


def _row(x, offset=0):
    """A device fp32 row holding ``x`` at ``offset`` floats past a 256-byte aligned base (offset 1: 4- but not 16-byte aligned)."""
    buf = torch.full((len(x) + offset + 4,), 7.0, dtype=torch.float32, device="cuda")
    r = buf[offset:offset + len(x)]
    r.copy_(torch.as_tensor(np.asarray(x, dtype=np.float32)))
    return r


def _draw_on_device(x, history, T, rp, tp, tk, seed, step, offset=0):
    st = _State(len(x), history, step)
    st.set_params(T, rp, tp, tk, seed)
    proc = torch.empty(len(x), dtype=torch.float32, device="cuda")
    st.advance(_row(x, offset), proc)
    torch.cuda.synchronize()
    return int(st.ids[0]), proc.cpu().numpy(), st


def _mass_above(pre):
    """float64 softmax mass ranked strictly above every token (value descending, the higher index first among equal values)."""
    order = np.argsort(pre, kind="stable")[::-1]
    e = np.exp(pre[order].astype(np.float64) - pre.max())
    e /= e.sum()
    above = np.empty_like(e)
    above[order] = np.concatenate([[0.0], np.cumsum(e)[:-1]])
    return above


def test_processed_row_matches_the_reference_fixture():
    z = np.load(GOLD)
    near_total = 0
    for i, (t, rp, tp, tk) in enumerate(z["params"]):
        t, rp, tp, tk = float(t), float(rp), float(tp), int(tk)
        logits, hist, want = z["logits"][i], z["history"][i], z["processed"][i]
        _, got, _ = _draw_on_device(logits, hist.tolist(), t, rp, tp, tk, seed=1, step=0)
        keep, gk = np.isfinite(want), np.isfinite(got)
        differ = np.nonzero(keep != gk)[0]
        if 1e-8 <= tp < 1.0:
            pre = so.process_logits(logits, hist, t, rp, 1.0, -1)
            near = np.abs(_mass_above(pre) - tp) < 1e-5
        else:
            near = np.zeros(len(want), dtype=bool)
        near_total += int(near.sum())
        assert np.all(near[differ]), (i, t, rp, tp, tk, differ[~near[differ]][:10])
        both = keep & gk
        assert np.array_equal(got[both], want[both]), (i, t, rp, tp, tk)      # temperature and penalty are IEEE-exact
    print(f"[sampling_chain] tokens within 1e-5 of the top-p boundary: {near_total}")


@pytest.mark.parametrize("V", [2048, 1001, 32000, 32016, 50432, 65024])
def test_draws_equal_the_reference_helper(V):
    rng = np.random.default_rng(V)
    checked = 0
    for j in range(64):
        T, rp, tp, tk = PARAM_SETS[j % len(PARAM_SETS)]
        x = (rng.standard_normal(V) * rng.uniform(0.5, 4.0)).astype(np.float32)
        if j % 5 == 0:
            x[rng.integers(0, V, 16)] = x.max()                       # ties at the top
        if j % 7 == 0:
            x = np.round(x * 4) / 4                                   # many ties everywhere (top-p boundary inside a tie group)
        hist = rng.integers(0, V, 40).tolist()
        seed, step = int(rng.integers(0, 2 ** 62)), int(rng.integers(0, 5000))
        tok, proc, _ = _draw_on_device(x, hist, T, rp, tp, tk, seed, step, offset=1 if j % 4 == 3 else 0)
        want, margin, wproc = sr.draw(x, hist, T, rp, tp, tk, seed, step)
        assert np.isfinite(proc[tok]), (j, T, rp, tp, tk)
        if margin > MARGIN:
            assert tok == want, (V, j, T, rp, tp, tk, seed, step, tok, want, margin)
            checked += 1
    assert checked >= 48, checked


def test_distribution_of_graph_replayed_draws():
    """20 000 replays of a graph holding one pc_sample_advance node: the step counter advances on the device."""
    rng = np.random.default_rng(11)
    V, n = 512, 20000
    x = (rng.standard_normal(V) * 2.5).astype(np.float32)
    T, tp, tk = 0.9, 0.9, 30
    st = _State(V, (), 0, ring=n)
    st.set_params(T, 1.0, tp, tk, 0x1234_5678_9abc)
    row = _row(x)
    st.advance(row)                                  # eager first launch (code object load) outside the capture
    st.ctr.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.advance(row)
    for _ in range(n):
        g.replay()
    torch.cuda.synchronize()
    assert int(st.ctr[0]) == n and int(st.pos[0]) == 100 + n + 1 and int(st.past[0]) == 50 + n + 1
    toks = st.ring.cpu().numpy()
    proc = so.process_logits(x, [], T, 1.0, tp, tk)
    keep = np.isfinite(proc)
    assert keep[toks].all(), "a filtered token was drawn"
    e = np.exp(proc[keep].astype(np.float64) - proc[keep].max())
    p = np.zeros(V)
    p[keep] = e / e.sum()
    tv = 0.5 * np.abs(np.bincount(toks, minlength=V) / n - p).sum()
    print(f"[distribution] TV over {n} draws, {keep.sum()} kept tokens: {tv:.4f}")
    assert tv < 0.02, tv


def test_state_contract_history_and_greedy_equivalence():
    from promptcache_amd import _native
    rng = np.random.default_rng(5)
    V, N = 32000, 6
    x = (rng.standard_normal(V) * 3).astype(np.float32)
    # greedy with a penalty: every step's token is penalised on the next (the history bit is set on the device)
    st = _State(V, [3, 77], step=10)
    st.set_params(0.0, 1.5, 1.0, -1, 99)
    row = _row(x)
    hist, toks = [3, 77], []
    for k in range(N):
        st.advance(row)
        want, _, _ = sr.draw(x, hist, 0.0, 1.5, 1.0, -1, 99, 10 + k)
        toks.append(want)
        hist.append(want)
    torch.cuda.synchronize()
    assert int(st.ids[0]) == toks[-1] and int(st.pos[0]) == 100 + N and int(st.past[0]) == 50 + N
    assert int(st.ctr[0]) == 10 + N and st.ring[10:10 + N].tolist() == toks and len(set(toks)) == N
    bits = st.hist.cpu().numpy().view(np.uint32)
    for t in set(hist):
        assert (bits[t >> 5] >> (t & 31)) & 1, t
    assert sum(bin(int(b)).count("1") for b in bits) == len(set(hist))

    # top_k = 1 and greedy mode pick pc_greedy_advance's token (ties: the lowest index)
    for V in (1001, 32000, 65024):
        x = (rng.standard_normal(V) * 3).astype(np.float32)
        x[[V // 3, V // 2]] = x.max() + 1.0
        g_ids, g_pos, g_past = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), \
            torch.zeros(2, dtype=torch.int32, device="cuda")
        g_ring, g_ctr = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        _native.greedy_advance(_row(x), V, g_ids, g_pos, g_past, g_ring, g_ctr)
        want = int(g_ids[0])
        assert want == V // 3
        assert _draw_on_device(x, [], 0.0, 1.0, 1.0, -1, 1, 0)[0] == want
        assert _draw_on_device(x, [], 1.0, 1.0, 0.0, -1, 1, 0)[0] == want
        for seed in range(4):
            assert _draw_on_device(x, [], 0.7, 1.0, 1.0, 1, seed, seed)[0] in (V // 3, V // 2)
        x[V // 2] = np.nextafter(x[V // 2], np.float32(np.inf))
        assert _draw_on_device(x, [], 1.0, 1.0, 1.0, 1, 3, 3)[0] == V // 2

    # all -inf (and NaN) rows give token 0
    for fill in (-np.inf, np.nan):
        tok, proc, _ = _draw_on_device(np.full(1000, fill, dtype=np.float32), [], 1.0, 1.0, 0.9, 10, 1, 0)
        assert tok == 0 and np.all(proc == -np.inf)


# ---- generate() end to end ------------------------------------------------------------------------------------------------
def _family(family):
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Falcon, Llama2
    from promptcache_amd.model.config import FALCON_SHAPES, SHAPES
    from promptcache_amd.model.weights import make_falcon_weights_np, make_weights_np
    if family == "falcon":
        lm = Falcon(name="x", shape=FALCON_SHAPES["falcon-mid"], weights=make_falcon_weights_np(FALCON_SHAPES["falcon-mid"], 4, 3.0), device="cuda:0")
    elif family == "llama_int8":
        lm = Llama2(name="x", shape=SHAPES["mid64_gqa"], weights=make_weights_np(SHAPES["mid64_gqa"], 4, 1.0), device="cuda:0", load_in_8bit=True)
    else:
        lm = Llama2(name="x", shape=SHAPES["mid_gqa"], weights=make_weights_np(SHAPES["mid_gqa"], 4, 3.0), device="cuda:0")
    sp, pp = synth.flat_docs("gl", 12, (40, 33), 9, seed=6)
    fmt = lm.get_formatter()
    eng = CacheEngine(160, lm)                     # S + q + 100 new tokens > 160: the loop must grow the arena up front
    eng.add_schema(fmt(sp))
    return lm, eng, Prompt(pp, [fmt])


def _engine_class():
    from promptcache_amd import GenerationEngine

    class Rec(GenerationEngine):
        """Records the emitted ids and refuses the stepped sampler."""

        def _render(self, output_ids, new_ids, stop_strs):
            self.ids = list(new_ids)
            return super()._render(output_ids, new_ids, stop_strs)

        @staticmethod
        def _pick(last_logits, greedy):
            raise AssertionError("the stepped sampler ran: the sampled device loop was not engaged")
    return Rec


def _generate(lm, eng, prompt, params, seed, engine=None, take=None):
    from promptcache_amd import GenerationEngine
    Eng = engine or _engine_class()
    ids, pos, _, cache = eng.process(prompt)
    torch.manual_seed(seed)
    e = Eng(lm)
    gen = e.generate(ids, pos, params, cache, stream_interval=1)
    outs = []
    for o in gen:
        outs.append(o)
        if take is not None and len(outs) >= take:
            gen.close()
            break
    return outs, getattr(e, "ids", None), ids, pos


@pytest.mark.parametrize("family", ["llama", "falcon", "llama_int8"])
def test_generate_runs_the_sampled_device_loop(family):
    from promptcache_amd import GenerationEngine, GenerationParameters
    lm, eng, prompt = _family(family)
    hf = lm.hf_model
    T, rp, tp, tk = 0.8, 1.1, 0.9, 40
    params = GenerationParameters(temperature=T, repetition_penalty=rp, top_p=tp, top_k=tk, max_new_tokens=100,
                                  stop_token_ids=[], stop_str=[])
    made = []
    orig = hf.sample_loop

    def spy(*a, **k):
        loop = orig(*a, **k)
        made.append(loop)
        return loop
    hf.sample_loop = spy
    try:
        outs, emitted, ids, pos = _generate(lm, eng, prompt, params, 7)
    finally:
        del hf.sample_loop
    # (a) the sampled loop ran (the recording engine refuses the stepped sampler)
    assert len(made) == 1 and made[0] is not None and type(made[0]).__name__ == "SampleLoop"
    assert len(emitted) == 100 and outs[-1].new_text == lm.decode(emitted)

    # (b) teacher-forced: the reference helper on the stepped logits picks the emitted token at every step
    torch.manual_seed(7)
    seed = int(torch.randint(0, 2 ** 62, (1,)))
    ids2, pos2, _, cache = eng.process(prompt)
    out = lm(input_ids=torch.tensor([ids2], device="cuda"), position_ids=torch.tensor([pos2], device="cuda"), past_key_values=cache,
             use_cache=True)
    past, p0, history, close = out.past_key_values, max(pos2) + 1, list(ids2), 0
    logits = out.logits[0, -1].float().cpu().numpy()
    for k in range(100):
        want, margin, _ = sr.draw(logits, history, T, rp, tp, tk, seed, k)
        if margin > MARGIN:
            assert emitted[k] == want, (family, k, emitted[k], want, margin)
        else:
            close += 1
        history.append(emitted[k])
        if k == 99:
            break
        o = lm(input_ids=torch.tensor([[emitted[k]]], device="cuda"), position_ids=torch.tensor([[p0 + 1 + k]], device="cuda"),
               past_key_values=past, use_cache=True)
        past, logits = o.past_key_values, o.logits[0, -1].float().cpu().numpy()
    del past, out
    assert close <= 5, close

    # (c) the torch seed governs the draw
    again, _, _, _ = _generate(lm, eng, prompt, params, 7)
    assert again[-1].new_text == outs[-1].new_text
    short = GenerationParameters(temperature=T, repetition_penalty=rp, top_p=tp, top_k=tk, max_new_tokens=12, stop_token_ids=[], stop_str=[])
    others = [_generate(lm, eng, prompt, short, s)[1] for s in (1, 2, 3, 4)]
    assert any(o != emitted[:12] for o in others), "four other seeds all reproduced the same tokens: the draw ignores the seed"

    # (d) a stop token seen mid-way truncates where the teacher-forced sequence says
    stop = emitted[12]
    first = emitted.index(stop)
    sp = GenerationParameters(temperature=T, repetition_penalty=rp, top_p=tp, top_k=tk, max_new_tokens=100, stop_token_ids=[stop], stop_str=[])
    s_outs, s_ids, _, _ = _generate(lm, eng, prompt, sp, 7)
    assert s_ids == emitted[:first + 1] and s_outs[-1].new_text == lm.decode(emitted[:first + 1])

    # (e) an abandoned generator leaves the arena right for the next process() + generate()
    _generate(lm, eng, prompt, params, 7, take=5)
    after, after_ids, _, _ = _generate(lm, eng, prompt, params, 7)
    assert after_ids == emitted

    # (f) another parameter set reuses the captured sampled-loop graph
    n_graphs = sum(1 for k in hf._graphs if k[:2] == ("loop", "sample"))
    assert n_graphs >= 1
    other = GenerationParameters(temperature=1.0, top_p=0.95, max_new_tokens=100, stop_token_ids=[], stop_str=[])
    _generate(lm, eng, prompt, other, 3)
    assert sum(1 for k in hf._graphs if k[:2] == ("loop", "sample")) == n_graphs
    assert GenerationEngine.device_sample_loop


def test_greedy_with_a_repetition_penalty_equals_stepping():
    from promptcache_amd import GenerationEngine, GenerationParameters
    lm, eng, prompt = _family("llama")
    params = GenerationParameters(temperature=0.0, repetition_penalty=1.3, max_new_tokens=100, stop_token_ids=[], stop_str=[])
    dev, dev_ids, _, _ = _generate(lm, eng, prompt, params, 0)
    try:
        GenerationEngine.device_sample_loop = False
        step, _, _, _ = _generate(lm, eng, prompt, params, 0, engine=GenerationEngine)
    finally:
        GenerationEngine.device_sample_loop = True
    assert len(dev_ids) == 100
    assert [o.new_text for o in dev] == [o.new_text for o in step]
    assert max(Counter(dev_ids).values()) < 100
