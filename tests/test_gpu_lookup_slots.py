"""Prompt-lookup drafts in the batched slot loop on the GPU: pc_lookup_draft_slots / pc_rope_append_slots_rows /
pc_attn_verify_slots / pc_lookup_verify_slots through the C-ABI against tests/lookup_slots_ref.py and the existing B = 1 and slot
entries, slot invariance bit for bit, ``LookupSlotLoop`` against solo runs, ``GreedyLoop``, the host model and the numpy oracle, and
``GenerationEngine.generate_batch(lookup=k)`` end to end."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import lookup_ref as lr
from tests import lookup_slots_ref as ref
from tests.test_gpu_slots import SENT, Slots, _append_ex, _i32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATT_TOL = 2e-4          # the project's attention-kernel bar (tests/test_gpu_slots.py)
LOGIT_TOL = 1e-2        # the project's parity bar
RING_CAP, HIST_CAP = 4, 64


def _n():
    from promptcache_amd import _native
    _native.load()
    return _native


def _dev(st):
    return {n_: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for n_, v in st.items()}


def _same(dev, want, names=None):
    for name in (names or want):
        got = dev[name].cpu().numpy()
        assert np.array_equal(got, want[name]), (name, got, want[name])


# ---- 1. draft and verify: every word ------------------------------------------------------------------------------------------
def _lookup_state(rng, S, k):
    """S slots: every third one idle, one without room for a step's rows, budgets 0 / 1 / 3 / 40, counters around the ring's end."""
    st = dict(hist=rng.integers(0, 5, size=(S, HIST_CAP)).astype(np.int32),           # 5 symbols: matches everywhere
              hist_len=rng.integers(6, 30, size=S).astype(np.int32), ids=np.full((S, k + 1), -7, dtype=np.int64),
              pos=np.full((S, k + 1), -9, dtype=np.int32), ndraft=np.full(S, -1, dtype=np.int32),
              budget=np.array([(40, 3, 1, 0)[b % 4] for b in range(S)], dtype=np.int32),
              stop_ids=np.full((S, 8), -1, dtype=np.int32), ring=np.full((S, RING_CAP, k + 2), -5, dtype=np.int32),
              ctr=np.array([RING_CAP - 1 + b for b in range(S)], dtype=np.int32),
              len=np.array([10 + 7 * b for b in range(S)], dtype=np.int32), cap=np.zeros(S, dtype=np.int32),
              live=np.array([0 if b % 3 == 1 else 1 for b in range(S)], dtype=np.int32))
    st["cap"][:] = st["len"] + 2 * (k + 1) + 1
    if S > 2:
        st["cap"][S - 1] = st["len"][S - 1] + k                      # live, but len + k + 1 > cap
        st["live"][S - 1] = 1
    if S > 1:                                                         # slot 0: the suffix 7 8 9 occurs at the front, k followers
        st["hist"][0, :20] = list(range(7, 24)) + [7, 8, 9]
        st["hist_len"][0] = 20
    for b in range(S):
        st["ids"][b, 0] = st["hist"][b, st["hist_len"][b] - 1]
        st["pos"][b, 0] = 100 + b
    return st


@pytest.mark.parametrize("V", [2048, 32003])
@pytest.mark.parametrize("S,k", [(1, 1), (1, 3), (1, 15), (3, 1), (3, 3), (3, 15), (16, 1), (16, 3)])
def test_draft_and_verify_words_equal_the_reference(S, k, V):
    n = _n()
    rng = np.random.default_rng(1000 * S + 10 * k + V % 7)
    st0 = _lookup_state(rng, S, k)
    dev = _dev(st0)
    args = lambda d: (d["hist"], d["hist_len"], d["ids"], d["pos"], d["ndraft"], d["cap"], d["len"], d["live"])
    n.lookup_draft_slots(*args(dev), S, k, 3)
    st1 = ref.draft_slots(st0, k, 3)
    _same(dev, st1)
    if S == 1:                                                        # ... and pc_lookup_draft's words, bit for bit
        one = _dev(st0)
        n.lookup_draft(one["hist"][0], one["hist_len"], one["ids"][0], one["pos"][0], one["ndraft"], k, 3)
        for name in ("hist", "hist_len", "ids", "pos", "ndraft"):
            assert torch.equal(one[name], dev[name]), name
    # the model agrees with the first acc_b drafts of slot b, then says its own tokens (the last columns)
    R = S * (k + 1)
    x = rng.standard_normal((R, V)).astype(np.float32)
    am = []
    for b in range(S):
        acc = (k, 0, 1, 2)[b % 4]
        for i in range(k + 1):
            agree = i < min(acc, k) and st1["ids"][b, 1 + i] >= 0      # (a slot that did not run has no drafts)
            a = int(st1["ids"][b, 1 + i]) if agree else V - 1 - (b * (k + 1) + i)
            x[b * (k + 1) + i, a] = 10.0
            am.append(a)
    if S > 1:
        # a stop id in the middle of an accepted run (slot 0: budget 40, the model agrees with every draft): row 1's token
        assert st1["ndraft"][0] == k
        st1["stop_ids"][0, 3] = am[min(1, k)]
        st1["stop_ids"][2, 0] = V - 1                                  # ... and one that does not occur
    dev = _dev(st1)
    amax = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    logits = torch.from_numpy(x).to(DEV)

    def launch(d):
        n.lookup_verify_slots(logits, V, V, S, k, amax, d["hist"], d["hist_len"], d["ids"], d["pos"], d["len"], d["cap"], d["live"],
                              d["ndraft"], d["budget"], d["stop_ids"], d["ring"], d["ctr"], RING_CAP)
    launch(dev)
    st2, want_am = ref.verify_slots(x, st1, k, RING_CAP)
    assert amax.tolist() == am == want_am.tolist()
    _same(dev, st2)
    if S > 1:
        rec = st2["ring"][0, int(st1["ctr"][0]) % RING_CAP]
        assert st2["live"][0] == 0 and rec[0] == min(2, k + 1) and rec[rec[0]] == st1["stop_ids"][0, 3]     # cut behind the stop id
        assert st2["live"][S - 1] == 0 and st2["len"][S - 1] == st1["len"][S - 1]                          # the too-full slot: off
    else:                                                             # pc_lookup_verify's words, bit for bit (len <-> past_len)
        one = _dev(st1)
        past = torch.tensor([int(st1["len"][0]), 17], dtype=torch.int32, device=DEV)
        n.lookup_verify(logits, V, V, k + 1, torch.zeros(16, dtype=torch.int32, device=DEV), one["hist"][0], one["hist_len"],
                        one["ids"][0], one["pos"][0], past, one["ndraft"], one["budget"], one["ring"].view(-1), one["ctr"], RING_CAP)
        for name in ("hist", "hist_len", "ids", "pos", "ndraft", "budget", "ring", "ctr"):
            assert torch.equal(one[name], dev[name]), name
        assert int(past[0]) == int(dev["len"][0])
    # a second launch: slots that went off leave empty records and nothing else
    launch(dev)
    st3, _ = ref.verify_slots(x, st2, k, RING_CAP)
    _same(dev, st3)


# ---- 2. pc_rope_append_slots_rows ---------------------------------------------------------------------------------------------
def _inv_freq(D):
    return (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))).to(DEV)


@pytest.mark.parametrize("H_,Hkv,D", [(4, 4, 128), (8, 2, 64)])
def test_rope_rows_equal_the_slot_entry_at_k0_and_successive_append_ex_calls(H_, Hkv, D):
    n = _n()
    rng = np.random.default_rng(D + H_)
    W = (H_ + 2 * Hkv) * D
    # k = 0: the bytes of pc_rope_append_slots (slot 4: len == cap, skipped by both)
    lens, caps = [10, 0, None, 33, 7], [40, 8, 16, 40, 7]
    res = []
    for rows_entry in (False, True):
        sl = Slots(np.random.default_rng(5), lens, caps, Hkv, D, L=2)
        S = sl.S
        qkv = torch.from_numpy(np.random.default_rng(6).standard_normal((S, W), dtype=np.float32)).to(DEV)
        cs = torch.empty((S, D // 2, 2), dtype=torch.float32, device=DEV)
        n.rope_table(_i32([5, 900, 3, 77, 2000]), _inv_freq(D), cs, S, D)
        qh = torch.full((S, H_ * D), SENT, dtype=torch.float16, device=DEV)
        ql = torch.full((S, H_ * D), SENT, dtype=torch.float16, device=DEV)
        if rows_entry:
            n.rope_append_slots_rows(qkv, W, 0, qh, ql, H_ * D, cs, sl.kv_base, sl.cap, sl.len, sl.livet, S, 0, 1, H_, Hkv, D)
        else:
            n.rope_append_slots(qkv, W, 0, qh, ql, H_ * D, cs, sl.kv_base, sl.cap, sl.len, sl.livet, S, 1, H_, Hkv, D)
        torch.cuda.synchronize()
        res.append([qh, ql] + sl.arenas)
    for x, y in zip(*res):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    # k = 3: k + 1 successive pc_rope_append_ex calls per slot; an idle slot and one without room for 4 rows are left alone
    k = 3
    lens, caps = [10, None, 0, 21], [20, 16, 4, 24]                   # slot 3: 21 + 4 > 24
    sl = Slots(rng, lens, caps, Hkv, D, L=3)
    twins = [a.clone() for a in sl.arenas]
    S, R = sl.S, sl.S * (k + 1)
    cs = torch.empty((R, D // 2, 2), dtype=torch.float32, device=DEV)
    n.rope_table(_i32(rng.integers(0, 3000, R)), _inv_freq(D), cs, R, D)
    for layer in range(3):
        qkv = torch.from_numpy(rng.standard_normal((R, W), dtype=np.float32)).to(DEV)
        qh = torch.full((R, H_ * D), SENT, dtype=torch.float16, device=DEV)
        ql = torch.full((R, H_ * D), SENT, dtype=torch.float16, device=DEV)
        n.rope_append_slots_rows(qkv, W, 0, qh, ql, H_ * D, cs, sl.kv_base, sl.cap, sl.len, sl.livet, S, k, layer, H_, Hkv, D)
        for b in (0, 2):
            for i in range(k + 1):
                r = b * (k + 1) + i
                qo, qol = _append_ex(n, qkv[r], cs[r], twins[b], layer, H_, Hkv, D, lens[b] + i, caps[b])
                assert torch.equal(qo[0].view(torch.int16), qh[r].view(torch.int16)), (layer, b, i)
                assert torch.equal(qol[0].view(torch.int16), ql[r].view(torch.int16)), (layer, b, i)
        for b in (1, 3):
            assert torch.all(qh[b * (k + 1):(b + 1) * (k + 1)] == SENT) and torch.all(ql[b * (k + 1):(b + 1) * (k + 1)] == SENT)
    torch.cuda.synchronize()
    for b in range(S):
        assert torch.equal(sl.arenas[b].view(torch.int16), twins[b].view(torch.int16)), b


# ---- 3. pc_attn_verify_slots ----------------------------------------------------------------------------------------------------
POISON = 1.0e4


def _verify_launch(n, sl, qkv, pos, H_, k, layer, nsplits):
    """pc_rope_append_slots_rows once, then pc_attn_verify_slots per split count -> (q_hi, q_lo, {nsplit: (out_hi, out_lo)})."""
    S, Hkv, D = sl.S, sl.Hkv, sl.D
    R = S * (k + 1)
    cs = torch.empty((R, D // 2, 2), dtype=torch.float32, device=DEV)
    n.rope_table(_i32(pos), _inv_freq(D), cs, R, D)
    qh = torch.full((R, H_ * D), SENT, dtype=torch.float16, device=DEV)
    ql = torch.full((R, H_ * D), SENT, dtype=torch.float16, device=DEV)
    n.rope_append_slots_rows(qkv, qkv.shape[1], 0, qh, ql, H_ * D, cs, sl.kv_base, sl.cap, sl.len, sl.livet, S, k, layer, H_, Hkv, D)
    outs = {}
    mt = (R + 15) // 16
    for ns in nsplits:
        ws = torch.empty(n.attn_verify_slots_workspace_bytes(S, k, H_, D, ns) // 4, dtype=torch.float32, device=DEV)
        out = (torch.full((mt, H_ * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
               torch.full((mt, H_ * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))
        n.attn_verify_slots(qh, ql, H_ * D, sl.kv_base, sl.cap, sl.len, sl.livet, S, k, layer, H_, Hkv, D, 1.0 / np.sqrt(D), ns, ws, out)
        outs[ns] = out
    torch.cuda.synchronize()
    return qh, ql, outs


@pytest.mark.parametrize("k", [1, 3, 15])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_verify_attention_against_the_reference(D, G, k):
    n = _n()
    Hkv, layer = 2, 1
    H_ = G * Hkv
    W = (H_ + 2 * Hkv) * D
    worst = 0.0
    # two launches of four slots (S * (k + 1) <= 64 at k = 15); None: idle; "full": live with len + k + 1 > cap
    for lens, full in (([0, 300, None, 64], None), ([1, 63, 65, 10], 3)):
        rng = np.random.default_rng(D + 10 * G + k + len(lens) + (full or 0))
        S = len(lens)
        caps = [(0 if m is None else m) + k + 1 + 2 + b for b, m in enumerate(lens)]
        if full is not None:
            caps[full] = lens[full] + k
        sl = Slots(rng, lens, caps, Hkv, D)
        for b, m in enumerate(lens):                          # everything behind the staged rows: poison no row may see
            sl.arenas[b][:, :, :, (m or 0):] = POISON
        before = [a.clone() for a in sl.arenas]
        R = S * (k + 1)
        qkv_np = rng.standard_normal((R, W), dtype=np.float32)
        qkv_np[:, H_ * D:(H_ + Hkv) * D] *= 0.7
        pos = [int(p) for p in rng.integers(0, 4000, R)]
        qh, ql, outs = _verify_launch(n, sl, torch.from_numpy(qkv_np).to(DEV), pos, H_, k, layer, (1, 4, 32))
        want = {}
        for ns, (oh, ol) in outs.items():
            got = (n.from_act_frags(oh, R).float() + n.from_act_frags(ol, R).float()).cpu().numpy()
            raw = n.from_act_frags(oh, R).cpu().numpy()
            for b, m in enumerate(lens):
                rows = slice(b * (k + 1), (b + 1) * (k + 1))
                a, a0 = sl.arenas[b], before[b]
                if m is None or b == full:
                    assert np.all(raw[rows] == SENT) and torch.all(qh[rows] == SENT), f"slot {b} does not run but was written"
                    assert torch.equal(a, a0)
                    continue
                keep = torch.ones_like(a, dtype=torch.bool)
                keep[layer, :, :, m:m + k + 1] = False
                assert torch.equal(a[keep], a0[keep]), f"slot {b}: bytes outside the appended rows changed"
                assert torch.all(a[layer, :, :, m + k + 1:] == POISON)          # (key len + k + 1 is poison: row k must not see it)
                if b not in want:
                    q = (qh[rows].float() + ql[rows].float()).cpu().numpy().reshape(k + 1, H_, D)
                    want[b] = ref.verify_attend(q, a[layer, 0].float().cpu().numpy(), a[layer, 1].float().cpu().numpy(), m, k)
                err = float(np.abs(got[rows].reshape(k + 1, H_, D) - want[b]).max())
                worst = max(worst, err)
                assert np.isfinite(got[rows]).all() and err < ATT_TOL, (ns, b, m, err)
    print(f"[verify attention D={D} G={G} k={k}] worst max|d| = {worst:.2e}")


# ---- 4. alone and in a crowd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H_,Hkv,D,k,nsplit,m", [(4, 4, 128, 3, 4, 300), (8, 2, 64, 3, 4, 65), (8, 1, 128, 7, 2, 129)])
def test_a_slot_alone_and_in_a_crowd_is_bit_identical(H_, Hkv, D, k, nsplit, m):
    n = _n()
    rng = np.random.default_rng(m + k)
    W = (H_ + 2 * Hkv) * D
    rows_qkv = rng.standard_normal((k + 1, W), dtype=np.float32)
    staged = rng.standard_normal((2, 2, Hkv, m, D), dtype=np.float32).astype(np.float16)
    pos_own = [1234 + i for i in range(k + 1)]
    res = []
    for S, slot, others in ((1, 0, []), (8, 5, [300, 1, None, 64, 77, 65, 120])):
        lens = list(others[:slot]) + [m] + list(others[slot:])
        caps = [(0 if x is None else x) + k + 4 + b for b, x in enumerate(lens)]
        caps[slot] = m + k + 5                                  # the sequence's own arena has the same shape in both runs
        sl = Slots(rng, lens, caps, Hkv, D)
        sl.arenas[slot][:, :, :, :m] = torch.from_numpy(staged).to(DEV)
        R = S * (k + 1)
        qkv = rng.standard_normal((R, W), dtype=np.float32)
        qkv[slot * (k + 1):(slot + 1) * (k + 1)] = rows_qkv
        pos = [int(p) for p in rng.integers(0, 4000, R)]
        pos[slot * (k + 1):(slot + 1) * (k + 1)] = pos_own
        qh, ql, outs = _verify_launch(n, sl, torch.from_numpy(qkv).to(DEV), pos, H_, k, 1, (nsplit,))
        oh, ol = outs[nsplit]
        rows = slice(slot * (k + 1), (slot + 1) * (k + 1))
        res.append((n.from_act_frags(oh, R)[rows].clone(), n.from_act_frags(ol, R)[rows].clone(), qh[rows].clone(), ql[rows].clone(),
                    sl.arenas[slot][1, :, :, m:m + k + 1].clone()))
    for x, y, what in zip(res[0], res[1], ("out hi", "out lo", "q hi", "q lo", "appended K / V rows")):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), what


# ---- 5. / 6. LookupSlotLoop -----------------------------------------------------------------------------------------------------
W_SCALE, CTX_LEN, N_NEW = 3.0, 40, 24
# Weight seeds chosen on the CPU beforehand, as tests/test_gpu_lookup.py's was: the oracle's own top-2 margin along its greedy
# answer is 0.064 (mid_gqa, that file's seed) and 0.065 (mid64; seeds 100..130 searched, 103 and 113 pass).  Re-checked in _greedy.
W_SEEDS = {"mid_gqa": 108, "mid64": 103}
_MODELS, _GREEDY = {}, {}


def _model(shape_name):
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    if shape_name not in _MODELS:
        shape, seed = SHAPES[shape_name], W_SEEDS[shape_name]
        w16 = make_weights_np(shape, seed, W_SCALE)
        lm = Llama2(name="lks", shape=shape, weights=w16, device=DEV)
        ctx = np.random.default_rng(seed).integers(3, shape.vocab_size, size=CTX_LEN).tolist()
        _MODELS[shape_name] = (lm, shape, w16, ctx)
    return _MODELS[shape_name]


@pytest.fixture(scope="module")
def gqa():
    return _model("mid_gqa")


def _prefill(lm, ctx):
    out = lm(input_ids=torch.tensor([ctx]), position_ids=torch.tensor([list(range(len(ctx)))]), use_cache=True)
    return out.past_key_values, int(out.logits[0, -1].argmax())


def _run_slots(lm, ctxs, corpora, k, max_new, slots=None, max_keys=None, extra=0, keep_logits=False):
    """One LookupSlotLoop generation of ``max_new`` tokens per sequence behind fresh prefills -> (first tokens, per-step token
    lists per sequence, loop, per-sequence logits rows of the emitted positions)."""
    from promptcache_amd.model.llama_hip import LookupSlotLoop
    pf = [_prefill(lm, c) for c in ctxs]
    firsts = [f for _, f in pf]
    loop = lm.hf_model.lookup_slot_loop([p for p, _ in pf], firsts, [len(c) for c in ctxs], max_new, k, corpora, slots=slots,
                                        max_keys=max_keys)
    assert isinstance(loop, LookupSlotLoop)
    n = len(ctxs)
    steps, rows, got = [], [[] for _ in range(n)], [0] * n
    while min(got) < max_new:
        i = loop.enqueue()
        rec = [loop.tokens(j, i) for j in range(n)]
        assert any(rec), "a step without any token before the budgets ran out"
        if keep_logits:
            for j in range(n):
                rows[j].append(loop.logits[j * (k + 1):j * (k + 1) + len(rec[j])].float().cpu().numpy())
        for j in range(n):
            got[j] += len(rec[j])
        steps.append(rec)
    for _ in range(extra):
        i = loop.enqueue()
        steps.append([loop.tokens(j, i) for j in range(n)])
    return firsts, steps, loop, rows


def _tokens(steps, j):
    return [t for s in steps for t in s[j]]


def _greedy(shape_name):
    """T: GreedyLoop's N_NEW tokens behind the first, and the oracle's logits / margin along them (teacher-forced)."""
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    if shape_name in _GREEDY:
        return _GREEDY[shape_name]
    lm, shape, w16, ctx = _model(shape_name)
    past, first = _prefill(lm, ctx)
    g = lm.hf_model.greedy_loop(past, first, len(ctx), N_NEW)
    T = [g.token(g.enqueue()) for _ in range(N_NEW)]
    g.close(N_NEW)
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=lm.hf_model.inv_freq_cpu.numpy())
    oracle = LlamaOracle(cfg, {n_: v.astype(np.float32) for n_, v in w16.items()})
    orows, margin = [], np.inf
    with H.oracle_blas():
        olog, present = oracle.forward(np.array([ctx]), np.arange(len(ctx))[None])
        assert int(np.argmax(olog[0, -1])) == first
        fed = first
        for i in range(N_NEW):                                  # the device leads: the oracle is fed the device's tokens
            olog, present = oracle.forward(np.array([[fed]]), np.array([[len(ctx) + i]]), past=present)
            top = np.sort(olog[0, -1])[-2:]
            margin = min(margin, float(top[1] - top[0]))
            orows.append(olog[0, -1].copy())
            fed = T[i]
    assert margin > 2e-2, margin                                # (re-checked on the inputs: twice the bar)
    _GREEDY[shape_name] = (first, T, np.stack(orows))
    return _GREEDY[shape_name]


@pytest.fixture(scope="module")
def greedy_run():
    return _greedy("mid_gqa")


def _corpora(ctx, first, T, vocab):
    full = ctx[-8:] + [first] + T                               # the context tail, then the answer itself: every draft is right
    wrong = list(full)
    for at in (8 + 1 + 6, 8 + 1 + 15):                          # two errors
        wrong[at] = (wrong[at] + 1) % vocab or 3
    return [], full, wrong


@pytest.mark.parametrize("n_seq,k", [(2, 3), (4, 7)])           # R = 8: the norm-folded step; R = 32: the generic launch sequence
@pytest.mark.parametrize("shape_name", ["mid_gqa", "mid64"])    # GQA 2:1 at D = 128, and MHA at D = 128: one row tile per head
def test_loop_tokens_counts_and_logits(shape_name, n_seq, k):
    lm, shape, w16, ctx = _model(shape_name)
    first, T, orows = _greedy(shape_name)
    empty, full, wrong = _corpora(ctx, first, T, shape.vocab_size)
    corpora = [empty, full, wrong, full][:n_seq]
    assert len(lr.simulate(full, first, T, k)) < len(T)         # (on the inputs: the full corpus actually saves steps)
    firsts, steps, loop, rows = _run_slots(lm, [ctx] * n_seq, corpora, k, N_NEW, keep_logits=True)
    loop.close([N_NEW] * n_seq)
    assert lm.hf_model._live_loop is None and all(a.length == CTX_LEN + N_NEW for a in loop.arenas)
    assert loop.S * (k + 1) == (8 if n_seq == 2 else 32)
    want_counts = ref.simulate_slots(corpora, [first] * n_seq, [T] * n_seq, k)
    assert [[len(r) for r in s] for s in steps] == want_counts
    worst = 0.0
    for j in range(n_seq):
        assert firsts[j] == first and _tokens(steps, j) == T, j                    # GreedyLoop's tokens
        dev_rows = np.concatenate(rows[j], axis=0)
        worst = max(worst, float(np.abs(dev_rows - orows).max()))
    print(f"[lookup slot loop {shape_name} S={loop.S} k={k}] logits vs oracle: max |d| = {worst:.2e}")
    assert worst < LOGIT_TOL
    # every sequence alone in a loop of the same slot count and max_keys: the same tokens at the same steps
    for j in range(n_seq):
        _, solo, sl, _ = _run_slots(lm, [ctx], [corpora[j]], k, N_NEW, slots=loop.S, max_keys=loop.max_keys)
        sl.close([N_NEW])
        assert [s[0] for s in solo] == [s[j] for s in steps][:len(solo)], j


def test_solo_equals_crowd_on_the_mha_shape():
    """mid64 (MHA, D = 128): sequences of different lengths together and alone -- the same tokens at the same steps."""
    lm, shape, w16, ctx = _model("mid64")
    ctxs = [ctx, ctx[:33], ctx[5:], ctx[:17]]
    for n_seq, k in ((2, 3), (4, 7)):
        firsts, steps, loop, _ = _run_slots(lm, ctxs[:n_seq], [c[-8:] for c in ctxs[:n_seq]], k, 12)
        loop.close([12] * n_seq)
        for j in range(n_seq):
            _, solo, sl, _ = _run_slots(lm, [ctxs[j]], [ctxs[j][-8:]], k, 12, slots=loop.S, max_keys=loop.max_keys)
            sl.close([12])
            assert [s[0] for s in solo] == [s[j] for s in steps][:len(solo)], (n_seq, k, j)


def test_budget_and_memory_safety_per_slot(gqa, greedy_run):
    lm, shape, w16, ctx = gqa
    m = lm.hf_model
    first, T, _ = greedy_run
    k, max_new = 3, 10
    ctxs = [ctx, ctx[:31]]                                      # different len0, one max_new
    pf = [_prefill(lm, c) for c in ctxs]
    corpora = [ctx[-8:] + [first] + T, []]
    loop = m.lookup_slot_loop([p for p, _ in pf], [f for _, f in pf], [len(c) for c in ctxs], max_new, k, corpora)
    los = [len(c) + max_new + k + 1 for c in ctxs]
    befores = []
    with torch.inference_mode():
        for a, lo in zip(loop.arenas, los):
            assert a.cap >= lo + 1
            a.buf[:, :, :, :, lo:] = 0.5
            befores.append(a.buf[:, :, :, :, lo:].clone())
    got, steps = [[], []], 0
    while min(map(len, got)) < max_new:
        i = loop.enqueue()
        for j in range(2):
            got[j] += loop.tokens(j, i)
        steps += 1
        assert steps <= max_new
    for _ in range(6):                                          # surplus replays: empty records, nothing written
        i = loop.enqueue()
        assert loop.tokens(0, i) == [] and loop.tokens(1, i) == []
    torch.cuda.synchronize()
    assert got[0] == T[:max_new] and len(got[1]) == max_new
    for a, lo, before in zip(loop.arenas, los, befores):
        assert torch.equal(a.buf[:, :, :, :, lo:], before)      # nothing behind the rows the budget allows
    consumed = [7, 4]
    loop.close(consumed)
    assert m._live_loop is None
    after = []
    for j, a in enumerate(loop.arenas):
        assert a.length == len(ctxs[j]) + consumed[j]
        nxt, p = got[j][consumed[j] - 1], len(ctxs[j]) + consumed[j]
        after.append(lm(input_ids=torch.tensor([[nxt]]), position_ids=torch.tensor([[p]]), past_key_values=a.views(),
                        use_cache=True).logits[0, -1].clone())
    # the same state behind a SlotLoop of the same tokens
    pf = [_prefill(lm, c) for c in ctxs]
    sl = m.slot_loop([p for p, _ in pf], [f for _, f in pf], [len(c) for c in ctxs], max_new)
    for i in range(max(consumed)):
        sl.enqueue()
        for j in range(2):
            if i < consumed[j]:
                assert sl.token(j, i) == got[j][i], (j, i)
    sl.close(consumed)
    for j, a in enumerate(sl.arenas):
        nxt, p = got[j][consumed[j] - 1], len(ctxs[j]) + consumed[j]
        want = lm(input_ids=torch.tensor([[nxt]]), position_ids=torch.tensor([[p]]), past_key_values=a.views(), use_cache=True).logits[0, -1]
        d = float((after[j] - want).abs().max())
        print(f"sequence {j}: logits behind a lookup slot loop vs behind a slot loop: max |d| = {d:.2e}")
        assert d < LOGIT_TOL


# ---- 7. GenerationEngine.generate_batch(lookup=k) ---------------------------------------------------------------------------------
def test_engine_batch_lookup_reproduces_the_golden_greedy_text():
    from promptcache_amd import GenerationEngine, GenerationParameters, Prompt
    from promptcache_amd.cache_engine import CacheEngine
    from promptcache_amd.model.llama_hip import LookupSlotLoop, SlotLoop
    from tests.test_gpu_engine import build_product
    g = H.load_case("mid_trip")
    lm, _ = build_product(g)
    eng = CacheEngine(int(g["max_ctx"]), lm, slots=3)
    mt = int(g["max_tokens"])
    eng.add_schema(lm.get_formatter()(str(g["schema_text"])), max_tokens=None if mt < 0 else mt)
    prompt = Prompt(str(g["prompt_text"]), [lm.get_formatter()])
    want = lm.decode(g["greedy"].tolist())
    ge = GenerationEngine(lm, lookup=7)                     # (the engine-level lookup is not consulted by generate_batch)
    m = lm.hf_model

    def run(lookup, params, nreq=3):
        reqs = [eng.process(prompt, slot=j) for j in range(nreq)]
        kinds, outs = set(), {j: [] for j in range(nreq)}
        for j, o in ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, stream_interval=1, lookup=lookup):
            outs[j].append(o)
            if m._live_loop is not None:
                kinds.add(type(m._live_loop))
        assert m._live_loop is None
        return outs, kinds

    greedy = GenerationParameters(temperature=0.0, max_new_tokens=len(g["greedy"]), stop_token_ids=[], stop_str=[])
    keys0 = set(m._graphs)
    outs0, kinds = run(None, greedy)                        # (PC_SLOT_LOOKUP unset: off)
    assert kinds == {SlotLoop} and all(outs0[j][-1].new_text == want for j in outs0)
    assert not any(isinstance(key, tuple) and key[:2] == ("slots", "lookup") for key in m._graphs)      # off: no lookup graph
    keys_off = set(m._graphs) - keys0
    outs, kinds = run(3, greedy)
    assert kinds == {LookupSlotLoop}
    for j in outs:
        assert outs[j][-1].new_text == want, j
        assert [o.new_text for o in outs[j]] == [o.new_text for o in outs0[j]], j       # one Output per token, as without lookup
    assert any(isinstance(key, tuple) and key[:2] == ("slots", "lookup") for key in m._graphs)
    assert keys_off <= set(m._graphs)
    # a stop id in the middle of the answer
    stop = int(g["greedy"][2])
    cut = g["greedy"].tolist().index(stop)
    outs, _ = run(3, GenerationParameters(temperature=0.0, max_new_tokens=len(g["greedy"]), stop_token_ids=[stop], stop_str=[]))
    assert all(outs[j][-1].new_text == lm.decode(g["greedy"].tolist()[:cut + 1]) for j in outs)
    # ... and as the ninth stop id, behind eight that never occur: batch_plan runs the sequences one after another, as without lookup
    never = [t for t in range(3, 40) if t not in set(g["greedy"].tolist())][:8]
    outs, kinds = run(3, GenerationParameters(temperature=0.0, max_new_tokens=len(g["greedy"]), stop_token_ids=never + [stop], stop_str=[]))
    assert LookupSlotLoop not in kinds and SlotLoop not in kinds and len(never) == 8
    assert all(outs[j][-1].new_text == lm.decode(g["greedy"].tolist()[:cut + 1]) for j in outs)
    sampled = GenerationParameters(temperature=0.8, top_p=0.9, max_new_tokens=6, stop_token_ids=[], stop_str=[])
    _, kinds = run(3, sampled)
    assert kinds == {SlotLoop}
    with pytest.raises(ValueError):
        next(ge.generate_batch([], greedy, lookup=3, share_trunk=True))
