"""Prompt-lookup drafts under continuous batching on the GPU: pc_lookup_verify_slots_each bit for bit against the three
entries it generalises and word for word against tests/lookup_serve_ref.py, pc_lookup_slot_arm word for word and in stream order,
``LookupSlotLoop(each=True)`` against the numpy oracle for a sequence admitted at a later replay, and
``GenerationEngine.serve(lookup=k)`` end to end -- every request against a solo run of the same prefill, against plain ``serve``
where the oracle's margin decides, with shared trunks, abandoned, and where today's path must run."""
import numpy as np
import pytest
import torch

from tests import lookup_sample_ref as lsr
from tests import lookup_serve_ref as ref
from tests import lookup_slots_ref as lsl
from tests import sample_ref as sr
from tests.test_gpu_lookup_slots import HIST_CAP, RING_CAP, _dev, _lookup_state
from tests.test_gpu_slots import LOGIT_TOL, PICKS, _collect, _n

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PICKS7 = PICKS + [((0, 0), 6), ((2, 2), 9), ((0, 2), 4)]
MAX_NEW7 = [5, 12, 20, 9, 16, 7, 11]


def _params_each(n, params):
    blk = b"".join(n.sample_params_bytes(T, rp, tp, tk if tk > 0 else -1, 0) for T, rp, tp, tk in params)
    return torch.frombuffer(bytearray(blk), dtype=torch.uint8).to(DEV)


def _each_words(n, st, V, params, seeds, draws=None, bits=None):
    """Device copies of the numpy state ``st`` plus the per-slot sampling words and dirty scratch."""
    S, k = st["ids"].shape[0], st["ids"].shape[1] - 1
    hw = (V + 31) // 32
    d = _dev({name: (v.view(np.int32) if v.dtype == np.uint32 else v) for name, v in st.items()})
    if "bits" not in d:
        d["bits"] = torch.from_numpy(np.zeros((S, hw), np.int32) if bits is None else np.asarray(bits).view(np.int32).copy()).to(DEV)
        d["draws"] = torch.tensor([1] * S if draws is None else list(draws), dtype=torch.int32, device=DEV)
    d["params"] = _params_each(n, params)
    d["seeds"] = torch.tensor([int(s) for s in seeds], dtype=torch.int64, device=DEV)
    d["row_bits"] = torch.full((S * (k + 1) * hw,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)      # scratch arrives dirty
    d["row_token"] = torch.full((S * (k + 1),), -1, dtype=torch.int32, device=DEV)
    return d


def _verify_each(n, logits, ldl, V, d, ring_cap):
    S, k = d["ids"].shape[0], d["ids"].shape[1] - 1
    n.lookup_verify_slots_each(logits, ldl, V, S, k, d["params"], d["seeds"], d["bits"], d["row_bits"], d["draws"], d["row_token"],
                               d["hist"], d["hist_len"], d["ids"], d["pos"], d["len"], d["cap"], d["live"], d["ndraft"], d["budget"],
                               d["stop_ids"], d["ring"], d["ctr"], ring_cap)


SLOT_WORDS = ("hist", "hist_len", "ids", "pos", "ndraft", "budget", "stop_ids", "ring", "ctr", "len", "cap", "live")


# ---- 1. bit identity: every output word ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1001, 32000])
@pytest.mark.parametrize("S,k", [(1, 1), (1, 3), (1, 15), (4, 1), (4, 3), (4, 15)])         # (4, 15): the 64-row limit
def test_greedy_blocks_are_lookup_verify_slots(S, k, V):
    """Every block plain greedy (rp = 1): the words of pc_lookup_verify_slots, over two launches (tests/test_gpu_lookup_slots'
    state: an idle slot, one without room, budgets 0 / 1 / 3 / 40, a stop id in the middle of an accepted run)."""
    n = _n()
    rng = np.random.default_rng(100 * S + k + V % 5)
    st1 = lsl.draft_slots(_lookup_state(rng, S, k), k, 3)
    R = S * (k + 1)
    x = rng.standard_normal((R, V)).astype(np.float32)
    am = []
    for b in range(S):
        acc = (k, 0, 1, 2)[b % 4]
        for i in range(k + 1):
            agree = i < min(acc, k) and st1["ids"][b, 1 + i] >= 0
            a = int(st1["ids"][b, 1 + i]) if agree else V - 1 - (b * (k + 1) + i)
            x[b * (k + 1) + i, a] = 10.0
            am.append(a)
    if S > 1:
        assert st1["ndraft"][0] == k
        st1["stop_ids"][0, 3] = am[min(1, k)]
    buf = torch.full((R, V + 4), 7.0, dtype=torch.float32, device=DEV)                      # (row stride V + 4)
    logits = buf[:, :V]
    logits.copy_(torch.from_numpy(x))
    a, b_ = _dev(st1), _each_words(n, st1, V, [ref.GREEDY] * S, [0] * S)
    amax = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    for launch in range(2):
        n.lookup_verify_slots(logits, V + 4, V, S, k, amax, a["hist"], a["hist_len"], a["ids"], a["pos"], a["len"], a["cap"], a["live"],
                              a["ndraft"], a["budget"], a["stop_ids"], a["ring"], a["ctr"], RING_CAP)
        before = b_["draws"].clone()
        _verify_each(n, logits, V + 4, V, b_, RING_CAP)
        torch.cuda.synchronize()
        for name in SLOT_WORDS:
            assert torch.equal(a[name], b_[name]), (launch, name)
        for b in range(S):
            rec = a["ring"][b, (int(st1["ctr"][b]) + launch) % RING_CAP]
            assert int(b_["draws"][b]) - int(before[b]) == int(rec[0]), (launch, b)           # draws += emit
    want_bits = [set() for _ in range(S)]
    got = a["ring"].cpu().numpy()
    for b in range(S):
        for c in range(2):
            rec = got[b, (int(st1["ctr"][b]) + c) % RING_CAP]
            want_bits[b] |= set(int(t) for t in rec[1:1 + rec[0]])
        assert lsr.bits_ids(b_["bits"][b].cpu().numpy().view(np.uint32), V) == sorted(want_bits[b]), b


@pytest.mark.parametrize("V", [1001, 32000])
def test_one_sampled_slot_is_lookup_verify_sample(V):
    """S = 1, no stop ids: every word of pc_lookup_verify_sample (len <-> past_len), accepted drafts and a wrong one included."""
    n = _n()
    k, params, seed, d0 = 3, ref.SAMPLED, 77123, 6
    rng = np.random.default_rng(V + 1)
    x = (rng.standard_normal((k + 1, V)) * 2.0).astype(np.float32)
    base = [int(t) for t in rng.integers(0, V, 30)]
    st = ref.new_state(1, k, V, HIST_CAP, RING_CAP)
    st["hist"][0, :5], st["hist_len"][0] = [9, 8, 7, 6, base[-1]], 5
    st["ids"][0, 0], st["pos"][0] = base[-1], 100 + np.arange(k + 1)
    st["cap"][0], st["len"][0], st["live"][0], st["budget"][0], st["ctr"][0], st["draws"][0] = 900, 60, 1, 9, 2, d0
    st["bits"][0] = lsr.history_bits(base, V)
    st["ring"][:] = -5
    drafts = []
    for i in range(k):                                                   # two right drafts, then a wrong one
        tok, _, _ = lsr.draw(x[i], base + drafts, params, seed, d0 + i)
        drafts.append(int(tok) if i < 2 else (int(tok) + 1) % V)
    st["ids"][0, 1:], st["ndraft"][0] = drafts, k
    logits = torch.from_numpy(x).to(DEV)
    for budget in (9, 2):
        st["budget"][0] = budget
        d = _each_words(n, st, V, [params], [seed])
        one = _each_words(n, st, V, [params], [seed])
        _verify_each(n, logits, V, V, d, RING_CAP)
        pd = torch.frombuffer(bytearray(n.sample_params_bytes(*params, seed)), dtype=torch.uint8).to(DEV)
        past = torch.tensor([60, 17], dtype=torch.int32, device=DEV)
        n.lookup_verify_sample(logits, V, V, k + 1, pd, one["bits"][0], one["row_bits"], one["draws"], one["row_token"], one["hist"][0],
                               one["hist_len"], one["ids"][0], one["pos"][0], past, one["ndraft"], one["budget"], one["ring"].view(-1),
                               one["ctr"], RING_CAP)
        torch.cuda.synchronize()
        for name in ("hist", "hist_len", "ids", "pos", "ndraft", "budget", "ring", "ctr", "draws", "bits"):
            assert torch.equal(d[name], one[name]), (budget, name)
        assert int(past[0]) == int(d["len"][0]) and int(d["ring"][0, 2, 0]) == min(3, budget) and int(d["live"][0]) == int(budget > 3)
        assert d["row_token"][:3].tolist() == one["row_token"][:3].tolist()


def test_without_drafts_it_is_advance_slots_each():
    """ndraft = 0 everywhere, caps far away: token, ids[.][0], pos, len, budget, draws and bitmap of pc_sample_advance_slots_each at
    equal draws, over three steps with mixed blocks, an idle slot and a stop id."""
    n = _n()
    S, k, V = 4, 3, 32000
    params = [ref.GREEDY, ref.SAMPLED, ref.WIDE, ref.GREEDY_RP]
    rng = np.random.default_rng(3)
    seeds = [int(s) for s in rng.integers(0, 2 ** 62, S)]
    st = ref.new_state(S, k, V, HIST_CAP, 16)
    hists = [[int(t) for t in rng.integers(0, V, 30)] for _ in range(S)]
    for b in range(S):
        st["bits"][b] = lsr.history_bits(hists[b], V)
    st["ids"][:], st["pos"][:, 0], st["hist_len"][:] = 5, 100, 1
    st["cap"][:], st["len"][:], st["live"][:], st["budget"][:], st["draws"][:] = 5000, [50, 53, 56, 59], [1, 1, 0, 1], 3, [4, 9, 1, 2]
    d = _each_words(n, st, V, params, seeds)
    e = dict(ids=d["ids"][:, 0].clone(), pos=d["pos"][:, 0].clone(), len=d["len"].clone(), live=d["live"].clone(), budget=d["budget"].clone(),
             draws=d["draws"].clone(), bits=d["bits"].clone(), ctr=torch.zeros(S, dtype=torch.int32, device=DEV),
             ring=torch.full((S * 16,), -1, dtype=torch.int32, device=DEV))
    for step in range(3):
        x = torch.from_numpy((rng.standard_normal((S * (k + 1), V)) * 2.0).astype(np.float32)).to(DEV)
        if step == 1:                                                    # slot 3's token of this step becomes a stop id of both
            x[3 * (k + 1), 4242] = 60.0
            d["stop_ids"][3, 2] = 4242
        _verify_each(n, x, V, V, d, 16)
        n.sample_advance_slots_each(x.view(S, (k + 1) * V), (k + 1) * V, V, d["params"], d["seeds"], e["bits"], e["ids"], e["pos"], e["len"],
                                    d["cap"], e["live"], e["budget"], d["stop_ids"], e["ring"], e["ctr"], e["draws"], 16, S)
        torch.cuda.synchronize()
        for b in range(S):
            rec = d["ring"][b, step]
            if int(e["ring"][b * 16 + step]) < 0:
                assert int(rec[0]) == 0, (step, b)                       # idle / stopped: an empty record there, nothing here
            else:
                assert rec[:2].tolist() == [1, int(e["ring"][b * 16 + step])], (step, b)
        assert torch.equal(d["ids"][:, 0], e["ids"]) and torch.equal(d["pos"][:, 0], e["pos"]), step
        for name in ("len", "budget", "draws", "bits", "live"):
            assert torch.equal(d[name], e[name]), (step, name)
    assert d["live"].tolist() == [0, 0, 0, 0] and int(d["len"][3]) == 61 and d["budget"].tolist() == [0, 0, 3, 1]


# ---- 2. against the numpy reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1001, 32000])
def test_mixed_blocks_equal_the_reference(V):
    """tests/lookup_serve_ref.each_case: mixed blocks, an idle slot, a live slot without room, a budget that cuts a step, a stop id
    in the middle of an accepted run; every state word and ring record after each of two steps.  A row whose float64 score margin
    in the reference is at most 1e-4 is followed on the device's token (tests/test_gpu_serve.py's rule); the rng seeds were
    checked on the CPU (test_lookup_serve_cpu.test_each_case_seeds_leave_three_quarters_comparable)."""
    n = _n()
    S, k = ref.EACH_S, ref.EACH_K
    st, seeds, logits = ref.each_case(V)
    pairs = checked = 0
    dev = None
    for step in range(ref.EACH_STEPS):
        ref.each_drafts(st, logits[step], seeds, ref.EACH_PLAN[step])
        if dev is None:
            dev = _each_words(n, st, V, ref.EACH_PARAMS, seeds)
        else:                                                            # (the draft stage's words of this step)
            for name in ("ids", "pos", "ndraft", "stop_ids"):
                dev[name].copy_(torch.from_numpy(st[name]))
        buf = torch.full((S * (k + 1), V + 4), 7.0, dtype=torch.float32, device=DEV)
        x = buf[:, :V]
        x.copy_(torch.from_numpy(logits[step]))
        _verify_each(n, x, V + 4, V, dev, ref.EACH_RING)
        torch.cuda.synchronize()
        row_token = dev["row_token"].cpu().numpy()
        want, infos = ref.verify_slots_each(logits[step], st, k, ref.EACH_RING, ref.EACH_PARAMS, seeds)
        force = {}
        for b, info in enumerate(infos):
            if info is None:
                assert np.all(row_token[b * (k + 1):(b + 1) * (k + 1)] == -1), (step, b)          # nothing was drawn for it
                continue
            for i, (tok, margin) in enumerate(zip(info["tokens"], info["margins"])):
                got = int(row_token[b * (k + 1) + i])
                sampled = ref.EACH_PARAMS[b] != ref.GREEDY
                pairs += sampled
                if margin > ref.MARGIN:
                    assert got == tok, (step, b, i, got, tok, margin)
                    checked += sampled
                elif got != tok:
                    force[(b, i)] = got
            assert np.all(row_token[b * (k + 1) + len(info["tokens"]):(b + 1) * (k + 1)] == -1), (step, b)   # pad rows are not drawn
        if force:
            want, infos = ref.verify_slots_each(logits[step], st, k, ref.EACH_RING, ref.EACH_PARAMS, seeds, force=force)
        for name in SLOT_WORDS + ("draws",):
            assert np.array_equal(dev[name].cpu().numpy(), want[name]), (step, name, dev[name].cpu().numpy(), want[name])
        assert np.array_equal(dev["bits"].cpu().numpy().view(np.uint32), want["bits"]), step
        if step == 0 and not force:
            rec = want["ring"][:, ref.EACH_CTR % ref.EACH_RING]
            assert rec[0, 0] == 2 and rec[0, 2] == want["stop_ids"][0, 1] and want["live"][0] == 0            # cut behind the stop id
            assert rec[4, 0] == 2 and want["budget"][4] == 0 and want["live"][4] == 0 and want["draws"][4] == ref.EACH_DRAWS[4] + 2
            assert rec[2, 0] == 0 and rec[3, 0] == 0 and want["live"][3] == 0 and want["len"][3] == ref.EACH_LENS[3]
            assert rec[1, 0] == 4 and rec[5, 0] == 2
        st = want
        dev["row_token"].fill_(-1)
    print(f"[verify_slots_each V={V}] sampled (slot, row) pairs {pairs}, compared outright {checked}")
    assert pairs == 18 and 4 * checked >= 3 * pairs, (checked, pairs)


# ---- 3. pc_lookup_slot_arm -------------------------------------------------------------------------------------------------------
def _sentinel_state(n, S, k, V, hist_cap):
    hw = (V + 31) // 32
    t = lambda dt, v, shape=(S,): torch.full(shape, v, dtype=dt, device=DEV)
    st = dict(kv_base=t(torch.int64, 111), cap=t(torch.int32, 112), len=t(torch.int32, 113), live=t(torch.int32, 0),
              leader=t(torch.int32, 117), trunk=t(torch.int32, 118), ids=t(torch.int64, 115, (S, k + 1)), pos=t(torch.int32, 114, (S, k + 1)),
              ndraft=t(torch.int32, 116), budget=t(torch.int32, 119), hist_len=t(torch.int32, 125), ctr=t(torch.int32, 120),
              draws=t(torch.int32, 121), seeds=t(torch.int64, 122), params=t(torch.uint8, 0x5a, (S * 24,)),
              stop_ids=t(torch.int32, 124, (S, 8)), bits=t(torch.int32, 0x5b5b5b5b, (S, hw)), hist=t(torch.int32, 126, (S, hist_cap)))
    handle = n.lookup_slot_state(st["kv_base"], st["cap"], st["len"], st["live"], st["leader"], st["trunk"], st["ids"], st["pos"],
                                 st["ndraft"], st["budget"], st["hist_len"], st["ctr"], st["draws"], st["seeds"], st["params"],
                                 st["stop_ids"], st["bits"], st["hist"])
    return st, handle


def _pinned(raw):
    host = torch.zeros(len(raw), dtype=torch.uint8, pin_memory=True)
    host.copy_(torch.frombuffer(raw, dtype=torch.uint8))
    return host


def test_lookup_slot_arm_writes_one_slot_and_orders_behind_enqueued_steps():
    """tests/test_gpu_serve.test_slot_arm_writes_one_slot_and_orders_behind_enqueued_steps' method on the lookup step's words."""
    n = _n()
    S, k, V, hist_cap = 4, 3, 1001, 40
    hw = (V + 31) // 32
    rng = np.random.default_rng(2)
    st, handle = _sentinel_state(n, S, k, V, hist_cap)
    before = {name: v.cpu().clone() for name, v in st.items()}
    arena = torch.zeros(8, dtype=torch.float16, device=DEV)
    bit_ids = sorted(set(int(t) for t in rng.integers(0, V, 40)))
    bits = lsr.history_bits(bit_ids, V)
    hist_ids = [int(t) for t in rng.integers(0, V, 13)]                  # (an odd count: the last 64-bit word is half used)
    seed = int(rng.integers(0, 2 ** 62))
    f = dict(slot=2, cap=900, kv_base=arena.data_ptr(), len=40, pos=77, id=hist_ids[-1], leader=-1, trunk=0, budget=3, counter=12,
             seed=seed, params=ref.SAMPLED, stop_ids=[5, 6, 7], bits=bits)
    host = _pinned(ref.lookup_arm_block_bytes(n, hw, hist_ids, **f))
    n.lookup_slot_arm(host, n.lookup_slot_arm_bytes(hw, len(hist_ids)), handle, S, k, hist_cap)
    torch.cuda.synchronize()
    after = {name: v.cpu().clone() for name, v in st.items()}
    want2 = dict(kv_base=arena.data_ptr(), cap=900, len=40, live=1, leader=-1, trunk=0, ndraft=0, budget=3, hist_len=13, ctr=12, draws=1,
                 seeds=seed)
    for name, v in want2.items():
        assert int(after[name][2]) == v, name
    assert after["ids"][2].tolist() == [hist_ids[-1], 115, 115, 115] and after["pos"][2].tolist() == [77, 114, 114, 114]
    assert bytes(after["params"][48:72].numpy()) == n.sample_params_bytes(*ref.SAMPLED, 0)
    assert after["stop_ids"][2].tolist() == [5, 6, 7, -1, -1, -1, -1, -1]
    assert np.array_equal(after["bits"][2].numpy().view(np.uint32), bits)
    assert after["hist"][2].tolist() == hist_ids + [126] * (hist_cap - 13)                      # the first hist_len ids, no more
    for name in st:                                                     # every word of every other slot is unchanged
        keep = [b for b in range(S) if b != 2]
        assert torch.equal(after[name].view(S, -1)[keep], before[name].view(S, -1)[keep]), name
    # one verify step moves slot 2 as the reference says (the other slots are idle: empty records)
    x = (rng.standard_normal((S * (k + 1), V)) * 2.0).astype(np.float32)
    logits = torch.from_numpy(x).to(DEV)
    ring = torch.full((S, 16, k + 2), -1, dtype=torch.int32, device=DEV)
    row_bits = torch.zeros(S * (k + 1) * hw, dtype=torch.int32, device=DEV)
    row_token = torch.zeros(S * (k + 1), dtype=torch.int32, device=DEV)

    def step():
        n.lookup_verify_slots_each(logits, V, V, S, k, st["params"], st["seeds"], st["bits"], row_bits, st["draws"], row_token, st["hist"],
                                   st["hist_len"], st["ids"], st["pos"], st["len"], st["cap"], st["live"], st["ndraft"], st["budget"],
                                   st["stop_ids"], ring, st["ctr"], 16)
    step()
    torch.cuda.synchronize()
    tok, margin, _ = lsr.draw(x[2 * (k + 1)], bit_ids, ref.SAMPLED, seed, 1)
    assert margin > ref.MARGIN, "pick another rng seed: the reference's draw is a near-tie"
    assert ring[2, 12].tolist()[:2] == [1, tok] and int(st["ids"][2, 0]) == tok and int(st["pos"][2, 0]) == 78
    assert [int(st[w][2]) for w in ("len", "live", "budget", "ctr", "draws", "hist_len")] == [41, 1, 2, 13, 2, 14]
    assert int(st["hist"][2, 13]) == tok and int(st["ctr"][3]) == 121 and int(st["pos"][0, 0]) == 114
    # arm slot 1 BEHIND an enqueued step on the same stream: that step saw the old words (idle), the next one sees the new
    f1 = dict(f, slot=1, pos=500, len=10, id=3, counter=122, params=ref.GREEDY, stop_ids=[], bits=np.zeros(hw, dtype=np.uint32))
    host1 = _pinned(ref.lookup_arm_block_bytes(n, hw, [8, 3], **f1))
    snap = torch.empty(2, dtype=torch.int32, device=DEV)
    step()
    snap.copy_(torch.stack([st["pos"][1, 0], st["live"][1]]))            # (on the stream, between the step and the arm launch)
    n.lookup_slot_arm(host1, n.lookup_slot_arm_bytes(hw, 2), handle, S, k, hist_cap)
    step()
    torch.cuda.synchronize()
    top = int(np.argmax(x[1 * (k + 1)]))
    assert snap.cpu().tolist() == [114, 0]
    assert int(st["pos"][1, 0]) == 501 and int(st["len"][1]) == 11 and int(st["ids"][1, 0]) == top and int(st["live"][1]) == 1
    assert ring[1, 122 % 16].tolist()[:2] == [1, top] and st["hist"][1, :3].tolist() == [8, 3, top]
    with pytest.raises(RuntimeError):                                    # a history longer than the buffer is refused on the host
        n.lookup_slot_arm(_pinned(ref.lookup_arm_block_bytes(n, hw, list(range(41)), **f1)), n.lookup_slot_arm_bytes(hw, 41), handle, S, k,
                          hist_cap)


# ---- 4. / 5. the model: admission, serve(lookup=k) --------------------------------------------------------------------------------
W_SEED, W_SCALE = 9, 2.0
_SETUP = {}


def _gqa_setup(slots):
    """tests/test_gpu_slots._mid_setup on the ``mid_gqa`` shape (GQA 2:1, D = 128), one model for the module."""
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    if "lm" not in _SETUP:
        shape = SHAPES["mid_gqa"]
        w16 = make_weights_np(shape, W_SEED, W_SCALE)
        _SETUP.update(shape=shape, w16=w16, lm=Llama2(name=shape.name, shape=shape, weights=w16, device=DEV))
    shape, w16, lm = _SETUP["shape"], _SETUP["w16"], _SETUP["lm"]
    traits = (("age", (30, 26, 33)), ("home", (41, 37, 44)))
    eng = CacheEngine(2048, lm, slots=slots)
    prompts = []
    for pick, qlen in PICKS7:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=traits, question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    eng.add_schema(lm.get_formatter()(sp))
    return shape, w16, lm, eng, prompts


def _oracle(shape, w16, m, eng):
    from oracle import engine_oracle as eo
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    model = LlamaOracle(cfg, {name: v.astype(np.float32) for name, v in w16.items()})
    sc = eng.get_schema("deep")
    jobs = []
    for p in sc.encode_paths():
        sf = sc.get_scaffold(p)
        jobs.append(dict(token_ids=sf.token_ids(), position_ids=sf.position_ids(), targets=sf.select(p).all_token_sequences()))
    return model, eo.encode_schema(model, jobs)


def _requests(prompts):
    """7 requests of 5..20 tokens: plain greedy, two sampled chains and greedy with a penalty in turn."""
    from promptcache_amd.generation_engine import GenerationParameters as G
    kinds = [dict(temperature=0.0), dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40), dict(temperature=0.0),
             dict(temperature=1.3, repetition_penalty=1.3, top_p=0.8, top_k=12), dict(temperature=0.0, repetition_penalty=1.2),
             dict(temperature=0.0), dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40)]
    return [(p, G(max_new_tokens=mn, **kw)) for p, mn, kw in zip(prompts, MAX_NEW7, kinds)]


def _lookup_snapshots(monkeypatch, m):
    """tests/test_gpu_serve._snapshots for the lookup loop: at every entry of a sequence, a byte copy of its arena rows and what the
    loop was told."""
    from promptcache_amd.model.llama_hip import LookupSlotLoop
    snaps, loops, retired = [], [], []

    def take(past, token, position, max_new, params, seed, history, stop_ids, corpus):
        a = past.arena
        snaps.append(dict(rows=a.buf[:, :, :, :, :a.length].clone(), n0=a.length, token=int(token), position=int(position),
                          max_new=int(max_new), params=params, seed=int(seed), history=list(history), stop_ids=list(stop_ids),
                          corpus=list(corpus)))
    real_loop, real_admit, real_retire = m.lookup_slot_loop, LookupSlotLoop.admit, LookupSlotLoop.retire

    def lookup_slot_loop(pasts, tokens, positions, max_new, k, corpora, **kw):
        for j in range(len(pasts)):
            take(pasts[j], tokens[j], positions[j], max_new[j], kw["params"][j], kw["seeds"][j], kw["histories"][j], kw["stop_ids"][j],
                 corpora[j])
        loop = real_loop(pasts, tokens, positions, max_new, k, corpora, **kw)
        loops.append(loop)
        return loop

    def admit(self, slot_index, past, token, position, max_new, params, seed, history, stop_ids, corpus, trunk=None):
        take(past, token, position, max_new, params, seed, history, stop_ids, corpus)
        return real_admit(self, slot_index, past, token, position, max_new, params, seed, history, stop_ids, corpus, trunk=trunk)

    def retire(self, j, consumed):
        real_retire(self, j, consumed)
        retired.append((j, self.arenas[j].length, self.len0[j], consumed))
    monkeypatch.setattr(m, "lookup_slot_loop", lookup_slot_loop)
    monkeypatch.setattr(LookupSlotLoop, "admit", admit)
    monkeypatch.setattr(LookupSlotLoop, "retire", retire)
    return snaps, loops, retired


def _solo(m, eng, snap, slots, k, max_keys, hist_cap):
    """The sequence of ``snap`` alone in an each=True lookup loop, from the byte copy of its prefill (in slot 0's staged buffer)."""
    a = eng.slot_cache(0).arena
    a.pending = None
    a.buf[:, :, :, :, :snap["n0"]].copy_(snap["rows"])
    a.length = snap["n0"]
    loop = m.lookup_slot_loop([a.views(snap["n0"])], [snap["token"]], [snap["position"]], snap["max_new"], k, [snap["corpus"]],
                              stop_ids=snap["stop_ids"], slots=slots, max_keys=max_keys, each=True, params=snap["params"],
                              seeds=[snap["seed"]], histories=[snap["history"]], hist_cap=hist_cap)
    toks = [snap["token"]]
    try:
        while len(toks) - 1 < snap["max_new"]:
            got = loop.tokens(0, loop.enqueue())
            if not got:
                break
            toks += got
    finally:
        loop.close({0: len(toks) - 1})
    return toks


@pytest.fixture(scope="module")
def plain_run():
    """Plain ``serve`` over the 7 requests (4 slots, a lazy iterator, seed 5) and the oracle's margins along its tokens: per request
    (tokens, comparable prefix length) -- the leading tokens at which the oracle's own decision, fed the device's tokens, is no
    near-tie: top-2 margin above 2 * 1e-2 for a greedy request, score margin above 2 * 1e-2 / T for a sampled one (DESIGN 3.19 /
    3.21) and the oracle's token the device's."""
    from oracle import engine_oracle as eo
    from promptcache_amd.generation_engine import GenerationEngine
    shape, w16, lm, eng, prompts = _gqa_setup(4)
    ge = GenerationEngine(lm)
    reqs = _requests(prompts)
    torch.manual_seed(5)
    seed0 = int(torch.randint(0, 2 ** 62, (1,)))
    torch.manual_seed(5)
    _collect(ge.serve(eng, iter(reqs), lookup=0))
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert [len(tokens[r]) for r in range(7)] == MAX_NEW7 and sorted(ge.last_serve_stats) == ["live_rows", "replays", "requests", "rows"]
    model, lib = _oracle(shape, w16, lm.hf_model, eng)
    sure = {}
    for r, (prompt, p) in enumerate(reqs):
        ids, pos, _, cache = eng.process(prompt, slot=0)
        used = [mm.token_sequence for mm in eng.slot_cache(0).staged]
        _, S0, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        prm = (p.temperature, p.repetition_penalty, p.top_p, p.top_k)
        bar = 2 * LOGIT_TOL if p.greedy else 2 * LOGIT_TOL / p.temperature
        hist, n_sure, position = list(ids), 0, max(pos) + 2
        for j, tok in enumerate(tokens[r]):
            row = olog[0, -1]
            otok, margin, _ = sr.draw(row, hist, *prm, seed0 + r, j)
            if otok != tok or margin <= bar:
                break
            n_sure += 1
            hist.append(tok)
            olog, present = model.forward(np.array([[tok]]), np.array([[position + j]]), past=present)
        sure[r] = n_sure
    print(f"[plain serve] tokens {MAX_NEW7}, comparable prefixes {[sure[r] for r in range(7)]}")
    return tokens, sure


@pytest.mark.parametrize("k", [3, 7])                                    # 16 rows: the <= 16-row projections; 32: the 17..64-row sequence
def test_serve_with_lookup_equals_solo_runs_and_plain_serve(monkeypatch, plain_run, k):
    from promptcache_amd.generation_engine import GenerationEngine
    from promptcache_amd.model.llama_hip import LookupSlotLoop
    plain, sure = plain_run
    shape, w16, lm, eng, prompts = _gqa_setup(4)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    assert "k = %d" % k in ge.serve_plan(k, 4)[1]
    reqs = _requests(prompts)
    # the corpus of every request is the plain run's own output behind what serve gives it: every draft can be right
    real_corpus, order = GenerationEngine._lookup_corpus, iter(range(7))

    def corpus(cache, token_ids):                                        # (asked once per request, in the order they are pulled)
        return real_corpus(cache, token_ids) + plain[next(order)]
    monkeypatch.setattr(ge, "_lookup_corpus", corpus, raising=False)
    snaps, loops, retired = _lookup_snapshots(monkeypatch, m)
    pulled = []

    def lazy():
        for r, req in enumerate(reqs):
            pulled.append(r)
            yield req
    torch.manual_seed(5)
    outs = _collect(ge.serve(eng, lazy(), lookup=k))
    monkeypatch.undo()
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    stats = ge.last_serve_stats
    assert sorted(outs) == list(range(7)) and len(loops) == 1 and isinstance(loops[0], LookupSlotLoop) and loops[0].each
    assert loops[0].S * (k + 1) == (16 if k == 3 else 32) and m._live_loop is None
    assert [len(tokens[r]) for r in range(7)] == MAX_NEW7
    assert stats["tokens"] == sum(MAX_NEW7) - 7 and stats["steps"] == stats["replays"] == loops[0].n
    print(f"[serve lookup={k}] {stats['tokens']} tokens in {stats['steps']} replays")
    assert stats["steps"] < stats["tokens"]
    assert any(t[0] == "start" and t[3] > 0 for t in ge.last_serve_trace)      # somebody was admitted into the running loop
    compared = 0
    for r in range(7):
        assert tokens[r][:sure[r]] == plain[r][:sure[r]], (r, sure[r], tokens[r], plain[r])
        compared += sure[r]
        assert outs[r][-1].new_text == lm.decode(tokens[r]), r
    print(f"[serve lookup={k}] against plain serve: {compared} of {sum(MAX_NEW7)} tokens decided by the oracle's margin")
    assert 2 * compared >= sum(MAX_NEW7)                                  # (a condition on the inputs: W_SEED)
    loop = loops[0]
    assert sorted(j for j, _, _, _ in retired) == list(range(7))
    for j, length, len0, consumed in retired:                             # every arena: prefill rows + consumed TOKENS
        assert length == len0 + consumed and consumed == MAX_NEW7[j] - 1, (j, length, len0, consumed)
    for r in range(7):
        assert snaps[r]["max_new"] == MAX_NEW7[r] - 1 and (snaps[r]["params"] is None) == (r in (0, 2, 5))
    for r in range(7):
        solo = _solo(m, eng, snaps[r], 4, k, eng.max_ctx_length, loop.hist_cap)
        assert tokens[r] == solo, (r, tokens[r], solo)


def test_admitted_sequence_against_the_oracle_with_the_device_leading():
    """tests/test_gpu_serve.test_admitted_sequence_against_the_oracle_with_the_device_leading's method for the lookup loop: a
    sequence that enters at replay 6, once with nothing to copy and once with its own answer as the corpus (several rows a step)."""
    from oracle import engine_oracle as eo
    shape, w16, lm, eng, prompts = _gqa_setup(4)
    m = lm.hf_model
    model, lib = _oracle(shape, w16, m, eng)
    k, steps = 3, 12

    def start(j, slot):
        ids, pos, _, cache = eng.process(prompts[j], slot=slot)
        out = lm(input_ids=torch.tensor([ids], device=DEV), position_ids=torch.tensor([pos], device=DEV), past_key_values=cache,
                 use_cache=True)
        used = [mm.token_sequence for mm in eng.slot_cache(slot).staged]
        _, S0, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        assert float(np.abs(out.logits[0, -1].cpu().numpy() - olog[0, -1]).max()) < LOGIT_TOL
        return out.past_key_values, int(torch.argmax(out.logits[0, -1])), max(pos) + 2, present, S0 + len(ids)
    answer, worst, widest = [], 0.0, 0
    for corpus_is_answer in (False, True):
        a, b = start(0, 0), start(1, 1)
        loop = m.lookup_slot_loop([a[0], b[0]], [a[1], b[1]], [a[2], b[2]], 100, k, [[], []], slots=4, max_keys=2048, each=True,
                                  slot_index=[0, 1])
        got = []
        try:
            for i in range(6):
                loop.enqueue()
            past, tok, pos, present, n0 = start(2, 3)
            j = loop.admit(3, past, tok, pos, steps, None, 0, (), (), [tok] + answer if corpus_is_answer else [])
            assert j == 2 and loop._start[j] == 6 and loop.tokens(j, 5) == []
            i = 6
            while len(got) < steps:
                assert loop.enqueue() == i
                torch.cuda.synchronize()
                toks = loop.tokens(j, i)
                assert 1 <= len(toks) <= k + 1, (i, toks)
                rows = loop.logits[3 * (k + 1):3 * (k + 1) + len(toks)].cpu().numpy()
                for e, t in enumerate(toks):                             # row e was fed the token in front of t, at its position
                    olog, present = model.forward(np.array([[tok]]), np.array([[pos]]), past=present)
                    err = float(np.abs(rows[e] - olog[0, -1]).max())
                    worst = max(worst, err)
                    assert err < LOGIT_TOL, (i, e, err)
                    assert t == int(np.argmax(rows[e])), (i, e)
                    tok, pos = t, pos + 1
                widest = max(widest, len(toks))
                got += toks
                assert loop.tokens(0, i) and loop.tokens(1, i)
                i += 1
            assert loop.tokens(j, loop.enqueue()) == []                   # the budget is spent: the slot is off
        finally:
            loop.close({0: 0, 1: 0, 2: len(got)})
        assert len(got) == steps and loop.arenas[j].length == n0 + steps
        if corpus_is_answer:
            assert got == answer and widest > 1
        answer = got
    print(f"[mid_gqa] admitted at replay 6, {steps} tokens, up to {widest} a replay, oracle fed the device's tokens: max|dlogit| = {worst:.2e}")


def test_share_trunk_abandon_and_the_paths_that_stay(monkeypatch):
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    from promptcache_amd.model.llama_hip import LookupSlotLoop, SlotLoop
    monkeypatch.setenv("PC_SLOT_TRUNK_MIN", "1")
    monkeypatch.setenv("PC_TRUNK_VERIFY", "1")
    shape, w16, lm, eng, prompts = _gqa_setup(3)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    max_new = [4, 14, 16, 8]

    def reqs():
        return [(p, GenerationParameters(temperature=0.0, max_new_tokens=mn)) for p, mn in zip(prompts, max_new)]

    def run(**kw):
        kinds = set()
        outs = {}
        for r, o in ge.serve(eng, reqs(), **kw):
            outs.setdefault(r, []).append(o)
            if m._live_loop is not None:
                kinds.add((type(m._live_loop), m._live_loop.nsplit_trunk > 0))
        return {r: list(t) for r, t in ge.last_serve_tokens.items()}, kinds, outs
    # share_trunk=True, lookup=3: the unshared lookup run's tokens, from the shared-trunk verify step
    unshared, kinds, _ = run(lookup=3, share_trunk=False)
    assert kinds == {(LookupSlotLoop, False)}
    shared, kinds, _ = run(lookup=3, share_trunk=True)
    assert kinds == {(LookupSlotLoop, True)} and ("hold", 0) in [t[:2] for t in ge.last_serve_trace]
    assert shared == unshared and [len(shared[r]) for r in range(4)] == max_new
    # slots * (k + 1) > 64 cannot happen at 3 slots; a k the rows do not allow at 16 slots is serve_plan's business (CPU test) --
    # here: lookup off and lookup on give the same tokens through different loops
    off, kinds, _ = run(lookup=0)
    assert kinds == {(SlotLoop, False)} and [len(off[r]) for r in range(4)] == max_new
    # abandoning the generator rewinds every arena
    params = GenerationParameters(temperature=0.0, max_new_tokens=16)
    ids, pos, _, cache = eng.process(prompts[0])
    first = [o.new_text for o in ge.generate(ids, pos, params, cache)]
    n_ids = [len(eng.process(prompts[j], slot=j)[0]) for j in range(3)]
    gen = ge.serve(eng, iter(prompts), params, lookup=3)
    seen = {}
    for r, o in gen:
        seen[r] = seen.get(r, 0) + 1
        if all(seen.get(j, 0) >= 3 for j in range(3)):
            break
    gen.close()
    assert m._live_loop is None and sorted(seen) == [0, 1, 2]             # the rest of the requests was never pulled
    for j in range(3):
        a = eng.slot_cache(j).arena
        used = a.length - (len(eng.slot_cache(j)) + n_ids[j])
        assert 4 <= used <= 15 and used == len(ge.last_serve_tokens[j]) - 1, (j, used)
    ids, pos, _, cache = eng.process(prompts[0])
    assert [o.new_text for o in ge.generate(ids, pos, params, cache)] == first
    # 16 slots x (7 + 1) rows > 64: today's loop, identical tokens
    eng16 = CacheEngine(2048, lm, slots=16)
    eng16.add_schema(lm.get_formatter()(synth.persona_like("deep", system_len=60, intro_len=20, traits=(("age", (30, 26, 33)), ("home", (41, 37, 44))),
                                                           question_len=8, seed=6, pick=(0, 1))[0]))
    want = {}
    for lookup in (0, 7):
        kinds = set()
        for r, o in ge.serve(eng16, reqs()[:2], lookup=lookup):
            if m._live_loop is not None:
                kinds.add(type(m._live_loop))
        assert kinds == {SlotLoop}
        want[lookup] = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert want[0] == want[7] and "one token per replay" in ge.serve_plan(7, 16)[1]
    # Falcon: no slot loop -> generate per request, with or without lookup
    from promptcache_amd.model import Falcon
    from promptcache_amd.model.config import FALCON_SHAPES
    from promptcache_amd.model.weights import make_falcon_weights_np
    fshape = FALCON_SHAPES["falcon-mid"]
    flm = Falcon(name="falcon-mid", shape=fshape, weights=make_falcon_weights_np(fshape, 3, 2.0), device=DEV)
    fge = GenerationEngine(flm)
    assert not fge.serve_plan(3, 2)[0]
    feng = CacheEngine(1024, flm, slots=2)
    fprompts = []
    for pick, qlen in PICKS[:2]:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=(("age", (30, 26, 33)), ("home", (41, 37, 44))),
                                    question_len=qlen, seed=6, pick=pick)
        fprompts.append(Prompt(pp, [flm.get_formatter()]))
    feng.add_schema(flm.get_formatter()(sp))
    fparams = [GenerationParameters(temperature=0.0, max_new_tokens=8), GenerationParameters(temperature=0.0, max_new_tokens=5)]
    texts = {}
    for lookup in (0, 3):
        outs = _collect(fge.serve(feng, zip(fprompts, fparams), lookup=lookup))
        texts[lookup] = [[o.new_text for o in outs[j]] for j in range(2)]
    assert texts[0] == texts[3]
