"""Continuous batching on the GPU: pc_sample_advance_slots_each against tests/serve_ref.py and against pc_sample_advance_slots,
pc_slot_arm word for word and in stream order, SlotLoop.admit against the numpy oracle, and GenerationEngine.serve end to end --
every request against a solo run of the same sequence, the replay count against the host simulation."""
import ctypes

import numpy as np
import pytest
import torch

from tests import serve_ref as sr
from tests.test_gpu_slots import LOGIT_TOL, PICKS, SENT, _AdvState, _collect, _i32, _mid_setup, _n, _prefill

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PICKS7 = PICKS + [((0, 0), 6), ((2, 2), 9), ((0, 2), 4)]
MAX_NEW7 = [5, 12, 20, 9, 16, 7, 11]


class _EachState(_AdvState):
    """Device words of pc_sample_advance_slots_each: _AdvState plus per-slot parameter blocks, stop rows and draw counters."""

    def __init__(self, S, V, lens, caps, live, params, stops, draws, **kw):
        super().__init__(S, V, lens, caps, live, **kw)
        from promptcache_amd import _native
        blk = b"".join(_native.sample_params_bytes(*p, 0) for p in params)
        self.params_each = torch.frombuffer(bytearray(blk), dtype=torch.uint8).to(DEV)
        self.stop_each = torch.tensor(np.asarray(stops, dtype=np.int32), device=DEV)
        self.draws = _i32(draws)

    def advance_each(self, logits, processed=None):
        from promptcache_amd import _native
        _native.sample_advance_slots_each(logits, logits.stride(0), self.V, self.params_each, self.seeds, self.hist, self.ids, self.pos,
                                          self.len, self.cap, self.live, self.budget, self.stop_each, self.ring, self.ctr, self.draws,
                                          self.ring_cap, self.S, processed)


def _words(st):
    return {k: getattr(st, k).cpu().clone() for k in ("ids", "pos", "len", "cap", "live", "budget", "ctr", "ring", "hist", "seeds")}


@pytest.mark.parametrize("V", [1001, 32000])
def test_advance_each_equals_the_reference_per_slot(V):
    """tests/test_gpu_slots.test_advance_equals_the_reference_per_slot's method with per-slot chains, stop rows and draw counters.
    The rng seeds were checked on the CPU (test_serve_cpu.test_each_case_seeds_leave_three_quarters_comparable): the reference's
    margins leave at least 3/4 of the live sampled (slot, step) pairs to be compared outright."""
    from promptcache_amd.model.llama_hip import _history_bits
    S, steps = sr.EACH_S, sr.EACH_STEPS
    rng, hists, seeds, x0, stops = sr.each_case(V)
    st = _EachState(S, V, sr.EACH_LENS, sr.EACH_CAPS, sr.EACH_LIVE, sr.EACH_PARAMS, stops, sr.EACH_DRAWS, histories=hists,
                    budget=sr.EACH_BUDGET, step=sr.EACH_CTR, seeds=seeds)
    want, whist = sr.each_states(seeds), [set(h) for h in hists]
    checked = sampled_pairs = 0
    for step in range(steps):
        x = x0 if step == 0 else (rng.standard_normal((S, V)) * 2.0).astype(np.float32)
        buf = torch.full((S, V + 4), 7.0, dtype=torch.float32, device=DEV)              # (row stride V + 4)
        logits = buf[:, :V]
        logits.copy_(torch.from_numpy(x))
        proc = torch.full((S, V), SENT, dtype=torch.float32, device=DEV)
        before = [dict(w) for w in want]
        st.advance_each(logits, proc)
        torch.cuda.synchronize()
        ids, pos, ln, live, bud, ctr, drw = (t.cpu().tolist() for t in (st.ids, st.pos, st.len, st.live, st.budget, st.ctr, st.draws))
        proc = proc.cpu().numpy()
        fields = ("pos", "len", "live", "budget", "ctr", "draws")
        for b in range(S):
            tok, margin, wproc = sr.advance_each(want[b], x[b], whist[b], sr.EACH_PARAMS[b], stops[b])
            got = dict(ids=ids[b], pos=pos[b], len=ln[b], live=live[b], budget=bud[b], ctr=ctr[b], draws=drw[b])
            if tok is None:                                                            # idle, or a full arena: only live may move
                assert np.all(proc[b] == SENT), (step, b)
                assert got == {k: want[b][k] for k in got}, (step, b, got, want[b])
                if before[b]["live"] and before[b]["len"] >= before[b]["cap"]:
                    assert live[b] == 0 and b == 7
                continue
            assert np.isfinite(proc[b][ids[b]])
            both = np.isfinite(proc[b]) & np.isfinite(wproc)
            assert np.array_equal(proc[b][both], wproc[both])                        # temperature and penalty are IEEE-exact
            is_sampled = sr.EACH_PARAMS[b] != sr.GREEDY
            sampled_pairs += is_sampled
            if margin > sr.MARGIN:
                assert ids[b] == tok, (step, b, ids[b], tok, margin)
                checked += is_sampled
            else:                                                                     # follow the device through a near-tie
                whist[b].discard(tok); whist[b].add(ids[b]); want[b]["ids"] = ids[b]
                stop_b = set(int(t) for t in stops[b] if t >= 0)
                want[b]["live"] = int(not (ids[b] in stop_b or want[b]["budget"] <= 0 or want[b]["len"] + 1 >= want[b]["cap"]))
            assert tuple(got[k] for k in fields) == tuple(want[b][k] for k in fields), (step, b, got, want[b])
            assert int(st.ring[b * st.ring_cap + (ctr[b] - 1) % st.ring_cap]) == ids[b]
        if step == 0:
            assert live[3] == 0 and [live[b] for b in (0, 1, 4, 5)] == [1] * 4 and live[7] == 0   # the stop id ended exactly its slot
            assert drw[1] == sr.EACH_DRAWS[1] + 1 and ctr[1] == sr.EACH_CTR + 1 and drw[2] == sr.EACH_DRAWS[2]
    print(f"[advance_each V={V}] sampled pairs {sampled_pairs}, compared outright {checked}")
    assert sampled_pairs == 9 and 4 * checked >= 3 * sampled_pairs, (checked, sampled_pairs)
    assert st.live.cpu().tolist() == [0] * S
    got_hist = st.hist.cpu()
    for b in range(S):                                                                 # histories do not leak between slots
        assert torch.equal(got_hist[b], _history_bits(sorted(whist[b]), V)), b


@pytest.mark.parametrize("prm", [sr.SAMPLED, sr.GREEDY])
def test_uniform_blocks_are_bit_identical_to_advance_slots(prm):
    V, S, steps = 32000, 8, 4
    rng = np.random.default_rng(5)
    live0, lens0, caps = [1, 1, 0, 1, 1, 1, 0, 1], [50 + 3 * b for b in range(S)], [1000] * 7 + [71]
    hists = [set(int(t) for t in rng.integers(0, V, 30)) for _ in range(S)]
    seeds = [int(s) for s in rng.integers(0, 2 ** 62, S)]
    stop = (17, 4242)
    kw = dict(histories=hists, budget=3, step=3, seeds=seeds)
    a = _AdvState(S, V, lens0, caps, live0, stop=stop, **kw)
    a.set_params(*prm)
    stops = [list(stop) + [-1] * 6] * S
    b = _EachState(S, V, lens0, caps, live0, [prm] * S, stops, [3] * S, **kw)          # draws == counters
    for step in range(steps):
        x = torch.from_numpy((rng.standard_normal((S, V)) * 2.0).astype(np.float32)).to(DEV)
        pa = torch.full((S, V), SENT, dtype=torch.float32, device=DEV)
        pb = pa.clone()
        a.advance(x, pa)
        b.advance_each(x, pb)
        torch.cuda.synchronize()
        wa, wb = _words(a), _words(b)
        for k in wa:
            assert torch.equal(wa[k], wb[k]), (step, k)
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), step
        assert torch.equal(b.draws, b.ctr)
    assert a.live.cpu().tolist() == [0] * S


def _sentinel_state(n, S, V):
    hw = (V + 31) // 32
    t = lambda dt, v, shape=(S,): torch.full(shape, v, dtype=dt, device=DEV)
    st = dict(kv_base=t(torch.int64, 111), cap=t(torch.int32, 112), len=t(torch.int32, 113), pos=t(torch.int32, 114),
              ids=t(torch.int64, 115), live=t(torch.int32, 0), leader=t(torch.int32, 117), trunk=t(torch.int32, 118),
              budget=t(torch.int32, 119), ctr=t(torch.int32, 120), draws=t(torch.int32, 121), seeds=t(torch.int64, 122),
              params=t(torch.uint8, 0x5a, (S * 24,)), stop=t(torch.int32, 124, (S, 8)), hist=t(torch.int32, 0x5b5b5b5b, (S, hw)))
    handle = n.slot_state(st["kv_base"], st["cap"], st["len"], st["pos"], st["ids"], st["live"], st["leader"], st["trunk"], st["budget"],
                          st["ctr"], st["draws"], st["seeds"], st["params"], st["stop"], st["hist"])
    return st, handle


def _pinned_block(n, hw, **f):
    raw = sr.arm_block_bytes(n, hw, **f)
    host = torch.zeros(len(raw), dtype=torch.uint8, pin_memory=True)
    host.copy_(torch.frombuffer(raw, dtype=torch.uint8))
    return host


def test_slot_arm_writes_one_slot_and_orders_behind_enqueued_steps():
    from promptcache_amd.model.llama_hip import _history_bits
    n = _n()
    S, V = 4, 1001
    hw = (V + 31) // 32
    rng = np.random.default_rng(2)
    st, handle = _sentinel_state(n, S, V)
    before = {k: v.cpu().clone() for k, v in st.items()}
    arena = torch.zeros(8, dtype=torch.float16, device=DEV)
    hist_ids = sorted(set(int(t) for t in rng.integers(0, V, 40)))
    hist = _history_bits(hist_ids, V).numpy().view(np.uint32)
    seed = int(rng.integers(0, 2 ** 62))
    f = dict(slot=2, cap=900, kv_base=arena.data_ptr(), len=40, pos=77, id=9, leader=-1, trunk=0, budget=3, counter=12, draws=1,
             seed=seed, params=sr.SAMPLED, stop_ids=[5, 6, 7], hist=hist)
    host = _pinned_block(n, hw, **f)
    n.slot_arm(host, n.slot_arm_bytes(hw), handle, S)
    torch.cuda.synchronize()
    after = {k: v.cpu().clone() for k, v in st.items()}
    want2 = dict(kv_base=arena.data_ptr(), cap=900, len=40, pos=77, ids=9, live=1, leader=-1, trunk=0, budget=3, ctr=12, draws=1,
                 seeds=seed)
    for k, v in want2.items():
        assert int(after[k][2]) == v, k
    assert bytes(after["params"][48:72].numpy()) == n.sample_params_bytes(*sr.SAMPLED, 0)
    assert after["stop"][2].tolist() == [5, 6, 7, -1, -1, -1, -1, -1]
    assert np.array_equal(after["hist"][2].numpy().view(np.uint32), hist)
    for k in st:                                                        # every other word is unchanged
        rows = after[k].view(S, -1)
        keep = [b for b in range(S) if b != 2]
        assert torch.equal(rows[keep], before[k].view(S, -1)[keep]), k
    # one advance_each step moves slot 2 as the reference says (the other slots are idle)
    x = (rng.standard_normal((S, V)) * 2.0).astype(np.float32)
    logits = torch.from_numpy(x).to(DEV)
    ring = torch.full((S * 16,), -1, dtype=torch.int32, device=DEV)

    def step():
        n.sample_advance_slots_each(logits, V, V, st["params"], st["seeds"], st["hist"], st["ids"], st["pos"], st["len"], st["cap"],
                                    st["live"], st["budget"], st["stop"], ring, st["ctr"], st["draws"], 16, S)
    step()
    torch.cuda.synchronize()
    w = dict(ids=9, pos=77, len=40, cap=900, live=1, budget=3, ctr=12, draws=1, seed=seed)
    tok, margin, _ = sr.advance_each(w, x[2], set(hist_ids), sr.SAMPLED, [5, 6, 7])
    assert margin > sr.MARGIN, "pick another rng seed: the reference's draw is a near-tie"
    got = {k: int(st[k2][2]) for k, k2 in (("ids", "ids"), ("pos", "pos"), ("len", "len"), ("live", "live"), ("budget", "budget"),
                                           ("ctr", "ctr"), ("draws", "draws"))}
    assert got == {k: w[k] for k in got} and got["ids"] == tok
    assert int(ring[2 * 16 + 12]) == tok
    assert st["pos"].cpu().tolist()[:2] == [114, 114] and int(st["ctr"][3]) == 120
    # arm slot 1 BEHIND an enqueued step on the same stream: that step saw the old words (idle), the next one sees the new
    f1 = dict(f, slot=1, pos=500, len=10, id=3, counter=13, hist=np.zeros(hw, dtype=np.uint32), params=sr.GREEDY, stop_ids=[])
    host1 = _pinned_block(n, hw, **f1)
    snap = torch.empty(2, dtype=torch.int32, device=DEV)
    step()
    snap.copy_(torch.stack([st["pos"][1], st["live"][1]]))              # (on the stream, between the step and the arm launch)
    n.slot_arm(host1, n.slot_arm_bytes(hw), handle, S)
    step()
    torch.cuda.synchronize()
    assert snap.cpu().tolist() == [114, 0]
    assert int(st["pos"][1]) == 501 and int(st["len"][1]) == 11 and int(st["ids"][1]) == int(np.argmax(x[1])) and int(st["live"][1]) == 1
    assert int(ring[1 * 16 + 13]) == int(np.argmax(x[1]))


# ---- the model: admission, serve ------------------------------------------------------------------------------------------------
def _snapshots(monkeypatch, m):
    """Record, at every entry of a sequence into a slot loop, a byte copy of its arena rows and what the loop was told."""
    from promptcache_amd.model.llama_hip import SlotLoop
    snaps, loops, retired = [], [], []

    def take(past, token, position, max_new, params, seed, history, stop_ids):
        a = past.arena
        snaps.append(dict(rows=a.buf[:, :, :, :, :a.length].clone(), n0=a.length, token=int(token), position=int(position),
                          max_new=int(max_new), params=params, seed=int(seed), history=list(history), stop_ids=list(stop_ids)))
    real_loop, real_admit, real_retire = m.slot_loop, SlotLoop.admit, SlotLoop.retire

    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, **kw):
        for j in range(len(pasts)):
            take(pasts[j], tokens[j], positions[j], max_new[j], params[j], seeds[j], histories[j], stop_ids[j])
        loop = real_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, **kw)
        loops.append(loop)
        return loop

    def admit(self, slot_index, past, token, position, max_new, params, seed, history, stop_ids, trunk=None):
        take(past, token, position, max_new, params, seed, history, stop_ids)
        return real_admit(self, slot_index, past, token, position, max_new, params, seed, history, stop_ids, trunk=trunk)

    def retire(self, k, consumed):
        real_retire(self, k, consumed)
        retired.append((k, self.arenas[k].length, self.len0[k], consumed))
    monkeypatch.setattr(m, "slot_loop", slot_loop)
    monkeypatch.setattr(SlotLoop, "admit", admit)
    monkeypatch.setattr(SlotLoop, "retire", retire)
    return snaps, loops, retired


def _solo(m, eng, snap, slots, max_keys):
    """The sequence of ``snap`` alone in an each=True loop, from the byte copy of its prefill (in slot 0's staged buffer)."""
    a = eng.slot_cache(0).arena
    a.pending = None                                                    # (no staging left over: the rows below are the sequence)
    a.buf[:, :, :, :, :snap["n0"]].copy_(snap["rows"])
    a.length = snap["n0"]
    loop = m.slot_loop([a.views(snap["n0"])], [snap["token"]], [snap["position"]], snap["max_new"], snap["params"], [snap["seed"]],
                       [snap["history"]], snap["stop_ids"], slots=slots, each=True, max_keys=max_keys)
    toks = [snap["token"]]
    try:
        for i in range(snap["max_new"]):
            loop.enqueue()
            t = loop.token(0, i)
            if t is None:
                break
            toks.append(t)
    finally:
        loop.close({0: len(toks) - 1})
    return toks


def test_serve_greedy_equals_solo_runs_and_the_simulated_replay_count(monkeypatch):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    from promptcache_amd.slot_scheduler import replay_count
    shape, w16, lm, eng, prompts = _mid_setup(3, 9, 4, PICKS7)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    assert ge.serve_plan()[0]
    snaps, loops, retired = _snapshots(monkeypatch, m)
    pulled = []

    def lazy():
        for r, (p, mn) in enumerate(zip(prompts, MAX_NEW7)):
            pulled.append(r)
            yield p, GenerationParameters(temperature=0.0, max_new_tokens=mn)
    outs = _collect(ge.serve(eng, lazy()))
    monkeypatch.undo()
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert sorted(outs) == list(range(7)) and len(snaps) == 7 and len(loops) == 1
    assert [len(tokens[r]) for r in range(7)] == MAX_NEW7
    assert ge.last_serve_stats["replays"] == replay_count(MAX_NEW7, 4) == 22
    starts = {t[1]: t[3] for t in ge.last_serve_trace if t[0] == "start"}
    assert [starts[r] for r in range(7)] == [0, 0, 0, 0, 5, 9, 12]       # requests 4..6 were admitted into the running loop
    for k, length, len0, consumed in retired:                            # every arena: prefill rows + consumed steps
        assert length == len0 + consumed and consumed == snaps[k]["max_new"], (k, length, len0, consumed)
    assert len(retired) == 7 and m._live_loop is None
    for r in range(7):
        assert snaps[r]["max_new"] == MAX_NEW7[r] - 1
        solo = _solo(m, eng, snaps[r], 4, eng.max_ctx_length)
        assert tokens[r] == solo, r
        assert outs[r][-1].new_text == lm.decode(solo), r
        assert len(outs[r]) == len([s for s in range(MAX_NEW7[r]) if s % 2 == 0 or s == MAX_NEW7[r] - 1]), r


def test_admitted_sequence_against_the_oracle_with_the_device_leading():
    """tests/test_gpu_slots.test_slot_loop_against_the_oracle_with_the_device_leading's method for a sequence that enters a running
    loop at replay 6."""
    from oracle import engine_oracle as eo
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    shape, w16, lm, eng, prompts = _mid_setup(3, 13, 4, PICKS)
    m = lm.hf_model
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    model = LlamaOracle(cfg, {k: v.astype(np.float32) for k, v in w16.items()})
    sc = eng.get_schema("deep")
    jobs = []
    for p in sc.encode_paths():
        sf = sc.get_scaffold(p)
        jobs.append(dict(token_ids=sf.token_ids(), position_ids=sf.position_ids(), targets=sf.select(p).all_token_sequences()))
    lib = eo.encode_schema(model, jobs)

    def start(k, slot):
        ids, pos, out = _prefill(lm, eng, prompts[k], slot)
        used = [mm.token_sequence for mm in eng.slot_cache(slot).staged]
        _, S0, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        assert float(np.abs(out.logits[0, -1].cpu().numpy() - olog[0, -1]).max()) < LOGIT_TOL
        return out.past_key_values, int(torch.argmax(out.logits[0, -1])), max(pos) + 2, present, S0 + len(ids)
    a, b = start(0, 0), start(1, 1)
    steps = 10
    loop = m.slot_loop([a[0], b[0]], [a[1], b[1]], [a[2], b[2]], 40, None, slots=4, slot_index=[0, 1], each=True, max_keys=2048)
    worst = 0.0
    try:
        for i in range(6):
            loop.enqueue()
        past, tok, pos, present, n0 = start(2, 3)
        k = loop.admit(3, past, tok, pos, steps + 1, None, 0, (), ())
        assert k == 2 and loop._start[k] == 6 and loop.token(k, 5) is None
        for i in range(6, 6 + steps):
            loop.enqueue()
            torch.cuda.synchronize()
            row = loop.logits[3].cpu().numpy()
            olog, present = model.forward(np.array([[tok]]), np.array([[pos]]), past=present)
            err = float(np.abs(row - olog[0, -1]).max())
            worst = max(worst, err)
            assert err < LOGIT_TOL, (i, err)
            got = loop.token(k, i)
            assert got == int(np.argmax(row)), i
            tok, pos = got, pos + 1
            assert loop.token(0, i) is not None and loop.token(1, i) is not None
    finally:
        loop.close({0: 6 + steps, 1: 6 + steps, 2: steps})
    print(f"[3 layers] admitted at replay 6, {steps} steps, oracle fed the device's tokens: max|dlogit| = {worst:.2e}")
    assert loop.arenas[k].length == n0 + steps


def test_serve_mixed_greedy_and_sampled_requests_equal_their_solo_runs(monkeypatch):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    shape, w16, lm, eng, prompts = _mid_setup(3, 9, 2, PICKS)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    G = GenerationParameters

    def requests(stops):
        return [(prompts[0], G(temperature=0.0, max_new_tokens=14, stop_token_ids=stops[0])),
                (prompts[1], G(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40, max_new_tokens=18, stop_token_ids=stops[1])),
                (prompts[2], G(temperature=0.0, max_new_tokens=9, stop_token_ids=stops[2])),
                (prompts[3], G(temperature=1.3, repetition_penalty=1.3, top_p=0.8, top_k=12, max_new_tokens=16, stop_token_ids=stops[3]))]
    torch.manual_seed(5)
    _collect(ge.serve(eng, requests([[], [], [], []])))
    free = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert [len(free[r]) for r in range(4)] == [14, 18, 9, 16]
    # stop ids of their own: each request's token at a step of its own, plus ids that hit nobody; request 3 gets eleven of them
    # (the device holds the first eight, the one that hits is the tenth: the host kills the slot)
    cut = {0: 6, 1: 9, 2: 4, 3: 7}
    never = [t for t in range(100, 140) if all(t not in free[r] for r in range(4))]
    stops = [[never[0], free[0][6]], [free[1][9]], [never[1], never[2], free[2][4]], never[3:12] + [free[3][7]] + never[12:13]]
    snaps, loops, retired = _snapshots(monkeypatch, m)
    torch.manual_seed(5)
    outs = _collect(ge.serve(eng, requests(stops)))
    monkeypatch.undo()
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    assert len(snaps) == 4 and m._live_loop is None
    for r in range(4):
        first = next(i for i, t in enumerate(free[r]) if t in stops[r])
        assert first <= cut[r] and tokens[r] == free[r][:first + 1], r                # the stream is the unstopped one, cut at the stop
        assert (snaps[r]["params"] is None) == (r in (0, 2))
        solo = _solo(m, eng, snaps[r], 2, eng.max_ctx_length)
        assert tokens[r] == solo[:len(tokens[r])], r
        if len(stops[r]) <= 8:
            assert tokens[r] == solo, r                                               # the device stopped the solo run at the same token
        assert outs[r][-1].new_text == lm.decode(tokens[r]), r
    assert len(snaps[3]["stop_ids"]) == 8 and stops[3][9] not in snaps[3]["stop_ids"]
    assert any(t[0] == "start" and t[3] > 0 for t in ge.last_serve_trace)              # somebody was admitted into the running loop


def test_serve_with_share_trunk_protects_the_leader_and_lets_a_request_join(monkeypatch):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    monkeypatch.setenv("PC_SLOT_TRUNK_MIN", "1")
    monkeypatch.setenv("PC_TRUNK_VERIFY", "1")
    shape, w16, lm, eng, prompts = _mid_setup(3, 9, 3, PICKS)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    max_new = [4, 14, 16, 8]                                             # the leader (request 0, slot 0) ends first

    def reqs():
        return [(p, GenerationParameters(temperature=0.0, max_new_tokens=mn)) for p, mn in zip(prompts, max_new)]
    plain = _collect(ge.serve(eng, reqs(), share_trunk=False))
    plain_tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    snaps, loops, retired = _snapshots(monkeypatch, m)
    outs = _collect(ge.serve(eng, reqs(), share_trunk=True))
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    trace = list(ge.last_serve_trace)
    loop = loops[0]
    assert loop.nsplit_trunk > 0 and loop.trunks[0][0] == 0 and loop.trunks[1][0] == 0 and loop.trunks[2][0] == 0
    T = loop.trunks[0][1]
    assert loop.trunks[3] == (0, T)                                       # the fourth request joined the group
    # the leader's slot was held while members lived: request 3 went to another slot, slot 0 was freed after the last member
    assert ("hold", 0) in [t[:2] for t in trace]
    pull3 = next(t for t in trace if t[0] == "pull" and t[1] == 3)
    assert pull3[2] != 0
    pos = {(t[0], t[1]): j for j, t in enumerate(trace) if t[0] in ("hold", "free")}
    last_member_end = max(j for j, t in enumerate(trace) if t[0] == "finish" and t[1] in (1, 2, 3))
    assert pos[("hold", 0)] < pos[("free", 0)] and pos[("free", 0)] > last_member_end
    assert not any(t[0] == "pull" and t[2] == 0 and t[1] != 0 for t in trace)
    for r in range(4):                                                   # test_generate_batch_with_share_trunk's bound: the same tokens
        assert tokens[r] == plain_tokens[r] and len(tokens[r]) == max_new[r], r
        assert outs[r][-1].new_text == plain[r][-1].new_text, r


def test_abandoned_serve_rewinds_every_arena_and_falcon_falls_back_to_generate():
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    shape, w16, lm, eng, prompts = _mid_setup(3, 9, 2, PICKS)
    ge = GenerationEngine(lm)
    params = GenerationParameters(temperature=0.0, max_new_tokens=16)
    ids, pos, _, cache = eng.process(prompts[0])
    first = [o.new_text for o in ge.generate(ids, pos, params, cache)]
    n_ids = [len(eng.process(prompts[k], slot=k)[0]) for k in range(2)]
    gen = ge.serve(eng, iter(prompts), params)
    seen = {}
    for r, o in gen:
        seen[r] = seen.get(r, 0) + 1
        if seen.get(0, 0) >= 3 and seen.get(1, 0) >= 3:
            break
    gen.close()
    assert lm.hf_model._live_loop is None and sorted(seen) == [0, 1]     # the rest of the requests was never pulled
    # Outputs come at steps 0, 2, 4, ...: three Outputs of a sequence = tokens of steps 0..4 consumed at least
    for k in range(2):
        a = eng.slot_cache(k).arena
        used = a.length - (len(eng.slot_cache(k)) + n_ids[k])
        assert 4 <= used <= 5, (k, used)
    ids, pos, _, cache = eng.process(prompts[0])
    assert [o.new_text for o in ge.generate(ids, pos, params, cache)] == first
    # Falcon: no slot loop -> generate per request, equal outputs
    from promptcache_amd.model import Falcon
    from promptcache_amd.model.config import FALCON_SHAPES
    from promptcache_amd.model.weights import make_falcon_weights_np
    fshape = FALCON_SHAPES["falcon-mid"]
    flm = Falcon(name="falcon-mid", shape=fshape, weights=make_falcon_weights_np(fshape, 3, 2.0), device=DEV)
    fge = GenerationEngine(flm)
    assert not fge.serve_plan()[0]
    feng = CacheEngine(1024, flm, slots=2)
    fprompts = []
    for pick, qlen in PICKS[:2]:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=(("age", (30, 26, 33)), ("home", (41, 37, 44))),
                                    question_len=qlen, seed=6, pick=pick)
        fprompts.append(Prompt(pp, [flm.get_formatter()]))
    feng.add_schema(flm.get_formatter()(sp))
    fparams = [GenerationParameters(temperature=0.0, max_new_tokens=8), GenerationParameters(temperature=0.0, max_new_tokens=5)]
    want = []
    for p, gp in zip(fprompts, fparams):
        ids, pos, _, cache = feng.process(p)
        want.append([o.new_text for o in fge.generate(ids, pos, gp, cache)])
    outs = _collect(fge.serve(feng, zip(fprompts, fparams)))
    assert [[o.new_text for o in outs[k]] for k in range(2)] == want
