"""Shared-trunk batched decode on the GPU: pc_attn_decode_slots_trunk through the C-ABI against tests/trunk_ref.py and the oracle's
attention, group / slot invariance and the no-trunk equivalence bit for bit, SlotLoop(share_trunk) against the numpy oracle, and
GenerationEngine.generate_batch(share_trunk=True) end to end."""
import numpy as np
import pytest
import torch

from oracle import engine_oracle as eo
from oracle import llama_oracle as orc
from tests import slots_ref
from tests import trunk_helpers as base
from tests import trunk_ref as ref

pytestmark = pytest.mark.gpu
DEV = base.DEV
ATT_TOL = 2e-4          # tests/test_gpu_slots.py's bar, from the baseline-size attention test
LOGIT_TOL = 1e-2        # tests/test_gpu_engine.py: the project's bar
SENT = base.SENT
_i32 = base.i32


def _split16(x):
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(np.float32)).astype(np.float16)


class Case:
    """S slots described by ``spec[b] = (keys, leader, T, live)`` (keys None: an idle slot without an arena of any use).  Every
    arena holds its own random rows everywhere, then rows [0, T) of a LEADER are what the group's expected values are built from:
    a member's private copy of the trunk rows is different data, so a kernel that reads it fails."""

    def __init__(self, rng, spec, H, Hkv, D, L=1, layer=0):
        self.S, self.H, self.Hkv, self.D, self.layer, self.spec = len(spec), H, Hkv, D, layer, spec
        self.arenas, caps = [], []
        for b, (keys, _, _, _) in enumerate(spec):
            n = keys or 0
            cap = n + 1 + 3 * (b % 4)
            a = torch.full((L, 2, Hkv, cap, D), SENT, dtype=torch.float16, device=DEV)
            if n:
                kv = rng.standard_normal((L, 2, Hkv, n, D), dtype=np.float32)
                kv[:, 0] *= 0.7
                a[:, :, :, :n] = torch.from_numpy(kv.astype(np.float16)).to(DEV)
            self.arenas.append(a)
            caps.append(cap)
        self.kv_base = torch.tensor([a.data_ptr() for a in self.arenas], dtype=torch.int64, device=DEV)
        self.cap = _i32(caps)
        self.len = _i32([(k or 1) - 1 for k, _, _, _ in spec])                # keys = len + 1 (the appended row included)
        self.live = _i32([0 if k is None else lv for k, _, _, lv in spec])
        self.leader = _i32([-1 if l is None else l for _, l, _, _ in spec])
        self.trunk = _i32([T for _, _, T, _ in spec])
        self.q = rng.standard_normal((self.S, H, D), dtype=np.float32)
        qh, ql = _split16(self.q.reshape(self.S, H * D))
        self.qh, self.ql = torch.from_numpy(qh).to(DEV), torch.from_numpy(ql).to(DEV)
        self.q_eff = (qh.astype(np.float32) + ql.astype(np.float32)).reshape(self.S, H, D)

    def planes(self):
        H, D = self.H, self.D
        return (torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV),
                torch.full((1, H * D // 32, 64, 8), SENT, dtype=torch.float16, device=DEV))

    def run(self, n, ns_own, ns_trunk):
        S, H, Hkv, D = self.S, self.H, self.Hkv, self.D
        ws = torch.empty(n.attn_decode_slots_trunk_workspace_bytes(S, H, D, ns_own, ns_trunk) // 4, dtype=torch.float32, device=DEV)
        out = self.planes()
        n.attn_decode_slots_trunk(self.qh, self.ql, H * D, self.kv_base, self.cap, self.len, self.live, self.leader, self.trunk, S,
                                  self.layer, H, Hkv, D, 1.0 / np.sqrt(D), ns_own, ns_trunk, ws, out)
        torch.cuda.synchronize()
        return out

    def run_plain(self, n, nsplit):
        S, H, Hkv, D = self.S, self.H, self.Hkv, self.D
        ws = torch.empty(n.attn_decode_slots_workspace_bytes(S, H, D, nsplit) // 4, dtype=torch.float32, device=DEV)
        out = self.planes()
        n.attn_decode_slots(self.qh, self.ql, H * D, self.kv_base, self.cap, self.len, self.live, S, self.layer, H, Hkv, D,
                            1.0 / np.sqrt(D), nsplit, ws, out)
        torch.cuda.synchronize()
        return out

    def check(self, n, out, tag):
        S, H, Hkv, D, ly = self.S, self.H, self.Hkv, self.D, self.layer
        got = (n.from_act_frags(out[0], S).float() + n.from_act_frags(out[1], S).float()).cpu().numpy()
        raw = n.from_act_frags(out[0], S).cpu().numpy()
        worst = 0.0
        for b, (keys, leader, T, live) in enumerate(self.spec):
            if keys is None or not live:
                assert np.all(raw[b] == SENT), f"idle slot {b} was written"
                continue
            own = self.arenas[b][ly, :, :, :keys].float().cpu().numpy()
            if leader is None:
                k, v, T = own[0], own[1], 0
            else:
                lead = self.arenas[leader][ly, :, :, :T].float().cpu().numpy()
                k = np.concatenate([lead[0], own[0][:, T:]], axis=1)
                v = np.concatenate([lead[1], own[1][:, T:]], axis=1)
            q = self.q_eff[b]
            want = ref.attend_trunk(q, k[:, :T], v[:, :T], k[:, T:], v[:, T:]).reshape(H * D)
            one = slots_ref.attend_slot(q, k, v).reshape(H * D)
            core = orc.attention_core(q[None, :, None, :], k[None], v[None], keys - 1, H // Hkv)[0, :, 0, :].reshape(H * D)
            err = max(float(np.abs(got[b] - w).max()) for w in (want, one, core))
            worst = max(worst, err)
            print(f"[{tag}] slot {b}: {keys} keys, leader {leader}, trunk {T}: max|d| = {err:.2e}")
            assert np.isfinite(got[b]).all() and err < ATT_TOL, (tag, b, keys, leader, T, err)
        print(f"[{tag}] worst max|d| = {worst:.2e}")


def _case1():
    spec = [(1726 + 9 * b, 0, 1725, 1) for b in range(8)]                              # group A: T = 1725, 8 members
    spec += [(8001 + 60 * b, 8, 8000, 1) for b in range(5)]                            # group B: T = 8000, 5 members
    spec[8] = (8100, 8, 8000, 0)                                                       # ... whose leader is not live
    spec += [(300, None, 0, 1), (1737, None, 0, 1), (None, None, 0, 0)]                # unshared, unshared, idle
    return spec


KERNEL_CASES = [
    # tag, H, Hkv, D, nsplit_own, nsplit_trunk, spec
    ("S=16 MHA two groups", 32, 32, 128, 2, 4, _case1()),
    ("GQA 8:1", 16, 2, 128, 4, 2, [(700, 1, 640, 1), (641, 1, 640, 1), (None, None, 0, 0), (1000, 1, 640, 1), (650, 1, 640, 1),
                                    (300, None, 0, 1), (645, 1, 640, 1), (2000, 1, 640, 1)]),
    ("MQA", 8, 1, 128, 1, 8, [(1737, 0, 1725, 1), (1800, 0, 1725, 1), (257, None, 0, 1), (1726, 0, 1725, 1)]),
    ("D=64", 8, 8, 64, 4, 1, [(70, None, 0, 1), (300, 1, 256, 1), (257, 1, 256, 1), (None, None, 0, 0), (1000, 4, 65, 1),
                              (66, 4, 65, 1), (900, 1, 256, 1), (66, 4, 65, 1)]),
    ("D=64 4:1", 8, 2, 64, 2, 3, [(300, 0, 256, 1), (257, 0, 256, 1), (1000, 0, 256, 1)]),
    ("a group of one", 4, 2, 128, 2, 2, [(1000, None, 0, 1), (1738, 1, 1725, 1), (66, 2, 1, 1)]),
]


@pytest.mark.parametrize("tag,H,Hkv,D,ns_own,ns_trunk,spec", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_trunk_attention_vs_the_reference(tag, H, Hkv, D, ns_own, ns_trunk, spec):
    n = base.native()
    c = Case(np.random.default_rng(H * 1000 + D + len(spec)), spec, H, Hkv, D)
    before = [a.clone() for a in c.arenas]
    out = c.run(n, ns_own, ns_trunk)
    for b, (a, a0) in enumerate(zip(c.arenas, before)):
        assert torch.equal(a.view(torch.int16), a0.view(torch.int16)), f"arena {b} was written"
    c.check(n, out, tag)


def test_a_slot_outside_the_host_contract_is_treated_as_unshared():
    """leader not leading itself, a leader index outside the slots, a trunk unlike the leader's, a trunk longer than the slot: each
    such slot gets the plain attention over its own arena (bit-equal to pc_attn_decode_slots), its neighbours are not disturbed."""
    n = base.native()
    H, Hkv, D, ns = 8, 2, 128, 2
    spec = [(700, 0, 640, 1), (800, 0, 640, 1),          # a proper group
            (900, 3, 640, 1),                            # its "leader" 3 does not lead itself
            (900, 0, 640, 1),                            # (slot 3: a member of group 0)
            (500, 9, 300, 1),                            # leader outside [0, S)
            (900, 0, 600, 1),                            # trunk unlike the leader's
            (300, 6, 400, 1)]                            # leads itself, but the trunk is longer than the slot
    c = Case(np.random.default_rng(5), spec, H, Hkv, D)
    out = c.run(n, ns, 3)
    plain = c.run_plain(n, ns)
    S = len(spec)
    for b in (2, 4, 5, 6):
        for a, p in zip(out, plain):
            assert torch.equal(n.from_act_frags(a, S)[b].view(torch.int16), n.from_act_frags(p, S)[b].view(torch.int16)), b
    c.spec = [s if b in (0, 1, 3) else (s[0], None, 0, 1) for b, s in enumerate(spec)]
    c.check(n, out, "contract")


@pytest.mark.parametrize("H,Hkv,D,ns_own,ns_trunk", [(32, 32, 128, 2, 4), (16, 2, 128, 4, 2), (8, 1, 64, 1, 3)])
def test_group_invariance_bit_for_bit(H, Hkv, D, ns_own, ns_trunk):
    """One sequence as the sole member of its group at slot 2 of 4, and the same sequence among 15 others at slot 11 of 16."""
    n = base.native()
    rng = np.random.default_rng(H + D)
    T, keys = 1725, 1740
    res = []
    for S, slot, others in ((4, 2, False), (16, 11, True)):
        spec = [(None, None, 0, 0)] * S
        if others:
            spec = [(T + 1 + 3 * b, 0, T, 1) for b in range(S)]
        spec[slot] = (keys, slot if not others else 0, T, 1)
        c = Case(rng, spec, H, Hkv, D)
        if not res:
            rows, q = c.arenas[slot][:, :, :, :keys].clone(), (c.qh[slot].clone(), c.ql[slot].clone())
        else:
            c.arenas[slot][:, :, :, :keys] = rows                         # the same own rows ...
            c.arenas[0][:, :, :, :T] = rows[:, :, :, :T]                    # ... and the same trunk rows, now in the leader's arena
            c.qh[slot], c.ql[slot] = q
        out = c.run(n, ns_own, ns_trunk)
        res.append((n.from_act_frags(out[0], S)[slot].clone(), n.from_act_frags(out[1], S)[slot].clone()))
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16)), "hi planes differ"
    assert torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16)), "lo planes differ"


def test_a_member_in_the_second_pass_of_the_trunk_launch():
    """Five members x 8 query heads of one kv head are 40 tile columns: the trunk launch takes two passes (32 columns each), their
    number follows from S, and the last member lies in the second.  It gets what the references give, and bit for bit what the
    same sequence gets as the only member of a group of one in a four-slot batch."""
    n = base.native()
    H, Hkv, D, ns_own, ns_trunk, T = 8, 1, 64, 1, 2, 65
    rng = np.random.default_rng(40)
    keys = [66, 70, 100, 129, 130]
    c = Case(rng, [(k, 0, T, 1) for k in keys], H, Hkv, D)
    out = c.run(n, ns_own, ns_trunk)
    c.check(n, out, "second pass")
    crowd = [n.from_act_frags(p, 5)[4].clone() for p in out]
    spec = [(None, None, 0, 0)] * 4
    spec[2] = (keys[4], 2, T, 1)
    solo = Case(rng, spec, H, Hkv, D)
    solo.arenas[2][:, :, :, :T] = c.arenas[0][:, :, :, :T]                 # the leader's trunk rows ...
    solo.arenas[2][:, :, :, T:keys[4]] = c.arenas[4][:, :, :, T:keys[4]]   # ... and the member's own
    solo.qh[2], solo.ql[2] = c.qh[4], c.ql[4]
    alone = [n.from_act_frags(p, 4)[2] for p in solo.run(n, ns_own, ns_trunk)]
    assert torch.equal(crowd[0].view(torch.int16), alone[0].view(torch.int16)), "hi planes differ"
    assert torch.equal(crowd[1].view(torch.int16), alone[1].view(torch.int16)), "lo planes differ"


@pytest.mark.parametrize("H,Hkv,D,ns_own", [(32, 32, 128, 4), (16, 2, 128, 8), (8, 1, 64, 2), (8, 8, 64, 1)])
def test_no_trunk_is_pc_attn_decode_slots_bit_for_bit(H, Hkv, D, ns_own):
    n = base.native()
    lens = [1, 2, 64, 65, 256, 258, 1738, 4000, None, 6, None, 101]
    c = Case(np.random.default_rng(D + ns_own), [(k, None, 0, 1) for k in lens], H, Hkv, D)
    a, b = c.run(n, ns_own, 5), c.run_plain(n, ns_own)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_shared_slot_loop_against_the_oracle_with_the_device_leading():
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    steps = 24
    shape, w16, lm, eng, prompts = base.mid_setup(24, 13, 4, base.PICKS)
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
    pasts, toks, poss, presents, lens = [], [], [], [], []
    for k, prompt in enumerate(prompts):
        ids, pos, out = base.prefill(lm, eng, prompt, k)
        used = [mm.token_sequence for mm in eng.slot_cache(k).staged]
        _, S, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        pasts.append(out.past_key_values)
        toks.append(int(torch.argmax(out.logits[0, -1])))
        poss.append(max(pos) + 2)
        presents.append(present)
        lens.append(S + len(ids))
    loop = m.slot_loop(pasts, toks, poss, steps + 1, share_trunk=True, min_trunk=1)
    assert loop is not None and loop.S == 4
    print("[shared SlotLoop] trunks:", loop.trunks, "nsplit own / trunk:", loop.nsplit, loop.nsplit_trunk)
    shared = [t for t in loop.trunks if t[0] is not None]
    assert len(shared) >= 2 and loop.nsplit_trunk >= 1 and all(T >= 60 for _, T in shared), loop.trunks
    assert ("slots", 4, loop.nsplit, "trunk", loop.nsplit_trunk) not in m._graphs
    worst = 0.0
    try:
        for i in range(steps):
            loop.enqueue()
            torch.cuda.synchronize()
            dev_logits = loop.logits.cpu().numpy()
            for k in range(4):
                olog, presents[k] = model.forward(np.array([[toks[k]]]), np.array([[poss[k]]]), past=presents[k])
                err = float(np.abs(dev_logits[k] - olog[0, -1]).max())
                worst = max(worst, err)
                assert err < LOGIT_TOL, (i, k, err)
                tok = loop.token(k, i)
                assert tok == int(np.argmax(dev_logits[k])), (i, k)
                toks[k], poss[k] = tok, poss[k] + 1
    finally:
        loop.close([steps] * 4)
    assert ("slots", 4, loop.nsplit, "trunk", loop.nsplit_trunk) in m._graphs
    print(f"[24 layers] shared SlotLoop, 4 ragged slots, {steps} steps, oracle fed the device's tokens: max|dlogit| = {worst:.2e}")
    for k in range(4):
        assert loop.arenas[k].length == lens[k] + steps


def test_shared_slot_loop_is_membership_invariant_over_32_steps():
    picks = base.PICKS + [((0, 0), 6), ((2, 2), 9), ((0, 2), 4), ((2, 1), 7)]
    shape, w16, lm, eng, prompts = base.mid_setup(3, 9, 8, picks)
    m = lm.hf_model
    steps = 32
    snap = []
    for k in range(8):
        ids, pos, out = base.prefill(lm, eng, prompts[k], k)
        a = out.past_key_values.arena
        snap.append((out.past_key_values, a.buf[:, :, :, :, :a.length].clone(), a.length, int(torch.argmax(out.logits[0, -1])), max(pos) + 2))

    def run(which, slot_index, follow):
        pasts, toks, poss = [], [], []
        for k in which:
            past, rows0, n0, tok, p0 = snap[k]
            past.arena.buf[:, :, :, :, :n0].copy_(rows0)
            past.arena.length = n0
            pasts.append(past); toks.append(tok); poss.append(p0)
        j = which.index(follow)
        loop = m.slot_loop(pasts, toks, poss, steps + 1, slots=8, slot_index=slot_index, share_trunk=True, min_trunk=1)
        assert loop.trunks[j][0] is not None, loop.trunks
        rows, tokens = [], [toks[j]]
        try:
            for i in range(steps):
                loop.enqueue()
                torch.cuda.synchronize()
                rows.append(loop.logits[slot_index[j]].clone())
                tokens.append(loop.token(j, i))
        finally:
            loop.close([steps] * len(which))
        a = loop.arenas[j]
        return torch.stack(rows), tokens, a.buf[:, :, :, :, :a.length].clone(), loop.trunks[j][1]

    pair = run([0, 1], [3, 6], 1)                                      # sequence 1 in a group of 2 (leader: sequence 0) ...
    crowd = run(list(range(8)), [6, 0, 1, 2, 3, 4, 5, 7], 1)           # ... and of 8, at another slot index
    assert pair[3] == crowd[3], "the two groups have different trunks: the comparison would not be like for like"
    assert pair[1] == crowd[1]
    bad = [i for i in range(steps) if not torch.equal(pair[0][i].view(torch.int32), crowd[0][i].view(torch.int32))]
    assert not bad, f"logits rows differ at steps {bad[:8]} ({len(bad)} of {steps})"
    assert torch.equal(pair[2].view(torch.int16), crowd[2].view(torch.int16))


def test_generate_batch_with_share_trunk(monkeypatch):
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    monkeypatch.setenv("PC_SLOT_TRUNK_MIN", "1")
    shape, w16, lm, eng, prompts = base.mid_setup(3, 9, 4, base.PICKS)
    m = lm.hf_model
    ge = GenerationEngine(lm)
    max_new = 20
    params = GenerationParameters(temperature=0.0, max_new_tokens=max_new, stop_token_ids=[])
    pasts, toks, poss = [], [], []
    for k, p in enumerate(prompts):
        ids, pos, out = base.prefill(lm, eng, p, k)
        pasts.append(out.past_key_values); toks.append(int(torch.argmax(out.logits[0, -1]))); poss.append(max(pos) + 2)
    hand = [[t] for t in toks]
    loop = m.slot_loop(pasts, toks, poss, max_new - 1, share_trunk=True)
    assert any(l is not None for l, _ in loop.trunks)
    key = ("slots", 4, loop.nsplit, "trunk", loop.nsplit_trunk)
    for i in range(max_new - 1):
        loop.enqueue()
        for k in range(4):
            hand[k].append(loop.token(k, i))
    loop.close([max_new - 1] * 4)
    assert key in m._graphs
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
    outs = base.collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, share_trunk=True))
    for k in range(4):
        assert outs[k][-1].new_text == lm.decode(hand[k]), k
        assert eng.slot_cache(k).arena.length == len(eng.slot_cache(k)) + len(reqs[k][0]) + max_new - 1
    # PC_SLOT_TRUNK=1 is share_trunk=None's default
    monkeypatch.setenv("PC_SLOT_TRUNK", "1")
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
    outs_env = base.collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params))
    assert [outs_env[k][-1].new_text for k in range(4)] == [outs[k][-1].new_text for k in range(4)]
    monkeypatch.delenv("PC_SLOT_TRUNK")
    # an abandoned generator rewinds every arena
    reqs = [eng.process(p, slot=k) for k, p in enumerate(prompts)]
    gen = ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, share_trunk=True)
    seen = {k: 0 for k in range(4)}
    for k, o in gen:
        seen[k] += 1
        if min(seen.values()) >= 3:
            break
    gen.close()
    assert m._live_loop is None
    for k in range(4):
        a = eng.slot_cache(k).arena
        used = a.length - (len(eng.slot_cache(k)) + len(reqs[k][0]))
        assert 4 <= used <= 5, (k, used)
    # two unrelated schemas: nothing to share, the unshared graph runs and the texts are share_trunk=False's
    sp2, pp2 = synth.persona_like("other", system_len=50, intro_len=30, traits=base.TRAITS,
                                  question_len=5, seed=11, pick=(1, 0))
    eng.add_schema(lm.get_formatter()(sp2))
    mixed = [prompts[0], Prompt(pp2, [lm.get_formatter()])]
    texts = []
    for share in (False, True):
        before = set(m._graphs)
        reqs = [eng.process(p, slot=k) for k, p in enumerate(mixed)]
        o = base.collect(ge.generate_batch([(r[0], r[1], r[3]) for r in reqs], params, share_trunk=share))
        texts.append([o[k][-1].new_text for k in range(2)])
        assert not [g for g in set(m._graphs) - before if "trunk" in g], "a batch without a shared group captured the trunk graph"
    assert texts[0] == texts[1]


def test_trunk_verify_passes_on_engine_staged_slots_and_raises_on_an_altered_row(monkeypatch):
    monkeypatch.setenv("PC_TRUNK_VERIFY", "1")
    shape, w16, lm, eng, prompts = base.mid_setup(3, 9, 2, base.PICKS[:2])
    m = lm.hf_model
    pasts, toks, poss = [], [], []
    for k, p in enumerate(prompts):
        ids, pos, out = base.prefill(lm, eng, p, k)
        pasts.append(out.past_key_values); toks.append(int(torch.argmax(out.logits[0, -1]))); poss.append(max(pos) + 2)
    loop = m.slot_loop(pasts, toks, poss, 4, share_trunk=True, min_trunk=1)
    assert loop.trunks[1][0] == 0 and loop.trunks[1][1] > 0
    loop.close([0, 0])
    a = pasts[1].arena
    a.buf[0, 1, 0, 0, 7, 3] += 1.0                                      # one value of one trunk row of the member
    with pytest.raises(RuntimeError, match="PC_TRUNK_VERIFY"):
        m.slot_loop(pasts, toks, poss, 4, share_trunk=True, min_trunk=1)
    assert m._live_loop is None                                         # (the refused loop took nothing over)
