"""Prefill inside the lookup step on the model: ``LookupSlotLoop.admit_prompt`` on ``mid`` (4 layers, S = 4, k = 3) and
once on ``mid64`` with MXFP4 weights -- the last question row's logits and the appended K/V rows against ``LlamaOracle``, the state
words against the serial arm, the decoding neighbours against a run without the admissions -- and ``serve(loop_prefill=True)``
against ``serve``: tokens where the oracle's margin decides, shared trunks, and the mode switched off."""
import dataclasses
import gc

import numpy as np
import pytest
import torch

from oracle import engine_oracle as eo
from tests import lookup_sample_ref as lsr
from tests import lookup_serve_ref as lsv
from tests import sample_ref as sr
from tests.test_gpu_lookup_serve import _pinned, _sentinel_state
from tests.test_gpu_slots import LOGIT_TOL, PICKS, _collect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, SLOTS = 3, 4
KV_TOL = 4e-3           # tests/test_gpu_baseline_sizes.py: appended rows are fp16(the oracle's fp32 K / V) up to an ulp
TRAITS = (("age", (30, 26, 33)), ("home", (41, 37, 44)))
PICKS7 = PICKS + [((0, 0), 6), ((2, 2), 9), ((0, 2), 4)]
MAX_NEW7 = [5, 12, 20, 9, 16, 7, 11]
W_SEED = 13
_SETUP = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The models, engines and loops of this module go when it ends, and the caching allocator hands their blocks back: block
    sizes that only this module asks for (4-layer arenas) must not be what a later test's allocations are carved from --
    tests that count ``torch.cuda.memory_allocated`` see an unsplit remainder of such a block as bytes nobody owns."""
    yield
    _SETUP.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _setup(name, slots):
    """One model per shape for the module: ``mid`` cut to 4 layers in fp16, ``mid64`` cut to 4 layers with MXFP4 weights."""
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    if name not in _SETUP:
        shape = dataclasses.replace(SHAPES[name], num_hidden_layers=4, name=f"{name}-4")
        w16 = make_weights_np(shape, W_SEED, 2.0)
        kw = dict(weight_format="mxfp4") if name == "mid64" else {}
        _SETUP[name] = (shape, Llama2(name=shape.name, shape=shape, weights=w16, device=DEV, **kw))
    shape, lm = _SETUP[name]
    eng = CacheEngine(2048, lm, slots=slots)
    prompts = []
    for pick, qlen in PICKS7:
        sp, pp = synth.persona_like("deep", system_len=60, intro_len=20, traits=TRAITS, question_len=qlen, seed=6, pick=pick)
        prompts.append(Prompt(pp, [lm.get_formatter()]))
    eng.add_schema(lm.get_formatter()(sp))
    return shape, lm, eng, prompts


def _oracle(shape, m, eng):
    """LlamaOracle on the weights the device computes with (``dequantized_weights``: the fp16 values, or W' of the 4-bit images)."""
    from oracle.llama_oracle import LlamaOracle, OracleConfig
    cfg = OracleConfig(vocab_size=shape.vocab_size, hidden_size=shape.hidden_size, intermediate_size=shape.intermediate_size,
                       num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                       num_key_value_heads=shape.num_key_value_heads, rms_norm_eps=shape.rms_norm_eps,
                       rope_theta=shape.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    model = LlamaOracle(cfg, {name: v.float().cpu().numpy() for name, v in m.dequantized_weights().items()})
    sc = eng.get_schema("deep")
    jobs = []
    for p in sc.encode_paths():
        sf = sc.get_scaffold(p)
        jobs.append(dict(token_ids=sf.token_ids(), position_ids=sf.position_ids(), targets=sf.select(p).all_token_sequences()))
    return model, eo.encode_schema(model, jobs)


def _prefilled(lm, eng, prompt, slot):
    ids, pos, _, cache = eng.process(prompt, slot=slot)
    out = lm(input_ids=torch.tensor([ids], device=DEV), position_ids=torch.tensor([pos], device=DEV), past_key_values=cache, use_cache=True)
    return out.past_key_values, int(torch.argmax(out.logits[0, -1])), max(pos) + 2


# ---- (a) - (d): admit_prompt beside two decoding sequences ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid", "mid64"])
def test_questions_fed_through_the_step_beside_two_decoding_sequences(name):
    """Two sequences decode; at replay 2 a third is admitted with q = 9 (greedy) and a fourth with q = 4 (sampled).  (a) the logits
    of each one's last question row against ``LlamaOracle`` over the staged rows plus the question, at the project's 1e-2 bar;
    (b) arena rows [T, T + q) against the oracle's K / V; (c) after the step that emits the first token, every word of the slot
    against a real ``pc_lookup_slot_arm`` launch for a serial prefill that drew the same token; (d) the neighbours' tokens
    against a run in which slots 2 and 3 stay idle.  Measured: DESIGN 3.30."""
    from promptcache_amd import _native as n
    from promptcache_amd.generation_engine import GenerationParameters
    from promptcache_amd.model.llama_hip import LookupSlotLoop, lookup_admit_history
    shape, lm, eng, prompts = _setup(name, SLOTS)
    m = lm.hf_model
    V = shape.vocab_size
    model, lib = _oracle(shape, m, eng)
    rng = np.random.default_rng(5)
    before, total = 2, 8                                    # replays in front of the admissions, replays in all
    # the two admissions: q = 9 greedy (chunks 4 + 4 + 1: the forced rows run out, an ordinary step feeds the last token) and q = 4
    # sampled (one step, row 3 ends the question); distinct ids, so the ordinary step finds nothing to draft
    sampled = GenerationParameters(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40)
    adm = [dict(slot=2, prompt=2, q=9, params=None, tuple=lsv.GREEDY, seed=0, max_new=6, stops=[]),
           dict(slot=3, prompt=3, q=4, params=sampled, tuple=(0.7, 1.1, 0.9, 40), seed=991, max_new=5, stops=[7])]
    for a in adm:
        a["ids"] = [int(t) for t in rng.choice(np.arange(3, V), a["q"], replace=False)]

    def run(admit):
        pasts, toks, poss = zip(*[_prefilled(lm, eng, prompts[j], j) for j in (0, 1)])
        loop = m.lookup_slot_loop(list(pasts), list(toks), list(poss), 40, K, [[], []], slots=SLOTS, max_keys=2048, each=True,
                                  slot_index=[0, 1], prompt_rows=True)
        assert isinstance(loop, LookupSlotLoop) and loop.prompt_rows and "forced" in loop.st
        seen = {}
        try:
            for i in range(total):
                if i == before and admit:
                    for a in adm:
                        ids_p, pos_p, _, cache = eng.process(prompts[a["prompt"]], slot=a["slot"])
                        a.update(cache=cache, pos0=pos_p[0], corpus=[int(t) for t in rng.integers(3, V, 30) if int(t) not in a["ids"]],
                                 used=[mm.token_sequence for mm in eng.slot_cache(a["slot"]).staged])
                        a["j"] = loop.admit_prompt(a["slot"], cache, a["ids"], a["pos0"], a["max_new"], a["params"], a["seed"], a["ids"],
                                                   a["stops"], a["corpus"])
                        a["T"] = loop.len0[a["j"]] - a["q"]
                        assert loop.prefill_replays(a["j"]) == -(-a["q"] // (K + 1)) and loop.first_step(a["j"]) == before + loop.prefill_replays(a["j"]) - 1
                assert loop.enqueue() == i
                torch.cuda.synchronize()
                seen[i] = dict(logits=loop.logits.cpu().numpy().copy(), st={w: loop.st[w].cpu().numpy().copy() for w in
                               ("hist", "hist_len", "ids", "pos", "len", "budget", "draws", "bits", "stop", "forced", "live", "cap", "kv_base")},
                               toks=[loop.tokens(j, i) for j in range(len(loop.arenas))])
        finally:
            arenas = list(loop.arenas)
            loop.close({j: 0 for j in range(len(arenas))})
        return loop, seen, arenas
    loop, seen, arenas = run(True)
    for a in adm:
        j, s, q, T = a["j"], a["slot"], a["q"], a["T"]
        first = loop.first_step(j)
        assert first == before + (2 if q == 9 else 0)
        for i in range(before, first):                       # nothing yet: EMPTY records, the words move by k + 1 rows
            assert seen[i]["toks"][j] == [] and int(seen[i]["st"]["len"][s]) == T + (i - before + 1) * (K + 1)
        assert len(seen[first]["toks"][j]) == 1
        g = seen[first]["toks"][j][0]
        # (a) the logits of the last question row against the oracle over the staged rows and the question
        pos = list(range(a["pos0"], a["pos0"] + q))
        _, S0, (olog, present) = eo.cached_prefill(model, lib, a["used"], a["ids"], pos, 2048)
        assert S0 == T
        row = s * (K + 1) + (q - 1) % (K + 1)
        got = seen[first]["logits"][row]
        err = float(np.abs(got - olog[0, -1]).max())
        print(f"[{name} loop prefill q={q}] last question row vs LlamaOracle: max|dlogit| = {err:.2e}")
        assert err < LOGIT_TOL, (q, err)
        otok, margin, _ = lsr.draw(olog[0, -1], a["ids"], a["tuple"], a["seed"], 0)
        if margin > (2 * LOGIT_TOL if a["params"] is None else 2 * LOGIT_TOL / 0.7):
            assert g == otok, (q, g, otok, margin)
        # (b) the appended rows [T, T + q) against the oracle's K / V
        buf = arenas[j].buf[0, :, :, :, T:T + q].float().cpu().numpy()
        kerr = max(float(np.abs(buf[li, w] - present[li][w][0, :, T:T + q]).max()) for li in range(shape.num_hidden_layers) for w in (0, 1))
        print(f"[{name} loop prefill q={q}] appended K / V rows vs LlamaOracle: max|d| = {kerr:.2e}")
        assert kerr < KV_TOL, (q, kerr)
        # (c) every word but ctr equals what pc_lookup_slot_arm writes behind a serial prefill that drew the same g
        hw, hist_cap = (V + 31) // 32, loop.hist_cap
        hist = lookup_admit_history(a["corpus"] + a["ids"], g, a["max_new"] - 1, hist_cap)
        sent, handle = _sentinel_state(n, SLOTS, K, V, hist_cap)
        sampled_bits = a["params"] is not None
        f = dict(slot=s, cap=int(seen[first]["st"]["cap"][s]), kv_base=int(seen[first]["st"]["kv_base"][s]), len=T + q, pos=a["pos0"] + q, id=g,
                 leader=-1, trunk=0, budget=a["max_new"] - 1, counter=0, seed=a["seed"], params=a["tuple"], stop_ids=a["stops"],
                 bits=lsr.history_bits(a["ids"] + [g], V) if sampled_bits else np.zeros(hw, dtype=np.uint32))
        host = _pinned(lsv.lookup_arm_block_bytes(n, hw, hist, **f))
        n.lookup_slot_arm(host, n.lookup_slot_arm_bytes(hw, len(hist)), handle, SLOTS, K, hist_cap)
        torch.cuda.synchronize()
        st = seen[first]["st"]
        L = len(hist)
        assert int(st["hist_len"][s]) == L == int(sent["hist_len"][s]) and st["hist"][s, :L].tolist() == sent["hist"][s, :L].tolist() == hist
        for w, w2 in (("len", "len"), ("budget", "budget"), ("draws", "draws"), ("cap", "cap"), ("kv_base", "kv_base")):
            assert int(st[w][s]) == int(sent[w2][s]), (q, w)
        assert int(st["ids"][s, 0]) == int(sent["ids"][s, 0]) == g and int(st["pos"][s, 0]) == int(sent["pos"][s, 0]) == a["pos0"] + q
        # (the bitmap of a plain-greedy block is never read and the host arms it as zeros in both flows; the device sets the bit of
        # every token it emits, g included)
        want_bits = sent["bits"][s].cpu().numpy() if sampled_bits else lsr.history_bits([g], V).view(np.int32)
        assert np.array_equal(st["bits"][s], want_bits) and st["stop"][s].tolist() == sent["stop_ids"][s].tolist()
        assert int(st["forced"][s]) == 0 and int(st["live"][s]) == int(sent["live"][s]) == 1
        assert seen[total - 1]["st"]["len"][s] > T + q        # ... and it decodes on from there
    # (d) the two decoding neighbours emit what they emit when slots 2 and 3 stay idle
    _, alone, _ = run(False)
    for i in range(total):
        assert seen[i]["toks"][:2] == alone[i]["toks"][:2], i
    assert sum(len(seen[i]["toks"][0]) for i in range(total)) >= total


# ---- (e) - (g): serve(loop_prefill=True) -------------------------------------------------------------------------------------------
def _requests(prompts):
    """7 requests of 5..20 tokens: plain greedy, two sampled chains and greedy with a penalty in turn (tests/test_gpu_lookup_serve)."""
    from promptcache_amd.generation_engine import GenerationParameters as G
    kinds = [dict(temperature=0.0), dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40), dict(temperature=0.0),
             dict(temperature=1.3, repetition_penalty=1.3, top_p=0.8, top_k=12), dict(temperature=0.0, repetition_penalty=1.2),
             dict(temperature=0.0), dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40)]
    return [(p, G(max_new_tokens=mn, **kw)) for p, mn, kw in zip(prompts, MAX_NEW7, kinds)]


def _count_new_entries(monkeypatch):
    from promptcache_amd import _native
    calls = []
    for name in ("lookup_slot_arm_prompt", "lookup_draft_slots_prompt", "lookup_verify_slots_prompt"):
        real = getattr(_native, name)

        def shim(*a, _real=real, _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(_native, name, shim)
    return calls


def test_serve_with_loop_prefill_against_serve(monkeypatch):
    """7 mixed requests through 3 slots.  serve(lookup=3) is the reference leg; the oracle is fed ITS tokens and says how far each
    request's decisions are no near-tie (3.22's margins: 2e-2 greedy, 2 * 1e-2 / T sampled); over that prefix the in-loop leg must
    emit the same tokens.  (g) rides along: with the mode off no new entry is called and stats / trace have today's shape."""
    from promptcache_amd.generation_engine import GenerationEngine
    shape, lm, eng, prompts = _setup("mid", 3)
    ge = GenerationEngine(lm)
    reqs = _requests(prompts)
    calls = _count_new_entries(monkeypatch)
    torch.manual_seed(5)
    seed0 = int(torch.randint(0, 2 ** 62, (1,)))
    torch.manual_seed(5)
    _collect(ge.serve(eng, iter(reqs), lookup=K))
    serial = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    serial_trace = list(ge.last_serve_trace)
    assert calls == [] and sorted(ge.last_serve_stats) == ["live_rows", "replays", "requests", "rows", "steps", "tokens"]      # (g)
    assert [len(serial[r]) for r in range(7)] == MAX_NEW7
    torch.manual_seed(5)
    outs = _collect(ge.serve(eng, iter(reqs), lookup=K, loop_prefill=True))
    tokens = {r: list(t) for r, t in ge.last_serve_tokens.items()}
    stats = ge.last_serve_stats
    print(f"[serve loop_prefill] {stats}")
    assert stats["loop_prefills"] + stats["step_prefills"] == 7 and stats["step_prefills"] >= 3 and stats["loop_prefills"] >= 1
    assert set(calls) == {"lookup_slot_arm_prompt", "lookup_draft_slots_prompt", "lookup_verify_slots_prompt"}
    assert calls.count("lookup_slot_arm_prompt") == stats["loop_prefills"]
    assert [t[1] for t in ge.last_serve_trace if t[0] == "pull"] == [t[1] for t in serial_trace if t[0] == "pull"] == list(range(7))
    assert [len(tokens[r]) for r in range(7)] == MAX_NEW7 and lm.hf_model._live_loop is None
    for r in range(7):
        assert outs[r][0].elapsed_time > 0.0 and outs[r][-1].new_text == lm.decode(tokens[r]), r
    model, lib = _oracle(shape, lm.hf_model, eng)
    sure = {}
    for r, (prompt, p) in enumerate(reqs):
        ids, pos, _, cache = eng.process(prompt, slot=0)
        used = [mm.token_sequence for mm in eng.slot_cache(0).staged]
        _, S0, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, 2048)
        prm = (p.temperature, p.repetition_penalty, p.top_p, p.top_k)
        bar = 2 * LOGIT_TOL if p.greedy else 2 * LOGIT_TOL / p.temperature
        hist, n_sure, position = list(ids), 0, max(pos) + 2
        for j, tok in enumerate(serial[r]):
            otok, margin, _ = sr.draw(olog[0, -1], hist, *prm, seed0 + r, j)
            if otok != tok or margin <= bar:
                break
            n_sure += 1
            hist.append(tok)
            olog, present = model.forward(np.array([[tok]]), np.array([[position + j]]), past=present)
        sure[r] = n_sure
    compared = sum(sure.values())
    print(f"[serve loop_prefill] comparable prefixes {[sure[r] for r in range(7)]} of {MAX_NEW7}")
    # a condition on the inputs (W_SEED): every request's first token and at least a third of all tokens are decided by the margin
    assert all(sure[r] >= 1 for r in range(7)) and 3 * compared >= sum(MAX_NEW7), sure
    for r in range(7):
        assert tokens[r][:sure[r]] == serial[r][:sure[r]], (r, sure[r], tokens[r], serial[r])


def test_share_trunk_is_token_for_token_the_unshared_run(monkeypatch):
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters
    monkeypatch.setenv("PC_SLOT_TRUNK_MIN", "1")
    monkeypatch.setenv("PC_TRUNK_VERIFY", "1")
    shape, lm, eng, prompts = _setup("mid", 3)
    ge = GenerationEngine(lm)
    max_new = [4, 14, 16, 8, 6, 9]

    def run(share):
        reqs = [(p, GenerationParameters(temperature=0.0, max_new_tokens=mn)) for p, mn in zip(prompts, max_new)]
        kinds = set()
        for r, o in ge.serve(eng, reqs, lookup=K, loop_prefill=True, share_trunk=share):
            loop = lm.hf_model._live_loop
            if loop is not None:
                kinds.add((loop.prompt_rows, loop.nsplit_trunk > 0))
        return {r: list(t) for r, t in ge.last_serve_tokens.items()}, kinds, dict(ge.last_serve_stats)
    unshared, kinds, stats = run(False)
    assert kinds == {(True, False)} and stats["loop_prefills"] >= 1
    shared, kinds, stats2 = run(True)
    assert kinds == {(True, True)} and stats2["loop_prefills"] == stats["loop_prefills"]
    assert shared == unshared and [len(shared[r]) for r in range(6)] == max_new
