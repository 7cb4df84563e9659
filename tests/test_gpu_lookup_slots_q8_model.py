"""Prompt-lookup drafts over int8 K / V images in the batched slot loop on the GPU (LlamaHIP.lookup_slot_loop(kv="int8"),
DESIGN 3.29): every draft row's logits against the numpy oracle run ONE TOKEN AT A TIME over the device's dequantised image rows
[0, len + i) with the row's own K / V exact, the images bit for bit against tests/kv_q8_ref.py of the fp16 arenas after every
replay; keep_arenas=False against keep_arenas=True bit for bit with the shared prefill arena overwritten (fp16 and MXFP4
weights); GenerationEngine.serve(lookup=3, slot_kv="int8") against serve(slot_kv="int8") where the oracle's margin decides; and
the mode off launching neither new entry."""
import numpy as np
import pytest
import torch

from tests import sample_ref as sr
from tests.test_gpu_lookup_serve import _oracle
from tests.test_gpu_slots import LOGIT_TOL, _collect, _prefill
from tests.test_gpu_slots_q8_model import MAX_CTX, _assert_image_is_the_quantised_arena, _build
from tests.test_gpu_slots_q8_only_model import _first, _image_rows

pytestmark = pytest.mark.gpu
K, STEPS = 3, 8
BUDGET = STEPS * (K + 1) + 8          # no sequence runs out of budget inside STEPS replays


@pytest.fixture(scope="module")
def mid4():
    return _build("mid", 4, 13)


def _four(lm, eng, prompts):
    """The four prompts prefilled in slots 0..3 -> (pasts, first tokens, positions, lengths, prompt ids)."""
    pasts, toks, poss, lens, idss = [], [], [], [], []
    for j in range(4):
        ids, pos, out = _prefill(lm, eng, prompts[j], j)
        pasts.append(out.past_key_values)
        toks.append(int(torch.argmax(out.logits[0, -1])))            # the device leads from the first token on
        poss.append(max(pos) + 2)
        lens.append(out.past_key_values.arena.length)
        idss.append(list(ids))
    return pasts, toks, poss, lens, idss


@pytest.fixture(scope="module")
def answers(mid4):
    """What every sequence goes on to say under the int8 lookup loop (drafting from its prompt alone), first token included: a
    corpus that ends in it makes most drafts right, so steps append rows that LATER steps read from the image."""
    _, _, lm, eng, prompts, _ = mid4
    pasts, toks, poss, _, idss = _four(lm, eng, prompts)
    loop = lm.hf_model.lookup_slot_loop(pasts, toks, poss, BUDGET, K, idss, kv="int8")
    said = [[t] for t in toks]
    try:
        for _ in range(BUDGET):
            i = loop.enqueue()
            for j in range(4):
                said[j] += loop.tokens(j, i)
    finally:
        loop.close([0] * 4)
    assert all(len(s) == BUDGET + 1 for s in said)
    return said


def test_every_draft_row_against_the_oracle_one_token_at_a_time(mid4, answers):
    from promptcache_amd.model.llama_hip import LookupSlotLoopQ8
    shape, w16, lm, eng, prompts, _ = mid4
    m = lm.hf_model
    model, _ = _oracle(shape, w16, m, eng)
    pasts, toks, poss, lens, idss = _four(lm, eng, prompts)
    assert len(set(lens)) == 4, lens                                  # ragged slots
    corpora = [ids[-8:] + said for ids, said in zip(idss, answers)]
    loop = m.lookup_slot_loop(pasts, toks, poss, BUDGET, K, corpora, kv="int8")
    assert type(loop) is LookupSlotLoopQ8 and loop.S == 4 and loop.qcap >= max(lens) + BUDGET + K + 2
    worst, accepted = 0.0, 0
    nl = shape.num_hidden_layers
    try:
        for i in range(STEPS):
            loop.enqueue()
            torch.cuda.synchronize()
            dev_logits = loop.logits.cpu().numpy()
            ids_d, pos_d = loop.st["ids"].cpu().numpy(), loop.st["pos"].cpu().numpy()
            for j in range(4):
                got = loop.tokens(j, i)
                assert 1 <= len(got) <= K + 1
                accepted += len(got) - 1
                # the rows this replay fed: the sequence's token, then the drafts / pads the draft launch left (the verify launch
                # rewrites word 0 only)
                row_ids = [toks[j]] + [int(t) for t in ids_d[j, 1:]]
                row_pos = [poss[j]] + [int(p) for p in pos_d[j, 1:]]
                assert row_pos == [poss[j] + r for r in range(K + 1)]
                c, s = _assert_image_is_the_quantised_arena(loop, j, lens[j] + len(got), f"after replay {i}")
                for r in range(K + 1):                               # the image rows in front of row r, quantised; its own row exact
                    n = lens[j] + r
                    deq = c[:, :, :, :n].astype(np.float32) * s[:, :, :, :n, None]
                    past = [(deq[l, 0][None], deq[l, 1][None]) for l in range(nl)]
                    olog, _ = model.forward(np.array([[row_ids[r]]]), np.array([[row_pos[r]]]), past=past)
                    err = float(np.abs(dev_logits[j * (K + 1) + r] - olog[0, -1]).max())
                    worst = max(worst, err)
                    assert err < LOGIT_TOL, (i, j, r, err)
                for r, t in enumerate(got):                          # greedy: an emitted token is its row's argmax
                    assert t == int(np.argmax(dev_logits[j * (K + 1) + r])), (i, j, r)
                toks[j], poss[j], lens[j] = got[-1], poss[j] + len(got), lens[j] + len(got)
    finally:
        loop.close([ln - l0 for ln, l0 in zip(lens, loop.len0)])
    print(f"[mid, 4 layers] LookupSlotLoopQ8, 4 ragged slots, k = {K}, {STEPS} replays ({accepted} drafts accepted), every row against "
          f"the oracle over the device's dequantised image rows: max|dlogit| = {worst:.2e}")
    assert [a.length for a in loop.arenas] == lens
    assert accepted >= STEPS                                          # (on the inputs: later steps read rows that drafts appended)


def _replays(loop, lens):
    """STEPS replays -> per replay (logits, ring records, written image rows of every slot); ``lens`` follows the records."""
    lens, got = list(lens), []
    for i in range(STEPS):
        loop.enqueue()
        torch.cuda.synchronize()
        recs = [loop.tokens(j, i) for j in range(4)]
        got.append((loop.logits.clone(), recs, [_image_rows(loop, j, lens[j] + K + 1) for j in range(4)]))
        lens = [n + len(r) for n, r in zip(lens, recs)]
    return got, lens


def _one_arena_vs_four(lm, eng, prompts, said=None):
    """tests/test_gpu_slots_q8_only_model._one_arena_vs_four under the lookup step: every sequence prefilled in slot 0's arena and
    admitted into an each=True loop without arenas, against the loop over four arenas that hold the very same rows.  ``said``:
    what each sequence goes on to say (``answers``), appended to its corpus."""
    from promptcache_amd.model.llama_hip import LookupSlotLoopQ8, LookupSlotLoopQ8Only
    m = lm.hf_model
    common = dict(each=True, slots=4, max_keys=MAX_CTX, kv="int8")
    loop, entered = None, []
    for j in range(4):
        ids, pos, out = _prefill(lm, eng, prompts[j], 0)
        past, tok, p0 = out.past_key_values, int(torch.argmax(out.logits[0, -1])), max(pos) + 2
        arena = past.arena
        corpus = list(ids) + ([] if said is None else said[j])
        entered.append((arena.buf[:, :, :, :, :arena.length].clone(), arena.length, tok, p0, corpus))
        if loop is None:
            loop = m.lookup_slot_loop([past], [tok], [p0], BUDGET, K, [corpus], slot_index=[0], keep_arenas=False, **common)
            assert type(loop) is LookupSlotLoopQ8Only
        else:
            assert loop.admit(j, past, tok, p0, BUDGET, None, 0, (), (), corpus) == j
        del past, out
    lens = [e[1] for e in entered]
    assert len(set(lens)) == 4, lens
    try:
        assert all(a.buf is None for a in loop.arenas) and loop.n == 0 and int(loop.st["cap"][0]) == loop.qcap
        images, qcap = sum(t.numel() for t in loop.kvq), loop.qcap
        assert loop.slot_kv_bytes() == images + 4 * m.L * 2 * m.Hkv * (K + 1) * m.D * 2     # images + fresh rows: no arena counted
        with torch.inference_mode():
            arena.buf.view(torch.int16).fill_(0x7e00)                                    # NaN everywhere: nothing may read it
        got, lens1 = _replays(loop, lens)
    finally:
        loop.close({})
    assert m._live_loop is None and torch.all(arena.buf.view(torch.int16) == 0x7e00), "the shared arena was written"
    with torch.inference_mode():
        arena.buf.zero_()
        for t in loop.kvq:                                                               # (the loops of one model share their images)
            t.fill_(0x55)
    del loop
    pasts = []
    for j, (rows, n, _, _, _) in enumerate(entered):                                     # four arenas holding those rows
        a = _first(lm, eng, prompts[j], j)[0].arena
        with torch.inference_mode():
            a.pending = None
            a.buf[:, :, :, :, :n].copy_(rows)
            a.length = n
        pasts.append(a.views(n))
    ref = m.lookup_slot_loop(pasts, [e[2] for e in entered], [e[3] for e in entered], BUDGET, K, [e[4] for e in entered],
                             slot_index=[0, 1, 2, 3], **common)
    assert type(ref) is LookupSlotLoopQ8 and ref.qcap == qcap
    try:
        want, lens2 = _replays(ref, lens)
    finally:
        ref.close({})
    assert lens1 == lens2
    print(f"[lookup q8, one arena vs four] {sum(lens1) - sum(lens)} tokens in {STEPS} replays of 4 slots")
    for i in range(STEPS):
        (logits, recs, rows), (wlogits, wrecs, wrows) = got[i], want[i]
        assert torch.equal(logits.view(torch.int32), wlogits.view(torch.int32)), f"replay {i}: logits differ"
        assert recs == wrecs and all(recs), f"replay {i}: records differ"
        for j in range(4):
            assert torch.equal(rows[j][0], wrows[j][0]) and torch.equal(rows[j][1], wrows[j][1]), f"replay {i}: image rows of slot {j} differ"


def test_without_arenas_equals_with_arenas_bit_for_bit(mid4, answers):
    _, _, lm, eng, prompts, _ = mid4
    _one_arena_vs_four(lm, eng, prompts, answers)


def test_without_arenas_equals_with_arenas_with_mxfp4_weights():
    _, _, lm, eng, prompts, _ = _build("mid64", 3, 9, weight_format="mxfp4")
    assert lm.hf_model.w4_stream
    _one_arena_vs_four(lm, eng, prompts)


def test_serve_with_lookup_over_images_gives_the_tokens_of_the_int8_mode(mid4, monkeypatch):
    from oracle import engine_oracle as eo
    from promptcache_amd import CacheEngine
    from promptcache_amd.generation_engine import GenerationEngine, GenerationParameters as G
    shape, w16, lm, eng4, prompts, schema = mid4
    m = lm.hf_model
    ge = GenerationEngine(lm)
    budgets = [5, 12, 9, 7, 10]
    kinds = [dict(temperature=0.0), dict(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=40), dict(temperature=0.0),
             dict(temperature=0.0, repetition_penalty=1.2), dict(temperature=0.0)]
    reqs = [(p, G(max_new_tokens=mn, **kw)) for p, mn, kw in zip(prompts, budgets, kinds)]
    loops = []
    real = m.lookup_slot_loop
    monkeypatch.setattr(m, "lookup_slot_loop", lambda *a, **k: (loops.append(real(*a, **k)), loops[-1])[1])

    def run(**kw):
        eng = CacheEngine(MAX_CTX, lm, slots=2)
        eng.add_schema(schema)
        torch.manual_seed(5)
        outs = _collect(ge.serve(eng, iter(reqs), slot_kv="int8", **kw))
        return eng, outs, {r: list(t) for r, t in ge.last_serve_tokens.items()}

    torch.manual_seed(5)
    seed0 = int(torch.randint(0, 2 ** 62, (1,)))
    _, outs0, plain = run()
    assert [len(plain[r]) for r in range(5)] == budgets and not loops
    # the leading tokens at which the oracle's decision, fed the plain run's tokens, is no near-tie.  The oracle
    # keeps exact K / V, so ITS token may differ from the int8 run's; only its margin is asked: both runs compute one function
    model, lib = _oracle(shape, w16, m, eng4)
    sure = {}
    for r, (prompt, p) in enumerate(reqs):
        ids, pos, _, cache = eng4.process(prompt, slot=0)
        used = [mm.token_sequence for mm in eng4.slot_cache(0).staged]
        _, _, (olog, present) = eo.cached_prefill(model, lib, used, ids, pos, MAX_CTX)
        prm = (p.temperature, p.repetition_penalty, p.top_p, p.top_k)
        bar = 2 * LOGIT_TOL if p.greedy else 2 * LOGIT_TOL / p.temperature
        hist, n_sure, position = list(ids), 0, max(pos) + 2
        for j, tok in enumerate(plain[r]):
            _, margin, _ = sr.draw(olog[0, -1], hist, *prm, seed0 + r, j)
            if margin <= bar:
                break
            n_sure += 1
            hist.append(tok)
            olog, present = model.forward(np.array([[tok]]), np.array([[position + j]]), past=present)
        sure[r] = n_sure
    assert "lookup, k = 3" in ge.serve_plan(3, 2, slot_kv="int8")[1] and "slot_kv='int8'" in ge.serve_plan(3, 2, slot_kv="int8")[1]
    for kw, cls in ((dict(), "LookupSlotLoopQ8"), (dict(keep_arenas=False), "LookupSlotLoopQ8Only")):
        n_loops = len(loops)
        eng1, outs1, tokens = run(lookup=K, **kw)
        assert len(loops) == n_loops + 1 and type(loops[-1]).__name__ == cls and loops[-1].each and len(loops[-1].arenas) == 5
        assert [len(tokens[r]) for r in range(5)] == budgets and ge.last_serve_stats["steps"] == loops[-1].n
        for r in range(5):
            assert tokens[r][:sure[r]] == plain[r][:sure[r]], (cls, r, sure[r], tokens[r], plain[r])
            assert outs1[r][-1].new_text == lm.decode(tokens[r]), r
        assert (eng1._slot_caches[1] is None) == bool(kw)            # keep_arenas=False never allocates slot 1's arena
        assert m._live_loop is None
    print(f"[serve lookup={K}, slot_kv=int8] against serve(slot_kv=int8): comparable prefixes {[sure[r] for r in range(5)]} of {budgets}")
    # (a condition on the inputs, not on the loops: the oracle decides every request's first token and a third of all tokens --
    # random weights give near-flat logits, and a prefix ends at the first near-tie)
    assert min(sure.values()) >= 1 and 3 * sum(sure.values()) >= sum(budgets)
    images = sum(t.numel() for t in loops[-1].kvq)
    assert loops[-1].slot_kv_bytes() == images + 2 * m.L * 2 * m.Hkv * (K + 1) * m.D * 2
    with pytest.raises(ValueError, match="lookup"):                  # generate_batch keeps refusing the combination
        next(ge.generate_batch([], G(max_new_tokens=4, temperature=0.0), slot_kv="int8", lookup=K))
    with pytest.raises(ValueError, match="share_trunk"):
        next(ge.serve(eng4, iter(reqs), slot_kv="int8", lookup=K, share_trunk=True))


def test_mode_off_launches_neither_new_entry(mid4, monkeypatch):
    from promptcache_amd import _native
    _, _, lm, eng, prompts, _ = mid4
    m = lm.hf_model
    calls = []
    for name in ("rope_append_slots_rows_q8", "attn_verify_slots_q8"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    m._graphs.clear()                                                                    # (a step captured earlier would hide the launches)

    def step(lookup, **kw):
        ids, pos, out = _prefill(lm, eng, prompts[1], 0)
        past, tok, p0 = out.past_key_values, int(torch.argmax(out.logits[0, -1])), max(pos) + 2
        if lookup:
            loop = m.lookup_slot_loop([past], [tok], [p0], 6, K, [list(ids)], each=True, slots=2, max_keys=MAX_CTX, **kw)
        else:
            loop = m.slot_loop([past], [tok], [p0], 6, each=True, slots=2, max_keys=MAX_CTX, **kw)
        try:
            i = loop.enqueue()
            return loop.tokens(0, i)[0] if lookup else loop.token(0, i)
        finally:
            loop.close({0: 1})
    t8 = step(False, kv="int8")
    step(False, kv="int8", keep_arenas=False)
    step(True)
    assert calls == []
    assert step(True, kv="int8") == t8 == step(True, kv="int8", keep_arenas=False)
    assert calls.count("rope_append_slots_rows_q8") == 4 * m.L and calls.count("attn_verify_slots_q8") == 4 * m.L    # 2 x (eager + capture)
