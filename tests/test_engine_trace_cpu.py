"""Call-by-call traces of ``GenerationEngine.generate`` / ``generate_batch`` / ``serve`` over scripted fakes, compared with
``tests/golden/engine_traces.json``.  A trace holds every call the engine makes on a loop (``enqueue``, ``token`` / ``tokens``,
``elapsed_ms``, ``kill``, ``admit``, ``retire``, ``close``), on the model (``forward``, ``sample_token``, the loop factories) and
every ``Output`` it yields, in order; next to it the number of ``torch.randint`` draws.  ``token(s)`` and ``elapsed_ms`` of the SAME
step may come in either order (``_canonical``); everything else must match the recording exactly.

The recording was made with the engine as it stood BEFORE its token-stream rule and decode pumps were folded into one each:

    python -m tests.test_engine_trace_cpu --write

so a trace that differs is a change of behaviour, not of taste.  Re-record only for a change that means to alter what the host does.
"""
import json
import os
import sys
import types

import pytest

from tests.test_serve_cpu import _FakeLoop

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_traces.json")
MS = (1.0, 0.5, 0.25, 2.0, 0.125, 4.0, 0.75, 1.5, 3.0, 0.375, 8.0, 1.25)      # per-step times: every partial sum is exact


def _decode(ids):
    return " ".join(map(str, ids))


# ---- scripted loops: today's protocols, every call logged -------------------------------------------------------------------------
class _OneTokenLoop:
    """GreedyLoop / SampleLoop on the host: step i gives ``toks[i]``."""

    def __init__(self, log, toks):
        self.log, self.toks, self.n = log, list(toks), 0

    def enqueue(self):
        self.log.append(["enqueue"])
        self.n += 1

    def token(self, i):
        assert i < self.n, "the host asked for a replay it never enqueued"
        self.log.append(["token", i, self.toks[i]])
        return self.toks[i]

    def elapsed_ms(self, i):
        assert i < self.n
        self.log.append(["elapsed_ms", i, MS[i % len(MS)]])
        return MS[i % len(MS)]

    def close(self, consumed):
        self.log.append(["close", consumed])


class _MultiTokenLoop(_OneTokenLoop):
    """LookupLoop / SampleLookupLoop on the host: step i gives the list ``toks[i]`` (empty: the device budget ran out)."""
    multi = True

    def __init__(self, log, steps, k):
        super().__init__(log, steps)
        self.k = k

    token = None

    def tokens(self, i):
        assert i < self.n, "the host asked for a replay it never enqueued"
        self.log.append(["tokens", i, list(self.toks[i])])
        return list(self.toks[i])


class _LoggedSlotLoop(_FakeLoop):
    """tests/test_serve_cpu._FakeLoop (sequence k's token at its local step j is ``1000 * tag + j + 1``) with every call logged,
    scripted step times and ``off_at = {k: i}``: the device switches sequence k off at replay i (its arena is full)."""

    def __init__(self, log, tags, max_news, stops, slot_index, off_at=None):
        super().__init__(tags, max_news, stops, slot_index)
        self.log, self.off_at = log, dict(off_at or {})

    def enqueue(self):
        self.log.append(["enqueue"])
        return super().enqueue()

    def elapsed_ms(self, i):
        assert i < self.n
        self.log.append(["elapsed_ms", i, MS[i % len(MS)]])
        return MS[i % len(MS)]

    def token(self, k, i):
        t = None if k in self.off_at and i >= self.off_at[k] else super().token(k, i)
        self.log.append(["token", k, i, t])
        return t

    def kill(self, k):
        self.log.append(["kill", k])
        super().kill(k)

    def admit(self, slot, past, token, position, max_new, params, seed, history, stop_ids, trunk=None):
        k = super().admit(slot, past, token, position, max_new, params, seed, history, stop_ids, trunk=trunk)
        self.log.append(["admit", slot, past.tag, token, position, max_new, params is not None, seed, list(history), list(stop_ids), trunk, k])
        return k

    def retire(self, k, consumed):
        self.log.append(["retire", k, consumed])
        super().retire(k, consumed)

    def close(self, consumed):
        self.log.append(["close", {str(k): v for k, v in consumed.items()} if isinstance(consumed, dict) else list(consumed)])


class _LookupSlotLoop:
    """LookupSlotLoop on the host: ``steps[i][j]`` is the token list of sequence j at replay i ([]: the slot is off)."""

    def __init__(self, log, steps, k):
        self.log, self.steps, self.k, self.n, self.nsplit_trunk = log, steps, k, 0, 0

    def enqueue(self):
        self.log.append(["enqueue"])
        self.n += 1

    def elapsed_ms(self, i):
        assert i < self.n
        self.log.append(["elapsed_ms", i, MS[i % len(MS)]])
        return MS[i % len(MS)]

    def tokens(self, j, i):
        assert i < self.n, "the host asked for a replay it never enqueued"
        self.log.append(["tokens", j, i, list(self.steps[i][j])])
        return list(self.steps[i][j])

    def kill(self, j):
        self.log.append(["kill", j])

    def close(self, consumed):
        self.log.append(["close", list(consumed)])


# ---- the engine over a scripted model ---------------------------------------------------------------------------------------------
def _engine(log, hf, first, full=False, **kw):
    """``first``: cache tag -> the token list the forwards over that cache pick, one per call (the prefill, then host steps)."""
    import torch
    from promptcache_amd.generation_engine import GenerationEngine
    lm = types.SimpleNamespace(hf_model=hf, use_full_position_ids=full, decode=_decode, device="cpu")
    ge = GenerationEngine(lm, **kw)
    ge.device_greedy_loop = ge.device_sample_loop = True                # (whatever PC_DEVICE_* says in this environment)
    calls = {}

    def forward(ids, positions, past):
        tag = getattr(past, "tag", None)
        n = calls[tag] = calls.get(tag, -1) + 1
        log.append(["forward", list(ids), list(positions), tag])
        logits = torch.zeros((1, len(ids), 8192))
        want = first[tag][n]
        for tok, value in (want if isinstance(want, list) else [(want, 1.0)]):
            logits[0, -1, tok] = value
        layout = types.SimpleNamespace(layout=[])
        return logits, types.SimpleNamespace(tag=tag, arena=layout), MS[(n + 3) % len(MS)]
    ge._forward = forward
    return ge


def _cache(tag):
    return types.SimpleNamespace(tag=tag, arena=types.SimpleNamespace(B=1, layout=[]))


def _single_hf(log, loop_toks=None, steps=None, sampled_first=None, offers_lookup=True):
    """A model with the single-sequence loops: the one-token loops give ``loop_toks``, the lookup loop ``steps``."""
    def greedy_loop(past, token, position, max_new):
        log.append(["greedy_loop", past.tag, token, position, max_new])
        return _OneTokenLoop(log, loop_toks)

    def sample_loop(past, token, position, max_new, params, seed, history):
        log.append(["sample_loop", past.tag, token, position, max_new, params.temperature, seed, list(history)])
        return _OneTokenLoop(log, loop_toks)

    def lookup_loop(past, token, position, total, k_, corpus, params=None, seed=None, history_ids=None):
        log.append(["lookup_loop", past.tag, token, position, total, k_, list(corpus), params is not None, seed,
                    None if history_ids is None else list(history_ids)])
        return _MultiTokenLoop(log, steps, k_)

    def can_loop(past):
        log.append(["can_loop", past.tag])
        return True

    def sample_token(row, params, seed, history):
        log.append(["sample_token", seed, list(history)])
        return sampled_first

    hf = types.SimpleNamespace(greedy_loop=greedy_loop, sample_loop=sample_loop, can_loop=can_loop, sample_token=sample_token)
    if steps is not None:
        hf.lookup_loop = lookup_loop
        hf.lookup_available = lambda: offers_lookup
    return hf


def _params(**kw):
    from promptcache_amd.generation_engine import GenerationParameters
    kw.setdefault("temperature", 0.0)
    return GenerationParameters(**kw)


def _drain(log, gen, abandon_after=None):
    seen = 0
    for item in gen:
        index, out = item if isinstance(item, tuple) else (None, item)
        log.append(["yield", index, out.text, out.new_text, out.response_time, out.elapsed_time])
        seen += 1
        if seen == abandon_after:
            log.append(["abandon"])
            break
    gen.close()


def _generate(params, first, stream_interval=2, abandon_after=None, full=False, no_loops=False, lookup=0, lookup_sampled=False, **hf_kw):
    log = []
    hf = None if no_loops else _single_hf(log, **hf_kw)
    ge = _engine(log, hf, {None: first if isinstance(first, list) else [first]}, full=full, lookup=lookup, lookup_sampled=lookup_sampled)
    _drain(log, ge.generate([7, 8, 9], [0, 1, 5], params, None, stream_interval, use_full_position_ids=full), abandon_after)
    return log


SAMPLED = dict(temperature=0.8, top_p=0.9)
SCENARIOS = {}


def scenario(fn):
    SCENARIOS[fn.__name__.replace("__", "/")] = fn
    return fn


# ---- generate -----------------------------------------------------------------------------------------------------------------
@scenario
def generate__greedy_loop_interval_1():
    return _generate(_params(max_new_tokens=6), 100, 1, loop_toks=[101, 102, 103, 104, 105])


@scenario
def generate__greedy_loop_interval_2():
    return _generate(_params(max_new_tokens=6), 100, 2, loop_toks=[101, 102, 103, 104, 105])


@scenario
def generate__greedy_loop_interval_3():
    return _generate(_params(max_new_tokens=8), 100, 3, loop_toks=[101, 102, 103, 104, 105, 106, 107])


@scenario
def generate__sample_loop():
    return _generate(_params(max_new_tokens=5, **SAMPLED), 0, 1, loop_toks=[201, 202, 203, 204], sampled_first=200)


@scenario
def generate__penalised_greedy_takes_the_sample_loop():
    return _generate(_params(max_new_tokens=4, repetition_penalty=1.2), 0, 2, loop_toks=[201, 202, 203], sampled_first=200)


@scenario
def generate__lookup_k3_steps_4_1_0_2():
    return _generate(_params(max_new_tokens=12), 300, 2, lookup=3, loop_toks=[], steps=[[301, 302, 303, 304], [305], [], [306, 307]])


@scenario
def generate__lookup_k3_to_the_budget():
    return _generate(_params(max_new_tokens=9), 300, 2, lookup=3, loop_toks=[], steps=[[301, 302, 303, 304], [305], [306, 307], [308], [309]])


@scenario
def generate__lookup_k20_is_taken_as_15():
    return _generate(_params(max_new_tokens=4), 300, 2, lookup=20, loop_toks=[], steps=[[301, 302], [303]])


@scenario
def generate__lookup_sampled_k3():
    return _generate(_params(max_new_tokens=8, **SAMPLED), 0, 2, lookup=3, lookup_sampled=True, sampled_first=400, loop_toks=[],
                     steps=[[401, 402], [403, 404, 405, 406], [407]])


@scenario
def generate__lookup_sampled_off_keeps_the_sample_loop():
    return _generate(_params(max_new_tokens=3, **SAMPLED), 0, 2, lookup=3, sampled_first=400, loop_toks=[401, 402], steps=[[9]])


@scenario
def generate__max_new_1():
    return _generate(_params(max_new_tokens=1), 100, 2, loop_toks=[])


@scenario
def generate__max_new_1_sampled():
    return _generate(_params(max_new_tokens=1, **SAMPLED), 0, 2, loop_toks=[], sampled_first=200)


@scenario
def generate__max_new_2():
    return _generate(_params(max_new_tokens=2), 100, 2, loop_toks=[101])


@scenario
def generate__max_new_2_lookup():
    return _generate(_params(max_new_tokens=2), 100, 2, lookup=3, loop_toks=[], steps=[[101], [102]])


@scenario
def generate__stop_id_mid_stream():
    return _generate(_params(max_new_tokens=10, stop_token_ids=[103, 999]), 100, 3, loop_toks=[101, 102, 103, 104, 105, 106, 107, 108, 109])


@scenario
def generate__stop_id_at_the_first_token():
    return _generate(_params(max_new_tokens=10, stop_token_ids=[100]), 100, 3, loop_toks=[101, 102])


@scenario
def generate__stop_id_inside_a_multi_token_step():
    return _generate(_params(max_new_tokens=12, stop_token_ids=[303]), 300, 2, lookup=3, loop_toks=[],
                     steps=[[301], [302, 303, 304, 305], [306]])


@scenario
def generate__stop_string_across_two_tokens():
    # "7 8" completes with token 8; after token 7 the tail "7" may still grow into it: that streaming point yields nothing
    return _generate(_params(max_new_tokens=10, stop_str=["7 8"]), 5, 1, loop_toks=[6, 7, 8, 9, 10, 11, 12, 13, 14])


@scenario
def generate__stop_string_inside_a_multi_token_step():
    return _generate(_params(max_new_tokens=10, stop_str=["7 8"]), 5, 1, lookup=3, loop_toks=[], steps=[[6, 7], [8, 9, 10], [11]])


@scenario
def generate__host_stepped_greedy():
    return _generate(_params(max_new_tokens=5), [100, 101, 102, 103, 104], 2, no_loops=True)


@scenario
def generate__host_stepped_stop_id():
    return _generate(_params(max_new_tokens=6, stop_token_ids=[102]), [100, 101, 102, 103, 104, 105], 3, no_loops=True)


@scenario
def generate__host_stepped_penalised():
    # 8 is in the prompt: its logit 1.0 / 1.2 falls under 0.9, so the penalty (and the history it is given) decides every token
    steps = [[(8, 1.0), (20, 0.9)], [(20, 1.0), (21, 0.9)], [(21, 1.0), (8, 0.95), (22, 0.9)], [(23, 1.0)]]
    return _generate(_params(max_new_tokens=4, repetition_penalty=1.2), steps, 1, no_loops=True)


@scenario
def generate__full_position_ids():
    return _generate(_params(max_new_tokens=4), [100, 101, 102, 103], 2, full=True, loop_toks=[901, 902, 903])


@scenario
def generate__abandoned_after_the_second_yield():
    return _generate(_params(max_new_tokens=8), 100, 2, abandon_after=2, loop_toks=[101, 102, 103, 104, 105, 106, 107])


@scenario
def generate__abandoned_inside_a_multi_token_step():
    return _generate(_params(max_new_tokens=12), 300, 1, abandon_after=3, lookup=3, loop_toks=[],
                     steps=[[301, 302, 303, 304], [305, 306], [307]])


# ---- generate_batch -------------------------------------------------------------------------------------------------------------
def _batch_hf(log, off_at=None, lookup_steps=None, sampled_firsts=None, refuse_lookup=False):
    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, share_trunk=False):
        log.append(["slot_loop", [p.tag for p in pasts], list(tokens), list(positions), max_new, params is not None, list(seeds),
                    [list(h) for h in histories], list(stop_ids), share_trunk])
        n = len(pasts)
        return _LoggedSlotLoop(log, [p.tag for p in pasts], [max_new] * n, [list(stop_ids)] * n, list(range(n)), off_at)

    def lookup_slot_loop(pasts, tokens, positions, max_new, k, corpora, stop_ids=(), share_trunk=False):
        log.append(["lookup_slot_loop", [p.tag for p in pasts], list(tokens), list(positions), max_new, k, [list(c) for c in corpora],
                    list(stop_ids), share_trunk])
        return None if refuse_lookup else _LookupSlotLoop(log, lookup_steps, k)

    def sample_token(row, params, seed, history):
        log.append(["sample_token", seed, list(history)])
        return sampled_firsts[history[0]]

    hf = types.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True, sample_token=sample_token)
    if lookup_steps is not None or refuse_lookup:
        hf.lookup_slot_loop = lookup_slot_loop
    return hf


def _batch(params, firsts, stream_interval=2, abandon_after=None, lookup=0, **hf_kw):
    """Request r is prompt [r + 1] at positions [10 + r] over cache tag r + 1; ``firsts[r]``: its first token."""
    log = []
    ge = _engine(log, _batch_hf(log, **hf_kw), {r + 1: [t] for r, t in enumerate(firsts)})
    reqs = [([r + 1], [10 + r], _cache(r + 1)) for r in range(len(firsts))]
    _drain(log, ge.generate_batch(reqs, params, stream_interval, lookup=lookup, share_trunk=False), abandon_after)
    return log


@scenario
def batch__slot_loop_four_endings():
    # sequence 0: the stop id 1003; 1: the stop string "2002 2003" (the host kills the slot); 2: off on the device at replay 2; 3: the budget
    p = _params(max_new_tokens=7, stop_token_ids=[1003], stop_str=["2002 2003"])
    return _batch(p, [1000, 2000, 3000, 4000], 2, off_at={2: 2})


@scenario
def batch__slot_loop_sampled():
    p = _params(max_new_tokens=4, stop_token_ids=[2002], **SAMPLED)
    return _batch(p, [0, 0, 0], 1, sampled_firsts={1: 1000, 2: 2000, 3: 3000})


@scenario
def batch__lookup_slot_loop_k2():
    # sequence 0: to the budget, which cuts its last step; 1: the stop id 2003 inside a step; 2: the stop string "3002 3003" (the host
    # kills the slot); 3: an empty record at replay 1 (the device switched the slot off)
    p = _params(max_new_tokens=8, stop_token_ids=[2003], stop_str=["3002 3003"])
    steps = [[[1001, 1002, 1003], [2001], [3001, 3002], [4001]],
             [[1004, 1005], [2002, 2003, 2004], [3003, 3004, 3005], []],
             [[1006, 1007, 1008], [], [], []],
             [[1009], [], [], []]]
    return _batch(p, [1000, 2000, 3000, 4000], 2, lookup=2, lookup_steps=steps)


@scenario
def batch__lookup_slot_loop_empty_record_ends_a_sequence():
    p = _params(max_new_tokens=8)
    steps = [[[1001], [2001, 2002]], [[1002], []], [[1003, 1004, 1005], [2003]], [[1006, 1007, 1008], [2004]]]
    return _batch(p, [1000, 2000], 3, lookup=2, lookup_steps=steps)


@scenario
def batch__refused_lookup_loop_falls_back_to_the_slot_loop():
    return _batch(_params(max_new_tokens=3), [1000, 2000], 2, lookup=20, refuse_lookup=True)


@scenario
def batch__one_sequence_ends_at_its_first_token():
    return _batch(_params(max_new_tokens=4, stop_token_ids=[2000]), [1000, 2000, 3000], 2)


@scenario
def batch__all_sequences_end_at_their_first_token():
    return _batch(_params(max_new_tokens=4, stop_token_ids=[1000, 2000]), [1000, 2000], 2)


@scenario
def batch__abandoned():
    return _batch(_params(max_new_tokens=9), [1000, 2000], 1, abandon_after=5)


@scenario
def batch__abandoned_lookup():
    steps = [[[1001, 1002], [2001]], [[1003], [2002, 2003]], [[1004], [2004]]]
    return _batch(_params(max_new_tokens=9), [1000, 2000], 1, abandon_after=6, lookup=2, lookup_steps=steps)


def _logged_generate(log):
    from promptcache_amd.generation_engine import Output

    def generate(token_ids, position_ids, params, cache, stream_interval, use_full_position_ids=False):
        log.append(["generate", list(token_ids), list(position_ids), params.max_new_tokens, getattr(cache, "tag", None), stream_interval,
                    use_full_position_ids])
        yield Output(f"t{token_ids[0]}", "a", 1.0, 0.5)
        yield Output(f"t{token_ids[0]}", "a b", 1.5, 0.5)
    return generate


@scenario
def batch__fallback_through_generate():
    log = []
    ge = _engine(log, types.SimpleNamespace(), {})                        # a model without slot_loop
    ge.generate = _logged_generate(log)
    reqs = [([r + 1], [10 + r], _cache(r + 1)) for r in range(2)]
    _drain(log, ge.generate_batch(reqs, _params(max_new_tokens=5, **SAMPLED), 3))
    return log


# ---- serve ------------------------------------------------------------------------------------------------------------------
def _serve(slots, reqs, default=None, stream_interval=2, abandon_after=None, sampled_firsts=None, hf=True):
    """Request r is prompt r + 1 (cache tag r + 1, first token ``1000 * (r + 1)``, loop tokens ``1000 * (r + 1) + j``), pulled lazily."""
    log = []

    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, slots=None, slot_index=None, each=False,
                  max_keys=None, trunks=None):
        log.append(["slot_loop", [p.tag for p in pasts], list(tokens), list(positions), list(max_new), [p is not None for p in params],
                    list(seeds), [list(h) for h in histories], [list(s) for s in stop_ids], slots, list(slot_index), each, max_keys, trunks])
        return _LoggedSlotLoop(log, [p.tag for p in pasts], max_new, stop_ids, slot_index)

    def sample_token(row, params, seed, history):
        log.append(["sample_token", seed, list(history)])
        return sampled_firsts[history[0]]

    model = types.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True, sample_token=sample_token) if hf else None
    ge = _engine(log, model, {r + 1: [1000 * (r + 1)] for r in range(len(reqs))})
    if not hf:
        ge.generate = _logged_generate(log)

    def process(prompt, slot=0, return_full_position_ids=False):
        log.append(["process", prompt, slot])
        return [prompt], [10 + prompt], 0.0, _cache(prompt)

    def lazy():
        for r, req in enumerate(reqs):
            log.append(["pull", r])
            yield req
    ce = types.SimpleNamespace(process=process, slots=slots, max_ctx_length=4096)
    _drain(log, ge.serve(ce, lazy(), default, stream_interval=stream_interval, share_trunk=False), abandon_after)
    if hf:
        log.append(["stats", ge.last_serve_stats, {str(r): t for r, t in ge.last_serve_tokens.items()}, [list(t) for t in ge.last_serve_trace]])
    return log


@scenario
def serve__five_requests_through_two_slots():
    # 0: the default params; 1: ends at its first token; 2: nine stop ids, the ninth (3003) fires -- the device holds eight;
    # 3: sampled, with a stop string; 4: sampled, to its budget
    nine = [90001 + j for j in range(8)] + [3003]
    reqs = [1, (2, _params(max_new_tokens=1)), (3, _params(max_new_tokens=9, stop_token_ids=nine)),
            (4, _params(max_new_tokens=9, stop_str=["4002 4003"], **SAMPLED)), (5, _params(max_new_tokens=3, **SAMPLED))]
    return _serve(2, reqs, _params(max_new_tokens=6, stop_token_ids=[1004]), 2, sampled_firsts={4: 4000, 5: 5000})


@scenario
def serve__first_fill_ends_at_first_tokens():
    reqs = [(1, _params(max_new_tokens=1)), (2, _params(max_new_tokens=4, stop_token_ids=[2000])), (3, _params(max_new_tokens=3)),
            (4, _params(max_new_tokens=1))]
    return _serve(2, reqs, None, 1)


@scenario
def serve__abandoned():
    reqs = [(r + 1, _params(max_new_tokens=9)) for r in range(3)]
    return _serve(2, reqs, None, 1, abandon_after=8)


@scenario
def serve__fallback_through_generate():
    return _serve(2, [1, (2, _params(max_new_tokens=9)), (3, None)], _params(max_new_tokens=3), 3, hf=False)


# ---- recording and comparing ------------------------------------------------------------------------------------------------------
def record(name):
    """-> {"log": the scenario's trace, "randint": draws it took from torch's default generator} (seeds are 10 ** 6 * draw number)."""
    import torch
    real, draws = torch.randint, []

    def randint(*a, **kw):
        draws.append(a)
        return torch.tensor([10 ** 6 * len(draws)])
    torch.randint = randint
    try:
        log = SCENARIOS[name]()
    finally:
        torch.randint = real
    return json.loads(json.dumps({"log": log, "randint": len(draws)}))


def _canonical(log):
    """``elapsed_ms`` of a step moved in front of the ``token`` / ``tokens`` reads of that step it stands among."""
    out, i = [], 0
    while i < len(log):
        j = i
        while j < len(log) and log[j][0] in ("token", "tokens", "elapsed_ms") and log[j][-2] == log[i][-2]:
            j += 1                                                        # (the step is the last argument: the entry before the result)
        if j == i:
            out.append(log[i])
            i += 1
            continue
        run = log[i:j]
        out += [e for e in run if e[0] == "elapsed_ms"] + [e for e in run if e[0] != "elapsed_ms"]
        i = j
    return out


def test_every_scenario_is_recorded():
    with open(FIXTURE) as f:
        assert sorted(json.load(f)) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_engine_trace_matches_the_recording(name):
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got = record(name)
    assert got["randint"] == want["randint"]
    a, b = _canonical(got["log"]), _canonical(want["log"])
    for n, (x, y) in enumerate(zip(a, b)):
        assert x == y, f"{name}: entry {n}: {x} != {y} (after {a[max(0, n - 3):n]})"
    assert len(a) == len(b), f"{name}: {len(a)} entries, recorded {len(b)}; the longer one goes on with {(a + b)[min(len(a), len(b))]}"


def test_canonical_only_moves_elapsed_ms_within_its_step():
    log = [["enqueue"], ["token", 0, 2, 7], ["elapsed_ms", 2, 1.0], ["token", 1, 2, 8], ["yield", 0, "", "", 0, 0], ["token", 2, 2, 9],
           ["elapsed_ms", 3, 1.0], ["tokens", 3, [1]], ["kill", 0]]
    assert _canonical(log) == [["enqueue"], ["elapsed_ms", 2, 1.0], ["token", 0, 2, 7], ["token", 1, 2, 8], ["yield", 0, "", "", 0, 0],
                               ["token", 2, 2, 9], ["elapsed_ms", 3, 1.0], ["tokens", 3, [1]], ["kill", 0]]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python -m tests.test_engine_trace_cpu --write")
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "prompt-cache_amd")]
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(name)}: {json.dumps(record(name))}" for name in sorted(SCENARIOS)) + "\n}\n")
    print(f"{len(SCENARIOS)} scenarios -> {FIXTURE}")
