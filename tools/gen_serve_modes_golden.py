"""Characterise which loop ``GenerationEngine.serve`` / ``serve_plan`` / ``generate_batch`` / ``batch_plan`` choose, and what they refuse
with which words, over the full product of their mode arguments, the environment and what a model offers.

Only the four public entry points are driven, over stubs, on the CPU: ``serve`` gets an empty request list (an accepted call simply
ends), ``generate_batch`` gets caches that are batch-1 arenas of their own and an engine whose ``_first_token`` / ``generate`` raise a
marker (the outcome says which one the call reached), and the stub model's ``slot_loop`` / ``lookup_slot_loop`` raise AssertionError:
nothing may be asked of the model before a refusal.  So the same code runs on any commit:

    python tools/gen_serve_modes_golden.py            # writes tests/golden/serve_modes.json from the package on the path
    python tools/gen_serve_modes_golden.py --check    # compares instead

``tests/test_serve_modes_cpu.py`` replays the recording.  The fixture is written ONCE per change of behaviour, from the commit whose
behaviour is to be kept (``PYTHONPATH`` pointing at that commit's package), never from the code under test."""
from __future__ import annotations

import contextlib
import gc
import itertools
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "serve_modes.json")
ENTRIES = ("serve", "serve_plan", "generate_batch", "batch_plan")
ENV_NAMES = ("PC_SLOT_KV", "PC_SLOT_KEEP_ARENAS", "PC_SLOT_TRUNK", "PC_SERVE_LOOKUP", "PC_SLOT_LOOKUP", "PC_SERVE_LOOP_PREFILL")
# one character per outcome index in the fixture's strings
ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz!#$%&()*+,-./:;<=>?@[]^_{|}~"

# the full product, in this order (the last axis runs fastest)
AXES = {
    "model": ["everything", "no_lookup_q8", "no_lookup", "head_dim_64", "no_loop"],
    "PC_SLOT_KV": [None, "int8"],
    "PC_SLOT_KEEP_ARENAS": [None, "0"],
    "slots": [4, 16],                                  # serve: the slot count; generate_batch / batch_plan: the request count
    "slot_kv": [None, "fp16", "int8", "fp8"],
    "share_trunk": [False, True],
    "lookup": [0, 3, 20],
    "keep_arenas": [None, True, False],
    "loop_prefill": [None, False, True],
}
# ... and rows beside it: each is one setting crossed with SUB_AXES (None arguments read the environment) and its models
SUB_AXES = {
    "slot_kv": [None, "int8"],
    "share_trunk": [None, True],
    "lookup": [None, 3],
    "keep_arenas": [None, False],
    "loop_prefill": [None, True],
}
BOTH = ["everything", "no_lookup"]
ROWS = [
    dict(name="nothing set", models=BOTH + ["lookup_says_no", "loop_method_only", "no_model"]),
    dict(name="PC_DEVICE_GREEDY=0", models=BOTH, engine=dict(device_greedy_loop=False)),
    dict(name="PC_DEVICE_SAMPLE=0", models=BOTH, engine=dict(device_sample_loop=False)),
    dict(name="PC_DEVICE_SAMPLE=0, sampled params", models=BOTH, engine=dict(device_sample_loop=False), params="sampled"),
    dict(name="use_full_position_ids", models=BOTH, lm=dict(use_full_position_ids=True)),
    dict(name="PC_SLOT_KEEP_ARENAS=2", models=BOTH, env={"PC_SLOT_KEEP_ARENAS": "2"}),
    dict(name="PC_SLOT_KEEP_ARENAS=1", models=BOTH, env={"PC_SLOT_KEEP_ARENAS": "1"}),
    dict(name="PC_SERVE_LOOP_PREFILL=1", models=BOTH, env={"PC_SERVE_LOOP_PREFILL": "1"}),
    dict(name="PC_SLOT_TRUNK=1", models=BOTH + ["no_lookup_trunk"], env={"PC_SLOT_TRUNK": "1"}),
    dict(name="share_trunk without the verify step", models=["no_lookup_trunk"]),
    dict(name="PC_SERVE_LOOKUP=3", models=BOTH, env={"PC_SERVE_LOOKUP": "3"}),
    dict(name="PC_SERVE_LOOKUP=20, 16 slots", models=BOTH, env={"PC_SERVE_LOOKUP": "20"}, slots=16),
    dict(name="PC_SLOT_LOOKUP=3", models=BOTH, env={"PC_SLOT_LOOKUP": "3"}),
    dict(name="PC_SLOT_KV=fp8", models=BOTH, env={"PC_SLOT_KV": "fp8"}),
    dict(name="PC_SLOT_KV=int8, PC_SLOT_KEEP_ARENAS=0, PC_SERVE_LOOKUP=3", models=BOTH + ["no_lookup_q8"],
         env={"PC_SLOT_KV": "int8", "PC_SLOT_KEEP_ARENAS": "0", "PC_SERVE_LOOKUP": "3"}),
    dict(name="sampled params", models=BOTH, params="sampled"),
    dict(name="nine stop ids", models=BOTH, params="nine_stops"),
    dict(name="max_new_tokens=1", models=BOTH, params="one_token"),
    dict(name="no requests", models=BOTH, slots=0),
    dict(name="17 requests", models=BOTH, slots=17),
    dict(name="two caches in one arena", models=BOTH, caches="shared"),
    dict(name="caches without an arena", models=BOTH, caches="none"),
]


class Reached(Exception):
    """generate_batch got as far as running something."""


def _model(kind: str):
    def refuse(*a, **kw):
        raise AssertionError("the stub model was asked for a loop")
    if kind == "no_model":
        return None
    hf = types.SimpleNamespace(slot_loop=refuse, slot_loop_available=lambda: kind != "no_loop", lookup_slot_loop=refuse,
                               lookup_available=lambda: True, lookup_slot_q8_available=lambda: True,
                               lookup_trunk_available=lambda: True, D=64 if kind == "head_dim_64" else 128)
    if kind == "head_dim_64":
        hf.lookup_slot_q8_available = lambda: False            # (as LlamaHIP says it: the step needs head_dim 128)
    elif kind == "no_lookup_q8":
        del hf.lookup_slot_q8_available
    elif kind == "no_lookup_trunk":
        del hf.lookup_trunk_available
    elif kind == "no_lookup":                                  # a model from before the lookup step
        del hf.lookup_slot_loop, hf.lookup_available, hf.lookup_slot_q8_available, hf.lookup_trunk_available
    elif kind == "lookup_says_no":
        hf.lookup_available = hf.lookup_slot_q8_available = hf.lookup_trunk_available = lambda: False
    elif kind == "loop_method_only":
        del hf.lookup_available, hf.lookup_slot_q8_available, hf.lookup_trunk_available
    else:
        assert kind in ("everything", "no_loop"), kind
    return hf


def _params(kind: str):
    from promptcache_amd.generation_engine import GenerationParameters
    kw = dict(sampled=dict(temperature=0.8, top_p=0.9), nine_stops=dict(temperature=0.0, stop_token_ids=list(range(9))),
              one_token=dict(temperature=0.0, max_new_tokens=1), greedy=dict(temperature=0.0))[kind]
    return GenerationParameters(**{"max_new_tokens": 8, **kw})


def _caches(kind: str, n: int):
    arenas = [types.SimpleNamespace(B=1) for _ in range(n)]
    if kind == "shared" and n > 1:
        arenas[1] = arenas[0]
    return [types.SimpleNamespace(arena=None if kind == "none" else a) for a in arenas]


@contextlib.contextmanager
def _environment(values: dict):
    saved = {k: os.environ.pop(k, None) for k in ENV_NAMES}
    os.environ.update({k: v for k, v in values.items() if v is not None})
    try:
        yield
    finally:
        for k in ENV_NAMES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def _outcome(call):
    try:
        got = call()
    except ValueError as e:
        return "ValueError: " + str(e)
    except Reached as e:
        return "reached " + str(e)
    return "ended" if got is None else list(got)


def outcomes(model: str, args: dict, slots: int, env: dict, engine=None, lm=None, params: str = "greedy", caches: str = "own"):
    """The outcome of each of ENTRIES for one case: a ValueError's text, the plan tuple (as a list), "ended" or "reached <name>"."""
    from promptcache_amd.generation_engine import GenerationEngine
    lm = types.SimpleNamespace(**{**dict(hf_model=_model(model), use_full_position_ids=False, decode=lambda ids: "", device="cpu"),
                                  **(lm or {})})
    ge = GenerationEngine(lm)
    ge.device_greedy_loop = ge.device_sample_loop = True
    for k, v in (engine or {}).items():
        setattr(ge, k, v)

    def reached(name):
        def f(*a, **kw):
            raise Reached(name)
        return f
    ge._first_token, ge.generate = reached("_first_token"), reached("generate")
    p = _params(params)
    ce = types.SimpleNamespace(slots=slots, max_ctx_length=2048)
    reqs = [([1, 2], [0, 1], c) for c in _caches(caches, slots)]
    plan = {k: args[k] for k in ("slot_kv", "keep_arenas")}
    if args["lookup"] is not None:
        plan["lookup"] = args["lookup"]
    batch = {k: args[k] for k in ("share_trunk", "lookup", "slot_kv", "keep_arenas")}
    with _environment(env):
        return [
            _outcome(lambda: next(ge.serve(ce, [], p, **args), None)),
            _outcome(lambda: ge.serve_plan(slots=slots, loop_prefill=args["loop_prefill"], **plan)),
            _outcome(lambda: next(ge.generate_batch(reqs, p, **batch), None)),
            _outcome(lambda: ge.batch_plan(slots, p, slot_kv=args["slot_kv"])),
        ]


def cases():
    """Every case as the keyword arguments of ``outcomes``: the product of AXES, then ROWS x their models x the product of SUB_AXES."""
    arg_names = ("slot_kv", "share_trunk", "lookup", "keep_arenas", "loop_prefill")
    for values in itertools.product(*AXES.values()):
        c = dict(zip(AXES, values))
        yield dict(model=c["model"], args={k: c[k] for k in arg_names}, slots=c["slots"],
                   env={k: c[k] for k in ("PC_SLOT_KV", "PC_SLOT_KEEP_ARENAS")})
    for row in ROWS:
        extra = {k: row[k] for k in ("engine", "lm", "params", "caches") if k in row}
        for model in row["models"]:
            for values in itertools.product(*SUB_AXES.values()):
                yield dict(model=model, args=dict(zip(SUB_AXES, values)), slots=row.get("slots", 4), env=row.get("env", {}), **extra)


def n_cases() -> int:
    n = lambda axes: len(list(itertools.product(*axes.values())))
    return n(AXES) + sum(len(row["models"]) for row in ROWS) * n(SUB_AXES)


def record() -> dict:
    """The fixture: the axes, the distinct outcomes in order of first appearance, and per entry point one character of ALPHABET
    (its position is the outcome's index) per case, in the order of ``cases``."""
    distinct, index, codes = [], {}, {e: [] for e in ENTRIES}
    import promptcache_amd.generation_engine  # noqa: F401
    gc.freeze()               # (serve and generate_batch end in gc.collect(): keep torch's objects out of its way)
    try:
        for case in cases():
            for entry, out in zip(ENTRIES, outcomes(**case)):
                key = json.dumps(out)
                if key not in index:
                    index[key] = len(distinct)
                    distinct.append(out)
                codes[entry].append(ALPHABET[index[key]])
    finally:
        gc.unfreeze()
    return dict(axes=AXES, sub_axes=SUB_AXES, rows=ROWS, entries=list(ENTRIES), outcomes=distinct,
                cases={e: "".join(c) for e, c in codes.items()})


def main() -> int:
    for p in (ROOT, os.path.join(ROOT, "prompt-cache_amd")):
        if p not in sys.path:
            sys.path.append(p)                                     # (behind PYTHONPATH: another commit's package wins)
    import promptcache_amd
    got = record()
    print(f"{n_cases()} cases x {len(ENTRIES)} entry points, {len(got['outcomes'])} distinct outcomes, package "
          f"{os.path.dirname(promptcache_amd.__file__)}", file=sys.stderr)
    if "--check" in sys.argv:
        want = json.load(open(FIXTURE))
        same = json.loads(json.dumps(got)) == want
        print("equal" if same else "DIFFERENT", file=sys.stderr)
        return 0 if same else 1
    with open(FIXTURE, "w") as f:
        json.dump(got, f, indent=None, separators=(",", ":"))
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
