"""The modes of the batched loops (``promptcache_amd/modes.py``): ``serve`` / ``serve_plan`` / ``generate_batch`` /
``batch_plan`` over the full product of their mode arguments, the environment and what a model offers, against the outcomes recorded
in ``tests/golden/serve_modes.json`` (``tools/gen_serve_modes_golden.py``, run on the commit in front of the refactor), and the
resolution itself called directly."""
import importlib.util
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("gen_serve_modes_golden", os.path.join(ROOT, "tools", "gen_serve_modes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_case_of_the_matrix_has_the_recorded_outcome():
    tool = _tool()
    want = json.load(open(tool.FIXTURE))
    # the product is the one that was recorded, and it is the one the issue asked for at least
    assert want["axes"] == json.loads(json.dumps(tool.AXES)) and want["sub_axes"] == json.loads(json.dumps(tool.SUB_AXES))
    assert want["rows"] == json.loads(json.dumps(tool.ROWS)) and want["entries"] == list(tool.ENTRIES)
    floor = dict(model=5, PC_SLOT_KV=[None, "int8"], PC_SLOT_KEEP_ARENAS=[None, "0"], slots=[4, 16], slot_kv=[None, "fp16", "int8", "fp8"],
                 share_trunk=[False, True], lookup=[0, 3, 20], keep_arenas=[None, True, False], loop_prefill=[None, False, True])
    assert len(tool.AXES["model"]) >= floor.pop("model") and all(tool.AXES[k] == v for k, v in floor.items())
    n_product = len(list(itertools.product(*tool.AXES.values())))
    assert n_product == 8640 and tool.n_cases() == n_product + sum(len(r["models"]) for r in tool.ROWS) * 32
    got = tool.record()
    cases = list(tool.cases())
    assert len(cases) == tool.n_cases()
    compared, wrong = 0, []
    for entry in tool.ENTRIES:
        g, w = got["cases"][entry], want["cases"][entry]
        assert len(g) == len(w) == len(cases), entry
        for case, a, b in zip(cases, g, w):
            compared += 1
            a, b = got["outcomes"][tool.ALPHABET.index(a)], want["outcomes"][tool.ALPHABET.index(b)]
            if json.loads(json.dumps(a)) != b:
                wrong.append((entry, case, a, b))
    assert not wrong, f"{len(wrong)} outcomes differ from the recording; the first: {wrong[0]}"
    assert compared == tool.n_cases() * len(tool.ENTRIES)
    assert sorted(map(json.dumps, got["outcomes"])) == sorted(map(json.dumps, want["outcomes"]))


def test_resolution_called_directly():
    from promptcache_amd.modes import Capabilities, Modes, resolve_batch, resolve_serve
    full = Capabilities(lookup_loop=True, lookup=True, lookup_q8=True, lookup_trunk=True, head_dim=128)
    # every mode off: the plain loop, and nothing new is handed to the model
    m = resolve_serve(full, 4, env={})
    assert m == Modes(True, "one device loop, new prompts admitted as slots free up") and m.reason() == m.base
    assert (m.share_trunk, m.lookup, m.drafts, m.no_drafts, m.slot_kv, m.keep_arenas, m.loop_prefill) == (False, 0, 0, None, "fp16", True, False)
    assert m.loop_kwargs() == {} and m.loop_kwargs(one_token=True) == {}
    # the environment is read where the argument is None, and only there
    env = {"PC_SLOT_KV": "int8", "PC_SLOT_KEEP_ARENAS": "0", "PC_SERVE_LOOKUP": "20", "PC_SLOT_TRUNK": "1", "PC_SERVE_LOOP_PREFILL": "1"}
    m = resolve_serve(full, 4, share_trunk=False, loop_prefill=False, env=env)
    assert (m.batched, m.lookup, m.drafts, m.slot_kv, m.keep_arenas, m.loop_prefill) == (True, 15, 15, "int8", False, False)
    assert m.loop_kwargs() == m.loop_kwargs(one_token=True) == {"kv": "int8", "keep_arenas": False}
    assert m.reason().endswith("(slot_kv='int8'), no fp16 slot arenas: every prefill runs in one shared arena (keep_arenas=False)")
    m = resolve_serve(full, 4, slot_kv="fp16", keep_arenas=True, lookup=3, share_trunk=False, env=env)
    assert (m.drafts, m.loop_prefill) == (3, True) and m.loop_kwargs() == {"prompt_rows": True} and m.loop_kwargs(one_token=True) == {}
    assert "loop_prefill=True" in m.reason() and "int8" not in m.reason()
    assert resolve_serve(full, 4, share_trunk=None, slot_kv="fp16", keep_arenas=True, loop_prefill=False, lookup=0, env=env).share_trunk
    # 16 slots x (7 + 1) rows do not fit: the one-token loop, and why
    m = resolve_serve(full, 16, lookup=7, env={})
    assert (m.batched, m.lookup, m.drafts) == (True, 7, 0) and "exceed the 64 rows" in m.no_drafts and m.no_drafts in m.reason()
    # the refusals come in serve's order: slot_kv, keep_arenas, loop_prefill
    with pytest.raises(ValueError, match="must be one of"):
        resolve_serve(full, 4, slot_kv="fp8", keep_arenas=False, loop_prefill=True, env={})
    with pytest.raises(ValueError, match="keep_arenas=False needs slot_kv='int8'"):
        resolve_serve(full, 4, keep_arenas=False, loop_prefill=True, env={})
    with pytest.raises(ValueError, match="lookup is off"):
        resolve_serve(full, 4, loop_prefill=True, env={})
    with pytest.raises(ValueError, match="PC_SLOT_KEEP_ARENAS must be 0 or 1"):
        resolve_serve(full, 4, env={"PC_SLOT_KEEP_ARENAS": "2"})
    # serve_plan's reading checks neither slot_kv nor keep_arenas, and does not read PC_SLOT_KEEP_ARENAS
    m = resolve_serve(full, 4, False, 3, "fp8", None, False, env={"PC_SLOT_KEEP_ARENAS": "2"}, validate=False)
    assert (m.slot_kv, m.keep_arenas, m.drafts) == ("fp8", True, 3)
    # a model without the loop
    none = Capabilities(no_loop="no loop here", not_batched="no loop here")
    m = resolve_serve(none, 4, lookup=3, env={})
    assert (m.batched, m.reason(), m.drafts, m.no_drafts) == (False, "no loop here", 0, "no loop here")
    with pytest.raises(ValueError, match="does not have: no loop here"):
        resolve_serve(none, 4, slot_kv="int8", env={})

    # generate_batch
    m = resolve_batch(full, 4, env={})
    assert m == Modes(True, "one device loop over all sequences") and m.loop_kwargs() == {}
    m = resolve_batch(full, 4, slot_kv="int8", env={})
    assert m.batched and m.loop_kwargs(one_token=True) == {"kv": "int8"} and m.reason().endswith("(slot_kv='int8')")
    m = resolve_batch(full, 4, lookup=20, share_trunk=True, env={})
    assert (m.batched, m.share_trunk, m.lookup, m.drafts) == (True, True, 20, 15)
    assert resolve_batch(full, 4, plain_greedy=False, lookup=3, env={}).drafts == 0
    assert resolve_batch(full, 4, env={"PC_SLOT_LOOKUP": "3", "PC_SLOT_TRUNK": "1", "PC_SLOT_KEEP_ARENAS": "0"}).drafts == 3
    for kw, why in ((dict(n_requests=0), "no requests"), (dict(n_requests=17), "more than 16 requests"),
                    (dict(n_requests=4, n_stop_ids=9), "more than 8 stop token ids"),
                    (dict(n_requests=4, max_new_tokens=1), "nothing to decode after the first token"),
                    (dict(n_requests=4, own_arenas=False), "a cache is not a staged batch-1 arena of its own")):
        m = resolve_batch(full, env={}, **kw)
        assert (m.batched, m.reason()) == (False, why)
        with pytest.raises(ValueError, match="is not: " + why):
            resolve_batch(full, slot_kv="int8", env={}, **kw)
    # ... in generate_batch's order: slot_kv, keep_arenas, lookup with share_trunk
    with pytest.raises(ValueError, match="share_trunk exclude each other"):
        resolve_batch(Capabilities(), 4, slot_kv="int8", keep_arenas=False, lookup=3, share_trunk=True, env={})
    with pytest.raises(ValueError, match="not for generate_batch"):
        resolve_batch(Capabilities(), 4, keep_arenas=False, lookup=3, share_trunk=True, env={})
    with pytest.raises(ValueError, match=r"cannot be combined \(no shared-trunk verify step\)"):
        resolve_batch(Capabilities(), 4, lookup=3, share_trunk=True, env={})
    with pytest.raises(ValueError, match="runs for this batch: more than 16 requests"):
        resolve_batch(full, 17, lookup=3, share_trunk=True, env={})
    # batch_plan's reading checks nothing
    assert resolve_batch(full, 4, slot_kv="fp8", keep_arenas=False, lookup=3, share_trunk=True, env={}, validate=False).batched


def test_modes_imports_without_torch():
    """``promptcache_amd/__init__.py`` imports the engines, and with them torch, so the module is loaded as the file it is: what
    it needs itself is ``os``, ``dataclasses`` and ``typing``."""
    code = ("import sys; import importlib.util as u; s = u.spec_from_file_location('modes', sys.argv[1]); m = u.module_from_spec(s); "
            "sys.modules['modes'] = m; s.loader.exec_module(m); "
            "assert not {'torch', 'numpy', 'promptcache_amd'} & set(sys.modules); m.resolve_serve(m.Capabilities(), 4, env={}); print('ok')")
    path = os.path.join(ROOT, "prompt-cache_amd", "promptcache_amd", "modes.py")
    assert subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, check=True).stdout.strip() == "ok"
    src = open(path).read()
    assert sorted(ln for ln in src.splitlines() if ln.startswith(("import ", "from "))) == [
        "from __future__ import annotations", "from dataclasses import dataclass", "from typing import Mapping, Optional", "import os"]
