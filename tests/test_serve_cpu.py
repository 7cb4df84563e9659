"""Continuous batching, the parts that need no GPU: the C-ABI of pc_sample_advance_slots_each / pc_slot_arm, the layout of
pc_slot_arm_block, argument checks, the slot scheduler with fakes, ``serve_plan``'s decision table and the replay-count simulation."""
import ctypes
import os
import re
import subprocess
import types

import pytest

from tests import serve_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pc_sample_advance_slots_each", "pc_slot_arm")


def test_header_declares_and_library_exports_the_serve_entries():
    from promptcache_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "promptcache_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.lib_path())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _native.SIGNATURES, name


def test_slot_arm_structs_match_the_header(tmp_path):
    """The method of test_abi_symbols.test_struct_layouts_match_the_header for the two structs of pc_slot_arm."""
    from promptcache_amd import _native
    structs = (("pc_slot_arm_block", _native.SlotArmBlock), ("pc_slot_state", _native.SlotState), ("pc_sample_params", _native.SampleParams))
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {']
    for st, cls in structs:
        body.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            body.append(f'  printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    body += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    for st, cls in structs:
        assert int(got[st]) == ctypes.sizeof(cls), st
        for name, _ in cls._fields_:
            assert int(got[f"{st}.{name}"]) == getattr(cls, name).offset, (st, name)
    assert ctypes.sizeof(_native.SlotArmBlock) % 8 == 0                  # the bitmap behind it is read as 64-bit words
    assert _native.slot_arm_bytes(1000) == ctypes.sizeof(_native.SlotArmBlock) + 4000
    assert _native.slot_arm_bytes(33) == ctypes.sizeof(_native.SlotArmBlock) + 136


def _fake_state(native, null=None):
    """A pc_slot_state of non-null (never dereferenced: every call below is rejected first) pointers."""
    st = native.SlotState(*[0x1000 + 64 * i for i in range(15)])
    if null is not None:
        setattr(st, null, None)
    return st


def test_serve_entries_reject_bad_arguments_without_a_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    hw = 4
    good = dict(slot=2, cap=64, kv_base=0x10000, len=10, pos=11, id=5, leader=-1, trunk=0, budget=4, counter=0, draws=1, seed=9,
                params=sr.GREEDY, stop_ids=[3], hist=[0] * hw)
    nbytes = _native.slot_arm_bytes(hw)

    def arm(fields, S=4, state=None, nb=nbytes, offset=0):
        raw = sr.arm_block_bytes(_native, hw, **fields)
        buf = (ctypes.c_uint8 * (len(raw) + 16)).from_buffer_copy(bytes(raw) + bytes(16))
        base = ctypes.addressof(buf)
        pad = (-base) % 8 + offset
        ctypes.memmove(base + pad, bytes(raw), len(raw))
        st = _fake_state(_native) if state is None else state
        return lib.pc_slot_arm(base + pad, nb, ctypes.byref(st), S, None)

    assert arm(dict(good, slot=4)) == -1001 and b"slot outside" in lib.pc_last_error_string()
    assert arm(dict(good, slot=-1)) == -1001 and b"slot outside" in lib.pc_last_error_string()
    assert arm(good, S=0) == -1001 and b"S <= 16" in lib.pc_last_error_string()
    assert arm(good, S=17) == -1001 and b"S <= 16" in lib.pc_last_error_string()
    assert lib.pc_slot_arm(None, nbytes, ctypes.byref(_fake_state(_native)), 4, None) == -1001
    assert b"null pointer" in lib.pc_last_error_string()
    assert arm(good, state=_fake_state(_native, "draws")) == -1001 and b"null pointer" in lib.pc_last_error_string()
    assert arm(good, state=_fake_state(_native, "history_bits")) == -1001
    assert arm(good, offset=4) == -1001 and b"8-byte aligned" in lib.pc_last_error_string()
    assert arm(good, nb=nbytes + 8) == -1001 and b"nbytes" in lib.pc_last_error_string()
    assert arm(good, nb=nbytes - 8) == -1001 and b"nbytes" in lib.pc_last_error_string()
    # pc_sample_advance_slots_each: pc_sample_advance_slots' checks, plus the draws pointer
    p = [0x1000] * 20
    each = lib.pc_sample_advance_slots_each
    assert each(None, 0, 10, None, None, None, None, None, None, None, None, None, None, None, None, None, 4, 8, None, None) == -1001
    assert each(p[0], 10, 10, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], None, 4, 8, None, None) == -1001
    assert b"null pointer" in lib.pc_last_error_string()
    assert each(p[0], 10, 10, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], 4, 17, None, None) == -1001
    assert b"S <= 16" in lib.pc_last_error_string()
    assert each(p[0], 9, 10, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], 4, 8, None, None) == -1001
    assert b"row stride" in lib.pc_last_error_string()
    assert each(p[0], 10, 1 << 24, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], 4, 8, None, None) == -1001


def test_each_case_seeds_leave_three_quarters_comparable():
    """The rng seeds of the per-slot advance case (tests/serve_ref.EACH_RNG_SEED) were picked here, on the reference alone."""
    for V in (1001, 32000):
        margins = sr.each_reference_margins(V)
        assert len(margins) == 9                                          # slots 1 and 5: 4 steps each, slot 3: its stop id at step 0
        assert 4 * sum(m > sr.MARGIN for m in margins) >= 3 * len(margins), (V, margins)


# ---- the scheduler -------------------------------------------------------------------------------------------------------------
def _sched(*a, **k):
    from promptcache_amd.slot_scheduler import SlotScheduler
    return SlotScheduler(*a, **k)


def test_admission_order_and_which_slot_is_taken():
    s = _sched(3, ["a", "b", "c", "d", "e"])
    got = [s.next_request() for _ in range(4)]
    assert got[:3] == [(0, 0, "a"), (1, 1, "b"), (2, 2, "c")] and got[3] is None          # full: admission waits
    for index, slot, _ in got[:3]:
        s.started(slot, index)
    s.finished(1, step=5)
    assert s.next_request() == (3, 1, "d")                               # the freed slot
    s.started(1, 3, 6)
    s.finished(2, step=7)
    s.finished(0, step=7)
    assert s.next_request() == (4, 0, "e")                               # the lowest free slot
    assert s.next_request() is None and s.exhausted
    assert [t for t in s.trace if t[0] == "pull"] == [("pull", 0, 0), ("pull", 1, 1), ("pull", 2, 2), ("pull", 3, 1), ("pull", 4, 0)]
    with pytest.raises(ValueError):
        _sched(0, [])
    with pytest.raises(ValueError):
        _sched(17, [])


def test_a_lazy_iterable_is_pulled_only_when_a_slot_frees():
    pulled = []

    def gen():
        for r in range(5):
            pulled.append(r)
            yield r
    s = _sched(2, gen())
    assert pulled == []
    a, b = s.next_request(), s.next_request()
    assert pulled == [0, 1] and s.next_request() is None and pulled == [0, 1]
    s.started(a[1], a[0]); s.started(b[1], b[0])
    s.finished(0)
    assert pulled == [0, 1] and s.next_request()[0] == 2 and pulled == [0, 1, 2]
    # a request that ends with its first token gives its slot back at once
    s.dropped(0, 2)
    assert s.next_request() == (3, 0, 3)


def _layouts():
    sysm, intro, a1, a2, other = (object() for _ in range(5))
    lay = lambda *runs: [(seq, rows, "fp16") for seq, rows in runs]
    return dict(lead=lay((sysm, 300), (intro, 40), (a1, 30)), m1=lay((sysm, 300), (intro, 40), (a2, 30)),
                m2=lay((sysm, 300), (intro, 40), (a1, 30)), short=lay((sysm, 300), (a2, 30)), alien=lay((other, 340), (a1, 30)),
                resized=lay((sysm, 300), (intro, 41)), int8=[(sysm, 300, "int8"), (intro, 40, "int8")])


def test_leader_protection_and_the_join_rule():
    L = _layouts()
    s = _sched(4, range(8), share_trunk=True, min_trunk=1)
    first = [s.next_request() for _ in range(3)]
    trunks = s.group_first_fill([0, 1, 2], [L["lead"], L["m1"], L["alien"]])
    assert trunks == [(0, 340), (0, 340), (None, 0)]                    # system + intro; the third sequence is on its own
    for index, slot, _ in first:
        s.started(slot, index)
    assert s.groups[0]["T"] == 340 and s.groups[0]["members"] == {0, 1}
    # a later request joins: at least T leading rows in common with the leader's layout
    index, slot, _ = s.next_request()
    assert slot == 3 and s.join(3, L["m2"]) == (0, 340)
    s.started(3, index)
    # the leader's own sequence ends first while two members live: its slot is held, not freed
    s.finished(0, step=4)
    assert 0 in s.held and 0 not in s.free and s.next_request() is None  # no free slot: admission waits
    assert ("hold", 0, 4) in s.trace
    s.finished(2, step=5)                                                # the unshared one: free at once
    index, slot, _ = s.next_request()
    assert slot == 2
    # layouts that share fewer rows than the trunk, or other bytes, run unshared
    assert s.join(2, L["short"]) is None and s.join(2, L["alien"]) is None and s.join(2, L["resized"]) is None
    assert s.join(2, L["int8"]) is None                                  # the same modules from another store format
    s.started(2, index)
    s.finished(1, step=6)
    assert 0 in s.held and s.free == [1]
    s.finished(3, step=9)                                                # the last member: the leader's slot comes back
    assert not s.held and sorted(s.free) == [0, 1, 3] and 0 not in s.groups
    assert s.join(1, L["m1"]) is None                                    # the group is over
    order = [t[:2] for t in s.trace if t[0] in ("hold", "free")]
    assert order.index(("hold", 0)) < order.index(("free", 0)) and order.index(("free", 3)) > order.index(("free", 0)) - 2
    # without share_trunk nothing is grouped and nobody joins
    t = _sched(2, range(2))
    assert t.group_first_fill([0, 1], [L["lead"], L["m1"]]) == [(None, 0), (None, 0)] and t.join(1, L["m1"]) is None


def test_more_than_eight_stop_ids_keep_the_first_eight_on_the_device():
    from promptcache_amd.slot_scheduler import split_stop_ids
    assert split_stop_ids([]) == ([], False)
    assert split_stop_ids(range(8)) == (list(range(8)), False)
    assert split_stop_ids(range(20, 31)) == (list(range(20, 28)), True)


def _engine(hf=None, full=False):
    from promptcache_amd.generation_engine import GenerationEngine
    return GenerationEngine(types.SimpleNamespace(hf_model=hf, use_full_position_ids=full))


def test_serve_plan_decision_table():
    ok = types.SimpleNamespace(slot_loop=lambda *a, **k: None, slot_loop_available=lambda: True)
    no = types.SimpleNamespace(slot_loop=lambda *a, **k: None, slot_loop_available=lambda: False)      # Falcon, int8, PC_DECODE_TAIL=1
    assert _engine(ok).serve_plan()[0]
    assert not _engine(ok, full=True).serve_plan()[0]                   # MPT
    assert not _engine(no).serve_plan()[0]
    assert not _engine(types.SimpleNamespace()).serve_plan()[0] and not _engine(None).serve_plan()[0]
    for knob in ("device_greedy_loop", "device_sample_loop"):            # PC_DEVICE_GREEDY=0 / PC_DEVICE_SAMPLE=0
        e = _engine(ok)
        setattr(e, knob, False)
        batched, why = e.serve_plan()
        assert not batched and "PC_DEVICE" in why


def test_serve_without_a_slot_loop_runs_generate_per_request_with_its_own_parameters():
    from promptcache_amd.generation_engine import GenerationParameters, Output
    e = _engine(None)
    calls = []

    def fake_generate(ids, pos, p, cache, stream_interval, use_full_position_ids=False):
        calls.append((ids, p.max_new_tokens))
        yield Output("t", f"{ids}:{p.max_new_tokens}")
    e.generate = fake_generate
    ce = types.SimpleNamespace(process=lambda prompt, return_full_position_ids=False: ([prompt], [0], 0.0, None), slots=2)
    dflt = GenerationParameters(max_new_tokens=3)
    reqs = iter(["a", ("b", GenerationParameters(max_new_tokens=9)), ("c", None)])
    got = [(r, o.new_text) for r, o in e.serve(ce, reqs, dflt)]
    assert got == [(0, "['a']:3"), (1, "['b']:9"), (2, "['c']:3")]


def test_replay_count_simulation():
    from promptcache_amd.slot_scheduler import replay_count
    assert replay_count([5, 5, 5, 5], 4) == 4                            # one wave: max_new - 1 replays, no look-ahead past the budget
    assert replay_count([1, 1, 1], 2) == 0                               # first tokens only: the loop never runs
    assert replay_count([2, 2], 1) == 2                                  # one slot: one after another
    # 4 slots, 7 requests: slot 0 frees after replay 3 with replay 4 in flight -> request 4 runs replays 5..19; slot 3 frees after
    # replay 7 -> request 5 runs 9..14; slot 1 frees after replay 10 -> request 6 runs 12..21
    assert replay_count([5, 12, 20, 9, 16, 7, 11], 4) == 22
    # static waves of 4 would take (20 - 1) + (16 - 1) = 34 replays for the same requests
    assert replay_count([5, 12, 20, 9, 16, 7, 11], 4) < 34


# ---- serve over a fake model and engine: the control flow without a device -------------------------------------------------------
class _FakeLoop:
    """SlotLoop's protocol on the host: sequence k's token at its local step j is ``1000 * tag + j + 1``."""

    def __init__(self, tags, max_news, stops, slot_index):
        self.n, self.nsplit_trunk = 0, 0
        self._start, self._max_new, self._stops, self._tag, self._killed, self.idx = [], [], [], [], [], []
        self.retired, self.closed = {}, None
        for t, mn, sp, s in zip(tags, max_news, stops, slot_index):
            self._add(t, mn, sp, s)

    def _add(self, tag, max_new, stops, slot):
        self._start.append(self.n); self._max_new.append(max_new); self._stops.append(set(stops)); self._tag.append(tag)
        self._killed.append(None); self.idx.append(slot)
        return len(self._tag) - 1

    def enqueue(self):
        self.n += 1
        return self.n - 1

    def elapsed_ms(self, i):
        assert i < self.n
        return 1.0

    def token(self, k, i):
        assert i < self.n, "the host asked for a replay it never enqueued"
        j = i - self._start[k]
        if j < 0 or j >= self._max_new[k] or (self._killed[k] is not None and i >= self._killed[k]):
            return None
        for jj in range(j):
            if 1000 * self._tag[k] + jj + 1 in self._stops[k]:
                return None
        return 1000 * self._tag[k] + j + 1

    def kill(self, k):
        self._killed[k] = self.n

    def admit(self, slot, past, token, position, max_new, params, seed, history, stop_ids, trunk=None):
        live = [k for k in range(len(self._tag)) if self.idx[k] == slot and k not in self.retired]
        assert not live, "admitted into a slot whose sequence was not retired"
        return self._add(past.tag, max_new, stop_ids, slot)

    def retire(self, k, consumed):
        self.retired[k] = consumed

    def close(self, consumed):
        self.closed = dict(consumed)


def _fake_serve(slots, reqs, stream_interval=1):
    import torch
    from promptcache_amd.generation_engine import GenerationEngine
    made = []

    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, slots=None, slot_index=None, each=False,
                  max_keys=None, trunks=None):
        assert each and max_keys == 4096 and all(len(s) <= 8 for s in stop_ids)
        made.append(_FakeLoop([p.tag for p in pasts], max_new, stop_ids, slot_index))
        return made[-1]
    hf = types.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True)
    lm = types.SimpleNamespace(hf_model=hf, use_full_position_ids=False, decode=lambda ids: " ".join(map(str, ids)))
    ge = GenerationEngine(lm)
    staged = []

    def process(prompt, slot=0):
        staged.append((prompt, slot))
        return [prompt], [10], 0.0, types.SimpleNamespace(tag=prompt)

    def forward(ids, positions, cache):
        V = 2000 * 64
        logits = torch.zeros((1, 1, V))
        logits[0, 0, 1000 * cache.tag] = 1.0                             # the first token of request `tag` is 1000 * tag
        return logits, types.SimpleNamespace(tag=cache.tag, arena=types.SimpleNamespace(layout=[])), 1.0
    ge._forward = forward
    ce = types.SimpleNamespace(process=process, slots=slots, max_ctx_length=4096)
    outs = {}
    for r, o in ge.serve(ce, reqs, stream_interval=stream_interval):
        outs.setdefault(r, []).append(o)
    return ge, made, staged, outs


def test_serve_control_flow_over_a_fake_model_matches_the_simulation():
    from promptcache_amd.generation_engine import GenerationParameters
    from promptcache_amd.slot_scheduler import replay_count
    lens = [5, 12, 20, 9, 16, 7, 11]
    pulled = []

    def lazy():
        for r, n in enumerate(lens):
            pulled.append(r)
            yield r + 1, GenerationParameters(temperature=0.0, max_new_tokens=n)
    ge, made, staged, outs = _fake_serve(4, lazy())
    loop = made[0]
    assert len(made) == 1 and loop.n == replay_count(lens, 4) == 22 and ge.last_serve_stats["replays"] == 22
    assert [s for _, s in staged] == [0, 1, 2, 3, 0, 3, 1]               # which slot each request was staged into
    assert loop._start == [0, 0, 0, 0, 5, 9, 12]
    for r, n in enumerate(lens):
        assert ge.last_serve_tokens[r] == [1000 * (r + 1) + j for j in range(n)], r
        assert len(outs[r]) == n and outs[r][-1].new_text == " ".join(str(1000 * (r + 1) + j) for j in range(n))
    assert loop.retired == {k: lens[k] - 1 for k in range(7)} and loop.closed == {}
    assert ge.last_serve_stats["live_rows"] == sum(n - 1 for n in lens)
    # requests that end with their first token never enter the loop; one slot serves everything one after another
    ge, made, staged, outs = _fake_serve(1, [(r + 1, GenerationParameters(temperature=0.0, max_new_tokens=n)) for r, n in enumerate([1, 3, 1, 2])])
    assert made[0].n == replay_count([1, 3, 1, 2], 1) == 3 and [len(outs[r]) for r in range(4)] == [1, 3, 1, 2]


def test_serve_kills_the_slot_for_a_stop_id_past_the_eighth_and_rewinds_when_abandoned():
    from promptcache_amd.generation_engine import GenerationParameters
    # request 0: eleven stop ids, the tenth (1004) hits at its fourth loop step -- the device holds the first eight only
    stops = [90001 + j for j in range(9)] + [1004, 90020]
    reqs = [(1, GenerationParameters(temperature=0.0, max_new_tokens=12, stop_token_ids=stops)),
            (2, GenerationParameters(temperature=0.0, max_new_tokens=12, stop_token_ids=[2003])),
            (3, GenerationParameters(temperature=0.0, max_new_tokens=4))]
    ge, made, staged, outs = _fake_serve(2, reqs)
    loop = made[0]
    assert ge.last_serve_tokens[0] == [1000, 1001, 1002, 1003, 1004] and loop._killed[0] is not None     # the host killed slot 0
    assert ge.last_serve_tokens[1] == [2000, 2001, 2002, 2003] and loop._killed[1] is None               # the device's own stop id
    assert ge.last_serve_tokens[2] == [3000, 3001, 3002, 3003] and loop.retired == {0: 4, 1: 3, 2: 3}
    assert loop._stops[0] == set(stops[:8])
    # abandoned at a yield: close() gets what every running sequence consumed
    import torch
    import types as _t
    from promptcache_amd.generation_engine import GenerationEngine
    lens = [9, 9, 9]
    hold = {}

    def slot_loop(pasts, tokens, positions, max_new, params, seeds, histories, stop_ids, **kw):
        hold["loop"] = _FakeLoop([p.tag for p in pasts], max_new, stop_ids, kw["slot_index"])
        return hold["loop"]
    hf = _t.SimpleNamespace(slot_loop=slot_loop, slot_loop_available=lambda: True)
    lm = _t.SimpleNamespace(hf_model=hf, use_full_position_ids=False, decode=lambda ids: " ".join(map(str, ids)))
    ge2 = GenerationEngine(lm)

    def forward(ids, positions, cache):
        logits = torch.zeros((1, 1, 8000))
        logits[0, 0, 1000 * cache.tag] = 1.0
        return logits, _t.SimpleNamespace(tag=cache.tag, arena=_t.SimpleNamespace(layout=[])), 1.0
    ge2._forward = forward
    ce = _t.SimpleNamespace(process=lambda prompt, slot=0: ([prompt], [10], 0.0, _t.SimpleNamespace(tag=prompt)), slots=2,
                            max_ctx_length=4096)
    gen = ge2.serve(ce, [(r + 1, GenerationParameters(temperature=0.0, max_new_tokens=n)) for r, n in enumerate(lens)], stream_interval=1)
    seen = 0
    for r, o in gen:
        seen += 1
        if seen == 8:                                                    # 2 first tokens + 3 loop steps of both sequences
            break
    gen.close()
    assert hold["loop"].closed == {0: 3, 1: 3}
