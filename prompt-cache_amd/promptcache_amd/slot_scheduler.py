"""Host side of continuous batching (``GenerationEngine.serve``): which request takes which slot, and when.

Pure host logic -- no torch, no GPU -- so that it can be tested with fakes.  The scheduler owns the request iterator (pulled only
when a slot can take the request), the free list, and the shared-trunk groups with their leader protection; ``replay_count`` is the
same rule run without a device, the expected number of replays of a serve run whose sequences all use their whole budget.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Tuple

from .model.kv_arena import common_trunks

DEVICE_STOP_IDS = 8          # stop ids a slot holds on the device (pc_sample_advance_slots_each); the host kills for the rest


def split_stop_ids(stop_token_ids) -> Tuple[List[int], bool]:
    """-> (the stop ids the device holds: the first 8, whether the host has to kill the slot for the others)."""
    ids = [int(t) for t in stop_token_ids]
    return ids[:DEVICE_STOP_IDS], len(ids) > DEVICE_STOP_IDS


def _same_run(a, b) -> bool:
    return a[0] is b[0] and tuple(a[1:]) == tuple(b[1:])                 # common_trunks' identity rule


def shared_leading_rows(lead_layout, layout) -> int:
    """Rows of the leading runs two staged layouts (``KVArena.layout``) have in common."""
    rows = 0
    for a, b in zip(lead_layout, layout):
        if not _same_run(a, b):
            break
        rows += int(a[1])
    return rows


class SlotScheduler:
    """``slots`` slots over an iterable of requests.

    ``next_request()`` pulls the next request when -- and only when -- a slot is free, and says which slot takes it (the lowest
    free one).  ``started(slot, index)`` / ``finished(slot)`` follow the sequences.  With ``share_trunk``: ``group_first_fill``
    groups the first fill by ``common_trunks``; ``join(slot, layout)`` lets a later request join a group whose trunk its layout
    covers; a slot whose arena leads a group with live members stays out of the free list after its own sequence ended, until
    the last member ends.  ``trace``: what happened, in order -- ("pull", index, slot), ("start", index, slot, step), ("finish",
    index, slot, step), ("free", slot, step), ("hold", slot, step) for a protected leader."""

    def __init__(self, slots: int, requests: Iterable, share_trunk: bool = False, min_trunk: Optional[int] = None):
        if not 1 <= int(slots) <= 16:
            raise ValueError(f"slots must be in [1, 16], not {slots!r}")
        self.slots = int(slots)
        self._it = iter(requests)
        self._exhausted = False
        self.share_trunk, self.min_trunk = bool(share_trunk), min_trunk
        self.free: List[int] = list(range(self.slots))
        self.running = {}                   # slot -> request index
        self.held = set()                   # leader slots whose own sequence is over while members live
        self.groups = {}                    # leader slot -> dict(T, layout, members: set of slots with a live sequence)
        self.member_of = {}                 # slot -> leader slot, for slots with a live sequence in a group
        self.pulled = 0
        self.trace: List[tuple] = []

    # ---- requests --------------------------------------------------------------------------------------------------------
    def next_request(self):
        """-> (index, slot, request) or None: no free slot (admission waits) or no request left."""
        if not self.free or self._exhausted:
            return None
        try:
            req = next(self._it)
        except StopIteration:
            self._exhausted = True
            return None
        slot = min(self.free)
        self.free.remove(slot)
        index = self.pulled
        self.pulled += 1
        self.trace.append(("pull", index, slot))
        return index, slot, req

    @property
    def exhausted(self) -> bool:
        return self._exhausted

    def started(self, slot: int, index: int, step: int = 0) -> None:
        self.running[slot] = index
        self.trace.append(("start", index, slot, step))

    def dropped(self, slot: int, index: int, step: int = 0) -> None:
        """The request pulled into ``slot`` ended with its first token (it never ran in the loop)."""
        self.trace.append(("finish", index, slot, step))
        self._release(slot, step)

    def finished(self, slot: int, step: int = 0) -> None:
        index = self.running.pop(slot)
        self.trace.append(("finish", index, slot, step))
        g = self.member_of.pop(slot, None)
        if g is not None:
            grp = self.groups[g]
            grp["members"].discard(slot)
            if not grp["members"]:                       # the last member: the group is over, a held leader slot comes back
                del self.groups[g]
                if g in self.held:
                    self.held.discard(g)
                    self._free(g, step)
        self._release(slot, step)

    def _release(self, slot: int, step: int) -> None:
        grp = self.groups.get(slot)
        if grp is not None and grp["members"]:           # its arena is still read by the members: never restaged
            self.held.add(slot)
            self.trace.append(("hold", slot, step))
        else:
            self._free(slot, step)

    def _free(self, slot: int, step: int) -> None:
        if slot not in self.free:
            self.free.append(slot)
            self.trace.append(("free", slot, step))

    # ---- shared trunks ---------------------------------------------------------------------------------------------------
    def group_first_fill(self, slots: List[int], layouts: List[list]):
        """Group the sequences of the first fill (``common_trunks`` over their layouts).  -> per sequence ``(leader, T)`` with the
        leader as an index into ``slots`` (what ``LlamaHIP.slot_loop(trunks=...)`` takes), ``(None, 0)`` for one on its own."""
        if not self.share_trunk:
            return [(None, 0)] * len(slots)
        trunks = common_trunks(layouts, self.min_trunk)
        for k, (l, T) in enumerate(trunks):
            if l is None:
                continue
            g = slots[l]
            grp = self.groups.setdefault(g, dict(T=T, layout=list(layouts[l]), members=set()))
            grp["members"].add(slots[k])
            self.member_of[slots[k]] = g
        return trunks

    def join(self, slot: int, layout) -> Optional[Tuple[int, int]]:
        """A later request staged as ``layout`` in ``slot``: ``(leader slot, T)`` of the group it joins -- the first whose trunk its
        layout covers (at least ``T`` leading rows in common with the leader's layout) -- or None: it runs unshared."""
        if not self.share_trunk:
            return None
        for g in sorted(self.groups):
            grp = self.groups[g]
            if g != slot and grp["members"] and shared_leading_rows(grp["layout"], layout) >= grp["T"]:
                grp["members"].add(slot)
                self.member_of[slot] = g
                return g, grp["T"]
        return None


def wants_look_ahead(seqs, i: int, k: int = 0) -> bool:
    """Whether replay i + 1 is enqueued before the host reads replay i's tokens.  ``seqs``: ``(start, left)`` of every running
    sequence -- the replay it entered at, the tokens its budget still allows from replay max(i, start) on.  Yes when a sequence
    enters at i + 1 or one has budget beyond replay i, which yields ``k + 1`` tokens at most: the GPU then never waits for the host;
    a stop id or stop string the host has not seen yet wastes at most that one replay."""
    return any(start > i or left > k + 1 for start, left in seqs)


def replay_count(max_new_tokens: List[int], slots: int) -> int:
    """Replays of the device step a ``serve`` run takes for requests that decode exactly ``max_new_tokens[r]`` tokens each (no stop
    id, no stop string, arenas large enough), through ``slots`` slots: the host simulation of the scheduling rule.

    The rule: a request's first token comes from its prefill; a request with more to decode enters the loop at the next replay to be
    enqueued and takes ``max_new_tokens - 1`` replays.  The host reads replay i's tokens with replay i + 1 already enqueued if some
    running sequence still has budget for it; a slot freed by what replay i showed is refilled before the next enqueue."""
    sched = SlotScheduler(slots, list(max_new_tokens))
    left = {}                                  # slot -> steps left in the loop
    start = {}

    def fill(n: int) -> None:
        while True:
            nxt = sched.next_request()
            if nxt is None:
                return
            index, slot, m = nxt
            if m < 2:
                sched.dropped(slot, index, n)
                continue
            sched.started(slot, index, n)
            left[slot], start[slot] = m - 1, n
    n = 0                                      # replays enqueued
    fill(0)
    i = 0
    while left:
        while n <= i:
            n += 1
        if n == i + 1 and wants_look_ahead([(start[s], left[s]) for s in left], i):
            n += 1
        for s in sorted(left):
            if start[s] > i:
                continue
            left[s] -= 1
            if left[s] == 0:
                del left[s], start[s]
                sched.finished(s, i)
        fill(n)
        i += 1
    return n
