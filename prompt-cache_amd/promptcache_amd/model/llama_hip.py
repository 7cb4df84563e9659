"""Llama-2-class forward pass on MI355X: HIP kernels (C-ABI) for the prompt-cache hot path, torch
(hipBLASLt) for the dense projections.

Replaces the reference's patched HF model for this path:
  ``LlamaForCausalLM.forward``   promptcache/model/llama2.py:986-1076
  ``LlamaModel.forward``         promptcache/model/llama2.py:822-951
  ``LlamaDecoderLayer.forward``  promptcache/model/llama2.py:600-654
  ``LlamaAttention.forward``     promptcache/model/llama2.py:315-410   (RoPE, KV concat, mask, softmax, PV)
  ``LlamaMLP.forward``           promptcache/model/llama2.py:242

Call surface (what ``CacheEngine`` / ``GenerationEngine`` use):
  ``model(input_ids=[B,q] long, position_ids=[B,q] long, past_key_values=None|seq of (K,V) [B,Hkv,S,D],
          attention_mask=None|[B,q], use_cache=True)`` -> object with ``.logits`` [B,q,V] fp32 and
  ``.past_key_values`` (indexable ``[layer][0|1]`` -> [B,Hkv,S+q,D]).

Differences by design (same numbers, less traffic):
  * new K/V are appended in place to the arena that backs ``past_key_values`` (no ``torch.cat``);
  * the additive mask is never materialised; it is implicit in the attention kernel;
  * the residual stream is kept in fp32 (the parity target is the reference's fp32 CPU path);
  * right-padded batches (``attention_mask`` with trailing zeros, ``cache_engine.py:240-246``) need no
    mask: causality already hides trailing pads from every real token, and pad rows are never read.

There is no CPU / eager fallback: without the HIP extension this module raises.
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional

import torch

import numpy as np

from .. import _native
# the pure refusals of formats and loop modes live in modes.py (no torch); the names stay importable from here
from ..modes import (SLOT_KV, WEIGHT_FORMATS, TokenControls, check_keep_fp16, check_logprobs, check_loop_prefill,  # noqa: F401
                     check_slot_keep_arenas, check_slot_kv, check_token_controls, check_weight_format, parse_keep_arenas,
                     parse_keep_fp16)
from .config import LlamaShape
from .kv_arena import KVArena, StagedKV, arena_from_past, common_trunks

_SEG_DTYPE = np.dtype([("src", "<u8"), ("dst_row", "<i4"), ("len", "<i4")])      # pc_kv_seg


class _InputBlock:
    """Everything a captured small-q forward reads per call, in ONE pinned host block that the graph's first node
    (``pc_fetch_block``) pulls into its device twin:

        ids   int64 [T] | pos int32 [T] | words int32 [8] = {past_len, residual-tail base, live rows, segments, rows of the row
        table, ids / pos already on the device (0 | 1), -, -} | pc_kv_seg [max_seg]  (the staging plan, when the forward stages
        while it reads)

    Per call the host writes the block (numpy views) and replays the graph: no copy is enqueued, no fill kernel launched.  The
    block may be rewritten once the replay that read it has finished (``acquire`` waits for the event ``release`` records)."""

    def __init__(self, device, T: int, max_seg: int):
        self.T, self.max_seg = T, max_seg
        self.o_pos = 8 * T
        self.o_words = 12 * T
        self.o_segs = (self.o_words + 32 + 15) // 16 * 16
        self.nbytes = self.o_segs + 16 * max_seg
        self.dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.ids = self.dev[:8 * T].view(torch.int64)
        self.pos = self.dev[self.o_pos:self.o_pos + 4 * T].view(torch.int32)
        self.words = self.dev[self.o_words:self.o_words + 32].view(torch.int32)
        self.segs = self.dev[self.o_segs:]
        self.host = torch.zeros(self.nbytes, dtype=torch.uint8, pin_memory=True)
        a = self.host.numpy()
        self.h_ids = a[:8 * T].view(np.int64)
        self.h_pos = a[self.o_pos:self.o_pos + 4 * T].view(np.int32)
        self.h_words = a[self.o_words:self.o_words + 32].view(np.int32)
        self.h_segs = a[self.o_segs:].view(_SEG_DTYPE) if max_seg else None
        self._done = torch.cuda.Event()
        self._busy = False

    def acquire(self) -> None:
        if self._busy:
            self._done.synchronize()
            self._busy = False

    def fetch(self) -> None:
        """(graph node) host block -> device block"""
        _native.fetch_block(self.host, self.dev, self.nbytes)

    def release(self) -> None:
        self._done.record()
        self._busy = True


_GRAPH_RNG_PRIMED: dict = {}


def prime_graph_capture(device) -> None:
    """torch allocates the CUDA generator's graph-capture state (seed / offset words) at the FIRST capture of the process and
    updates it in place at every later one.  The forwards of this package capture under ``torch.inference_mode()``; if theirs is
    the first capture, those words are inference tensors and any capture the CALLER later takes outside inference mode dies in
    ``capture_begin`` ("Inplace update to inference tensor outside InferenceMode").  So the first capture of the process is a
    trivial one taken with inference mode switched off (once, ~1 ms) -- and KEPT: torch frees those words again when the last
    registered graph dies and would re-allocate them under whatever mode the next capture runs in."""
    # (the capture state is per DEVICE: one primed graph per device index this process drives)
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _GRAPH_RNG_PRIMED:
        return
    with torch.inference_mode(False), torch.cuda.device(idx):
        t = torch.zeros(8, device=torch.device("cuda", idx))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t.add_(1.0)
    _GRAPH_RNG_PRIMED[idx] = (g, t)


def lw0_fp16(layers) -> bool:
    """fp16 weight images (no int8 scales) in the layer stack."""
    return len(layers) > 0 and layers[0].get("wqkv_s") is None


@dataclass
class CausalLMOutput:
    logits: torch.Tensor
    past_key_values: Optional[StagedKV]


def logprob_records(ids, lp) -> list:
    """Host records of pc_token_logprobs' two output arrays (``[R][1 + n]``, on the host): per row ``(token, logprob, [(id,
    logprob), ...])`` -- entry 0, then the n alternatives by (value descending, index ascending)."""
    return [(int(i[0]), float(l[0]), [(int(a), float(b)) for a, b in zip(i[1:], l[1:])]) for i, l in zip(ids.tolist(), lp.tolist())]


class _LogprobRing:
    """The host side of a step's log-probability node (``logprobs=n``): the node leaves ``[rows][1 + n]`` ids and
    log-probabilities in fixed device buffers of the loop state, and ``copy(r)`` -- called right behind the replay, where the token
    ring is copied -- takes them into pinned ring row ``r``.  Stream order makes a device-side ring unnecessary."""

    def __init__(self, dev: dict, ring: int):
        self.dev = dev
        self.ids = torch.zeros((ring,) + tuple(dev["ids"].shape), dtype=torch.int32, pin_memory=True)
        self.lp = torch.zeros((ring,) + tuple(dev["lp"].shape), dtype=torch.float32, pin_memory=True)

    def copy(self, r: int) -> None:
        self.ids[r].copy_(self.dev["ids"], non_blocking=True)
        self.lp[r].copy_(self.dev["lp"], non_blocking=True)

    def records(self, r: int, row0: int, count: int) -> list:
        return logprob_records(self.ids[r, row0:row0 + count], self.lp[r, row0:row0 + count])


def logit_ctl_image(controls, vocab: int, stop_free_len: int = 0):
    """The device image of one slot's token controls -> ``(pc_logit_ctl bytes, allowed row | None)``: the block with
    ``stop_free_len`` as given (``len_at_entry + min_new_tokens - 1`` for a sequence entering a device loop; 0 where the controls
    hold no stop ids back) and the uint32 ``[ceil(vocab / 32)]`` row with the bit of every allowed id set.  ``controls`` None: the
    neutral block, under which the adjusted row is the raw row.  Ids must lie inside the vocabulary (``check_token_controls``)."""
    if controls is None:
        return _native.logit_ctl_bytes(), None
    check_token_controls(controls, vocab=vocab)
    bits = None
    if controls.allowed is not None:
        bits = _history_bits(controls.allowed, vocab).numpy().view(np.uint32)
    return _native.logit_ctl_bytes(controls.bias, bits is not None, stop_free_len if controls.stop_ids else 0, controls.stop_ids), bits


class _TokenControlled:
    """What every device loop shares for the token-control node: ``with_controls(controls, ...)`` builds the loop with
    one more node between the lm_head and its advance / verify launch -- ``pc_logit_adjust`` into a fixed ``[rows][V]`` buffer the
    launch then reads instead of the logits (the log-probability node keeps reading the raw rows).  ``controls``: None -- plain
    ``cls(...)``, no node, today's graph keys and launches; a ``TokenControls`` for every sequence, a list with one (or None) per
    sequence, or True: the node with neutral blocks, for a serving loop whose requests bring their own at admission."""

    ctl_on = False                   # the step carries the node (the graph key gains ("ctl",))
    _controls = None                 # what the slots are filled with when the loop is built
    _cs = None                       # the node's state: blocks, allowed rows, the adjusted buffer (LlamaHIP._ctl_state)

    @classmethod
    def with_controls(cls, controls, *args, **kw):
        """``cls(*args, **kw)`` with the node (None: without).  The option is in place before ``__init__`` builds state and graph
        key, and the constructors keep their signatures."""
        loop = cls.__new__(cls)
        if controls is not None:
            check_token_controls(TokenControls(), getattr(cls, "prompt_rows", False))
            loop.ctl_on, loop._controls = True, None if controls is True else controls
        loop.__init__(*args, **kw)
        return loop

    def _controls_of(self, j: int):
        c = self._controls
        return c[j] if isinstance(c, (list, tuple)) else c


class GreedyLoop(_TokenControlled):
    """Greedy decode steps that never leave the GPU (reference loop: generation_engine.py:123-168, greedy branch).

    Every step is one replay of a captured hipGraph whose last node (``pc_greedy_advance``) takes the argmax of the
    step's logits and writes it -- with position + 1 and past length + 1 -- into the device words the next replay reads
    its inputs from.  The host only enqueues replays (as far ahead as it likes) and picks tokens up from a small ring
    through pinned memory when it needs them for stop conditions; there is no ``int(argmax)`` sync, no H2D fill and no
    logits copy per token.  ``enqueue()`` -> slot index; ``token(i)`` waits for slot i only.
    ``logprobs`` = n (None: off, and then nothing below exists): the step gains one node behind the advance,
    ``pc_token_logprobs`` over the row the advance just read at the token it left in ``ids[0]``; ``logprobs(i)`` -> the one
    record of ``token(i)``."""

    RING = 4096

    @torch.inference_mode()
    def __init__(self, model: "LlamaHIP", arena: KVArena, token: int, position: int, max_new: int, ctr0: int = 0,
                 logprobs: Optional[int] = None):
        self.m = model
        self.lp_n = check_logprobs(logprobs)
        self._lp = None if self.lp_n is None else _LogprobRing(model._lp_state(("loop",), 1, self.lp_n), self.RING)
        past_len = arena.length
        if self.ctl_on:                  # the first step draws generated token number 1 at arena length past_len
            self._cs = model._ctl_state(("loop",), 1, 1)
            model._ctl_fill(self._cs, 0, self._controls, past_len)
        need = past_len + max_new + 2
        if need > arena.cap:
            arena = arena.grown(max(need, 2 * arena.cap))
        self.arena = arena
        st = model._loop_state()
        self.st = st
        # The loop state (token / position / past words, ring, counter) is ONE set of device words per model: the newest
        # loop owns it.  A loop that was superseded (two generate() generators advanced alternately on one model) must
        # not keep replaying over the other's words -- enqueue() refuses instead of corrupting both sequences.
        model._live_loop = self
        dev = model.device
        st["ids"].copy_(torch.tensor([token], dtype=torch.int64), non_blocking=True)
        st["pos"].copy_(torch.tensor([position], dtype=torch.int32), non_blocking=True)
        st["ctr"].fill_(ctr0)
        self.ctr0 = ctr0                 # the device step counter at slot 0 (slot i's token lands in ring[(ctr0 + i) % RING])
        self.len0 = past_len
        self.n = 0                       # replays enqueued
        self._last_ent = None
        self.events = []                 # (start, end) per slot
        self.host = torch.empty(self.RING, dtype=torch.int32, pin_memory=True)

    @torch.inference_mode()
    def enqueue(self) -> int:
        m, a, st = self.m, self.arena, self.st
        if getattr(m, "_live_loop", None) is not self:
            raise RuntimeError("GreedyLoop: another greedy loop on this model took over the device loop state "
                               "(one device-side greedy generation per model at a time; set "
                               "GenerationEngine.device_greedy_loop = False to interleave generations)")
        past_len = self.len0 + self.n
        m._lo_mode = m._tail_mode(a, 1, past_len)
        ent = self._graph(a, past_len)
        # host-known words of the step (the kernels read past_len / tail base from the device)
        if self.n == 0 or ent is not self._last_ent:
            st["past"][0:1].fill_(past_len)
            if m._lo_mode == 2:
                st["past"][1:2].fill_(a.tail_base)
        self._last_ent = ent
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ent[0].replay()
        e1.record()
        i = self.n
        r = (self.ctr0 + i) % self.RING
        self.host[r: r + 1].copy_(st["ring"][r: r + 1], non_blocking=True)
        if self._lp is not None:
            self._lp.copy(r)
        done = torch.cuda.Event()
        done.record()
        self.events.append((e0, e1, done))
        a.length = past_len + 1
        m._tail_done(a, m._lo_mode, 1, past_len)
        self.n += 1
        return i

    def token(self, i: int) -> int:
        self.events[i][2].synchronize()
        return int(self.host[(self.ctr0 + i) % self.RING])

    def logprobs(self, i: int) -> list:
        """One record per token of ``token(i)``: ``[(token, logprob, [(id, logprob)] * n)]`` (a loop built with ``logprobs=n``)."""
        self.events[i][2].synchronize()
        return self._lp.records((self.ctr0 + i) % self.RING, 0, 1)

    def close(self, consumed: int) -> None:
        """The generation ended after ``consumed`` of the enqueued steps were used: a look-ahead replay enqueued past the
        stop wrote one row too many -- the arena's length goes back to the real sequence, and the loop state is released."""
        if consumed < self.n:
            self.arena.length = self.len0 + consumed
            if self.arena.tail_base >= 0:            # (the residual tail is valid while tail_base + tail_len == length)
                self.arena.tail_len = max(0, self.arena.length - self.arena.tail_base)
        if getattr(self.m, "_live_loop", None) is self:
            self.m._live_loop = None

    def elapsed_ms(self, i: int) -> float:
        e0, e1, done = self.events[i]
        done.synchronize()
        return e0.elapsed_time(e1)

    def _graph(self, arena: KVArena, past_len: int):
        return self.m._loop_graph(arena, past_len, logprobs=self.lp_n, ctl=self._cs)


def _history_bits(ids, vocab: int) -> torch.Tensor:
    """Host bitmap (int32 [ceil(vocab / 32)]) with the bit of every id in ``ids`` set (ids outside the vocabulary ignored)."""
    bits = np.zeros((vocab + 31) // 32, dtype=np.uint32)
    a = np.asarray(list(ids), dtype=np.int64)
    a = a[(a >= 0) & (a < vocab)]
    np.bitwise_or.at(bits, a >> 5, (np.uint32(1) << (a & 31).astype(np.uint32)))
    return torch.from_numpy(bits.view(np.int32))


def sample_params_block(params, seed: int) -> bytes:
    """The ``pc_sample_params`` image of a generation's ``GenerationParameters``, canonical: every decision the reference takes
    in double (generation_engine.py:32-42 and the greedy rule of :159) is taken here, so that the kernel's fp32 re-tests of
    the same thresholds cannot decide otherwise.  Greedy -> T = 0; no temperature warper -> T = 1; no top-p warper -> top_p = 1;
    no penalty processor -> rp = 1; top_k clamped into [-1, 2^31 - 1] (<= 0: off).  What stays is a top_p in [1e-8, 1) that
    rounds to 1.0f (top-p off on the device; the mass involved is below 1e-7)."""
    T, rp, top_p, top_k = float(params.temperature), float(params.repetition_penalty), float(params.top_p), int(params.top_k)
    if params.greedy:
        T = 0.0
    elif not (T >= 1e-5 and T != 1.0):
        T = 1.0
    if not (1e-8 <= top_p < 1.0):
        top_p = 1.0
    if not rp > 1.0:
        rp = 1.0
    top_k = -1 if top_k <= 0 else min(top_k, 2 ** 31 - 1)
    return _native.sample_params_bytes(T, rp, top_p, top_k, seed)


class SampleLoop(GreedyLoop):
    """Sampled decode steps that never leave the GPU (reference loop: generation_engine.py:123-168, sampling branch :149-163).

    GreedyLoop's protocol and state, with ``pc_sample_advance`` as the graph's last node: the reference's logits chain and one
    draw per step from the parameter block and the history bitmap of the loop state (device words, so one captured graph
    serves every parameter set).  The first token was drawn from the prefill logits at step 0 (``LlamaHIP.sample_token``);
    the loop's steps continue that random stream at 1, 2, ..."""

    @torch.inference_mode()
    def __init__(self, model: "LlamaHIP", arena: KVArena, token: int, position: int, max_new: int, params, seed: int,
                 history_ids, logprobs: Optional[int] = None):
        super().__init__(model, arena, token, position, max_new, ctr0=1, logprobs=logprobs)
        model._sample_state_fill(self.st, params, seed, history_ids)

    def _graph(self, arena: KVArena, past_len: int):
        return self.m._loop_graph(arena, past_len, sample=True, logprobs=self.lp_n, ctl=self._cs)


class LookupLoop(_TokenControlled):
    """Greedy decode with prompt-lookup drafts, on the device: up to ``k + 1`` tokens per weight stream.

    One step = ``pc_lookup_draft`` (copy the ``k`` tokens that followed the most recent earlier occurrence of the history's last
    few tokens) -> the ordinary ``k + 1``-row forward over the ids / positions / past length in the loop's device words ->
    ``pc_lookup_verify`` (per-row argmax; the longest draft prefix the model agrees with, plus its own next token, goes to the
    ring and advances the words by that many rows).  The step is ONE captured graph that serves the whole loop; the host only
    enqueues replays and reads ``{count, tokens}`` records through pinned memory.  How many tokens a replay yields is known on
    the device only, so the loop is safe by construction instead of by host bookkeeping: the arena holds
    ``len0 + max_new + k + 2`` rows, the device ``budget`` word keeps the past length at or below ``len0 + max_new``, a step
    writes rows ``[past, past + k]`` only, and a replay with no budget left changes nothing but its (empty) record.

    ``enqueue()`` -> step index; ``tokens(i)`` -> the 0..k+1 tokens of step i (waits for that step only);
    ``close(consumed_tokens)``.  ``PC_DEVICE_LOOKUP=0`` runs the same three stages eagerly with a host read per step."""

    RING = 1024
    ROWS_MAX = 16
    multi = True                     # a step yields a list of tokens (GenerationEngine)
    device_loop = os.environ.get("PC_DEVICE_LOOKUP", "1") != "0"
    graph_tag = ()                   # appended to the step's graph key (a subclass with another last stage)

    @torch.inference_mode()
    def __init__(self, model: "LlamaHIP", arena: KVArena, token: int, position: int, max_new: int, k: int, corpus_ids, nmax: int = 3,
                 logprobs: Optional[int] = None):
        if not 1 <= k < self.ROWS_MAX:
            raise ValueError(f"LookupLoop: k = {k} outside 1..{self.ROWS_MAX - 1}")
        self.m, self.k, self.nmax = model, int(k), int(nmax)
        # logprobs = n: one more stage behind the verify, over the k + 1 rows at the tokens it left in its int32 row scratch
        self.lp_n = check_logprobs(logprobs)
        self._lp = None if self.lp_n is None else _LogprobRing(model._lp_state(("lookup",), k + 1, self.lp_n), self.RING)
        arena.materialize()
        len0 = arena.length
        if self.ctl_on:                  # row i of a step draws token number past - len0 + 1 + i
            self._cs = model._ctl_state(("lookup",), 1, k + 1)
            model._ctl_fill(self._cs, 0, self._controls, len0)
        need = len0 + max_new + k + 2
        if need > arena.cap:
            arena = arena.grown(max(need, 2 * arena.cap))
        self.arena = arena
        self.len0, self.max_new = len0, int(max_new)
        # the attention's split counts (and its kernel) for the WHOLE loop, from an upper bound of the keys a step can see
        # (64-row buckets so that generations of similar length share a graph): the tokens of a generation do not depend on how
        # far ahead the host enqueues, and the stepped mode runs the very same launches
        self.kv_ceiling = min((len0 + max_new + k + 1 + 63) // 64 * 64, arena.cap)
        hist0 = [int(t) for t in corpus_ids] + [int(token)]
        st = self.st = model._lookup_state(len(hist0) + max_new)
        model._live_loop = self
        st["past"][0:1].fill_(len0)
        st["hist_len"].fill_(len(hist0))
        st["budget"].fill_(max_new)
        st["pos"].fill_(position)
        st["ids"].fill_(int(token))
        st["ndraft"].zero_()
        st["ctr"].zero_()
        st["hist"][:len(hist0)].copy_(torch.tensor(hist0, dtype=torch.int32))
        self.n = 0
        self.events = []
        self.host = torch.zeros((self.RING, k + 2), dtype=torch.int32, pin_memory=True)
        self.ring = st["ring"][:self.RING * (k + 2)].view(self.RING, k + 2)

    def _step(self):
        """The three stages of one step on the current stream (captured, or launched eagerly by the stepped mode)."""
        m, st, k, n = self.m, self.st, self.k, _native
        V = m.config.vocab_size
        n.lookup_draft(st["hist"], st["hist_len"], st["ids"], st["pos"], st["ndraft"], k, self.nmax)
        out = m._forward_skinny(st["ids"][:k + 1], st["pos"][:k + 1], st["past"], self.arena, 1, k + 1, self.kv_ceiling - (k + 1),
                                False, None)
        if self._cs is not None:         # the verify reads the adjusted rows; the log-probability node keeps the raw ones
            m._ctl_node(self._cs, out, V, 1, k + 1, st["past"])
            self._verify(self._cs["out"], V, self._cs["ldo"])
        else:
            self._verify(out, V)
        if self._lp is not None:
            m._lp_node(self._lp.dev, out, k + 1, st[self.row_tokens], 1, self.lp_n)
        return out

    row_tokens = "amax"              # the int32 scratch the verify stage leaves every row's token in

    def _verify(self, out, V: int, ld: Optional[int] = None) -> None:
        """The last stage of a step: which rows' tokens are emitted, and the state advance."""
        st = self.st
        _native.lookup_verify(out, V if ld is None else ld, V, self.k + 1, st["amax"], st["hist"], st["hist_len"], st["ids"], st["pos"], st["past"],
                              st["ndraft"], st["budget"], st["ring"], st["ctr"], self.RING)

    @torch.inference_mode()
    def enqueue(self) -> int:
        m, a = self.m, self.arena
        if getattr(m, "_live_loop", None) is not self:
            raise RuntimeError("LookupLoop: another device loop on this model took over (one device-side generation per model "
                               "at a time)")
        m._lo_mode = 0                     # appended rows carry no residual planes, as in default decode
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if self.device_loop:
            ent = m._lookup_graph(self)
            e0.record()
            ent[0].replay()
        else:
            e0.record()
            self.logits = self._step()     # (the stepped mode keeps the step's logits for whoever wants to look)
        e1.record()
        i = self.n
        r = i % self.RING
        self.host[r].copy_(self.ring[r], non_blocking=True)
        if self._lp is not None:
            self._lp.copy(r)
        done = torch.cuda.Event()
        done.record()
        self.events.append((e0, e1, done))
        if not self.device_loop:
            done.synchronize()             # the host read per step
        m._tail_done(a, 0, 1, self.len0)
        self.n += 1
        return i

    def tokens(self, i: int):
        self.events[i][2].synchronize()
        rec = self.host[i % self.RING]
        c = int(rec[0])
        return [int(t) for t in rec[1:1 + c]]

    def logprobs(self, i: int) -> list:
        """One record per token of ``tokens(i)``, in its order: rows ``i < emit`` of the step (a loop built with ``logprobs=n``)."""
        self.events[i][2].synchronize()
        return self._lp.records(i % self.RING, 0, int(self.host[i % self.RING][0]))

    def close(self, consumed_tokens: int) -> None:
        """The generation used ``consumed_tokens`` of the tokens the enqueued steps produced: the arena's length becomes the
        real sequence (rows behind it -- rejected drafts, steps past a stop -- are rewritten before anything reads them), and
        the loop state is released."""
        self.arena.length = self.len0 + consumed_tokens
        self.arena.tail_base, self.arena.tail_len = -1, 0
        if getattr(self.m, "_live_loop", None) is self:
            self.m._live_loop = None

    def elapsed_ms(self, i: int) -> float:
        e0, e1, done = self.events[i]
        done.synchronize()
        return e0.elapsed_time(e1)


class SampleLookupLoop(LookupLoop):
    """Sampled decode with prompt-lookup drafts, on the device: ``LookupLoop`` whose last stage is
    ``pc_lookup_verify_sample``.  Row i of a step is drawn by ``pc_sample_advance``'s rule at Philox step ``draws + i`` under the
    penalty history it would have had drafts 1..i been emitted; the draws that equal their drafts are accepted and the first one
    that differs is emitted as it is, so token number n of a generation is drawn at step n whatever the drafts were: on identical
    logits the tokens are ``SampleLoop``'s, one for one.  The state gains the parameter block and history bitmap of
    ``SampleLoop``, ``draws`` (1: the first token was drawn at step 0, ``LlamaHIP.sample_token``) and per-row scratch.  One
    graph serves every parameter set; protocol, memory-safety argument and the stepped mode are ``LookupLoop``'s."""

    graph_tag = ("sample",)
    row_tokens = "row_token"

    @torch.inference_mode()
    def __init__(self, model: "LlamaHIP", arena: KVArena, token: int, position: int, max_new: int, k: int, corpus_ids, params,
                 seed: int, history_ids, nmax: int = 3, logprobs: Optional[int] = None):
        super().__init__(model, arena, token, position, max_new, k, corpus_ids, nmax, logprobs)
        st = self.st
        model._lookup_sample_state(st)
        model._sample_state_fill(st, params, seed, history_ids)
        st["draws"].fill_(1)

    def _verify(self, out, V: int, ld: Optional[int] = None) -> None:
        st = self.st
        _native.lookup_verify_sample(out, V if ld is None else ld, V, self.k + 1, st["params"], st["bits"], st["row_bits"], st["draws"], st["row_token"],
                                     st["hist"], st["hist_len"], st["ids"], st["pos"], st["past"], st["ndraft"], st["budget"],
                                     st["ring"], st["ctr"], self.RING)


def lookup_admit_history(corpus, token: int, max_new: int, hist_cap: int) -> list:
    """The draft history a sequence enters a ``LookupSlotLoop(each=True)`` with: ``corpus ++ [token]``, the OLDEST corpus ids
    dropped until ``hist_len + max_new <= hist_cap`` (the buffer is fixed when the loop is built: the captured step holds it).
    ValueError when ``max_new + 1`` alone does not fit."""
    if max_new + 1 > hist_cap:
        raise ValueError(f"lookup admission: max_new + 1 = {max_new + 1} ids do not fit a draft history of {hist_cap}")
    keep = hist_cap - max_new - 1
    ids = [int(t) for t in corpus]
    return ids[max(0, len(ids) - keep):] + [int(token)]


def lookup_prompt_history(corpus, ids, max_new: int, hist_cap: int) -> list:
    """The draft history a sequence enters a ``LookupSlotLoop(prompt_rows=True)`` with through ``admit_prompt``: ``corpus ++ ids``
    with the whole question ``ids`` kept and the OLDEST corpus ids dropped until the history, the first token and the rest of the
    budget fit (``len + max_new <= hist_cap``) -- the ids ``lookup_admit_history`` keeps behind a serial prefill of ``ids``.
    ValueError when ``len(ids) + max_new`` alone does not fit."""
    q = len(ids)
    if q + max_new > hist_cap:
        raise ValueError(f"lookup admission: a question of {q} ids and max_new = {max_new} do not fit a draft history of {hist_cap}")
    keep = hist_cap - max_new - q
    c = [int(t) for t in corpus]
    return c[max(0, len(c) - keep):] + [int(t) for t in ids]


def _is_sampled(params) -> bool:
    """Whether ``params`` take the sampled chain (None / greedy without a repetition penalty: the argmax of the raw row)."""
    return params is not None and not (params.greedy and params.repetition_penalty <= 1.0)


def _slot_trunks(trunks, lengths) -> list:
    """The shared trunks of a slot loop, normalised and checked: per sequence ``(leader index | None, T)`` -- rows [0, T) of the
    sequence's arena are the bytes of the same rows of the leader's, and every step reads them from the leader's arena once for
    the group.  None: nobody shares.  A leader leads itself over the same T rows, and both arenas (``lengths``) hold them."""
    n = len(lengths)
    trunks = [(None, 0)] * n if trunks is None else [(None, 0) if l is None else (int(l), int(T)) for l, T in trunks]
    for k, (l, T) in enumerate(trunks):
        assert l is None or (trunks[l] == (l, T) and 0 < T <= lengths[k] and T <= lengths[l]), (k, trunks)
    return trunks


def _trunk_verify(a, la, T: int, who: str, leader: str) -> None:
    """``PC_TRUNK_VERIFY=1``: rows [0, T) of arena ``a`` must be the bytes of the same rows of its trunk leader's arena ``la``."""
    if os.environ.get("PC_TRUNK_VERIFY", "0") == "1" and la is not a and not torch.equal(a.buf[:, :, :, :, :T], la.buf[:, :, :, :, :T]):
        raise RuntimeError(f"PC_TRUNK_VERIFY: rows [0, {T}) of {who} differ from its trunk leader's ({leader})")


def _fill_arm_block(arr, header, fields: dict, seed: int, params, stop_ids, history, vocab: int) -> int:
    """The host block of ``pc_slot_arm`` / ``pc_lookup_slot_arm`` into ``arr`` (writable uint8): the header (``header``: the ctypes
    image, ``SlotArmBlock`` | ``LookupSlotArmBlock``) with ``fields`` by name, ``hist_words``, the seed's low 63 bits, the parameter
    block of ``params`` and eight stop ids (-1: none), then the penalty bitmap of ``history`` (zeros where ``params`` do not
    sample).  -> the offset behind the bitmap, padded to 8 bytes (where the lookup block's history ids go)."""
    hw, sampled = (vocab + 31) // 32, _is_sampled(params)
    b = header.from_buffer(arr)
    for name, v in fields.items():
        setattr(b, name, v)
    b.hist_words = hw
    b.seed = int(seed) & (2 ** 63 - 1)
    b.params = _native.SampleParams.from_buffer_copy(sample_params_block(params, 0) if sampled else
                                                     _native.sample_params_bytes(0.0, 1.0, 1.0, -1, 0))   # greedy: argmax of the raw row
    for j in range(8):
        b.stop_ids[j] = stop_ids[j] if j < len(stop_ids) else -1
    del b
    n0 = ctypes.sizeof(header)
    arr[n0:n0 + 4 * hw].view(np.int32)[:] = _history_bits(history, vocab).numpy() if sampled else 0
    return n0 + ((4 * hw + 7) & ~7)


class _SlotLoopHost(_TokenControlled):
    """The host side of a batched device loop, once for ``SlotLoop`` and ``LookupSlotLoop``: slots and arenas,
    shared trunks, the per-sequence tables, admission into a running ``each=True`` loop through a ring of pinned arm blocks, and
    the replay / ring / event protocol ``GenerationEngine`` drives.  What a leaf says itself: the ring record (``_record``), the
    split counts, its state words and graph, the arm launch, when a slot may be taken again and its own bookkeeping."""

    RING = 1024
    MAX_SLOTS = 16
    MAX_ROWS = 64                    # rows of one step, S * (k + 1): what the weight-streaming projections take
    k = 0                            # draft rows per slot
    kv = "fp16"                      # what the step's attention reads: the fp16 arenas, or int8 images of them (SlotLoop(kv="int8"))
    lp_n = None                      # logprobs = n: the step ends in the log-probability node at top_n = n
    _lp = None
    prompt_rows = False
    ctr0 = 0                         # the device step counter at replay 0 (step i's record lands in ring row (ctr0 + i) % RING)

    @classmethod
    def with_logprobs(cls, logprobs: Optional[int], *args, **kw):
        """``cls(*args, **kw)`` whose step ends in the log-probability node at ``top_n = logprobs`` (None: plain ``cls(...)``).  The
        option is in place before ``__init__`` builds state and graph key, and the constructors keep their signatures."""
        return cls.with_options(logprobs, None, *args, **kw)

    @classmethod
    def with_options(cls, logprobs: Optional[int], controls, *args, **kw):
        """``with_logprobs`` and ``with_controls`` in one: both options are in place before ``__init__`` runs."""
        loop = cls.__new__(cls)
        loop.lp_n = check_logprobs(logprobs, cls.prompt_rows)
        if controls is not None:
            check_token_controls(TokenControls(), cls.prompt_rows)
            loop.ctl_on, loop._controls = True, None if controls is True else controls
        loop.__init__(*args, **kw)
        return loop

    def _ctl_tag(self):
        return self._lp_tag()

    def _build(self, model, arenas, tokens, positions, max_new, params, seeds, histories, stop_ids, slots, slot_index, trunks, each,
               max_keys, corpora=None, hist_cap=None) -> None:
        """``each``: the step with per-slot sampling state -- ``max_new`` / ``params`` / ``stop_ids`` are one value for all
        sequences or a list with one per sequence, and every initial sequence enters through ``admit``'s path, at replay 0."""
        n, k = len(arenas), self.k
        idx = list(range(n)) if slot_index is None else [int(i) for i in slot_index]
        S = slots if slots is not None else next(b for b in (1, 2, 4, 8, 16) if b >= max(idx) + 1)
        assert 1 <= n and len(set(idx)) == n and 0 <= min(idx) and max(idx) < S <= self.MAX_SLOTS, (n, idx, S)
        assert S * (k + 1) <= self.MAX_ROWS, (S, k)
        per = lambda v: list(v) if each and isinstance(v, (list, tuple)) else [v] * n
        max_news, paramss = per(max_new), per(params)
        stops = list(stop_ids) if each and len(stop_ids) and isinstance(stop_ids[0], (list, tuple)) else [tuple(stop_ids)] * n
        assert len(tokens) == n and len(positions) == n and len(max_news) == n and len(paramss) == n and len(stops) == n
        assert (corpora is None or len(corpora) == n) and (each or (len(stop_ids) <= 8 and max_new >= 1))
        self.m, self.S, self.each, self.max_new = model, S, bool(each), max(max_news)
        self.idx, self.arenas, self.len0, self.trunks = [], [], [], []
        self._start = []                  # the replay at which sequence k entered the loop
        self._killed = []                 # step count at which kill(k) took effect
        self._slot_seq = [None] * S       # the newest sequence of every slot
        self._retired = set()
        self.n = 0
        self.events = {}                  # step -> (start, end, tokens on the host); steps the ring no longer holds are dropped
        if not each:
            arenas = [self._prepared(a, max_new) for a in arenas]
        trunks = _slot_trunks(trunks, [a.length for a in arenas])
        if not each:
            for j, (l, T) in enumerate(trunks):
                if l is not None:
                    _trunk_verify(arenas[j], arenas[l], T, f"sequence {j}", f"sequence {l}")
        self._split_counts([a.length for a in arenas], max_news, trunks, max_keys)
        st = self.st = self._make_state(tokens, corpora, hist_cap)
        if self.kv == "int8":             # one int8 image per slot index, owned by the loop state and allocated before any capture
            self.qcap, self.kvq = model._slot_kvq(st, S, self._image_rows(arenas, max_news, max_keys))
        model._live_loop = self
        self.logits = st["logits"]
        if self.lp_n is not None:
            self._lp = _LogprobRing(model._lp_state(self._lp_tag(), S * (k + 1), self.lp_n), self.RING)
        if self.ctl_on:                   # every slot starts neutral; a sequence's block is written where it enters
            self._cs = model._ctl_state(self._ctl_tag(), S, k + 1)
            for s in range(S):
                model._ctl_fill(self._cs, s, None, 0)
        self.host = torch.zeros((self.RING, S) + self._record, dtype=torch.int32, pin_memory=True)
        self._ring = st["ring"].view((S, self.RING) + self._record)
        if each:
            st["live"].zero_()
            st["leader"].fill_(-1)
            st["trunk"].zero_()
            nbytes, self._arm_state = self._arm_setup((model.config.vocab_size + 31) // 32)
            self._arm_ring = [[torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True), torch.cuda.Event(), False] for _ in range(4)]
            self._arm_next = 0
            if self.ctl_on:               # ... and beside every arm block the pinned image of the slot's token controls
                self._ctl_ring = [model._ctl_pinned() for _ in self._arm_ring]
            seeds = [0] * n if seeds is None else list(seeds)
            histories = [()] * n if histories is None else list(histories)
            for j, (l, T) in enumerate(trunks):
                self._admit(idx[j], arenas[j], tokens[j], positions[j], max_news[j], paramss[j], seeds[j], histories[j], stops[j],
                            None if l is None else (idx[l], T), None if corpora is None else corpora[j],
                            controls=self._controls_of(j))
            return
        seats = [self._seat(s, a) for s, a in zip(idx, arenas)]
        for j, (s, a, trunk, seat) in enumerate(zip(idx, arenas, trunks, seats)):
            self._enter(s, seat[0], trunk, max_new, stop_ids)
            self._quantise_entry(s, a)
            if self.ctl_on:
                model._ctl_fill(self._cs, s, self._controls_of(j), a.length)

        def col(vals, dtype, fill=0):
            t = torch.full((S,), fill, dtype=dtype)
            for s, v in zip(idx, vals):
                t[s] = v
            return t
        st["kv_base"].copy_(col([base for _, base, _ in seats], torch.int64), non_blocking=True)
        st["cap"].copy_(col([cap for _, _, cap in seats], torch.int32), non_blocking=True)
        st["len"].copy_(col(self.len0, torch.int32), non_blocking=True)
        st["live"].copy_(col([1] * n, torch.int32), non_blocking=True)
        st["leader"].copy_(col([-1 if l is None else idx[l] for l, _ in trunks], torch.int32, -1), non_blocking=True)
        st["trunk"].copy_(col([T for _, T in trunks], torch.int32), non_blocking=True)
        st["budget"].copy_(col([max_new] * n, torch.int32), non_blocking=True)
        self._fill_state(col, tokens, positions, max_new, params, seeds, histories, stop_ids)
        torch.cuda.current_stream().synchronize()        # (the pageable sources of the copies above may go now)

    def _prepared(self, a, max_new: int):
        """The arena a sequence decodes in: room for every row the loop can write (no address may move under the captured step),
        and rows are appended without residuals: a residual tail ends here."""
        need = a.length + max_new + self.k + 2
        if need > a.cap:
            a = a.grown(max(need, 2 * a.cap))
        self.m._tail_done(a, 0, 1, a.length)
        return a

    def _image_rows(self, arenas, max_news, max_keys) -> int:
        """kv="int8": the rows per plane the images must hold -- every arena's capacity (the cap word bounds ``len``)."""
        return max([a.cap for a in arenas] + [int(max_keys or 0)])

    def _seat(self, s: int, a):
        """-> (what the loop keeps of the arena a sequence enters slot ``s`` with, the slot's ``kv_base`` word, its ``cap`` word)."""
        return a, a.buf.data_ptr(), a.cap

    def _quantise_entry(self, s: int, a) -> None:
        """kv="int8": rows [0, length) of the arena a sequence enters with -> the image of slot ``s`` (``pc_kv_quant_q8_rows``), on
        the loop's stream behind ``materialize()`` and in front of the arm launch or the first replay."""
        if self.kv != "int8":
            return
        if a.cap > self.qcap:
            raise RuntimeError(f"{type(self).__name__}: the arena of slot {s} holds {a.cap} rows, the loop's int8 images {self.qcap} "
                               "(build the loop with max_keys >= the largest arena capacity)")
        m = self.m
        _native.kv_quant_q8_rows(a.buf, a.cap, a.length, m.L * 2 * m.Hkv, m.D, self.kvq[s], self.qcap)

    def _trunk_verify_images(self, s: int, leader: int, T: int) -> None:
        """kv="int8" under ``PC_TRUNK_VERIFY=1``, behind ``_quantise_entry``: rows [0, T) of every plane of the image of slot ``s``
        -- codes and scales -- must be the bytes of the same rows of its trunk leader's image, which the step reads in their place
        (``pc_kv_quant_q8_rows`` is row-local, so equal fp16 rows give equal image rows)."""
        if self.kv != "int8" or leader == s or os.environ.get("PC_TRUNK_VERIFY", "0") != "1":
            return
        m = self.m
        P, qcap, D = m.L * 2 * m.Hkv, self.qcap, m.D

        def rows(img):
            return img[:P * qcap * D].view(P, qcap, D)[:, :T], img[P * qcap * D:P * qcap * (D + 4)].view(torch.int32).view(P, qcap)[:, :T]
        (c, sc), (lc, lsc) = rows(self.kvq[s]), rows(self.kvq[leader])
        if not (torch.equal(c, lc) and torch.equal(sc, lsc)):
            raise RuntimeError(f"PC_TRUNK_VERIFY: image rows [0, {T}) of the sequence for slot {s} differ from its trunk leader's "
                               f"(slot {leader})")

    def _enter(self, s: int, a, trunk, max_new: int, stop_ids) -> int:
        """Sequence number ``len(arenas)`` sits in slot ``s`` from replay ``n`` on: one more row of every per-sequence table."""
        k, prev = len(self.arenas), self._slot_seq[s]
        self.arenas.append(a)
        self.len0.append(a.length)
        self.idx.append(s)
        self.trunks.append(trunk)
        self._start.append(self.n)
        self._killed.append(None)
        self._slot_seq[s] = k
        self._entered(k, prev, max_new, stop_ids)
        return k

    def _admit_arena(self, past):
        name = type(self).__name__
        if not self.each:
            raise RuntimeError(f"{name}.admit needs a loop built with each=True")
        a = self.m._loop_arena(past)
        if a is None:
            raise RuntimeError(f"{name}.admit: the cache is not a staged batch-1 arena")
        return a

    def _admit(self, s: int, a, token, position, max_new, params, seed, history, stop_ids, trunk, corpus=None, question=None,
               controls=None) -> int:
        """``question`` (``LookupSlotLoop.admit_prompt``): the ids still to be prefilled, ``token`` the first of them -- the arena
        also gets room for their rows, and the leaf's ``_admit_check`` / ``_arm`` see them.  ``controls`` (a loop built with the
        token-control node): the sequence's ``TokenControls``; None writes the neutral block, so nothing of the slot's previous
        sequence stays."""
        m, name = self.m, type(self).__name__
        if controls is not None and not self.ctl_on:
            raise ValueError(f"{name}.admit: the sequence carries token controls and the loop was built without the node "
                             "(with_controls / token_controls=True)")
        more = () if question is None else (question,)
        if getattr(m, "_live_loop", None) is not self:
            raise RuntimeError(f"{name}: another device loop on this model took over")
        if not 0 <= s < self.S or max_new < 1:
            raise ValueError(f"{name}.admit: slot {s} outside [0, {self.S}) or max_new < 1")
        running, extra, hist = self._admit_check(s, corpus, token, int(max_new), *more)
        if any(a is self.arenas[k] for k in running):
            raise RuntimeError(f"{name}.admit: the arena belongs to a running sequence")
        a.materialize()
        a = self._prepared(a, max_new + len(question or ()))
        leader, T = (-1, 0) if trunk is None else (int(trunk[0]), int(trunk[1]))
        if leader >= 0:
            lead = self._slot_seq[leader] if leader != s else None
            la = a if leader == s else (None if lead is None else self.arenas[lead])
            if not self.nsplit_trunk or la is None or not 0 < T <= a.length or T > la.cap:
                raise ValueError(f"{name}.admit: no trunk of {T} rows led by slot {leader} in this loop")
            _trunk_verify(a, la, T, f"the sequence for slot {s}", f"slot {leader}")
        stop_ids = [int(t) for t in stop_ids]
        assert len(stop_ids) <= 8, "at most 8 stop ids live on the device (the host kills for the rest)"
        # the next pinned block of the ring, once the launch that read it last has finished
        ent, ring_i = self._arm_ring[self._arm_next], self._arm_next
        self._arm_next = (self._arm_next + 1) % len(self._arm_ring)
        if ent[2]:
            ent[1].synchronize()
        arr = ent[0].numpy()
        held, base, cap = self._seat(s, a)
        fields = dict(slot=s, cap=cap, kv_base=base, len=a.length, pos=int(position), id=int(token), leader=leader,
                      trunk=T, budget=int(max_new), counter=self.ctr0 + self.n, **extra)
        off = _fill_arm_block(arr, self._arm_header, fields, seed, params, stop_ids, history, m.config.vocab_size)
        self._quantise_entry(s, a)
        if leader >= 0:
            self._trunk_verify_images(s, leader, T)
        if self.ctl_on:                   # the slot's block and allowed row, on the loop's stream in front of the arm launch: its
            m._ctl_fill(self._cs, s, controls, a.length, self._ctl_ring[ring_i])   # live = 1 stays the last store
        self._arm(ent[0], arr, off, hist, *more)
        ent[1].record()
        ent[2] = True
        return self._enter(s, held, (None, 0) if leader < 0 else (leader, T), max_new, stop_ids)

    def _set_length(self, a, length: int) -> None:
        a.length = length

    def _length_after(self, k: int, consumed: int) -> int:
        return self.len0[k] + consumed

    def retire(self, k: int, consumed: int) -> None:
        """Sequence ``k`` is over and its consumer used ``consumed`` of what it produced (``close``'s unit): its arena's ``length``
        goes to exactly that (``close``'s rule, for one sequence) -- before the buffer is staged again for the slot's next sequence."""
        self._set_length(self.arenas[k], self._length_after(k, int(consumed)))
        self._retired.add(k)

    @torch.inference_mode()
    def enqueue(self) -> int:
        if getattr(self.m, "_live_loop", None) is not self:
            raise RuntimeError(f"{type(self).__name__}: another device loop on this model took over (one device-side generation "
                               "per model at a time)")
        g = self._graph()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        i = self.n
        r = (self.ctr0 + i) % self.RING
        if i >= self.RING:
            self._ring_row_reused(i - self.RING)         # (row r still holds step i - RING)
        self.host[r].copy_(self._ring[:, r], non_blocking=True)
        if self._lp is not None:
            self._lp.copy(r)
        done = torch.cuda.Event()
        done.record()
        self.events[i] = (e0, e1, done)
        self.events.pop(i - self.RING, None)             # nobody can ask for a step whose ring row is being reused
        self.n += 1
        return i

    def _ring_row_reused(self, step: int) -> None:
        pass

    def slot_kv_bytes(self) -> int:
        """Bytes of K/V storage behind the loop's slots: the int8 images and fresh-row buffers of its state (``kv="int8"``) plus
        every distinct arena a sequence of the loop references."""
        size = lambda t: t.numel() * t.element_size()
        total = sum(map(size, self.kvq)) if self.kv == "int8" else 0
        total += sum(map(size, getattr(self, "fresh", ())))
        bufs = {a.buf.data_ptr(): a.buf for a in self.arenas if getattr(a, "buf", None) is not None}
        return total + sum(map(size, bufs.values()))

    def kill(self, k: int) -> None:
        """Switch sequence ``k`` off from the next replay on (ordered behind the replays already enqueued)."""
        s = self.idx[k]
        self.st["live"][s: s + 1].fill_(0)
        if self._killed[k] is None:
            self._killed[k] = self.n

    def elapsed_ms(self, i: int) -> float:
        e0, e1, done = self.events[i]
        done.synchronize()
        return e0.elapsed_time(e1)

    def close(self, consumed) -> None:
        """``consumed[k]``: how much of what sequence k produced its consumer used (``SlotLoop``: steps, ``LookupSlotLoop``:
        tokens).  Each arena's ``length`` goes to exactly that (rows behind it -- look-ahead replays, rejected drafts -- are dead:
        rewritten before anything reads them), and the loop state is released.  An ``each=True`` loop: a dict over the sequences
        that were not retired one by one."""
        if isinstance(consumed, dict):
            consumed = [consumed.get(k) for k in range(len(self.arenas))]
        for k, (a, c) in enumerate(zip(self.arenas, consumed)):
            if c is not None:
                self._set_length(a, self._length_after(k, int(c)))
        if getattr(self.m, "_live_loop", None) is self:
            self.m._live_loop = None


class SlotLoop(_SlotLoopHost):
    """Batched decode: up to 16 sequences, each in a batch-1 arena of its own, advanced together by one captured step.

    GreedyLoop's protocol over SLOTS.  Every replay runs the layer stack over ``S`` rows (one per slot), RoPE + append and the
    attention per slot over the slot's own arena (``pc_rope_append_slots`` / ``pc_attn_decode_slots``), and one advance launch
    (``pc_sample_advance_slots``) that draws every slot's token and rewrites the device words the next replay reads: token,
    position, length, live flag, step counter, history bitmap.  A slot stops on the device (stop id, step budget, full arena)
    and costs nothing afterwards but its GEMM row; the host mirrors those rules, so ``token(k, i)`` is None from the step after
    sequence k's last one.  ``kill(k)`` switches a sequence off between replays (stop strings).

    ``enqueue()`` -> step index; ``token(k, i)`` waits for step i only; ``logits`` is the ``[S][V]`` fp32 tensor of the last
    replay (row = slot index ``slot_index[k]``)."""

    _record = ()                     # a step leaves one token per slot: ``host`` is [RING][S]
    _arm_header = _native.SlotArmBlock

    @torch.inference_mode()
    def __init__(self, model: "LlamaHIP", arenas, tokens, positions, max_new: int, params=None, seeds=None, histories=None,
                 stop_ids=(), slots: Optional[int] = None, slot_index=None, trunks=None, each: bool = False,
                 max_keys: Optional[int] = None):
        self._alive = []                  # host mirror of the live words, after the newest step whose tokens were looked at
        self._seen = 0                    # steps whose tokens the mirror has taken in
        self._last = []                   # index of the last step that produced a token for sequence k (-1: none yet)
        self._max_new, self._stops = [], []
        self._active = []                 # sequences the mirror still follows
        self._build(model, arenas, tokens, positions, max_new, params, seeds, histories, stop_ids, slots, slot_index, trunks, each,
                    max_keys)

    def _split_counts(self, lens, max_news, trunks, max_keys) -> None:
        """From raw key counts.  ``max_keys``: the caller's bound, instead of this batch's."""
        m, S = self.m, self.S
        shared = any(l is not None for l, _ in trunks)
        if self.each:
            if max_keys is None:
                max_keys = max(l0 + mn for l0, mn in zip(lens, max_news)) + 1
            self.nsplit = m._slot_nsplit(S, int(max_keys))
            self.nsplit_trunk = m._slot_nsplit(1, int(max_keys)) if shared else 0
            return
        self.nsplit_trunk = 0
        if shared:
            self.nsplit_trunk = m._slot_nsplit(len({l for l, _ in trunks if l is not None}), max(T for _, T in trunks))
            self.nsplit = m._slot_nsplit(S, max(l0 - T for l0, (_, T) in zip(lens, trunks)) + max_news[0] + 1)
        else:
            self.nsplit = m._slot_nsplit(S, max(lens) + max_news[0] + 1)
        if max_keys is not None:
            self.nsplit = m._slot_nsplit(S, int(max_keys))
            if self.nsplit_trunk:
                self.nsplit_trunk = m._slot_nsplit(1, int(max_keys))

    def _make_state(self, tokens, corpora, hist_cap) -> dict:
        return self.m._slot_state(self.S)

    def _graph(self):
        return self.m._slot_graph(self.S, self.nsplit, self.nsplit_trunk, self.each, self.qcap if self.kv == "int8" else 0,
                                  logprobs=self.lp_n, ctl=self._cs)

    def _lp_tag(self):
        return ("slots", self.S)

    def _fill_state(self, col, tokens, positions, max_new, params, seeds, histories, stop_ids) -> None:
        """The state words of the loop over ``pc_sample_advance_slots``: one parameter block and one stop list for all slots."""
        st, S, n = self.st, self.S, len(tokens)
        sampled = _is_sampled(params)
        self.ctr0 = 1 if sampled else 0                # (a sampled stream drew its first token at step 0: sample_token)
        V = self.m.config.vocab_size
        st["pos"].copy_(col(positions, torch.int32), non_blocking=True)
        st["ids"].copy_(col(tokens, torch.int64), non_blocking=True)
        st["ctr"].fill_(self.ctr0)
        st["stop"].copy_(torch.tensor(list(stop_ids) + [-1] * (8 - len(stop_ids)), dtype=torch.int32), non_blocking=True)
        seeds = [0] * n if seeds is None else list(seeds)
        st["seeds"].copy_(col([sd & (2 ** 63 - 1) for sd in seeds], torch.int64), non_blocking=True)
        if sampled:
            blk = sample_params_block(params, 0)
            hist = torch.zeros((S, (V + 31) // 32), dtype=torch.int32)
            for s, h in zip(self.idx, histories):
                hist[s] = _history_bits(h, V)
            st["hist"].copy_(hist, non_blocking=True)
        else:
            blk = _native.sample_params_bytes(0.0, 1.0, 1.0, -1, 0)        # greedy: the argmax of the raw row
        st["params"].copy_(torch.frombuffer(bytearray(blk), dtype=torch.uint8))

    # ---- per-slot sampling state and admission (each=True) ---------------------------------------------------------------
    def _arm_setup(self, hw: int):
        """(every stream drew its first token at step 0: draws start at 1, and the counters index the ring only)"""
        st = self.st
        return _native.slot_arm_bytes(hw), _native.slot_state(
            st["kv_base"], st["cap"], st["len"], st["pos"], st["ids"], st["live"], st["leader"], st["trunk"], st["budget"], st["ctr"],
            st["draws"], st["seeds"], st["params_each"], st["stop_each"], st["hist"])

    @torch.inference_mode()
    def admit(self, slot_index: int, past, token: int, position: int, max_new: int, params, seed: int, history, stop_ids,
              trunk=None, controls=None) -> int:
        """A new sequence into slot ``slot_index`` of a running ``each=True`` loop, from the next replay on: the arena behind ``past``
        feeds ``token`` at ``position`` for at most ``max_new`` steps, with its own ``params`` (None / plain greedy: argmax), random
        stream ``seed`` (continuing at step 1), ``history`` ids and up to 8 ``stop_ids``.  ``trunk = (leader slot, T)``: rows [0, T) are
        read from the arena of that slot.  Only legal when the slot's previous sequence is over on the host mirror (stopped, out of
        budget or killed) and was retired.  -> the new sequence's index."""
        return self._admit(int(slot_index), self._admit_arena(past), token, position, max_new, params, seed, history, stop_ids, trunk,
                           controls=controls)

    def _admit_check(self, s: int, corpus, token, max_new: int):
        prev = self._slot_seq[s]
        if prev is not None:
            if self._alive[prev] and self._killed[prev] is None:
                raise RuntimeError(f"SlotLoop.admit: the sequence in slot {s} is still running")
            self._alive[prev] = False
            if prev in self._active:
                self._active.remove(prev)
        return self._active, {"draws": 1}, None

    def _arm(self, block, arr, off: int, hist) -> None:
        _native.slot_arm(block, off, self._arm_state, self.S)

    def _entered(self, k: int, prev, max_new: int, stop_ids) -> None:
        self._alive.append(True)
        self._last.append(-1)
        self._max_new.append(int(max_new))
        self._stops.append(set(int(t) for t in stop_ids))
        self._active.append(k)

    def _ring_row_reused(self, step: int) -> None:
        self._advance_mirror(step)                       # (the mirror takes the row's step in first)

    def _advance_mirror(self, upto: int) -> None:
        """Take the tokens of steps [seen, upto] into the host mirror of the live words (the rule of pc_sample_advance_slots)."""
        while self._seen <= upto:
            i = self._seen
            self.events[i][2].synchronize()
            row = self.host[(self.ctr0 + i) % self.RING]
            for k in list(self._active):
                if i < self._start[k]:
                    continue
                if not self._alive[k] or (self._killed[k] is not None and i >= self._killed[k]):
                    self._alive[k] = False
                    self._active.remove(k)
                    continue
                self._last[k] = i
                tok, j = int(row[self.idx[k]]), i - self._start[k]
                if tok in self._stops[k] or j + 1 >= self._max_new[k] or self.len0[k] + j + 2 >= self.arenas[k].cap:
                    self._alive[k] = False
                    self._active.remove(k)
            self._seen += 1

    def token(self, k: int, i: int) -> Optional[int]:
        """Token of sequence ``k`` at step ``i`` of the loop (the global replay index).  None: the sequence had stopped before
        that step, or had not been admitted yet."""
        self._advance_mirror(i)
        if i > self._last[k] or i < self._start[k]:
            return None
        return int(self.host[(self.ctr0 + i) % self.RING][self.idx[k]])

    def logprobs(self, k: int, i: int) -> list:
        """One record per token of ``token(k, i)``: ``[(token, logprob, [(id, logprob)] * n)]``, empty where ``token`` gives None (a
        loop built with ``logprobs=n``; the row of an idle slot is stale and never handed out)."""
        if self.token(k, i) is None:
            return []
        return self._lp.records((self.ctr0 + i) % self.RING, self.idx[k], 1)


class SlotLoopQ8(SlotLoop):
    """``SlotLoop`` whose attention reads int8 images of the slots' K / V rows (``LlamaHIP.slot_loop(kv="int8")``):
    the loop state also holds one image per slot index (``kvq``, ``qcap`` rows per plane) and their addresses (``kvq_base``);
    a sequence that enters has its arena rows quantised into its slot's image, and every step stages the row it appends.  The
    fp16 arenas stay complete, so ``close`` / ``retire`` and whatever reads an arena afterwards behave as ``SlotLoop``'s."""

    kv = "int8"


class _ImageSeat:
    """What a ``SlotLoopQ8Only`` keeps of the arena a sequence entered with: its rows at entry and the bound on its rows (the
    image's) -- no buffer.  ``close`` / ``retire`` set ``length`` here and touch no arena."""

    buf = None

    def __init__(self, length: int, cap: int):
        self.length, self.cap = int(length), int(cap)


class _ImageRows:
    """Images sized by the sequences, not by their arenas (in front of a ``_SlotLoopHost`` leaf with ``kv = "int8"``): ``qcap`` is
    the larger of ``max_keys`` and the longest ``length + max_new + k + 2`` known at build, and a sequence that is longer than the
    images raises when it enters."""

    def _image_rows(self, arenas, max_news, max_keys) -> int:
        return max([a.length + mn + self.k + 2 for a, mn in zip(arenas, max_news)] + [int(max_keys or 0)])

    def _quantise_entry(self, s: int, a) -> None:
        if a.length > self.qcap:
            raise RuntimeError(f"{type(self).__name__}: the sequence for slot {s} holds {a.length} rows, the loop's int8 images "
                               f"{self.qcap} (build the loop with max_keys >= the longest sequence)")
        m = self.m
        _native.kv_quant_q8_rows(a.buf, a.cap, a.length, m.L * 2 * m.Hkv, m.D, self.kvq[s], self.qcap)


class _ImageOnly(_ImageRows):
    """No fp16 slot arenas (``keep_arenas=False``): a slot's only K/V storage is its image and a fresh-row buffer,
    fp16 ``[L * 2 * Hkv][k + 1][D]``, holding the rows of the current step (``fresh``; ``st["kv_base"]`` holds these addresses).
    The cap word of a slot is ``qcap``, and the loop keeps an ``_ImageSeat`` in place of the arena a sequence entered with."""

    def _make_state(self, tokens, corpora, hist_cap) -> dict:
        st = super()._make_state(tokens, corpora, hist_cap)
        self.fresh = self.m._slot_fresh(st, self.S, self.k + 1)          # (allocated before any capture, like the images)
        return st

    def _prepared(self, a, max_new: int):
        """No arena is decoded in: nothing grows.  A residual tail still ends here, in front of the quantise launch."""
        self.m._tail_done(a, 0, 1, a.length)
        return a

    def _seat(self, s: int, a):
        return _ImageSeat(a.length, self.qcap), self.fresh[s].data_ptr(), self.qcap


class SlotLoopQ8Only(_ImageOnly, SlotLoopQ8):
    """``SlotLoopQ8`` without the fp16 slot arenas (``LlamaHIP.slot_loop(kv="int8", keep_arenas=False)``): a slot's
    only K/V storage is its int8 image and a fresh-row buffer, fp16 ``[L * 2 * Hkv][D]``, holding the row of the current step
    (``fresh``; ``st["kv_base"]`` holds these addresses).  The step runs ``pc_rope_append_slots_q8`` /
    ``pc_attn_decode_slots_q8_fresh``.  A sequence enters from whatever arena its prefill ran in: ``materialize()``, the tail
    ended, ``pc_kv_quant_q8_rows`` into the slot's image on the loop's stream in front of the arm launch -- after that the loop
    holds no reference to the arena, which may be staged again at once (same stream: the quantise launch is ordered in front).
    The cap word of a slot is ``qcap``: a sequence whose image is full ends by the device's "buffer full" rule.  ``qcap`` is the
    larger of ``max_keys`` and the longest ``length + max_new + 2`` known at build; split counts are ``SlotLoopQ8``'s, so on the
    same ``max_keys`` a sequence's tokens are that loop's, bit for bit."""

    def _graph(self):
        return self.m._slot_graph(self.S, self.nsplit, self.nsplit_trunk, self.each, self.qcap, fresh=True, logprobs=self.lp_n,
                                  ctl=self._cs)


class LookupSlotLoop(_SlotLoopHost):
    """Batched decode with prompt-lookup drafts: ``SlotLoop``'s slots x ``LookupLoop``'s ``k + 1`` rows.

    Every replay of the ONE captured step runs ``pc_lookup_draft_slots`` -> the layer stack over ``R = S * (k + 1)`` rows (row
    ``b * (k + 1) + i`` = draft row i of slot b) with ``pc_rope_append_slots_rows`` / ``pc_attn_verify_slots`` per slot ->
    ``pc_lookup_verify_slots``, which leaves one ``{count, tokens...}`` record per slot and advances the slot's words by what it
    accepted.  A slot stops on the device (stop id, budget) and leaves empty records afterwards.  Safe by construction, per slot,
    as ``LookupLoop`` is: every arena holds ``len0 + max_new + k + 2`` rows, ``budget`` keeps ``len`` at or below
    ``len0 + max_new``, a step writes rows ``[len, len + k]`` only.

    ``enqueue()`` -> step index; ``tokens(j, i)`` -> the 0..k+1 tokens of sequence j at step i (waits for that step only);
    ``kill(j)``; ``close(consumed)`` with the TOKENS each sequence's consumer used; ``logits`` is the ``[R][V]`` fp32 tensor of
    the last replay.  ``trunks`` (``lookup_slot_loop(share_trunk=True)``): ``SlotLoop``'s grouping -- the step then
    reads a group's shared rows from the leader's arena, once for all draft rows of all members
    (``pc_attn_verify_slots_trunk``); ``nsplit_trunk`` > 0 says so.

    ``prompt_rows`` (``LookupSlotLoopPrompt``, ``each=True`` only): the step runs the ``_prompt`` entries over one more word per slot,
    ``forced``, and ``admit_prompt`` feeds a request's question through the slot's ``k + 1`` rows -- ``ceil(q / (k + 1))`` replays
    with EMPTY records, the last of which draws the first token (``first_step`` says which replay that is)."""

    _arm_header = _native.LookupSlotArmBlock
    prompt_rows = False

    @torch.inference_mode()
    def __init__(self, model: "LlamaHIP", arenas, tokens, positions, max_new: int, k: int, corpora, nmax: int = 3, stop_ids=(),
                 slots: Optional[int] = None, max_keys: Optional[int] = None, trunks=None, each: bool = False, slot_index=None,
                 params=None, seeds=None, histories=None, hist_cap: Optional[int] = None):
        assert 1 <= k <= 15, k
        assert each or not self.prompt_rows, "prompt_rows needs each=True"
        self.k, self.nmax = int(k), int(nmax)
        self._record = (self.k + 2,)      # a step leaves {count, tokens...} per slot: ``host`` is [RING][S][k + 2]
        self._end = []                    # the replay at which the slot's next sequence entered (None: none has)
        self._prefill = []                # admit_prompt: (question length, replays its prefill takes) of sequence j; (0, 0): none
        self._gaps = {}                   # replay -> [(slot, position gap)]: added to pos[slot][0] behind that replay
        self._build(model, arenas, tokens, positions, max_new, params, seeds, histories, stop_ids, slots, slot_index, trunks, each,
                    max_keys, corpora, hist_cap)

    def _split_counts(self, lens, max_news, trunks, max_keys) -> None:
        """From ``max_keys`` (kept): the caller's bound of all keys of a sequence, or this batch's, rounded up to 64 -- in a loop
        with shared trunks and no bound from the caller, of a sequence's OWN keys behind its trunk (the trunk has a split count
        of its own)."""
        m, k = self.m, self.k
        shared = any(l is not None for l, _ in trunks)
        self.nsplit_trunk = 0
        if max_keys is None and self.each:
            max_keys = (max(l0 + mn for l0, mn in zip(lens, max_news)) + k + 1 + 63) // 64 * 64
        if max_keys is not None:
            self.max_keys = int(max_keys)
            if shared:
                self.nsplit_trunk = m._slot_nsplit(1, self.max_keys)
        elif shared:
            self.nsplit_trunk = m._slot_nsplit(len({l for l, _ in trunks if l is not None}), max(T for _, T in trunks))
            self.max_keys = (max(l0 - T for l0, (_, T) in zip(lens, trunks)) + max_news[0] + k + 1 + 63) // 64 * 64
        else:
            self.max_keys = (max(lens) + max_news[0] + k + 1 + 63) // 64 * 64
        self.nsplit = m._slot_nsplit(self.S, self.max_keys)

    def _make_state(self, tokens, corpora, hist_cap) -> dict:
        """``each``: ``hist_cap`` ids of draft history per slot (default 8192), fixed here: the captured step holds the buffer."""
        m, S, k = self.m, self.S, self.k
        if self.each:
            st = m._lookup_slot_state(S, k, 8192 if hist_cap is None else int(hist_cap), each=True, prompt=self.prompt_rows)
            self.hist_cap = st["hist"].shape[1]
            if self.prompt_rows:
                st["forced"].zero_()
        else:
            self._hists = [[int(t) for t in c] + [int(tok)] for c, tok in zip(corpora, tokens)]
            st = m._lookup_slot_state(S, k, max(map(len, self._hists)) + self.max_new)
        st["ndraft"].zero_()
        st["ctr"].zero_()
        return st

    def _graph(self):
        self.m._lo_mode = 0                # appended rows carry no residual planes, as in default decode
        return self.m._lookup_slot_graph(self)

    def _lp_tag(self):
        return ("slots", "lookup", self.S, self.k)

    def _fill_state(self, col, tokens, positions, max_new, params, seeds, histories, stop_ids) -> None:
        """The state words of the loop over ``pc_lookup_verify_slots``: greedy, one stop list for all slots."""
        st, S, hists = self.st, self.S, self.__dict__.pop("_hists")
        st["hist_len"].copy_(col(map(len, hists), torch.int32), non_blocking=True)
        ids = torch.zeros((S, self.k + 1), dtype=torch.int64)
        pos = torch.zeros((S, self.k + 1), dtype=torch.int32)
        hist = torch.zeros((S, max(map(len, hists))), dtype=torch.int32)
        for s, h, tok, p in zip(self.idx, hists, tokens, positions):
            ids[s], pos[s] = int(tok), int(p)
            hist[s, :len(h)] = torch.tensor(h, dtype=torch.int32)
        st["ids"].copy_(ids, non_blocking=True)
        st["pos"].copy_(pos, non_blocking=True)
        st["hist"][:, :hist.shape[1]].copy_(hist, non_blocking=True)
        stop = torch.full((S, 8), -1, dtype=torch.int32)
        stop[:, :len(stop_ids)] = torch.tensor([int(t) for t in stop_ids], dtype=torch.int32)
        st["stop"].copy_(stop, non_blocking=True)

    # ---- per-slot sampling state and admission (each=True) ---------------------------------------------------
    def _arm_setup(self, hw: int):
        st = self.st
        return _native.lookup_slot_arm_bytes(hw, self.hist_cap), _native.lookup_slot_state(
            st["kv_base"], st["cap"], st["len"], st["live"], st["leader"], st["trunk"], st["ids"], st["pos"], st["ndraft"], st["budget"],
            st["hist_len"], st["ctr"], st["draws"], st["seeds"], st["params_each"], st["stop"], st["bits"], st["hist"])

    @torch.inference_mode()
    def admit(self, slot_index: int, past, token: int, position: int, max_new: int, params, seed: int, history, stop_ids, corpus,
              trunk=None, controls=None) -> int:
        """A new sequence into slot ``slot_index`` of a running ``each=True`` loop, from the next replay on (``SlotLoop.admit``'s
        contract): the arena behind ``past`` feeds ``token`` at ``position`` and may emit ``max_new`` tokens, with its own ``params``
        (None / plain greedy: argmax), random stream ``seed`` (continuing at step 1), penalty ``history`` ids, up to 8
        ``stop_ids`` and the ``corpus`` its drafts may copy from (``lookup_admit_history``: the oldest ids go where the history
        buffer is too small).  ``trunk = (leader slot, T)``.  Only legal when the slot's previous sequence was retired.
        -> the new sequence's index."""
        return self._admit(int(slot_index), self._admit_arena(past), token, position, max_new, params, seed, history, stop_ids, trunk,
                           corpus, controls=controls)

    @torch.inference_mode()
    def admit_prompt(self, slot_index: int, past, ids, position0: int, max_new: int, params, seed: int, history, stop_ids, corpus,
                     trunk=None, decode_gap: int = 0) -> int:
        """``admit`` without the serial prefill (``prompt_rows=True`` loops): ``past`` holds the staged rows only, and the question
        ``ids`` -- at positions ``position0, position0 + 1, ...`` -- is fed through the slot's rows from the next replay on, k + 1
        tokens per replay; the replay that feeds the last one draws the sequence's first token on the device (step 0 of the
        stream ``seed``, under the bits of ``history``) and leaves it in the ring.  ``max_new`` counts that token.  The staging is
        carried out (``materialize()``), the arena gets ``T + q + max_new + k + 2`` rows and the WHOLE question stays in the draft
        history behind ``corpus``, the ids in front of it (``lookup_prompt_history``; ValueError where question and budget alone do
        not fit ``hist_cap``).  ``decode_gap``: added to the position of the first token once it is drawn (``GenerationEngine``
        places it one position behind the question's end + 1).  Question rows are appended as plain fp16 rows, as decoded rows
        are.  -> the new sequence's index; ``first_step`` gives the replay that carries its first token."""
        if not self.prompt_rows:
            raise RuntimeError("LookupSlotLoop.admit_prompt needs a loop built with prompt_rows=True")
        ids, s = [int(t) for t in ids], int(slot_index)
        if not ids:
            raise ValueError("LookupSlotLoop.admit_prompt: an empty question")
        if decode_gap and len(ids) % (self.k + 1) == 1:
            # (the forced rows run out at a step's end: an ordinary step feeds the last token and may draft behind it, gap or not)
            raise ValueError(f"LookupSlotLoop.admit_prompt: decode_gap needs a question that is not 1 mod k + 1 = {self.k + 1} tokens "
                             f"long, not {len(ids)}")
        j = self._admit(s, self._admit_arena(past), ids[0], position0, max_new, params, seed, history, stop_ids, trunk, corpus, ids)
        q, n = len(ids), -(-len(ids) // (self.k + 1))
        self.len0[j] += q                                # (the rows in front of the first decoded token, as behind a serial prefill)
        self._prefill[j] = (q, n)
        if decode_gap:
            self._gaps.setdefault(self._start[j] + n - 1, []).append((s, int(decode_gap)))
        return j

    def prefill_replays(self, j: int) -> int:
        """The replays sequence ``j``'s in-loop prefill takes, ``ceil(q / (k + 1))`` (0: it was prefilled before it entered)."""
        return self._prefill[j][1]

    def first_step(self, j: int) -> int:
        """The first replay whose record can carry a token of sequence ``j``: its start, or the last replay of its in-loop prefill.
        ``tokens(j, i)`` is empty for every earlier i because nothing has been drawn yet -- not because the sequence is over."""
        return self._start[j] + max(self._prefill[j][1] - 1, 0)

    @torch.inference_mode()
    def enqueue(self) -> int:
        i = super().enqueue()
        for s, gap in self._gaps.pop(i, ()):             # (stream-ordered behind replay i, which drew the slot's first token)
            self.st["pos"][s, :1] += gap
        return i

    def _length_after(self, j: int, consumed: int) -> int:
        """(a sequence that ends inside its in-loop prefill consumed nothing: its arena goes back to the staged rows)"""
        return self.len0[j] + consumed if consumed >= 0 else self.len0[j] - self._prefill[j][0]

    def _admit_check(self, s: int, corpus, token, max_new: int, question=None):
        hist = (lookup_admit_history(corpus, token, max_new, self.hist_cap) if question is None else
                lookup_prompt_history(corpus, question, max_new, self.hist_cap))
        prev = self._slot_seq[s]
        if prev is not None and prev not in self._retired:
            raise RuntimeError(f"LookupSlotLoop.admit: the sequence in slot {s} was not retired")
        return [j for j in self._slot_seq if j is not None and j not in self._retired], {"hist_len": len(hist)}, hist

    def _arm(self, block, arr, off: int, hist, question=None) -> None:
        """(the history ids behind the bitmap; the launch reads the bytes of THIS admission only)"""
        arr[off:off + 4 * len(hist)].view(np.int32)[:] = np.asarray(hist, dtype=np.int32)
        nbytes, s = off + ((4 * len(hist) + 7) & ~7), self._arm_header.from_buffer(arr).slot
        for gaps in self._gaps.values():                 # (a gap owed to the slot's previous sequence, killed inside its prefill)
            gaps[:] = [g for g in gaps if g[0] != s]
        if question is not None:
            _native.lookup_slot_arm_prompt(block, nbytes, self._arm_state, self.st["forced"], len(question) - 1, self.S, self.k,
                                           self.hist_cap)
            return
        if self.prompt_rows:                             # (forced rows a killed prefill left behind: this sequence has none)
            self.st["forced"][s: s + 1].fill_(0)
        _native.lookup_slot_arm(block, nbytes, self._arm_state, self.S, self.k, self.hist_cap)

    def _entered(self, j: int, prev, max_new: int, stop_ids) -> None:
        if prev is not None:
            self._end[prev] = self.n
        self._end.append(None)
        self._prefill.append((0, 0))

    def _set_length(self, a, length: int) -> None:
        a.length = length
        a.tail_base, a.tail_len = -1, 0

    def tokens(self, j: int, i: int):
        """The tokens sequence ``j`` emitted at step ``i`` (empty: the sequence was over, or had no budget left).  ``i`` is the global
        replay index -- empty before the sequence's start and from the replay its slot's next sequence entered (``each=True``),
        and before ``first_step(j)``, while an in-loop prefill has not drawn the first token yet."""
        if i < self._start[j] or (self._end[j] is not None and i >= self._end[j]):
            return []
        self.events[i][2].synchronize()
        rec = self.host[i % self.RING][self.idx[j]]
        c = int(rec[0])
        return [int(t) for t in rec[1:1 + c]]

    def logprobs(self, j: int, i: int) -> list:
        """One record per token of ``tokens(j, i)``, in its order: rows ``i < emit`` of the slot's k + 1 rows (a loop built with
        ``logprobs=n``)."""
        return self._lp.records(i % self.RING, self.idx[j] * (self.k + 1), len(self.tokens(j, i)))

    def kill(self, j: int) -> None:
        """``SlotLoop.kill``; nothing once the slot holds a later sequence."""
        if self._end[j] is None:
            super().kill(j)


class LookupSlotLoopPrompt(LookupSlotLoop):
    """``LookupSlotLoop(each=True)`` whose step takes forced rows (``lookup_slot_loop(prompt_rows=True)``): the state
    holds ``forced``, the captured step runs the ``_prompt`` entries and ``admit_prompt`` works."""

    prompt_rows = True


class LookupSlotLoopQ8(_ImageRows, LookupSlotLoop):
    """``LookupSlotLoop`` whose attention reads int8 images of the slots' K / V rows
    (``LlamaHIP.lookup_slot_loop(kv="int8")``): ``SlotLoopQ8``'s images, held by the (S, k) state.  Every step writes
    its ``k + 1`` rows per slot into arena AND image (``pc_rope_append_slots_rows_q8``) and draft row i attends to image keys
    ``[0, len + i)`` and to its own key exactly (``pc_attn_verify_slots_q8``) -- the function of the token sequence that
    ``SlotLoopQ8`` computes one token at a time, wherever the step boundaries fall.  The fp16 arenas stay complete.  A sequence
    that could outgrow the images (``length + max_new + k + 2 > qcap``) raises when it enters."""

    kv = "int8"

    def _prepared(self, a, max_new: int):
        a = super()._prepared(a, max_new)
        qcap = getattr(self, "qcap", None)           # (None while the loop is built: the images are sized from these sequences)
        if qcap is not None and a.length + max_new + self.k + 2 > qcap:
            raise RuntimeError(f"{type(self).__name__}: a sequence of {a.length} rows with max_new = {max_new} needs "
                               f"{a.length + max_new + self.k + 2} image rows, the loop's int8 images hold {qcap} (build the loop "
                               "with a larger max_keys)")
        return a


class LookupSlotLoopQ8Only(_ImageOnly, LookupSlotLoopQ8):
    """``LookupSlotLoopQ8`` without the fp16 slot arenas (``lookup_slot_loop(kv="int8", keep_arenas=False)``): ``SlotLoopQ8Only``'s
    residency under the lookup step.  The fresh-row buffers hold the step's ``k + 1`` rows per plane, the cap word of a slot is
    ``qcap`` and ``kv_base`` holds the fresh addresses, so the draft / arm / verify launches are ``LookupSlotLoop``'s; a sequence
    whose image is full ends by the device's "no room for a step" rule."""


# weight_format="mxfp4": most rows of a step that streams the 4-bit images (PC_W4_MAX_ROWS, clamped to 16..64).  64: at 17, 32, 48
# and 64 rows the 4-bit images beat the fp16 images of W' by more than the latter's own spread
W4_MAX_ROWS_DEFAULT = "64"


class LlamaHIP:
    """Weights live on one MI355X in fp16; ``wqkv`` and ``wgu`` are the row-concatenated q|k|v and
    gate|up projections so each is one GEMM."""

    SKINNY_MAX_ROWS = 64   # B*q_len at or below this: split-precision weight-streaming kernels inside one hipGraph
    # ... and at or below this the RMSNorms are folded into the projections.  The kernels take two row tiles as well
    # (PC_NORM_FUSED_MAX=32), but at 17..32 rows the six-launch loop measured SLOWER than slabs + pc_rmsnorm_frag (7b, 24 rows:
    # 110 vs 107 us of projections per layer -- o_proj / down_proj lose their K slices; profiles/r04_variants.txt)
    NORM_FUSED_MAX_ROWS = int(os.environ.get("PC_NORM_FUSED_MAX", "16"))
    # ... and up to here: the row-split weight-streaming kernel (gemm_rows_kernel, pc_gemm.hip), launched eagerly; above,
    # pc_gemm_dense.  Crossover against pc_gemm_dense_ws (tools/dense_vs_rows.py, profiles/r02_dense_splitk.txt, 7b layer,
    # split-precision planes on both sides): 259 rows 322 vs 402 us per layer, 512 rows 455 vs 441 us -- the streaming
    # kernel holds up to its own limit of 512 rows (round 1's 256 was measured against the vendor GEMM this tree no
    # longer carries)
    MID_MAX_ROWS = int(os.environ.get("PC_MID_MAX_ROWS", "512"))

    def _setup(self, shape, device, decode_headroom: int) -> None:
        """State every architecture shares: device, KV-arena headroom, workspace and the hipGraph cache."""
        _native.load()  # fail loudly if the extension is missing
        self.config = shape
        self.device = torch.device(device)
        self.dtype = torch.float16
        self.decode_headroom = decode_headroom
        self._ws = None
        # hipGraph cache for the small-q (prefill over staged KV / decode) forward: one captured graph per
        # (B, q_len, arena, split count); past_len, token ids and positions are read from device buffers so
        # every decode step and every same-shaped prompt replays the same graph.
        self.use_graphs = True
        self._graphs = {}
        self.max_graphs = 256   # one per (q_len, split count, mode): a serving mix of prompt lengths stays resident
        self.kslices = 4        # K-slices of the o_proj / down_proj launches (see _forward_skinny)
        # pc_gemm_chain (one persistent launch for o_proj -> gate|up -> down -> next q|k|v): correct and bit-identical, but
        # measured SLOWER than the four launches on MI355X (106-121 vs 88 us per layer, profiles/r02_chain_trace.txt): opt-in
        self.use_chain = os.environ.get("PC_CHAIN", "0") == "1" and _native.has("pc_gemm_chain")      # (dev builds only: csrc/pc_dev.h)
        self._chain_sync = None
        # split-precision activations in the many-row path (see _forward_dense_split); PC_FAST_DENSE=1 trades the
        # full-depth parity for 2x fewer GEMM flops
        self.precise_dense = os.environ.get("PC_FAST_DENSE", "0") != "1"
        # Many-row projections that run on the hi activation plane only (a tile pass of 1 plane instead of 2: half the MFMAs of that
        # launch).  Measured at full depth against the numpy oracle (tests/test_gpu_fullsize.py, 32 layers at the 7b shape; plain
        # init / six 60x outlier channels), max |dlogit| by which projection drops its lo plane: none 1.1e-3 / 7.0e-4, gate|up
        # 3.4e-3 / 3.1e-3, down 2.7e-3 / 2.4e-3, o 2.9e-3 / 2.8e-3, gate|up + down 4.4e-3 / 3.9e-3, q|k|v 1.5e-2 / 7.5e-3 (FAILS:
        # its outputs are the stored K / V and the attention's Q).  gate|up is 45 % of a layer's projection MACs: default.
        # PC_DENSE_LO_SKIP= (empty): every projection on both planes, as in rounds 1-3.
        # Depth matters (the error grows with every layer): the 40-layer 13b stack measured 7.2e-3 with gate|up on one plane against
        # 1.7e-3 on two -- inside the bar, but with little room -- so the default applies up to 32 layers; deeper stacks keep both
        # planes everywhere unless PC_DENSE_LO_SKIP says otherwise.
        _skip = os.environ.get("PC_DENSE_LO_SKIP")
        if _skip is None:
            _skip = "gu" if getattr(shape, "num_hidden_layers", 99) <= 32 else ""
        self.dense_lo_skip = tuple(t for t in _skip.split(",") if t)
        self.mid_lo_skip = tuple(t for t in os.environ.get("PC_MID_LO_SKIP", "").split(",") if t)
        self.fused_dense_qkv = os.environ.get("PC_FUSED_DENSE_QKV", "1") != "0"   # RoPE + KV append in the many-row q|k|v epilogue
        # Round 5: the many-row projections that keep their residual activation plane run it on the INT8 MFMA (pc_gemm_dense_lo8:
        # x_lo as row-wise absmax int8 codes against an int8 image of the weights, exact int32 sums at twice the fp16 MFMA rate:
        # 24 matrix-pipe slots per K-step instead of 32).  The residual only has to be good to a few bits -- it is 2^-11 of the
        # activation -- and is carried to 2^-8 of its row maximum.  MEASURED (profiles/r05_variants.txt): the launches are 3-8 %
        # faster than with the fp16 residual plane (not the 25 % the slot count promises: at ~1.15 PFLOP/s executed the kernel sits at
        # ~75 % of the matrix peak at the clock the chip holds under this load), the persona encode 101.9 -> 104.2 k tok/s, full-depth
        # parity unchanged at 7b (5.1e-3) and 3.3e-3 instead of 2.0e-3 at 13b -- for 6.7 GB of int8 weight images at 7b.  Not worth a
        # second weight image by default: OPT-IN (PC_DENSE_LO8=1).
        self.dense_lo8 = os.environ.get("PC_DENSE_LO8", "0") == "1" and _native.has("pc_gemm_dense_lo8")      # (dev builds only: csrc/pc_dev.h)
        self.encode_mid = os.environ.get("PC_ENC_MID", "1") != "0"    # encode passes of 65..512 rows on the row-split stack
        # keep the fp16 residuals of the K / V rows appended behind a staged cache -- the prompt's own tokens and every
        # decoded token -- in the arena's residual tail and feed them to the attention (the reference keeps those rows in
        # fp32 for the whole generation, llama2.py:361-388, generation_engine.py:123-147; the arena still holds the fp16
        # values).  See _tail_mode / _dense_pass_lo.
        self.new_kv_lo = os.environ.get("PC_NEW_KV_LO", "1") != "0"
        # ... and keep doing so through the DECODE steps of a generation (every decoded row gets a residual, every step's
        # attention reads residual tiles): decode logits 5e-5 from the oracle instead of 2-4e-3 -- both far inside the
        # 1e-2 bar -- for ~5 % of the decode rate.  Opt-in (PC_DECODE_TAIL=1 or model.decode_tail = True).
        self.decode_tail = os.environ.get("PC_DECODE_TAIL", "0") == "1"
        self.defer_merge = os.environ.get("PC_DEFER_MERGE", "1") != "0"    # one-row steps: o_proj merges the attention's partials
        # arrival counters of the single-launch split-KV merge (pc_attn `counters`: zero now, every launch leaves them zero).
        # Opt-in (PC_ATTN_FUSED=1): measured on MI355X the in-launch hand-off (write-through partials, drain, arrival counter,
        # the last arriver's read-back: ~4.5 us on the critical path) costs what the second launch costs -- persona step 3.922 /
        # 3.933 ms fused against 3.907 / 3.908 ms with attn_combine_kernel (gpurun_out/r3b)
        self._attn_counters = torch.zeros(8192, dtype=torch.int32, device=self.device) \
            if os.environ.get("PC_ATTN_FUSED", "0") == "1" else None
        # N = hidden projections of the <= 16-row stack with K split across workgroups and the reduction inside the launch
        # (pc_gemm_skinny_ks): "tiles,slices" per projection, empty = the one-tile-per-workgroup EPI_ADD launch
        def _ks(env, default):
            v = os.environ.get(env, default)
            return tuple(int(t) for t in v.split(",")) if v else None
        # Measured at 12 rows (tools/ks_micro.py, in-graph): down_proj (K = 11008) 22.75 -> 20.16 us at 2 tiles x 2 slices, every
        # other shape of either projection loses to the one-tile launch (o_proj 9.4 -> 10.4 .. 13.5 us; one row: 19.0 -> 20.3 us):
        # the in-launch reduction costs ~3 us, only the long-K launch with its 2:1 activation traffic earns it back.
        self.ks_o, self.ks_down = _ks("PC_KS_O", ""), _ks("PC_KS_DOWN", "2,2")
        self.ks_min_rows = 5       # ... and only with more than 4 rows (decode keeps the one-tile launch)
        self._ks_state = None      # (scratch, counters), lazily
        self._kv_only = False      # set per call (see __call__)
        self._past_lens = None     # set per call: per-row past lengths of a ragged-prefix encode batch
        self.supports_ragged_past = True    # the many-row path takes past_lens (see __call__)
        self._shared = None        # set per call: (trunk arena, per-row prefix lengths int32 [B], their maximum)
        self.supports_greedy_loop = True    # decode steps can run as a device-side loop (GreedyLoop)
        self._live_loop = None              # the device loop that owns the loop state words right now (one per model)
        self.llm_int8 = False
        self.weight_format, self.w4, self.w4_stream = "fp16", False, False    # MXFP4 decoder weights (LlamaHIP.__init__)
        self.w4_max_rows = 16
        self.keep_fp16, self._w16_scratch = True, None                       # MXFP4 without fp16 images (LlamaHIP.__init__, _w16)
        self._last_qt = None
        self.batch_invariant = True         # a row's result does not depend on the other rows of the forward (see llm_int8)
        self.tail_supported = True  # a subclass whose layer loops do not thread `_tail_for` through must switch this off
        self._gather = None         # set per forward: the row table while the attention launches stage as they read
        self._pre = None            # set per captured forward: (fp32 residual stream, rotation table) from pc_prefill_prologue
        self.fused_prologue = os.environ.get("PC_FUSED_PROLOGUE", "1") != "0"
        self.stats = {"fused_gather": 0}     # forwards that carried out a pending staging inside their attention launches
        self._gather_ok_cache, self._nsplit_cache = {}, {}
        # hipGraphs for the 65..512-row forward as well (B = 1, 16-row buckets): nine launches per layer from Python are host-bound
        # at 7b and ~100 rows (PC_GRAPH_MID=0: launched eagerly, as in rounds 1-3)
        self.graph_mid = os.environ.get("PC_GRAPH_MID", "1") != "0"
        self.max_mid_graphs = 8

    # the many-row layer loop of THIS class hands the attention a shared key prefix (__call__'s ``shared_prefix``); a subclass
    # with its own loop says so itself
    _shared_prefix_loop = True
    # The <= 16-row cached prefill of THIS class's layer loops can carry out a pending staging (KVArena.pending) inside its
    # attention launches (pc_attn gather_rows): CacheEngine then defers PromptCache.update's copy to the first lm() call.
    supports_fused_gather = True
    GATHER_MAX_SEG = 512            # segments of a staging plan the captured forward has room for (longer plans: pc_kv_gather)

    @property
    def supports_shared_prefix(self) -> bool:
        return bool(self._shared_prefix_loop and self.precise_dense and not self.llm_int8)

    def __init__(self, shape: LlamaShape, weights: Dict[str, torch.Tensor], device="cuda:0",
                 decode_headroom: int = 256, skinny: bool = True, int8_weights: bool = False, weight_format: str = "fp16",
                 keep_fp16: Optional[bool] = None):
        """``int8_weights`` (the adapters' ``load_in_8bit=True``): the decoder-layer linears are quantised row-wise to
        int8 (``_native.quantize_rows_int8``); passes of <= 64 rows stream the int8 fragment images (half the bytes, exact
        arithmetic on the dequantised values); longer passes run hipBLASLt on the int8 codes held in fp16 (exact) and
        scale the product per output feature (``_proj``).

        ``weight_format="mxfp4"``: every decoder-layer linear is quantised at load to MXFP4 (``_native.quantize_mxfp4``) and the
        model IS the fp16 model with the dequantised weights ``W'`` (exact in fp16): the layer keeps the fp16 images of ``W'``
        for every path above 16 rows and, next to them, the two 4-bit images the <= 16-row projections stream (``pc_gemm_w4``:
        the cached step, decode, the device loops).  ``PC_W4_MAX_ROWS`` (16..64) extends the images to the steps of 17 rows up
        to it (``pc_gemm_w4_rows``: a cached step with a longer question, the slot-lookup verify step).  ``PC_W4_STREAM=0`` runs
        the fp16 images of ``W'`` everywhere.

        ``keep_fp16=False`` (``None``: ``PC_W4_KEEP_FP16=0``; MXFP4 only): the layers keep the two 4-bit images and NO fp16 image of
        ``W'``.  Steps of at most ``PC_W4_MAX_ROWS`` rows never needed one; every other projection launch is preceded by a
        ``pc_w4_expand`` of its weight into the model's one scratch buffer (``_w16``) -- exact, so every forward is bit-identical
        to the ``keep_fp16=True`` model's.  The embeddings, the norms and both lm_head images stay fp16."""
        check_weight_format(weight_format, int8_weights, shape)     # (before anything is allocated)
        keep_fp16 = check_keep_fp16(keep_fp16, weight_format)
        self._setup(shape, device, decode_headroom)
        c = shape
        self.H, self.Hkv, self.D, self.L = c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.num_hidden_layers
        dev = self.device

        def w(name):
            t = weights[name]
            if not isinstance(t, torch.Tensor):
                t = torch.from_numpy(t)
            return t.to(device=dev, dtype=self.dtype).contiguous()

        self.embed = w("embed")
        self.norm = w("norm")
        self.lm_head = w("lm_head")
        # Two resident images of every projection (288 GB of HBM: 2 x 13.5 GB for 7b is cheap):
        # row-major [N][K] for the dense (large q: encode / no-cache) GEMMs, and the MFMA-fragment-major
        # image the weight-streaming kernels read as one sequential stream per wave (small q: cached
        # prefill, decode).  Shapes that do not tile (N%16, K%32) simply keep the dense path.
        self.skinny = bool(skinny) and c.hidden_size % 32 == 0 and c.intermediate_size % 32 == 0 and \
            c.vocab_size % 16 == 0 and (self.H * self.D) % 32 == 0
        fr = _native.to_weight_frags if self.skinny else (lambda t: None)
        self.lm_head_f = fr(self.lm_head)
        self.layers = []
        # (the int8 images are cut on pairs of 32-feature k-steps: every GEMM K must be a multiple of 64)
        self.int8_weights = bool(int8_weights) and self.skinny and c.hidden_size % 64 == 0 and \
            c.intermediate_size % 64 == 0 and (self.H * self.D) % 64 == 0
        # load_in_8bit on the Llama family = LLM.int8() as published (int8 weights AND vector-wise int8 activations with the
        # fp16 outlier decomposition, threshold 6.0: what the reference's GPU runs execute through bitsandbytes;
        # csrc/pc_int8.hip, oracle/llmint8_oracle.py).  PC_INT8_WEIGHT_ONLY=1 keeps round 1's weight-only mode instead
        # (split-precision fp16 activations over the int8 weights) -- the mode the Falcon / MPT adapters still run.
        self.llm_int8 = self.int8_weights and os.environ.get("PC_INT8_WEIGHT_ONLY", "0") != "1"
        if self.int8_weights:
            self.MID_MAX_ROWS = self.SKINNY_MAX_ROWS      # the row-split kernel has no int8 variant: 65+ rows go dense
        if self.llm_int8:
            kmax = max(c.hidden_size, c.intermediate_size, self.H * self.D)
            # outlier-column flags, one row per activation slot; 16384 bytes each: the in-launch correction (pc_gemm_*_a8c)
            # scans a whole row, 32 bytes per thread
            self._i8_flags = torch.zeros((4, max(kmax, 16384)), dtype=torch.uint8, device=dev)
            self.i8_fused_corr = os.environ.get("PC_INT8_FUSED_CORR", "1") != "0"
            # <= 16 rows (the cached step, decode): the activation quantisers run INSIDE the projections (pc_gemm_q8): six launches
            # per layer instead of ten.  PC_INT8_INLAUNCH=0: round 4's separate quantiser launches.  PC_Q8_DOWN="tiles,slices" of the
            # K-sliced down_proj (2 / 4 / 8 output tiles per workgroup, 1..8 slices)
            self.i8_inlaunch = os.environ.get("PC_INT8_INLAUNCH", "1") != "0" and c.hidden_size <= 6144 and \
                self.H * self.D <= 6144 and c.intermediate_size <= 16384
            self.q8_down = tuple(int(v) for v in os.environ.get("PC_Q8_DOWN", "4,4").split(","))
            self.q8_down_small = tuple(int(v) for v in os.environ.get("PC_Q8_DOWN_SMALL", "1,1").split(","))   # <= 4 rows (decode)
            self.q8_p_max_rows = int(os.environ.get("PC_Q8_P_MAX_ROWS", "4"))
            self.q8_defer_merge = os.environ.get("PC_Q8_DEFER_MERGE", "1") != "0"
            self.q8_image = os.environ.get("PC_Q8_IMAGE", "1") != "0"    # 5..16 rows: pc_gemm_q8 on the quantiser launches' images
            self._q8_flags = torch.zeros(16384, dtype=torch.uint8, device=dev)
            self._q8_pmax = torch.zeros((c.intermediate_size // 16, 16), dtype=torch.float32, device=dev)
            self._i8_zero = torch.zeros(((self.SKINNY_MAX_ROWS + 15) // 16) * 16 * kmax, dtype=self.dtype, device=dev)
            self.fuse_norm = False                        # activations are quantised between the norm and the projection
            self.batch_invariant = False                  # the fp16 outlier columns are chosen over ALL rows of a call

        prep = self._prep_linear
        self.weight_format = weight_format
        self.w4 = weight_format == "mxfp4"
        # the <= 16-row projections on the 4-bit images.  They leave q|k|v as a plain fp32 store for pc_rope_append_ex (natural
        # row order), which writes the residual tail as the fused epilogue does.  The forms that need fp16 fragment images
        # inside their launch (pc_gemm_part, the in-launch K reduction, pc_gemm_chain) are off.
        self.w4_stream = self.w4 and self.skinny and os.environ.get("PC_W4_STREAM", "1") != "0"
        # ... and the 17..w4_max_rows-row steps (the generic loop of _forward_skinny, the 17..64-row branch of the slot-lookup step)
        # on the same images (pc_gemm_w4_rows); 16 = those steps stay on the fp16 images of W' (DESIGN 3.25 has the measurements)
        self.w4_max_rows = min(max(int(os.environ.get("PC_W4_MAX_ROWS", W4_MAX_ROWS_DEFAULT)), 16), self.SKINNY_MAX_ROWS)
        if self.w4_stream:
            self.use_chain = False
            self.defer_merge = False
            self.ks_o = self.ks_down = None
        self.keep_fp16 = keep_fp16
        if not keep_fp16:
            if not self.w4_stream:
                raise ValueError("keep_fp16=False needs the 4-bit images, which this shape does not tile (hidden, intermediate "
                                 "% 32, vocab % 16): there would be nothing left to expand")
            # ONE scratch for the expanded image of whichever projection runs next, sized for the largest (gate|up).  Allocated
            # here, before any capture, and never resized: the captured 65..512-row graphs keep its address.  One buffer is
            # enough because every forward of this class issues its launches on one stream, in order: a projection has read
            # the scratch before the next expand overwrites it.
            self._w16_scratch = torch.empty(max(2 * c.intermediate_size * c.hidden_size, (self.H + 2 * self.Hkv) * self.D * c.hidden_size,
                                                c.hidden_size * self.H * self.D), dtype=self.dtype, device=dev)

        for i in range(self.L):
            wqkv = torch.cat([w(f"l{i}.wq"), w(f"l{i}.wk"), w(f"l{i}.wv")], dim=0).contiguous()
            wgu = torch.cat([w(f"l{i}.gate"), w(f"l{i}.up")], dim=0).contiguous()
            wo, wdown = w(f"l{i}.wo"), w(f"l{i}.down")
            w4 = {}
            if self.w4:
                # W -> W' = dequant(quant(W)); the 4-bit images are in natural row order (q|k|v included)
                def mx(wt, key):
                    q = _native.quantize_mxfp4(wt)
                    if self.w4_stream:
                        w4[key + "_c4"], w4[key + "_e4"] = _native.to_weight_frags_w4(*q)
                    return _native.dequantize_mxfp4(*q)
                wqkv, wo, wgu, wdown = mx(wqkv, "wqkv"), mx(wo, "wo"), mx(wgu, "wgu"), mx(wdown, "wdown")
            if self.skinny and i == 0:
                self._qkv_perm = _native.qkv_rope_row_perm(self.H + 2 * self.Hkv, self.D).to(dev)
            if not keep_fp16:
                # W' goes: the layer is its norms and the 4-bit images (every wX / wX_f / scale entry None)
                del wqkv, wo, wgu, wdown
                self.layers.append(dict(ln1=w(f"l{i}.ln1"), ln2=w(f"l{i}.ln2"), **w4,
                                        **{key + sfx: None for key in ("wqkv", "wo", "wgu", "wdown")
                                           for sfx in ("", "_f", "_s", "_ds", "_t8")}))
                continue
            # q|k|v fragment image: rotary pairs share a 16-row tile (pc_gemm_qkv_rope)
            wqkv, wqkv_f, wqkv_s = prep(wqkv, self._qkv_perm if self.skinny else None); t_qkv = self._last_qt
            wo, wo_f, wo_s = prep(wo); t_o = self._last_qt
            wgu, wgu_f, wgu_s = prep(wgu); t_gu = self._last_qt
            wdown, wdown_f, wdown_s = prep(wdown); t_d = self._last_qt
            q8 = {}
            if self.dense_lo8 and self.precise_dense and not self.int8_weights:
                # int8 images (+ row scales) of the projections whose many-row launches keep the residual plane (dense_lo_skip)
                for key, wt, tag in (("wqkv", wqkv, "qkv"), ("wo", wo, "o"), ("wgu", wgu, "gu"), ("wdown", wdown, "down")):
                    if tag not in self.dense_lo_skip and wt.shape[1] % 64 == 0:
                        q8[key + "_q8"], q8[key + "_q8s"] = _native.quantize_rows_int8(wt)
            self.layers.append(dict(ln1=w(f"l{i}.ln1"), ln2=w(f"l{i}.ln2"), wqkv=wqkv, wo=wo, wgu=wgu, wdown=wdown, **q8, **w4,
                                    wqkv_t8=t_qkv, wo_t8=t_o, wgu_t8=t_gu, wdown_t8=t_d,
                                    wqkv_f=wqkv_f, wo_f=wo_f, wgu_f=wgu_f, wdown_f=wdown_f,
                                    wqkv_s=wqkv_s[0], wo_s=wo_s[0], wgu_s=wgu_s[0], wdown_s=wdown_s[0],
                                    wqkv_ds=wqkv_s[1], wo_ds=wo_s[1], wgu_ds=wgu_s[1], wdown_ds=wdown_s[1]))
        # exactly the reference formula, evaluated on the CPU like the reference does (llama2.py:121)
        self.inv_freq_cpu = 1.0 / (c.rope_theta ** (torch.arange(0, self.D, 2).float() / self.D))
        self.inv_freq = self.inv_freq_cpu.to(dev)
        self.softmax_scale = 1.0 / math.sqrt(self.D)
        self.fuse_norm = os.environ.get("PC_FUSE_NORM", "1") != "0" and not getattr(self, "llm_int8", False)
        if self.skinny:
            self._qkv_perm_i32 = self._qkv_perm.to(torch.int32).contiguous()

    # ------------------------------------------------------------------------------------------
    def dequantized_weights(self) -> Dict[str, torch.Tensor]:
        """name -> fp16 tensor of the weights this model computes with, under the names of the constructor's ``weights``: with
        ``weight_format="mxfp4"`` the decoder linears are ``W' = dequant(quant(W))`` -- what an oracle of this model loads
        (``keep_fp16=False``: rebuilt here from the 4-bit images)."""
        if self.int8_weights:
            raise ValueError("dequantized_weights: not kept in int8 mode")
        HD, KD, inter = self.H * self.D, self.Hkv * self.D, self.config.intermediate_size
        out = {"embed": self.embed, "norm": self.norm, "lm_head": self.lm_head}
        for i, lw in enumerate(self.layers):
            if not self.keep_fp16:
                lw = dict(lw, **{key: _native.dequantize_mxfp4(*_native.from_weight_frags_w4(lw[key + "_c4"], lw[key + "_e4"]))
                                 for key in ("wqkv", "wo", "wgu", "wdown")})
            out.update({f"l{i}.ln1": lw["ln1"], f"l{i}.ln2": lw["ln2"], f"l{i}.wq": lw["wqkv"][:HD],
                        f"l{i}.wk": lw["wqkv"][HD:HD + KD], f"l{i}.wv": lw["wqkv"][HD + KD:], f"l{i}.wo": lw["wo"],
                        f"l{i}.gate": lw["wgu"][:inter], f"l{i}.up": lw["wgu"][inter:], f"l{i}.down": lw["wdown"]})
        return out

    def resident_tensors(self):
        """The tensors this model holds, one per distinct storage: the attributes and every layer entry (weights and images, the
        expand scratch, state words and whatever workspace a forward has left; not the captured graphs' private pools)."""
        seen, out = set(), []
        for t in list(vars(self).values()) + [v for lw in self.layers for v in lw.values()]:
            if isinstance(t, torch.Tensor) and t.device.type == self.device.type and t.untyped_storage().data_ptr() not in seen:
                seen.add(t.untyped_storage().data_ptr())
                out.append(t)
        return out

    def resident_bytes(self) -> int:
        return sum(t.untyped_storage().nbytes() for t in self.resident_tensors())

    def new_arena(self, batch: int, cap: int) -> KVArena:
        return KVArena(batch, self.L, self.Hkv, cap, self.D, self.device, self.dtype)

    def _prep_linear(self, wt: torch.Tensor, perm=None):
        """One projection -> (row-major image for the many-row GEMMs, fragment image for the streaming kernels,
        (fragment-order scales, row-order scales) | (None, None)).  int8 mode: both images hold the int8 codes."""
        fr = _native.to_weight_frags if self.skinny else (lambda t: None)
        if not self.int8_weights:
            src = wt if perm is None else wt[perm].contiguous()
            return wt, fr(src), (None, None)
        q, sc = _native.quantize_rows_int8(wt)
        dense = q.to(self.dtype)                      # the int8 codes, exact in fp16; _proj applies the scales (many-row paths)
        dsc = sc
        self._last_qt = q.t().contiguous() if getattr(self, "llm_int8", False) else None   # [K][N] int8: columns for pc_outlier_corr
        if perm is not None:
            q, sc = q[perm].contiguous(), sc[perm].contiguous()
        return dense, _native.to_weight_frags_i8(q), (sc, dsc)

    def _linear_entries(self, name: str, prepped) -> dict:
        dense, frag, (sc, dsc) = prepped
        return {name: dense, name + "_f": frag, name + "_s": sc, name + "_ds": dsc, name + "_t8": getattr(self, "_last_qt", None)}

    TAIL_HEADROOM = 256     # decoded rows a generation's residual tail has room for past the prompt's own

    def _tail_mode(self, arena: KVArena, q_len: int, past_len: int) -> int:
        """How the weight-streaming paths treat the fp16 residuals of the rows they append (``KVArena.tail_lo``):
        1 = a prefill pass starts a new tail at ``past_len`` (rows [0, q_len)); 2 = a decode step continues the tail the
        prefill started, so every row since the staged cache ended -- prompt tokens and decoded tokens alike -- reaches
        the attention in split precision, as in the reference's fp32 generation (generation_engine.py:123-147);
        0 = no residuals (switched off, a tail that does not cover the rows since its base, or no room left)."""
        if not self.new_kv_lo or not self.tail_supported:
            return 0
        if q_len > 1:
            arena.ensure_tail(q_len + self.TAIL_HEADROOM)
            return 1
        t = arena.tail_lo
        if not self.decode_tail:
            return 0
        # (a caller may rewind the arena by a few rows: the tail then still covers [tail_base, past_len))
        if t is not None and 0 <= arena.tail_base <= past_len <= arena.tail_base + arena.tail_len and \
                past_len - arena.tail_base + 1 <= t.shape[4]:
            return 2
        return 0

    def _dense_pass_lo(self, arena: KVArena, B: int, Hkv: int, q_len: int, past_len: int):
        """Residual planes for the K / V rows a many-row pass appends: ``layer -> (k_lo, v_lo, bs, hs, row0)``.
        An encode arena (``arena.lo``) keeps residuals for all of its rows; a prefill in front of a generation writes them
        into the arena's residual tail so the decode steps after it find them (``_tail_mode``); a batch-padded or kv-only
        pass gets a scratch buffer shared by the layers (each layer's attention consumes it before the next overwrites it)."""
        if arena.lo is not None and arena.lo_len == past_len:
            return (lambda li: arena.lo_planes(li)), True
        if self.new_kv_lo and self.tail_supported and not self._kv_only:
            arena.ensure_tail(q_len + self.TAIL_HEADROOM)
            self._lo_mode = 1
            return (lambda li: arena.tail_planes(li) + (past_len,)), False
        lo = torch.empty((2, B, Hkv, q_len, self.D), dtype=self.dtype, device=self.device)
        scratch = (lo[0], lo[1], Hkv * q_len * self.D, q_len * self.D, past_len)
        return (lambda li: scratch), False

    @staticmethod
    def _tail_done(arena: KVArena, mode: int, q_len: int, past_len: int) -> None:
        if mode == 1:
            arena.tail_base, arena.tail_len = past_len, q_len
        elif mode == 2:
            arena.tail_len = past_len + q_len - arena.tail_base
        else:
            arena.tail_base, arena.tail_len = -1, 0          # rows appended without residuals: the tail no longer covers

    def _workspace(self, nbytes: int) -> Optional[torch.Tensor]:
        if nbytes <= 0:
            return None
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        return self._ws

    def _resolve_arena(self, past, B: int, q_len: int, keep_pending: bool = False):
        """-> (arena, past_len) with room for q_len more rows.  A staging the arena still owes (``KVArena.pending``) is carried
        out here unless the caller takes care of it itself (``keep_pending``)."""
        if past is None:
            return self.new_arena(B, q_len + self.decode_headroom), 0
        found = arena_from_past(past, self.L, self.Hkv, self.D)
        if found is not None and not keep_pending:
            found[0].materialize()
        if found is None:
            # foreign tensors (e.g. a caller-built legacy cache): copy once into an arena
            k0 = past[0][0]
            S = k0.shape[-2]
            arena = self.new_arena(B, S + q_len + self.decode_headroom)
            for i in range(self.L):
                k, v = past[i][0], past[i][1]
                if k.dim() == 3:
                    k, v = k.unsqueeze(0), v.unsqueeze(0)
                arena.buf[:, i, 0, :, :S].copy_(k)
                arena.buf[:, i, 1, :, :S].copy_(v)
            arena.length = S
            return arena, S
        arena, S = found
        if arena.B != B:
            raise ValueError(f"past_key_values batch {arena.B} != input batch {B}")
        if S + q_len > arena.cap:
            arena.length = S
            arena = arena.grown(max(S + q_len + self.decode_headroom, 2 * arena.cap))
        return arena, S

    # ------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def __call__(self, input_ids: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
                 past_key_values=None, attention_mask: Optional[torch.Tensor] = None, use_cache: bool = True,
                 last_token_only: bool = False, num_layers: Optional[int] = None, many_rows: bool = False,
                 kv_only: bool = False, past_lens: Optional[torch.Tensor] = None, shared_prefix=None,
                 **_unused) -> CausalLMOutput:
        """``shared_prefix = (trunk arena, [n_pre per batch row])`` (schema encode, split-precision many-row path): batch row b
        attends to rows [0, n_pre[b]) of the trunk arena IN PLACE and then to its own rows, which go into a fresh arena from
        row 0 on -- the suffix passes of an encode without a copy of the trunk per batch row.
        ``past_lens`` (int32 [B], many-row path over an encode arena): one past length per batch row -- row b appends
        behind its own ``past_lens[b]`` rows and attends to those plus its new rows (scaffold suffixes of different
        unions batched over their trunk prefixes); the arena's ``length`` must be their maximum.
        ``kv_only`` (many-row path): stop after the last layer's K / V are in the arena and return no logits -- all a
        schema-encode pass is run for (the reference discards the rest, cache_engine.py:243-296).
        ``many_rows``: take the stacked-GEMM path for more than 64 rows even where the row-split kernel would be
        faster -- it alone keeps the pass's own K/V in split precision, which is what a schema encode wants (its K/V
        are the product)."""
        n = _native
        dev = self.device
        B, q_len = input_ids.shape
        self._shared = None
        if shared_prefix is not None:
            trunk, n_pre = shared_prefix
            if not (many_rows and past_key_values is None and self.supports_shared_prefix and position_ids is not None
                    and len(n_pre) == B and trunk.B == 1 and max(n_pre) <= trunk.length):
                raise ValueError("shared_prefix goes with many_rows=True, explicit position ids, no past_key_values and a one-row "
                                 "trunk arena that holds every prefix")
            self._shared = (trunk, torch.tensor(list(n_pre), device=dev, dtype=torch.int32), int(max(n_pre)))
        arena, past_len = self._resolve_arena(past_key_values, B, q_len, keep_pending=True)
        if many_rows and self.precise_dense and past_key_values is None:
            arena.with_lo()           # a schema-encode pass: keep the residuals of every row it appends
        if position_ids is None:  # llama2.py:859-864
            position_ids = torch.arange(past_len, past_len + q_len, device=input_ids.device).unsqueeze(0).expand(B, q_len)
        position_ids = position_ids.view(-1, q_len)
        if attention_mask is not None:
            # (checked where the mask LIVES: a host mask -- what CacheEngine passes since round 5 -- costs no upload and no
            # device sync; a device mask, the reference's convention (cache_engine.py:246), is read back for the test: one
            # pipeline drain per forward, which is what made 10 % of the schema encode's wall time idle in rounds 1-4)
            am = attention_mask
            # only right padding is expressible without an explicit mask (cache_engine.py:38-47 pads right)
            if am.dim() == 2 and am.shape[1] == q_len and bool((am[:, 1:] > am[:, :-1]).any()):
                raise NotImplementedError("left / interior padding masks are not supported by the HIP path")

        T = B * q_len
        self._kv_only = bool(kv_only)
        self._past_lens = None
        if past_lens is not None:
            if not (many_rows and past_key_values is not None):
                raise ValueError("past_lens goes with many_rows=True over an encode arena")
            self._past_lens = past_lens.to(device=dev, dtype=torch.int32).contiguous()
        # a schema-encode pass (fresh arena, or a suffix over a trunk arena that carries residuals) always takes the
        # many-row path, however few rows it has: that path alone reads the prefix's residual planes and stops after the
        # last layer's K / V; and a pass that is not the serving prefill / decode must not capture a throwaway hipGraph
        encode_pass = many_rows and (self._past_lens is not None or
                                     self.precise_dense and (past_key_values is None or arena.lo is not None))
        graphed = self.skinny and T <= self.SKINNY_MAX_ROWS and self.use_graphs and not many_rows and not kv_only
        mid = self.skinny and not encode_pass and not kv_only and T <= self.MID_MAX_ROWS and \
            not (many_rows and self.precise_dense and T > self.SKINNY_MAX_ROWS)   # (the streaming stacks have no kv_only exit)
        streaming = graphed or mid
        self._lo_mode = self._tail_mode(arena, q_len, past_len) if streaming else 0
        if mid and not graphed and self.graph_mid and self.use_graphs and B == 1 and not many_rows and not self.llm_int8 and \
                T > self.SKINNY_MAX_ROWS and (self._shared_prefix_loop or type(self)._forward_skinny is LlamaHIP._forward_skinny):
            graphed = True                    # a long question over a staged cache: the row-split stack, captured per 16-row bucket
        if graphed:
            # Token ids and positions on the HOST (what GenerationEngine hands over) travel with the call's other words in one
            # pinned copy (_InputBlock); device tensors (the reference's calling convention, generation_engine.py:96-97) are
            # copied into the graph's input block on the device.  A pending staging is consumed by the attention launches.
            logits = self._graphed_skinny(input_ids.reshape(-1), position_ids.reshape(-1), arena, B, q_len, past_len,
                                          last_token_only, num_layers)
            arena.length = past_len + q_len
            self._tail_done(arena, self._lo_mode, q_len, past_len)
            return CausalLMOutput(logits=logits, past_key_values=arena.views() if use_cache else None)
        arena.materialize()           # every other path reads staged rows from the arena itself
        input_ids, position_ids = input_ids.to(dev), position_ids.to(dev)
        pos32 = position_ids.reshape(-1).to(torch.int32).contiguous()
        ids = input_ids.reshape(-1).to(torch.int64).contiguous()
        # an encode pass of 65..512 rows without per-row prefixes (the trunk of a schema, small whole scaffolds) runs the
        # row-split weight-streaming stack as well: same split-precision arithmetic, residuals of every row into arena.lo
        if (encode_pass and self.skinny and self.encode_mid and self._shared_prefix_loop and self._shared is None and self._past_lens is None
                and not self.llm_int8 and self.SKINNY_MAX_ROWS < T <= self.MID_MAX_ROWS and arena.lo is not None
                and arena.lo_len == past_len):
            self._lo_mode = 3                                # residual rows go to arena.lo (arena-shaped, row = key index)
            logits = self._forward_skinny(ids, pos32, None, arena, B, q_len, past_len, last_token_only, num_layers)
            arena.length = past_len + q_len
            arena.lo_len = past_len + q_len
            self._tail_done(arena, 0, q_len, past_len)
            return CausalLMOutput(logits=logits, past_key_values=arena.views() if use_cache else None)
        if mid:
            logits = self._forward_skinny(ids, pos32, None, arena, B, q_len, past_len, last_token_only, num_layers)
            arena.length = past_len + q_len
            self._tail_done(arena, self._lo_mode, q_len, past_len)
            return CausalLMOutput(logits=logits, past_key_values=arena.views() if use_cache else None)

        logits = self._forward_dense(ids, pos32, arena, B, q_len, past_len, last_token_only, num_layers)
        arena.length = past_len + q_len
        self._tail_done(arena, self._lo_mode, q_len, past_len)       # (_dense_pass_lo sets mode 1 when it starts a tail)
        return CausalLMOutput(logits=logits, past_key_values=arena.views() if use_cache else None)

    # ------------------------------------------------------------------------------------------
    def rows_kslices(self, T: int, N: int) -> int:
        """K slices of the N = hidden projections (o_proj, down_proj) of a T-row pass.  65..288 rows run the wide-panel form of
        the row-split kernel (128 columns per workgroup, csrc/pc_gemm_rows.hip): N / 128 panels, so the slices are what fills the
        256 CUs (13b: 40 panels x 6).  Other row counts keep 4."""
        forced = os.environ.get("PC_ROWS_KQ")
        if forced:
            return int(forced)
        if self.SKINNY_MAX_ROWS < T <= 512 and os.environ.get("PC_ROWS_WIDE", "1") != "0":
            blocks = 1 if T <= 288 else 2                     # (289..512 rows: two row blocks per column panel)
            # (above 128 rows six slices beat eight at the 7b shape -- 192 workgroups, fewer slabs for the norm to fold:
            # q = 130 / 194 / 258 / 288: 7.56 / 9.31 / 11.49 / 12.53 -> 7.45 / 9.09 / 10.97 / 11.92 ms; profiles/r04_variants.txt)
            return max(1, min(8 if T <= 128 else 6, 256 // (blocks * -(-N // 128))))
        return self.kslices

    def _w16(self, lw: dict, key: str, frag: bool):
        """The fp16 image of the decoder linear ``key`` of layer ``lw`` for the launch that follows: the fragment image of the
        weight-streaming kernels (``frag``; q|k|v in ``_qkv_perm`` order) or the row-major one of pc_gemm_dense.  The resident
        tensor when the model keeps one; ``keep_fp16=False``: ``pc_w4_expand`` of the 4-bit images into the model's scratch, on
        the current stream -- so it is captured with a graph's launches -- and a view of the scratch, valid until the next call."""
        if self.keep_fp16 or key + "_c4" not in lw:          # (lm_head goes through _proj with a dict of its own: always resident)
            return lw[key + "_f" if frag else key]
        ci, si = lw[key + "_c4"], lw[key + "_e4"]
        N, K = 16 * ci.shape[0], 128 * ci.shape[1]
        out = self._w16_scratch[:N * K]
        if frag:
            _native.w4_expand(ci, si, out, N, K, _native.W4_EXPAND_FRAG, row_perm=self._qkv_perm_i32 if key == "wqkv" else None)
            return out.view(N // 16, K // 32, 4, 16, 8)
        _native.w4_expand(ci, si, out, N, K, _native.W4_EXPAND_ROWMAJOR, ld_out=K)
        return out.view(N, K)

    def _proj(self, a_hi, a_lo, lw: dict, key: str, M: int, N: int, K: int, epi: int, **out) -> None:
        """One many-row projection on the hand-written MFMA kernel (pc_gemm_dense.hip): ``(a_hi + a_lo) @ W^T`` with the
        epilogue fused.  int8 mode: ``lw[key]`` holds the int8 codes as fp16 (exact) and the per-output scales
        (``key_ds``) are applied to the accumulator tile -- the many-row paths then compute with exactly the dequantised
        weights the streaming kernels use."""
        ws = None
        if epi in (_native.EPI_ADD, _native.EPI_STORE) and M <= 2048:
            # few-row launches of the N = hidden projections cut K into slices (pc_gemm_dense_ws): the slabs of the widest
            # split it ever takes are 256 tiles x 128 x 256 x 4 B
            ws = getattr(self, "_dense_ws", None)
            if ws is None:
                ws = self._dense_ws = torch.empty(34 << 20, dtype=torch.uint8, device=self.device)
        w8 = lw.get(key + "_q8") if (a_lo is not None and self.dense_lo8) else None
        if w8 is not None:
            # the residual plane on the int8 MFMA: one quantiser launch (M x K x 3 bytes of traffic), then the projection
            codes, sc = self._lo8_codes(a_lo, M, K)
            _native.gemm_dense_lo8(a_hi, codes, sc, lw[key], w8, lw[key + "_q8s"], M, N, K, epi, workspace=ws, **out)
            return
        _native.gemm_dense(a_hi, a_lo, self._w16(lw, key, False), M, N, K, epi, wscale=lw.get(key + "_ds"), workspace=ws, **out)

    def _lo8_codes(self, a_lo, M: int, K: int):
        """Row-wise absmax int8 codes + scales of a residual activation plane (pc_quant_rows_i8)."""
        codes = torch.empty((M, K), dtype=torch.int8, device=self.device)
        sc = torch.empty(M, dtype=torch.float32, device=self.device)
        _native.quant_rows_i8(a_lo, M, K, codes, sc)
        return codes, sc

    def _forward_dense(self, ids, pos32, arena, B, q_len, past_len, last_token_only, num_layers):
        """Layer stack for many rows (schema encode, no-cache prefill): every projection is a pc_gemm_dense launch with
        its residual add / SiLU*up fused; RMSNorm, RoPE + KV append and the attention are HIP kernels between them.
        precise_dense (default): split-precision activations (hi, lo fp16 planes) -- an fp16 activation costs 2^-12 per
        projection input and through 32 layers that alone moves 7b-shape logits by 2-3e-2 against the reference's fp32
        path (the module KV an encode stores drifts the same way).  Both planes meet the same weight fragments inside
        the GEMM tile; Q, P and the pass's own K / V rows are split-precision in the attention as well.
        PC_FAST_DENSE=1: the hi plane only (half the MFMA work, fp16-activation accuracy)."""
        if self.llm_int8:
            return self._forward_dense_int8(ids, pos32, arena, B, q_len, past_len, last_token_only, num_layers)
        n = _native
        dev = self.device
        two = self.precise_dense
        H, Hkv, D, hid = self.H, self.Hkv, self.D, self.config.hidden_size
        inter = self.config.intermediate_size
        T = B * q_len
        W = (H + 2 * Hkv) * D
        eps = self.config.rms_norm_eps
        f32 = torch.float32
        cs = torch.empty((T, D // 2, 2), dtype=f32, device=dev)
        n.rope_table(pos32, self.inv_freq, cs, T, D)
        h2 = torch.empty((2, T, hid), dtype=self.dtype, device=dev)          # (hi, lo) of the normalised stream
        n.embed_gather(self.embed, ids, h2[0], T, hid, self.config.vocab_size)
        x = h2[0].float()  # fp32 residual stream
        attn2 = torch.empty((2, T, H * D), dtype=self.dtype, device=dev)
        act2 = torch.empty((2, T, inter), dtype=self.dtype, device=dev)
        q16 = torch.empty((T, H * D), dtype=self.dtype, device=dev)
        q16l = torch.empty((T, H * D), dtype=self.dtype, device=dev) if two else None
        lo_for, full_lo = self._dense_pass_lo(arena, B, Hkv, q_len, past_len) if two else ((lambda li: None), False)
        # shared prefix: the rows of this pass sit at arena rows [0, q_len) and the attention walks the trunk's planes first
        trunk, pre_lens, pre_max = self._shared if self._shared is not None else (None, self._past_lens, past_len)
        trunk_lo = trunk is not None and trunk.lo is not None and trunk.lo_len >= pre_max

        def prefix_of(li):
            if trunk is None:
                return None
            return (trunk.buf[0, li, 0], trunk.buf[0, li, 1], trunk.lo[0, li, 0] if trunk_lo else None,
                    trunk.lo[0, li, 1] if trunk_lo else None, trunk.head_stride)
        ws = self._workspace(n.attn_workspace_bytes(B, H, D, q_len, pre_max + q_len))
        lo = (lambda t: t[1]) if two else (lambda t: None)
        layers = self.layers if num_layers is None else self.layers[:num_layers]

        def norm(src, gain, rows, want_lo=True):
            if two and want_lo:
                n.rmsnorm_split(src, gain, h2[0], h2[1], rows, hid, eps)
            else:
                n.rmsnorm(src, gain, h2[0], rows, hid, eps, True)

        # head_dim 128, fp16 weights: RoPE and the KV append run in the q|k|v projection's epilogue (pc_gemm_dense_qkv_rope);
        # otherwise the projection leaves fp32 [T, W] for pc_rope_append
        fused_qkv = D == 128 and len(layers) > 0 and layers[0].get("wqkv_ds") is None and self.fused_dense_qkv
        qkv = None if fused_qkv else torch.empty((T, W), dtype=f32, device=dev)
        skip = self.dense_lo_skip                  # dev probe (PC_DENSE_LO_SKIP): projections that run on the hi plane only
        lo_q = (lambda t: None) if "qkv" in skip else lo
        lo_o = (lambda t: None) if "o" in skip else lo
        lo_g = (lambda t: None) if "gu" in skip else lo
        lo_d = (lambda t: None) if "down" in skip else lo
        for li, lw in enumerate(layers):
            norm(x, lw["ln1"], T)
            kp, vp = arena.k_plane(li), arena.v_plane(li)
            kv_lo = lo_for(li)
            if fused_qkv:
                xlo, lo8 = lo_q(h2), None
                if xlo is not None and self.dense_lo8 and lw.get("wqkv_q8") is not None:
                    codes, sc = self._lo8_codes(xlo, T, hid)
                    xlo, lo8 = None, (codes, sc, lw["wqkv_q8"], lw["wqkv_q8s"])
                n.gemm_dense_qkv_rope(h2[0], xlo, self._w16(lw, "wqkv", False), hid, cs, q16, q16l, H * D, kp, vp, arena.batch_stride,
                                      arena.head_stride, B, H, Hkv, D, q_len, past_len, arena.cap, kv_lo=kv_lo,
                                      past_lens=self._past_lens, lo8=lo8)
            else:
                self._proj(h2[0], lo_q(h2), lw, "wqkv", T, W, hid, n.EPI_STORE, y=qkv)
                n.rope_append(qkv, q_len * W, W, q16, q_len * H * D, H * D, qkv[:, H * D:], qkv[:, (H + Hkv) * D:], q_len * W, W,
                              kp, vp, arena.batch_stride, arena.head_stride, cs, B, H, Hkv, D, q_len, past_len, arena.cap, True,
                              q_out_lo=q16l, kv_lo=kv_lo, past_lens=self._past_lens)
            if self._kv_only and li == len(layers) - 1:
                break             # schema encode: the K / V of the last layer are written; nothing after them is used
            # q_lo: split-precision Q and P in the attention as well (fp16 Q alone costs 1.6e-2 on 32-layer logits)
            n.attn_fwd(q16, q_len * H * D, H * D, kp, vp, arena.batch_stride, arena.head_stride, attn2[0],
                       q_len * H * D, H * D, B, H, Hkv, D, q_len, pre_max, self.softmax_scale, ws, q_lo=q16l,
                       out_lo=lo(attn2), kv_lo=kv_lo, past_lens=pre_lens, prefix=prefix_of(li))
            self._proj(attn2[0], lo_o(attn2), lw, "wo", T, hid, H * D, n.EPI_ADD, y=x)                  # x += attn @ Wo^T
            norm(x, lw["ln2"], T, want_lo="gu" not in skip)
            self._proj(h2[0], lo_g(h2), lw, "wgu", T, 2 * inter, hid, n.EPI_SILU, out_hi=act2[0], out_lo=lo_d(act2))
            self._proj(act2[0], lo_d(act2), lw, "wdown", T, hid, inter, n.EPI_ADD, y=x)                 # x += act @ Wd^T
        if full_lo:
            arena.lo_len = past_len + q_len
        if self._kv_only:
            return None
        head = {"lm_head": self.lm_head}
        V = self.config.vocab_size
        if last_token_only:
            xl = x.view(B, q_len, hid)[:, -1, :].contiguous()
            norm(xl, self.norm, B)
            logits = torch.empty((B, V), dtype=f32, device=dev)
            self._proj(h2[0, :B], h2[1, :B] if two else None, head, "lm_head", B, V, hid, n.EPI_STORE, y=logits)
            return logits.view(B, 1, V)
        norm(x, self.norm, T)
        logits = torch.empty((T, V), dtype=f32, device=dev)
        self._proj(h2[0], lo(h2), head, "lm_head", T, V, hid, n.EPI_STORE, y=logits)   # llama2.py:1050-1051: every row
        return logits.view(B, q_len, V)

    # ------------------------------------------------------------------------------------------
    # LLM.int8 layer stacks (load_in_8bit=True): every decoder-layer projection input is quantised vector-wise to int8 codes
    # (pc_quant_act_i8), the projection runs over weight codes x activation codes and is rescaled by w_scale[n] * x_scale[m]
    # in its epilogue, and columns holding an activation >= 6 are carried in fp16 (pc_outlier_corr) -- Dettmers et al. 2022 as
    # bitsandbytes' Linear8bitLt applies it.  Norms, RoPE, attention, residual stream and lm_head are the fp16-mode kernels.
    def _i8_lin_frag(self, slot, act_hi, K, lw, key, perm, T, N, bufs, norm=None):
        """Quantise a fragment-plane activation (its hi plane is the fp16 value bitsandbytes would see) and prepare the outlier
        correction for projection ``key``: -> (codes, x_scale, corr, has).  ``norm=(x_f32, gain, eps)``: the activation is
        RMSNorm(x) -- normalised, written to ``act_hi`` and quantised in ONE launch (pc_rmsnorm_quant_i8)."""
        n = _native
        codes, xs, corr, has, c8 = bufs
        if norm is not None:
            n.rmsnorm_quant_i8(norm[0], norm[1], norm[2], T, K, act_hi, codes, xs, self._i8_flags[slot], self._i8_flags[(slot + 1) % 4],
                               codes8=c8)
        else:
            n.quant_act_i8(act_hi, True, T, K, codes, xs, self._i8_flags[slot], self._i8_flags[(slot + 1) % 4], codes8=c8)
        n.outlier_corr(self._i8_flags[slot], K, act_hi, codes, True, xs, lw[key + "_t8"], lw[key + "_ds"], perm, T, N, corr, has)
        return codes, xs, corr, has

    def _forward_skinny_int8(self, ids, pos32, past_dev, arena, B, q_len, past_len, last_token_only, num_layers):
        n = _native
        dev = self.device
        c = self.config
        H, Hkv, D, hid, inter = self.H, self.Hkv, self.D, c.hidden_size, c.intermediate_size
        T = B * q_len
        W = (H + 2 * Hkv) * D
        eps = c.rms_norm_eps
        mt = (T + 15) // 16
        f32 = torch.float32
        cs = torch.empty((T, D // 2, 2), dtype=f32, device=dev)
        n.rope_table(pos32, self.inv_freq, cs, T, D)
        h16 = torch.empty((T, hid), dtype=self.dtype, device=dev)
        n.embed_gather(self.embed, ids, h16, T, hid, c.vocab_size)
        x = h16.float()
        q16 = torch.empty((T, H * D), dtype=self.dtype, device=dev)
        q16l = torch.empty((T, H * D), dtype=self.dtype, device=dev)
        ws = torch.empty(max(n.attn_workspace_bytes(B, H, D, q_len, past_len + q_len), 4) // 4, dtype=f32, device=dev)
        tail = self._tail_for(arena, past_dev)

        def planes(k, cnt=2):
            return tuple(torch.empty((mt, k // 32, 64, 8), dtype=self.dtype, device=dev) for _ in range(cnt))

        xh, xl, xq = planes(hid, 3)
        ah, al, aq = planes(H * D, 3)
        ch, cl, cq = planes(inter, 3)
        zero = self._i8_zero
        q8_all = self.i8_inlaunch and T <= self.q8_p_max_rows          # every quantiser inside its projection
        q8_down = self.i8_inlaunch and self.i8_fused_corr and T <= 16    # at least down_proj's
        # (the correction-has words of the two-launch forms: one fill node per forward, not needed when the projections quantise)
        has = None if q8_all else torch.zeros(4, dtype=torch.int32, device=dev)

        def image8(k):        # the int8 MFMA's operand image of a code plane (pc_quant_act_i8 codes8; K % 64 == 0 with int8 weights)
            return torch.empty((mt, k // 64, 64, 16), dtype=torch.int8, device=dev)

        x8, a8, c8 = image8(hid), image8(H * D), image8(inter)
        bufs = None if q8_all else \
            [(xq, torch.empty(T, dtype=f32, device=dev), torch.empty((T, W), dtype=f32, device=dev), has[0:1], x8),
             (aq, torch.empty(T, dtype=f32, device=dev), torch.empty((T, hid), dtype=f32, device=dev), has[1:2], a8),
             (xq, torch.empty(T, dtype=f32, device=dev), torch.empty((T, 2 * inter), dtype=f32, device=dev), has[2:3], x8),
             (cq, torch.empty(T, dtype=f32, device=dev), torch.empty((T, hid), dtype=f32, device=dev), has[3:4], c8)]
        layers = self.layers if num_layers is None else self.layers[:num_layers]
        # Outlier flags are set-only and slot s is cleared by the quantiser of slot s - 1: a pass that stopped behind a
        # layer's q|k|v (kv_only encodes) left slot 0 set, and this pass's first quantiser would OR onto it -- results would
        # depend on the call history.  One memset node (graph-capturable) makes every forward start clean.
        if not q8_all:
            self._i8_flags[0].zero_()
        if q8_all:
            # every projection derives its input's codes / row scales / outlier flags itself (csrc/pc_gemm_q8.hip): q|k|v and gate|up
            # from the fp32 residual stream (RMSNorm folded in), o_proj from the attention's fp16 plane, down_proj from the plane, the
            # per-tile row maxima and the flag bytes gate|up's SiLU epilogue leaves (the o_proj launch zeroes those flag bytes)
            qf, pm = self._q8_flags, self._q8_pmax
            sc, ctr = self._ks_buffers(hid)
            for li, lw in enumerate(layers):
                kp, vp = arena.k_plane(li), arena.v_plane(li)
                kvlo, lo_base = tail(li)
                lo4 = (None, None, 0, 0) if not kvlo else kvlo[:4]
                n.gemm_q8(epilogue=n.EPI_QKV_ROPE, wf=lw["wqkv_f"], w_scale=lw["wqkv_s"], w_codes_t=lw["wqkv_t8"], row_perm=self._qkv_perm_i32,
                          x=x, norm_weight=lw["ln1"], eps=eps, M=T, K=hid, cs=cs, q_hi=q16, q_lo=q16l, q_token_stride=H * D, k_arena=kp,
                          v_arena=vp, arena_batch_stride=arena.batch_stride, arena_head_stride=arena.head_stride, B=B, H=H, Hkv=Hkv, D=D,
                          q_len=q_len, past_len=past_len, cap=arena.cap, past_len_dev=past_dev, k_lo=lo4[0], v_lo=lo4[1],
                          lo_batch_stride=lo4[2], lo_head_stride=lo4[3], lo_base=lo_base)
                # (one row -- a decode step: the attention leaves its split-KV partials in `ws` and the o_proj launch merges them in
                # its prologue; the merge launch, 4.8 us of a 75 us layer, disappears)
                ns = n.attn_fwd(q16, q_len * H * D, H * D, kp, vp, arena.batch_stride, arena.head_stride, None, 0, 0,
                                B, H, Hkv, D, q_len, past_len, self.softmax_scale, ws, past_len_dev=past_dev, out_frag=(ah, al),
                                q_lo=q16l, kv_lo=kvlo,
                                gather=None if self._gather is None else (self._gather, li * 2 * Hkv, (li * 2 + 1) * Hkv),
                                defer_merge=self.q8_defer_merge and T == 1 and H * D <= 4096)
                src = dict(xf_hi=ah) if ns <= 1 else dict(part_o=ws, part_ml=ws[H * ns * D:], part_nsplit=ns, part_head_dim=D)
                n.gemm_q8(epilogue=n.EPI_ADD, wf=lw["wo_f"], w_scale=lw["wo_s"], w_codes_t=lw["wo_t8"], M=T, N=hid, K=H * D,
                          y=x, ldy=hid, flags_clear=qf, clear_bytes=qf.numel(), **src)
                n.gemm_q8(epilogue=n.EPI_SILU, wf=lw["wgu_f"], w_scale=lw["wgu_s"], w_codes_t=lw["wgu_t8"], x=x, norm_weight=lw["ln2"],
                          eps=eps, M=T, N=2 * inter, K=hid, of_hi=ch, row_max_out=pm, flags_out=qf)
                dn = self.q8_down_small if T <= 4 else self.q8_down
                n.gemm_q8(epilogue=n.EPI_ADD, wf=lw["wdown_f"], w_scale=lw["wdown_s"], w_codes_t=lw["wdown_t8"], xf_hi=ch, row_max=pm,
                          row_max_units=inter // 16, flags_in=qf, M=T, N=hid, K=inter, y=x, ldy=hid, ks_tiles=dn[0],
                          kslices=dn[1], ks_scratch=sc, ks_scratch_bytes=sc.numel() * 4, ks_counters=ctr)
            layers = []
        elif self.i8_fused_corr:
            # the outlier correction runs INSIDE the projection launches (pc_gemm_*_a8c): 10 launches per layer instead of 14
            fl = self._i8_flags
            pm = self._q8_pmax
            ksc, kctr = self._ks_buffers(hid) if q8_down else (None, None)
            q8_img = q8_down and self.q8_image and hid <= 6144

            def quant(slot, act_hi, K, buf, norm=None):
                codes, xs = buf[0], buf[1]
                if norm is not None:
                    n.rmsnorm_quant_i8(norm[0], norm[1], eps, T, K, act_hi, codes, xs, fl[slot], fl[(slot + 1) % 4], codes8=buf[4])
                else:
                    n.quant_act_i8(act_hi, True, T, K, codes, xs, fl[slot], fl[(slot + 1) % 4], codes8=buf[4])
                return codes, xs

            for li, lw in enumerate(layers):
                kp, vp = arena.k_plane(li), arena.v_plane(li)
                kvlo, lo_base = tail(li)
                cd, xs = quant(0, xh, hid, bufs[0], norm=(x, lw["ln1"]))
                if q8_img:
                    # (5..16 rows: the quantiser stays a launch, but the projection is pc_gemm_q8's -- the image copied to LDS once,
                    # activation operands read from there, two weight blocks in flight; same bits as pc_gemm with x_scale + flags)
                    lo4 = (None, None, 0, 0) if not kvlo else kvlo[:4]
                    n.gemm_q8(epilogue=n.EPI_QKV_ROPE, wf=lw["wqkv_f"], w_scale=lw["wqkv_s"], w_codes_t=lw["wqkv_t8"], row_perm=self._qkv_perm_i32,
                              xf_hi=xh, x_codes8=x8, x_scale=xs, x_flags=fl[0], M=T, K=hid, cs=cs, q_hi=q16, q_lo=q16l, q_token_stride=H * D,
                              k_arena=kp, v_arena=vp, arena_batch_stride=arena.batch_stride, arena_head_stride=arena.head_stride, B=B, H=H,
                              Hkv=Hkv, D=D, q_len=q_len, past_len=past_len, cap=arena.cap, past_len_dev=past_dev, k_lo=lo4[0], v_lo=lo4[1],
                              lo_batch_stride=lo4[2], lo_head_stride=lo4[3], lo_base=lo_base)
                else:
                    n.gemm_qkv_rope_a8c(lw["wqkv_f"], lw["wqkv_s"], cd, zero, xs, fl[0], xh, lw["wqkv_t8"], self._qkv_perm_i32, T, hid, cs,
                                        q16, q16l, H * D, kp, vp, arena.batch_stride, arena.head_stride, B, H, Hkv, D, q_len, past_len,
                                        arena.cap, past_dev, kv_lo=kvlo and kvlo[:4], lo_base=lo_base, codes8=x8)
                n.attn_fwd(q16, q_len * H * D, H * D, kp, vp, arena.batch_stride, arena.head_stride, None, 0, 0,
                           B, H, Hkv, D, q_len, past_len, self.softmax_scale, ws, past_len_dev=past_dev, out_frag=(ah, al),
                           q_lo=q16l, kv_lo=kvlo,
                           gather=None if self._gather is None else (self._gather, li * 2 * Hkv, (li * 2 + 1) * Hkv))
                cd, xs = quant(1, ah, H * D, bufs[1])
                if q8_img and H * D <= 6144:
                    n.gemm_q8(epilogue=n.EPI_ADD, wf=lw["wo_f"], w_scale=lw["wo_s"], w_codes_t=lw["wo_t8"], xf_hi=ah, x_codes8=a8, x_scale=xs,
                              x_flags=fl[1], M=T, N=hid, K=H * D, y=x, ldy=hid)
                else:
                    n.gemm_skinny_a8c(lw["wo_f"], lw["wo_s"], cd, zero, xs, fl[1], ah, lw["wo_t8"], T, hid, H * D, n.EPI_ADD, y=x, ldy=hid,
                                      codes8=a8)
                cd, xs = quant(2, xh, hid, bufs[2], norm=(x, lw["ln2"]))
                # (more than q8_p_max_rows rows: the quantisers of q|k|v, o_proj and gate|up stay launches -- a 12-row prologue in
                # every workgroup costs more vector ALU time than the launch it saves -- but down_proj reads what this SiLU
                # epilogue leaves: flag slot 3 was zeroed by the quantiser above, slot 0 is zeroed by the down_proj launch)
                if q8_img:
                    n.gemm_q8(epilogue=n.EPI_SILU, wf=lw["wgu_f"], w_scale=lw["wgu_s"], w_codes_t=lw["wgu_t8"], xf_hi=xh, x_codes8=x8, x_scale=xs,
                              x_flags=fl[2], M=T, N=2 * inter, K=hid, of_hi=ch, of_lo=cl, row_max_out=pm, flags_out=fl[3])
                else:
                    n.gemm_skinny_a8c(lw["wgu_f"], lw["wgu_s"], cd, zero, xs, fl[2], xh, lw["wgu_t8"], T, 2 * inter, hid, n.EPI_SILU,
                                      of_hi=ch, of_lo=cl, codes8=x8, row_max_out=pm if q8_down else None, flags_out=fl[3] if q8_down else None)
                if q8_down:
                    n.gemm_q8(epilogue=n.EPI_ADD, wf=lw["wdown_f"], w_scale=lw["wdown_s"], w_codes_t=lw["wdown_t8"], xf_hi=ch, row_max=pm,
                              row_max_units=inter // 16, flags_in=fl[3], M=T, N=hid, K=inter, y=x, ldy=hid, ks_tiles=self.q8_down[0],
                              kslices=self.q8_down[1], ks_scratch=ksc, ks_scratch_bytes=ksc.numel() * 4, ks_counters=kctr,
                              flags_clear=fl[0], clear_bytes=16384)
                    continue
                cd, xs = quant(3, ch, inter, bufs[3])
                n.gemm_skinny_a8c(lw["wdown_f"], lw["wdown_s"], cd, zero, xs, fl[3], ch, lw["wdown_t8"], T, hid, inter, n.EPI_ADD,
                                  y=x, ldy=hid, codes8=c8)
            layers = []
        for li, lw in enumerate(layers):
            kp, vp = arena.k_plane(li), arena.v_plane(li)
            kvlo, lo_base = tail(li)
            cd, xs, corr, hs = self._i8_lin_frag(0, xh, hid, lw, "wqkv", self._qkv_perm_i32, T, W, bufs[0], norm=(x, lw["ln1"], eps))
            n.gemm_qkv_rope_a8(lw["wqkv_f"], lw["wqkv_s"], cd, zero, xs, corr, hs, T, hid, cs, q16, q16l, H * D, kp, vp,
                               arena.batch_stride, arena.head_stride, B, H, Hkv, D, q_len, past_len, arena.cap, past_dev,
                               kv_lo=kvlo and kvlo[:4], lo_base=lo_base, codes8=x8)
            n.attn_fwd(q16, q_len * H * D, H * D, kp, vp, arena.batch_stride, arena.head_stride, None, 0, 0,
                       B, H, Hkv, D, q_len, past_len, self.softmax_scale, ws, past_len_dev=past_dev, out_frag=(ah, al),
                       q_lo=q16l, kv_lo=kvlo, counters=self._counters_for(B, H),
                       gather=None if self._gather is None else (self._gather, li * 2 * Hkv, (li * 2 + 1) * Hkv))
            cd, xs, corr, hs = self._i8_lin_frag(1, ah, H * D, lw, "wo", None, T, hid, bufs[1])
            n.gemm_skinny_a8(lw["wo_f"], lw["wo_s"], cd, zero, xs, corr, hs, T, hid, H * D, n.EPI_ADD, y=x, ldy=hid, codes8=a8)
            cd, xs, corr, hs = self._i8_lin_frag(2, xh, hid, lw, "wgu", None, T, 2 * inter, bufs[2], norm=(x, lw["ln2"], eps))
            n.gemm_skinny_a8(lw["wgu_f"], lw["wgu_s"], cd, zero, xs, corr, hs, T, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl, codes8=x8)
            cd, xs, corr, hs = self._i8_lin_frag(3, ch, inter, lw, "wdown", None, T, hid, bufs[3])
            n.gemm_skinny_a8(lw["wdown_f"], lw["wdown_s"], cd, zero, xs, corr, hs, T, hid, inter, n.EPI_ADD, y=x, ldy=hid, codes8=c8)
        V = c.vocab_size
        if last_token_only:
            xlast = x.view(B, q_len, hid)[:, -1, :].contiguous()
            lh, ll = planes(hid)
            n.rmsnorm_frag(xlast, self.norm, lh, ll, B, hid, eps)
            logits = torch.empty((B, V), dtype=f32, device=dev)
            n.gemm_skinny(self.lm_head_f, lh, ll, B, V, hid, n.EPI_STORE, y=logits, ldy=V)
            return logits.view(B, 1, V)
        n.rmsnorm_frag(x, self.norm, xh, xl, T, hid, eps)
        logits = torch.empty((T, V), dtype=f32, device=dev)
        n.gemm_skinny(self.lm_head_f, xh, xl, T, V, hid, n.EPI_STORE, y=logits, ldy=V)
        return logits.view(B, q_len, V)

    def _forward_dense_int8(self, ids, pos32, arena, B, q_len, past_len, last_token_only, num_layers):
        """Many-row LLM.int8 stack: row-major activations, pc_gemm_dense_a8 over the codes.  Q, P and the pass's own K / V rows
        stay split-precision in the attention, as in the fp16 mode."""
        n = _native
        dev = self.device
        H, Hkv, D, hid = self.H, self.Hkv, self.D, self.config.hidden_size
        inter = self.config.intermediate_size
        T = B * q_len
        W = (H + 2 * Hkv) * D
        eps = self.config.rms_norm_eps
        f32 = torch.float32
        cs = torch.empty((T, D // 2, 2), dtype=f32, device=dev)
        n.rope_table(pos32, self.inv_freq, cs, T, D)
        h16 = torch.empty((T, hid), dtype=self.dtype, device=dev)
        n.embed_gather(self.embed, ids, h16, T, hid, self.config.vocab_size)
        x = h16.float()
        hq = torch.empty((T, hid), dtype=self.dtype, device=dev)
        attn2 = torch.empty((2, T, H * D), dtype=self.dtype, device=dev)
        aq = torch.empty((T, H * D), dtype=self.dtype, device=dev)
        act = torch.empty((T, inter), dtype=self.dtype, device=dev)
        cq = torch.empty((T, inter), dtype=self.dtype, device=dev)
        q16 = torch.empty((T, H * D), dtype=self.dtype, device=dev)
        q16l = torch.empty((T, H * D), dtype=self.dtype, device=dev)
        qkv = torch.empty((T, W), dtype=f32, device=dev)
        xs = torch.empty(T, dtype=f32, device=dev)
        corr = torch.empty(T * max(W, 2 * inter), dtype=f32, device=dev)
        has = torch.zeros(4, dtype=torch.int32, device=dev)
        lo_for, full_lo = self._dense_pass_lo(arena, B, Hkv, q_len, past_len)
        ws = self._workspace(n.attn_workspace_bytes(B, H, D, q_len, past_len + q_len))
        layers = self.layers if num_layers is None else self.layers[:num_layers]
        fl = self._i8_flags
        fl[0].zero_()                            # (see _forward_skinny_int8: a kv_only pass leaves slot 0 set)

        def lin(slot, a16, codes, K, lw, key, N, epi, **out):
            n.quant_act_i8(a16, False, T, K, codes, xs, fl[slot], fl[(slot + 1) % 4])
            cv = corr[:T * N].view(T, N)
            n.outlier_corr(fl[slot], K, a16, codes, False, xs, lw[key + "_t8"], lw[key + "_ds"], None, T, N, cv, has[slot:slot + 1])
            n.gemm_dense_a8(codes, lw[key], lw[key + "_ds"], xs, cv, has[slot:slot + 1], T, N, K, epi, **out)

        for li, lw in enumerate(layers):
            n.rmsnorm(x, lw["ln1"], h16, T, hid, eps, True)
            lin(0, h16, hq, hid, lw, "wqkv", W, n.EPI_STORE, y=qkv)
            kp, vp = arena.k_plane(li), arena.v_plane(li)
            kv_lo = lo_for(li)
            n.rope_append(qkv, q_len * W, W, q16, q_len * H * D, H * D, qkv[:, H * D:], qkv[:, (H + Hkv) * D:], q_len * W, W,
                          kp, vp, arena.batch_stride, arena.head_stride, cs, B, H, Hkv, D, q_len, past_len, arena.cap, True,
                          q_out_lo=q16l, kv_lo=kv_lo, past_lens=self._past_lens)
            if self._kv_only and li == len(layers) - 1:
                break
            n.attn_fwd(q16, q_len * H * D, H * D, kp, vp, arena.batch_stride, arena.head_stride, attn2[0],
                       q_len * H * D, H * D, B, H, Hkv, D, q_len, past_len, self.softmax_scale, ws, q_lo=q16l,
                       out_lo=attn2[1], kv_lo=kv_lo, past_lens=self._past_lens)
            lin(1, attn2[0], aq, H * D, lw, "wo", hid, n.EPI_ADD, y=x)
            n.rmsnorm(x, lw["ln2"], h16, T, hid, eps, True)
            lin(2, h16, hq, hid, lw, "wgu", 2 * inter, n.EPI_SILU, out_hi=act)
            lin(3, act, cq, inter, lw, "wdown", hid, n.EPI_ADD, y=x)
        if full_lo:
            arena.lo_len = past_len + q_len
        if self._kv_only:
            return None
        V = self.config.vocab_size
        head = {"lm_head": self.lm_head}
        h2 = torch.empty((2, T, hid), dtype=self.dtype, device=dev)
        if last_token_only:
            xl = x.view(B, q_len, hid)[:, -1, :].contiguous()
            n.rmsnorm_split(xl, self.norm, h2[0], h2[1], B, hid, eps)
            logits = torch.empty((B, V), dtype=f32, device=dev)
            self._proj(h2[0, :B], h2[1, :B], head, "lm_head", B, V, hid, n.EPI_STORE, y=logits)
            return logits.view(B, 1, V)
        n.rmsnorm_split(x, self.norm, h2[0], h2[1], T, hid, eps)
        logits = torch.empty((T, V), dtype=f32, device=dev)
        self._proj(h2[0], h2[1], head, "lm_head", T, V, hid, n.EPI_STORE, y=logits)
        return logits.view(B, q_len, V)

    # ------------------------------------------------------------------------------------------
    def _layers_norm_fused(self, x, cs, q16, q16l, ws, ah, al, ch, cl, arena, layers, B, q_len, past_len, past_dev,
                           last_token_only, tail=None):
        """T <= 32 rows (NORM_FUSED_MAX_ROWS): six launches per layer.  Both RMSNorms are folded into the projections that consume them
        (pc_gemm_*_norm read the fp32 residual stream directly) and both residual adds into the o_proj / down_proj
        epilogues, so x is the only activation that round-trips through memory in fp32."""
        n = _native
        c = self.config
        H, Hkv, D, hid, inter = self.H, self.Hkv, self.D, c.hidden_size, c.intermediate_size
        T, eps, V = B * q_len, c.rms_norm_eps, c.vocab_size
        # fp16 weights: everything between two attention calls -- o_proj, gate|up, down_proj and the NEXT layer's q|k|v -- is
        # one persistent launch (pc_gemm_chain: the same four bodies, bit-identical, but the weight stream runs through
        # the seams); three launches per layer instead of six.  Shapes without an instantiation fall back here.
        rows_dev = past_dev[2:3] if (past_dev is not None and past_dev.numel() > 2 and B == 1) else None
        chain = self.use_chain and layers and layers[0]["wqkv_s"] is None and T <= 16
        if chain and self._chain_sync is None:
            self._chain_sync = n.chain_sync_state(self.device)
        qkv_done = False
        # the projections of this loop on the 4-bit images (pc_gemm_w4).  (PC_NORM_FUSED_MAX=32 set by hand: 17..32 rows of this
        # loop stay on the fp16 images -- pc_gemm_w4_rows has no norm-folded source and no ADD epilogue)
        w4 = self.w4_stream and T <= 16
        if w4:
            W = (H + 2 * Hkv) * D
            qkv = torch.empty((T, W), dtype=torch.float32, device=self.device)
        for li, lw in enumerate(layers):
            kp, vp = arena.k_plane(li), arena.v_plane(li)
            kvlo, lo_base = tail(li) if tail is not None else (None, -1)
            if w4:
                # q|k|v as a plain store in natural row order, then RoPE + append (+ the residual rows: kvlo[4] is the row offset,
                # -1 / -2 = read on the device like lo_base of the fused epilogue)
                n.gemm_w4(lw["wqkv_c4"], lw["wqkv_e4"], T, W, hid, n.EPI_STORE, x=x, norm_weight=lw["ln1"], eps=eps, y=qkv, ldy=W,
                          rows_dev=rows_dev)
                n.rope_append(qkv, q_len * W, W, q16, q_len * H * D, H * D, qkv[:, H * D:], qkv[:, (H + Hkv) * D:], q_len * W, W,
                              kp, vp, arena.batch_stride, arena.head_stride, cs, B, H, Hkv, D, q_len, past_len, arena.cap, True,
                              past_len_dev=past_dev, q_out_lo=q16l, kv_lo=kvlo)
            elif not qkv_done:
                n.gemm_qkv_rope_norm(self._w16(lw, "wqkv", True), x, lw["ln1"], eps, T, hid, cs, q16, q16l, H * D, kp, vp, arena.batch_stride,
                                     arena.head_stride, B, H, Hkv, D, q_len, past_len, arena.cap, past_dev,
                                     kv_lo=kvlo and kvlo[:4], wscale=lw["wqkv_s"], lo_base=lo_base, rows_dev=rows_dev)
            qkv_done = False
            # (one row -- a decode step: the attention leaves its split-KV partials and o_proj merges them in its prologue,
            # pc_gemm_part; PC_DEFER_MERGE=0 keeps the merge launch)
            # (rows_dev: a one-row graph has one live row)
            part_ok = self.defer_merge and T == 1 and B == 1 and H * D <= 4096 and lw["wo_s"] is None and not chain and \
                self._attn_counters is None
            ns = n.attn_fwd(q16, q_len * H * D, H * D, kp, vp, arena.batch_stride, arena.head_stride, None, 0, 0,
                            B, H, Hkv, D, q_len, past_len, self.softmax_scale, ws, past_len_dev=past_dev, out_frag=(ah, al),
                            q_lo=q16l, kv_lo=kvlo, counters=self._counters_for(B, H),
                            gather=None if self._gather is None else (self._gather, li * 2 * Hkv, (li * 2 + 1) * Hkv),
                            defer_merge=part_ok)
            if w4:
                n.gemm_w4(lw["wo_c4"], lw["wo_e4"], T, hid, H * D, n.EPI_ADD, xf_hi=ah, xf_lo=al, y=x, ldy=hid, rows_dev=rows_dev)
                n.gemm_w4(lw["wgu_c4"], lw["wgu_e4"], T, 2 * inter, hid, n.EPI_SILU, x=x, norm_weight=lw["ln2"], eps=eps,
                          of_hi=ch, of_lo=cl, rows_dev=rows_dev)
                n.gemm_w4(lw["wdown_c4"], lw["wdown_e4"], T, hid, inter, n.EPI_ADD, xf_hi=ch, xf_lo=cl, y=x, ldy=hid,
                          rows_dev=rows_dev)
                continue
            if chain:
                nxt = None
                if li + 1 < len(layers):
                    nl = layers[li + 1]
                    nkv, nbase = tail(li + 1) if tail is not None else (None, -1)
                    nxt = dict(wqkv_f=nl["wqkv_f"], ln1=nl["ln1"], cs=cs, q_hi=q16, q_lo=q16l, q_ts=H * D,
                               k_arena=arena.k_plane(li + 1), v_arena=arena.v_plane(li + 1), a_bs=arena.batch_stride,
                               a_hs=arena.head_stride, B=B, H=H, Hkv=Hkv, D=D, q_len=q_len, past_len=past_len, cap=arena.cap,
                               past_len_dev=past_dev, kv_lo=nkv and nkv[:4], lo_base=nbase)
                try:
                    n.gemm_chain(lw["wo_f"], ah, al, H * D, x, T, hid, lw["wgu_f"], lw["ln2"], eps, inter, ch, cl, lw["wdown_f"],
                                 self._chain_sync, qkv=nxt)
                    qkv_done = nxt is not None
                    continue
                except RuntimeError:
                    chain = self.use_chain = False       # no instantiation for this shape: nothing was launched
            if ns > 1:
                n.gemm_part(self._w16(lw, "wo", True), ws, ws[H * ns * D:], ns, H, D, hid, x)
            elif self.ks_o and lw["wo_s"] is None and self.ks_min_rows <= T <= 32 and (T <= 16 or (self.ks_o[1] <= 4 and self.ks_o[0] in (1, 2, 4))):   # (in-launch K reduction)
                sc, ctr = self._ks_buffers(hid)
                n.gemm_skinny_ks(self._w16(lw, "wo", True), ah, al, T, hid, H * D, x, hid, self.ks_o[1], self.ks_o[0], sc, ctr, rows_dev=rows_dev)
            else:
                n.gemm_skinny(self._w16(lw, "wo", True), ah, al, T, hid, H * D, n.EPI_ADD, y=x, ldy=hid, wscale=lw["wo_s"], rows_dev=rows_dev)  # x += attn @ Wo^T
            n.gemm_skinny_norm(self._w16(lw, "wgu", True), x, lw["ln2"], eps, T, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl,
                               wscale=lw["wgu_s"], rows_dev=rows_dev)
            if self.ks_down and lw["wdown_s"] is None and self.ks_min_rows <= T <= 32 and (T <= 16 or (self.ks_down[1] <= 4 and self.ks_down[0] in (1, 2, 4))) and inter >= 2 * hid:
                sc, ctr = self._ks_buffers(hid)
                n.gemm_skinny_ks(self._w16(lw, "wdown", True), ch, cl, T, hid, inter, x, hid, self.ks_down[1], self.ks_down[0], sc, ctr, rows_dev=rows_dev)
            else:
                n.gemm_skinny(self._w16(lw, "wdown", True), ch, cl, T, hid, inter, n.EPI_ADD, y=x, ldy=hid, wscale=lw["wdown_s"], rows_dev=rows_dev)  # x += act @ Wd^T
        if last_token_only:
            xs = x.view(B, q_len, hid)[:, -1, :].contiguous()
            logits = torch.empty((B, V), dtype=torch.float32, device=self.device)
            n.gemm_skinny_norm(self.lm_head_f, xs, self.norm, eps, B, V, hid, n.EPI_STORE, y=logits, ldy=V)
            return logits.view(B, 1, V)
        logits = torch.empty((T, V), dtype=torch.float32, device=self.device)
        n.gemm_skinny_norm(self.lm_head_f, x, self.norm, eps, T, V, hid, n.EPI_STORE, y=logits, ldy=V, rows_dev=rows_dev)
        return logits.view(B, q_len, V)

    # rows a captured small-q graph is padded to (B = 1, q > 1): a prompt of q new tokens replays the graph of its bucket with
    # pad tokens BEHIND its own (under the causal mask nothing reaches back from them; their K/V rows lie past the arena's
    # length and are overwritten by the first decode steps), so a question length seen for the first time does not pay an
    # eager pass + capture (cold-shape TTFT 9.5-10.7 ms against ~4 ms warm) as long as its bucket was seen.  0 = exact q.
    # The projections read the number of LIVE rows from a device word next to past_len (pc_gemm rows_dev) and do not load the
    # pad rows' activations, so one graph per row tile (16) costs the 12-row headline prompt nothing measurable.
    graph_row_bucket = int(os.environ.get("PC_GRAPH_BUCKET", "16"))

    def _graph_rows(self, arena, B: int, q_len: int, past_len: int, last_token_only: bool) -> int:
        g = self.graph_row_bucket
        if g <= 1 or B != 1 or q_len == 1 or last_token_only or self.llm_int8 or self.use_chain:
            return q_len          # (LLM.int8 picks its outlier columns over all rows of a call: no pad rows there)
        qb = (q_len + g - 1) // g * g
        if qb > (self.MID_MAX_ROWS if self.graph_mid else self.SKINNY_MAX_ROWS) or past_len + qb > arena.cap:
            return q_len
        if (qb + 15) // 16 != (q_len + 15) // 16 or (q_len <= 32) != (qb <= 32):
            return q_len          # never across a row-tile count or the residual-tail regime of the attention
        return qb

    def _gather_ok(self, arena, B: int, q_len: int, past_len: int, num_layers: Optional[int] = None) -> bool:
        """Will the attention launches of this (bucketed) forward run on the kernel that stages while it reads?  Asked of the
        library itself (pc_attn_gather_ok) with the arguments _forward_skinny passes; the answer only depends on the row count,
        the residual mode and whether the key range reaches the streaming kernel's minimum, so it is remembered."""
        plan = arena.pending
        if plan is None or plan.total != past_len or len(plan.segs) > self.GATHER_MAX_SEG:
            return False
        if num_layers is not None and num_layers < self.L:
            return False      # a partial-depth forward would stage only its own layers' planes: materialise the whole plan instead
        return self._gather_shape_ok(arena, B, q_len, past_len)

    def _gather_shape_ok(self, arena, B: int, q_len: int, past_len: int) -> bool:
        if not self.supports_fused_gather or B != 1 or self.use_chain or past_len <= 0:
            return False
        ck = (q_len, self._lo_mode, past_len + q_len >= 256)
        ok = self._gather_ok_cache.get(ck)
        if ok is None:
            buf = arena.buf
            kvlo = (arena.tail_planes(0) + (-1,)) if self._lo_mode == 1 else None
            H, D = self.H, self.D
            ok = _native.attn_gather_ok(buf, q_len * H * D, H * D, arena.k_plane(0), arena.v_plane(0), arena.batch_stride,
                                        arena.head_stride, None, 0, 0, B, H, self.Hkv, D, q_len, past_len, self.softmax_scale,
                                        None, past_len_dev=buf, out_frag=(buf, buf), q_lo=buf, kv_lo=kvlo)
            self._gather_ok_cache[ck] = ok
        return ok

    def _nsplit_key(self, B: int, q_len: int, kv_len: int) -> int:
        k = (B, q_len, kv_len)
        v = self._nsplit_cache.get(k)
        if v is None:
            if len(self._nsplit_cache) > 4096:
                self._nsplit_cache.clear()
            v = self._nsplit_cache[k] = _native.attn_workspace_bytes(B, self.H, self.D, q_len, kv_len)   # monotone in the split count
        return v

    def _graph_key(self, arena, B, q_len, past_len, last_token_only, num_layers, gather):
        mode = self._lo_mode
        tail = arena.tail_lo if mode else None
        # (a staging forward captures the address of the arena's row table as well: a NEW arena that happens to land on the freed
        # buffer address of an old one must not replay a graph that writes through the old arena's freed row table)
        return (B, q_len, arena.buf.data_ptr(), arena.cap, self._nsplit_key(B, q_len, past_len + q_len), bool(last_token_only), num_layers,
                self.fuse_norm, self.use_chain, mode, tail.data_ptr() if mode else 0, tail.shape[4] if mode else 0,
                arena.row_table().data_ptr() if gather else 0)

    def _graph_entry(self, key, arena, B, q_len, past_len, last_token_only, num_layers, gather, eager_first=True):
        """The captured forward for ``key`` -> ``[graph, input block, logits buffer]`` (captured now when it does not exist yet:
        the block's host side must already hold valid inputs; ``eager_first`` runs the forward once before capturing)."""
        ent = self._graphs.pop(key, None)
        if ent is not None:
            self._graphs[key] = ent                          # LRU: a hit moves the entry to the young end
            return ent, False
        n = _native
        T = B * q_len
        if len(self._graphs) >= self.max_graphs:
            self._graphs.pop(next(iter(self._graphs)))       # evict the least recently used
        if T > self.SKINNY_MAX_ROWS:
            # the captured 65..512-row forwards hold their slabs and planes in the graph's pool (a few hundred MB each): a handful
            big = [k for k in self._graphs if isinstance(k[0], int) and k[0] * k[1] > self.SKINNY_MAX_ROWS]
            if len(big) >= self.max_mid_graphs:
                self._graphs.pop(big[0])
        blk = _InputBlock(self.device, T, self.GATHER_MAX_SEG if gather else 0)
        ent = [None, blk, None]
        self._graphs[key] = ent
        return ent, True

    def _fused_pro(self) -> bool:
        """Does a captured forward of this model start with pc_prefill_prologue (one launch: block fetch, embedding, rotation
        table, row table)?"""
        return self.fused_prologue and type(self)._forward_skinny is LlamaHIP._forward_skinny and not self.llm_int8

    def _capture(self, ent, arena, B, q_len, past_len, last_token_only, num_layers, gather, eager_first=True):
        n = _native
        blk = ent[1]

        fused_pro = self._fused_pro()

        def run():
            if fused_pro:
                # ONE launch: block fetch + embedding rows (fp32 residual stream) + rotation table + row table
                T = B * q_len
                x = torch.empty((T, self.config.hidden_size), dtype=torch.float32, device=self.device)
                cs = torch.empty((T, self.D // 2, 2), dtype=torch.float32, device=self.device)
                n.prefill_prologue(blk.host, blk.dev, blk.nbytes, T, blk.o_pos, blk.o_words, blk.o_segs, blk.max_seg, self.embed,
                                   self.config.hidden_size, self.config.vocab_size, x, self.inv_freq, self.D, cs,
                                   rows=arena.row_table() if gather else None, dst=arena.buf if gather else None,
                                   max_ctx=arena.cap if gather else 0)
                self._pre = (x, cs)
            else:
                blk.fetch()
                if gather:
                    n.kv_row_table(blk.segs, blk.words[3:4], self.GATHER_MAX_SEG, blk.words[4:5], arena.buf, self.Hkv, self.D, arena.cap,
                                   arena.row_table())
            if gather:
                self._gather = arena.row_tab
            try:
                return self._forward_skinny(blk.ids, blk.pos, blk.words, arena, B, q_len, past_len, last_token_only, num_layers)
            finally:
                self._gather = None
                self._pre = None

        if eager_first:
            # one eager pass first (loads code objects / sizes the allocator), then capture
            run()
            torch.cuda.synchronize()
        prime_graph_capture(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run()
        ent[0], ent[2] = g, out

    def _graphed_skinny(self, ids, pos, arena, B, q_len, past_len, last_token_only, num_layers):
        """Replay (capturing on first use) the hipGraph of the small-q forward for this shape.  ``ids`` / ``pos``: flat integer
        tensors; host tensors are the fast path (device tensors -- the reference's calling convention -- are read back first)."""
        q_real = q_len
        q_len = self._graph_rows(arena, B, q_len, past_len, last_token_only)
        if q_len != q_real:
            self._lo_mode = self._tail_mode(arena, q_len, past_len)
        gather = self._gather_ok(arena, B, q_len, past_len, num_layers)
        plan = arena.pending if gather else None
        if not gather:
            arena.materialize()
        mode = self._lo_mode
        key = self._graph_key(arena, B, q_len, past_len, last_token_only, num_layers, gather)
        ent, fresh = self._graph_entry(key, arena, B, q_len, past_len, last_token_only, num_layers, gather)
        T = B * q_len
        blk = ent[1]
        # ---- this call's inputs: written into the pinned block the graph's first node fetches ----
        blk.acquire()
        n_real = q_real * B
        w = blk.h_words
        dev_in = ids.is_cuda or pos.is_cuda
        if dev_in and self._fused_pro():
            # device inputs (the reference's calling convention, generation_engine.py:96-97): copied into the device twin's
            # ids | pos region on this stream; the prologue reads them there (words[5]) -- no read-back, no host sync
            blk.ids[:n_real].copy_(ids, non_blocking=True)
            blk.pos[:n_real].copy_(pos, non_blocking=True)
            if q_len != q_real:                              # pad rows BEHIND the prompt's own (see _graph_rows)
                blk.ids[n_real:].zero_()
                blk.pos[n_real:] = blk.pos[n_real - 1] + torch.arange(1, T - n_real + 1, dtype=torch.int32, device=self.device)
            w[5] = 1
        else:
            if dev_in:                                       # (stacks without the fused prologue: correct, one read-back)
                ids, pos = ids.cpu(), pos.cpu()
            blk.h_ids[:n_real] = ids.numpy()
            blk.h_pos[:n_real] = pos.numpy()
            if q_len != q_real:                              # pad rows BEHIND the prompt's own (see _graph_rows)
                blk.h_ids[n_real:] = 0
                blk.h_pos[n_real:] = int(blk.h_pos[n_real - 1]) + np.arange(1, T - n_real + 1, dtype=np.int32)
            w[5] = 0
        w[0] = past_len
        w[1] = arena.tail_base if mode == 2 else 0
        w[2] = n_real                                        # rows that carry tokens: the projections do not load the pad rows' activations
        w[4] = min(past_len + q_len, arena.cap)              # rows of the row table (this pass's own rows: entries that point at the arena)
        if gather:
            w[3] = len(plan.segs)
            blk.h_segs[:len(plan.segs)] = plan.seg_array(_SEG_DTYPE)
        if fresh:
            try:
                self._capture(ent, arena, B, q_len, past_len, last_token_only, num_layers, gather)
            except BaseException:
                self._graphs.pop(key, None)                  # no half-built entry: the next call captures again
                raise
        g, out = ent[0], ent[2]
        g.replay()
        blk.release()
        if gather:
            arena.pending = None                             # the staged rows are in the arena now
            self.stats["fused_gather"] += 1
        res = out[:, :q_real].clone() if q_len != q_real else out.clone()
        if fresh and self.prewarm_tiles and B == 1 and q_real > 1 and T <= self.SKINNY_MAX_ROWS and not last_token_only:
            self._prewarm(arena, past_len + q_real, num_layers)
        return res

    # Capture the sibling row tiles of a prompt-sized forward as soon as the first one is captured: a question whose tile count
    # (16 / 32 / 48 / 64 rows) is new then replays instead of paying an eager pass + capture on its own TTFT (cold-shape TTFT
    # 14.7 ms against 4.7 ms warm in round 3).  Capture only -- nothing is executed, so the arena and the residual tail are not
    # touched; the host spends ~5 ms per tile, once per arena, behind the replay of the request that triggered it.
    prewarm_tiles = os.environ.get("PC_PREWARM_TILES", "1") != "0"

    def _prewarm(self, arena, past_len: int, num_layers) -> None:
        if self.llm_int8 or self.use_chain or self.graph_row_bucket != 16 or self.decode_tail:
            return
        saved = self._lo_mode
        try:
            for q in (16, 32, 48, 64):
                if past_len + q > arena.cap:
                    break
                self._lo_mode = self._tail_mode(arena, q, past_len)
                # both ways a prompt of this tile may arrive: rows already staged, or a staging plan for the attention to carry out
                for gather in ((False, True) if self._gather_shape_ok(arena, 1, q, past_len) else (False,)):
                    key = self._graph_key(arena, 1, q, past_len, False, num_layers, gather)
                    if key in self._graphs:
                        continue
                    ent, fresh = self._graph_entry(key, arena, 1, q, past_len, False, num_layers, gather)
                    if fresh:
                        try:
                            self._capture(ent, arena, 1, q, past_len, False, num_layers, gather, eager_first=False)
                        except Exception:                       # a capture that cannot be taken cold is simply taken on first use
                            self._graphs.pop(key, None)
                            self.prewarm_tiles = False
                            return
        finally:
            self._lo_mode = saved

    @torch.inference_mode()
    def _loop_state(self) -> dict:
        """Device words shared by every captured decode-loop graph of this model: token id, position id, {past length,
        residual-tail base}, the token ring and its counter (see GreedyLoop)."""
        st = getattr(self, "_loop_st", None)
        if st is None:
            st = self._new_loop_state(GreedyLoop.RING)
            self._loop_st = st
        return st

    def _new_loop_state(self, ring: int) -> dict:
        dev = self.device
        return dict(ids=torch.zeros(1, dtype=torch.int64, device=dev), pos=torch.zeros(1, dtype=torch.int32, device=dev),
                    past=torch.zeros(2, dtype=torch.int32, device=dev), ring=torch.zeros(ring, dtype=torch.int32, device=dev),
                    ctr=torch.zeros(1, dtype=torch.int32, device=dev),
                    # pc_sample_advance's parameter block (pc_sample_params) and history bitmap
                    params=torch.zeros(ctypes.sizeof(_native.SampleParams), dtype=torch.uint8, device=dev),
                    hist=torch.zeros((self.config.vocab_size + 31) // 32, dtype=torch.int32, device=dev))

    def _sample_state_fill(self, st: dict, params, seed: int, history_ids) -> None:
        """Parameter block and history bitmap of a sampled generation into the state ``st`` (ordered on the current stream)."""
        blk = sample_params_block(params, seed)
        st["params"].copy_(torch.frombuffer(bytearray(blk), dtype=torch.uint8))
        st["bits" if "bits" in st else "hist"].copy_(_history_bits(history_ids, self.config.vocab_size))

    @torch.inference_mode()
    def sample_token(self, logits_row: torch.Tensor, params, seed: int, history_ids, step: int = 0) -> int:
        """One eager draw of pc_sample_advance from a [vocab] fp32 row (the prefill's last row), at ``step`` of the random
        stream of ``seed``, on a scratch state of its own (the device loop's words are not touched)."""
        V = self.config.vocab_size
        assert logits_row.dtype == torch.float32 and logits_row.numel() == V and logits_row.stride(-1) == 1
        st = getattr(self, "_draw_st", None)
        if st is None:
            st = self._draw_st = self._new_loop_state(1)
        self._sample_state_fill(st, params, seed, history_ids)
        st["ctr"].fill_(step)
        _native.sample_advance(logits_row, V, st["params"], st["hist"], st["ids"], st["pos"], st["past"], st["ring"], st["ctr"])
        return int(st["ids"][0])

    # ---- per-token log-probabilities (pc_token_logprobs) -----------------------------------------------------
    def _lp_state(self, tag: tuple, rows: int, top_n: int) -> dict:
        """The fixed output buffers of a step's log-probability node: ``ids`` int32 / ``lp`` fp32 ``[rows][1 + top_n]``, one pair
        per (loop state ``tag``, rows, top_n) -- the captured steps hold their addresses, and the graph keys carry ``top_n``."""
        sts = self.__dict__.setdefault("_lp_sts", {})
        st = sts.get((tag, rows, top_n))
        if st is None:
            dev = self.device
            if not sts:
                # first launch of the kernel outside any capture (code-object load): stateless, on a scratch row of zeros
                V = self.config.vocab_size
                _native.token_logprobs(torch.zeros(V, dtype=torch.float32, device=dev), V, V, 1, torch.zeros(1, dtype=torch.int64, device=dev),
                                       1, 0, torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev))
            st = sts[(tag, rows, top_n)] = dict(ids=torch.full((rows, 1 + top_n), -1, dtype=torch.int32, device=dev),
                                                lp=torch.full((rows, 1 + top_n), float("nan"), dtype=torch.float32, device=dev))
        return st

    def _lp_node(self, lp: dict, logits, rows: int, tokens, stride: int, top_n: int) -> None:
        """The node: the log-softmax of the RAW ``logits`` rows the sampler just read (it leaves them untouched: no step hands it a
        ``processed_out``) at the tokens its last node left in ``tokens``, into the fixed buffers ``lp``."""
        V = self.config.vocab_size
        _native.token_logprobs(logits, V, V, rows, tokens, stride, top_n, lp["ids"], lp["lp"])

    @torch.inference_mode()
    def token_logprobs(self, logits_rows: torch.Tensor, tokens, top_n: int) -> list:
        """One eager launch of pc_token_logprobs on rows the caller already has (``[vocab]`` or ``[R][vocab]`` logits, ``tokens``: one
        id per row) -> host records ``[(token, logprob, [(id, logprob)] * top_n)]``.  The log-probabilities are the model's own: the
        log-softmax of the raw logits, before temperature, repetition penalty, top-p and top-k.  The first token of a generation
        (the prefill's last row) and the stepped paths come through here."""
        top_n = check_logprobs(int(top_n))
        V = self.config.vocab_size
        x = logits_rows.reshape(-1, logits_rows.shape[-1])
        if x.shape[1] != V:
            raise ValueError(f"token_logprobs: rows of {x.shape[1]} logits, vocab_size = {V}")
        if not x.is_cuda or x.dtype != torch.float32 or x.stride(1) != 1:
            x = x.to(device=self.device, dtype=torch.float32).contiguous()
        toks = torch.as_tensor([int(t) for t in tokens], dtype=torch.int64).to(x.device)
        if toks.numel() != x.shape[0]:
            raise ValueError(f"token_logprobs: {toks.numel()} tokens for {x.shape[0]} rows")
        out = []
        for r0 in range(0, x.shape[0], 64):
            r = min(64, x.shape[0] - r0)
            ids = torch.empty((r, 1 + top_n), dtype=torch.int32, device=x.device)
            lp = torch.empty((r, 1 + top_n), dtype=torch.float32, device=x.device)
            _native.token_logprobs(x[r0:], x.stride(0), V, r, toks[r0:], 1, top_n, ids, lp)
            out += logprob_records(ids.cpu(), lp.cpu())
        return out

    # ---- token controls (pc_logit_adjust) ------------------------------------------------------------------------
    def _ctl_state(self, tag: tuple, S: int, rows_per_slot: int) -> dict:
        """The state of a step's token-control node, one per (loop state ``tag``, S, rows per slot): ``ctl`` -- S ``pc_logit_ctl``
        blocks, ``allowed`` -- int32 ``[S][ceil(V / 32)]``, and ``out``, the fixed fp32 ``[S * rows_per_slot][ldo]`` buffer of adjusted
        rows that the step's advance / verify launch reads (``ldo``: V rounded up to 4).  The captured steps hold the addresses."""
        sts = self.__dict__.setdefault("_ctl_sts", {})
        st = sts.get((tag, S, rows_per_slot))
        if st is None:
            dev, V = self.device, self.config.vocab_size
            ldo, nb = (V + 3) & ~3, ctypes.sizeof(_native.LogitCtl)
            st = dict(ctl=torch.zeros(S * nb, dtype=torch.uint8, device=dev), allowed=torch.zeros((S, (V + 31) // 32), dtype=torch.int32, device=dev),
                      out=torch.zeros((S * rows_per_slot, ldo), dtype=torch.float32, device=dev), ldo=ldo, S=S, rows=rows_per_slot)
            if not sts:
                # first launch of the kernel outside any capture (code-object load): stateless, on zeroed rows under neutral blocks
                _native.logit_adjust(torch.zeros((S * rows_per_slot, V), dtype=torch.float32, device=dev), V, V, S, rows_per_slot,
                                     st["ctl"], st["allowed"], None, st["out"], ldo)
            sts[(tag, S, rows_per_slot)] = st
        return st

    def _ctl_pinned(self) -> torch.Tensor:
        """A pinned host buffer for one slot's image: the ``pc_logit_ctl`` block, then the allowed row."""
        return torch.zeros(ctypes.sizeof(_native.LogitCtl) + 4 * ((self.config.vocab_size + 31) // 32), dtype=torch.uint8, pin_memory=True)

    def _ctl_fill(self, cs: dict, s: int, controls, len_at_entry: int, pinned: Optional[torch.Tensor] = None) -> None:
        """Slot ``s`` of the node state ``cs`` takes the image of ``controls`` (None: the neutral block) for a sequence that enters
        with ``len_at_entry`` arena rows: row ``(s, i)`` of a step at arena length ``len`` draws generated token number
        ``len - len_at_entry + 1 + i``, so the stop ids are held back while ``len + i < len_at_entry + min_new_tokens - 1``.  Two
        copies ordered on the current stream; ``pinned`` (``_ctl_pinned``; the caller keeps it until they have run) for a loop that
        is replaying."""
        V, nb = self.config.vocab_size, ctypes.sizeof(_native.LogitCtl)
        free = 0 if controls is None else len_at_entry + controls.min_new_tokens - 1
        blk, bits = logit_ctl_image(controls, V, free)
        host = torch.zeros(nb + 4 * cs["allowed"].shape[1], dtype=torch.uint8) if pinned is None else pinned
        arr = host.numpy()
        arr[:nb] = np.frombuffer(blk, dtype=np.uint8)
        arr[nb:].view(np.uint32)[:] = 0 if bits is None else bits
        cs["ctl"][s * nb:(s + 1) * nb].copy_(host[:nb], non_blocking=pinned is not None)
        cs["allowed"][s].view(torch.uint8).copy_(host[nb:], non_blocking=pinned is not None)

    def _ctl_node(self, cs: dict, logits, ldl: int, S: int, rows_per_slot: int, length) -> None:
        """The node: the adjusted copy of the step's raw ``logits`` rows into ``cs["out"]`` under the slots' blocks and the arena
        lengths in ``length`` (int32 device words: ``past`` of a single-sequence loop, ``len`` of a slot loop)."""
        _native.logit_adjust(logits, ldl, self.config.vocab_size, S, rows_per_slot, cs["ctl"], cs["allowed"], length, cs["out"], cs["ldo"])

    @torch.inference_mode()
    def adjust_logits(self, logits_row: torch.Tensor, controls, generated: int = 0) -> torch.Tensor:
        """One eager launch of pc_logit_adjust on a row the caller already has (``[vocab]`` logits, any float dtype) -> the adjusted
        fp32 ``[vocab]`` row under ``controls`` for generated token number ``generated`` (0: the token drawn from the prefill): the
        stop ids are ``-inf`` while ``generated < min_new_tokens``.  The first token of a generation and the host-stepped paths
        come through here, in front of their argmax / sampler.  ``controls`` None: the row itself."""
        if controls is None:
            return logits_row
        V = self.config.vocab_size
        if logits_row.numel() != V:
            raise ValueError(f"adjust_logits: a row of {logits_row.numel()} logits, vocab_size = {V}")
        x = logits_row.reshape(V)
        if not x.is_cuda or x.dtype != torch.float32 or x.stride(0) != 1:
            x = x.to(device=self.device, dtype=torch.float32).contiguous()
        cs = self._ctl_state(("eager",), 1, 1)
        blk, bits = logit_ctl_image(controls, V, controls.min_new_tokens - int(generated))     # (len reads as 0)
        ctl = torch.frombuffer(bytearray(blk), dtype=torch.uint8).to(x.device)
        allowed = None if bits is None else torch.from_numpy(bits.view(np.int32).copy()).to(x.device)
        out = torch.empty(cs["ldo"], dtype=torch.float32, device=x.device)
        _native.logit_adjust(x, V, V, 1, 1, ctl, allowed, None, out, cs["ldo"])
        return out[:V]

    def _loop_graph(self, arena: KVArena, past_len: int, sample: bool = False, logprobs: Optional[int] = None, ctl=None):
        """The captured graph of ONE greedy (``sample``: sampled) decode step over ``arena`` (forward of the token in the loop
        state + argmax / draw + state advance), keyed like ``_graphed_skinny``.  ``logprobs`` = n: one more node behind the advance
        (the key gains ``("logprobs", n)``; None: today's key and launches)."""
        n = _native
        nsplit_key = n.attn_workspace_bytes(1, self.H, self.D, 1, past_len + 1)
        mode = self._lo_mode
        key = ("loop",) + (("sample",) if sample else ()) + (arena.buf.data_ptr(), arena.cap, nsplit_key, self.fuse_norm, self.use_chain, mode,
               arena.tail_lo.data_ptr() if mode else 0, arena.tail_lo.shape[4] if mode else 0)
        lp = None
        if logprobs is not None:
            key += ("logprobs", logprobs)
            lp = self._lp_state(("loop",), 1, logprobs)
        if ctl is not None:               # one more node in front of the advance, which then reads the adjusted row
            key += ("ctl",)
        ent = self._graphs.pop(key, None)
        if ent is not None:
            self._graphs[key] = ent
            return ent
        if len(self._graphs) >= self.max_graphs:
            self._graphs.pop(next(iter(self._graphs)))
        st = self._loop_state()
        st["past"][0:1].fill_(past_len)
        if mode == 2:
            st["past"][1:2].fill_(arena.tail_base)
        V = self.config.vocab_size
        # one eager pass first (loads code objects / sizes the allocator): it rewrites the K / V row the first replay
        # writes again and does not touch the loop state
        self._forward_skinny(st["ids"], st["pos"], st["past"], arena, 1, 1, past_len, False, None)
        torch.cuda.synchronize()
        prime_graph_capture(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = self._forward_skinny(st["ids"], st["pos"], st["past"], arena, 1, 1, past_len, False, None)
            row = out
            if ctl is not None:
                self._ctl_node(ctl, out, V, 1, 1, st["past"])
                row = ctl["out"]
            if sample:
                n.sample_advance(row, V, st["params"], st["hist"], st["ids"], st["pos"], st["past"], st["ring"], st["ctr"])
            else:
                n.greedy_advance(row, V, st["ids"], st["pos"], st["past"], st["ring"], st["ctr"])
            if lp is not None:
                self._lp_node(lp, out, 1, st["ids"], 1, logprobs)
        ent = (g, out)
        self._graphs[key] = ent
        return ent

    def _loop_arena(self, past) -> Optional[KVArena]:
        if not (self.skinny and self.use_graphs and self.supports_greedy_loop):
            return None
        found = arena_from_past(past, self.L, self.Hkv, self.D)
        if found is None or found[0].B != 1:
            return None
        arena, S = found
        arena.length = S
        return arena

    def can_loop(self, past) -> bool:
        """Whether ``greedy_loop`` / ``sample_loop`` over ``past`` would give a loop (not None)."""
        return self._loop_arena(past) is not None

    def greedy_loop(self, past, token: int, position: int, max_new: int, logprobs: Optional[int] = None,
                    token_controls=None) -> Optional["GreedyLoop"]:
        """A device-side greedy decode loop over the arena behind ``past`` (None when this model / cache cannot host one:
        the caller then steps through ``__call__``).  ``logprobs`` = n in 0..8: every step also leaves the log-probability of its
        token and of the n most likely ones under the raw logits (``GreedyLoop.logprobs``); all device loops take it.
        ``token_controls`` (a ``TokenControls``): the step gains ``pc_logit_adjust`` in front of the advance, which then
        takes the argmax of the adjusted row; all device loops take it too.  None: today's graph keys and launches."""
        arena = self._loop_arena(past)
        return None if arena is None else GreedyLoop.with_controls(token_controls, self, arena, token, position, max_new, logprobs=logprobs)

    def sample_loop(self, past, token: int, position: int, max_new: int, params, seed: int, history_ids,
                    logprobs: Optional[int] = None, token_controls=None) -> Optional["SampleLoop"]:
        """A device-side sampled decode loop (``params``: temperature, repetition_penalty, top_p, top_k as in
        GenerationParameters; ``history_ids``: the ids the repetition penalty sees, ``token`` included) over the arena
        behind ``past``, continuing the random stream of ``seed`` at step 1.  None where ``greedy_loop`` gives None."""
        arena = self._loop_arena(past)
        return None if arena is None else SampleLoop.with_controls(token_controls, self, arena, token, position, max_new, params, seed,
                                                                   history_ids, logprobs)

    # ---- prompt-lookup speculative decoding (LookupLoop) ----------------------------------------------------------------
    def lookup_available(self) -> bool:
        """Whether this model runs ``LookupLoop``: the Llama layer loop over fp16 weight images, default decode precision (no
        residual tail through decode).  Everything else (Falcon, MPT, int8 weights, PC_DECODE_TAIL=1) keeps ``GreedyLoop``."""
        return bool(self.skinny and self.use_graphs and self.supports_greedy_loop and not self.int8_weights and
                    not self.llm_int8 and not self.decode_tail and not self.use_chain and
                    type(self)._forward_skinny is LlamaHIP._forward_skinny)

    @torch.inference_mode()
    def _lookup_state(self, hist_need: int) -> dict:
        """Device words of the lookup loop (one set per model: the newest loop owns it, as with ``_loop_state``).  The history
        buffer grows in powers of two; a captured step holds its address, so the graph key carries it (and the entry keeps the
        buffer alive)."""
        st = getattr(self, "_lookup_st", None)
        dev = self.device
        if st is None:
            R = LookupLoop.ROWS_MAX
            st = self._lookup_st = dict(
                ids=torch.zeros(R, dtype=torch.int64, device=dev), pos=torch.zeros(R, dtype=torch.int32, device=dev),
                past=torch.zeros(2, dtype=torch.int32, device=dev), ndraft=torch.zeros(1, dtype=torch.int32, device=dev),
                budget=torch.zeros(1, dtype=torch.int32, device=dev), hist_len=torch.zeros(1, dtype=torch.int32, device=dev),
                ctr=torch.zeros(1, dtype=torch.int32, device=dev), amax=torch.zeros(R, dtype=torch.int32, device=dev),
                ring=torch.zeros(LookupLoop.RING * (R + 1), dtype=torch.int32, device=dev), hist=None)
            # first launches of the two kernels outside any capture (code-object load), on words that hold zeros:
            # budget 0 -> an empty record in ring[0], nothing else changes
            warm = torch.zeros(1, dtype=torch.int32, device=dev)
            _native.lookup_draft(warm, st["hist_len"], st["ids"], st["pos"], st["ndraft"], 1, 1)
            _native.lookup_verify(torch.zeros(16, dtype=torch.float32, device=dev), 16, 16, 1, st["amax"], warm, st["hist_len"],
                                  st["ids"], st["pos"], st["past"], st["ndraft"], st["budget"], st["ring"], st["ctr"], LookupLoop.RING)
        if st["hist"] is None or st["hist"].numel() < hist_need:
            cap = 8192
            while cap < hist_need:
                cap *= 2
            st["hist"] = torch.zeros(cap, dtype=torch.int32, device=dev)
        return st

    @torch.inference_mode()
    def _lookup_sample_state(self, st: dict) -> None:
        """What ``SampleLookupLoop`` adds to the lookup state ``st``, once per model: pc_lookup_verify_sample's parameter block,
        history bitmap (``bits``: ``hist`` is the token history here), ``draws`` word and per-row scratch."""
        if "bits" in st:
            return
        dev, R = self.device, LookupLoop.ROWS_MAX
        V = self.config.vocab_size
        hw = (V + 31) // 32
        st.update(params=torch.zeros(ctypes.sizeof(_native.SampleParams), dtype=torch.uint8, device=dev),
                  bits=torch.zeros(hw, dtype=torch.int32, device=dev), draws=torch.zeros(1, dtype=torch.int32, device=dev),
                  row_bits=torch.zeros(R * hw, dtype=torch.int32, device=dev), row_token=torch.zeros(R, dtype=torch.int32, device=dev))
        # first launch of the kernels outside any capture, as in _lookup_state: zeroed words, budget 0 -> an empty record
        warm = torch.zeros(1, dtype=torch.int32, device=dev)
        zero = {n: torch.zeros_like(st[n]) for n in ("hist_len", "ids", "pos", "past", "ndraft", "budget", "ctr")}
        _native.lookup_verify_sample(torch.zeros(V, dtype=torch.float32, device=dev), V, V, 1, st["params"], st["bits"],
                                     st["row_bits"], st["draws"], st["row_token"], warm, zero["hist_len"], zero["ids"], zero["pos"],
                                     zero["past"], zero["ndraft"], zero["budget"], torch.zeros(2, dtype=torch.int32, device=dev),
                                     zero["ctr"], 1)

    def _lookup_graph(self, loop: "LookupLoop"):
        """The captured graph of ONE lookup step of ``loop`` (draft + ``k + 1``-row forward + verify), one per key."""
        arena, st, k = loop.arena, loop.st, loop.k
        key = ("loop", "lookup", k, arena.buf.data_ptr(), arena.cap, self._nsplit_key(1, k + 1, loop.kv_ceiling), loop.kv_ceiling,
               loop.nmax, st["hist"].data_ptr(), st["hist"].numel(), self.fuse_norm) + loop.graph_tag
        if loop.lp_n is not None:
            key += ("logprobs", loop.lp_n)
        if loop._cs is not None:
            key += ("ctl",)
        ent = self._graphs.pop(key, None)
        if ent is not None:
            self._graphs[key] = ent
            return ent
        if len(self._graphs) >= self.max_graphs:
            self._graphs.pop(next(iter(self._graphs)))
        # one eager pass of the forward first (loads code objects / sizes the allocator): it writes K / V rows [past, past + k],
        # which the first replay writes again, reads whatever valid ids the draft rows hold, and does not touch the loop state
        self._forward_skinny(st["ids"][:k + 1], st["pos"][:k + 1], st["past"], arena, 1, k + 1, loop.kv_ceiling - (k + 1), False, None)
        torch.cuda.synchronize()
        prime_graph_capture(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = loop._step()
        ent = (g, out, st["hist"])
        self._graphs[key] = ent
        return ent

    def lookup_loop(self, past, token: int, position: int, max_new: int, k: int, corpus_ids, nmax: int = 3, params=None,
                    seed: int = 0, history_ids=None, logprobs: Optional[int] = None, token_controls=None):
        """A device-side greedy decode loop with prompt-lookup drafts (``LookupLoop``: up to ``k + 1`` tokens per step, ``k`` in
        1..15) over the arena behind ``past``.  ``corpus_ids``: the ids the drafts may copy from besides the output itself --
        the context in key order; the history starts as ``corpus_ids ++ [token]``.  ``max_new``: the most tokens the loop
        emits.  None where ``greedy_loop`` gives None; a plain ``GreedyLoop`` where the model has no lookup step
        (``lookup_available``).  With ``params`` (and ``seed`` / ``history_ids`` as in ``sample_loop``) the loop is the sampled one,
        ``SampleLookupLoop``: ``SampleLoop``'s tokens, up to ``k + 1`` per step; a ``SampleLoop`` where the model has no lookup
        step."""
        if params is not None:
            history_ids = [int(token)] if history_ids is None else history_ids
            if not self.lookup_available():
                return self.sample_loop(past, token, position, max_new, params, seed, history_ids, logprobs, token_controls)
            arena = self._loop_arena(past)
            return None if arena is None else SampleLookupLoop.with_controls(token_controls, self, arena, token, position, max_new, k,
                                                                             corpus_ids, params, seed, history_ids, nmax, logprobs)
        if not self.lookup_available():
            return self.greedy_loop(past, token, position, max_new, logprobs, token_controls)
        arena = self._loop_arena(past)
        return None if arena is None else LookupLoop.with_controls(token_controls, self, arena, token, position, max_new, k, corpus_ids,
                                                                   nmax, logprobs)

    # ---- batched decode over slots (SlotLoop) ---------------------------------------------------------------------------
    supports_slot_loop = True       # (a subclass with layer loops of its own says no)

    def slot_loop_available(self) -> bool:
        """Whether this model can host a ``SlotLoop``: the fp16 weight-streaming stack with folded norms, default decode
        precision (no residual tail through decode), head_dim 64 or 128."""
        return bool(self.supports_slot_loop and self.skinny and self.use_graphs and self.supports_greedy_loop and
                    not self.int8_weights and not self.llm_int8 and self.fuse_norm and not self.decode_tail and
                    not self.use_chain and self.D in (64, 128) and self.batch_invariant)

    def slot_trunk_q8_available(self) -> bool:
        """Whether ``slot_loop(each=True, kv="int8", trunks=...)`` runs: the slot loop, and head_dim 128
        (``pc_attn_decode_slots_trunk_q8``)."""
        return bool(self.slot_loop_available() and self.D == 128)

    def slot_loop(self, pasts, tokens, positions, max_new: int, params=None, seeds=None, histories=None, stop_ids=(),
                  slots: Optional[int] = None, slot_index=None, share_trunk: bool = False,
                  min_trunk: Optional[int] = None, each: bool = False, max_keys: Optional[int] = None,
                  trunks=None, kv: str = "fp16", keep_arenas: bool = True, logprobs: Optional[int] = None,
                  token_controls=None) -> Optional["SlotLoop"]:
        """A batched device-side decode loop over the arenas behind ``pasts`` (one ``past_key_values`` per sequence, each a
        batch-1 arena of its own): sequence k feeds ``tokens[k]`` at position ``positions[k]`` next.  ``params`` None or plain
        greedy: argmax; otherwise the sampled chain with ``seeds[k]`` (the stream continues at step 1) and ``histories[k]``.
        ``stop_ids``: up to 8 token ids that end a sequence on the device.  None where no batched loop is available -- the
        caller then decodes the sequences one after another.  ``share_trunk``: sequences whose arenas staged the same leading
        module rows (``kv_arena.common_trunks`` over ``KVArena.layout``; at least ``min_trunk`` rows, default
        ``PC_SLOT_TRUNK_MIN`` = 256) read those rows from one arena, once per step for the whole group
        (``pc_attn_decode_slots_trunk``); a batch without such a group runs the unshared step, bit for bit (``trunks``: the
        grouping, where the caller has worked it out already).
        ``each``: the step ends in ``pc_sample_advance_slots_each`` -- ``params``, ``max_new`` and ``stop_ids`` may then be lists
        with one entry per sequence, and ``SlotLoop.admit`` puts new sequences into slots whose sequence is over.
        ``max_keys``: the upper bound of keys the split counts of the attention are taken from (default: from this batch).  A
        serving loop passes the capacity of the slot buffers, once: a sequence's bits must not depend on who joins later, and the
        attention's summation order depends on the split counts.
        ``kv="int8"``: the loop keeps an int8 image (the format of ``pc_kv_quant_q8``) of every slot's rows and the
        attention reads that instead of the fp16 arena -- about half the bytes; accuracy is the format's.  The arenas stay
        complete (every decoded row is still appended), so memory GROWS by 0.516 of an arena per slot.  ``max_keys`` then also
        sizes the images.  head_dim 128 only: ``check_slot_kv`` raises ValueError.  With ``share_trunk`` / ``trunks`` and
        ``each=True`` (``slot_trunk_q8_available``): a group's shared rows are read once per step from the LEADER's
        image, every slot's rows behind them from its own (``pc_attn_decode_slots_trunk_q8``) -- equal fp16 rows give equal image
        rows, since ``pc_kv_quant_q8_rows`` is row-local; ``PC_TRUNK_VERIFY=1`` compares image rows [0, T) of member and leader
        byte for byte as a member enters.  Memory is unchanged: every member keeps its own copy.  With ``each=False``, and with
        ``keep_arenas=False``, the pair raises ValueError.
        ``keep_arenas=False`` (with ``kv="int8"`` only): the loop keeps the images and one fresh-row buffer per slot
        and NO reference to the arenas behind ``pasts`` -- their rows are quantised into the images on entry and the arenas are
        free afterwards (``SlotLoopQ8Only``); with ``each=True`` one arena can prefill every sequence in turn.
        ``logprobs`` = n in 0..8: the step gains one node behind the advance launch, ``pc_token_logprobs`` over the S
        logits rows at the tokens in ``ids[b]``; ``SlotLoop.logprobs(k, i)`` hands out the record of ``token(k, i)``.  None: today's
        graph keys, state and launches.
        ``token_controls``: the step gains ``pc_logit_adjust`` in front of the advance launch, which then reads the
        adjusted rows -- a ``TokenControls`` for every sequence, a list with one (or None) per sequence, or True: neutral blocks, the
        sequences bring theirs through ``admit(..., controls=...)``.  None: today's graph keys, state and launches."""
        check_logprobs(logprobs)
        check_slot_kv(kv, share_trunk=bool(share_trunk) or trunks is not None, head_dim=self.D,
                      no_loop=None if self.slot_loop_available() else "the model has no batched decode loop",
                      trunk_q8=bool(each) and getattr(self, "slot_trunk_q8_available", lambda: False)())
        check_slot_keep_arenas(keep_arenas, kv, share_trunk=bool(share_trunk) or trunks is not None)
        front = self._slot_loop_front(pasts, stop_ids, each, share_trunk, min_trunk, trunks)
        if front is None:
            return None
        arenas, trunks = front
        cls = (SlotLoopQ8 if keep_arenas else SlotLoopQ8Only) if kv == "int8" else SlotLoop
        return cls.with_options(logprobs, token_controls, self, arenas, tokens, positions, max_new, params, seeds, histories, stop_ids,
                                slots, slot_index, trunks, each, max_keys)

    def _slot_loop_front(self, pasts, stop_ids, each: bool, share_trunk: bool, min_trunk, trunks):
        """What ``slot_loop`` and ``lookup_slot_loop`` do before they build their loop -> (arenas, trunks), or None where there is
        no batched loop: the model has none, more than 16 sequences, more than 8 stop ids (of one sequence, with ``each``), a
        cache that is no batch-1 arena of its own."""
        per_seq_stops = each and len(stop_ids) and isinstance(stop_ids[0], (list, tuple))
        if not self.slot_loop_available() or not 1 <= len(pasts) <= SlotLoop.MAX_SLOTS or \
                (max(map(len, stop_ids)) if per_seq_stops else len(stop_ids)) > 8:
            return None
        arenas = []
        for past in pasts:
            a = self._loop_arena(past)
            if a is None or any(a is b for b in arenas):
                return None
            a.materialize()                       # (a staging no forward carried out yet)
            arenas.append(a)
        if trunks is None and share_trunk:
            trunks = common_trunks([a.layout for a in arenas], min_trunk)
        return arenas, trunks

    def _slot_nsplit(self, S: int, max_keys: int) -> int:
        """Splits of the key axis of pc_attn_decode_slots: enough workgroups to cover the chip at S slots, at least 256 keys
        per split at the longest length the loop can reach (a power of two, so that few graphs are captured)."""
        G = self.H // self.Hkv
        passes = 1 if G == 1 else (G + 3) // 4 if G <= 4 else (G + 7) // 8
        want = max(1, 1024 // max(1, S * self.Hkv * passes))
        ns = 1
        while ns < 32 and ns < want and ns * 2 * 256 <= max_keys:
            ns *= 2
        return ns

    def _slot_state(self, S: int) -> dict:
        """Device words of the S-slot decode step (one set per S: the captured steps hold their addresses)."""
        sts = self.__dict__.setdefault("_slot_sts", {})
        st = sts.get(S)
        if st is None:
            dev, V = self.device, self.config.vocab_size
            z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
            st = dict(kv_base=z(S, torch.int64), cap=z(S, torch.int32), len=z(S, torch.int32), pos=z(S, torch.int32),
                      ids=z(S, torch.int64), live=z(S, torch.int32), leader=torch.full((S,), -1, dtype=torch.int32, device=dev),
                      trunk=z(S, torch.int32), budget=z(S, torch.int32), ctr=z(S, torch.int32),
                      stop=torch.full((8,), -1, dtype=torch.int32, device=dev), seeds=z(S, torch.int64),
                      ring=z(S * SlotLoop.RING, torch.int32),
                      params=z(ctypes.sizeof(_native.SampleParams), torch.uint8), hist=z((S, (V + 31) // 32), torch.int32),
                      logits=z((S, V), torch.float32),
                      # per-slot sampling state of the each=True step (pc_sample_advance_slots_each)
                      params_each=z(S * ctypes.sizeof(_native.SampleParams), torch.uint8),
                      stop_each=torch.full((S, 8), -1, dtype=torch.int32, device=dev), draws=z(S, torch.int32))
            sts[S] = st
        return st

    def _slot_kvq(self, st: dict, S: int, need: int):
        """The int8 images of the S-slot step with ``kv="int8"``: one per slot index, ``qcap >= need`` rows per plane, and their
        addresses in ``st["kvq_base"]`` (int64[S], device data of the captured step).  Kept with the slot state and reused by
        later loops; they only grow.  -> (qcap, images)."""
        if st.get("kvq_cap", 0) < need:
            st["kvq"] = None                   # (the smaller images go first)
            nbytes = _native.kv_q8_image_bytes(int(need), self.L * 2 * self.Hkv, self.D)
            st["kvq"] = [torch.empty(nbytes, dtype=torch.uint8, device=self.device) for _ in range(S)]
            st["kvq_cap"] = int(need)
            if "kvq_base" not in st:
                st["kvq_base"] = torch.zeros(S, dtype=torch.int64, device=self.device)
            st["kvq_base"].copy_(torch.tensor([t.data_ptr() for t in st["kvq"]], dtype=torch.int64))
        return st["kvq_cap"], st["kvq"]

    def _slot_fresh(self, st: dict, S: int, rows: int = 1):
        """The fresh-row buffers of the S-slot step without arenas (``keep_arenas=False``): one per slot index, fp16
        ``[L * 2 * Hkv][D]`` -- the K / V row of the current step (the lookup step's (S, k) state: ``[L * 2 * Hkv][rows][D]``,
        ``rows = k + 1``).  Kept with the slot state."""
        if "fresh" not in st:
            shape = (self.L * 2 * self.Hkv, self.D) if rows == 1 else (self.L * 2 * self.Hkv, rows, self.D)
            st["fresh"] = [torch.zeros(shape, dtype=self.dtype, device=self.device) for _ in range(S)]
        return st["fresh"]

    def _slot_graph(self, S: int, nsplit: int, nsplit_trunk: int = 0, each: bool = False, qcap: int = 0, fresh: bool = False,
                    logprobs: Optional[int] = None, ctl=None):
        """The captured S-slot decode step.  Everything that changes from step to step or from batch to batch -- arena
        addresses included -- is read from the slot state, so one graph per (S, split count) serves every batch.
        ``nsplit_trunk`` > 0: the step with shared trunks; which slots share what is device data as well (leader / trunk).
        ``qcap`` > 0: the step over int8 images (``kv="int8"``); the image addresses are device data too, the key gains "q8" and
        the images' rows per plane, which is an argument of the launch.  ``fresh``: the step without arenas, which launches other
        entries: the key gains "fresh"."""
        key = ("slots", S, nsplit, "trunk", nsplit_trunk) if nsplit_trunk else ("slots", S, nsplit)
        if each:
            key += ("each",)
        if qcap:
            key += ("q8", qcap)
        if fresh:
            key += ("fresh",)
        more = {"fresh": True} if fresh else {}
        if logprobs is not None:          # one more node behind the advance launch: the key gains its top_n
            key += ("logprobs", logprobs)
            more["lp"] = (self._lp_state(("slots", S), S, logprobs), logprobs)
        if ctl is not None:               # one more node in front of the advance launch, which then reads the adjusted rows
            key += ("ctl",)
            more["ctl"] = ctl
        g = self._graphs.pop(key, None)
        if g is not None:
            self._graphs[key] = g
            return g
        if len(self._graphs) >= self.max_graphs:
            self._graphs.pop(next(iter(self._graphs)))
        st = self._slot_state(S)
        # one eager pass first (loads code objects / sizes the allocator) with every slot idle: it appends nothing and
        # advances nothing, the live words are put back behind it
        live = st["live"].clone()
        st["live"].zero_()
        self._forward_slots(st, S, nsplit, nsplit_trunk, each, qcap, **more)
        torch.cuda.synchronize()
        prime_graph_capture(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._forward_slots(st, S, nsplit, nsplit_trunk, each, qcap, **more)
        st["live"].copy_(live)
        self._graphs[key] = g
        return g

    def _forward_slots(self, st: dict, S: int, nsplit: int, nsplit_trunk: int = 0, each: bool = False, qcap: int = 0,
                       fresh: bool = False, lp=None, ctl=None) -> None:
        """One decode step over S slots: the <= 16-row projections of ``_layers_norm_fused`` around per-slot RoPE + append
        and attention; logits to ``st["logits"]``, then the advance launch.  ``qcap`` > 0: the attention reads the slots' int8
        images (``pc_attn_decode_slots_q8``) and stages the appended row into them; the arenas are appended to as always.
        ``fresh`` (with ``qcap``): no arenas -- ``st["kv_base"]`` holds the fresh-row buffers, ``pc_rope_append_slots_q8`` writes the
        row there and into the image, ``pc_attn_decode_slots_q8_fresh`` reads both."""
        n = _native
        dev, c = self.device, self.config
        H, Hkv, D, hid, inter = self.H, self.Hkv, self.D, c.hidden_size, c.intermediate_size
        W, eps, V = (H + 2 * Hkv) * D, c.rms_norm_eps, c.vocab_size
        cs = torch.empty((S, D // 2, 2), dtype=torch.float32, device=dev)
        n.rope_table(st["pos"], self.inv_freq, cs, S, D)
        h16 = torch.empty((S, hid), dtype=self.dtype, device=dev)
        n.embed_gather(self.embed, st["ids"], h16, S, hid, V)
        x = h16.float()
        qkv = torch.empty((S, W), dtype=torch.float32, device=dev)
        q16 = torch.zeros((S, H * D), dtype=self.dtype, device=dev)
        q16l = torch.zeros((S, H * D), dtype=self.dtype, device=dev)
        ws_bytes = (n.attn_decode_slots_trunk_workspace_bytes(S, H, D, nsplit, nsplit_trunk) if nsplit_trunk
                    else n.attn_decode_slots_workspace_bytes(S, H, D, nsplit))
        ws = torch.empty(max(ws_bytes, 8) // 4, dtype=torch.float32, device=dev)

        def planes(k):          # (zeroed: rows of idle slots are never written and must not hold NaN bit patterns)
            return (torch.zeros((1, k // 32, 64, 8), dtype=self.dtype, device=dev),
                    torch.zeros((1, k // 32, 64, 8), dtype=self.dtype, device=dev))
        ah, al = planes(H * D)
        ch, cl = planes(inter)
        ks_down = self.ks_down and self.ks_min_rows <= S and inter >= 2 * hid
        w4 = self.w4_stream and S <= 16               # the 4-bit images: q|k|v in natural row order (in_layout 0)
        for li, lw in enumerate(self.layers):
            if w4:
                n.gemm_w4(lw["wqkv_c4"], lw["wqkv_e4"], S, W, hid, n.EPI_STORE, x=x, norm_weight=lw["ln1"], eps=eps, y=qkv, ldy=W)
            else:
                n.gemm_skinny_norm(self._w16(lw, "wqkv", True), x, lw["ln1"], eps, S, W, hid, n.EPI_STORE, y=qkv, ldy=W)
            if fresh:
                n.rope_append_slots_q8(qkv, W, 0 if w4 else 1, q16, q16l, H * D, cs, st["kv_base"], st["cap"], st["len"], st["live"], S, li,
                                       H, Hkv, D, st["kvq_base"], qcap, self.L)
            else:
                n.rope_append_slots(qkv, W, 0 if w4 else 1, q16, q16l, H * D, cs, st["kv_base"], st["cap"], st["len"], st["live"], S, li, H,
                                    Hkv, D)
            if fresh:
                n.attn_decode_slots_q8_fresh(q16, q16l, H * D, st["kv_base"], st["cap"], st["len"], st["live"], S, li, H, Hkv, D,
                                             self.softmax_scale, nsplit, ws, (ah, al), st["kvq_base"], qcap, self.L)
            elif qcap and nsplit_trunk:
                n.attn_decode_slots_trunk_q8(q16, q16l, H * D, st["kv_base"], st["cap"], st["len"], st["live"], st["leader"],
                                             st["trunk"], S, li, H, Hkv, D, self.softmax_scale, nsplit, nsplit_trunk, ws, (ah, al),
                                             st["kvq_base"], qcap, self.L)
            elif qcap:
                n.attn_decode_slots_q8(q16, q16l, H * D, st["kv_base"], st["cap"], st["len"], st["live"], S, li, H, Hkv, D,
                                       self.softmax_scale, nsplit, ws, (ah, al), st["kvq_base"], qcap, self.L)
            elif nsplit_trunk:
                n.attn_decode_slots_trunk(q16, q16l, H * D, st["kv_base"], st["cap"], st["len"], st["live"], st["leader"],
                                          st["trunk"], S, li, H, Hkv, D, self.softmax_scale, nsplit, nsplit_trunk, ws, (ah, al))
            else:
                n.attn_decode_slots(q16, q16l, H * D, st["kv_base"], st["cap"], st["len"], st["live"], S, li, H, Hkv, D,
                                    self.softmax_scale, nsplit, ws, (ah, al))
            if w4:
                n.gemm_w4(lw["wo_c4"], lw["wo_e4"], S, hid, H * D, n.EPI_ADD, xf_hi=ah, xf_lo=al, y=x, ldy=hid)
                n.gemm_w4(lw["wgu_c4"], lw["wgu_e4"], S, 2 * inter, hid, n.EPI_SILU, x=x, norm_weight=lw["ln2"], eps=eps, of_hi=ch, of_lo=cl)
                n.gemm_w4(lw["wdown_c4"], lw["wdown_e4"], S, hid, inter, n.EPI_ADD, xf_hi=ch, xf_lo=cl, y=x, ldy=hid)
                continue
            n.gemm_skinny(self._w16(lw, "wo", True), ah, al, S, hid, H * D, n.EPI_ADD, y=x, ldy=hid)                  # x += attn @ Wo^T
            n.gemm_skinny_norm(self._w16(lw, "wgu", True), x, lw["ln2"], eps, S, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl)
            if ks_down:
                sc, ctr = self._ks_buffers(hid)
                n.gemm_skinny_ks(self._w16(lw, "wdown", True), ch, cl, S, hid, inter, x, hid, self.ks_down[1], self.ks_down[0], sc, ctr)
            else:
                n.gemm_skinny(self._w16(lw, "wdown", True), ch, cl, S, hid, inter, n.EPI_ADD, y=x, ldy=hid)           # x += act @ Wd^T
        n.gemm_skinny_norm(self.lm_head_f, x, self.norm, eps, S, V, hid, n.EPI_STORE, y=st["logits"], ldy=V)
        rows, ld = st["logits"], V
        if ctl is not None:           # the token-control node: the advance reads the adjusted rows
            self._ctl_node(ctl, st["logits"], V, S, 1, st["len"])
            rows, ld = ctl["out"], ctl["ldo"]
        if each:
            n.sample_advance_slots_each(rows, ld, V, st["params_each"], st["seeds"], st["hist"], st["ids"], st["pos"], st["len"],
                                        st["cap"], st["live"], st["budget"], st["stop_each"], st["ring"], st["ctr"], st["draws"],
                                        SlotLoop.RING, S)
        else:
            n.sample_advance_slots(rows, ld, V, st["params"], st["seeds"], st["hist"], st["ids"], st["pos"], st["len"],
                                   st["cap"], st["live"], st["budget"], st["stop"], st["ring"], st["ctr"], SlotLoop.RING, S)
        if lp is not None:            # (buffers, top_n): the log-probabilities of the tokens the advance left in ids[b]
            self._lp_node(lp[0], st["logits"], S, st["ids"], 1, lp[1])

    # ---- prompt-lookup drafts in the slot loop (LookupSlotLoop) ----------------------------------------------------------
    def lookup_slot_loop(self, pasts, tokens, positions, max_new: int, k: int, corpora, nmax: int = 3, stop_ids=(),
                         slots: Optional[int] = None, max_keys: Optional[int] = None, share_trunk: bool = False,
                         min_trunk: Optional[int] = None, trunks=None, each: bool = False, slot_index=None, params=None, seeds=None,
                         histories=None, hist_cap: Optional[int] = None, kv: str = "fp16",
                         keep_arenas: bool = True, prompt_rows: bool = False,
                         logprobs: Optional[int] = None, token_controls=None) -> Optional["LookupSlotLoop"]:
        """``slot_loop`` with prompt-lookup drafts: up to ``k + 1`` greedy tokens per sequence and step (``LookupSlotLoop``).
        ``corpora[j]``: the ids sequence j's drafts may copy from besides its own output (``lookup_loop``'s ``corpus_ids``).  None
        where ``slot_loop`` gives None, where the model has no lookup step (``lookup_available``) and where ``S * (k + 1)``
        exceeds the 64 rows of the weight-streaming projections -- the caller then runs ``slot_loop``.  ``share_trunk`` /
        ``min_trunk`` / ``trunks``: ``slot_loop``'s -- sequences that staged the same leading module rows read them from one
        arena, once per step for all draft rows of the group (``pc_attn_verify_slots_trunk``); a batch without such a group runs
        the unshared step, bit for bit.
        ``each``: the step ends in ``pc_lookup_verify_slots_each`` -- ``params`` (None / plain greedy: argmax),
        ``max_new`` and ``stop_ids`` may then be lists with one entry per sequence, ``seeds`` / ``histories`` are ``slot_loop``'s,
        sequence j sits in slot ``slot_index[j]`` and ``LookupSlotLoop.admit`` puts new sequences into slots whose sequence was
        retired.  ``hist_cap``: the ids a slot's draft history holds, fixed for the loop (default 8192).
        ``kv="int8"`` / ``keep_arenas=False``: ``slot_loop``'s -- the step reads int8 images of the slots' rows
        (``LookupSlotLoopQ8``), without fp16 slot arenas where asked (``LookupSlotLoopQ8Only``); ``max_keys`` then also sizes the
        images.  Not with ``share_trunk`` / ``trunks`` and head_dim 128 only: ``check_slot_kv`` raises ValueError.
        ``prompt_rows`` (with ``each``, fp16 arenas): the step takes forced rows and ``LookupSlotLoop.admit_prompt``
        prefills an admitted request's question inside it.  False: today's loop, graph key and launches.
        ``logprobs`` = n in 0..8: the step gains one node behind the verify launches, ``pc_token_logprobs`` over the
        ``S * (k + 1)`` rows at the tokens the verify left in its int32 row scratch; ``LookupSlotLoop.logprobs(j, i)`` hands out the
        records of ``tokens(j, i)``.  Not with ``prompt_rows`` (ValueError).  None: today's graph keys, state and launches.
        ``token_controls``: ``slot_loop``'s -- ``pc_logit_adjust`` over the ``S * (k + 1)`` rows in front of the verify
        launch, row ``(b, i)`` under slot b's block at arena length ``len[b] + i``.  Not with ``prompt_rows`` (ValueError)."""
        if prompt_rows and (not each or kv != "fp16"):
            raise ValueError("lookup_slot_loop: prompt_rows=True needs each=True and kv='fp16'")
        check_logprobs(logprobs, prompt_rows)
        if token_controls is not None:    # (``slot_loop``'s ``token_controls``, in front of the verify launch; not with prompt_rows)
            check_token_controls(TokenControls(), prompt_rows)
        if kv != "fp16" or not keep_arenas:       # (with the mode off nothing is asked of the model here)
            check_slot_kv(kv, share_trunk=bool(share_trunk) or trunks is not None, lookup=k, head_dim=getattr(self, "D", None),
                          no_loop=None if self.slot_loop_available() else "the model has no batched decode loop",
                          lookup_q8=kv == "int8" and self.lookup_slot_q8_available())
            check_slot_keep_arenas(keep_arenas, kv)
        n = len(pasts)
        if not self.lookup_available() or not 1 <= n <= SlotLoop.MAX_SLOTS:
            return None
        S = slots if slots is not None else next(b for b in (1, 2, 4, 8, 16) if b >= (n if slot_index is None else max(slot_index) + 1))
        if not 1 <= k <= 15 or not n <= S <= SlotLoop.MAX_SLOTS or S * (k + 1) > LookupSlotLoop.MAX_ROWS:
            return None
        front = self._slot_loop_front(pasts, stop_ids, each, share_trunk, min_trunk, trunks)
        if front is None:
            return None
        arenas, trunks = front
        cls = ((LookupSlotLoopQ8 if keep_arenas else LookupSlotLoopQ8Only) if kv == "int8" else
               LookupSlotLoopPrompt if prompt_rows else LookupSlotLoop)
        if each:
            return cls.with_options(logprobs, token_controls, self, arenas, tokens, positions, max_new, k, corpora, nmax, stop_ids, S,
                                    max_keys, trunks, True, slot_index, params, seeds, histories, hist_cap)
        return cls.with_options(logprobs, token_controls, self, arenas, tokens, positions, max_new, k, corpora, nmax, stop_ids, S, max_keys,
                                trunks)

    def lookup_slot_q8_available(self) -> bool:
        """Whether ``lookup_slot_loop(kv="int8")`` can run: the lookup step, the slot step and head_dim 128
        (``pc_attn_verify_slots_q8``)."""
        return bool(self.lookup_available() and self.slot_loop_available() and self.D == 128)

    def lookup_trunk_available(self) -> bool:
        """Whether ``lookup_slot_loop`` can share trunks: the lookup step and the slot step are both there."""
        return bool(self.lookup_available() and self.slot_loop_available())

    @torch.inference_mode()
    def _lookup_slot_state(self, S: int, k: int, hist_need: int, each: bool = False, prompt: bool = False) -> dict:
        """Device words of the (S, k) lookup step (one set per (S, k): the captured steps hold their addresses).  The history
        buffer grows in powers of two; the graph key carries its address."""
        sts = self.__dict__.setdefault("_lookup_slot_sts", {})
        st = sts.get((S, k))
        dev, V = self.device, self.config.vocab_size
        if st is None:
            R = S * (k + 1)
            z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
            st = sts[(S, k)] = dict(
                kv_base=z(S, torch.int64), cap=z(S, torch.int32), len=z(S, torch.int32), live=z(S, torch.int32),
                leader=torch.full((S,), -1, dtype=torch.int32, device=dev), trunk=z(S, torch.int32),
                ids=z((S, k + 1), torch.int64), pos=z((S, k + 1), torch.int32), ndraft=z(S, torch.int32), budget=z(S, torch.int32),
                hist_len=z(S, torch.int32), ctr=z(S, torch.int32), amax=z(R, torch.int32),
                stop=torch.full((S, 8), -1, dtype=torch.int32, device=dev), ring=z(S * LookupSlotLoop.RING * (k + 2), torch.int32),
                logits=z((R, V), torch.float32), hist=None)
        if st["hist"] is None or st["hist"].shape[1] < hist_need:
            cap = 8192
            while cap < hist_need:
                cap *= 2
            st["hist"] = torch.zeros((S, cap), dtype=torch.int32, device=dev)
        if each and "bits" not in st:
            # per-slot sampling state of the each=True step (pc_lookup_verify_slots_each): parameter blocks, seeds, penalty
            # bitmaps (``hist`` is the token history here), draw counters and the per-row scratch
            R, hw = S * (k + 1), (V + 31) // 32
            z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
            st.update(params_each=z(S * ctypes.sizeof(_native.SampleParams), torch.uint8), seeds=z(S, torch.int64),
                      bits=z((S, hw), torch.int32), draws=z(S, torch.int32), row_bits=z(R * hw, torch.int32),
                      row_token=z(R, torch.int32))
        if prompt and "forced" not in st:     # forced rows of the prompt_rows step (pc_lookup_*_slots_prompt)
            st["forced"] = torch.zeros(S, dtype=torch.int32, device=dev)
        return st

    def _lookup_slot_graph(self, loop: "LookupSlotLoop"):
        """The captured (S, k) lookup step.  Arena addresses, lengths and histories are device data: one graph per key."""
        st, S, k = loop.st, loop.S, loop.k
        key = ("slots", "lookup", S, k, loop.nsplit) + (("trunk", loop.nsplit_trunk) if loop.nsplit_trunk else ()) + \
            (loop.nmax, st["hist"].data_ptr(), st["hist"].shape[1])
        each = bool(getattr(loop, "each", False))
        if each:
            key += ("each",)
        more = {"each": True} if each else {}
        if getattr(loop, "prompt_rows", False):
            key += ("prompt",)
            more["prompt"] = True
        if loop.kv == "int8":             # the step over int8 images: their rows per plane are an argument of the launches
            key += ("q8", loop.qcap)
            more["qcap"] = loop.qcap
            if getattr(loop, "fresh", None) is not None:
                key += ("fresh",)
                more["fresh"] = True
        if loop.lp_n is not None:         # one more node behind the verify launches: the key gains its top_n
            key += ("logprobs", loop.lp_n)
            more["lp"] = (loop._lp.dev, loop.lp_n)
        if loop._cs is not None:          # one more node in front of the verify launch, which then reads the adjusted rows
            key += ("ctl",)
            more["ctl"] = loop._cs
        ent = self._graphs.pop(key, None)
        if ent is not None:
            self._graphs[key] = ent
            return ent[0]
        if len(self._graphs) >= self.max_graphs:
            self._graphs.pop(next(iter(self._graphs)))
        # one eager pass first (loads code objects / sizes the allocator) with every slot idle: it appends nothing and advances
        # nothing but the record counters, which are put back behind it with the live words
        live, ctr = st["live"].clone(), st["ctr"].clone()
        st["live"].zero_()
        self._forward_lookup_slots(st, S, k, loop.nsplit, loop.nmax, loop.nsplit_trunk, **more)
        torch.cuda.synchronize()
        prime_graph_capture(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._forward_lookup_slots(st, S, k, loop.nsplit, loop.nmax, loop.nsplit_trunk, **more)
        st["live"].copy_(live)
        st["ctr"].copy_(ctr)
        self._graphs[key] = (g, st["hist"])
        return g

    def _forward_lookup_slots(self, st: dict, S: int, k: int, nsplit: int, nmax: int = 3, nsplit_trunk: int = 0,
                              each: bool = False, qcap: int = 0, fresh: bool = False, prompt: bool = False, lp=None,
                              ctl=None) -> None:
        """One lookup step over S slots, ``R = S * (k + 1)`` rows: draft -> per layer {q|k|v plain store, per-slot RoPE + append of
        k + 1 rows, per-slot causal attention, o_proj, gate|up, down} -> lm_head over R rows -> verify.  R <= 16: the norm-folded
        projections of ``_forward_slots``; 17..64 rows: the launch sequence of ``_forward_skinny``'s generic loop (on the 4-bit
        images up to ``w4_max_rows`` rows).
        ``nsplit_trunk`` > 0: the attention with shared trunks (leader / trunk words of the state).
        ``qcap`` > 0: the step over the slots' int8 images -- ``pc_rope_append_slots_rows_q8`` writes every row into
        image and arena, ``pc_attn_verify_slots_q8`` reads the image and the row's own key; ``fresh``: no arenas, ``st["kv_base"]``
        holds the fresh-row buffers.
        ``prompt``: the two ends are the ``_prompt`` entries over ``st["forced"]`` -- a slot with forced rows feeds
        its question through the unchanged middle of the step."""
        n = _native
        dev, c = self.device, self.config
        H, Hkv, D, hid, inter = self.H, self.Hkv, self.D, c.hidden_size, c.intermediate_size
        W, eps, V = (H + 2 * Hkv) * D, c.rms_norm_eps, c.vocab_size
        R = S * (k + 1)
        mt = (R + 15) // 16
        slot = (st["kv_base"], st["cap"], st["len"], st["live"])
        if prompt:
            n.lookup_draft_slots_prompt(st["hist"], st["hist_len"], st["ids"], st["pos"], st["ndraft"], st["cap"], st["len"], st["live"],
                                        st["forced"], S, k, nmax)
        else:
            n.lookup_draft_slots(st["hist"], st["hist_len"], st["ids"], st["pos"], st["ndraft"], st["cap"], st["len"], st["live"], S, k, nmax)
        cs = torch.empty((R, D // 2, 2), dtype=torch.float32, device=dev)
        n.rope_table(st["pos"], self.inv_freq, cs, R, D)
        h16 = torch.empty((R, hid), dtype=self.dtype, device=dev)
        n.embed_gather(self.embed, st["ids"], h16, R, hid, V)
        x = h16.float()
        qkv = torch.empty((R, W), dtype=torch.float32, device=dev)
        q16 = torch.zeros((R, H * D), dtype=self.dtype, device=dev)
        q16l = torch.zeros((R, H * D), dtype=self.dtype, device=dev)
        ws_bytes = (n.attn_verify_slots_q8_workspace_bytes(S, k, H, D, nsplit) if qcap
                    else n.attn_verify_slots_trunk_workspace_bytes(S, k, H, D, nsplit, nsplit_trunk) if nsplit_trunk
                    else n.attn_verify_slots_workspace_bytes(S, k, H, D, nsplit))
        ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=dev)

        def planes(kk, zero=False):   # (zeroed where rows of idle slots are never written: they must not hold NaN bit patterns)
            mk = torch.zeros if zero else torch.empty
            return (mk((mt, kk // 32, 64, 8), dtype=self.dtype, device=dev), mk((mt, kk // 32, 64, 8), dtype=self.dtype, device=dev))
        ah, al = planes(H * D, True)
        ch, cl = planes(inter, True)

        # the 4-bit images: q|k|v in natural row order (in_layout 0); 17..w4_max_rows rows run pc_gemm_w4_rows
        w4 = self.w4_stream and R <= self.w4_max_rows

        def attend(li):
            if qcap:
                n.rope_append_slots_rows_q8(qkv, W, 0 if w4 else 1, q16, q16l, H * D, cs, *slot, S, k, li, H, Hkv, D, st["kvq_base"], qcap,
                                            self.L, fresh)
                n.attn_verify_slots_q8(q16, q16l, H * D, *slot, S, k, li, H, Hkv, D, self.softmax_scale, nsplit, ws, (ah, al),
                                       st["kvq_base"], qcap, self.L, fresh)
                return
            n.rope_append_slots_rows(qkv, W, 0 if w4 else 1, q16, q16l, H * D, cs, *slot, S, k, li, H, Hkv, D)
            if nsplit_trunk:
                n.attn_verify_slots_trunk(q16, q16l, H * D, *slot, st["leader"], st["trunk"], S, k, li, H, Hkv, D, self.softmax_scale,
                                          nsplit, nsplit_trunk, ws, (ah, al))
            else:
                n.attn_verify_slots(q16, q16l, H * D, *slot, S, k, li, H, Hkv, D, self.softmax_scale, nsplit, ws, (ah, al))

        if R <= 16:
            ks_down = self.ks_down and self.ks_min_rows <= R and inter >= 2 * hid
            for li, lw in enumerate(self.layers):
                if w4:
                    n.gemm_w4(lw["wqkv_c4"], lw["wqkv_e4"], R, W, hid, n.EPI_STORE, x=x, norm_weight=lw["ln1"], eps=eps, y=qkv, ldy=W)
                    attend(li)
                    n.gemm_w4(lw["wo_c4"], lw["wo_e4"], R, hid, H * D, n.EPI_ADD, xf_hi=ah, xf_lo=al, y=x, ldy=hid)
                    n.gemm_w4(lw["wgu_c4"], lw["wgu_e4"], R, 2 * inter, hid, n.EPI_SILU, x=x, norm_weight=lw["ln2"], eps=eps, of_hi=ch, of_lo=cl)
                    n.gemm_w4(lw["wdown_c4"], lw["wdown_e4"], R, hid, inter, n.EPI_ADD, xf_hi=ch, xf_lo=cl, y=x, ldy=hid)
                    continue
                n.gemm_skinny_norm(self._w16(lw, "wqkv", True), x, lw["ln1"], eps, R, W, hid, n.EPI_STORE, y=qkv, ldy=W)
                attend(li)
                n.gemm_skinny(self._w16(lw, "wo", True), ah, al, R, hid, H * D, n.EPI_ADD, y=x, ldy=hid)
                n.gemm_skinny_norm(self._w16(lw, "wgu", True), x, lw["ln2"], eps, R, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl)
                if ks_down:
                    sc, ctr = self._ks_buffers(hid)
                    n.gemm_skinny_ks(self._w16(lw, "wdown", True), ch, cl, R, hid, inter, x, hid, self.ks_down[1], self.ks_down[0], sc, ctr)
                else:
                    n.gemm_skinny(self._w16(lw, "wdown", True), ch, cl, R, hid, inter, n.EPI_ADD, y=x, ldy=hid)
            n.gemm_skinny_norm(self.lm_head_f, x, self.norm, eps, R, V, hid, n.EPI_STORE, y=st["logits"], ldy=V)
        else:
            xh, xl = planes(hid)
            KQ = self.rows_kslices(R, hid)
            slabs = torch.empty((KQ, R, hid), dtype=torch.float32, device=dev)
            pending = 0
            for li, lw in enumerate(self.layers):
                n.rmsnorm_frag(x, lw["ln1"], xh, xl, R, hid, eps, slabs, pending)
                pending = KQ
                if w4:
                    n.gemm_w4_rows(lw["wqkv_c4"], lw["wqkv_e4"], xh, xl, R, W, hid, n.EPI_STORE, y=qkv, ldy=W)
                    attend(li)
                    n.gemm_w4_rows(lw["wo_c4"], lw["wo_e4"], ah, al, R, hid, H * D, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ)
                    n.rmsnorm_frag(x, lw["ln2"], xh, xl, R, hid, eps, slabs, KQ)
                    n.gemm_w4_rows(lw["wgu_c4"], lw["wgu_e4"], xh, xl, R, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl)
                    n.gemm_w4_rows(lw["wdown_c4"], lw["wdown_e4"], ch, cl, R, hid, inter, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ)
                    continue
                n.gemm_skinny(self._w16(lw, "wqkv", True), xh, xl, R, W, hid, n.EPI_STORE, y=qkv, ldy=W)
                attend(li)
                n.gemm_skinny(self._w16(lw, "wo", True), ah, al, R, hid, H * D, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ)
                n.rmsnorm_frag(x, lw["ln2"], xh, xl, R, hid, eps, slabs, KQ)
                n.gemm_skinny(self._w16(lw, "wgu", True), xh, xl, R, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl)
                n.gemm_skinny(self._w16(lw, "wdown", True), ch, cl, R, hid, inter, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ)
            n.rmsnorm_frag(x, self.norm, xh, xl, R, hid, eps, slabs, pending)
            n.gemm_skinny(self.lm_head_f, xh, xl, R, V, hid, n.EPI_STORE, y=st["logits"], ldy=V)
        rows, ld = st["logits"], V
        if ctl is not None:           # the token-control node: the verify reads the adjusted rows
            self._ctl_node(ctl, st["logits"], V, S, k + 1, st["len"])
            rows, ld = ctl["out"], ctl["ldo"]
        if prompt:                    # ... and the forced rows of a slot that is still fed its question
            n.lookup_verify_slots_prompt(rows, ld, V, S, k, st["params_each"], st["seeds"], st["bits"], st["row_bits"], st["draws"],
                                         st["row_token"], st["hist"], st["hist_len"], st["ids"], st["pos"], st["len"], st["cap"],
                                         st["live"], st["ndraft"], st["budget"], st["stop"], st["ring"], st["ctr"], st["forced"],
                                         LookupSlotLoop.RING)
        elif each:                    # the sampler on every row, per slot
            n.lookup_verify_slots_each(rows, ld, V, S, k, st["params_each"], st["seeds"], st["bits"], st["row_bits"], st["draws"],
                                       st["row_token"], st["hist"], st["hist_len"], st["ids"], st["pos"], st["len"], st["cap"],
                                       st["live"], st["ndraft"], st["budget"], st["stop"], st["ring"], st["ctr"], LookupSlotLoop.RING)
        else:
            n.lookup_verify_slots(rows, ld, V, S, k, st["amax"], st["hist"], st["hist_len"], st["ids"], st["pos"], st["len"],
                                  st["cap"], st["live"], st["ndraft"], st["budget"], st["stop"], st["ring"], st["ctr"], LookupSlotLoop.RING)
        if lp is not None:            # (buffers, top_n): the log-probabilities of the row tokens the verify left in its int32 scratch
            self._lp_node(lp[0], st["logits"], R, st["row_token" if each else "amax"], 1, lp[1])

    def _ks_buffers(self, hid: int):
        """Scratch slabs + arrival counters of pc_gemm_skinny_ks (shared by every such launch of the model: they run one
        after another on one stream; the counters are zero between launches)."""
        if self._ks_state is None:
            sc = torch.empty(_native.gemm_skinny_ks_scratch_bytes(hid, 8) // 4, dtype=torch.float32, device=self.device)
            self._ks_state = (sc, torch.zeros(hid // 16, dtype=torch.int32, device=self.device))
        return self._ks_state

    def _counters_for(self, B: int, H: int):
        """Arrival counters for the in-launch split merge (PC_ATTN_FUSED=1) -- not for a forward that stages while it reads: that
        one runs the two-launch form of the streaming kernel (pc_attn_gather_ok)."""
        c = self._attn_counters
        return c if c is not None and self._gather is None and B * H <= c.numel() else None

    def _tail_for(self, arena, past_dev):
        """Per-layer ``((k_lo, v_lo, batch_stride, head_stride, lo_row0) | None, lo_base)`` for the current tail mode."""
        mode = self._lo_mode
        if mode == 0:
            return lambda li: (None, -1)
        if mode == 3:                                        # encode pass: the arena's own residual planes, row = key index
            return lambda li: (arena.lo_planes(li), 0)
        base = -1 if mode == 1 else (-2 if past_dev is not None else arena.tail_base)
        return lambda li: (arena.tail_planes(li) + (base,), base)

    def _forward_skinny(self, ids, pos32, past_dev, arena, B, q_len, past_len, last_token_only, num_layers):
        """Layer stack for T = B*q_len <= 64 rows: every projection is a weight-streaming pc_gemm_skinny
        launch over fragment-major weights with split-precision (hi/lo fp16) activations; residual adds and
        SiLU*up are fused into GEMM epilogues; RMSNorm and attention emit the fragment planes directly.
        ``past_dev`` (device int32[1]) makes the pass graph-capturable: the kernels read past_len from it."""
        if self.llm_int8:
            return self._forward_skinny_int8(ids, pos32, past_dev, arena, B, q_len, past_len, last_token_only, num_layers)
        n = _native
        dev = self.device
        c = self.config
        H, Hkv, D, hid, inter = self.H, self.Hkv, self.D, c.hidden_size, c.intermediate_size
        T = B * q_len
        W = (H + 2 * Hkv) * D
        eps = c.rms_norm_eps
        mt = (T + 15) // 16
        if self._pre is not None:                     # (captured forward: pc_prefill_prologue already produced both)
            x, cs = self._pre
        else:
            cs = torch.empty((T, D // 2, 2), dtype=torch.float32, device=dev)
            n.rope_table(pos32, self.inv_freq, cs, T, D)
            h16 = torch.empty((T, hid), dtype=self.dtype, device=dev)
            n.embed_gather(self.embed, ids, h16, T, hid, c.vocab_size)
            x = h16.float()  # fp32 residual stream
        q16 = torch.empty((T, H * D), dtype=self.dtype, device=dev)
        q16l = torch.empty((T, H * D), dtype=self.dtype, device=dev)       # low-order plane of the split-precision q
        ws_bytes = n.attn_workspace_bytes(B, H, D, q_len, past_len + q_len)
        ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.float32, device=dev)
        tail = self._tail_for(arena, past_dev)

        def planes(k):
            return (torch.empty((mt, k // 32, 64, 8), dtype=self.dtype, device=dev),
                    torch.empty((mt, k // 32, 64, 8), dtype=self.dtype, device=dev))

        xh, xl = planes(hid)
        ah, al = planes(H * D)
        ch, cl = planes(inter)
        # The two N = hidden projections (o_proj, down_proj) split K over KQ workgroup slices and leave KQ slabs of
        # partial sums; the next RMSNorm launch folds them into the residual stream (x += sum of slabs).
        KQ = self.rows_kslices(T, hid)
        slabs = torch.empty((KQ, T, hid), dtype=torch.float32, device=dev)
        # ... and so does q|k|v there: its 128-column panels are half as many as the CUs, so K is cut in two and the rotation /
        # append runs over the two slabs (pc_gemm: q|k|v epilogue with kslices = 2)
        QS = int(os.environ.get("PC_ROWS_QKV_KS", "2")) if (self.SKINNY_MAX_ROWS < T <= 288 and KQ != self.kslices and lw0_fp16(self.layers)) else 1
        qkv_slabs = torch.empty((QS, T, W), dtype=torch.float32, device=dev) if QS > 1 else None
        pending = 0                                   # slabs waiting to be added to x
        layers = self.layers if num_layers is None else self.layers[:num_layers]
        if T <= (16 if self.int8_weights else self.NORM_FUSED_MAX_ROWS) and self.fuse_norm:   # (int8 weight images: one row tile)
            return self._layers_norm_fused(x, cs, q16, q16l, ws, ah, al, ch, cl, arena, layers, B, q_len, past_len, past_dev,
                                           last_token_only, tail)
        # 17..w4_max_rows rows of an MXFP4 model: the four projections on the 4-bit images (pc_gemm_w4_rows), q|k|v as a plain
        # store in natural row order followed by pc_rope_append_ex, as the <= 16-row loop has it (_layers_norm_fused)
        w4 = self.w4_stream and 16 < T <= self.w4_max_rows
        qkv = torch.empty((T, W), dtype=torch.float32, device=dev) if w4 else None
        for li, lw in enumerate(layers):
            n.rmsnorm_frag(x, lw["ln1"], xh, xl, T, hid, eps, slabs, pending)
            kp, vp = arena.k_plane(li), arena.v_plane(li)
            kvlo, lo_base = tail(li)
            if w4:
                n.gemm_w4_rows(lw["wqkv_c4"], lw["wqkv_e4"], xh, xl, T, W, hid, n.EPI_STORE, y=qkv, ldy=W)
                n.rope_append(qkv, q_len * W, W, q16, q_len * H * D, H * D, qkv[:, H * D:], qkv[:, (H + Hkv) * D:], q_len * W, W,
                              kp, vp, arena.batch_stride, arena.head_stride, cs, B, H, Hkv, D, q_len, past_len, arena.cap, True,
                              past_len_dev=past_dev, q_out_lo=q16l, kv_lo=kvlo)
            else:
                # q|k|v projection + RoPE + in-place KV append in one weight-streaming launch
                n.gemm_qkv_rope(self._w16(lw, "wqkv", True), xh, xl, T, hid, cs, q16, q16l, H * D, kp, vp, arena.batch_stride,
                                arena.head_stride, B, H, Hkv, D, q_len, past_len, arena.cap, past_dev, kv_lo=kvlo and kvlo[:4],
                                wscale=lw["wqkv_s"], lo_base=lo_base, kslices=QS, scratch=qkv_slabs)
            if self._kv_only and li == len(layers) - 1:
                return None       # schema encode: the K / V of the last layer are written; nothing after them is used
            n.attn_fwd(q16, q_len * H * D, H * D, kp, vp, arena.batch_stride, arena.head_stride, None, 0, 0,
                       B, H, Hkv, D, q_len, past_len, self.softmax_scale, ws, past_len_dev=past_dev, out_frag=(ah, al),
                       q_lo=q16l, kv_lo=kvlo, counters=self._counters_for(B, H),
                       gather=None if self._gather is None else (self._gather, li * 2 * Hkv, (li * 2 + 1) * Hkv))
            if w4:
                n.gemm_w4_rows(lw["wo_c4"], lw["wo_e4"], ah, al, T, hid, H * D, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ)
                n.rmsnorm_frag(x, lw["ln2"], xh, xl, T, hid, eps, slabs, KQ)
                n.gemm_w4_rows(lw["wgu_c4"], lw["wgu_e4"], xh, xl, T, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl)
                n.gemm_w4_rows(lw["wdown_c4"], lw["wdown_e4"], ch, cl, T, hid, inter, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ)
                pending = KQ
                continue
            mid_skip = self.mid_lo_skip if (T > self.SKINNY_MAX_ROWS and self._lo_mode != 3) else ()      # (precision audit: tools/plane_audit.py)
            n.gemm_skinny(self._w16(lw, "wo", True), ah, None if "o" in mid_skip else al, T, hid, H * D, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ,
                          wscale=lw["wo_s"])                                                    # attn @ Wo^T
            n.rmsnorm_frag(x, lw["ln2"], xh, xl, T, hid, eps, slabs, KQ)                       # x += ...; norm
            # (an encode pass on this stack follows the many-row stack's plane policy: dense_lo_skip; PC_MID_LO_SKIP=gu extends it to
            # the long-question forward)
            gu_lo = None if (T > self.SKINNY_MAX_ROWS and ((self._lo_mode == 3 and "gu" in self.dense_lo_skip) or
                                                           (self._lo_mode != 3 and "gu" in self.mid_lo_skip))) else xl
            n.gemm_skinny(self._w16(lw, "wgu", True), xh, gu_lo, T, 2 * inter, hid, n.EPI_SILU, of_hi=ch, of_lo=cl, wscale=lw["wgu_s"])  # silu(g)*u
            n.gemm_skinny(self._w16(lw, "wdown", True), ch, None if "down" in mid_skip else cl, T, hid, inter, n.EPI_STORE, y=slabs, ldy=hid, kslices=KQ,
                          wscale=lw["wdown_s"])                                                 # act @ Wd^T
            pending = KQ
        V = c.vocab_size
        if last_token_only:
            if pending:
                x.add_(slabs.sum(dim=0))
            xlast = x.view(B, q_len, hid)[:, -1, :].contiguous()
            lh, ll = planes(hid)
            n.rmsnorm_frag(xlast, self.norm, lh, ll, B, hid, eps)
            logits = torch.empty((B, V), dtype=torch.float32, device=dev)
            n.gemm_skinny(self.lm_head_f, lh, ll, B, V, hid, n.EPI_STORE, y=logits, ldy=V)
            return logits.view(B, 1, V)
        n.rmsnorm_frag(x, self.norm, xh, xl, T, hid, eps, slabs, pending)
        logits = torch.empty((T, V), dtype=torch.float32, device=dev)
        n.gemm_skinny(self.lm_head_f, xh, xl, T, V, hid, n.EPI_STORE, y=logits, ldy=V)          # llama2.py:1050-1051
        return logits.view(B, q_len, V)
