"""Generation engine: one prefill over the staged KV (TTFT), then token-by-token decode.

Public surface of ``promptcache/generation_engine.py`` in the reference -- ``GenerationParameters`` (:21-42),
``is_partial_stop`` (:45-50), ``Output`` (:53-58), ``GenerationEngine.generate`` (:67-209) -- kept, including
its observable quirks:

* the first decoded token is placed at position ``max(position_ids) + 2``: the reference adds the loop index,
  which starts at 1 for the first decode step, to ``max(position_ids) + 1`` (:82, :132);
* ``Output`` is constructed positionally as ``Output(text, new_text, inference_time, response_time)`` (:201), so
  the field called ``response_time`` carries the running total and ``elapsed_time`` the prefill latency (TTFT).

Underneath, every forward is the HIP path: K/V of new tokens are appended in place to the arena behind ``cache``
(no per-layer ``torch.cat`` of the whole past, ``llama2.py:361-364``) and each decode step replays one captured
hipGraph (``model/llama_hip.py``).
"""
from __future__ import annotations

import gc
import os
import time
from dataclasses import dataclass, field
from typing import Dict, Generator, List, Optional, Tuple

import torch

from . import modes
from .model import LanguageModel
from .model.kv_arena import StagedKV
from .slot_scheduler import SlotScheduler, split_stop_ids, wants_look_ahead


@dataclass
class GenerationParameters:
    temperature: float = 1.0
    repetition_penalty: float = 1.0
    top_p: float = 1.0
    top_k: int = -1
    max_new_tokens: int = 256
    stop_token_ids: List[int] = field(default_factory=list)
    stop_str: List[str] = field(default_factory=list)
    echo: bool = True
    # None: off.  n in 0..8: every generated token comes with its log-probability and those of the n most likely tokens, under the
    # model's own distribution -- the log-softmax of the raw logits, BEFORE temperature, repetition penalty, top-p and top-k
    logprobs: Optional[int] = None
    # Token controls (all off by default).  They act on the logits row IN FRONT of the chain above -- temperature,
    # repetition penalty, top-p, top-k, the greedy rule -- and leave ``Output.logprobs`` alone (the model's own distribution).
    # logit_bias: token id -> a value added to its logit (finite, or -inf: a ban); banned_token_ids: shorthand for -inf, a ban wins
    # over a finite bias on the same id; together at most modes.LOGIT_BIAS_MAX = 64 distinct ids
    logit_bias: Optional[Dict[int, float]] = None
    banned_token_ids: Optional[List[int]] = None
    # every token NOT listed becomes -inf ("answer with A, B, C or D")
    allowed_token_ids: Optional[List[int]] = None
    # the ids in stop_token_ids are -inf for the generated tokens numbered g < min_new_tokens (g = 0: the token drawn from the
    # prefill; transformers' MinNewTokensLengthLogitsProcessor); stop strings are not affected; at most 8 stop ids with it
    min_new_tokens: int = 0

    def __post_init__(self):
        modes.check_logprobs(self.logprobs, what="GenerationParameters.logprobs")
        self.token_controls                # (validates: ValueError here, not at the first token)

    @property
    def token_controls(self) -> Optional[modes.TokenControls]:
        """The merged, validated token controls (``modes.token_controls``), or None when all four fields are vacuous."""
        return modes.token_controls(self.logit_bias, self.banned_token_ids, self.allowed_token_ids, self.min_new_tokens,
                                    self.stop_token_ids)

    @property
    def greedy(self) -> bool:
        return self.temperature < 1e-5 or self.top_p < 1e-8

    @property
    def plain_greedy(self) -> bool:
        """Greedy decoding whose processed argmax is the raw argmax: the greedy device loops; everything else is sampled."""
        return self.greedy and self.repetition_penalty <= 1.0

    def get_logits_processor(self):
        """Same processor chain, same order and thresholds as the reference (:32-42)."""
        from transformers.generation import logits_process as lp
        chain = lp.LogitsProcessorList()
        if self.temperature >= 1e-5 and self.temperature != 1.0:
            chain.append(lp.TemperatureLogitsWarper(self.temperature))
        if self.repetition_penalty > 1.0:
            chain.append(lp.RepetitionPenaltyLogitsProcessor(self.repetition_penalty))
        if 1e-8 <= self.top_p < 1.0:
            chain.append(lp.TopPLogitsWarper(self.top_p))
        if self.top_k > 0:
            chain.append(lp.TopKLogitsWarper(self.top_k))
        return chain


def is_partial_stop(output: str, stop_str: str) -> bool:
    """True while the tail of ``output`` may still grow into ``stop_str`` (reference :45-50; note that
    ``output[-0:]`` is the whole string, so the first probe compares against everything generated so far)."""
    return any(stop_str.startswith(output[-i:]) for i in range(0, min(len(output), len(stop_str))))


@dataclass
class TokenLogprob:
    """One generated token: its id, its log-probability under the model's own distribution (the log-softmax of the raw logits,
    before temperature, repetition penalty, top-p and top-k) and the ``GenerationParameters.logprobs`` most likely tokens of that
    step as ``(id, logprob)``, by (logprob descending, id ascending); the token itself may be among them."""
    token: int
    logprob: float
    top: List[Tuple[int, float]] = field(default_factory=list)


@dataclass
class Output:
    text: str
    new_text: str
    response_time: float = 0.0
    elapsed_time: float = 0.0
    # ``GenerationParameters.logprobs``: one entry per token generated so far, stop id included -- cumulative like ``new_text``, but
    # a stop string cuts the text, not the list.  None when not asked for.
    logprobs: Optional[List[TokenLogprob]] = None


class _Timer:
    """HIP-event stopwatch around one ``lm()`` call (the reference's measuring recipe, :104-115)."""

    def __enter__(self):
        self.t0 = torch.cuda.Event(enable_timing=True)
        self.t1 = torch.cuda.Event(enable_timing=True)
        self.t0.record()
        return self

    def __exit__(self, *exc):
        self.t1.record()
        torch.cuda.synchronize()
        self.ms = self.t0.elapsed_time(self.t1)
        return False


class _Stream:
    """What the host keeps per sequence, and the one rule for a token that came back from the device (``emit``).  ``index`` is
    the sequence's number in ``generate_batch`` / ``serve``; ``slot``, ``k`` (its index in the loop) and ``device_stops`` (the
    stop ids the device holds, None: all) are ``serve``'s; a loop is built or armed from ``seed``, ``past`` and ``first_free``."""

    def __init__(self, render, params: GenerationParameters, stream_interval: int, prompt_ids: List[int], first_free: int,
                 index: int = 0, seed: int = 0, slot: int = 0, device_stops: Optional[List[int]] = None):
        self.render, self.params, self.stream_interval = render, params, stream_interval
        self.output_ids, self.new_ids = list(prompt_ids), []
        self.first_free, self.index, self.seed, self.slot, self.k, self.past = first_free, index, seed, slot, None, None
        self.device_stops = params.stop_token_ids if device_stops is None else device_stops
        self.total_ms = self.ttft_ms = 0.0
        self.last_step, self.done = params.max_new_tokens - 1, False
        self.want_lp = getattr(params, "logprobs", None)      # n: every token comes with a record (``emit``'s ``lp``)
        self.lps: Optional[List[TokenLogprob]] = None if self.want_lp is None else []

    def emit(self, token: int, lp=None) -> Optional[Output]:
        """Take the next token: append it, test the stop ids, and at a streaming point (every ``stream_interval`` tokens, the last
        step, a stop id) render the text, cut it at a stop string and hold it back while its tail may still grow into one.
        Sets ``done``; -> the Output to yield, if any.  The step is the number of tokens taken before this one.
        ``lp``: the token's record ``(token, logprob, [(id, logprob), ...])`` where the parameters ask for log-probabilities -- kept
        with its first ``logprobs`` alternatives (a serving loop's step ranks as many as ``serve(logprobs=...)`` said)."""
        step = len(self.new_ids)
        self.output_ids.append(token)
        self.new_ids.append(token)
        if self.lps is not None:
            if lp is None:
                raise RuntimeError("a token arrived without its log-probabilities although GenerationParameters.logprobs asks for them")
            self.lps.append(TokenLogprob(int(token), float(lp[1]), [(int(a), float(b)) for a, b in lp[2][:self.want_lp]]))
        fin = token in self.params.stop_token_ids
        out = None
        if step % self.stream_interval == 0 or step == self.last_step or fin:
            text, new_text, hit, partial = self.render(self.output_ids, self.new_ids, self.params.stop_str)
            fin = fin or hit
            if not partial:
                out = Output(text, new_text, self.total_ms, self.ttft_ms, None if self.lps is None else list(self.lps))
        self.done = fin or step >= self.last_step
        return out

    def ended_on_the_host(self, token: int) -> bool:
        """After ``emit(token)``: the sequence ended for a reason its device loop cannot know -- a stop string, a stop id the
        device does not hold -- so neither one of the device's stop ids nor the budget: the host must switch the slot off."""
        return self.done and token not in self.device_stops and len(self.new_ids) - 1 != self.last_step


def _reader(loop):
    """-> ``(read, k)`` over any device loop: ``read(i)`` / ``read(j, i)`` gives the list of tokens of step ``i`` (of sequence
    ``j``), empty when nothing more will come (the budget ran out, the slot is off), and a step gives ``k + 1`` tokens at most.
    A one-token loop (``token``: GreedyLoop, SampleLoop, SlotLoop) is a multi-token loop (``tokens``: LookupLoop,
    SampleLookupLoop, LookupSlotLoop) with k = 0.  A new kind of loop plugs in here."""
    if hasattr(loop, "tokens"):
        return loop.tokens, loop.k

    def one(*at):
        token = loop.token(*at)
        return [] if token is None else [token]
    return one, 0


def _first_logprobs(hf, logits_row, token: int, n: Optional[int]):
    """The record of a token drawn on the host side from ``logits_row`` (the prefill's last row, a stepped forward's row): one
    eager launch (``LlamaHIP.token_logprobs``).  None when not asked for; a model without the call is an error, not a fallback."""
    if n is None:
        return None
    if not hasattr(hf, "token_logprobs"):
        raise RuntimeError("GenerationParameters.logprobs needs a model with token_logprobs (pc_token_logprobs)")
    return hf.token_logprobs(logits_row, [token], n)[0]


def _adjusted(hf, logits_row, controls, generated: int):
    """``logits_row`` as the draw of generated token number ``generated`` sees it under ``controls``: one eager launch
    (``LlamaHIP.adjust_logits``) in front of the argmax / sampler.  None: the row itself; a model without the call is an error, not
    a fallback."""
    if controls is None:
        return logits_row
    if not hasattr(hf, "adjust_logits"):
        raise RuntimeError("token controls (logit_bias, banned_token_ids, allowed_token_ids, min_new_tokens) need a model with "
                           "adjust_logits (pc_logit_adjust)")
    return hf.adjust_logits(logits_row, controls, generated)


def _controls_of(hf, params, loop_prefill: bool = False):
    """The token controls a request runs with, checked against the model's vocabulary (first use) -> ``TokenControls`` or None."""
    vocab = getattr(getattr(hf, "config", None), "vocab_size", None)
    return modes.check_token_controls(params.token_controls, loop_prefill, vocab, len(params.stop_token_ids))


class GenerationEngine:
    # decode greedy generations as a device-side loop when the model offers one (PC_DEVICE_GREEDY=0: step through lm())
    device_greedy_loop = os.environ.get("PC_DEVICE_GREEDY", "1") != "0"
    # ... and every other generation (sampled, or greedy with a repetition penalty) as the sampled device loop
    # (model/llama_hip.py SampleLoop; PC_DEVICE_SAMPLE=0: step through lm() and torch's sampler)
    device_sample_loop = os.environ.get("PC_DEVICE_SAMPLE", "1") != "0"

    def __init__(self, lm: LanguageModel, verbose: bool = False, lookup: Optional[int] = None,
                 lookup_sampled: Optional[bool] = None):
        """``lookup`` = k > 0 (None: ``PC_LOOKUP``, default 0 = off): plain-greedy generations draft up to k tokens per step by
        prompt lookup and verify them in one k+1-row forward (model/llama_hip.py LookupLoop) where the model offers it.
        ``lookup_sampled`` (None: ``PC_LOOKUP_SAMPLE=1``, default off): with ``lookup`` > 0, every other generation of
        ``generate`` -- sampled, or greedy with a repetition penalty -- does the same with the sampler on every row
        (SampleLookupLoop) instead of the one-token SampleLoop; on identical logits the tokens are SampleLoop's."""
        self.lm = lm
        self.verbose = verbose
        self.lookup = int(os.environ.get("PC_LOOKUP", "0")) if lookup is None else int(lookup)
        self.lookup_sampled = os.environ.get("PC_LOOKUP_SAMPLE", "0") == "1" if lookup_sampled is None else bool(lookup_sampled)

    # -- pieces of the loop ---------------------------------------------------------------------
    def _forward(self, ids: List[int], positions: List[int], past) -> Tuple[torch.Tensor, object, float]:
        # Host tensors: the model's captured small-q forward takes token ids, positions, past length and a pending staging plan
        # in ONE pinned host-to-device copy (model/llama_hip.py _InputBlock); the reference uploads ids and positions as two
        # pageable copies in front of the timed call (:96-97).  Paths that want device tensors move them themselves.
        ids_t = torch.tensor([ids], dtype=torch.long)
        pos_t = torch.tensor([positions], dtype=torch.long)
        with _Timer() as t:
            out = self.lm(input_ids=ids_t, position_ids=pos_t, past_key_values=past, use_cache=True)
        return out.logits, out.past_key_values, t.ms

    @staticmethod
    def _pick(last_logits: torch.Tensor, greedy: bool) -> int:
        if greedy:
            return int(torch.argmax(last_logits))
        return int(torch.multinomial(torch.softmax(last_logits, dim=-1), num_samples=1))

    def _render(self, output_ids: List[int], new_ids: List[int], stop_strs: List[str]) -> Tuple[str, str, bool, bool]:
        """-> (text, new_text, hit_stop_string, partially_matched)."""
        text, new_text = self.lm.decode(output_ids), self.lm.decode(new_ids)
        for stop in stop_strs:
            cut = new_text.rfind(stop, 0)
            if cut != -1:
                return text, new_text[:cut], True, False
            if is_partial_stop(text, stop):
                return text, new_text, False, True
        return text, new_text, False, False

    @staticmethod
    def _lookup_corpus(cache, token_ids: List[int]) -> List[int]:
        """What a lookup generation may copy from: the ids of the staged rows in arena row order (the ``KVArena.layout`` runs
        carry their token sequences; a run whose ids cannot be recovered contributes nothing), then the prompt's new ids."""
        ids: List[int] = []
        for run in getattr(getattr(cache, "arena", None), "layout", None) or []:
            try:
                t = [int(x) for x in run[0].token_ids()]
            except Exception:
                continue
            if len(t) == run[1]:
                ids += t
        return ids + [int(x) for x in token_ids]

    # -- the two pumps ----------------------------------------------------------------------------
    @staticmethod
    def _pump(loop, total: int, want_lp: bool = False):
        """Read a single-sequence device loop: yields ``(token, ms)`` -- ``(token, ms, record)`` with ``want_lp``, the only case in
        which the loop is asked for ``logprobs(i)`` -- until ``total`` tokens came or a step is empty.  ``ms`` is the
        step's device time on its first token and 0.0 on the others.  Every step of such a loop is one hipGraph replay that also
        picks the token(s) and feeds the next replay (model/llama_hip.py GreedyLoop, SampleLoop: one token; LookupLoop,
        SampleLookupLoop: 1..k+1 tokens).  The host keeps ONE replay in flight ahead of the step it reads, so the GPU never waits
        for the host's stop handling, but only while the step in flight cannot exhaust the budget (a replay behind the last token
        would stream the weights for nothing).  The consumer stops reading at a stop; a step enqueued past it, and the tokens of
        a step behind it, are simply discarded."""
        read, k = _reader(loop)
        got = i = 0
        while got < total:
            if loop.n <= i:
                loop.enqueue()
            if loop.n == i + 1 and got + k + 1 < total:
                loop.enqueue()                                     # the replay AFTER the one whose tokens are read below
            toks, ms = read(i), loop.elapsed_ms(i)
            if not toks:
                return
            lps = loop.logprobs(i) if want_lp else None
            for t, token in enumerate(toks):
                yield (token, ms, lps[t]) if want_lp else (token, ms)
                ms = 0.0
            got += len(toks)
            i += 1

    @staticmethod
    def _pump_slots(loop, seqs: List[_Stream]):
        """Read a batched device loop (SlotLoop, LookupSlotLoop) until every stream of ``seqs`` (``seqs[j]`` is sequence j of the
        loop) is done; yields ``(index, Output)``.  One replay ahead as in ``_pump``, while the step in flight cannot exhaust
        every budget.  A sequence ends at a stop id or its budget, which the device sees too, at an empty step (the device
        switched the slot off) or for a reason only the host knows (``_Stream.ended_on_the_host``): then the host switches
        the slot off between replays (``loop.kill``) and drops the rest of the step.  A loop is asked for ``logprobs(j, i)`` only
        for a stream whose parameters ask for them."""
        read, k = _reader(loop)
        i = 0
        while not all(st.done for st in seqs):
            room = max(st.last_step - (len(st.new_ids) - 1) for st in seqs if not st.done)
            if loop.n <= i:
                loop.enqueue()
            if loop.n == i + 1 and room > k + 1:
                loop.enqueue()                                     # the replay AFTER the one whose tokens are read below
            ms = loop.elapsed_ms(i)
            for j, st in enumerate(seqs):
                if st.done:
                    continue
                toks = read(j, i)
                if not toks:
                    st.done = True
                    continue
                st.total_ms += ms
                lps = loop.logprobs(j, i) if st.lps is not None else None
                for t, token in enumerate(toks):
                    out = st.emit(token, None if lps is None else lps[t])
                    kill = st.ended_on_the_host(token)
                    if kill and not k:                             # (a one-token loop is told before the yield, a multi-token
                        loop.kill(j)                               # loop after it: each as it was before there was one pump)
                    if out is not None:
                        yield st.index, out
                    if kill and k:
                        loop.kill(j)
                    if st.done:
                        break
            i += 1

    def _first_token(self, st: _Stream, token_ids: List[int], position_ids: List[int], cache) -> Optional[Output]:
        """Prefill and first token of a sequence of ``generate_batch`` / ``serve``: the forward ``generate`` runs, the token drawn as
        ``generate`` draws it (argmax, or step 0 of the random stream of ``st.seed`` on the device).  Fills ``st.past``."""
        logits, st.past, ms = self._forward(token_ids, position_ids, cache)
        st.ttft_ms = st.total_ms = ms
        if self.verbose:
            print(f"Prefill latency: {ms:.2f} ms")
        hf = getattr(self.lm, "hf_model", None)
        ctl = _controls_of(hf, st.params)
        if ctl is not None:                                        # (generated token number 0, under the request's controls)
            row = _adjusted(hf, logits[0, -1], ctl, 0)
            token = self._pick(row, True) if st.params.plain_greedy else hf.sample_token(row, st.params, st.seed, st.output_ids)
        elif st.params.plain_greedy:
            token = self._pick(st.params.get_logits_processor()(None, logits[:, -1, :])[0], True)
        else:
            token = self.lm.hf_model.sample_token(logits[0, -1], st.params, st.seed, st.output_ids)
        return st.emit(token, _first_logprobs(hf, logits[0, -1], token, st.want_lp))

    # -- the generator ----------------------------------------------------------------------------
    @torch.inference_mode()
    def generate(self, token_ids: List[int], position_ids: List[int], params: GenerationParameters,
                 cache=None, stream_interval: int = 2, use_full_position_ids: bool = False
                 ) -> Generator[Output, None, None]:
        n_lp = modes.check_logprobs(params.logprobs, what="GenerationParameters.logprobs")
        lp_kw = {} if n_lp is None else {"logprobs": n_lp}      # (a loop is handed nothing new when they are off)
        ctl = _controls_of(getattr(self.lm, "hf_model", None), params)
        if ctl is not None:                                     # (the loops draw from the adjusted row)
            lp_kw["token_controls"] = ctl
        processors = params.get_logits_processor()
        prompt_positions = list(position_ids)
        first_free = max(prompt_positions) + 1
        st = _Stream(self._render, params, stream_interval, token_ids, first_free)
        loop = past = None

        # Plain-greedy generations decode in the greedy device loop when the model offers one, every other generation in the
        # sampled device loop: the last node of each replay applies the reference's logits chain and draws the token on the GPU
        # (pc_sample_advance).  Its first token is drawn from the prefill logits by the same kernel at step 0 of the same random
        # stream, whose seed comes from torch's default generator, so torch.manual_seed governs reproducibility.
        hf = getattr(self.lm, "hf_model", None)
        plain_greedy = params.plain_greedy
        want_loop = plain_greedy and not use_full_position_ids and hasattr(hf, "greedy_loop") and self.device_greedy_loop
        want_sample = not plain_greedy and not use_full_position_ids and hasattr(hf, "sample_loop") and self.device_sample_loop
        seed = int(torch.randint(0, 2 ** 62, (1,))) if want_sample else 0
        # ... and with ``lookup`` = k > 0 a plain-greedy generation runs the lookup loop instead: a step yields 1..k+1 tokens.
        want_lookup = want_loop and self.lookup > 0 and hasattr(hf, "lookup_loop")
        # ... and with ``lookup_sampled`` the other generations do the same in the sampled lookup loop (SampleLookupLoop): the
        # first token, the seed, the history and the host's stop handling per token are the sampled loop's, the steps the lookup's
        want_lookup_sample = (want_sample and self.lookup > 0 and self.lookup_sampled and hasattr(hf, "lookup_loop") and
                              hasattr(hf, "lookup_available") and hf.lookup_available())

        def pick(logits):
            last = logits[:, -1, :]
            if ctl is not None:                                    # (the token about to be drawn is number len(new_ids))
                last = _adjusted(hf, logits[0, -1], ctl, len(st.new_ids))[None, :]
            if want_sample:                                        # (the first token only: the loop draws every later one)
                return hf.sample_token(last[0], params, seed, st.output_ids)
            history = torch.as_tensor([st.output_ids], device=self.lm.device) if params.repetition_penalty > 1.0 else None
            return self._pick(processors(history, last)[0], params.greedy)

        def host_steps():
            nonlocal past
            while not st.done:
                step = len(st.new_ids)
                positions = (prompt_positions + list(range(first_free, first_free + step))) if use_full_position_ids \
                    else [first_free + step]
                logits, past, ms = self._forward([st.new_ids[-1]], positions, past)
                token = pick(logits)
                yield (token, ms) if n_lp is None else (token, ms, _first_logprobs(hf, logits[0, -1], token, n_lp))

        try:
            if params.max_new_tokens < 1:
                return
            # 1. prefill and first token
            if cache is not None and not isinstance(cache, StagedKV):
                # a plain list of [Hkv, S, D] views: add the batch dim like the reference does (:101-102)
                cache = [(k.unsqueeze(0), v.unsqueeze(0)) if k.dim() == 3 else (k, v) for k, v in cache]
            logits, past, ms = self._forward(list(token_ids), prompt_positions, cache)
            st.ttft_ms = st.total_ms = ms
            if self.verbose:
                print(f"Prefill latency: {ms:.2f} ms")
            if want_sample:
                want_sample = hf.can_loop(past)
            token = pick(logits)
            out = st.emit(token, _first_logprobs(hf, logits[0, -1], token, n_lp))
            if out is not None:
                yield out
            # 2. a device loop, where there is one and something is left to decode
            if not st.done and (want_loop or want_sample):
                # the first decoded token sits at position first_free + 1 (the reference's loop index starts at 1, :132)
                token, position = st.new_ids[0], first_free + 1
                if want_lookup or want_lookup_sample:
                    sampled = dict(params=params, seed=seed, history_ids=st.output_ids) if want_lookup_sample else {}
                    loop = hf.lookup_loop(past, token, position, st.last_step, min(self.lookup, 15),
                                          self._lookup_corpus(cache, token_ids), **sampled, **lp_kw)
                elif want_loop:
                    loop = hf.greedy_loop(past, token, position, params.max_new_tokens, **lp_kw)
                else:
                    loop = hf.sample_loop(past, token, position, params.max_new_tokens, params, seed, st.output_ids, **lp_kw)
            # 3. the rest: that loop's tokens, or one forward per token
            for token, ms, *lp in (host_steps() if loop is None else self._pump(loop, st.last_step, n_lp is not None)):
                st.total_ms += ms
                out = st.emit(token, *lp)
                if out is not None:
                    yield out
                if st.done:                                        # (before the source is asked for more)
                    break
        finally:
            # also when the consumer abandons the generator at a yield (GeneratorExit): a look-ahead replay enqueued past the last
            # token the caller saw wrote one arena row too many, and the model's loop state must be released
            if loop is not None:
                loop.close(len(st.new_ids) - 1)              # steps of the loop that produced a token (the first came from the prefill)
            del past, loop
            gc.collect()

    # -- several prompts at once ------------------------------------------------------------------
    MAX_BATCH = modes.MAX_BATCH

    def _capabilities(self, greedy: bool, sampled: bool) -> modes.Capabilities:
        """What this model and engine offer a call that decodes greedy and / or sampled sequences (modes.py resolves the call's
        modes from it): the one place that asks the model.  A model without a method does not have the step."""
        hf = getattr(self.lm, "hf_model", None)

        def says(name: str) -> bool:
            offered = getattr(hf, name, None)
            return offered is not None and bool(offered())
        no_loop = off = None
        if getattr(self.lm, "use_full_position_ids", False):
            no_loop = "the model takes full position ids (per-key positions are re-based on the host every step)"
        elif not hasattr(hf, "slot_loop") or not hf.slot_loop_available():
            no_loop = "the model has no batched decode loop (architecture, int8 weights or PC_DECODE_TAIL=1)"
        elif greedy and not self.device_greedy_loop:
            off = "PC_DEVICE_GREEDY=0"
        elif sampled and not self.device_sample_loop:
            off = "PC_DEVICE_SAMPLE=0"
        has = hasattr(hf, "lookup_slot_loop")
        return modes.Capabilities(no_loop, no_loop or off, has, has and says("lookup_available"), says("lookup_slot_q8_available"),
                                  says("lookup_trunk_available"), getattr(hf, "D", None), says("slot_trunk_q8_available"))

    def _batch_modes(self, n_requests: int, params: GenerationParameters, **kw) -> modes.Modes:
        return modes.resolve_batch(self._capabilities(params.plain_greedy, not params.plain_greedy), n_requests, params.plain_greedy,
                                   len(params.stop_token_ids), params.max_new_tokens, **kw)

    def batch_plan(self, n_requests: int, params: GenerationParameters, slot_kv: Optional[str] = None) -> Tuple[bool, str]:
        """``(batched, reason)``: whether ``generate_batch`` decodes ``n_requests`` sequences together in one device loop
        (``model/llama_hip.py`` SlotLoop) or runs them one after another through ``generate``, and why.  Host logic only.
        ``slot_kv`` (None: ``PC_SLOT_KV``): with "int8" the reason of a batched plan says that the loop reads int8 K/V images."""
        m = self._batch_modes(n_requests, params, share_trunk=False, lookup=0, slot_kv=slot_kv, validate=False)
        return m.batched, m.reason()

    @torch.inference_mode()
    def generate_batch(self, requests, params: GenerationParameters, stream_interval: int = 2,
                       share_trunk: Optional[bool] = None, lookup: Optional[int] = None, slot_kv: Optional[str] = None,
                       keep_arenas: Optional[bool] = None) -> Generator[Tuple[int, Output], None, None]:
        """Generate for several prompts at once: ``requests = [(token_ids, position_ids, cache), ...]``, each as
        ``CacheEngine.process(prompt, slot=k)`` returned it (every cache in a staged buffer of its own).  Yields ``(index,
        Output)`` pairs; per sequence the ``Output`` stream, the stop-token and stop-string handling, ``max_new_tokens`` and the
        position rule are ``generate``'s.  The prefills run one after another through the path ``generate`` takes and the first
        token of each sequence is drawn as ``generate`` draws it; then ONE device loop decodes all sequences together, the
        host one replay ahead.  Sequence k of a sampled batch uses seed ``seed + k`` of the one seed taken from torch's default
        generator.  Where no batched loop is available (``batch_plan``) the sequences run one after another through
        ``generate``.  ``share_trunk``: sequences that staged the same leading modules read those rows once per step for the
        whole group (``LlamaHIP.slot_loop(share_trunk=True)``); None reads ``PC_SLOT_TRUNK`` (default 0).
        ``lookup`` = k > 0 (None: ``PC_SLOT_LOOKUP``, default 0 = off; the engine's own ``lookup`` is NOT consulted): a
        plain-greedy batch drafts up to k tokens per sequence and step by prompt lookup and verifies them in one
        ``S * (k + 1)``-row step (``LlamaHIP.lookup_slot_loop``); the tokens are greedy decoding's.  Sampled or
        penalised params, a model without that step and ``S * (k + 1) > 64`` run the loop above instead.  k above 15 is
        taken as 15 (a step's draft rows fill one 16-row tile at most).  Up to 8 stop ids end a sequence on the device and a
        stop string is seen by the host, which switches the slot off between replays; with more than 8 stop ids
        ``batch_plan`` runs the sequences one after another, with or without ``lookup``.  Together with
        ``share_trunk`` the lookup step reads a group's shared rows once for all draft rows of the group
        (``LlamaHIP.lookup_slot_loop(share_trunk=True)``) where the model has that step
        (``lookup_trunk_available``) and ``batch_plan`` decodes the batch in a device loop; a refused lookup loop falls back to
        ``slot_loop(share_trunk=True)``.  Anywhere else the combination raises ValueError, as it did before that step existed,
        before anything is asked of the model.
        ``slot_kv`` (None: ``PC_SLOT_KV``, default "fp16"): "int8" decodes over int8 images of the slots' K/V rows
        (``LlamaHIP.slot_loop(kv="int8")``) -- about half the attention's bytes, the format's accuracy, and 0.516 of
        an arena MORE memory per slot.  ValueError with ``share_trunk``, ``lookup`` > 0, head_dim other than 128, a model without
        the slot loop or a batch that is not decoded in the device loop.
        ``keep_arenas=False`` (``serve``'s int8-only residency) raises ValueError here: the callers hand in one live
        arena per sequence, so there is nothing to save.
        ``params.logprobs`` = n covers all sequences: the first tokens through ``LlamaHIP.token_logprobs``, the rest
        from the loop's own node (``slot_loop(logprobs=n)`` / ``lookup_slot_loop(logprobs=n)``); one ``generate`` after another
        keeps them.
        ``params.token_controls`` (``logit_bias``, ``banned_token_ids``, ``allowed_token_ids``, ``min_new_tokens``) cover
        all sequences the same way: the first tokens through ``LlamaHIP.adjust_logits``, the rest through the loop's own node
        (``slot_loop(token_controls=...)``), every slot with the same block."""
        n_lp = modes.check_logprobs(params.logprobs, what="GenerationParameters.logprobs")
        lp_kw = {} if n_lp is None else {"logprobs": n_lp}      # (a model from before the option is handed nothing new)
        requests = [(list(t), list(p), c) for t, p, c in requests]
        hf = getattr(self.lm, "hf_model", None)
        ctl = _controls_of(hf, params)
        if ctl is not None:                                     # (one parameter set: every slot gets the same block)
            lp_kw["token_controls"] = ctl
        # every cache must be a staged batch-1 arena, no two the same
        arenas = [getattr(c, "arena", None) for _, _, c in requests]
        own = all(a is not None and a.B == 1 for a in arenas) and len(set(map(id, arenas))) == len(arenas)
        m = self._batch_modes(len(requests), params, own_arenas=own, share_trunk=share_trunk, lookup=lookup, slot_kv=slot_kv,
                              keep_arenas=keep_arenas)
        if not m.batched:
            full = bool(getattr(self.lm, "use_full_position_ids", False))
            for k, (token_ids, position_ids, cache) in enumerate(requests):
                for out in self.generate(token_ids, position_ids, params, cache, stream_interval, use_full_position_ids=full):
                    yield k, out
            return

        plain_greedy = params.plain_greedy
        seed = 0 if plain_greedy else int(torch.randint(0, 2 ** 62, (1,)))
        seqs = [_Stream(self._render, params, stream_interval, t, max(p) + 1, index=k, seed=seed + k)
                for k, (t, p, _) in enumerate(requests)]
        loop, members, first = None, [], None
        try:
            for st, (token_ids, position_ids, cache) in zip(seqs, requests):
                out = self._first_token(st, token_ids, position_ids, cache)
                if out is not None:
                    yield st.index, out
            members = [st for st in seqs if not st.done]
            if members:
                # the first decoded token sits at position first_free + 1, as in generate
                first = ([st.past for st in members], [st.new_ids[-1] for st in members], [st.first_free + 1 for st in members],
                         members[0].last_step)
                if m.drafts:
                    loop = hf.lookup_slot_loop(*first, m.drafts,
                                               [self._lookup_corpus(requests[st.index][2], requests[st.index][0]) for st in members],
                                               stop_ids=params.stop_token_ids, share_trunk=m.share_trunk, **lp_kw)
                if loop is None:
                    loop = hf.slot_loop(*first, None if plain_greedy else params, [st.seed for st in members],
                                        [st.output_ids for st in members], params.stop_token_ids, share_trunk=m.share_trunk,
                                        **m.loop_kwargs(one_token=True), **lp_kw)
                if loop is None:
                    raise RuntimeError("generate_batch: the model refused a batched decode loop over these caches")
                yield from self._pump_slots(loop, members)
        finally:
            # also when the consumer abandons the generator at a yield: every arena's length goes back to what was consumed
            if loop is not None:
                loop.close([len(st.new_ids) - 1 for st in members])
            del seqs, members, first, st, loop
            gc.collect()

    # -- a stream of requests: continuous batching ------------------------------------------------
    def serve_plan(self, lookup: int = 0, slots: Optional[int] = None, slot_kv: Optional[str] = None,
                   keep_arenas: Optional[bool] = None, loop_prefill: bool = False, token_controls: bool = False) -> Tuple[bool, str]:
        """``(batched, reason)``: whether ``serve`` runs its requests through one device loop that admits new prompts as slots free
        up (``model/llama_hip.py`` SlotLoop, ``each=True``), or one after another through ``generate``, and why.  Host logic only.
        Requests carry their own parameters, so both device loops must be on.  ``lookup`` = k > 0 (``serve(lookup=k)`` over
        ``slots`` slots): the reason also says which form of the loop runs -- the one with prompt-lookup drafts
        (LookupSlotLoop, ``each=True``) or today's one-token loop, and why.  ``slot_kv`` (None: ``PC_SLOT_KV``): with "int8" the
        reason of a batched plan says that the loop reads int8 K/V images, and with ``keep_arenas=False`` (None: not named) that
        no slot keeps an fp16 arena.  ``loop_prefill=True`` (``serve``'s): the reason of a plan in the lookup form says that
        admitted requests are prefilled inside the step; where ``serve`` would refuse the mode (``check_loop_prefill``) this
        raises the same ValueError.  ``token_controls=True`` (``serve``'s): the reason of a batched plan says that the step carries
        the token-control node; together with ``loop_prefill=True`` it raises ``serve``'s ValueError."""
        m = modes.resolve_serve(self._capabilities(True, True), slots, False, int(lookup), slot_kv, keep_arenas, bool(loop_prefill),
                                validate=False,                    # (the plan reads PC_SLOT_KV from the environment, nothing else)
                                token_controls=bool(token_controls))
        return m.batched, m.reason()

    @torch.inference_mode()
    def serve(self, cache_engine, requests, params: Optional[GenerationParameters] = None, stream_interval: int = 2,
              share_trunk: Optional[bool] = None, lookup: Optional[int] = None, slot_kv: Optional[str] = None,
              keep_arenas: Optional[bool] = None, loop_prefill: Optional[bool] = None, logprobs: Optional[int] = None,
              token_controls: Optional[bool] = None) -> Generator[Tuple[int, Output], None, None]:
        """Continuous batching over ``cache_engine.slots`` slots.  ``requests``: any iterable -- it may be lazy -- of ``Prompt`` or
        ``(Prompt, GenerationParameters)``; ``params`` is the default for bare prompts.  Requests are numbered in the order they
        are pulled; yields ``(index, Output)``.  A request is pulled when a slot is free: ``cache_engine.process(prompt, slot=k)``,
        the prefill and the first token as ``generate_batch`` does them, then the sequence enters the running device loop
        (``SlotLoop.admit``) at the next replay, with its own sampling parameters, stop ids and budget.  A sequence that ends --
        stop id, budget, stop string, full arena -- is retired and its slot refilled.  Per sequence the ``Output`` stream, the
        stop-string handling and the position rule are ``generate``'s; sampled request number r uses seed ``seed + r`` of the one
        seed taken from torch's default generator.  A request with more than 8 stop ids keeps the first 8 on the device; the
        host kills the slot for the rest.  ``share_trunk`` (None: ``PC_SLOT_TRUNK``): the first fill is grouped by
        ``common_trunks``; a later request joins a group whose trunk its staged layout covers; the slot of a group's leader is
        not refilled while members live.  The split counts of the attention are fixed from the slot buffers' capacity, so a
        sequence's tokens do not depend on who joins later.  Where ``serve_plan`` says no, the requests run one after another
        through ``generate``.  Abandoning the generator rewinds every arena.  ``last_serve_stats`` / ``last_serve_trace`` /
        ``last_serve_tokens``: replays and live rows, the scheduler's trace and the decoded tokens per request of the newest run.
        ``lookup`` = k > 0 (None: ``PC_SERVE_LOOKUP``, default 0 = off; the engine's own ``lookup`` is NOT consulted; k above 15
        is taken as 15): every sequence drafts up to k tokens per replay by prompt lookup in ``_lookup_corpus`` and its own
        output, and one ``slots * (k + 1)``-row step verifies them with the request's own sampler on every row
        (``LlamaHIP.lookup_slot_loop(each=True)``): on identical logits the tokens are the one-token loop's, sampled
        ones included.  Where the model has no lookup step or ``slots * (k + 1) > 64`` (``serve_plan(lookup, slots)``) today's
        loop runs.  With ``share_trunk`` the step reads a group's shared rows once for all draft rows of the group.  In the
        lookup form ``last_serve_stats`` gains ``tokens`` (decoded in the loop) and ``steps`` (replays).
        ``slot_kv`` (None: ``PC_SLOT_KV``, default "fp16"): ``generate_batch``'s -- "int8" serves over int8 images of the slots' rows,
        sized from ``cache_engine.max_ctx_length``; ValueError where ``serve_plan`` says no.  Together with ``share_trunk`` (DESIGN
        3.33) the one-token loop reads a group's shared rows once per step from the LEADER's image and every slot's own rows from
        its own (``LlamaHIP.slot_loop(each=True, kv="int8", trunks=...)``, ``pc_attn_decode_slots_trunk_q8``); grouping, joining and
        the hold on the leader's slot are ``share_trunk``'s.  ValueError on a model without that step
        (``slot_trunk_q8_available``), with ``lookup`` > 0 (the lookup step over images has no shared-trunk form) and with
        ``keep_arenas=False``.  Together with
        ``lookup`` > 0 the lookup step itself reads the images (``LlamaHIP.lookup_slot_loop(kv="int8")``): every draft
        row attends to the quantised rows in front of it and to its own row exactly, so on identical logits the tokens are
        ``serve(slot_kv="int8")``'s; ValueError on a model without that step (``lookup_slot_q8_available``).
        ``keep_arenas=False`` (None: ``PC_SLOT_KEEP_ARENAS``, default 1; with ``slot_kv="int8"`` only): no slot keeps an
        fp16 arena.  Every request is staged and prefilled in slot 0's buffer, whatever slot the scheduler gives it, its rows are
        quantised into the slot's image as it enters the loop (``SlotLoopQ8Only``) and the buffer is free for the next request;
        the buffers of slots 1.. are never allocated.  The loop is built with the first sequence that has more to decode and the
        rest of the first fill is admitted in front of replay 0.  Tokens are ``slot_kv="int8"``'s.
        ``loop_prefill`` (None: ``PC_SERVE_LOOP_PREFILL``, default 0; with ``lookup`` > 0 in the lookup form only): a
        request admitted into the RUNNING loop is not prefilled on its own -- its new tokens are fed through the k + 1 rows of its
        slot, ``ceil(q / (k + 1))`` replays in which nobody else waits (``LookupSlotLoop.admit_prompt``), and its first token is
        drawn on the device and comes back in the ring; ``ttft_ms`` is then the wall time from admission to that read.  The
        first fill, a request whose position ids are not ``p, p + 1, ...``, one whose question and budget do not fit the draft
        history and one with ``q = 1 mod (k + 1)`` new tokens (its last token would be fed by an ordinary, drafting step, in front of
        the position gap ``generate`` leaves behind a prompt) are prefilled serially, as without the mode.  Question rows are
        appended without the serial prefill's residual tail, so logits differ from the serial flow at the level decoded rows
        already do.  ``last_serve_stats`` gains
        ``loop_prefills`` (requests prefilled inside the loop) and ``step_prefills`` (requests prefilled by a step of their
        own).  ValueError without the lookup form and with ``slot_kv="int8"``.
        ``logprobs`` = n in 0..8 (None: ``PC_SERVE_LOGPROBS``, unset: off): the requests are lazy and the step is
        captured once, so the capacity is a mode of the loop -- its step carries the log-probability node at ``top_n = n``.  A
        request whose ``params.logprobs`` is m <= n gets m alternatives per token, one with None gets ``Output.logprobs = None``, and
        one that asks for more than n -- or asks at all while this is off -- raises ValueError naming ``serve(logprobs=...)`` before
        its prefill.  Works with ``lookup``, ``share_trunk``, ``slot_kv="int8"`` and ``keep_arenas=False``; ValueError together with
        ``loop_prefill`` (``modes.check_logprobs``: a request admitted that way draws its first token inside the step from a forced
        row).
        ``token_controls`` (None: ``PC_SERVE_TOKEN_CONTROLS``, default 0): the step is captured once, so the
        token-control node is a mode of the loop -- with it the step runs ``pc_logit_adjust`` in front of its draw, every slot under
        the block of the request it holds (``logit_bias``, ``banned_token_ids``, ``allowed_token_ids``, ``min_new_tokens`` of its own
        ``GenerationParameters``; a request without controls gets the neutral block, written at admission like any other, so nothing
        of the slot's previous request stays).  A request that carries controls while the mode is off raises ValueError naming
        ``serve(token_controls=...)`` before its prefill.  Works with ``lookup``, ``share_trunk``, ``slot_kv="int8"``,
        ``keep_arenas=False`` and ``logprobs`` (which stay the raw rows'); ValueError together with ``loop_prefill``
        (``modes.check_token_controls``: the progress word also counts forced question rows there)."""
        m = modes.resolve_serve(self._capabilities(True, True), getattr(cache_engine, "slots", None), share_trunk, lookup, slot_kv,
                                keep_arenas, loop_prefill, logprobs=logprobs, token_controls=token_controls)
        hf = getattr(self.lm, "hf_model", None)
        share_trunk, drafts, drop, in_loop = m.share_trunk, m.drafts, not m.keep_arenas, m.loop_prefill

        def unpack(req):
            """-> (prompt, params) of a request; its ``logprobs`` must fit what the loop was built for."""
            prompt, p = (req[0], req[1] if req[1] is not None else params) if isinstance(req, (tuple, list)) else (req, params)
            want = None if p is None else modes.check_logprobs(getattr(p, "logprobs", None), what="GenerationParameters.logprobs")
            if want is not None and (m.logprobs is None or want > m.logprobs):
                raise ValueError(f"serve: a request asks for logprobs={want}, and the loop "
                                 + ("carries no log-probability node" if m.logprobs is None else f"ranks {m.logprobs} alternatives")
                                 + f": call serve(logprobs=n) with n >= {want} (or set PC_SERVE_LOGPROBS)")
            if p is not None and _controls_of(hf, p, m.loop_prefill) is not None and not m.token_controls:
                raise ValueError("serve: a request carries token controls (logit_bias, banned_token_ids, allowed_token_ids or "
                                 "min_new_tokens) and the loop has no token-control node: call serve(token_controls=True) (or set "
                                 "PC_SERVE_TOKEN_CONTROLS=1)")
            return prompt, p

        if not m.batched:
            full = bool(getattr(self.lm, "use_full_position_ids", False))
            for r, req in enumerate(requests):
                prompt, p = unpack(req)
                ids, pos, _, cache = cache_engine.process(prompt, return_full_position_ids=full)
                for out in self.generate(ids, pos, p, cache, stream_interval, use_full_position_ids=full):
                    yield r, out
            return

        S = cache_engine.slots
        sched = SlotScheduler(S, requests, share_trunk=share_trunk)    # (drafts = k > 0: the lookup form, serve_plan(lookup, S))
        stats = self.last_serve_stats = dict(replays=0, rows=0, live_rows=0, requests=0)
        if drafts:
            stats.update(tokens=0, steps=0)
        if in_loop:
            stats.update(loop_prefills=0, step_prefills=0)
        self.last_serve_trace = sched.trace
        tokens = self.last_serve_tokens = {}          # request index -> the tokens it decoded
        seq = {}            # slot -> stream of the running sequence
        loop, seed, read_k = None, None, 0
        pending: list = []  # first fill: sequences waiting for the loop to be built

        def loop_args(st):
            return (st.past, st.new_ids[-1], st.first_free + 1, st.last_step, None if st.params.plain_greedy else st.params, st.seed,
                    st.output_ids, st.device_stops)

        def admit_free_slots():
            """Pull requests into free slots: process, prefill and first token; sequences with more to decode enter the loop (or
            wait for it to be built).  ``drop``: everything runs in slot 0's buffer, so nobody can wait: the first such sequence
            builds the loop, and a sequence that has entered lets go of the buffer."""
            nonlocal seed
            while True:
                nxt = sched.next_request()
                if nxt is None:
                    return
                index, slot, req = nxt
                stats["requests"] += 1
                prompt, p = unpack(req)
                if p is None:
                    raise ValueError("serve: a bare prompt needs the default params")
                ids, pos, _, cache = cache_engine.process(prompt, slot=0 if drop else slot)
                if not p.plain_greedy and seed is None:
                    seed = int(torch.randint(0, 2 ** 62, (1,)))
                st = _Stream(self._render, p, stream_interval, ids, max(pos) + 1, index=index, slot=slot,
                             seed=0 if p.plain_greedy else seed + index, device_stops=split_stop_ids(p.stop_token_ids)[0])
                tokens[index] = st.new_ids
                st.ctl = _controls_of(hf, p)
                if in_loop and loop is not None and admit_prompt(st, list(ids), list(pos), cache):
                    continue
                if in_loop:
                    stats["step_prefills"] += 1
                out = self._first_token(st, list(ids), list(pos), cache)
                if drafts:
                    st.corpus = self._lookup_corpus(cache, ids)        # (behind the prefill: the staged layout is carried out)
                if out is not None:
                    yield index, out
                if st.done:
                    sched.dropped(slot, index, 0 if loop is None else loop.n)
                    continue
                if loop is None:
                    pending.append(st)
                    sched.started(slot, index, 0)
                    if drop:
                        build_loop()
                else:
                    trunk = sched.join(slot, st.past.arena.layout) if share_trunk and loop.nsplit_trunk else None
                    st.k = loop.admit(slot, *loop_args(st), *((st.corpus,) if read_k else ()), trunk=trunk,
                                      **({"controls": st.ctl} if m.token_controls else {}))
                    sched.started(slot, index, loop.n)
                if drop:
                    st.past = cache = None                         # (the loop holds the rows; the buffer is the next request's)
                seq[slot] = st

        def admit_prompt(st, ids, pos, cache) -> bool:
            """``loop_prefill``: the request goes into the running loop unprefilled (``LookupSlotLoop.admit_prompt``) -- where its
            positions are contiguous, question and budget fit the draft history and q is not 1 mod (k + 1): such a question's
            last token is fed by an ordinary step, whose drafts would sit at positions without the gap ``generate`` leaves in
            front of the first decoded token.  False: it takes the serial path."""
            q, p = len(ids), st.params
            if not (getattr(loop, "prompt_rows", False) and q % (loop.k + 1) != 1 and p.max_new_tokens >= 1
                    and pos == list(range(pos[0], pos[0] + q))
                    and q + p.max_new_tokens <= loop.hist_cap and getattr(cache, "arena", None) is not None):
                return False
            st.t_admit = time.perf_counter()
            cache.arena.materialize()                              # (the staged layout is carried out: the trunk rows are there)
            trunk = sched.join(st.slot, cache.arena.layout) if share_trunk and loop.nsplit_trunk else None
            # the first decoded token sits at position first_free + 1, as behind a serial prefill: one behind the question's end
            st.k = loop.admit_prompt(st.slot, cache, ids, pos[0], p.max_new_tokens, None if p.plain_greedy else p, st.seed,
                                     st.output_ids, st.device_stops, self._lookup_corpus(cache, []), trunk=trunk, decode_gap=1)
            st.past = cache
            stats["loop_prefills"] += 1
            sched.started(st.slot, st.index, loop.n)
            seq[st.slot] = st
            return True

        def build_loop():
            """The ``each=True`` loop over the sequences waiting in ``pending``."""
            nonlocal loop, read_k
            slots_ = [st.slot for st in pending]
            trunks = sched.group_first_fill(slots_, [st.past.arena.layout for st in pending]) if share_trunk else None
            # (loop_args per sequence -> one list per argument)
            pasts, toks0, poss, max_news, paramss, seeds_, hists, stops = map(list, zip(*map(loop_args, pending)))
            ctl_kw = {"token_controls": [st.ctl for st in pending]} if m.token_controls else {}    # (on: one block, or None, per sequence)
            if drafts:
                loop = hf.lookup_slot_loop(pasts, toks0, poss, max_news, drafts, [st.corpus for st in pending], stop_ids=stops,
                                           slots=S, max_keys=cache_engine.max_ctx_length, trunks=trunks, each=True,
                                           slot_index=slots_, params=paramss, seeds=seeds_, histories=hists,
                                           hist_cap=2 * cache_engine.max_ctx_length, **{**m.loop_kwargs(), **ctl_kw})
            if loop is None:
                loop = hf.slot_loop(pasts, toks0, poss, max_news, paramss, seeds_, hists, stops, slots=S, slot_index=slots_, each=True,
                                    max_keys=cache_engine.max_ctx_length, trunks=trunks, **{**m.loop_kwargs(one_token=True), **ctl_kw})
            if loop is None:
                raise RuntimeError("serve: the model refused a batched decode loop over these caches")
            read_k = _reader(loop)[1]                              # (keep_arenas=False admits the rest of the first fill at once)
            for k, st in enumerate(pending):
                st.k = k
            pending.clear()

        try:
            yield from admit_free_slots()
            if pending:
                build_loop()
            i = 0
            if loop is not None:
                read, read_k = _reader(loop)                       # (one read loop for k = 0 and k > 0)
            while seq:
                # the look-ahead rule of _pump_slots over sequences that start at different replays (slot_scheduler.wants_look_ahead):
                # the step in flight cannot exhaust a budget -- a sequence has room for more than its k + 1 tokens
                while loop.n <= i:
                    loop.enqueue()
                # (loop_prefill: a sequence "starts" at the replay that draws its first token; the replays in front feed its question)
                first = loop.first_step if in_loop and hasattr(loop, "first_step") else loop._start.__getitem__
                if loop.n == i + 1 and wants_look_ahead(
                        [(first(st.k), st.last_step - (len(st.new_ids) - 1)) for st in seq.values()], i, read_k):
                    loop.enqueue()                                 # the replay AFTER the one whose tokens are read below
                ms = loop.elapsed_ms(i)
                stats["rows"] += S
                for slot in sorted(seq):
                    st = seq[slot]
                    if first(st.k) > i:
                        continue
                    toks = read(st.k, i)
                    outs = []
                    if not toks:                                   # (the device switched the slot off: its arena is full)
                        st.done = True
                    else:
                        stats["live_rows"] += 1
                        st.total_ms += ms
                        if not st.new_ids:                         # (loop_prefill: the first token, from the ring)
                            st.ttft_ms = st.total_ms = (time.perf_counter() - st.t_admit) * 1e3
                        lps = loop.logprobs(st.k, i) if st.lps is not None else None
                        for t, token in enumerate(toks):
                            out = st.emit(token, None if lps is None else lps[t])
                            if read_k:
                                stats["tokens"] += 1
                            if out is not None:
                                outs.append(out)
                            if st.ended_on_the_host(token):
                                loop.kill(st.k)                    # a stop string or a stop id past the first 8
                            if st.done:                            # (the rest of the step lies behind the sequence's end)
                                break
                    if st.done:
                        loop.retire(st.k, len(st.new_ids) - 1)     # the TOKENS consumed (= the replays of a one-token loop)
                        del seq[slot]
                        st.past = None
                        sched.finished(slot, i)
                    for out in outs:
                        yield st.index, out
                yield from admit_free_slots()
                i += 1
        finally:
            # also when the consumer abandons the generator at a yield: every arena's length goes back to what was consumed
            if loop is not None:
                stats["replays"] = loop.n
                if drafts:
                    stats["steps"] = loop.n
                loop.close({st.k: len(st.new_ids) - 1 for st in seq.values() if st.k is not None})
            del seq, loop, pending
            gc.collect()
