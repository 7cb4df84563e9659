"""Modes of the model and of the batched loops: which formats and combinations run, where each default comes from, and the ONE
resolution behind ``GenerationEngine.serve`` / ``serve_plan`` / ``generate_batch`` / ``batch_plan``.

Pure host logic -- no torch, no native library: the ``check_*`` functions raise ``ValueError`` naming the conflict before anything is
read, drawn or allocated, ``resolve_serve`` / ``resolve_batch`` turn a caller's arguments, the environment and what the model
offers (``Capabilities``) into one frozen ``Modes`` record, calling the checks in the order the entry points always did."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Mapping, Optional


# ---- the model's weights ----------------------------------------------------------------------------------------------------------
WEIGHT_FORMATS = ("fp16", "mxfp4")


def check_weight_format(weight_format: str, int8_weights: bool, shape=None, llama: bool = True) -> None:
    """``ValueError`` for a weight format this model cannot load -- raised before anything is allocated."""
    if weight_format not in WEIGHT_FORMATS:
        raise ValueError(f"weight_format must be one of {WEIGHT_FORMATS}, not {weight_format!r}")
    if weight_format != "mxfp4":
        return
    if not llama:
        raise ValueError("weight_format='mxfp4' is implemented for the Llama family only (not Falcon / MPT)")
    if int8_weights:
        raise ValueError("weight_format='mxfp4' and load_in_8bit / int8_weights exclude each other")
    dims = (("hidden_size", shape.hidden_size), ("intermediate_size", shape.intermediate_size),
            ("num_attention_heads * head_dim", shape.num_attention_heads * shape.head_dim))
    for name, v in dims:
        if v % 128:
            raise ValueError(f"weight_format='mxfp4' needs {name} to be a multiple of 128 (a 16-byte lane load of the 4-bit "
                             f"image is four 32-feature MX blocks); {name} = {v}")


def _parse_01(name: str, value) -> bool:
    """A ``0`` / ``1`` variable whose default is on: unset, empty or ``1`` -> True, ``0`` -> False, anything else ``ValueError``."""
    if value is None or value in ("", "1"):
        return True
    if value == "0":
        return False
    raise ValueError(f"{name} must be 0 or 1, not {value!r}")


def parse_keep_fp16(value) -> bool:
    """``PC_W4_KEEP_FP16``: unset, empty or ``1`` keeps the fp16 images of an MXFP4 model's decoder linears, ``0`` drops them."""
    return _parse_01("PC_W4_KEEP_FP16", value)


def check_keep_fp16(keep_fp16, weight_format: str, env=None) -> bool:
    """The ``keep_fp16`` a model runs with: the argument, else ``PC_W4_KEEP_FP16`` for an MXFP4 model, else True.  ``ValueError``
    for a combination in which dropping the fp16 images leaves a path without weights -- raised before anything is allocated."""
    env = os.environ if env is None else env
    if keep_fp16 is None:
        keep_fp16 = parse_keep_fp16(env.get("PC_W4_KEEP_FP16")) if weight_format == "mxfp4" else True
    if keep_fp16:
        return True
    if weight_format != "mxfp4":
        raise ValueError(f"keep_fp16=False needs weight_format='mxfp4' (the fp16 images are all a weight_format={weight_format!r} "
                         "model has)")
    if env.get("PC_W4_STREAM", "1") == "0":
        raise ValueError("keep_fp16=False and PC_W4_STREAM=0 exclude each other: PC_W4_STREAM=0 builds no 4-bit images, so nothing "
                         "would be left to expand")
    if env.get("PC_DENSE_LO8", "0") == "1":
        raise ValueError("keep_fp16=False and PC_DENSE_LO8=1 exclude each other: the int8 residual-plane GEMM keeps int8 images of the "
                         "fp16 weights")
    return False


# ---- the batched loops ------------------------------------------------------------------------------------------------------------
SLOT_KV = ("fp16", "int8")


def check_slot_kv(kv: str, share_trunk: bool = False, lookup: int = 0, head_dim: Optional[int] = None, no_loop: Optional[str] = None,
                  not_batched: Optional[str] = None, lookup_q8: bool = False, trunk_q8: bool = False) -> None:
    """``ValueError`` naming the conflict for a ``slot_kv`` / ``kv`` mode the batched decode loop cannot run -- raised before
    anything is allocated.  Pure.  ``no_loop``: why the model has no slot loop (Falcon / MPT, ``load_in_8bit``,
    ``PC_DECODE_TAIL=1``), ``not_batched``: why ``batch_plan`` / ``serve_plan`` would not decode this batch in the device loop
    (None: they would).  ``lookup_q8``: the caller is ``serve`` / ``lookup_slot_loop`` and the model has the lookup step over
    int8 images (``lookup_slot_q8_available``) -- ``lookup > 0`` is then no conflict.  ``trunk_q8``: the caller is
    ``serve`` / ``slot_loop(each=True)`` and the model has the shared-trunk attention over int8 images
    (``slot_trunk_q8_available``) -- ``share_trunk`` is then no conflict in the one-token loop (``lookup`` 0); the
    lookup step over images has no shared-trunk form."""
    if kv not in SLOT_KV:
        raise ValueError(f"slot_kv must be one of {SLOT_KV}, not {kv!r}")
    if kv != "int8":
        return
    if share_trunk and not trunk_q8:
        raise ValueError("slot_kv='int8' and share_trunk exclude each other (the shared-trunk attention reads the leader's fp16 "
                         "arena; int8 images under share_trunk are not implemented)")
    if share_trunk and int(lookup) > 0:
        raise ValueError("slot_kv='int8', share_trunk and lookup > 0 exclude each other (the lookup step over int8 images has no "
                         "shared-trunk form; share_trunk over images is the one-token loop's, pc_attn_decode_slots_trunk_q8)")
    if int(lookup) > 0 and not lookup_q8:
        raise ValueError("slot_kv='int8' and lookup > 0 exclude each other (the k + 1 row verify step reads the fp16 arenas; "
                         "int8 images under lookup are not implemented)")
    if no_loop is not None:
        raise ValueError(f"slot_kv='int8' needs the batched decode loop, which this model does not have: {no_loop}")
    if head_dim is not None and head_dim != 128:
        raise ValueError(f"slot_kv='int8' is implemented for head_dim 128 only (pc_attn_decode_slots_q8); head_dim = {head_dim}")
    if not_batched is not None:
        raise ValueError(f"slot_kv='int8' needs a batch decoded in the device loop, and this one is not: {not_batched}")


def check_loop_prefill(loop_prefill: bool, drafts: int, kv: str = "fp16", why: Optional[str] = None) -> None:
    """``ValueError`` naming the conflict for ``serve(loop_prefill=True)`` where it cannot run -- raised before anything is
    allocated.  Pure.  ``drafts``: the k ``serve`` runs the lookup form with (``Modes.drafts``; 0: it does not, ``why`` says
    why where there is a reason beyond ``lookup`` being off)."""
    if not loop_prefill:
        return
    if int(drafts) <= 0:
        raise ValueError("loop_prefill=True needs the lookup form of the serving loop (serve(lookup=k), k > 0: a question is fed "
                         "through the k draft rows of the step), and it does not run: " + (why or "lookup is off"))
    if kv == "int8":
        raise ValueError("loop_prefill=True and slot_kv='int8' exclude each other (question rows are appended as fp16 rows; "
                         "forced rows over int8 images are not implemented)")


def check_slot_keep_arenas(keep_arenas: bool, kv: str, generate_batch: bool = False, share_trunk: bool = False) -> None:
    """``ValueError`` for ``keep_arenas=False`` (int8-only slot residency) where it cannot run -- raised before anything
    is allocated, behind ``check_slot_kv``'s own refusals of ``kv``.  Pure.  ``share_trunk`` (``serve``'s, over int8 images): the
    one-buffer prefill builds the loop from a single sequence, so no group is founded."""
    if keep_arenas:
        return
    if share_trunk and kv == "int8":
        raise ValueError("keep_arenas=False and share_trunk exclude each other under slot_kv='int8': the one-buffer prefill builds "
                         "the loop from a single sequence, so no group is founded in the first fill (share_trunk over int8 images "
                         "keeps the fp16 slot arenas)")
    if generate_batch:
        raise ValueError("keep_arenas=False is not for generate_batch: its callers hand in one live fp16 arena per sequence, so "
                         "there is nothing to save; serve(slot_kv='int8', keep_arenas=False) prefills every request in one arena")
    if kv != "int8":
        raise ValueError(f"keep_arenas=False needs slot_kv='int8' (without the int8 images the fp16 arenas are the only K/V a "
                         f"slot has); slot_kv = {kv!r}")


LOGPROBS_MAX_TOP = 8         # PC_LOGPROBS_MAX_TOP: the most alternatives pc_token_logprobs ranks per token


def check_logprobs(logprobs, loop_prefill: bool = False, what: str = "logprobs") -> Optional[int]:
    """The ``logprobs`` a call runs with: None (off), or n in 0..8 -- the chosen token's log-probability plus the n most likely
    alternatives, under the model's own distribution.  ``ValueError`` for anything else and for ``loop_prefill=True`` together with
    it -- raised before anything runs.  Pure."""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= LOGPROBS_MAX_TOP:
        raise ValueError(f"{what} must be None or an integer in 0..{LOGPROBS_MAX_TOP} (the alternatives per token), not {logprobs!r}")
    if loop_prefill:
        raise ValueError("loop_prefill=True and logprobs exclude each other: the first token of a request admitted that way is drawn "
                         "inside the step from a forced row, whose record the step's log-probability node does not hand out "
                         "(loop_prefill with logprobs is not implemented)")
    return int(logprobs)


def parse_logprobs(value) -> Optional[int]:
    """``PC_SERVE_LOGPROBS``: unset or empty is off, else the n of ``serve(logprobs=n)``."""
    if value is None or value == "":
        return None
    try:
        return int(value)
    except ValueError:
        raise ValueError(f"PC_SERVE_LOGPROBS must be an integer in 0..{LOGPROBS_MAX_TOP}, not {value!r}") from None


# ---- token controls: logit_bias, banned / allowed ids, min_new_tokens -------------------------------------------------
LOGIT_BIAS_MAX = 64          # PC_LOGIT_BIAS_MAX: distinct ids of the merged bias table (logit_bias and banned_token_ids)
LOGIT_STOP_MAX = 8           # PC_LOGIT_STOP_MAX: stop ids min_new_tokens can hold back (what the device loops hold)
_INF = float("inf")


@dataclass(frozen=True)
class TokenControls:
    """The merged, validated token controls of one request, as ``pc_logit_adjust`` takes them: ``bias`` = ``((id, value), ...)`` by
    id, a ban being ``-inf``; ``allowed`` = the sorted ids that may be drawn (None: all); the ids in ``stop_ids`` are ``-inf`` for the
    generated tokens numbered ``g < min_new_tokens`` (``g = 0``: the token drawn from the prefill)."""
    bias: tuple = ()                   # ((id, value), ...)
    allowed: Optional[tuple] = None    # (id, ...)
    min_new_tokens: int = 0
    stop_ids: tuple = ()

    def max_id(self) -> int:
        return max([i for i, _ in self.bias] + list(self.allowed or ()) + list(self.stop_ids) + [-1])


def _token_ids(ids, what: str) -> list:
    out = []
    for i in ids:
        if isinstance(i, bool) or not isinstance(i, int) or i < 0:
            raise ValueError(f"{what} holds {i!r}: token ids are non-negative integers")
        out.append(int(i))
    return out


def token_controls(logit_bias=None, banned_token_ids=None, allowed_token_ids=None, min_new_tokens: int = 0, stop_token_ids=(),
                   vocab: Optional[int] = None) -> Optional[TokenControls]:
    """``GenerationParameters``' four token-control fields, merged and validated -> ``TokenControls``, or None when all four are
    vacuous (nothing to bias or ban, no allow-list, no stop id to hold back).  ``ValueError``: a bias that is NaN or ``+inf``, an id
    that is no non-negative integer (with ``vocab``: one outside the vocabulary), more than 64 distinct biased or banned ids, a
    negative ``min_new_tokens``, ``min_new_tokens > 0`` with more than 8 stop ids, and a set of tokens that can still be drawn --
    allowed minus banned, minus the stop ids while ``min_new_tokens > 0`` -- that is empty.  A ban wins over a finite bias on the
    same id.  Pure."""
    table = {}
    for i, v in (logit_bias or {}).items():
        (i,) = _token_ids([i], "logit_bias")
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v == _INF:
            raise ValueError(f"logit_bias[{i}] = {v!r}: a bias is finite, or -inf (a ban)")
        table[i] = float(v)
    for i in _token_ids(banned_token_ids or (), "banned_token_ids"):
        table[i] = -_INF
    if len(table) > LOGIT_BIAS_MAX:
        raise ValueError(f"logit_bias and banned_token_ids name {len(table)} distinct ids, more than LOGIT_BIAS_MAX = {LOGIT_BIAS_MAX}")
    allowed = None if allowed_token_ids is None else tuple(sorted(set(_token_ids(allowed_token_ids, "allowed_token_ids"))))
    if isinstance(min_new_tokens, bool) or not isinstance(min_new_tokens, int) or min_new_tokens < 0:
        raise ValueError(f"min_new_tokens must be a non-negative integer, not {min_new_tokens!r}")
    stops = tuple(sorted(set(int(t) for t in stop_token_ids))) if min_new_tokens > 0 else ()
    if len(stops) > LOGIT_STOP_MAX:
        raise ValueError(f"min_new_tokens > 0 holds back at most {LOGIT_STOP_MAX} stop token ids (what a device loop holds), "
                         f"not {len(stops)}")
    stops = tuple(t for t in stops if t >= 0)
    ctl = TokenControls(tuple(sorted(table.items())), allowed, int(min_new_tokens) if stops else 0, stops)
    if not ctl.bias and ctl.allowed is None and not ctl.stop_ids:
        return None
    check_token_controls(ctl, vocab=vocab)
    return ctl


def check_token_controls(controls: Optional[TokenControls], loop_prefill: bool = False, vocab: Optional[int] = None,
                         n_stop_ids: int = 0) -> Optional[TokenControls]:
    """What ``token_controls`` cannot know when the parameters are made: ``ValueError`` for an id outside ``[0, vocab)`` once the
    vocabulary is known, for an empty set of drawable tokens, for ``loop_prefill=True`` together with controls, and for more than 8
    stop ids (``n_stop_ids``) together with ``min_new_tokens > 0`` -- raised before anything runs.  None passes.  Pure."""
    if controls is None:
        return None
    if loop_prefill:
        raise ValueError("loop_prefill=True and token controls (logit_bias, banned_token_ids, allowed_token_ids, min_new_tokens) "
                         "exclude each other: the progress word min_new_tokens counts from, the slot's arena length, also counts "
                         "the forced question rows there (loop_prefill with token controls is not implemented)")
    if controls.min_new_tokens > 0 and max(n_stop_ids, len(controls.stop_ids)) > LOGIT_STOP_MAX:
        raise ValueError(f"min_new_tokens > 0 holds back at most {LOGIT_STOP_MAX} stop token ids, not {max(n_stop_ids, len(controls.stop_ids))}")
    if vocab is not None and controls.max_id() >= vocab:
        raise ValueError(f"token controls name id {controls.max_id()}, outside the vocabulary [0, {vocab})")
    gone = {i for i, v in controls.bias if v == -_INF} | set(controls.stop_ids)
    if controls.allowed is not None:
        left = len(set(controls.allowed) - gone)
    else:
        left = 1 if vocab is None else vocab - len(gone)
    if left < 1:
        raise ValueError("token controls leave no token that can be drawn (allowed_token_ids minus banned ids"
                         + (", minus the stop ids while min_new_tokens > 0" if controls.stop_ids else "") + " is empty)")
    return controls


def parse_token_controls(value) -> bool:
    """``PC_SERVE_TOKEN_CONTROLS``: unset, empty or ``0`` is off, ``1`` on."""
    if value is None or value in ("", "0"):
        return False
    if value == "1":
        return True
    raise ValueError(f"PC_SERVE_TOKEN_CONTROLS must be 0 or 1, not {value!r}")


def parse_keep_arenas(value) -> bool:
    """``PC_SLOT_KEEP_ARENAS``: unset, empty or ``1`` keeps the fp16 slot arenas under ``slot_kv="int8"``, ``0`` drops them."""
    return _parse_01("PC_SLOT_KEEP_ARENAS", value)


# ---- one resolution for the engine's entry points ------------------------------------------------------------------------------
MAX_BATCH = 16        # sequences of one generate_batch loop
MAX_ROWS = 64         # rows of one step of the weight-streaming projections: slots * (k + 1) of the lookup form


@dataclass(frozen=True)
class Capabilities:
    """What the engine needs to know about a model to choose a loop (``GenerationEngine._capabilities`` asks, once per call).
    A model that lacks a method does not have the step."""
    no_loop: Optional[str] = None       # why the model has no batched loop (None: it has one)
    not_batched: Optional[str] = None   # ``no_loop``, else the PC_DEVICE_GREEDY / PC_DEVICE_SAMPLE switch that keeps this call off it
    lookup_loop: bool = False           # it has ``lookup_slot_loop``: generate_batch tries it and falls back where it gives None ...
    lookup: bool = False                # ... and says ``lookup_available()``: serve decides the form of its loop up front
    lookup_q8: bool = False             # the lookup step over int8 images (``lookup_slot_q8_available``)
    lookup_trunk: bool = False          # the shared-trunk verify step (``lookup_trunk_available``)
    head_dim: Optional[int] = None
    trunk_q8: bool = False              # the shared-trunk attention over int8 images (``slot_trunk_q8_available``)


@dataclass(frozen=True, kw_only=True)
class _ModeSwitches:
    """The keyword-only part of ``Modes``: a base class, so that its fields neither move a positional argument of ``Modes(...)`` nor
    come behind ``logprobs``, the last field of the record."""
    token_controls: bool = False       # serve: the step carries the token-control node in front of its draw


@dataclass(frozen=True)
class Modes(_ModeSwitches):
    """What ``serve`` / ``generate_batch`` run with, resolved once.  ``batched``: one device loop (False: one ``generate`` after the
    other) and ``base`` says why or which form; ``drafts`` = k > 0: the lookup form (``no_drafts``: why not, None where ``lookup`` is
    off, ``serve`` only); ``lookup`` is the k asked for, in ``serve`` 15 at most."""
    batched: bool
    base: str
    share_trunk: bool = False
    lookup: int = 0
    drafts: int = 0
    no_drafts: Optional[str] = None
    slot_kv: str = "fp16"
    keep_arenas: bool = True
    loop_prefill: bool = False
    logprobs: Optional[int] = None     # serve: the step carries the log-probability node at top_n = logprobs (None: it does not)

    def reason(self) -> str:
        """The plan's text: ``base`` and one clause per mode that is on."""
        why = self.base
        if self.loop_prefill:
            why += ", requests admitted into the running loop are prefilled inside its step (loop_prefill=True)"
        if self.batched and self.slot_kv == "int8":
            why += ", K/V read from int8 images (slot_kv='int8')"
            if not self.keep_arenas:
                why += ", no fp16 slot arenas: every prefill runs in one shared arena (keep_arenas=False)"
        if self.batched and self.logprobs is not None:
            why += f", per-token log-probabilities with up to {self.logprobs} alternatives (logprobs={self.logprobs})"
        if self.batched and self.token_controls:
            why += ", per-request logit_bias / banned / allowed ids / min_new_tokens applied in front of the draw (token_controls=True)"
        return why

    def loop_kwargs(self, one_token: bool = False) -> dict:
        """What ``lookup_slot_loop`` (``one_token``: ``slot_loop``, which has no question rows) is handed beyond the fp16 defaults:
        a mode that is off passes nothing, so a model from before the mode existed still serves."""
        kw = {}
        if self.slot_kv != "fp16":
            kw["kv"] = self.slot_kv
        if not self.keep_arenas:
            kw["keep_arenas"] = False
        if self.loop_prefill and not one_token:
            kw["prompt_rows"] = True
        if self.logprobs is not None:
            kw["logprobs"] = self.logprobs
        if self.token_controls:
            kw["token_controls"] = True
        return kw


def _serve_drafts(caps: Capabilities, lookup: int, slots: Optional[int]):
    """``(k, None)``: serve over ``slots`` slots runs the lookup form with k drafts per sequence and replay (k above 15 is taken as
    15); ``(0, why)``: it runs the one-token loop (``why`` None: ``lookup`` is off)."""
    k = min(int(lookup), 15)
    if k <= 0:
        return 0, None
    if not caps.lookup:
        return 0, "the model has no lookup step"
    if slots is not None and int(slots) * (k + 1) > MAX_ROWS:
        return 0, f"{int(slots)} slots x (k + 1 = {k + 1}) rows exceed the {MAX_ROWS} rows of the weight-streaming projections"
    return k, None


def resolve_serve(caps: Capabilities, slots: Optional[int] = None, share_trunk: Optional[bool] = None, lookup: Optional[int] = None,
                  slot_kv: Optional[str] = None, keep_arenas: Optional[bool] = None, loop_prefill: Optional[bool] = None,
                  env: Optional[Mapping[str, str]] = None, validate: bool = True, logprobs: Optional[int] = None,
                  token_controls: Optional[bool] = None) -> Modes:
    """``serve``'s modes over ``slots`` slots (None: not known, no row limit applies).  An argument that is None reads the
    environment: ``PC_SLOT_TRUNK`` (default 0), ``PC_SERVE_LOOKUP`` (0), ``PC_SLOT_KV`` ("fp16"), ``PC_SLOT_KEEP_ARENAS`` (1),
    ``PC_SERVE_LOOP_PREFILL`` (0), ``PC_SERVE_LOGPROBS`` (unset: off), ``PC_SERVE_TOKEN_CONTROLS`` (0).  Refusals, in this order:
    ``check_slot_kv``, ``check_slot_keep_arenas``, ``check_loop_prefill``, ``check_logprobs``, ``token_controls`` with
    ``loop_prefill``.
    ``validate=False`` is ``serve_plan``'s reading: ``slot_kv`` is taken as it comes and ``keep_arenas`` None means "not named"
    -- neither is checked and ``PC_SLOT_KEEP_ARENAS`` is not read -- while ``loop_prefill=True`` is refused as in ``serve``."""
    env = os.environ if env is None else env
    if share_trunk is None:
        share_trunk = env.get("PC_SLOT_TRUNK", "0") == "1"
    lookup = min(int(env.get("PC_SERVE_LOOKUP", "0")) if lookup is None else int(lookup), 15)
    kv = env.get("PC_SLOT_KV", "fp16") if slot_kv is None else slot_kv
    batched = caps.not_batched is None
    drafts, no_drafts = _serve_drafts(caps, lookup, slots) if batched else (0, caps.not_batched)
    if validate and kv != "fp16":
        check_slot_kv(kv, share_trunk=bool(share_trunk), lookup=lookup, head_dim=caps.head_dim, no_loop=caps.no_loop,
                      not_batched=caps.not_batched, lookup_q8=caps.lookup_q8, trunk_q8=caps.trunk_q8)
    if keep_arenas is None:
        keep_arenas = parse_keep_arenas(env.get("PC_SLOT_KEEP_ARENAS")) if validate else True
    if validate:
        check_slot_keep_arenas(bool(keep_arenas), kv, share_trunk=bool(share_trunk))
    if loop_prefill is None:
        loop_prefill = env.get("PC_SERVE_LOOP_PREFILL", "0") == "1"
    check_loop_prefill(bool(loop_prefill), drafts, kv, no_drafts)
    if logprobs is None:
        logprobs = parse_logprobs(env.get("PC_SERVE_LOGPROBS"))
    logprobs = check_logprobs(logprobs, bool(loop_prefill), "serve(logprobs=...) / PC_SERVE_LOGPROBS")
    if token_controls is None:
        token_controls = parse_token_controls(env.get("PC_SERVE_TOKEN_CONTROLS"))
    if token_controls:
        check_token_controls(TokenControls(), bool(loop_prefill))
    if not batched:
        base = caps.not_batched
    elif drafts:
        base = (f"one device loop with prompt-lookup drafts (lookup, k = {drafts}): up to k + 1 tokens per sequence and replay, "
                "new prompts admitted as slots free up")
    elif no_drafts is not None:
        base = "one device loop, one token per replay: " + no_drafts
    else:
        base = "one device loop, new prompts admitted as slots free up"
    return Modes(batched, base, bool(share_trunk), lookup, drafts, no_drafts, kv, bool(keep_arenas), bool(loop_prefill), logprobs,
                 token_controls=bool(token_controls))


def resolve_batch(caps: Capabilities, n_requests: int, plain_greedy: bool = True, n_stop_ids: int = 0, max_new_tokens: int = 2,
                  own_arenas: bool = True, share_trunk: Optional[bool] = None, lookup: Optional[int] = None,
                  slot_kv: Optional[str] = None, keep_arenas: Optional[bool] = None, env: Optional[Mapping[str, str]] = None,
                  validate: bool = True) -> Modes:
    """``generate_batch``'s modes for ``n_requests`` sequences of one ``GenerationParameters`` (``plain_greedy``, ``n_stop_ids``,
    ``max_new_tokens``); ``own_arenas``: every cache is a staged batch-1 arena, no two the same.  An argument that is None reads
    the environment: ``PC_SLOT_TRUNK`` (default 0), ``PC_SLOT_LOOKUP`` (0), ``PC_SLOT_KV`` ("fp16"); ``keep_arenas`` None is True
    (``PC_SLOT_KEEP_ARENAS`` is ``serve``'s).  Refusals, in this order: ``check_slot_kv``, ``check_slot_keep_arenas``, ``lookup``
    > 0 with ``share_trunk`` where no shared-trunk verify step runs.  ``validate=False`` is ``batch_plan``'s reading: nothing is
    checked."""
    env = os.environ if env is None else env
    if share_trunk is None:
        share_trunk = env.get("PC_SLOT_TRUNK", "0") == "1"
    lookup = int(env.get("PC_SLOT_LOOKUP", "0")) if lookup is None else int(lookup)
    kv = env.get("PC_SLOT_KV", "fp16") if slot_kv is None else slot_kv
    if n_requests < 1:
        why = "no requests"
    elif n_requests > MAX_BATCH:
        why = f"more than {MAX_BATCH} requests"
    elif caps.not_batched is not None:
        why = caps.not_batched
    elif n_stop_ids > 8:
        why = "more than 8 stop token ids"
    elif max_new_tokens < 2:
        why = "nothing to decode after the first token"
    else:
        why = None
    not_batched = why if why is not None or own_arenas else "a cache is not a staged batch-1 arena of its own"
    keep_arenas = True if keep_arenas is None else bool(keep_arenas)
    if validate:
        if kv != "fp16":
            check_slot_kv(kv, share_trunk=bool(share_trunk), lookup=lookup, head_dim=caps.head_dim, no_loop=caps.no_loop,
                          not_batched=not_batched)
        check_slot_keep_arenas(keep_arenas, kv, generate_batch=True)
        if lookup > 0 and share_trunk:
            if not caps.lookup_trunk:
                raise ValueError("generate_batch: lookup > 0 and share_trunk=True cannot be combined (no shared-trunk verify step)")
            if why is not None:
                raise ValueError("generate_batch: lookup > 0 and share_trunk=True cannot be combined (no shared-trunk verify step "
                                 f"runs for this batch: {why})")
    drafts = min(lookup, 15) if lookup > 0 and plain_greedy and caps.lookup_loop else 0
    return Modes(not_batched is None, not_batched or "one device loop over all sequences", bool(share_trunk), lookup, drafts, None,
                 kv, keep_arenas)
