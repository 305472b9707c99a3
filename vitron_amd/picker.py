"""What generate() decides before it touches the device, and how a step's logits become the next ids.

`resolve_generate_args` turns generate()'s keyword arguments into one frozen `GenerateArgs` and raises every refusal that needs no device
work, in a fixed order. `StepPicker` is built from that record once, before the prefill: it uploads everything the picks of ALL steps
need (the static allow masks and every step's pointer array, every step's vt_sample_row / vt_ban_row / vt_bias_row array, the device
histories, the adjustment buffers, an automaton's cells and row array) and
then serves `pick(step, logits) -> ids` without an upload or a host wait. `device_history` is the one builder of a penalty / ban
history; ServingEngine fills a request's `hist` with it too. With guidance_scale `negative_prompt` yields the second
prompt of every sample and `StepPicker.attach_guidance` uploads every step's vt_cfg_row array between the prefills and the loop.
`penalty_alpha` (contrastive search) resolves to `GenerateArgs.penalty_alpha` / `.contrastive`; that mode has a loop of
its own and no StepPicker.
"""
from __future__ import annotations

import dataclasses
import math
import numbers
from dataclasses import dataclass
from typing import Any, FrozenSet, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .engine import parse_kv_cache_dtype
from .sampling import (BAN_ROW_BYTES, BIAS_ROW_BYTES, BIAS_ROWS_MAX_V, CFG_ROW_BYTES, DOLA_ROW_BYTES, FSM_ROW_BYTES, ROW_BYTES, allow_mask, check_penalties,
                       check_sampling_values, check_top_logprobs, check_truncation_values, log_beta, mask_words, normalise_bias, pack_ban_rows,
                       pack_bias_rows, pack_cfg_rows, pack_dola_rows, pack_fsm_rows, pack_sample_rows, pack_trunc_rows, truncation_active, check_dola)
from .sampling import check_mirostat, check_mirostat_request, pack_miro_rows


@dataclass(frozen=True, eq=False)
class GenerateArgs:
    """generate()'s arguments, resolved: the defaults of the config filled in, the lists converted, the static masks built on the host."""
    num_beams: int
    num_return_sequences: int
    length_penalty: float
    early_stopping: Any
    do_sample: bool
    temperature: float
    top_p: float
    top_k: int                                   # None resolved to config.top_k (GenerationConfig's 50)
    repetition_penalty: float
    return_logits: bool
    return_logprobs: bool
    padded_batch: bool
    eos: FrozenSet[int]
    pad: int
    max_new_tokens: int
    ngram: int
    given: Tuple[str, ...]                       # the optional arguments a beam call refuses, as "name=..." in the order they are refused
    sample_seed: int = 0                         # of the counter-based sampler; 0 for a greedy call
    banned_always: Tuple[int, ...] = ()          # suppress_tokens and the single-token bad_words_ids
    banned_begin: Tuple[int, ...] = ()           # begin_suppress_tokens: the first generated token only
    min_new: int = 0
    allowed_ids: Optional[Tuple[int, ...]] = None
    masks: Optional[np.ndarray] = None           # uint32 [n_masks, ceil(V / 32)]: the distinct static allow masks, or None (unconstrained)
    step_mask: Tuple[int, ...] = ()              # per step: the row of `masks` in force, -1 for none
    bias: Tuple[Tuple[int, float], ...] = ()     # sequence_bias, normalised: (id, value) sorted by id, single-token keys only
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    trunc: Tuple[float, float, float, float] = (0.0, 1.0, 0.0, 0.0)   # (min_p, typical_p, epsilon_cutoff, eta_cutoff); off when greedy
    top_logprobs: int = 0                        # N > 0: every step's N most likely tokens and the chosen token's rank (vt_logprob_rows)
    automaton: Any = None                        # a TokenAutomaton every row runs from its start state (vt_fsm_rows)
    guidance_scale: Optional[float] = None       # classifier-free guidance (vt_cfg_rows); None is off (a scale of 1 resolves to it)
    guidance_plausibility: float = 0.0           # beta of the adaptive plausibility cut; 0 is off
    penalty_alpha: float = 0.0                   # contrastive search (vt_contrast_rows); 0 is off
    dola_layers: Optional[Tuple[int, ...]] = None   # DoLa (vt_dola_rows): the candidate layers, resolved; None is off
    dola_relative_top: float = 0.1               # a token stays iff p_final >= relative_top * max p_final
    watermark: Any = None                        # a watermark.SynthIDWatermark (vt_sample_rows_wm); None is off
    mirostat_tau: float = 0.0                    # Mirostat v2 (vt_sample_rows_miro): the target surprise in bits; 0 is off
    mirostat_eta: float = 0.1                    # its learning rate

    @property
    def guided(self) -> bool:
        return self.guidance_scale is not None

    @property
    def dola(self) -> bool:
        return self.dola_layers is not None

    @property
    def contrastive(self) -> bool:
        """transformers' rule for the mode: penalty_alpha > 0 and top_k > 1, greedy, one beam."""
        return self.penalty_alpha > 0 and int(self.top_k or 0) > 1 and not self.do_sample and self.num_beams == 1

    @property
    def constrained(self) -> bool:
        return self.masks is not None

    @property
    def count_penalties(self) -> bool:
        """Does the adjustment depend on what a row has generated (a vt_bias_rows launch before every pick)?"""
        return float(self.presence_penalty) != 0.0 or float(self.frequency_penalty) != 0.0

    @property
    def adjusted(self) -> bool:
        return bool(self.bias) or self.count_penalties

    @property
    def truncated(self) -> bool:
        """Is one of min_p / typical_p / epsilon_cutoff / eta_cutoff on (vt_sample_rows_trunc; a sampling call only)?"""
        return truncation_active(*self.trunc)

    @property
    def per_row(self) -> bool:
        """Does a step need the per-row sampler (vt_sample_rows) instead of vt_argmax / vt_sample_top_p?"""
        return (float(self.repetition_penalty) != 1.0 or bool(self.return_logprobs) or self.constrained or self.ngram > 0
                or self.adjusted or self.truncated or self.automaton is not None or self.guidance_plausibility > 0
                or self.dola or self.watermark is not None or self.mirostat_tau > 0)


def static_mask_schedule(V: int, steps: int, banned_always, banned_begin, min_new: int, eos, allowed_ids):
    """Which ids any row may emit at step st is a pure function of st: at most four distinct masks, keyed by (the first step and something
    is begin-suppressed, st < min_new_tokens and there is an EOS id in [0, V)). Returns (masks uint32 [n, words], per-step row of masks or
    -1), or (None, ()) when no step masks anything (min_new_tokens without an EOS id inside the vocabulary, or no step at all)."""
    eos_in = [int(e) for e in eos if 0 <= int(e) < V]
    masks = {}
    step_key = []
    for st in range(max(int(steps), 0)):
        key = (st == 0 and bool(banned_begin), st < min_new and bool(eos_in))
        if key not in masks:
            banned = list(banned_always) + (list(banned_begin) if key[0] else []) + (eos_in if key[1] else [])
            m = allow_mask(V, allowed_ids, banned)
            if not m.any():
                raise ValueError(f"generate: the constraints leave no token to emit at step {st}")
            masks[key] = None if (allowed_ids is None and not banned) else m
        step_key.append(key)
    live = [k for k, m in masks.items() if m is not None]
    if not live:
        return None, ()
    return np.stack([masks[k] for k in live]), tuple(live.index(k) if k in live else -1 for k in step_key)


def resolve_generate_args(config, input_len: int, *, do_sample, temperature, top_p, top_k, max_new_tokens, max_length, stopping_criteria,
                          eos_token_id, pad_token_id, num_beams, seed, return_logits, padded_batch, repetition_penalty, return_logprobs,
                          suppress_tokens, begin_suppress_tokens, min_new_tokens, bad_words_ids, allowed_token_ids, num_return_sequences,
                          length_penalty, early_stopping, no_repeat_ngram_size, sequence_bias=None, presence_penalty=0.0,
                          frequency_penalty=0.0, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None,
                          top_logprobs=0, automaton=None, choices=None, guidance_scale=None, negative_prompt_ids=None,
                          negative_attention_mask=None, negative_images=None, negative_regions=None, guidance_plausibility=0.0,
                          batch_size=None, penalty_alpha=None, dola_layers=None, dola_relative_top=0.1,
                          watermarking_config=None, mirostat_tau=None, mirostat_eta=0.1, mirostat_mode=2) -> GenerateArgs:
    """generate()'s keyword arguments as a GenerateArgs. Raises, in this order and before any device work: the argument errors of
    num_beams / no_repeat_ngram_size, everything a beam call refuses, the padded_batch refusals that depend on arguments alone, the
    sampling values, the constraint arguments, a step the constraints leave no token for, constraints with padded_batch, the values of
    sequence_bias / presence_penalty / frequency_penalty, those three with padded_batch, the values of min_p / typical_p / epsilon_cutoff /
    eta_cutoff (None is off, as in GenerationConfig; ignored without do_sample), those four with padded_batch, the value of top_logprobs
    (an int in [0, 20]; a beam call refuses it with its other optional arguments), top_logprobs with padded_batch, automaton / choices
    with padded_batch, and what TokenAutomaton.check refuses for the call's EOS ids (a beam call refuses `automaton` with its other
    optional arguments; choices=[...] is automaton=TokenAutomaton.from_choices(...), giving both is a ValueError), and last the
    guidance arguments: ValueError for a guidance_scale that is not a finite number, a guidance_plausibility outside
    [0, 1], a negative_* argument or a plausibility > 0 without a guidance_scale other than 1, an empty negative prompt or one whose batch
    size is neither 1 nor `batch_size`; NotImplementedError with padded_batch (a beam call refuses guidance_scale with its other optional
    arguments). guidance_scale None or 1 is off and resolves to None. Contrastive search: the VALUE of penalty_alpha
    (ValueError: not a finite number in [0, 1]; > 0 together with do_sample=True) is checked right behind num_beams; a beam call refuses
    penalty_alpha > 0 with its other optional arguments; everything else the mode refuses comes last, behind the guidance arguments, in
    check_contrastive's order. penalty_alpha None or 0, or top_k == 1, is off. DoLa: the VALUES of dola_layers and
    dola_relative_top (sampling.check_dola: ValueError) are checked right behind penalty_alpha's; a beam call refuses dola_layers with its
    other optional arguments; padded_batch, guidance_scale and penalty_alpha > 0 are refused with it (NotImplementedError) at the very end.
    dola_layers None is off. The SynthID watermark: watermarking_config is resolved by watermark.SynthIDWatermark right
    behind dola_layers' values (its ValueError / NotImplementedError, the green-list scheme among them); a beam call refuses it with its
    other optional arguments; do_sample=False, penalty_alpha > 0, padded_batch and a vocabulary beyond the sampler's register form are
    refused with it (NotImplementedError) right behind the beam refusals. None is off. Mirostat v2: the VALUES of
    mirostat_tau / mirostat_eta / mirostat_mode (sampling.check_mirostat: ValueError; mirostat_mode=1 NotImplementedError) are checked right
    behind watermarking_config's; with mirostat_tau on, do_sample=False, num_beams > 1, penalty_alpha > 0, padded_batch,
    watermarking_config and a vocabulary beyond the sampler's register form are refused by name (sampling.check_mirostat_request:
    NotImplementedError) IN FRONT of the beam refusals, so that each names mirostat_tau. mirostat_tau None or 0 is off. The sample seed
    is drawn from torch's global CPU generator (so torch.manual_seed makes sampling reproducible, as with GenerationMixin.sample) and
    only when sampling without `seed`, after the beam refusals: greedy and refused calls leave the RNG state alone."""
    num_beams = int(num_beams)
    if num_beams < 1:
        raise ValueError(f"generate: num_beams must be >= 1, got {num_beams}")
    alpha = check_penalty_alpha(penalty_alpha, do_sample)
    dola, dola_rt = check_dola(dola_layers, dola_relative_top, 0 if dola_layers is None else int(config.num_hidden_layers),
                               bool(getattr(config, "tie_word_embeddings", False)))
    from .watermark import as_watermark
    watermark = as_watermark(watermarking_config)
    miro_tau = check_mirostat(mirostat_tau, mirostat_eta, mirostat_mode, "generate")
    top_k_given = top_k
    if no_repeat_ngram_size is None:
        no_repeat_ngram_size = 0
    if not isinstance(no_repeat_ngram_size, int) or isinstance(no_repeat_ngram_size, bool) or not 0 <= no_repeat_ngram_size <= 2 ** 31 - 1:
        raise ValueError(f"generate: no_repeat_ngram_size must be None or an int >= 0 (0 is off), got {no_repeat_ngram_size!r}")
    if choices is not None:
        if automaton is not None:
            raise ValueError("generate: give automaton or choices, not both")
        from .automaton import TokenAutomaton
        automaton = TokenAutomaton.from_choices(choices)
    if automaton is not None:
        from .automaton import TokenAutomaton
        if not isinstance(automaton, TokenAutomaton):
            raise ValueError(f"generate: automaton must be a TokenAutomaton or None, got {automaton!r}")
    eos = config.eos_token_id if eos_token_id is None else eos_token_id
    if max_new_tokens is None:
        max_new_tokens = (max_length - input_len) if max_length else 20
    if top_k is None:     # GenerationConfig's default: the reference's sampling calls (app.py:562-571) run TopKLogitsWarper(50)
        top_k = int(getattr(config, "top_k", 50) or 0)
    optional = (("suppress_tokens", suppress_tokens), ("begin_suppress_tokens", begin_suppress_tokens), ("min_new_tokens", min_new_tokens),
                ("bad_words_ids", bad_words_ids), ("allowed_token_ids", allowed_token_ids), ("stopping_criteria", stopping_criteria),
                ("no_repeat_ngram_size", no_repeat_ngram_size))
    a = GenerateArgs(
        num_beams=num_beams, num_return_sequences=int(num_return_sequences), length_penalty=float(length_penalty), early_stopping=early_stopping,
        do_sample=do_sample, temperature=temperature, top_p=top_p, top_k=top_k, repetition_penalty=repetition_penalty,
        return_logits=return_logits, return_logprobs=return_logprobs, padded_batch=padded_batch,
        eos=frozenset(eos) if isinstance(eos, (list, tuple)) else (frozenset([eos]) if eos is not None else frozenset()),
        pad=pad_token_id if pad_token_id is not None else (config.pad_token_id if config.pad_token_id is not None else 0),
        max_new_tokens=max_new_tokens, ngram=int(no_repeat_ngram_size),
        given=tuple(f"{name}=..." for name, value in optional if value)
        + tuple(f"{name}=True" for name, value in (("return_logits", return_logits), ("return_logprobs", return_logprobs)) if value)
        + tuple(f"{name}=..." for name, value in (("sequence_bias", sequence_bias), ("presence_penalty", presence_penalty),
                                                  ("frequency_penalty", frequency_penalty)) if value)
        + tuple(f"{name}=..." for name, value, off in (("min_p", min_p, 0.0), ("typical_p", typical_p, 1.0),
                                                       ("epsilon_cutoff", epsilon_cutoff, 0.0), ("eta_cutoff", eta_cutoff, 0.0))
                if value is not None and value != off)
        + (("top_logprobs=...",) if top_logprobs else ()) + (("automaton=...",) if automaton is not None else ())
        + (("guidance_scale=...",) if guidance_scale is not None and guidance_scale != 1 else ())
        + (("penalty_alpha=...",) if alpha > 0 else ())
        + (("dola_layers=...",) if dola is not None else ())
        + (("watermarking_config=...",) if watermark is not None else ())
        + (("mirostat_tau=...",) if miro_tau > 0 else ()))
    if miro_tau > 0:
        check_mirostat_request(not do_sample, num_beams, alpha, bool(padded_batch), watermark is not None, int(config.vocab_size),
                               "generate(mirostat_tau=...)")
        a = dataclasses.replace(a, mirostat_tau=miro_tau, mirostat_eta=float(mirostat_eta))
    if num_beams > 1:
        check_beam_arguments(a, int(config.vocab_size))
    elif a.num_return_sequences != 1:
        raise NotImplementedError("generate(num_return_sequences=...) needs num_beams > 1")
    if watermark is not None:
        if not do_sample:
            raise NotImplementedError("generate(watermarking_config=..., do_sample=False) is not implemented: the SynthID tournament "
                                      "reshapes the distribution a token is DRAWN from; a greedy call has none")
        if alpha > 0:
            raise NotImplementedError("generate(watermarking_config=..., penalty_alpha > 0) is not implemented")
        if padded_batch:
            raise NotImplementedError("generate(watermarking_config=..., padded_batch=True) is not implemented; use the default packed "
                                      "batch")
        watermark.check_vocab(int(config.vocab_size), "generate(watermarking_config=...)")
        a = dataclasses.replace(a, watermark=watermark)
    if a.ngram and padded_batch:
        raise NotImplementedError("generate(padded_batch=True) does not take no_repeat_ngram_size; use the default packed batch")
    if padded_batch and parse_kv_cache_dtype(getattr(config, "kv_cache_dtype", None)) == "fp8":
        raise NotImplementedError("generate(padded_batch=True) cannot run on the fp8 KV cache: its fix-up edits views of the 16-bit pages "
                                  "(engine.padded_batch_fixup); call set_kv_cache_dtype('16bit') first")
    sample_seed = 0
    if do_sample:
        sample_seed = int(seed) if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    check_sampling_values(temperature if do_sample else 0.0, top_p if (do_sample and top_p) else 1.0, int(top_k or 0), repetition_penalty,
                          "generate")
    banned_always = [int(t) for t in (suppress_tokens or ())]
    for w in (bad_words_ids or ()):
        if len(w) != 1:
            raise NotImplementedError(f"generate(bad_words_ids=...): the multi-token entry {list(w)!r} is not implemented (single-token "
                                      "entries only: the constraint is a mask over ids)")
        banned_always.append(int(w[0]))
    banned_begin = [int(t) for t in (begin_suppress_tokens or ())]
    min_new = int(min_new_tokens or 0)
    if min_new < 0:
        raise ValueError(f"generate: min_new_tokens must be >= 0, got {min_new_tokens!r}")
    allowed_ids = None if allowed_token_ids is None else tuple(int(t) for t in allowed_token_ids)
    masks, step_mask = None, ()
    if banned_always or banned_begin or allowed_ids is not None or (min_new > 0 and a.eos):
        masks, step_mask = static_mask_schedule(int(config.vocab_size), max_new_tokens, banned_always, banned_begin, min_new, a.eos, allowed_ids)
    if masks is not None and padded_batch:
        raise NotImplementedError("generate(padded_batch=True) does not take suppress_tokens / begin_suppress_tokens / min_new_tokens / "
                                  "bad_words_ids / allowed_token_ids; use the default packed batch")
    V = int(config.vocab_size)
    bias = normalise_bias(sequence_bias, V, "generate(sequence_bias=...)", tuple_keys=True)
    check_penalties(presence_penalty, frequency_penalty, "generate")
    a = dataclasses.replace(a, sample_seed=sample_seed, banned_always=tuple(banned_always), banned_begin=tuple(banned_begin),
                            min_new=min_new, allowed_ids=allowed_ids, masks=masks, step_mask=step_mask, bias=bias,
                            presence_penalty=float(presence_penalty), frequency_penalty=float(frequency_penalty))
    if a.adjusted and padded_batch:
        raise NotImplementedError("generate(padded_batch=True) does not take sequence_bias / presence_penalty / frequency_penalty; use "
                                  "the default packed batch")
    if a.adjusted and V > BIAS_ROWS_MAX_V:
        raise NotImplementedError(f"generate(sequence_bias / presence_penalty / frequency_penalty): vocab_size={V} is beyond vt_bias_rows' "
                                  f"{BIAS_ROWS_MAX_V}")
    trunc = (0.0 if min_p is None else min_p, 1.0 if typical_p is None else typical_p, 0.0 if epsilon_cutoff is None else epsilon_cutoff,
             0.0 if eta_cutoff is None else eta_cutoff)
    check_truncation_values(*trunc, what="generate")
    if do_sample:        # transformers applies warpers only when sampling
        a = dataclasses.replace(a, trunc=tuple(float(x) for x in trunc))
    if a.truncated and padded_batch:
        raise NotImplementedError("generate(padded_batch=True) does not take min_p / typical_p / epsilon_cutoff / eta_cutoff; use the "
                                  "default packed batch")
    check_top_logprobs(top_logprobs, "generate")
    if top_logprobs and padded_batch:
        raise NotImplementedError("generate(padded_batch=True) does not take top_logprobs; use the default packed batch")
    if top_logprobs:
        a = dataclasses.replace(a, top_logprobs=int(top_logprobs))
    if automaton is not None:
        if padded_batch:
            raise NotImplementedError("generate(padded_batch=True) does not take automaton / choices; use the default packed batch")
        automaton.check(V, sorted(a.eos))
        a = dataclasses.replace(a, automaton=automaton)
    scale, beta = check_guidance(guidance_scale, guidance_plausibility, negative_prompt_ids, negative_attention_mask, negative_images,
                                 negative_regions, batch_size)
    if scale is not None:
        if padded_batch:
            raise NotImplementedError("generate(padded_batch=True) does not take guidance_scale; use the default packed batch")
        a = dataclasses.replace(a, guidance_scale=scale, guidance_plausibility=beta)
    if alpha > 0 and num_beams == 1:
        check_contrastive(a, top_k_given)
        a = dataclasses.replace(a, penalty_alpha=alpha)
    if dola is not None and num_beams == 1:
        if padded_batch:
            raise NotImplementedError("generate(dola_layers=..., padded_batch=True) is not implemented; use the default packed batch")
        if a.guided:
            raise NotImplementedError("generate(dola_layers=..., guidance_scale=...) is not implemented: one contrast per call")
        if alpha > 0:
            raise NotImplementedError("generate(dola_layers=..., penalty_alpha > 0) is not implemented: one contrast per call")
        a = dataclasses.replace(a, dola_layers=dola, dola_relative_top=dola_rt)
    return a


def check_penalty_alpha(penalty_alpha, do_sample, what: str = "generate") -> float:
    """The value of penalty_alpha: None is 0 (off). ValueError for anything but a finite number in [0, 1], and for a value > 0 together with
    do_sample=True (transformers' rule makes that a sampling call and drops the penalty silently; here it is said)."""
    if penalty_alpha is None:
        return 0.0
    if not isinstance(penalty_alpha, numbers.Real) or isinstance(penalty_alpha, bool) or not 0 <= penalty_alpha <= 1:     # (a NaN fails both)
        raise ValueError(f"{what}: penalty_alpha must be None or a finite number in [0, 1] (None and 0 are off), got {penalty_alpha!r}")
    if penalty_alpha > 0 and do_sample:
        raise ValueError(f"{what}: penalty_alpha={penalty_alpha!r} with do_sample=True: contrastive search is deterministic")
    return float(penalty_alpha)


CONTRASTIVE_MAX_K = 16          # VT_CONTRAST_MAX_K: the candidates are the 16-wide operand of one MFMA


def check_contrastive(a: GenerateArgs, top_k_given) -> None:
    """Everything a call with penalty_alpha > 0 and one beam refuses, before any page is taken, in this order. top_k == 1 is the mode's off
    switch (transformers' rule) and refuses nothing. stopping_criteria is served."""
    if top_k_given is None:
        raise NotImplementedError("generate(penalty_alpha > 0) needs an explicit top_k in [2, 16]: the configuration's default of "
                                  f"{a.top_k} would be {a.top_k} decode rows per sequence and step")
    if int(top_k_given) == 1:
        return
    if not 2 <= int(top_k_given) <= CONTRASTIVE_MAX_K:
        raise NotImplementedError(f"generate(penalty_alpha > 0, top_k={top_k_given!r}): top_k must lie in [2, {CONTRASTIVE_MAX_K}] "
                                  "(vt_contrast_rows; top_k=1 switches the mode off)")
    if a.padded_batch:
        raise NotImplementedError("generate(penalty_alpha > 0, padded_batch=True) is not implemented: the candidates run in the packed batch")
    if float(a.repetition_penalty) != 1.0:
        raise NotImplementedError("generate(penalty_alpha > 0, repetition_penalty != 1) is not implemented")
    given = [g for g in a.given if g not in ("stopping_criteria=...", "penalty_alpha=...", "dola_layers=...")]
    if given:
        raise NotImplementedError(f"generate(penalty_alpha > 0, {given[0]}) is not implemented")


def check_guidance(guidance_scale, guidance_plausibility, negative_prompt_ids, negative_attention_mask, negative_images, negative_regions,
                   batch_size, what: str = "generate"):
    """The values of the guidance arguments, before any device work: returns (scale or None when guidance is off, beta)."""
    def num(x):
        return isinstance(x, numbers.Real) and not isinstance(x, bool)
    if guidance_scale is not None and (not num(guidance_scale) or not math.isfinite(guidance_scale)):
        raise ValueError(f"{what}: guidance_scale must be None or a finite number (None and 1 are off), got {guidance_scale!r}")
    beta = guidance_plausibility
    if beta is None:
        beta = 0.0
    if not num(beta) or not 0 <= beta <= 1:       # (a NaN fails both comparisons)
        raise ValueError(f"{what}: guidance_plausibility must be a number in [0, 1] (0 is off), got {guidance_plausibility!r}")
    on = guidance_scale is not None and guidance_scale != 1
    if not on:
        for name, value in (("negative_prompt_ids", negative_prompt_ids), ("negative_attention_mask", negative_attention_mask),
                            ("negative_images", negative_images), ("negative_regions", negative_regions)):
            if value is not None and guidance_scale is None:
                raise ValueError(f"{what}: {name} needs guidance_scale")
        if beta > 0:
            raise ValueError(f"{what}: guidance_plausibility needs a guidance_scale other than 1")
        return None, 0.0
    if negative_prompt_ids is None:
        for name, value in (("negative_attention_mask", negative_attention_mask), ("negative_images", negative_images),
                            ("negative_regions", negative_regions)):
            if value is not None:
                raise ValueError(f"{what}: {name} needs negative_prompt_ids")
    else:
        shape = tuple(getattr(negative_prompt_ids, "shape", ()))
        if len(shape) != 2:
            raise ValueError(f"{what}: negative_prompt_ids must be a [B, Ln] or [1, Ln] tensor of ids, got shape {shape}")
        if shape[1] == 0 or shape[0] == 0:
            raise ValueError(f"{what}: negative_prompt_ids is empty (shape {shape})")
        if batch_size is not None and shape[0] not in (1, int(batch_size)):
            raise ValueError(f"{what}: negative_prompt_ids has batch size {shape[0]}, expected 1 or {int(batch_size)}")
        if negative_attention_mask is not None:
            if tuple(negative_attention_mask.shape) != shape:
                raise ValueError(f"{what}: negative_attention_mask has shape {tuple(negative_attention_mask.shape)}, negative_prompt_ids {shape}")
            if not bool((negative_attention_mask != 0).any(-1).all()):
                raise ValueError(f"{what}: negative_attention_mask leaves a negative prompt empty")
    return float(guidance_scale), float(beta)


def negative_prompt(input_ids: torch.Tensor, attention_mask, negative_prompt_ids, negative_attention_mask):
    """The [B, Ln] negative prompt of a guided call and its mask (or None). Without negative_prompt_ids it is the last token of every
    sample's input_ids -- the last one its attention_mask keeps -- as transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor takes
    input_ids[:, -1:]; an image / region sentinel there raises ValueError. A [1, Ln] prompt is every sample's."""
    B = input_ids.shape[0]
    if negative_prompt_ids is None:
        ids = input_ids.cpu()
        if attention_mask is None:
            last = ids[:, -1:]
        else:
            am = attention_mask.cpu() != 0
            if not bool(am.any(-1).all()):
                raise ValueError("generate(guidance_scale=...): a sample without a valid token has no default negative prompt")
            idx = (am.long() * torch.arange(1, ids.shape[1] + 1)).argmax(-1, keepdim=True)
            last = ids.gather(1, idx)
        if bool((last < 0).any()):
            raise ValueError("generate(guidance_scale=...): the default negative prompt is each sample's last token, which is an image / "
                             "region sentinel here; give negative_prompt_ids")
        return last.to(input_ids.device), None
    neg = negative_prompt_ids.to(input_ids.device)
    am = negative_attention_mask
    if neg.shape[0] == 1 and B > 1:
        neg = neg.expand(B, -1).contiguous()
        am = None if am is None else am.expand(B, -1).contiguous()
    return neg, am


def check_beam_arguments(a: GenerateArgs, V: int) -> None:
    """Everything a beam call refuses, before any page is taken or given back."""
    from .beam import num_candidates
    if a.do_sample:
        raise NotImplementedError("generate(num_beams > 1, do_sample=True): beam sampling is not implemented (greedy beam search only)")
    if a.padded_batch:
        raise NotImplementedError("generate(num_beams > 1, padded_batch=True) is not implemented: beams run in the packed batch")
    if float(a.repetition_penalty) != 1.0:
        raise NotImplementedError("generate(num_beams > 1, repetition_penalty != 1) is not implemented")
    if a.given:
        raise NotImplementedError(f"generate(num_beams > 1, {a.given[0]}) is not implemented")
    if a.num_beams > 16:
        raise NotImplementedError(f"generate(num_beams={a.num_beams}): at most 16 beams (vt_beam_step)")
    if a.early_stopping not in (False, True, "never"):
        raise ValueError(f"generate: early_stopping must be False, True or 'never', got {a.early_stopping!r}")
    if not 1 <= a.num_return_sequences <= a.num_beams:
        raise ValueError(f"generate: num_return_sequences={a.num_return_sequences} must lie in [1, num_beams={a.num_beams}]")
    n_cand = num_candidates(a.num_beams, len(a.eos))
    if n_cand > V:
        raise NotImplementedError(f"generate(num_beams={a.num_beams}): a step keeps {n_cand} candidates (max(2, 1 + EOS ids) * num_beams), "
                                  f"more than the vocabulary of {V}")
    if n_cand > 32:
        raise NotImplementedError(f"generate(num_beams={a.num_beams}, eos_token_id=...): a step keeps max(2, 1 + {len(a.eos)} EOS ids) * num_beams "
                                  f"= {n_cand} candidates, vt_beam_step returns at most 32")


def device_history(input_ids: torch.Tensor, room: int, attention_mask: Optional[torch.Tensor] = None, nonneg: bool = False):
    """The histories vt_sample_rows / vt_ban_rows read: int32 [B, longest + room] on input_ids' device, row b holding sample b's prompt
    ids -- those where attention_mask is 1 when a mask is given, only the non-negative ones (the image / region sentinels are negative)
    with nonneg -- followed by `room` slots for what it emits. Returns (buffer, the rows' prompt lengths)."""
    keep = []
    for b in range(input_ids.shape[0]):
        row = input_ids[b] if attention_mask is None else input_ids[b][attention_mask[b].to(input_ids.device).bool()]
        keep.append((row[row >= 0] if nonneg else row).to(torch.int32))
    lens = [int(k.numel()) for k in keep]
    buf = torch.zeros((len(keep), max(lens) + room), dtype=torch.int32, device=input_ids.device)
    for b, k in enumerate(keep):
        buf[b, :lens[b]] = k
    return buf, lens


def row_ptr(t: torch.Tensor, r: int) -> int:
    """The device address of row r of a tensor of 4-byte elements."""
    return t.data_ptr() + 4 * r * t.stride(0)


def row_buffer(buf: torch.Tensor):
    """(buf, the host list of its rows' addresses, the int64 device tensor of them) for a [B, ...] device buffer of 4-byte elements: what
    a launch that writes one row per sample gets, and what the launch that reads the rows gets."""
    ptr = [row_ptr(buf, b) for b in range(buf.shape[0])]
    return buf, ptr, torch.tensor(ptr, dtype=torch.int64).to(buf.device)


class _History:
    """A device_history that grows on the device: `append` writes one id per row behind what the row holds, with no host wait."""

    def __init__(self, input_ids, room, attention_mask=None, nonneg=False):
        self.buf, self.lens = device_history(input_ids, room, attention_mask, nonneg)
        self._pos = torch.tensor(self.lens, dtype=torch.long, device=self.buf.device).unsqueeze(1)

    def row_ptr(self, b: int) -> int:
        return row_ptr(self.buf, b)

    def append(self, ids: torch.Tensor) -> None:
        self.buf.scatter_(1, self._pos, ids.unsqueeze(1))
        self._pos += 1


class StepPicker:
    """pick(step, logits) -> the [B] next ids of a generate() call, in one of three modes chosen once: ops.argmax; ops.sample_top_p; or
    ONE ops.sample_rows launch per step (row b: stream = b, counter = step -- the draws of the scalar sampler), preceded by ONE
    ops.ban_rows launch when an n-gram ban is on. Everything the per-row mode reads is uploaded here, once, for all steps:
      - the static allow masks and the [steps, B] array of their addresses (vt_sample_rows_allow reads row `step` of it);
      - the [steps, B] vt_sample_row array (counter = step, history_len = prompt ids + step);
      - the penalty history (the non-negative prompt ids, then the picks) -- with a repetition penalty;
      - with no_repeat_ngram_size: the ban history (the ids where attention_mask is 1, sentinels included, then the picks), the [steps, B]
        vt_ban_row array (history_len = prompt ids + step, base = the step's static mask or NULL) and the B working masks vt_ban_rows
        writes, which are what the sampler's allow pointers name then -- the same B addresses at every step;
      - with sequence_bias / presence_penalty / frequency_penalty: B adjustment buffers [V][2] and their B addresses (the
        sampler's adjust pointers, the same at every step), the bias ids / values, and the ids every row has GENERATED -- the tail of
        the penalty history where there is one, else a history of its own. With a penalty != 0 the [steps, B] vt_bias_row array
        (history_len = step) is uploaded too and every pick is preceded by ONE ops.bias_rows launch; with sequence_bias alone the
        buffers never change and are built by ONE launch here, before the prefill;
      - with min_p / typical_p / epsilon_cutoff / eta_cutoff: the B vt_trunc_row entries, the same at every step; the
        sampler launch is vt_sample_rows_trunc then.
      - with watermarking_config: the watermark's table and layer constants (once per device, kept on the watermark), one
        all-zero cell per sample and the B vt_wm_row entries, the same at every step; the sampler launch is vt_sample_rows_wm then and
        the cells live and change on the device only.
      - with mirostat_tau: nothing here. The first pick allocates the [B, 2] fp32 cells {2 * tau, 0} and uploads the B
        vt_miro_row entries, the same at every step; the sampler launch is vt_sample_rows_miro then and the cells change on the device
        only. `mirostat_state()` reads them back (once, behind the loop); `drop_mirostat()` lets them go.
      - with an automaton: its tables (once per device, kept on the automaton), the [B, 2] cells {start, 0}, the B
        working masks vt_fsm_rows writes, the ids every row has GENERATED (the tail of the penalty history, or the history the
        penalties count over, or one of its own) and the [steps, B] vt_fsm_row array (gen_len = step, base = the step's static mask or
        NULL). A step is ONE ops.fsm_rows launch; with no_repeat_ngram_size its working masks are the `base` of the vt_ban_row array
        instead of the static mask, and the sampler's allow pointers name the last mask built.
    The histories grow on the device. The device-built masks and adjustments are never read back.
    With top_logprobs = N > 0, in every mode: the [steps, B, N] id and log-probability buffers and the [steps, B] rank
    buffer are allocated here, and every pick is followed by ONE ops.logprob_rows launch over the step's RAW logits with the picked ids
    as targets, which writes step `step` of them -- no allocation, no upload, no host wait. The pick itself is the launch it was.
    With guidance_scale, in every mode: `attach_guidance`, called once between the prefills and the loop, uploads the
    [steps, B] vt_cfg_row array over the addresses the steps' logits will have (the two prefills' rows at step 0, the caller's two
    alternating [2B, V_pad] decode buffers after it), and every pick starts with ONE ops.cfg_rows launch that writes the guided rows in
    place over the conditional ones. Everything behind it -- penalties and bias, masks, the sampler, return_logprobs, top_logprobs --
    sees the guided row. With guidance_plausibility > 0 the mode is per-row: the launch also writes the B working masks
    (base = the step's static mask or NULL), which take the static mask's place as the `base` of the vt_fsm_row array, or of the
    vt_ban_row array when there is no automaton, or as the sampler's allow pointers when there is neither.
    With dola_layers (the mode is per-row): `attach_dola`, called once between the prefill and the loop, uploads the
    [steps, B] vt_dola_row array over the addresses the steps' logits and candidate rows will have, and every pick starts with ONE
    ops.dola_rows launch that writes the contrasted rows in place over the final ones, the chosen candidate of step `step` into
    `dola_choice[step]`, and the B working masks of the kept tokens (base = the step's static mask or NULL) -- the same working masks,
    in the same three places, as guidance_plausibility's (the two modes exclude each other)."""

    def __init__(self, a: GenerateArgs, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], V: int):
        self.a = a
        self.V = int(V)
        self.B = B = input_ids.shape[0]
        self.device = input_ids.device
        self.mode = "rows" if a.per_row else ("top_p" if a.do_sample else "argmax")
        self._lp: List[torch.Tensor] = []
        if a.top_logprobs and a.max_new_tokens > 0:
            n = a.max_new_tokens
            self.top_ids = torch.empty((n, B, a.top_logprobs), dtype=torch.int32, device=self.device)
            self.top_lp = torch.empty((n, B, a.top_logprobs), dtype=torch.float32, device=self.device)
            self.top_rank = torch.empty((n, B), dtype=torch.int32, device=self.device)
        self.cfg_rows = self.cfg_ptrs = self.cfg_mask_ptr = None
        self.dola_rows = self.dola_choice = None
        self.step_base: List[int] = [0] * max(a.max_new_tokens, 0)
        self.miro_rows = self.miro_cells = None     # (Mirostat makes the mode per-row; allocated at the first pick)
        if self.mode != "rows":
            return
        dev, steps = self.device, a.max_new_tokens
        self.allow_ptrs = None
        step_base = [0] * max(steps, 0)          # host: the address of every step's static mask (0: none), the `base` of its vt_ban_row
        if a.constrained:
            self.allow_dev = torch.from_numpy(a.masks.view("<i4")).to(dev)                                      # [n_masks, words]
            step_base = [0 if i < 0 else self.allow_dev[i].data_ptr() for i in a.step_mask]
            self.allow_ptrs = torch.tensor([[p] * B for p in step_base], dtype=torch.int64).to(dev)             # [steps, B]
        self.hist = _History(input_ids, steps, nonneg=True) if float(a.repetition_penalty) != 1.0 else None
        T, p, k = (float(a.temperature), float(a.top_p if a.top_p else 1.0), int(a.top_k or 0)) if a.do_sample else (0.0, 1.0, 0)
        self.rows = pack_sample_rows(
            [(T, k, p, float(a.repetition_penalty), a.sample_seed, st, b,
              0 if self.hist is None else self.hist.row_ptr(b), 0 if self.hist is None else self.hist.lens[b] + st)
             for st in range(steps) for b in range(B)], dev).view(steps, B, ROW_BYTES)
        self.step_base = step_base
        cfg_ptr = None
        if a.guidance_plausibility > 0 or a.dola:   # the masks vt_cfg_rows / vt_dola_rows write stand where the static masks stood
            self.cfg_work, cfg_ptr, self.cfg_ptrs = row_buffer(torch.empty((B, mask_words(self.V)), dtype=torch.int32, device=dev))
        self.cfg_mask_ptr = cfg_ptr
        self.fsm_rows = None
        ban_base = step_base
        if a.automaton is not None:
            self.fsm_work, fsm_ptr, self.fsm_ptrs = row_buffer(torch.empty((B, mask_words(self.V)), dtype=torch.int32, device=dev))
            ban_base = None                      # the ban's base is the row's automaton mask, whatever the step
        self.ban_rows = None
        if a.ngram:
            self.ban_hist = h = _History(input_ids, steps, attention_mask)
            self.ban_work = w = torch.empty((B, mask_words(self.V)), dtype=torch.int32, device=dev)
            self.ban_rows = pack_ban_rows([(h.row_ptr(b), h.lens[b] + st, fsm_ptr[b] if ban_base is None else (ban_base[st] if cfg_ptr is None else cfg_ptr[b]),
                                            row_ptr(w, b), a.ngram, 0, 0, 0)
                                           for st in range(steps) for b in range(B)], dev).view(steps, B, BAN_ROW_BYTES)
            self.ban_ptrs = row_buffer(w)[2]     # (uploaded behind the rows that name the same addresses)
        self.trunc = pack_trunc_rows([a.trunc] * B, dev) if a.truncated else None
        self.wm_rows = self.wm_cells = None
        if a.watermark is not None:              # one cell per sample; the array is constant over the steps
            from .watermark import pack_wm_rows
            self.wm_cells = [a.watermark.new_cell(dev) for _ in range(B)]
            self.wm_rows = pack_wm_rows([(a.watermark, c) for c in self.wm_cells], dev)
        self.adj_ptrs = self.bias_rows = self.gen_hist = None
        gen_ptr = None

        def generated_ptrs():                    # where every row's GENERATED ids stand
            if self.hist is not None:            # the tail of the penalty history
                return [self.hist.row_ptr(b) + 4 * self.hist.lens[b] for b in range(B)]
            if self.gen_hist is None:
                self.gen_hist = _History(input_ids[:, :0], steps)
            return [self.gen_hist.row_ptr(b) for b in range(B)]

        if a.adjusted and steps > 0:
            self.adj, adj_ptr, self.adj_ptrs = row_buffer(torch.zeros((B, self.V, 2), dtype=torch.float32, device=dev))
            self.bias_ids = torch.tensor([t for t, _ in a.bias], dtype=torch.int32).to(dev)
            self.bias_vals = torch.tensor([v for _, v in a.bias], dtype=torch.float32).to(dev)
            ids_ptr, vals_ptr = (self.bias_ids.data_ptr(), self.bias_vals.data_ptr()) if a.bias else (0, 0)
            if not a.count_penalties:            # the rows never change: one launch, here
                ops.bias_rows(pack_bias_rows([(0, 0, ids_ptr, vals_ptr, len(a.bias), adj_ptr[b], 0.0, 0.0) for b in range(B)], dev), B, self.V)
            else:
                gen_ptr = generated_ptrs()
                self.bias_rows = pack_bias_rows(
                    [(gen_ptr[b] if st else 0, st, ids_ptr, vals_ptr, len(a.bias), adj_ptr[b], a.presence_penalty, a.frequency_penalty)
                     for st in range(steps) for b in range(B)], dev).view(steps, B, BIAS_ROW_BYTES)
        if a.automaton is not None:
            if gen_ptr is None:
                gen_ptr = generated_ptrs()
            self.fsm_cell = c = torch.tensor([[a.automaton.start, 0]] * B, dtype=torch.int32).to(dev)
            cell_ptr = [c.data_ptr() + 8 * b for b in range(B)]
            tables, eos = a.automaton.row_fields(dev), sorted(a.eos)
            self.fsm_rows = pack_fsm_rows([(gen_ptr[b] if st else 0, st, cell_ptr[b], step_base[st] if cfg_ptr is None else cfg_ptr[b], fsm_ptr[b], *tables, eos)
                                           for st in range(steps) for b in range(B)], dev).view(steps, B, FSM_ROW_BYTES)

    def attach_guidance(self, cond0: torch.Tensor, uncond0: torch.Tensor, bufs) -> None:
        """Upload every step's vt_cfg_row array, once. cond0 / uncond0: the fp32 [B, V] logits of the two prefills (step 0). bufs: the two
        contiguous fp32 [2B, V_pad] buffers the decode passes write in turn -- step st >= 1 reads bufs[st & 1], rows [0, B) conditional and
        rows [B, 2B) unconditional. The guided row goes in place over the conditional one."""
        a, B = self.a, self.B
        if not a.guided or a.max_new_tokens <= 0:
            return
        if cond0.shape[1] != self.V or uncond0.shape[1] != self.V:
            raise RuntimeError(f"generate: guidance was set up for V = {self.V}, the logits have {cond0.shape[1]} columns")
        lb = log_beta(a.guidance_plausibility)

        rows = []
        for st in range(a.max_new_tokens):
            for b in range(B):
                c, u = (row_ptr(cond0, b), row_ptr(uncond0, b)) if st == 0 else (row_ptr(bufs[st & 1], b), row_ptr(bufs[st & 1], B + b))
                rows.append((c, u, c, self.step_base[st], 0 if self.cfg_mask_ptr is None else self.cfg_mask_ptr[b], 0, a.guidance_scale, lb))
        self._cfg_keep = (cond0, uncond0, bufs)
        self.cfg_rows = pack_cfg_rows(rows, self.device).view(a.max_new_tokens, B, CFG_ROW_BYTES)

    def attach_dola(self, final0: torch.Tensor, prem0: torch.Tensor, final_bufs, prem_bufs) -> None:
        """Upload every step's vt_dola_row array, once. final0: the fp32 [B, V] logits of the prefill (step 0); prem0: its candidate rows,
        fp32 [n_cand, B, V_pad]. final_bufs / prem_bufs: the two contiguous fp32 [B, V_pad] / [n_cand, B, V_pad] buffers the decode passes and
        their candidate lm_head launches write in turn -- step st >= 1 reads index st & 1. The contrasted row goes in place over the final
        one; candidate j of row b is prem[j, b]."""
        a, B = self.a, self.B
        if not a.dola or a.max_new_tokens <= 0:
            return
        if final0.shape[1] != self.V:
            raise RuntimeError(f"generate: DoLa was set up for V = {self.V}, the logits have {final0.shape[1]} columns")
        n_cand, steps = len(a.dola_layers), a.max_new_tokens
        lrt = math.log(a.dola_relative_top)
        self.dola_choice = ch = torch.zeros((steps, B), dtype=torch.int32, device=self.device)

        rows = []
        for st in range(steps):
            f, p = (final0, prem0) if st == 0 else (final_bufs[st & 1], prem_bufs[st & 1])
            for b in range(B):
                rows.append((row_ptr(f, b), p.data_ptr() + 4 * b * p.stride(1), p.stride(0), n_cand, row_ptr(f, b), self.step_base[st],
                             self.cfg_mask_ptr[b], ch.data_ptr() + 4 * (st * B + b), 0, 0, lrt))
        self._dola_keep = (final0, prem0, final_bufs, prem_bufs)
        self.dola_rows = pack_dola_rows(rows, self.device).view(steps, B, DOLA_ROW_BYTES)

    def check_width(self, logits: torch.Tensor) -> None:
        if self.mode == "rows" and (self.a.constrained or self.a.ngram or self.a.automaton is not None) and logits.shape[1] != self.V:
            raise RuntimeError(f"generate: the allow masks were built for V = {self.V}, the logits have {logits.shape[1]} columns")
        if self.mode == "rows" and self.a.adjusted and logits.shape[1] != self.V:
            raise RuntimeError(f"generate: the logit adjustments were built for V = {self.V}, the logits have {logits.shape[1]} columns")

    def pick(self, step: int, logits: torch.Tensor) -> torch.Tensor:
        if self.cfg_rows is not None:            # the guided rows, in place over the conditional ones `logits` names: one launch
            ops.cfg_rows(self.cfg_rows[step], self.B, self.V)
        if self.dola_rows is not None:           # the contrasted rows, in place over the final ones `logits` names: one launch
            ops.dola_rows(self.dola_rows[step], self.B, self.V)
        nxt = self._pick_ids(step, logits)
        if self.a.top_logprobs:                  # the distribution behind the pick: RAW logits, the picked ids as targets
            ops.logprob_rows(logits, nxt, self.a.top_logprobs, out={"rank": self.top_rank[step], "top_ids": self.top_ids[step],
                                                                    "top_logprobs": self.top_lp[step]})
        return nxt

    def _pick_ids(self, step: int, logits: torch.Tensor) -> torch.Tensor:
        a = self.a
        if self.mode == "argmax":
            return ops.argmax(logits)
        if self.mode == "top_p":   # device-side temperature / top-k / top-p sampler (no host sync, counter-based RNG)
            return ops.sample_top_p(logits, a.temperature, a.top_p if a.top_p else 1.0, a.sample_seed, step, top_k=int(a.top_k or 0))
        ptrs = None if self.allow_ptrs is None else self.allow_ptrs[step]
        if self.cfg_ptrs is not None:            # the plausibility masks ops.cfg_rows has just written (they start from the static one)
            ptrs = self.cfg_ptrs
        if self.fsm_rows is not None:            # the rows' states catch up with what they emitted; their masks for this pick: one launch
            ops.fsm_rows(self.fsm_rows[step], self.B, self.V)
            ptrs = self.fsm_ptrs
        if self.ban_rows is not None:            # the rows' masks for this pick, from their histories: one launch, nothing uploaded
            ops.ban_rows(self.ban_rows[step], self.B, logits.shape[1])
            ptrs = self.ban_ptrs
        if self.bias_rows is not None:           # the rows' adjustments for this pick, from what they have generated: one launch
            ops.bias_rows(self.bias_rows[step], self.B, self.V)
        if a.mirostat_tau > 0 and self.miro_rows is None:      # one cell per sample; the array is constant over the steps
            self.miro_cells = torch.tensor([[2.0 * a.mirostat_tau, 0.0]] * self.B, dtype=torch.float32).to(self.device)
            self.miro_rows = pack_miro_rows([(self.miro_cells[b], a.mirostat_tau, a.mirostat_eta) for b in range(self.B)], self.device)
        nxt = ops.sample_rows(logits, self.rows[step], return_logprob=bool(a.return_logprobs), _allow_ptrs=ptrs, _adjust_ptrs=self.adj_ptrs,
                              trunc=self.trunc, watermark=self.wm_rows, miro=self.miro_rows)
        if a.return_logprobs:
            nxt, lp = nxt
            self._lp.append(lp)
        if self.hist is not None:
            self.hist.append(nxt)
        if self.ban_rows is not None:
            self.ban_hist.append(nxt)
        if self.gen_hist is not None:
            self.gen_hist.append(nxt)
        return nxt

    def mirostat_state(self) -> Optional[dict]:
        """{"mu": [B floats], "surprise": [B floats]} read back from the cells (one device -> host copy), or None without Mirostat or
        before the first pick."""
        if self.miro_cells is None:
            return None
        host = self.miro_cells.cpu()
        return {"mu": host[:, 0].tolist(), "surprise": host[:, 1].tolist()}

    def drop_mirostat(self) -> None:
        self.miro_rows = self.miro_cells = None

    def logprobs(self, n: int) -> torch.Tensor:
        """fp32 [B, n]: the log-probabilities collected by the first n picks."""
        if not self._lp:
            return torch.empty((self.B, 0), dtype=torch.float32, device=self.device)
        return torch.stack(self._lp, 1)[:, :n]

    def top(self, n: int) -> dict:
        """What the first n picks' ops.logprob_rows launches wrote: top_ids int32 [B, n, N], top_logprobs fp32 [B, n, N], rank int32
        [B, n] (the picked id's rank in the RAW order)."""
        N = self.a.top_logprobs
        if not hasattr(self, "top_ids"):
            return {"top_ids": torch.empty((self.B, 0, N), dtype=torch.int32, device=self.device),
                    "top_logprobs": torch.empty((self.B, 0, N), dtype=torch.float32, device=self.device),
                    "rank": torch.empty((self.B, 0), dtype=torch.int32, device=self.device)}
        return {"top_ids": self.top_ids[:n].permute(1, 0, 2).contiguous(), "top_logprobs": self.top_lp[:n].permute(1, 0, 2).contiguous(),
                "rank": self.top_rank[:n].permute(1, 0).contiguous()}
