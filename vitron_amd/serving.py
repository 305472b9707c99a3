"""Continuous batching on the paged KV cache (the serving half).

The reference serves one request at a time (`app.py:1128`: Gradio queue, concurrency 1; global `model` / `conv`). With a paged
cache and packed sequences a second request does not have to wait for the first one's 1024 decode steps: every step of this
engine decodes ONE token for every active sequence in a single `vt_llama_forward` call (one row per sequence, weight-streaming
GEMMs + the fused decode attention), and requests join / leave between steps.

  eng = ServingEngine(model, max_batch=16, kv_pages=512)
  a = eng.submit(ids_a, images=[img], regions=[box], max_new_tokens=256)
  b = eng.submit(ids_b, max_new_tokens=64)           # may be submitted while `a` is already decoding
  for rid, token in eng.step(): ...                  # or: outputs = eng.run()   -> {rid: LongTensor of new tokens}

Admission runs the request's multimodal prefill on its own (towers -> splice -> decoder prefill, exactly what `generate` does,
including the visual-feature cache), so a request's tokens are bit-identical to running it alone -- with greedy decoding, and with
sampling for a request submitted with its own `SamplingParams` (submit(..., sampling=): its draws depend on its seed and on how many
tokens it has generated, never on its neighbours; DESIGN.md 8, the `_pick` contract) -- as long
as the decode batch stays on one kernel path (<= 16 rows: the folded-norm path; the engine never mixes a sequence between the
<= 16 and > 16 row paths within one request unless max_batch > 16).

Failures are isolated per request: a request whose own multimodal encoding or prefill fails (bad image shape, bad region, a prompt
beyond the rotary table) is moved to `failed` with its exception and leaves the queue -- the requests behind it are served. Only
errors that are not tied to one request (a HIP runtime error) propagate out of step(), with every page this call took given back
and the candidates re-queued. A pool whose pages are held by someone else (a `past_key_values` the caller keeps) makes the waiting
requests WAIT: step() returns [] and run() raises "no progress" instead of spinning when nothing is active and nothing can be admitted. `kv_pages` given to the constructor is an UPPER BOUND of the pool: the
engine never rebuilds a larger one behind the caller's back; requests that do not fit next to the running ones wait, and one that
cannot fit even an empty pool of that size fails instead of blocking the queue forever.
"""
from __future__ import annotations

import collections
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .engine import PagedKVCache, SequenceState, llama_forward, pair_lo, parse_kv_cache_dtype
from .picker import device_history
from .sampling import (BIAS_ROWS_MAX_V, LogitAdjust, SamplingParams, check_constraints, flatten_ban_seqs, mask_words, pack_ban_rows,
                       pack_bias_rows, pack_cfg_rows, pack_dola_rows, check_dola, pack_fsm_rows, pack_sample_rows, pack_trunc_rows, step_allow_mask)


@dataclass
class _Request:
    rid: int
    input_ids: torch.Tensor
    images: Optional[list]
    regions: Optional[list]
    max_new_tokens: int
    eos: frozenset
    seq: SequenceState = field(default_factory=SequenceState)
    tokens: List[int] = field(default_factory=list)
    last: Optional[torch.Tensor] = None      # device int32 [1]: the token to feed next
    done: bool = False
    flat: Optional[torch.Tensor] = None      # spliced prompt rows [rows, H] (kept while the request waits for pages)
    flat_lo: Optional[torch.Tensor] = None   # their low halves in the precise levels 2 / 3 (the embeddings travel as an operand pair)
    need: int = 0                            # KV pages for prompt + max_new_tokens
    error: Optional[BaseException] = None    # set when the request failed on its own (it is in ServingEngine.failed then)
    sampling: Optional[SamplingParams] = None  # per-request sampling; None: the engine-wide setting (the legacy draw)
    hist: Optional[torch.Tensor] = None      # device int32: prompt ids + the tokens fed back. With a repetition penalty alone the non-negative
                                             # prompt ids; with a device ban input_ids as submitted, sentinels included --
                                             # the penalty reads the same buffer then (vt_sample_rows skips ids outside [0, V))
    hist_len: int = 0
    last_lp: Optional[torch.Tensor] = None   # device fp32 [1]: log-probability of `last` (sampling.logprobs)
    logprobs: List[float] = field(default_factory=list)
    last_top: Optional[tuple] = None         # (device int32 buffer, row, rows, n_top) of `last`'s vt_logprob_rows output (sampling.top_logprobs)
    top: List[tuple] = field(default_factory=list)   # per emitted token: (rank, top ids, top log-probabilities)
    allow_host: dict = field(default_factory=dict)   # step_allow_mask's cache: the static host masks, the choices trie
    allow_dev: dict = field(default_factory=dict)    # static masks on the device ("pre" / "post"): uploaded once, released with hist
    allow_cur: Optional[torch.Tensor] = None         # the mask of the next pick (a static one, a step-dependent upload, or None)
    allow_at: int = -1                               # len(tokens) `allow_cur` was prepared for
    mask_uploads: int = 0                            # host -> device mask copies this request has cost
    ban_mask: Optional[torch.Tensor] = None          # device int32 [ceil(V / 32)]: the working mask vt_ban_rows writes before every pick
    ban_seqs: Optional[torch.Tensor] = None          # device int32: sampling.bad_words flattened ({L, ids} repeated), uploaded once
    adjust: Optional[LogitAdjust] = None             # additive adjustment; None: none. What follows is released with hist
    adj_buf: Optional[torch.Tensor] = None           # device fp32 [V, 2]: the (pre, post) pairs vt_bias_rows writes, vt_sample_rows_adj reads
    adj_ids: Optional[torch.Tensor] = None           # device int32 / fp32: the logit bias, uploaded once
    adj_vals: Optional[torch.Tensor] = None
    gen: Optional[torch.Tensor] = None               # device int32 [max_new_tokens]: the tokens fed back (what the penalties count over,
    gen_len: int = 0                                 # what an automaton's state moves over)
    fsm_cell: Optional[torch.Tensor] = None          # device int32 [2]: {state, consumed} of sampling.automaton
    fsm_mask: Optional[torch.Tensor] = None          # device int32 [ceil(V / 32)]: the working mask vt_fsm_rows writes before every pick
    nseq: Optional[SequenceState] = None             # a guided request's second sequence: its negative prompt
    neg_ids: Optional[torch.Tensor] = None           # device ids [1, Ln] of the negative prompt (text only)
    neg_flat: Optional[torch.Tensor] = None          # its embedded rows [Ln, H] (kept while the request waits for pages)
    need_neg: int = 0                                # the part of `need` that is the second sequence's
    dola: Optional[tuple] = None                     # a DoLa request's candidate layers, resolved against the model
    wm_cell: Optional[torch.Tensor] = None           # device int64: the SynthID state of sampling.watermark, taken at the
                                                     # request's first pick (its admission), dropped with the masks when it retires
    miro_cell: Optional[torch.Tensor] = None         # device fp32 {mu, last_surprise}: the Mirostat state of sampling.mirostat_tau,
                                                     # taken at the request's first pick (its admission), released with the masks
    miro_final: Optional[tuple] = None               # (mu, last_surprise) read from the cell when the request retires

    @property
    def rows(self) -> int:
        """Decode rows the request takes in a step: a guided one runs its negative sequence beside its own."""
        return 2 if self.nseq is not None else 1


class ServingEngine:
    def __init__(self, model, max_batch: int = 16, kv_pages: Optional[int] = None, do_sample: bool = False,
                 temperature: float = 1.0, top_p: float = 1.0, seed: int = 0, batch_prefill: bool = False):
        self.model = model
        self.max_batch = int(max_batch)
        self.do_sample, self.temperature, self.top_p, self.seed = bool(do_sample), float(temperature), float(top_p), int(seed)
        # batch_prefill: requests admitted in the same step share ONE packed decoder prefill (larger GEMMs: higher throughput);
        # their logits then differ from a solo run by bf16 noise (other GEMM tiles), so it is off where bit-identity matters
        self.batch_prefill = bool(batch_prefill)
        self.waiting: "collections.deque[_Request]" = collections.deque()
        self.active: List[_Request] = []
        self.finished: Dict[int, _Request] = {}
        self.failed: Dict[int, _Request] = {}            # requests that failed on their own (`.error` holds the exception)
        self._next_id = 0
        self._step = 0
        self.kv_cap: Optional[int] = None                # upper bound of the pool (pages) when the caller fixed one
        if kv_pages is not None:
            model.reset_prefix_cache()
            llama = model.get_model().llama
            if parse_kv_cache_dtype(getattr(model.config, "kv_cache_dtype", None)) == "fp8":    # the pool in the model's KV format
                model.kv = model.new_kv_pool(int(kv_pages))
            else:
                model.kv = PagedKVCache(llama, int(kv_pages))
            self.kv_cap = int(kv_pages)
        from .prefix_cache import VisualFeatureCache
        self._vis_cache = VisualFeatureCache(int(getattr(model.config, "vis_cache_entries", 16)))

    # ---- queue ----------------------------------------------------------------------------------------------------------
    def submit(self, input_ids: torch.Tensor, images=None, regions=None, max_new_tokens: int = 256,
               eos_token_id=None, sampling: Optional[SamplingParams] = None, adjust: Optional[LogitAdjust] = None) -> int:
        """sampling: this request's own SamplingParams. It then draws with (seed = sampling.seed, counter = tokens it has generated so
        far, stream = 0) -- what generate() uses for a batch of one -- so its tokens equal
        generate(do_sample=temperature > 0, temperature, top_p, top_k, seed, repetition_penalty) for the request alone, whatever else is in
        the batch. Without it the request follows the engine-wide setting exactly as before.
        adjust: this request's own LogitAdjust: a logit bias added before the repetition penalty, presence / frequency
        penalties over the tokens it has generated after it. Its tokens equal generate(sequence_bias=..., presence_penalty=...,
        frequency_penalty=...) for the request alone, whatever else is in the batch; a request with `adjust` and without `sampling` keeps
        its legacy row parameters.
        sampling.guidance_scale (None or 1 is off): classifier-free guidance against sampling.negative_prompt_ids (text
        only; None: the prompt's last token, a ValueError when that is a sentinel). The request owns a second sequence and takes two of
        max_batch's rows; its tokens equal generate(guidance_scale=, negative_prompt_ids=) for the request alone.
        sampling.dola_layers (None is off): DoLa decoding with sampling.dola_relative_top. The request takes one decode
        row; its tokens equal generate(dola_layers=, dola_relative_top=) for the request alone. ValueError here when the layers do not
        fit the model.
        sampling.watermarking_config (None is off): the SynthID text watermark of generate(watermarking_config=). The
        request's state lives in a cell on the device from its first pick to its retirement; its tokens equal
        generate(watermarking_config=) for the request alone, whatever else is in the batch. NotImplementedError here when the
        vocabulary is beyond the sampler's register form.
        sampling.mirostat_tau (None or 0 is off): Mirostat v2 with sampling.mirostat_eta. The request's {mu, last_surprise}
        lives in a cell of its own on the device from its first pick until it retires, fails or is cancelled (mirostat_state(rid));
        its tokens equal generate(mirostat_tau=, mirostat_eta=) for the request alone, whatever joins or leaves the batch.
        NotImplementedError here, naming mirostat_tau: a greedy request, watermarking_config, a vocabulary beyond the sampler's register
        form."""
        ids = input_ids if input_ids.dim() == 2 else input_ids.unsqueeze(0)
        if ids.shape[0] != 1:
            raise ValueError("submit() takes one sequence per request")
        if sampling is not None:                 # rejected here, before anything is queued
            if not isinstance(sampling, SamplingParams):
                raise TypeError(f"submit(sampling=...) takes a SamplingParams, got {type(sampling).__name__}")
            sampling.validate()
        eos = self.model.config.eos_token_id if eos_token_id is None else eos_token_id
        eos_set = frozenset(eos) if isinstance(eos, (list, tuple, set, frozenset)) else (frozenset([eos]) if eos is not None else frozenset())
        if sampling is not None and (sampling.constrained or sampling.mirostat):
            check_constraints(sampling, eos_set, int(self.model.config.vocab_size))     # ValueError: nothing is queued
            if sampling.automaton is not None:
                sampling.automaton.check(int(self.model.config.vocab_size), sorted(eos_set))
        if sampling is not None and sampling.watermark is not None:
            sampling.watermark.check_vocab(int(self.model.config.vocab_size), "submit(sampling=SamplingParams(watermarking_config=...))")
        dola = None
        if sampling is not None and sampling.dola:
            dola, _ = check_dola(sampling.dola_layers, sampling.dola_relative_top, int(self.model.config.num_hidden_layers),
                                 bool(getattr(self.model.config, "tie_word_embeddings", False)), what="submit(sampling=SamplingParams(...))")
        neg = None
        if sampling is not None and sampling.guided:
            if self.max_batch < 2:
                raise ValueError("submit(sampling=SamplingParams(guidance_scale=...)): a guided request takes two decode rows, max_batch is "
                                 f"{self.max_batch}")
            if sampling.negative_prompt_ids is not None:
                neg = torch.tensor([list(sampling.negative_prompt_ids)], dtype=ids.dtype)
            else:                                # transformers' default: the last token of the prompt
                neg = ids[:, -1:].cpu()
                if int(neg[0, 0]) < 0:
                    raise ValueError("submit(sampling=SamplingParams(guidance_scale=...)): the default negative prompt is the prompt's last "
                                     "token, which is an image / region sentinel here; give negative_prompt_ids")
        if adjust is not None:                   # rejected here too
            if not isinstance(adjust, LogitAdjust):
                raise TypeError(f"submit(adjust=...) takes a LogitAdjust, got {type(adjust).__name__}")
            V = int(self.model.config.vocab_size)
            adjust.check_vocab(V)
            if adjust.active and V > BIAS_ROWS_MAX_V:
                raise ValueError(f"submit(adjust=...): vocab_size={V} is beyond vt_bias_rows' {BIAS_ROWS_MAX_V}")
            if not adjust.active:
                adjust = None
        r = _Request(self._next_id, ids.to(self.model.device), images, regions, int(max_new_tokens), eos_set, sampling=sampling,
                     adjust=adjust, dola=dola)
        if neg is not None:
            r.nseq, r.neg_ids = SequenceState(), neg.to(self.model.device)
        self._next_id += 1
        self.waiting.append(r)
        return r.rid

    def pending(self) -> int:
        return len(self.waiting) + len(self.active)

    def cancel(self, rid: int) -> bool:
        """Drop a request that is still waiting (True) -- a running or finished one is left alone (False)."""
        for r in self.waiting:
            if r.rid == rid:
                self.waiting.remove(r)
                r.flat = r.last_top = r.neg_flat = None
                self._drop_masks(r)
                return True
        return False

    def _fail(self, r: _Request, exc: BaseException) -> None:
        """The request failed on its own: it leaves the engine with its exception; nothing else is disturbed."""
        self._release(r)
        r.last, r.flat, r.hist, r.last_lp, r.last_top, r.neg_flat = None, None, None, None, None, None
        self._drop_masks(r)
        r.error, r.done = exc, True
        self.failed[r.rid] = r

    def _release(self, r: _Request) -> None:
        """The request's pages, those of a guided request's second sequence included, go back to the pool."""
        for q in (r.seq, r.nseq):
            if q is not None:
                if q.pages:
                    self.model.kv.release(q.pages)
                q.pages, q.length = [], 0

    def _guide(self, logits: torch.Tensor, reqs: List[_Request], uncond: Dict[int, torch.Tensor]) -> None:
        """Classifier-free guidance in front of _pick: ONE vt_cfg_rows launch over the rows of `logits` writes the guided
        row in place over the conditional row of every guided request (uncond[i]: the fp32 [V] row of reqs[i]'s negative sequence);
        every other row carries cond = NULL and is untouched."""
        V = int(logits.shape[1])
        rows = []
        for i, r in enumerate(reqs):
            if i in uncond:
                c = logits[i].data_ptr()
                rows.append((c, uncond[i].data_ptr(), c, 0, 0, 0, float(r.sampling.guidance_scale), -float("inf")))
            else:
                rows.append((0, 0, 0, 0, 0, 0, 1.0, -float("inf")))
        ops.cfg_rows(pack_cfg_rows(rows, logits.device), len(rows), V)

    @staticmethod
    def _dola_layers(reqs: List[_Request]) -> Optional[List[int]]:
        """The union of the candidate layers of the DoLa requests among `reqs` -- what their decoder pass traces -- or None."""
        layers = sorted({l for r in reqs if r.dola for l in r.dola})
        return layers or None

    def _forward(self, llama, seqs, x, lens, reqs: List[_Request], embeds_lo=None):
        """llama_forward over `seqs` (the sequences of `reqs` first); with a DoLa request among `reqs` the pass also traces the union of
        their candidate layers at its logit rows and _dola contrasts those requests' rows before the logits are returned. Without
        one it is the call it always was."""
        layers = self._dola_layers(reqs)
        if layers is None:
            return llama_forward(llama, self.model.kv, seqs, x, lens, embeds_lo=embeds_lo)
        logits, trace = llama_forward(llama, self.model.kv, seqs, x, lens, embeds_lo=embeds_lo, trace_rows_layers=layers)
        self._dola(llama, logits, reqs, trace)
        return logits

    def _dola(self, llama, logits: torch.Tensor, reqs: List[_Request], trace: torch.Tensor) -> None:
        """DoLa in front of _pick. trace: the operand-dtype [L, rows, H] logit-row trace of the pass that produced
        `logits` (row i belongs to reqs[i]). ONE gather of the DoLa requests' candidate rows, the bare lm_head over them in launches of
        at most 16 rows (the weight-streaming GEMM of a decode step's lm_head), and ONE vt_dola_rows launch over the rows of `logits`
        that writes the contrasted row in place over the final row of every DoLa request; every other row carries final = NULL and is
        untouched. The filtered tokens are -inf in the row, which no later stage can raise."""
        V, n_rows = int(logits.shape[1]), int(trace.shape[1])
        idx, first = [], {}
        for i, r in enumerate(reqs):
            if r.dola:
                first[i] = len(idx)
                idx += [l * n_rows + i for l in r.dola]
        gathered = trace.view(-1, llama.H).index_select(0, torch.tensor(idx, dtype=torch.long).to(trace.device))
        prem = torch.empty((len(idx), llama.V_pad), dtype=torch.float32, device=trace.device)
        for r0 in range(0, len(idx), 16):
            ops.gemm(gathered[r0:r0 + 16], llama.lm_head, None, ops.EPI_F32, out=prem[r0:r0 + 16])
        rows = []
        for i, r in enumerate(reqs):
            if i in first:
                f = logits[i].data_ptr()
                rows.append((f, prem[first[i]].data_ptr(), llama.V_pad, len(r.dola), f, 0, 0, 0, 0, 0, math.log(r.sampling.dola_relative_top)))
            else:
                rows.append((0,) * 10 + (0.0,))
        ops.dola_rows(pack_dola_rows(rows, logits.device), len(rows), V)

    @staticmethod
    def _is_device_error(exc: BaseException) -> bool:
        """Errors that are not one request's fault: the HIP runtime (status -2 of the C ABI), the allocator."""
        return isinstance(exc, torch.cuda.OutOfMemoryError) or "status -2" in str(exc) or "HIP error" in str(exc)

    @staticmethod
    def _drop_masks(r: _Request) -> None:
        r.allow_dev, r.allow_host, r.allow_cur, r.allow_at = {}, {}, None, -1
        r.ban_mask = r.ban_seqs = None
        r.adj_buf = r.adj_ids = r.adj_vals = r.gen = None
        r.fsm_cell = r.fsm_mask = None
        r.wm_cell = None
        r.miro_cell = None

    def _prepare_allow(self, r: _Request) -> None:
        """The allow mask of r's next pick: a pure host function of (r.sampling, r.tokens, r.eos) -- the host has read back
        every token r has generated before the pick that follows. A static mask is uploaded once and kept on the request; a
        step-dependent one (choices, allowed_tokens_fn) is one ceil(V / 32) * 4-byte upload for this row. Raises ValueError when the
        constraints leave nothing to emit (the caller fails this request alone)."""
        n = len(r.tokens)
        if r.allow_at == n:
            return
        key, mask = step_allow_mask(r.sampling, n, r.tokens, r.eos, int(self.model.config.vocab_size), r.allow_host)
        if mask is None:
            r.allow_cur = None
        elif key is not None and key in r.allow_dev:
            r.allow_cur = r.allow_dev[key]
        else:
            r.allow_cur = torch.from_numpy(mask.view("<i4")).to(self.model.device)
            r.mask_uploads += 1
            if key is not None:
                r.allow_dev[key] = r.allow_cur
        r.allow_at = n

    # ---- one scheduling step ---------------------------------------------------------------------------------------------
    def _pick(self, logits: torch.Tensor, reqs: Optional[List[_Request]] = None) -> torch.Tensor:
        """One token per logits row (row i belongs to reqs[i]). While no row's request carries `sampling` this is the launch it always
        was: ops.argmax, or ops.sample_top_p with the engine's scalars. Otherwise ONE ops.sample_rows launch serves every row: a request
        with `sampling` draws from (its seed, the number of tokens it has generated, stream 0); a request without gets the parameters
        that reproduce its legacy draw (the engine's temperature / top_p, top_k 0, the engine's seed, counter = the engine's step,
        stream = its batch row; greedy when the engine does not sample). Log-probabilities land in r.last_lp.
        A request whose SamplingParams carry a constraint passes its allow mask (_prepare_allow) and the launch is vt_sample_rows_allow;
        rows without one, and legacy rows, pass NULL. While no row has a mask the launches are exactly the ones above.
        A request with no_repeat_ngram_size / bad_words keeps its history and one working mask on the device: ONE
        vt_ban_rows launch in front of the sampler turns (the mask above as base, or NULL; the history; the rules) into the working masks
        of all such rows, and those rows' allow pointers name their working masks. Nothing is uploaded per step but the 48-byte rows, and
        the masks are never read back: a row they leave nothing for returns what vt_sample_rows_allow defines for it instead of failing.
        While no active request carries such a ban the launches are exactly the ones above.
        A request with SamplingParams(automaton=A) keeps a {state, consumed} cell, one working mask and the tokens it
        has generated on the device; A's tables are uploaded once per device and shared. ONE vt_fsm_rows launch, in front of the ban
        launch, moves every such row's state over the token fed last and turns (the mask above as base, or NULL; the state) into its
        working mask, which is the base of its vt_ban_row when it has a device ban too and what its allow pointer names otherwise.
        Nothing is uploaded per step but the 96-byte rows; the request's mask_uploads counts only what its other constraints cost.
        While no active request carries an automaton the launches are exactly the ones above.
        A request with `adjust` owns a [V][2] adjustment, its bias and its generated tokens on the device: ONE
        vt_bias_rows launch serves every row that needs a rebuild (a row with penalties at every pick, a bias-only row at its first pick
        only), the launch is vt_sample_rows_adj and the row's adjust pointer names its buffer; all other rows pass NULL. While no
        active request carries `adjust` the launches are exactly the ones above.
        A request whose SamplingParams are `truncated` (min_p, typical_p, epsilon_cutoff or eta_cutoff on a sampled request; DESIGN.md
        9.9) turns the launch into ONE vt_sample_rows_trunc: its row carries its four values, every other row an all-inactive entry,
        which the kernel treats bit for bit as vt_sample_rows_adj does. While no active request is truncated the launches are exactly
        the ones above.
        A request with SamplingParams(watermarking_config=) turns the launch into ONE vt_sample_rows_wm: its row names
        its cell, every other row carries cell = NULL, which the kernel treats bit for bit as vt_sample_rows_trunc does. While no active
        request is watermarked the launches are exactly the ones above.
        A request with SamplingParams(mirostat_tau=) turns the launch into ONE vt_sample_rows_miro: its row names its
        cell, tau and eta, every other row carries cell = NULL, which the kernel treats bit for bit as vt_sample_rows_trunc does. While
        no active request runs Mirostat the launches are exactly the ones above. A request cannot carry both (submit() refuses it), but
        a watermarked request and a Mirostat request can share a step: that step is TWO launches over all rows, one vt_sample_rows_wm and
        one vt_sample_rows_miro, and every row is taken from the launch that carries its entry.
        A request with SamplingParams(top_logprobs=N > 0): AFTER the pick, ONE vt_logprob_rows launch over the span of
        rows from the first to the last such request, the device ids just picked as targets and the largest N asked for as n_top (a
        shorter list is a prefix of a longer one, bit for bit). Its output stays on the device (r.last_top) until step() reads it back
        together with the tokens. While no row's request asks, the launches are exactly the ones above."""
        if reqs is None or all(r.sampling is None and r.adjust is None for r in reqs):
            if self.do_sample:
                return ops.sample_top_p(logits, self.temperature, self.top_p, self.seed, self._step)
            return ops.argmax(logits)
        rows = []
        for i, r in enumerate(reqs):
            sp = r.sampling
            if sp is None:
                rows.append((self.temperature if self.do_sample else 0.0, 0, self.top_p, 1.0, self.seed, self._step, i, 0, 0))
                continue
            if (sp.repetition_penalty != 1.0 or sp.device_bans) and r.hist is None:
                buf, lens = device_history(r.input_ids, r.max_new_tokens, nonneg=not sp.device_bans)
                r.hist, r.hist_len = buf[0], lens[0]
            rows.append((sp.temperature, sp.resolved_top_k(self.model.config), sp.top_p, sp.repetition_penalty, sp.seed, len(r.tokens), 0,
                         *((r.hist.data_ptr(), r.hist_len) if sp.repetition_penalty != 1.0 else (0, 0))))
        want_lp = any(r.sampling is not None and r.sampling.wants_logprobs for r in reqs)
        allow = None
        if any(r.sampling is not None and r.sampling.constrained for r in reqs):
            for r in reqs:
                if r.sampling is not None and r.sampling.constrained:
                    self._prepare_allow(r)
            allow = [r.allow_cur for r in reqs]
            fsm = [r for r in reqs if r.sampling is not None and r.sampling.automaton is not None]
            if fsm:
                V = int(logits.shape[1])
                fsm_rows = []
                for r in fsm:
                    if r.allow_cur is not None and r.allow_cur.numel() != mask_words(V):        # (the base is read for ceil(V / 32) words)
                        raise ValueError(f"request {r.rid}: its allow mask has {r.allow_cur.numel()} words, the logits have {V} columns")
                    A = r.sampling.automaton
                    if r.fsm_cell is None:
                        r.fsm_cell = torch.tensor([A.start, 0], dtype=torch.int32).to(logits.device)
                        r.fsm_mask = torch.empty((mask_words(V),), dtype=torch.int32, device=logits.device)
                        if r.gen is None:
                            r.gen = torch.zeros((max(r.max_new_tokens, 1),), dtype=torch.int32, device=logits.device)
                    n_gen = min(r.gen_len, int(r.gen.numel()))
                    fsm_rows.append((r.gen.data_ptr() if n_gen else 0, n_gen, r.fsm_cell.data_ptr(),
                                     0 if r.allow_cur is None else r.allow_cur.data_ptr(), r.fsm_mask.data_ptr(), *A.row_fields(logits.device),
                                     sorted(r.eos)))
                ops.fsm_rows(pack_fsm_rows(fsm_rows, logits.device), len(fsm_rows), V)
                allow = [r.fsm_mask if (r.sampling is not None and r.sampling.automaton is not None) else a for r, a in zip(reqs, allow)]
            ban = [r for r in reqs if r.sampling is not None and r.sampling.device_bans]
            if ban:
                V = int(logits.shape[1])
                ban_rows = []
                for r in ban:
                    base = r.fsm_mask if r.sampling.automaton is not None else r.allow_cur      # the automaton's mask holds allow_cur already
                    if base is not None and base.numel() != mask_words(V):                      # (the base is read for ceil(V / 32) words)
                        raise ValueError(f"request {r.rid}: its allow mask has {base.numel()} words, the logits have {V} columns")
                    if r.ban_mask is None:
                        r.ban_mask = torch.empty((mask_words(V),), dtype=torch.int32, device=logits.device)
                        if r.sampling.bad_words:
                            r.ban_seqs = torch.from_numpy(flatten_ban_seqs(r.sampling.bad_words)).to(logits.device)
                    n_ints = 0 if r.ban_seqs is None else int(r.ban_seqs.numel())
                    ban_rows.append((r.hist.data_ptr(), r.hist_len, 0 if base is None else base.data_ptr(),
                                     r.ban_mask.data_ptr(), r.sampling.no_repeat_ngram_size,
                                     0 if r.ban_seqs is None else r.ban_seqs.data_ptr(), len(r.sampling.bad_words or ()), n_ints))
                ops.ban_rows(pack_ban_rows(ban_rows, logits.device), len(ban_rows), V)
                allow = [r.ban_mask if (r.sampling is not None and r.sampling.device_bans) else a for r, a in zip(reqs, allow)]
            if all(a is None for a in allow):
                allow = None
        adj = None
        if any(r.adjust is not None for r in reqs):
            V, dev = int(logits.shape[1]), logits.device
            bias_rows = []
            for r in reqs:
                if r.adjust is None:
                    continue
                first = r.adj_buf is None
                if first:
                    r.adj_buf = torch.zeros((V, 2), dtype=torch.float32, device=dev)
                    if r.adjust.bias:
                        r.adj_ids = torch.tensor([t for t, _ in r.adjust.bias], dtype=torch.int32).to(dev)
                        r.adj_vals = torch.tensor([v for _, v in r.adjust.bias], dtype=torch.float32).to(dev)
                    if r.adjust.penalties and r.gen is None:
                        r.gen = torch.zeros((max(r.max_new_tokens, 1),), dtype=torch.int32, device=dev)
                elif r.adj_buf.numel() != 2 * V:                  # (the buffer is read for 2 * V floats)
                    raise ValueError(f"request {r.rid}: its adjustment was built for V = {r.adj_buf.numel() // 2}, the logits have {V} columns")
                if first or r.adjust.penalties:
                    n_gen = min(r.gen_len, int(r.gen.numel())) if r.gen is not None else 0
                    bias_rows.append((r.gen.data_ptr() if n_gen else 0, n_gen, 0 if r.adj_ids is None else r.adj_ids.data_ptr(),
                                      0 if r.adj_vals is None else r.adj_vals.data_ptr(), len(r.adjust.bias), r.adj_buf.data_ptr(),
                                      r.adjust.presence_penalty, r.adjust.frequency_penalty))
            if bias_rows:
                ops.bias_rows(pack_bias_rows(bias_rows, dev), len(bias_rows), V)
            adj = [r.adj_buf for r in reqs]
        trunc = None
        if any(r.sampling is not None and r.sampling.truncated for r in reqs):
            trunc = pack_trunc_rows([r.sampling.trunc_row if (r.sampling is not None and r.sampling.truncated) else None for r in reqs],
                                    logits.device)
        wm = None
        if any(r.sampling is not None and r.sampling.watermark is not None for r in reqs):
            from .watermark import pack_wm_rows
            entries = []
            for r in reqs:
                w = None if r.sampling is None else r.sampling.watermark
                if w is not None and r.wm_cell is None:
                    r.wm_cell = w.new_cell(logits.device)
                entries.append(None if w is None else (w, r.wm_cell))
            wm = pack_wm_rows(entries, logits.device)
        miro = None
        if any(r.sampling is not None and r.sampling.mirostat for r in reqs):
            from .sampling import new_miro_cell, pack_miro_rows
            entries = []
            for r in reqs:
                on = r.sampling is not None and r.sampling.mirostat
                if on and r.miro_cell is None:
                    r.miro_cell = new_miro_cell(r.sampling.mirostat_tau, logits.device)
                entries.append((r.miro_cell, r.sampling.mirostat_tau, r.sampling.mirostat_eta) if on else None)
            miro = pack_miro_rows(entries, logits.device)
        params = pack_sample_rows(rows, logits.device)
        if wm is not None and miro is not None:
            # Watermarked and Mirostat requests in one step: no kernel carries both, so the step is TWO launches over all rows, one per
            # array. A row's draw depends on its own entry alone and a launch touches only the cells its array names, so each kind of
            # row is taken from its own launch (every other row is vt_sample_rows_trunc's in both) and every request gets the ids it
            # gets alone.
            first = ops.sample_rows(logits, params, return_logprob=want_lp, allow=allow, adjust=adj, trunc=trunc, watermark=wm)
            second = ops.sample_rows(logits, params, return_logprob=want_lp, allow=allow, adjust=adj, trunc=trunc, miro=miro)
            on_miro = torch.tensor([r.sampling is not None and r.sampling.mirostat for r in reqs], dtype=torch.bool).to(logits.device)
            res = tuple(torch.where(on_miro, b, a) for a, b in zip(first, second)) if want_lp else torch.where(on_miro, second, first)
        else:
            res = ops.sample_rows(logits, params, return_logprob=want_lp, allow=allow, adjust=adj, trunc=trunc, watermark=wm, miro=miro)
        ids, lp = res if want_lp else (res, None)
        for i, r in enumerate(reqs):
            if r.sampling is not None and r.sampling.wants_logprobs:
                r.last_lp = lp[i:i + 1]
        ask = [i for i, r in enumerate(reqs) if r.sampling is not None and r.sampling.top_logprobs > 0]
        if ask:
            i0, n = ask[0], ask[-1] + 1 - ask[0]
            n_top = max(reqs[i].sampling.top_logprobs for i in ask)
            got = ops.logprob_rows(logits[i0:i0 + n], ids[i0:i0 + n], n_top, return_rank=True)
            for i in ask:
                reqs[i].last_top = (got["packed"], i - i0, n, n_top)
        return ids

    def _embed(self, r: _Request) -> torch.Tensor:
        m = self.model
        (_, _, _, _, embeds, _) = m.prepare_inputs_labels_for_multimodal(r.input_ids, None, None, None, None, r.images, r.regions,
                                                                         feature_cache=self._vis_cache if r.images is not None else None)
        if embeds is None:
            return m.get_model().embed_tokens(r.input_ids)[0]
        mask = torch.tensor(m._last_splice[0][0], dtype=torch.bool, device=embeds.device)
        lo = pair_lo(embeds)                  # precise levels 2 / 3: the spliced embeddings are an operand pair -- the low half travels explicitly
        r.flat_lo = None if lo is None else lo[0][mask]          # (a tensor attribute would not survive the indexing below: ADVICE r5)
        return embeds[0][mask]

    def _admit(self, reqs: List[_Request]) -> List[_Request]:
        """Multimodal prefill of the requests that fit: towers + splice per request (once: the rows and the page need stay on the
        request while it waits), decoder prefill per request (default) or one packed pass for all of them (batch_prefill). Every
        admitted request RESERVES its worst case up front -- pages for prompt + max_new_tokens are allocated here, so a sequence
        that is already decoding can never find the pool empty because a later admission took its pages. When nothing of this
        engine is live the pool is (re)built for the candidate batch, never beyond the constructor's `kv_pages`; if it cannot be
        grown (out of memory, pages held by someone else) the prefix of `reqs` that fits the pool there is gets admitted and the rest
        waits, as requests that do not fit next to running ones always do. Returns the requests that stay queued, in order.
        A request that fails on its own is moved to `failed` (module docstring); a device-level error propagates with the engine left
        as it was: pages taken by this call released, the surviving candidates back at the head of the queue."""
        m = self.model
        llama = m.get_model().llama
        live: List[_Request] = []                           # candidates that are still in the game
        for r in reqs:
            if r.flat is None:
                try:
                    r.flat = self._embed(r)
                    r.need = (r.flat.shape[0] + r.max_new_tokens + 63) // 64 + 1
                    if r.nseq is not None:                  # a guided request reserves its second sequence's worst case too
                        r.neg_flat = m.get_model().embed_tokens(r.neg_ids)[0]
                        r.need_neg = (r.neg_flat.shape[0] + r.max_new_tokens + 63) // 64 + 1
                        r.need += r.need_neg
                except Exception as e:  # noqa: BLE001 -- classified below
                    if self._is_device_error(e):
                        for q in reversed([x for x in reqs if x.error is None]):
                            self.waiting.appendleft(q)
                        raise
                    self._fail(r, e)                        # bad image shape / region / ids: this request's own problem
                    continue
            if self.kv_cap is not None and r.need > self.kv_cap:      # larger than the pool may ever be: no point in waiting
                self._fail(r, RuntimeError(f"request {r.rid} needs {r.need} KV pages, the pool is capped at {self.kv_cap}"))
                continue
            live.append(r)
        admitted: List[_Request] = []
        try:
            if not self.active and live:
                # idle: size the pool for every candidate (the first len(reqs) <= max_batch requests decode together), within the cap
                total = sum(r.need for r in live)
                want = total if self.kv_cap is None else min(total, self.kv_cap)
                if m.kv is None or len(m.kv.free) < want:
                    try:
                        m._ensure_kv(want)
                    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
                        if m.kv is None or (self._is_device_error(e) and not isinstance(e, torch.cuda.OutOfMemoryError)):
                            raise                           # no pool at all, or a HIP runtime error: nothing can be scheduled
                        # the pool could not grow: go on with the one that is there (the prefix that fits is admitted below)
            for r in live:
                if len(m.kv.free) < r.need:
                    if not admitted and not self.active and len(m.kv.free) == m.kv.num_pages:
                        # nothing is running, every page of the pool is free, the pool is as large as it could be made (the cap, or
                        # what the allocator gave), and the head request still does not fit: it never will -- fail it instead of
                        # blocking everything behind it
                        self._fail(r, RuntimeError(f"request {r.rid} needs {r.need} KV pages, the pool holds {m.kv.num_pages}"
                                                   + (f" (capped at {self.kv_cap})" if self.kv_cap is not None else "")))
                        continue
                    break                                   # wait for running requests to retire (or for an idle engine to grow the pool)
                pages = m.kv.alloc(r.need)
                r.seq.pages = pages[:r.need - r.need_neg]
                if r.nseq is not None:
                    r.nseq.pages = pages[r.need - r.need_neg:]
                admitted.append(r)
        except Exception:
            for r in admitted:
                self._release(r)
            for r in reversed(live):
                if r.error is None:
                    self.waiting.appendleft(r)
            raise
        rest = [r for r in live if r.error is None and r not in admitted]
        ok: List[_Request] = []

        def prefill_neg(r):      # a guided request's negative prompt: always a solo pass, as in generate() for the request alone
            return llama_forward(llama, m.kv, [r.nseq], r.neg_flat, [r.neg_flat.shape[0]])[0]

        def prefill_one(r):
            try:
                logits = self._forward(llama, [r.seq], r.flat, [r.flat.shape[0]], [r], embeds_lo=getattr(r, "flat_lo", None))
                if r.nseq is not None:
                    self._guide(logits, [r], {0: prefill_neg(r)})
                r.last = self._pick(logits, [r])
                ok.append(r)
            except Exception as e:  # noqa: BLE001
                if self._is_device_error(e):
                    raise
                self._fail(r, e)                            # e.g. a prompt beyond the rotary table: this request's own problem

        try:
            if self.batch_prefill and len(admitted) > 1:
                for r in list(admitted):                    # the first pick's masks before the shared forward, as step() does: a request
                    if r.sampling is not None and r.sampling.constrained:     # whose constraints leave nothing fails here, alone and once
                        try:
                            self._prepare_allow(r)
                        except Exception as e:  # noqa: BLE001
                            if self._is_device_error(e):
                                raise
                            admitted.remove(r)
                            self._fail(r, e)
            if self.batch_prefill and len(admitted) > 1:
                try:
                    flats = [r.flat for r in admitted]
                    los = [getattr(r, "flat_lo", None) for r in admitted]
                    lo_cat = None
                    if any(l is not None for l in los):      # (requests without visual rows have an exact 16-bit embedding: low half zero)
                        lo_cat = torch.cat([l if l is not None else torch.zeros_like(f) for l, f in zip(los, flats)], 0)
                    logits = self._forward(llama, [r.seq for r in admitted], torch.cat(flats, 0), [f.shape[0] for f in flats], admitted,
                                           embeds_lo=lo_cat)
                    unc = {i: prefill_neg(r) for i, r in enumerate(admitted) if r.nseq is not None}
                    if unc:
                        self._guide(logits, admitted, unc)
                    nxt = self._pick(logits, admitted)
                    for i, r in enumerate(admitted):
                        r.last = nxt[i:i + 1]
                    ok = list(admitted)
                except Exception as e:  # noqa: BLE001
                    if self._is_device_error(e):
                        raise
                    for r in admitted:                      # find the culprit: every request on its own (a solo prefill is always legal)
                        r.seq.length = 0
                        if r.nseq is not None:
                            r.nseq.length = 0
                        prefill_one(r)
            else:
                for r in admitted:
                    prefill_one(r)
        except Exception:                                   # device-level: pages back, every surviving candidate queued again
            for r in admitted:
                if r.error is None:
                    self._release(r)
                    r.last = None
            for r in reversed(live):
                if r.error is None:
                    self.waiting.appendleft(r)
            raise
        for r in ok:
            r.flat = r.flat_lo = r.neg_flat = None                       # the rows are in the cache now
        self.active += ok
        return rest

    def mirostat_state(self, rid: int) -> Optional[Tuple[float, float]]:
        """(mu, last_surprise) of a request with SamplingParams(mirostat_tau=): read from its cell while it runs (one 8-byte copy), what the cell held
        when it retired afterwards. None: no such request, no Mirostat, not picked yet, or failed / cancelled (the cell is gone)."""
        for r in self.active:
            if r.rid == rid:
                return None if r.miro_cell is None else tuple(float(x) for x in r.miro_cell.tolist())
        r = self.finished.get(rid)
        return None if r is None else r.miro_final

    def _retire(self, r: _Request) -> None:
        r.done = True
        if r.miro_cell is not None:
            r.miro_final = tuple(float(x) for x in r.miro_cell.tolist())
        self._release(r)
        r.hist = r.last_lp = r.last_top = None
        self._drop_masks(r)
        self.finished[r.rid] = r

    def step(self) -> List[Tuple[int, int]]:
        """Admit waiting requests while there is room, emit one token for every active request. Returns [(request id, token)]."""
        cand: List[_Request] = []
        rows = sum(r.rows for r in self.active)         # max_batch counts decode rows: a guided request takes two
        while self.waiting and rows + self.waiting[0].rows <= self.max_batch:
            rows += self.waiting[0].rows
            cand.append(self.waiting.popleft())
        if cand:
            for r in reversed(self._admit(cand)):          # what did not fit keeps its place at the head of the queue
                self.waiting.appendleft(r)
        if not self.active:
            return []
        # tokens chosen at the end of the previous step (or by the prefill) become visible now: ONE read-back per step
        toks = torch.cat([r.last for r in self.active]).tolist()
        with_lp = [r for r in self.active if r.last_lp is not None]
        if with_lp:
            for r, v in zip(with_lp, torch.cat([r.last_lp for r in with_lp]).tolist()):
                r.logprobs.append(float(v))
        with_top = [r for r in self.active if r.last_top is not None]
        if with_top:                                    # the same read-back point: the stream has been waited for above
            host = {}                                   # one copy per launch's buffer (a decode step: one buffer for all rows)
            for r in with_top:
                if id(r.last_top[0]) not in host:
                    host[id(r.last_top[0])] = r.last_top[0].cpu().numpy()
            for r in with_top:
                buf, j, n, n_top = r.last_top
                a = host[id(buf)]
                # planes of ops.logprob_rows' packed buffer: logprob [n], rank [n], top_ids [n, n_top], top_logprobs [n, n_top]
                k = r.sampling.top_logprobs
                ids_at = 2 * n + j * n_top
                lps_at = 2 * n + n * n_top + j * n_top
                r.top.append((int(a[n + j]), tuple(int(t) for t in a[ids_at:ids_at + k]),
                              tuple(float(v) for v in a[lps_at:lps_at + k].view(np.float32))))
                r.last_top = None
        out: List[Tuple[int, int]] = []
        still: List[_Request] = []
        for r, t in zip(self.active, toks):
            r.tokens.append(int(t))
            out.append((r.rid, int(t)))
            if int(t) in r.eos or len(r.tokens) >= r.max_new_tokens:
                self._retire(r)
            else:
                still.append(r)
        for r in list(still):        # the masks of the coming pick, before the forward: a request whose constraints leave nothing fails alone
            if r.sampling is not None and r.sampling.constrained:
                try:
                    self._prepare_allow(r)
                except Exception as e:  # noqa: BLE001 -- the request's own constraint (allowed_tokens_fn included)
                    if self._is_device_error(e):
                        raise
                    still.remove(r)
                    self._fail(r, e)
        self.active = still
        if self.active:
            m = self.model
            llama = m.get_model().llama
            # the active sequences, then the negative sequences of the guided ones (fed the same token): one pass
            guided = [i for i, r in enumerate(self.active) if r.nseq is not None]
            seqs = [r.seq for r in self.active] + [self.active[i].nseq for i in guided]
            ids = torch.cat([r.last for r in self.active] + [self.active[i].last for i in guided]).to(torch.int32)
            plan = torch.stack([torch.zeros_like(ids), ids], dim=1).contiguous()
            x = ops.embed_splice(llama.embed, None, None, plan)
            logits = self._forward(llama, seqs, x, [1] * len(seqs), self.active)
            if guided:
                n = len(self.active)
                unc = {i: logits[n + j] for j, i in enumerate(guided)}
                logits = logits[:n]
                self._guide(logits, self.active, unc)
            for r in self.active:                       # the token just fed joins the request's penalty / ban history, on the device
                if r.hist is not None:
                    r.hist[r.hist_len:r.hist_len + 1].copy_(r.last)
                    r.hist_len += 1
                if r.gen is not None and r.gen_len < int(r.gen.numel()):
                    r.gen[r.gen_len:r.gen_len + 1].copy_(r.last)
                    r.gen_len += 1
            nxt = self._pick(logits, self.active)
            for i, r in enumerate(self.active):
                r.last = nxt[i:i + 1]
        self._step += 1
        return out

    def run(self, on_token=None) -> Dict[int, torch.Tensor]:
        """Drive step() until every submitted request has finished; returns {request id: LongTensor of generated tokens}."""
        while self.pending():
            before = (len(self.waiting), len(self.failed), len(self.finished))
            emitted = self.step()
            for rid, t in emitted:
                if on_token is not None:
                    on_token(rid, t)
            if not emitted and not self.active and (len(self.waiting), len(self.failed), len(self.finished)) == before:
                # nothing admitted, nothing failed, nothing running: the KV pages the waiting requests need are held OUTSIDE this
                # engine (e.g. a past_key_values the caller keeps alive) and no later step can change that -- do not spin
                free = len(self.model.kv.free) if self.model.kv is not None else 0
                raise RuntimeError(f"ServingEngine.run: no progress -- {len(self.waiting)} request(s) waiting, none active, {free} KV pages free "
                                   f"(the head request needs {self.waiting[0].need}); pages are held outside the engine")
        return {rid: torch.tensor(r.tokens, dtype=torch.long) for rid, r in sorted(self.finished.items())}

    def logprobs(self, rid: int) -> torch.Tensor:
        """fp32 log-probabilities (log_softmax of the raw logits at the chosen id) of the tokens request `rid` has emitted so far, in
        order; the request must have been submitted with SamplingParams(logprobs=True)."""
        for r in list(self.finished.values()) + self.active:
            if r.rid == rid:
                if r.sampling is None or not r.sampling.wants_logprobs:
                    raise ValueError(f"request {rid} was not submitted with SamplingParams(logprobs=True)")
                return torch.tensor(r.logprobs, dtype=torch.float32)
        raise KeyError(f"request {rid} has emitted nothing (waiting, failed or unknown)")

    def top_logprobs(self, rid: int) -> List[tuple]:
        """One entry per token request `rid` has emitted so far, in order: (token, logprob, rank, top_ids, top_logprobs) -- the token, its
        log-probability (what logprobs() returns for it), its rank in the RAW distribution (1: the most likely; larger logit first, ties
        by the lower id), and the N most likely tokens with their log-probabilities as tuples. The request must have been submitted
        with SamplingParams(top_logprobs=N > 0)."""
        for r in list(self.finished.values()) + self.active:
            if r.rid == rid:
                if r.sampling is None or not r.sampling.top_logprobs:
                    raise ValueError(f"request {rid} was not submitted with SamplingParams(top_logprobs=N > 0)")
                return [(int(t), float(lp), rank, ids, lps) for t, lp, (rank, ids, lps) in zip(r.tokens, r.logprobs, r.top)]
        raise KeyError(f"request {rid} has emitted nothing (waiting, failed or unknown)")

    def errors(self) -> Dict[int, BaseException]:
        """{request id: exception} of the requests that failed on their own."""
        return {rid: r.error for rid, r in sorted(self.failed.items())}
