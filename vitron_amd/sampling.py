"""Per-request sampling parameters and their device form (struct vt_sample_row of include/vitron_hip.h).

`SamplingParams` is what a caller hands to `ServingEngine.submit(..., sampling=)`; `pack_sample_rows` turns one tuple per logits row
into the array `ops.sample_rows` / `vt_sample_rows` reads: one numpy structured array, one small host -> device copy.

Constrained decoding: which ids a request may emit at all is a V-bit allow mask per row (`allow_mask`, the layout of
vt_sample_rows_allow). `SamplingParams` carries the constraints; `step_allow_mask` is the pure host function that turns them and the
tokens generated so far into the mask of the next pick.

History-dependent bans: `no_repeat_ngram_size` and multi-token `bad_words` forbid ids that depend on what the request has
seen so far, so their mask is built on the DEVICE (struct vt_ban_row, `pack_ban_rows`, ops.ban_rows) from a device-resident history;
`history_bans` is the host statement of that contract.

Additive adjustments: a logit bias and the presence / frequency penalties add to a logit instead of forbidding it. A
row's adjustment is V pairs (pre, post) of fp32 built on the DEVICE (struct vt_bias_row, `pack_bias_rows`, ops.bias_rows) and read by
vt_sample_rows_adj; `LogitAdjust` is what a caller hands to `ServingEngine.submit(..., adjust=)`, `logit_adjust` the host statement of
the contract.

Truncation: min_p, typical_p, epsilon_cutoff and eta_cutoff are fields of `SamplingParams`; a row's four values are a
struct vt_trunc_row (`pack_trunc_rows`) that vt_sample_rows_trunc reads.

Token automata: `SamplingParams(automaton=A)` holds the reply to the language of a vitron_amd.automaton.TokenAutomaton
(a regex over the vocabulary's strings, a set of choices). The allowed set depends on where the reply stands, so the mask is built on the
DEVICE from a two-int cell per request (struct vt_fsm_row, `pack_fsm_rows`, ops.fsm_rows); nothing is uploaded per step.

Classifier-free guidance: `SamplingParams(guidance_scale=s, negative_prompt_ids=...)` blends the request's logits with
those of a second sequence that runs its negative prompt, in front of everything above: struct vt_cfg_row (`pack_cfg_rows`,
ops.cfg_rows); `log_beta` is the field of generate()'s plausibility cut.

DoLa: `SamplingParams(dola_layers=, dola_relative_top=)` contrasts the request's final logits with those of an early layer
it chooses per step (`dola_candidate_layers`, `check_dola`), in front of everything above: struct vt_dola_row (`pack_dola_rows`,
ops.dola_rows).

Mirostat v2: `SamplingParams(mirostat_tau=, mirostat_eta=)` steers the surprise of the reply to tau bits per token with a
cutoff that moves after every pick, inside the sampler behind the truncation stages: struct vt_miro_row (`pack_miro_rows`) names the
request's two-float cell {mu, last_surprise} on the device (`new_miro_cell`), which only the kernel changes.

Top-N log-probabilities: `SamplingParams(top_logprobs=N)` asks for the N most likely tokens and the chosen token's rank
at every generated token; they come from one vt_logprob_rows launch behind the pick and need no struct here.
"""
from __future__ import annotations

import dataclasses
import math
import numbers
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

# struct vt_sample_row: the offsets are part of the ABI (tests/test_sample_ref_host.py checks them against the header's table)
ROW_DTYPE = np.dtype({
    "names": ["temperature", "top_p", "top_k", "repetition_penalty", "seed", "counter", "history", "history_len", "stream"],
    "formats": ["<f4", "<f4", "<i4", "<f4", "<u8", "<u8", "<u8", "<i4", "<u4"],
    "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 44],
    "itemsize": 48,
})
ROW_BYTES = ROW_DTYPE.itemsize
_U64 = 2 ** 64 - 1
# struct vt_ban_row: the offsets are part of the ABI (tests/test_ban_ref_host.py checks them against the header's table)
BAN_ROW_DTYPE = np.dtype({
    "names": ["history", "base", "out", "seqs", "history_len", "ngram", "n_seqs", "seqs_len"],
    "formats": ["<u8", "<u8", "<u8", "<u8", "<i4", "<i4", "<i4", "<i4"],
    "offsets": [0, 8, 16, 24, 32, 36, 40, 44],
    "itemsize": 48,
})
BAN_ROW_BYTES = BAN_ROW_DTYPE.itemsize
# struct vt_fsm_row: the offsets are part of the ABI (tests/test_fsm_ref_host.py checks them against the header's table)
FSM_ROW_DTYPE = np.dtype({
    "names": ["gen", "cell", "base", "out", "offsets", "edge_tok", "edge_next", "state_info", "gen_len", "n_states", "n_edges", "n_eos", "eos"],
    "formats": ["<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<i4", "<i4", "<i4", "<i4", ("<i4", (4,))],
    "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80],
    "itemsize": 96,
})
FSM_ROW_BYTES = FSM_ROW_DTYPE.itemsize
FSM_MAX_EOS = 4                    # the eos[4] of vt_fsm_row
# struct vt_cfg_row: the offsets are part of the ABI (tests/test_cfg_ref_host.py checks them against the header's table)
CFG_ROW_DTYPE = np.dtype({
    "names": ["cond", "uncond", "out", "base", "mask_out", "lse_out", "scale", "log_beta"],
    "formats": ["<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<f4", "<f4"],
    "offsets": [0, 8, 16, 24, 32, 40, 48, 52],
    "itemsize": 56,
})
CFG_ROW_BYTES = CFG_ROW_DTYPE.itemsize
# struct vt_dola_row: the offsets are part of the ABI (tests/test_dola_ref_host.py checks them against the header's table)
DOLA_ROW_DTYPE = np.dtype({
    "names": ["final", "prem", "out", "base", "mask_out", "layer_out", "div_out", "lse_out", "prem_stride", "n_cand", "log_relative_top"],
    "formats": ["<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<i8", "<i4", "<f4"],
    "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76],
    "itemsize": 80,
})
DOLA_ROW_BYTES = DOLA_ROW_DTYPE.itemsize
DOLA_MAX_LAYERS = 16               # VT_DOLA_MAX_LAYERS
# struct vt_bias_row: the offsets are part of the ABI (tests/test_bias_ref_host.py checks them against the header's table)
BIAS_ROW_DTYPE = np.dtype({
    "names": ["history", "bias_ids", "bias_vals", "out", "history_len", "n_bias", "presence", "frequency"],
    "formats": ["<u8", "<u8", "<u8", "<u8", "<i4", "<i4", "<f4", "<f4"],
    "offsets": [0, 8, 16, 24, 32, 36, 40, 44],
    "itemsize": 48,
})
BIAS_ROW_BYTES = BIAS_ROW_DTYPE.itemsize
BIAS_ROWS_MAX_V = 65536            # VT_BIAS_ROWS_MAX_V
# struct vt_trunc_row: the offsets are part of the ABI (tests/test_trunc_ref_host.py checks them against the header's table)
TRUNC_ROW_DTYPE = np.dtype({
    "names": ["min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"],
    "formats": ["<f4", "<f4", "<f4", "<f4"],
    "offsets": [0, 4, 8, 12],
    "itemsize": 16,
})
TRUNC_ROW_BYTES = TRUNC_ROW_DTYPE.itemsize
# struct vt_miro_row: the offsets are part of the ABI (tests/test_miro_ref_host.py checks them against the header's table)
MIRO_ROW_DTYPE = np.dtype({
    "names": ["cell", "tau", "eta"],
    "formats": ["<u8", "<f4", "<f4"],
    "offsets": [0, 8, 12],
    "itemsize": 16,
})
MIRO_ROW_BYTES = MIRO_ROW_DTYPE.itemsize
MIRO_MAX_V = 32768                 # the sampler's register form: the only one that carries Mirostat
MIRO_TAU_MAX = 64.0                # bits: beyond any surprise an fp32 probability over <= 32768 tokens can state
TRUNC_OFF = (0.0, 1.0, 0.0, 0.0)   # (min_p, typical_p, epsilon_cutoff, eta_cutoff) of a row without truncation: every stage inactive


def check_truncation_values(min_p, typical_p, epsilon_cutoff, eta_cutoff, what: str = "sampling") -> None:
    """min_p in [0, 1] (0 is off), typical_p in (0, 1] (1 is off), epsilon_cutoff and eta_cutoff in [0, 1) (0 is off), all finite: the
    ranges of transformers' MinP / Typical / Epsilon / Eta warpers with their off values added."""
    def num(x):
        return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x)
    if not num(min_p) or not 0 <= min_p <= 1:
        raise ValueError(f"{what}: min_p must be a finite number in [0, 1] (0 is off), got {min_p!r}")
    if not num(typical_p) or not 0 < typical_p <= 1:
        raise ValueError(f"{what}: typical_p must be a finite number in (0, 1] (1 is off), got {typical_p!r}")
    for name, x in (("epsilon_cutoff", epsilon_cutoff), ("eta_cutoff", eta_cutoff)):
        if not num(x) or not 0 <= x < 1:
            raise ValueError(f"{what}: {name} must be a finite number in [0, 1) (0 is off), got {x!r}")


def check_mirostat(tau, eta, mode=2, what: str = "sampling") -> float:
    """The values of mirostat_tau / mirostat_eta / mirostat_mode; returns tau as a float, 0.0 when Mirostat is off (tau
    None or 0). ValueError: a tau that is not a finite number in [0, MIRO_TAU_MAX], an eta that is not a finite number in [0, 1], a mode
    that is not 0, 1 or 2. With Mirostat on, mode 1 (Mirostat v1: it needs the sorted top of the row for its Zipf estimate) is a
    NotImplementedError that names it, mode 0 a ValueError (it contradicts mirostat_tau). With tau off the feature is not in use and eta
    and mode are not looked at, as transformers ignores a warper's arguments when the warper is off."""
    def num(x):
        return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x)
    if tau is not None and (not num(tau) or not 0 <= tau <= MIRO_TAU_MAX):
        raise ValueError(f"{what}: mirostat_tau must be None or a finite number in [0, {MIRO_TAU_MAX:g}] bits (None and 0 are off), got "
                         f"{tau!r}")
    if not tau:
        return 0.0
    if not num(eta) or not 0 <= eta <= 1:
        raise ValueError(f"{what}: mirostat_eta must be a finite number in [0, 1], got {eta!r}")
    if not isinstance(mode, numbers.Integral) or isinstance(mode, bool) or mode not in (0, 1, 2):
        raise ValueError(f"{what}: mirostat_mode must be 0, 1 or 2, got {mode!r}")
    if mode == 1:
        raise NotImplementedError(f"{what}: mirostat_tau with mirostat_mode=1 (Mirostat v1) is not implemented; mirostat_mode=2 is")
    if mode == 0:
        raise ValueError(f"{what}: mirostat_tau={tau!r} with mirostat_mode=0 (off): give mirostat_mode=2 or leave mirostat_tau out")
    return float(tau)


def check_top_logprobs(n, what: str = "sampling") -> None:
    """top_logprobs is an int in [0, 20] (0 is off; 20 is VT_LOGPROB_MAX_TOP)."""
    if not isinstance(n, numbers.Integral) or isinstance(n, bool) or not 0 <= n <= 20:
        raise ValueError(f"{what}: top_logprobs must be an int in [0, 20] (0 is off), got {n!r}")


def truncation_active(min_p, typical_p, epsilon_cutoff, eta_cutoff) -> bool:
    """Is any of the four stages on (the kernel's rule: min_p > 0, the others inside (0, 1))?"""
    return bool(min_p > 0 or 0 < typical_p < 1 or 0 < epsilon_cutoff < 1 or 0 < eta_cutoff < 1)


def check_sampling_values(temperature, top_p, top_k, repetition_penalty, what: str = "sampling") -> None:
    """What Python guarantees before anything is uploaded: temperature >= 0, top_p > 0, top_k >= 0, repetition_penalty > 0, all finite.
    (The kernel is total whatever the fields hold; these are the values that MEAN something.)"""
    def num(x):
        return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x)
    if not num(temperature) or temperature < 0:
        raise ValueError(f"{what}: temperature must be a finite number >= 0 (0 is greedy), got {temperature!r}")
    if not num(top_p) or top_p <= 0:
        raise ValueError(f"{what}: top_p must be a finite number > 0 (>= 1 keeps all), got {top_p!r}")
    if top_k is not None and (not isinstance(top_k, numbers.Integral) or isinstance(top_k, bool) or top_k < 0 or top_k > 2 ** 31 - 1):
        raise ValueError(f"{what}: top_k must be None or an int >= 0 (0 is off), got {top_k!r}")
    if not num(repetition_penalty) or repetition_penalty <= 0:
        raise ValueError(f"{what}: repetition_penalty must be a finite number > 0 (1 is off), got {repetition_penalty!r}")


@dataclass(frozen=True)
class _SamplingFields:
    """The dataclass part of SamplingParams (below): its field list is pinned (tests/test_allow_ref_host.py).
    How ONE request picks its tokens. temperature 0 is greedy; top_k None means config.top_k (default 50, as in `generate`);
    `seed` with the number of tokens generated so far is the whole state of the request's random stream, so its draws do not depend on
    what else is in the batch. logprobs=True collects the chosen token's log-probability per step (ServingEngine.logprobs).
    The last two fields are history-dependent bans: no_repeat_ngram_size (int >= 0, 0 is off: no n-gram of
    that size occurs twice in prompt + reply, NoRepeatNGramLogitsProcessor) and bad_words (non-empty id sequences, one or several tokens:
    the last id of a sequence is banned while the ids before it are the end of prompt + reply, NoBadWordsLogitsProcessor). Their masks
    depend on the history and are built on the device, never read back: a step at which they leave nothing to emit cannot raise; the
    row returns what vt_sample_rows_allow defines for a row with nothing allowed."""
    temperature: float = 0.0
    top_p: float = 1.0
    top_k: Optional[int] = None
    seed: int = 0
    repetition_penalty: float = 1.0
    logprobs: bool = False
    # ---- constraints: which ids the request may emit at all (all off by default; they compose by intersection) ----
    allowed_token_ids: Optional[Tuple[int, ...]] = None      # only these ids, at every step
    banned_token_ids: Optional[Tuple[int, ...]] = None       # never these (SuppressTokensLogitsProcessor, single-token NoBadWords)
    min_new_tokens: int = 0                                  # the request's EOS ids are banned while it has generated fewer tokens
    choices: Optional[Tuple[Tuple[int, ...], ...]] = None    # the reply is exactly one of these id sequences, followed by EOS
    allowed_tokens_fn: Optional[Callable] = None             # generated ids -> iterable of allowed ids, or None (PrefixConstrained)
    # ---- history-dependent bans: their masks are built on the device from the request's history ----
    no_repeat_ngram_size: int = 0                            # no n-gram of this size occurs twice in prompt + reply (0 is off)
    bad_words: Optional[Tuple[Tuple[int, ...], ...]] = None  # id sequences whose last id is banned while the ids before it end the history

    def __post_init__(self):
        def ids(x, what):
            if x is None:
                return None
            if isinstance(x, (str, bytes)) or not hasattr(x, "__iter__"):
                raise ValueError(f"SamplingParams: {what} must be a sequence of token ids, got {x!r}")
            return tuple(_as_id(t, what) for t in x)
        object.__setattr__(self, "allowed_token_ids", ids(self.allowed_token_ids, "allowed_token_ids"))
        object.__setattr__(self, "banned_token_ids", ids(self.banned_token_ids, "banned_token_ids"))
        for name in ("choices", "bad_words"):
            seqs = getattr(self, name)
            if seqs is not None:
                if isinstance(seqs, (str, bytes)) or not hasattr(seqs, "__iter__"):
                    raise ValueError(f"SamplingParams: {name} must be a sequence of token-id sequences, got {seqs!r}")
                object.__setattr__(self, name, tuple(ids(c, name) for c in seqs))
        self.validate()

    def validate(self) -> None:
        check_sampling_values(self.temperature, self.top_p, self.top_k, self.repetition_penalty, "SamplingParams")
        if not isinstance(self.seed, numbers.Integral) or isinstance(self.seed, bool):
            raise ValueError(f"SamplingParams: seed must be an int, got {self.seed!r}")
        if not isinstance(self.logprobs, bool):
            raise ValueError(f"SamplingParams: logprobs must be a bool, got {self.logprobs!r}")
        if not isinstance(self.min_new_tokens, numbers.Integral) or isinstance(self.min_new_tokens, bool) or self.min_new_tokens < 0:
            raise ValueError(f"SamplingParams: min_new_tokens must be an int >= 0, got {self.min_new_tokens!r}")
        if self.allowed_token_ids is not None and len(self.allowed_token_ids) == 0:
            raise ValueError("SamplingParams: allowed_token_ids is empty: nothing could be emitted")
        if self.choices is not None and (len(self.choices) == 0 or any(len(c) == 0 for c in self.choices)):
            raise ValueError("SamplingParams: choices must hold at least one choice and no empty one")
        if self.allowed_tokens_fn is not None and not callable(self.allowed_tokens_fn):
            raise ValueError(f"SamplingParams: allowed_tokens_fn must be callable, got {self.allowed_tokens_fn!r}")
        g = self.no_repeat_ngram_size
        if not isinstance(g, numbers.Integral) or isinstance(g, bool) or g < 0 or g > 2 ** 31 - 1:
            raise ValueError(f"SamplingParams: no_repeat_ngram_size must be an int >= 0 (0 is off), got {g!r}")
        if self.bad_words is not None and any(len(w) == 0 for w in self.bad_words):
            raise ValueError("SamplingParams: bad_words must hold no empty sequence")

    @property
    def device_bans(self) -> bool:
        """Does the request need a mask built on the device from its history (vt_ban_rows)?"""
        return self.no_repeat_ngram_size > 0 or bool(self.bad_words)

    @property
    def constrained(self) -> bool:
        return (self.allowed_token_ids is not None or bool(self.banned_token_ids) or self.min_new_tokens > 0
                or self.choices is not None or self.allowed_tokens_fn is not None or self.device_bans)

    def resolved_top_k(self, config=None) -> int:
        if self.top_k is not None:
            return int(self.top_k)
        return int(getattr(config, "top_k", 50) or 0)


class SamplingParams(_SamplingFields):
    """What a caller hands to ServingEngine.submit(..., sampling=): the fields above, and behind them four truncation settings
     -- min_p (MinPLogitsWarper: q < min_p * max q leaves; 0 is off), typical_p (TypicalLogitsWarper: the mass kept around
    the entropy; 1 is off), epsilon_cutoff (EpsilonLogitsWarper: q < epsilon leaves; 0 is off) and eta_cutoff (EtaLogitsWarper: q <
    min(eta, sqrt(eta) * exp(-entropy)) leaves; 0 is off). They run in that order after top-k and top-p inside the sampler kernel
    (vt_sample_rows_trunc), on a sampled request only; a greedy one ignores them.
    The four are keyword arguments of the constructor, frozen, validated, and part of ==, hash, repr and replace() like every field --
    but they are attributes of this subclass, not dataclass fields: the field list is pinned as it is, so dataclasses.replace() would
    drop them; use SamplingParams.replace().
    top_logprobs is a fifth attribute of the same kind: an int in [0, TOP_LOGPROBS_MAX]; N > 0 collects, per generated
    token, its log-probability, its rank and the N most likely tokens of the RAW distribution with their log-probabilities
    (ServingEngine.top_logprobs; one vt_logprob_rows launch per step). It implies what logprobs=True collects. repr shows it when set.
    automaton is a sixth: None, or a vitron_amd.automaton.TokenAutomaton the reply has to follow (guided decoding by
    regex or choices). It makes the request `constrained`; its mask is built on the device by vt_fsm_rows from the request's own
    {state, consumed} cell and intersects with every other constraint. Compared and hashed by identity; repr shows it when set.
    guidance_scale and negative_prompt_ids are of the same kind: classifier-free guidance against a TEXT-ONLY negative
    prompt (a sequence of ids >= 0, stored as a tuple; None: the last token of the request's prompt). None or 1 is off. A guided request
    owns a second sequence and two decode rows; its logits are blended by vt_cfg_rows in front of everything else the request asks for.
    guidance_plausibility and negative_images exist to be refused (NotImplementedError): the engine runs neither. repr shows them when set.
    dola_layers and dola_relative_top are of the same kind: DoLa decoding, generate(dola_layers=...)'s arguments --
    "low", "high" or a sequence of layer indices (stored as a tuple; resolved against the model at submit()), None is off;
    dola_relative_top in (0, 1], 0.1 by default. A DoLa request takes one decode row. Refused together with guidance_scale
    (NotImplementedError). repr shows them when dola_layers is set.
    watermarking_config is of the same kind: a transformers SynthIDTextWatermarkingConfig, a dict of its fields or a
    vitron_amd.watermark.SynthIDWatermark, resolved at construction and kept as `.watermark` (None is off). The request's draws go through
    the SynthID tournament inside the sampler (vt_sample_rows_wm), its state in a cell on the device. A sampled request only: with
    temperature 0 it is refused (NotImplementedError). Compared by the configuration's values; repr shows it when set.
    mirostat_tau and mirostat_eta are of the same kind: Mirostat v2 (llama.cpp's `mirostat 2`) with the target surprise
    tau in bits (None and 0 are off) and the learning rate eta (0.1 by default), inside the sampler behind the truncation stages
    (vt_sample_rows_miro); the request's {mu, last_surprise} lives in a cell on the device (ServingEngine.mirostat_state). ValueError here for a
    value outside its range; a greedy request and one with watermarking_config are refused at submit() (check_constraints). repr shows
    them when mirostat_tau is on."""
    MIRO_NAMES = ("mirostat_tau", "mirostat_eta")
    DOLA_NAMES = ("dola_layers", "dola_relative_top")
    GUIDE_NAMES = ("guidance_scale", "negative_prompt_ids", "guidance_plausibility", "negative_images")
    TRUNC_NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
    TOP_LOGPROBS_MAX = 20                        # VT_LOGPROB_MAX_TOP

    def __init__(self, *args, min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0,
                 top_logprobs: int = 0, automaton=None, guidance_scale=None, negative_prompt_ids=None, guidance_plausibility=0.0,
                 negative_images=None, dola_layers=None, dola_relative_top=0.1, watermarking_config=None, mirostat_tau=None,
                 mirostat_eta=0.1, **kw):
        for name, value in zip(self.TRUNC_NAMES, (min_p, typical_p, epsilon_cutoff, eta_cutoff)):
            object.__setattr__(self, name, value)
        object.__setattr__(self, "top_logprobs", top_logprobs)
        object.__setattr__(self, "automaton", automaton)
        if negative_prompt_ids is not None:      # a tensor, an array or a sequence (one prompt; a [1, Ln] batch of one is taken as it)
            flat = np.asarray(negative_prompt_ids.cpu() if hasattr(negative_prompt_ids, "cpu") else negative_prompt_ids)
            if flat.ndim == 2 and flat.shape[0] == 1:
                flat = flat[0]
            negative_prompt_ids = tuple(flat.tolist()) if flat.ndim == 1 else flat
        for name, value in zip(self.GUIDE_NAMES, (guidance_scale, negative_prompt_ids, guidance_plausibility, negative_images)):
            object.__setattr__(self, name, value)
        object.__setattr__(self, "dola_layers", tuple(dola_layers) if isinstance(dola_layers, list) else dola_layers)
        object.__setattr__(self, "dola_relative_top", dola_relative_top)
        from .watermark import as_watermark      # (its ValueError / NotImplementedError: the green-list scheme, debug_mode, ...)
        object.__setattr__(self, "watermark", as_watermark(watermarking_config))
        object.__setattr__(self, "mirostat_tau", mirostat_tau)
        object.__setattr__(self, "mirostat_eta", mirostat_eta)
        super().__init__(*args, **kw)            # (its __post_init__ validates: the four are set by then)

    def __setattr__(self, name, value):          # (the frozen base guards its own fields only once it is subclassed)
        raise dataclasses.FrozenInstanceError(f"cannot assign to field {name!r}")

    def __delattr__(self, name):
        raise dataclasses.FrozenInstanceError(f"cannot delete field {name!r}")

    def validate(self) -> None:
        super().validate()
        check_truncation_values(*self.trunc_row_raw(), what="SamplingParams")
        check_top_logprobs(self.top_logprobs, "SamplingParams")
        if self.automaton is not None:
            from .automaton import TokenAutomaton
            if not isinstance(self.automaton, TokenAutomaton):
                raise ValueError(f"SamplingParams: automaton must be a TokenAutomaton or None, got {self.automaton!r}")
        if self.negative_images is not None:
            raise NotImplementedError("SamplingParams: negative_images is not implemented (the engine's negative prompt is text-only; use "
                                      "generate(negative_images=...))")
        if self.guidance_plausibility:
            raise NotImplementedError("SamplingParams: guidance_plausibility is not implemented in the engine; use "
                                      "generate(guidance_plausibility=...)")
        g = self.guidance_scale
        if g is not None and (not isinstance(g, numbers.Real) or isinstance(g, bool) or not math.isfinite(g)):
            raise ValueError(f"SamplingParams: guidance_scale must be None or a finite number (None and 1 are off), got {g!r}")
        n = self.negative_prompt_ids
        if n is not None:
            if g is None:
                raise ValueError("SamplingParams: negative_prompt_ids needs guidance_scale")
            if not isinstance(n, tuple) or not n:
                raise ValueError("SamplingParams: negative_prompt_ids must be one non-empty sequence of token ids")
            if any(not isinstance(t, numbers.Integral) or isinstance(t, bool) or t < 0 for t in n):
                raise ValueError("SamplingParams: negative_prompt_ids is text-only here: every entry must be a token id >= 0 (no image / "
                                 "region sentinels)")

        # (the layer indices are checked against the model at submit(): 2 ** 30 stands for "any depth" here)
        check_dola(self.dola_layers, self.dola_relative_top, 2 ** 30, what="SamplingParams")
        if self.dola and self.guided:
            raise NotImplementedError("SamplingParams: dola_layers together with guidance_scale is not implemented: one contrast per request")
        if self.watermark is not None and not self.temperature > 0:
            raise NotImplementedError("SamplingParams: watermarking_config on a greedy request (temperature 0) is not implemented: the "
                                      "SynthID tournament reshapes the distribution a token is DRAWN from")
        check_mirostat(self.mirostat_tau, self.mirostat_eta, 2, "SamplingParams")

    @property
    def mirostat(self) -> bool:
        """Does the request run Mirostat v2 (vt_sample_rows_miro, a cell on the device)?"""
        return bool(self.mirostat_tau)

    @property
    def dola(self) -> bool:
        """Does the request run DoLa (vt_dola_rows in front of its pick)?"""
        return self.dola_layers is not None

    @property
    def guided(self) -> bool:
        """Does the request run classifier-free guidance (a second sequence, vt_cfg_rows in front of its pick)?"""
        return self.guidance_scale is not None and self.guidance_scale != 1

    @property
    def constrained(self) -> bool:
        return super().constrained or self.automaton is not None

    @property
    def wants_logprobs(self) -> bool:
        """Is the chosen token's log-probability collected (logprobs=True, or implied by top_logprobs > 0)?"""
        return bool(self.logprobs) or self.top_logprobs > 0

    def trunc_row_raw(self) -> tuple:
        return tuple(getattr(self, n) for n in self.TRUNC_NAMES)

    def _key(self) -> tuple:
        return tuple(getattr(self, n) for n in self.__dataclass_fields__) + self.trunc_row_raw() + (int(self.top_logprobs),) \
            + (None if self.automaton is None else id(self.automaton),) \
            + ((self.guidance_scale, self.negative_prompt_ids) if self.guidance_scale is not None or self.negative_prompt_ids is not None else ()) \
            + (("dola", self.dola_layers, self.dola_relative_top) if self.dola_layers is not None else ()) \
            + (("watermark", self.watermark.key()) if self.watermark is not None else ()) \
            + (("mirostat", float(self.mirostat_tau), float(self.mirostat_eta)) if self.mirostat else ())

    def __eq__(self, other):
        return self._key() == other._key() if other.__class__ is self.__class__ else NotImplemented

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        names = list(self.__dataclass_fields__) + list(self.TRUNC_NAMES)
        if self.top_logprobs:
            names.append("top_logprobs")
        if self.automaton is not None:
            names.append("automaton")
        names += [n for n, off in zip(self.GUIDE_NAMES, (None, None, 0.0, None)) if getattr(self, n) is not off and getattr(self, n) != off]
        if self.dola_layers is not None:
            names += list(self.DOLA_NAMES)
        if self.mirostat:
            names += list(self.MIRO_NAMES)
        wm = "" if self.watermark is None else f", watermarking_config={self.watermark.to_dict()!r}"
        return "SamplingParams(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in names) + wm + ")"

    def replace(self, **changes) -> "SamplingParams":
        """A copy with some settings changed (dataclasses.replace knows only the dataclass fields)."""
        kw = {n: getattr(self, n) for n in list(self.__dataclass_fields__) + list(self.TRUNC_NAMES) + ["top_logprobs", "automaton"]
              + list(self.GUIDE_NAMES) + list(self.DOLA_NAMES)}
        kw["watermarking_config"] = self.watermark
        kw.update({n: getattr(self, n) for n in self.MIRO_NAMES})
        kw.update(changes)
        return SamplingParams(**kw)

    @property
    def truncated(self) -> bool:
        """Does the request need vt_sample_rows_trunc (a sampled request with min_p, typical_p, epsilon_cutoff or eta_cutoff on)?"""
        return self.temperature > 0 and truncation_active(*self.trunc_row_raw())

    @property
    def trunc_row(self) -> Tuple[float, float, float, float]:
        """(min_p, typical_p, epsilon_cutoff, eta_cutoff) of the request's vt_trunc_row"""
        return tuple(float(x) for x in self.trunc_row_raw())


def _as_id(t, what: str) -> int:
    if not isinstance(t, numbers.Integral) or isinstance(t, bool):
        raise ValueError(f"SamplingParams: {what} holds {t!r}, not a token id")
    return int(t)


# ---- allow masks: the word / bit layout of vt_sample_rows_allow ---------------------------------------------------------------------
def mask_words(V: int) -> int:
    return (int(V) + 31) // 32


def allow_mask(V: int, allowed: Optional[Iterable[int]] = None, banned: Optional[Iterable[int]] = None) -> np.ndarray:
    """uint32 [ceil(V / 32)]: token i may be chosen iff bit (i & 31) of word (i >> 5) is set. The allowed set (every id of [0, V) when
    None) minus the banned ids; bits at positions >= V stay clear. An id outside [0, V) is a ValueError."""
    V = int(V)
    if V <= 0:
        raise ValueError(f"allow_mask: V must be > 0, got {V}")

    def ids(x, what):
        a = np.asarray(x if isinstance(x, np.ndarray) else list(x), dtype=np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= V):
            bad = a[(a < 0) | (a >= V)]
            raise ValueError(f"allow_mask: {what} id {int(bad[0])} is outside [0, {V})")
        return a
    bits = np.zeros((mask_words(V) * 32,), dtype=bool)
    if allowed is None:
        bits[:V] = True
    else:
        bits[ids(allowed, "allowed")] = True
    if banned is not None:
        bits[ids(banned, "banned")] = False
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def mask_ids(mask: np.ndarray, V: int) -> np.ndarray:
    """The ids in [0, V) whose bit is set (the inverse of allow_mask)."""
    bits = np.unpackbits(np.ascontiguousarray(mask, dtype="<u4").view(np.uint8), bitorder="little")[:V]
    return np.nonzero(bits)[0]


class TokenTrie:
    """The choices of SamplingParams.choices as a trie over token ids: node = the ids generated so far; `children(prefix)` are the ids
    that may come next, `ends(prefix)` says whether the prefix is a complete choice (EOS may follow)."""

    def __init__(self, choices: Sequence[Sequence[int]]):
        self.root: dict = {}
        for c in choices:
            node = self.root
            for t in c:
                node = node.setdefault(int(t), {})
            node[None] = True               # end marker: a choice ends at this node

    def _node(self, prefix: Sequence[int]):
        node = self.root
        for t in prefix:
            node = node.get(int(t))
            if node is None:
                return None
        return node

    def children(self, prefix: Sequence[int]) -> list:
        node = self._node(prefix)
        return [] if node is None else sorted(t for t in node if t is not None)

    def ends(self, prefix: Sequence[int]) -> bool:
        node = self._node(prefix)
        return node is not None and None in node


def step_allow_mask(sampling: Optional[SamplingParams], n_generated: int, tokens: Sequence[int], eos: Iterable[int], V: int,
                    cache: Optional[Dict] = None):
    """The allow mask of a request's NEXT pick as a pure host function of (sampling, tokens generated so far, the request's EOS ids):
    returns (key, mask). mask is None when the step is unconstrained (the row passes NULL), else uint32 [ceil(V / 32)]. key names a
    mask that does not depend on the tokens ("pre": fewer than min_new_tokens generated, "post": after) so that its device copy can be
    kept; it is None for a step-dependent mask (choices, allowed_tokens_fn). `cache` (a dict the caller keeps per request) holds the
    static masks and the trie between calls. All constraints intersect; an empty result is a ValueError."""
    if sampling is None or not sampling.constrained:
        return None, None
    cache = {} if cache is None else cache
    eos_in = sorted(int(e) for e in eos if isinstance(e, numbers.Integral) and 0 <= int(e) < V)
    key = "pre" if n_generated < sampling.min_new_tokens else "post"
    if key not in cache:
        static = None
        banned = list(sampling.banned_token_ids or ()) + (eos_in if key == "pre" else [])
        if sampling.allowed_token_ids is not None or banned:
            static = allow_mask(V, sampling.allowed_token_ids, banned)
            if not static.any():
                raise ValueError(f"sampling constraints leave no token to emit ({'before' if key == 'pre' else 'after'} min_new_tokens)")
        cache[key] = static
    mask = cache[key]
    dynamic = False
    if sampling.choices is not None:
        if not eos_in:
            raise ValueError(f"choices need an EOS id inside [0, {V}) to end the reply")
        trie = cache.get("trie")
        if trie is None:
            trie = cache["trie"] = TokenTrie(sampling.choices)
        nxt = trie.children(tokens) + (eos_in if trie.ends(tokens) else [])
        step = allow_mask(V, nxt)
        mask, dynamic = step if mask is None else (mask & step), True
    if sampling.allowed_tokens_fn is not None:
        got = sampling.allowed_tokens_fn(list(tokens))
        if got is not None:
            step = allow_mask(V, got)
            mask, dynamic = step if mask is None else (mask & step), True
    if mask is not None and dynamic and not mask.any():
        raise ValueError(f"sampling constraints leave no token to emit after {n_generated} generated token(s)")
    return (None if dynamic else (key if mask is not None else None)), mask


def check_constraints(sampling: Optional[SamplingParams], eos: Iterable[int], V: int) -> None:
    """What submit() refuses before anything is queued: ids outside [0, V) (those of bad_words included), choices without an EOS id in
    [0, V), a combination that leaves nothing to emit (the static masks before / after min_new_tokens and the first step of `choices`;
    allowed_tokens_fn is not called here, and what no_repeat_ngram_size / bad_words leave is known on the device only).
    First of all, what a request with mirostat_tau refuses (NotImplementedError, by name): a greedy request, one with
    watermarking_config, a vocabulary beyond the sampler's register form."""
    if sampling is not None and getattr(sampling, "mirostat", False):
        check_mirostat_request(not sampling.temperature > 0, 1, 0.0, False, sampling.watermark is not None, V,
                               "SamplingParams(mirostat_tau=...)", greedy_name="temperature=0")
    if sampling is None or not sampling.constrained:
        return
    sp = sampling.replace(allowed_tokens_fn=None)
    for c in (sp.choices or ()) + (sp.bad_words or ()):
        allow_mask(V, c)
    cache: Dict = {}
    step_allow_mask(sp, 0, [], eos, V, cache)
    if sp.min_new_tokens > 0:
        step_allow_mask(sp.replace(choices=None), sp.min_new_tokens, [], eos, V, {})


def _upload_rows(arr: np.ndarray, device):
    """A host array of row structs as a uint8 device tensor [len(arr), bytes per struct]: the form every ops.*_rows launcher takes."""
    import torch
    return torch.from_numpy(arr.view(np.uint8).reshape(len(arr), arr.dtype.itemsize)).to(device)


def sample_rows_array(rows: Sequence[tuple]) -> np.ndarray:
    """Host array of vt_sample_row from one tuple per row:
        (temperature, top_k, top_p, repetition_penalty, seed, counter, stream, history_ptr, history_len)
    history_ptr is a DEVICE address (tensor.data_ptr(), 0 for none) whose owner the caller keeps alive until the launch has run.
    Values are validated here (check_sampling_values); seed wraps to 64 bits like vt_sample_top_p's."""
    arr = np.zeros((len(rows),), dtype=ROW_DTYPE)
    for i, (temperature, top_k, top_p, penalty, seed, counter, stream, hist_ptr, hist_len) in enumerate(rows):
        check_sampling_values(temperature, top_p, int(top_k), penalty, f"sample row {i}")
        if counter < 0 or stream < 0 or stream > 2 ** 32 - 1 or hist_len < 0 or (hist_len > 0 and not hist_ptr):
            raise ValueError(f"sample row {i}: counter / stream / history out of range")
        arr[i] = (temperature, top_p, int(top_k), penalty, int(seed) & _U64, int(counter) & _U64, int(hist_ptr), int(hist_len), int(stream))
    return arr


def pack_sample_rows(rows: Sequence[tuple], device):
    """Device form of `sample_rows_array(rows)`: a uint8 tensor [len(rows), 48] for ops.sample_rows."""
    return _upload_rows(sample_rows_array(rows), device)


# ---- truncation: struct vt_trunc_row ---------------------------------------------------------------------------------------------------
def trunc_rows_array(rows: Sequence[Optional[tuple]]) -> np.ndarray:
    """Host array of vt_trunc_row from one entry per row: (min_p, typical_p, epsilon_cutoff, eta_cutoff), or None for a row without
    truncation (TRUNC_OFF: every stage inactive). Values are validated here (check_truncation_values)."""
    arr = np.zeros((len(rows),), dtype=TRUNC_ROW_DTYPE)
    for i, t in enumerate(rows):
        t = TRUNC_OFF if t is None else tuple(t)
        if len(t) != 4:
            raise ValueError(f"trunc row {i}: expected (min_p, typical_p, epsilon_cutoff, eta_cutoff), got {t!r}")
        check_truncation_values(*t, what=f"trunc row {i}")
        arr[i] = tuple(float(x) for x in t)
    return arr


def pack_trunc_rows(rows: Sequence[Optional[tuple]], device):
    """Device form of `trunc_rows_array(rows)`: a uint8 tensor [len(rows), 16] for ops.sample_rows(..., trunc=)."""
    return _upload_rows(trunc_rows_array(rows), device)


# ---- Mirostat v2: struct vt_miro_row (the host statement of the contract is tests/miro_ref.py) ----------------------------------------
def check_mirostat_request(greedy: bool, num_beams: int, penalty_alpha: float, padded_batch: bool, watermark: bool, V: int, what: str,
                           greedy_name: str = "do_sample=False") -> None:
    """What a call or request with mirostat_tau refuses, by name and in this order (NotImplementedError): a greedy pick, beams,
    contrastive search, padded_batch, watermarking_config, a vocabulary beyond the sampler's register form."""
    for bad, name, why in ((greedy, greedy_name, "Mirostat truncates the distribution a token is DRAWN from"),
                           (num_beams > 1, "num_beams > 1", "beams are not sampled"),
                           (penalty_alpha > 0, "penalty_alpha > 0", "contrastive search is not sampled"),
                           (padded_batch, "padded_batch=True", "use the default packed batch"),
                           (watermark, "watermarking_config=...", "Mirostat together with the SynthID watermark is not built")):
        if bad:
            raise NotImplementedError(f"{what}: mirostat_tau with {name} is not implemented: {why}")
    if int(V) > MIRO_MAX_V:
        raise NotImplementedError(f"{what}: mirostat_tau: vocab_size={int(V)} is beyond the sampler's register form ({MIRO_MAX_V}), the only "
                                  "one that carries Mirostat")


def new_miro_cell(tau: float, device):
    """A fresh Mirostat cell on `device`: fp32 {mu = 2 * tau, last_surprise = 0}. Written here once; after that only the kernel writes it."""
    import torch
    return torch.tensor([2.0 * float(tau), 0.0], dtype=torch.float32).to(device)


def miro_rows_array(rows: Sequence[Optional[tuple]]) -> np.ndarray:
    """Host array of vt_miro_row from one entry per row: None (cell = NULL: the row runs no Mirostat) or (cell_ptr, tau, eta). cell_ptr
    is a DEVICE address (tensor.data_ptr()) of two fp32 words, 8-byte aligned, whose owner the caller keeps alive. Values are validated
    here (check_mirostat); tau 0 makes the row one without Mirostat."""
    arr = np.zeros((len(rows),), dtype=MIRO_ROW_DTYPE)
    for i, r in enumerate(rows):
        if r is None:
            continue
        if len(r) != 3:
            raise ValueError(f"miro row {i}: expected (cell_ptr, tau, eta), got {r!r}")
        cell, tau, eta = r
        check_mirostat(tau, eta, 2, f"miro row {i}")
        if int(cell) < 0 or int(cell) % 8:
            raise ValueError(f"miro row {i}: the cell must be an 8-byte aligned device address, got {cell!r}")
        arr[i] = (int(cell), float(tau or 0.0), float(eta) if tau else 0.0)
    return arr


def pack_miro_rows(rows: Sequence[Optional[tuple]], device):
    """Device form of vt_miro_row for ops.sample_rows(..., miro=): a uint8 tensor [len(rows), 16]. rows: one entry per row, None (no
    Mirostat) or (cell, tau, eta) with `cell` a contiguous fp32 device tensor of two elements (new_miro_cell). The array holds addresses
    only: the caller keeps the cells alive."""
    import torch
    out = []
    for i, r in enumerate(rows):
        if r is None:
            out.append(None)
            continue
        cell, tau, eta = r
        if not isinstance(cell, torch.Tensor) or cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != 2 \
                or cell.device != torch.device(device):
            raise ValueError(f"miro row {i}: a cell is a contiguous fp32 tensor of two elements on the launch's device (new_miro_cell)")
        out.append((cell.data_ptr(), tau, eta))
    return _upload_rows(miro_rows_array(out), device)


# ---- history-dependent bans: struct vt_ban_row and the host statement of vt_ban_rows' contract --------------------------------------
def flatten_ban_seqs(seqs: Optional[Iterable[Sequence[int]]]) -> np.ndarray:
    """int32 array {L, id_0 .. id_{L-1}} repeated: the `seqs` buffer of vt_ban_row. Every sequence must be non-empty and its ids int32."""
    flat = []
    for w in seqs or ():
        w = [int(t) for t in w]
        if not w:
            raise ValueError("flatten_ban_seqs: an empty sequence")
        flat.append(len(w))
        flat.extend(w)
    if any(not -2 ** 31 <= t < 2 ** 31 for t in flat):
        raise ValueError("flatten_ban_seqs: an id outside int32")
    return np.asarray(flat, dtype=np.int32)


def history_bans(V: int, history: Sequence[int], ngram: int = 0, seqs: Optional[Iterable[Sequence[int]]] = None) -> list:
    """The ids of [0, V) that vt_ban_rows clears for a row whose history is `history` (include/vitron_hip.h), sorted:
    n-gram rule (g = ngram >= 1, n >= g - 1): for every i in [0, n - g + 1) with h[i .. i + g - 2] == h[n - g + 1 .. n - 1], the id
    h[i + g - 1]; sequence rule: s[0] for a sequence of one id, s[L - 1] when L >= 2, n >= L - 1 and h[n - L + 1 .. n - 1] == s[0 .. L - 2].
    Plain integer equality (sentinels take part); an id outside [0, V) is not banned."""
    h = [int(t) for t in history]
    n, g = len(h), int(ngram)
    banned = set()
    if g >= 1 and n >= g - 1:
        tail = h[n - g + 1:]
        for i in range(n - g + 1):
            if h[i:i + g - 1] == tail:
                banned.add(h[i + g - 1])
    for s in seqs or ():
        s = [int(t) for t in s]
        L = len(s)
        if L == 1 or (L >= 2 and n >= L - 1 and h[n - L + 1:] == s[:L - 1]):
            banned.add(s[L - 1])
    return sorted(t for t in banned if 0 <= t < int(V))


def ban_rows_array(rows: Sequence[tuple]) -> np.ndarray:
    """Host array of vt_ban_row from one tuple per row:
        (history_ptr, history_len, base_ptr, out_ptr, ngram, seqs_ptr, n_seqs, seqs_len)
    The pointers are DEVICE addresses (tensor.data_ptr(), 0 for NULL) whose owners the caller keeps alive until the launch has run."""
    arr = np.zeros((len(rows),), dtype=BAN_ROW_DTYPE)
    for i, (hist_ptr, hist_len, base_ptr, out_ptr, ngram, seqs_ptr, n_seqs, seqs_len) in enumerate(rows):
        if min(int(hist_ptr), int(base_ptr), int(out_ptr), int(seqs_ptr)) < 0 or (int(hist_len) > 0 and not hist_ptr) \
                or (int(n_seqs) > 0 and int(seqs_len) > 0 and not seqs_ptr):
            raise ValueError(f"ban row {i}: a negative address, or a length without its buffer")
        arr[i] = (int(hist_ptr), int(base_ptr), int(out_ptr), int(seqs_ptr), int(hist_len), int(ngram), int(n_seqs), int(seqs_len))
    return arr


def pack_ban_rows(rows: Sequence[tuple], device):
    """Device form of `ban_rows_array(rows)`: a uint8 tensor [len(rows), 48] for ops.ban_rows."""
    return _upload_rows(ban_rows_array(rows), device)


# ---- token automata: struct vt_fsm_row (the host statement of the contract is vitron_amd.automaton.TokenAutomaton) ---------------------
def fsm_rows_array(rows: Sequence[tuple]) -> np.ndarray:
    """Host array of vt_fsm_row from one tuple per row:
        (gen_ptr, gen_len, cell_ptr, base_ptr, out_ptr, offsets_ptr, edge_tok_ptr, edge_next_ptr, state_info_ptr, n_states, n_edges, eos)
    eos: at most 4 EOS ids. The pointers are DEVICE addresses (tensor.data_ptr(), 0 for NULL) whose owners the caller keeps alive until
    the launch has run; (offsets_ptr .. n_edges) is TokenAutomaton.row_fields(device)."""
    arr = np.zeros((len(rows),), dtype=FSM_ROW_DTYPE)
    for i, (gen_ptr, gen_len, cell_ptr, base_ptr, out_ptr, off_ptr, tok_ptr, nxt_ptr, info_ptr, n_states, n_edges, eos) in enumerate(rows):
        eos = [int(e) for e in eos]
        ptrs = [int(x) for x in (gen_ptr, cell_ptr, base_ptr, out_ptr, off_ptr, tok_ptr, nxt_ptr, info_ptr)]
        if min(ptrs) < 0 or (int(gen_len) > 0 and not gen_ptr) or (int(n_states) > 0 and not (off_ptr and info_ptr)) \
                or (int(n_edges) > 0 and not (tok_ptr and nxt_ptr)):
            raise ValueError(f"fsm row {i}: a negative address, or a length without its buffer")
        if len(eos) > FSM_MAX_EOS or any(not -2 ** 31 <= e < 2 ** 31 for e in eos):
            raise ValueError(f"fsm row {i}: at most {FSM_MAX_EOS} EOS ids, each an int32, got {eos!r}")
        arr[i] = (ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7], int(gen_len), int(n_states), int(n_edges),
                  len(eos), eos + [0] * (FSM_MAX_EOS - len(eos)))
    return arr


def pack_fsm_rows(rows: Sequence[tuple], device):
    """Device form of `fsm_rows_array(rows)`: a uint8 tensor [len(rows), 96] for ops.fsm_rows."""
    return _upload_rows(fsm_rows_array(rows), device)


# ---- classifier-free guidance: struct vt_cfg_row (the host statement of the contract is tests/cfg_ref.py) -----------------------------
def log_beta(beta: float) -> float:
    """The `log_beta` field of vt_cfg_row for a plausibility beta in [0, 1]: log(beta), -inf (no cut) for beta == 0."""
    return math.log(beta) if beta > 0 else -math.inf


def cfg_rows_array(rows: Sequence[tuple]) -> np.ndarray:
    """Host array of vt_cfg_row from one tuple per row:
        (cond_ptr, uncond_ptr, out_ptr, base_ptr, mask_out_ptr, lse_out_ptr, scale, log_beta)
    cond_ptr == 0 makes the row one the kernel skips. The pointers are DEVICE addresses (tensor.data_ptr(), 0 for NULL) whose owners the
    caller keeps alive until the launch has run; out_ptr may equal cond_ptr (in place) and must not equal uncond_ptr."""
    arr = np.zeros((len(rows),), dtype=CFG_ROW_DTYPE)
    for i, (cond, uncond, out, base, mask_out, lse_out, scale, lb) in enumerate(rows):
        ptrs = [int(x) for x in (cond, uncond, out, base, mask_out, lse_out)]
        if min(ptrs) < 0 or (ptrs[0] and not (ptrs[1] and ptrs[2])):
            raise ValueError(f"cfg row {i}: a negative address, or a conditional row without its uncond and out")
        if ptrs[0] and ptrs[2] == ptrs[1]:
            raise ValueError(f"cfg row {i}: out must not alias uncond")
        if ptrs[0] and ptrs[4] and ptrs[4] == ptrs[3]:
            raise ValueError(f"cfg row {i}: mask_out must not alias base")
        arr[i] = (*ptrs, float(scale), float(lb))
    return arr


def pack_cfg_rows(rows: Sequence[tuple], device):
    """Device form of `cfg_rows_array(rows)`: a uint8 tensor [len(rows), 56] for ops.cfg_rows."""
    return _upload_rows(cfg_rows_array(rows), device)


# ---- DoLa: struct vt_dola_row (the host statement of the contract is tests/dola_ref.py) ------------------------------------------------
def dola_candidate_layers(dola_layers, num_hidden_layers: int, tie_word_embeddings: bool = False) -> Tuple[int, ...]:
    """The candidate (premature) layers of generate(dola_layers=...), transformers 4.4x' rule: index i is hidden_states[i], the INPUT
    stream of decoder layer i (0 = the embeddings). "low" / "high" are every second layer of the lower / upper half (N <= 40), or of the
    first / last 20 layers (N > 40), starting at 2 when the embeddings are tied (layer 0 is then the lm_head's own transpose). A list:
    distinct ints in [0, N), kept in the given order. At most DOLA_MAX_LAYERS candidates; anything else, or an empty result, is a
    ValueError."""
    N = int(num_hidden_layers)
    start = 2 if tie_word_embeddings else 0
    if isinstance(dola_layers, str):
        if dola_layers not in ("low", "high"):
            raise ValueError(f"dola_layers must be 'low', 'high' or a list of layer indices, got {dola_layers!r}")
        if N <= 40:
            cand = range(start, N // 2, 2) if dola_layers == "low" else range(N // 2, N, 2)
        else:
            cand = range(start, 20, 2) if dola_layers == "low" else range(N - 20, N, 2)
        cand = tuple(cand)
    elif isinstance(dola_layers, (list, tuple)):
        for t in dola_layers:
            if not isinstance(t, numbers.Integral) or isinstance(t, bool) or not 0 <= t < N:
                raise ValueError(f"dola_layers: every entry must be an int in [0, {N}), got {t!r}")
        cand = tuple(int(t) for t in dola_layers)
        if len(set(cand)) != len(cand):
            raise ValueError(f"dola_layers: a layer is named twice in {list(cand)!r}")
    else:
        raise ValueError(f"dola_layers must be 'low', 'high' or a list of layer indices, got {dola_layers!r}")
    if not cand:
        raise ValueError(f"dola_layers={dola_layers!r} names no layer of a {N}-layer model")
    if len(cand) > DOLA_MAX_LAYERS:
        raise ValueError(f"dola_layers={dola_layers!r} names {len(cand)} layers, more than {DOLA_MAX_LAYERS}")
    return cand


def check_dola(dola_layers, relative_top, num_hidden_layers: int, tie_word_embeddings: bool = False, what: str = "generate"):
    """(candidate layers, relative_top) of a DoLa request, or (None, relative_top) when dola_layers is None (off). relative_top is a
    finite number in (0, 1] (transformers fixes it at 0.1)."""
    if not isinstance(relative_top, numbers.Real) or isinstance(relative_top, bool) or not 0 < relative_top <= 1:
        raise ValueError(f"{what}: dola_relative_top must be a number in (0, 1], got {relative_top!r}")
    if dola_layers is None:
        return None, float(relative_top)
    try:
        return dola_candidate_layers(dola_layers, num_hidden_layers, tie_word_embeddings), float(relative_top)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None


def dola_rows_array(rows: Sequence[tuple]) -> np.ndarray:
    """Host array of vt_dola_row from one tuple per row:
        (final_ptr, prem_ptr, prem_stride, n_cand, out_ptr, base_ptr, mask_out_ptr, layer_out_ptr, div_out_ptr, lse_out_ptr, log_relative_top)
    final_ptr == 0 makes the row one the kernel skips. The pointers are DEVICE addresses (tensor.data_ptr(), 0 for NULL) whose owners the
    caller keeps alive until the launch has run; out_ptr may equal final_ptr (in place)."""
    arr = np.zeros((len(rows),), dtype=DOLA_ROW_DTYPE)
    for i, (final, prem, stride, n_cand, out, base, mask_out, layer_out, div_out, lse_out, lrt) in enumerate(rows):
        ptrs = [int(x) for x in (final, prem, out, base, mask_out, layer_out, div_out, lse_out)]
        if min(ptrs) < 0 or (ptrs[0] and not (ptrs[1] and ptrs[2])):
            raise ValueError(f"dola row {i}: a negative address, or a final row without its candidates and out")
        if ptrs[0] and ptrs[4] and ptrs[4] == ptrs[3]:
            raise ValueError(f"dola row {i}: mask_out must not alias base")
        arr[i] = (*ptrs, int(stride), int(n_cand), float(lrt))
    return arr


def pack_dola_rows(rows: Sequence[tuple], device):
    """Device form of `dola_rows_array(rows)`: a uint8 tensor [len(rows), 80] for ops.dola_rows."""
    return _upload_rows(dola_rows_array(rows), device)


# ---- additive adjustments: struct vt_bias_row and the host statement of vt_bias_rows' contract --------------------------------------
def _finite(x) -> bool:
    return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x)


def normalise_bias(bias, V: Optional[int], what: str, tuple_keys: bool) -> Tuple[Tuple[int, float], ...]:
    """((id, value), ...) sorted by id from a mapping. tuple_keys: transformers' sequence_bias form, keys are tuples of ids (a bare int
    is a one-token key) and a key of more than one token is a NotImplementedError; otherwise keys are ids (logit_bias). ValueError: a key
    that is no id, an id outside [0, V) (when V is given), a value that is not a finite number, the same id twice."""
    if bias is None:
        return ()
    if not hasattr(bias, "items"):
        raise ValueError(f"{what} must be a mapping, got {bias!r}")
    out = {}
    for key, value in bias.items():
        if tuple_keys and isinstance(key, (tuple, list)):
            if len(key) == 0:
                raise ValueError(f"{what}: an empty key")
            if len(key) > 1:
                raise NotImplementedError(f"{what}: the multi-token key {tuple(key)!r} is not implemented (single-token keys only: its "
                                          "bias depends on the history)")
            key = key[0]
        if not isinstance(key, numbers.Integral) or isinstance(key, bool):
            raise ValueError(f"{what}: the key {key!r} is not a token id")
        t = int(key)
        if t < 0 or (V is not None and t >= int(V)):
            raise ValueError(f"{what}: the id {t} is outside [0, {'vocab_size' if V is None else int(V)})")
        if not _finite(value):
            raise ValueError(f"{what}: the bias of id {t} must be a finite number, got {value!r}")
        if t in out:
            raise ValueError(f"{what}: the id {t} is given twice")
        out[t] = float(value)
    return tuple(sorted(out.items()))


def check_penalties(presence, frequency, what: str) -> None:
    if not _finite(presence):
        raise ValueError(f"{what}: presence_penalty must be a finite number, got {presence!r}")
    if not _finite(frequency):
        raise ValueError(f"{what}: frequency_penalty must be a finite number, got {frequency!r}")


@dataclass(frozen=True)
class LogitAdjust:
    """What ONE request adds to its logits (ServingEngine.submit(..., adjust=)): logit_bias maps a token id to a finite float added
    BEFORE the repetition penalty (OpenAI's / vLLM's logit_bias, transformers' single-token sequence_bias); presence_penalty and
    frequency_penalty take presence + frequency * count off every token the request has GENERATED so far, AFTER the repetition penalty
    (any finite float; OpenAI's [-2, 2] is not enforced). `bias` is the normalised form: ((id, value), ...) sorted by id."""
    logit_bias: Optional[Dict[int, float]] = None
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0

    def __post_init__(self):
        object.__setattr__(self, "bias", normalise_bias(self.logit_bias, None, "LogitAdjust: logit_bias", tuple_keys=False))
        check_penalties(self.presence_penalty, self.frequency_penalty, "LogitAdjust")

    def __hash__(self):
        return hash((self.bias, float(self.presence_penalty), float(self.frequency_penalty)))

    @property
    def penalties(self) -> bool:
        """Does the adjustment depend on what the request has generated (a rebuild before every pick)?"""
        return float(self.presence_penalty) != 0.0 or float(self.frequency_penalty) != 0.0

    @property
    def active(self) -> bool:
        return bool(self.bias) or self.penalties

    def check_vocab(self, V: int) -> None:
        for t, _ in self.bias:
            if t >= int(V):
                raise ValueError(f"LogitAdjust: logit_bias: the id {t} is outside [0, {int(V)})")


def logit_adjust(V: int, generated: Sequence[int], bias=None, presence: float = 0.0, frequency: float = 0.0):
    """(pre, post), fp32 [V] each: what vt_bias_rows writes for a row that has generated `generated`, with the logit bias `bias` (a mapping
    id -> value or pairs (id, value), distinct ids) and the two penalties (include/vitron_hip.h):
    pre[t] = the bias of t, else 0; post[t] = 0 where t was not generated, else -(frequency * count(t) + presence) with the product and
    the sum rounded to fp32 separately. Ids outside [0, V) are skipped; only the last 65535 generated ids are counted."""
    V = int(V)
    pre = np.zeros((V,), dtype=np.float32)
    for t, v in (bias.items() if hasattr(bias, "items") else (bias or ())):
        if 0 <= int(t) < V:
            pre[int(t)] = np.float32(v)
    g = np.asarray(list(generated), dtype=np.int64).reshape(-1)[-65535:]
    g = g[(g >= 0) & (g < V)]
    c = np.bincount(g, minlength=V).astype(np.float32)
    prod = (np.float32(frequency) * c).astype(np.float32)
    post = np.where(c > 0, -(prod + np.float32(presence)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return pre, post


def bias_rows_array(rows: Sequence[tuple]) -> np.ndarray:
    """Host array of vt_bias_row from one tuple per row:
        (history_ptr, history_len, bias_ids_ptr, bias_vals_ptr, n_bias, out_ptr, presence, frequency)
    The pointers are DEVICE addresses (tensor.data_ptr(), 0 for NULL) whose owners the caller keeps alive until the launch has run."""
    arr = np.zeros((len(rows),), dtype=BIAS_ROW_DTYPE)
    for i, (hist_ptr, hist_len, ids_ptr, vals_ptr, n_bias, out_ptr, presence, frequency) in enumerate(rows):
        if min(int(hist_ptr), int(ids_ptr), int(vals_ptr), int(out_ptr)) < 0 or (int(hist_len) > 0 and not hist_ptr) \
                or (int(n_bias) > 0 and not (ids_ptr and vals_ptr)):
            raise ValueError(f"bias row {i}: a negative address, or a length without its buffer")
        arr[i] = (int(hist_ptr), int(ids_ptr), int(vals_ptr), int(out_ptr), int(hist_len), int(n_bias), float(presence), float(frequency))
    return arr


def pack_bias_rows(rows: Sequence[tuple], device):
    """Device form of `bias_rows_array(rows)`: a uint8 tensor [len(rows), 48] for ops.bias_rows."""
    return _upload_rows(bias_rows_array(rows), device)
