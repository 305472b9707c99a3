"""SynthID text watermarking: transformers' SynthIDTextWatermarkingConfig / SynthIDTextWatermarkLogitsProcessor
(Dathathri et al., Nature 2024) for the per-row sampler. The processor runs last in GenerationMixin's chain, behind every warper, so
the tournament lives inside vt_sample_rows_wm, behind the truncation stages; this module is its host side:

  * `SynthIDWatermark`: one configuration -- the sampling table exactly as transformers draws it, packed to bits; the per-layer
    constants k_i * M + 1; both uploaded once per device; `new_cell` (an all-zero cell IS a fresh SynthIDTextWatermarkState);
  * `pack_wm_rows`: the device array of struct vt_wm_row that ops.sample_rows(..., watermark=) takes;
  * the detector's host side, equal to the processor's compute_* methods: `g_values`, `context_repetition_mask`, `eos_token_mask`,
    and `mean_g`, the mean g-value over the scored n-grams of a reply (about 0.5 for text that was not watermarked with these keys).

The green-list scheme (transformers' WatermarkingConfig) reseeds a torch.Generator and calls torch.randperm(vocab) for every token,
which cannot be restated on the device without a host round trip per step: it is refused by name. The trained Bayesian detector of
transformers is out of scope; `mean_g` is the paper's simplest score."""
from __future__ import annotations

import numbers
from typing import Optional, Sequence

import numpy as np

WM_MUL = 6364136223846793005            # accumulate_hash: h <- (h + d) * M + 1 in wrapping 64-bit arithmetic
_U64 = (1 << 64) - 1
WM_MAX_DEPTH, WM_MAX_TABLE, WM_MAX_NGRAM, WM_MAX_HISTORY = 32, 65536, 8, 4096          # VT_WM_MAX_* of include/vitron_hip.h
WM_MAX_V = 32 * 1024                    # the sampler's register form: the only one that carries the tournament
WM_CELL_HEADER = 12                     # words in front of the history ring: vt_wm_cell_words(h) = 12 + h
WM_FLAG_WATERMARKED, WM_FLAG_REPEATED, WM_FLAG_SKIPPED = 1, 2, 4

# struct vt_wm_row: the offsets are part of the ABI (tests/test_synthid_ref_host.py checks them against the header's table)
WM_ROW_DTYPE = np.dtype({"names": ["cell", "layer_add", "table", "depth", "table_size", "ngram_len", "history_size", "skip_first",
                                   "reserved"],
                         "formats": ["<u8", "<u8", "<u8", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4"],
                         "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44], "itemsize": 48})
WM_ROW_BYTES = WM_ROW_DTYPE.itemsize

_FIELDS = ("ngram_len", "keys", "sampling_table_size", "sampling_table_seed", "context_history_size", "skip_first_ngram_calls",
           "debug_mode")
_DEFAULTS = {"sampling_table_size": 65536, "sampling_table_seed": 0, "context_history_size": 1024, "skip_first_ngram_calls": False,
             "debug_mode": False}
_GREENLIST_FIELDS = ("greenlist_ratio", "seeding_scheme", "hashing_key")


def _is_int(x) -> bool:
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def accumulate_hash(h: np.ndarray, data: np.ndarray) -> np.ndarray:
    """transformers' accumulate_hash over the last axis of `data`, in uint64 (the same bits as its wrapping int64)."""
    h = np.asarray(h, dtype=np.uint64)
    data = np.asarray(data).astype(np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        for i in range(data.shape[-1]):
            h = (h + data[..., i]) * np.uint64(WM_MUL) + np.uint64(1)
    return h


class SynthIDWatermark:
    """One SynthID text watermark. `config`: a transformers SynthIDTextWatermarkingConfig (duck-typed by its fields), a dict of those
    fields, or another SynthIDWatermark. ValueError: keys empty or more than 32, a key outside int64, ngram_len outside [2, 8],
    context_history_size outside [1, 4096]. NotImplementedError, naming the field: a sampling_table_size that is not a power of two in
    [32, 65536], debug_mode, and the green-list WatermarkingConfig."""

    def __init__(self, config):
        if isinstance(config, SynthIDWatermark):
            config = config.to_dict()
        if isinstance(config, dict):
            get, has = config.get, config.__contains__
        else:
            get, has = (lambda k, d=None: getattr(config, k, d)), (lambda k: hasattr(config, k))
        if any(has(f) for f in _GREENLIST_FIELDS) and not has("keys"):
            raise NotImplementedError("watermarking_config: the green-list scheme (WatermarkingConfig: greenlist_ratio, seeding_scheme) "
                                      "is not implemented: it reseeds a torch.Generator and calls torch.randperm(vocab) for every "
                                      "token, which the device sampler cannot restate without a host round trip per step; use "
                                      "SynthIDTextWatermarkingConfig")
        if not has("keys") or not has("ngram_len"):
            raise ValueError("watermarking_config: expected a SynthIDTextWatermarkingConfig or a dict with at least ngram_len and keys")
        if isinstance(config, dict):
            unknown = sorted(set(config) - set(_FIELDS))
            if unknown:
                raise ValueError(f"watermarking_config: unknown field(s) {unknown}; the fields are {list(_FIELDS)}")
        vals = {f: get(f, _DEFAULTS.get(f)) for f in _FIELDS}
        vals = {f: (_DEFAULTS[f] if v is None and f in _DEFAULTS else v) for f, v in vals.items()}
        ngram_len, keys = vals["ngram_len"], vals["keys"]
        if not _is_int(ngram_len) or not 2 <= ngram_len <= WM_MAX_NGRAM:
            raise ValueError(f"watermarking_config: ngram_len must be an int in [2, {WM_MAX_NGRAM}], got {ngram_len!r}")
        keys = list(keys) if isinstance(keys, (list, tuple, np.ndarray)) else None
        if not keys or len(keys) > WM_MAX_DEPTH:
            raise ValueError(f"watermarking_config: keys must be a list of 1 to {WM_MAX_DEPTH} ints (one per tournament layer), got "
                             f"{vals['keys']!r}")
        for k in keys:
            if not _is_int(k) or not -(1 << 63) <= int(k) < (1 << 63):
                raise ValueError(f"watermarking_config: the key {k!r} is not an int64")
        hs = vals["context_history_size"]
        if not _is_int(hs) or not 1 <= hs <= WM_MAX_HISTORY:
            raise ValueError(f"watermarking_config: context_history_size must be an int in [1, {WM_MAX_HISTORY}], got {hs!r}")
        size = vals["sampling_table_size"]
        if not _is_int(size) or size <= 0:
            raise ValueError(f"watermarking_config: sampling_table_size must be a positive int, got {size!r}")
        if size < 32 or size > WM_MAX_TABLE or size & (size - 1):
            raise NotImplementedError(f"watermarking_config: sampling_table_size={size} is not implemented (a power of two in [32, "
                                      f"{WM_MAX_TABLE}]: the device reduces a key with a mask and keeps the table's bits in LDS)")
        seed = vals["sampling_table_seed"]
        if not _is_int(seed):
            raise ValueError(f"watermarking_config: sampling_table_seed must be an int, got {seed!r}")
        if vals["debug_mode"]:
            raise NotImplementedError("watermarking_config: debug_mode=True is not implemented (it replaces the scores by ones)")
        self.ngram_len = int(ngram_len)
        self.keys = tuple(int(k) for k in keys)
        self.sampling_table_size = int(size)
        self.sampling_table_seed = int(seed)
        self.context_history_size = int(hs)
        self.skip_first_ngram_calls = bool(vals["skip_first_ngram_calls"])
        self.debug_mode = False
        import torch
        table = torch.randint(0, 2, (self.sampling_table_size,), generator=torch.Generator("cpu").manual_seed(self.sampling_table_seed))
        self.table = table.numpy().astype(np.uint8)                                                 # [size] of 0 / 1, as transformers'
        self.table_bits = np.packbits(self.table, bitorder="little").view("<u4").astype(np.uint32)  # bit t of the array = table[t]
        self.layer_add = np.asarray([((k & _U64) * WM_MUL + 1) & _U64 for k in self.keys], dtype=np.uint64)
        self._dev = {}

    # ---- configuration --------------------------------------------------------------------------------------------------------
    @property
    def depth(self) -> int:
        return len(self.keys)

    @property
    def cell_words(self) -> int:
        return WM_CELL_HEADER + self.context_history_size

    def to_dict(self) -> dict:
        return {"ngram_len": self.ngram_len, "keys": list(self.keys), "sampling_table_size": self.sampling_table_size,
                "sampling_table_seed": self.sampling_table_seed, "context_history_size": self.context_history_size,
                "skip_first_ngram_calls": self.skip_first_ngram_calls, "debug_mode": False}

    def key(self) -> tuple:
        """A hashable identity: two configurations with the same key watermark alike."""
        return (self.ngram_len, self.keys, self.sampling_table_size, self.sampling_table_seed, self.context_history_size,
                self.skip_first_ngram_calls)

    def check_vocab(self, V: int, what: str = "watermarking_config") -> None:
        if int(V) > WM_MAX_V:
            raise NotImplementedError(f"{what}: vocab_size={int(V)} is beyond the sampler's register form ({WM_MAX_V}), the only one "
                                      "that carries the watermark's tournament")

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def device_tables(self, device):
        """(layer_add int64 [depth], table bits int32 [size / 32]) on `device`: uploaded once per device and kept here."""
        import torch
        dev = torch.device(device)
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.layer_add.view("<i8").copy()).to(dev),
                              torch.from_numpy(self.table_bits.view("<i4").copy()).to(dev))
        return self._dev[dev]

    def new_cell(self, device):
        """The all-zero state of one sequence: int64 [12 + context_history_size] on `device`."""
        import torch
        return torch.zeros((self.cell_words,), dtype=torch.int64, device=device)

    def row_fields(self, cell) -> tuple:
        """The vt_wm_row of a sequence whose state is `cell` (from `new_cell`, on the device the launch runs on)."""
        import torch
        if not isinstance(cell, torch.Tensor) or cell.dtype != torch.int64 or not cell.is_contiguous() or cell.numel() != self.cell_words:
            raise ValueError(f"watermark: a cell is a contiguous int64 tensor of {self.cell_words} words (SynthIDWatermark.new_cell)")
        add, table = self.device_tables(cell.device)
        return (cell.data_ptr(), add.data_ptr(), table.data_ptr(), self.depth, self.sampling_table_size, self.ngram_len,
                self.context_history_size, int(self.skip_first_ngram_calls), 0)

    # ---- the detector's host side -------------------------------------------------------------------------------------------------
    @staticmethod
    def _ids2d(ids) -> np.ndarray:
        a = np.asarray(ids.cpu().numpy() if hasattr(ids, "cpu") else ids, dtype=np.int64)
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2:
            raise ValueError(f"watermark: ids must be [len] or [batch, len], got shape {a.shape}")
        return a

    def context_hash(self, context) -> np.ndarray:
        """uint64 hash of contexts [..., ngram_len - 1], from 1."""
        context = np.asarray(context, dtype=np.int64)
        return accumulate_hash(np.ones(context.shape[:-1], dtype=np.uint64), context)

    def g_of_keys(self, ngram_keys: np.ndarray) -> np.ndarray:
        return self.table[(np.asarray(ngram_keys, dtype=np.uint64) & np.uint64(self.sampling_table_size - 1)).astype(np.int64)]

    def g_next(self, context_hash, V: int) -> np.ndarray:
        """g of every continuation v in [0, V) behind a context with hash `context_hash`: uint8 [V, depth]."""
        with np.errstate(over="ignore"):
            h = (np.uint64(context_hash) + np.arange(V, dtype=np.uint64)) * np.uint64(WM_MUL) + np.uint64(1)
            return self.g_of_keys(h[:, None] * np.uint64(WM_MUL) + self.layer_add[None, :])     # ((h + k) * M + 1 = h * M + (k * M + 1))

    def g_values(self, ids) -> np.ndarray:
        """compute_g_values: uint8 [batch, len - (ngram_len - 1), depth], entry t for the n-gram ids[t : t + ngram_len]."""
        a = self._ids2d(ids)
        n = self.ngram_len
        if a.shape[1] < n:
            return np.zeros((a.shape[0], 0, self.depth), dtype=np.uint8)
        grams = np.lib.stride_tricks.sliding_window_view(a, n, axis=1)                         # [B, L - n + 1, n]
        h = accumulate_hash(np.ones(grams.shape[:2], dtype=np.uint64), grams)
        with np.errstate(over="ignore"):
            return self.g_of_keys(h[..., None] * np.uint64(WM_MUL) + self.layer_add)

    def context_repetition_mask(self, ids) -> np.ndarray:
        """compute_context_repetition_mask: bool [batch, len - (ngram_len - 1)], True where the n-gram's context was NOT seen among the
        last context_history_size contexts (a zero-initialised history, as the processor's)."""
        a = self._ids2d(ids)
        n = self.ngram_len
        if a.shape[1] < n:
            return np.zeros((a.shape[0], 0), dtype=bool)
        ctx = np.lib.stride_tricks.sliding_window_view(a[:, :-1], n - 1, axis=1)               # [B, L - n + 1, n - 1]
        h = accumulate_hash(np.ones(ctx.shape[:2], dtype=np.uint64), ctx)
        out = np.zeros(h.shape, dtype=bool)
        for b in range(h.shape[0]):
            hist = np.zeros((self.context_history_size,), dtype=np.uint64)
            for t in range(h.shape[1]):
                out[b, t] = not (hist == h[b, t]).any()
                hist = np.concatenate(([h[b, t]], hist[:-1]))
        return out

    @staticmethod
    def eos_token_mask(ids, eos_token_id: int) -> np.ndarray:
        """compute_eos_token_mask: bool [batch, len], False from the first eos_token_id on."""
        a = SynthIDWatermark._ids2d(ids)
        return np.cumsum(a == int(eos_token_id), axis=1) == 0

    def mean_g(self, ids, generated_from: int = 0, eos_token_id: Optional[int] = None, return_count: bool = False):
        """The mean g-value over the scored n-grams of `ids` ([len] or [batch, len]): those lying wholly in ids[generated_from:], whose
        context is not a repetition (context_repetition_mask over the generated part) and, with eos_token_id, that hold no token at
        or behind the first EOS of the generated part. Unwatermarked text scores about 0.5 with a standard deviation of
        0.5 / sqrt(count); count = scored n-grams x depth (return_count=True returns (mean, count)). NaN when nothing is scored."""
        a = self._ids2d(ids)[:, int(generated_from):]
        g = self.g_values(a)
        keep = self.context_repetition_mask(a)
        if eos_token_id is not None:
            keep = keep & self.eos_token_mask(a, eos_token_id)[:, self.ngram_len - 1:]
        count = int(keep.sum()) * self.depth
        mean = float(g[keep].mean()) if count else float("nan")
        return (mean, count) if return_count else mean


def as_watermark(config) -> Optional[SynthIDWatermark]:
    """None stays None; a SynthIDWatermark is itself; anything else goes through SynthIDWatermark(config)."""
    if config is None or isinstance(config, SynthIDWatermark):
        return config
    return SynthIDWatermark(config)


def wm_rows_array(rows: Sequence[Optional[tuple]]) -> np.ndarray:
    """Host array of vt_wm_row from one entry per row: None (cell = NULL: the row is not watermarked) or the nine fields
    (cell_ptr, layer_add_ptr, table_ptr, depth, table_size, ngram_len, history_size, skip_first, reserved) -- SynthIDWatermark.row_fields."""
    arr = np.zeros((len(rows),), dtype=WM_ROW_DTYPE)
    for i, r in enumerate(rows):
        if r is None:
            continue
        if len(r) != 9:
            raise ValueError(f"wm row {i}: expected the nine fields of vt_wm_row, got {r!r}")
        arr[i] = tuple(int(x) for x in r)
    return arr


def pack_wm_rows(rows: Sequence[Optional[tuple]], device):
    """Device form of vt_wm_row for ops.sample_rows(..., watermark=): a uint8 tensor [len(rows), 48]. rows: one entry per row, None (not
    watermarked) or (SynthIDWatermark, cell). The array holds addresses only: the caller keeps the cells alive."""
    from .sampling import _upload_rows
    return _upload_rows(wm_rows_array([None if r is None else r[0].row_fields(r[1]) for r in rows]), device)
