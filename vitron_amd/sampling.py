"""Per-request sampling parameters and their device form (struct vt_sample_row of include/vitron_hip.h).

`SamplingParams` is what a caller hands to `ServingEngine.submit(..., sampling=)`; `pack_sample_rows` turns one tuple per logits row
into the array `ops.sample_rows` / `vt_sample_rows` reads: one numpy structured array, one small host -> device copy.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Optional, Sequence

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
class SamplingParams:
    """How ONE request picks its tokens. temperature 0 is greedy; top_k None means config.top_k (default 50, as in `generate`);
    `seed` with the number of tokens generated so far is the whole state of the request's random stream, so its draws do not depend on
    what else is in the batch. logprobs=True collects the chosen token's log-probability per step (ServingEngine.logprobs)."""
    temperature: float = 0.0
    top_p: float = 1.0
    top_k: Optional[int] = None
    seed: int = 0
    repetition_penalty: float = 1.0
    logprobs: bool = False

    def __post_init__(self):
        self.validate()

    def validate(self) -> None:
        check_sampling_values(self.temperature, self.top_p, self.top_k, self.repetition_penalty, "SamplingParams")
        if not isinstance(self.seed, numbers.Integral) or isinstance(self.seed, bool):
            raise ValueError(f"SamplingParams: seed must be an int, got {self.seed!r}")
        if not isinstance(self.logprobs, bool):
            raise ValueError(f"SamplingParams: logprobs must be a bool, got {self.logprobs!r}")

    def resolved_top_k(self, config=None) -> int:
        if self.top_k is not None:
            return int(self.top_k)
        return int(getattr(config, "top_k", 50) or 0)


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
    import torch
    arr = sample_rows_array(rows)
    return torch.from_numpy(arr.view(np.uint8).reshape(len(rows), ROW_BYTES)).to(device)
