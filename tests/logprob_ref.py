"""Host restatement of vt_logprob_rows (vitron_amd/csrc/vt_logprob.hip, include/vitron_hip.h) for
tests/test_logprob_ref_host.py, tests/test_gpu_logprob_rows.py and tests/test_gpu_logprob_requests.py: the ORDER (larger raw logit first,
exact ties to the lower index, NaNs removed first) by a stable sort on (-x, index), the rank, the (-1, NaN) padding, the fp64 log_softmax
and the bound an fp32 implementation of  x_t - (m + logf(sum expf(x - m)))  must meet. The bound is tests/sample_ref.py's, restated with
the chain length of THIS kernel's sum. Plain numpy / torch on the CPU; nothing here calls the library."""
import numpy as np
import torch

from tests.sample_ref import E_EXP, E_LOG, F32, U

MAX_TOP = 20


# ---- order, top lists, rank --------------------------------------------------------------------------------------------------------------
def order(row) -> np.ndarray:
    """The ids of one row in the kernel's order: NaNs removed, then a stable sort on -x (so equal values keep ascending index)."""
    x = np.asarray(row, dtype=F32)
    ids = np.flatnonzero(~np.isnan(x))
    return ids[np.argsort(-x[ids].astype(np.float64), kind="stable")]


def log_softmax64(raw) -> np.ndarray:
    """fp64 log_softmax of fp32 row(s). A row that holds a NaN is NaN everywhere; -inf entries are -inf."""
    with np.errstate(all="ignore"):
        return torch.log_softmax(torch.as_tensor(np.asarray(raw, dtype=F32)).double(), -1).numpy()


def lse64(raw) -> np.ndarray:
    with np.errstate(all="ignore"):
        return torch.logsumexp(torch.as_tensor(np.atleast_2d(np.asarray(raw, dtype=F32))).double(), -1).numpy()


def top(raw, n_top: int):
    """(top_ids int32 [rows, n_top], top_lp fp64 [rows, n_top]): the first n_top ids of every row's order and their fp64
    log-probabilities; slots past the takeable values hold (-1, NaN)."""
    raw = np.atleast_2d(np.asarray(raw, dtype=F32))
    ls = log_softmax64(raw)
    ids = np.full((raw.shape[0], n_top), -1, dtype=np.int32)
    lp = np.full((raw.shape[0], n_top), np.nan, dtype=np.float64)
    for r in range(raw.shape[0]):
        o = order(raw[r])[:n_top]
        ids[r, :o.size] = o
        lp[r, :o.size] = ls[r, o]
    return ids, lp


def rank(raw, targets) -> np.ndarray:
    """int32 [rows]: 1 + the number of tokens strictly ahead of the target in the order; 0 for a target outside [0, V). A NaN never
    counts as ahead; a target whose own logit is NaN stands behind every value that is not a NaN."""
    raw = np.atleast_2d(np.asarray(raw, dtype=F32))
    V = raw.shape[1]
    out = np.zeros((raw.shape[0],), dtype=np.int32)
    idx = np.arange(V)
    for r, t in enumerate(np.asarray(targets, dtype=np.int64).reshape(-1)):
        if not 0 <= t < V:
            continue
        x, xt = raw[r], raw[r, t]
        with np.errstate(invalid="ignore"):
            ahead = (~np.isnan(x)) if np.isnan(xt) else ((x > xt) | ((x == xt) & (idx < t)))
        out[r] = 1 + int(ahead.sum())
    return out


def target_lp(raw, targets) -> np.ndarray:
    """fp64 [rows]: log_softmax at the target, NaN for a target outside [0, V)."""
    raw = np.atleast_2d(np.asarray(raw, dtype=F32))
    ls = log_softmax64(raw)
    out = np.full((raw.shape[0],), np.nan)
    for r, t in enumerate(np.asarray(targets, dtype=np.int64).reshape(-1)):
        if 0 <= t < raw.shape[1]:
            out[r] = ls[r, t]
    return out


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------
def register_form(V: int, ldl: int, base_offset_bytes: int = 0) -> bool:
    """The launcher's choice: V <= 32 * 1024, a 16-byte aligned base and a row stride that is a multiple of 4 floats."""
    return V <= 32 * 1024 and ldl % 4 == 0 and base_offset_bytes % 16 == 0


def lse_chain(V: int, reg: bool) -> int:
    """Longest chain of fp32 additions behind vt_logprob_rows' sum of the exponentials, read off logprob_rows_kernel: a thread adds its
    own terms serially -- 32 in the register form (the slots past V add an exact 0); in the streaming form 4 per 16-byte load,
    ceil((V / 4) / 1024) loads, plus at most one term of the ragged tail, or ceil(V / 1024) single terms without 16-byte loads: at most
    4 * ceil(V / 4096) + 1 either way -- then 6 shuffle levels add the wave and 16 serial additions the wave totals."""
    own = 32 if reg else 4 * (-(-V // 4096)) + 1
    return own + 6 + 16


def lse_bound(raw, chain: int) -> np.ndarray:
    """|kernel lse - fp64 logsumexp(raw)| per row: tests/sample_ref.logprob_bound's terms without the final subtraction --
    U A + E_EXP for the exponentials' arguments and values (A = sum e_i |d_i| / z), `chain` U for the additions, 1 % for second-order
    products, log(z (1 + r)) - log z <= r (1 + r), E_LOG |log z| for logf, U |lse| for m + logf(z), 1e-30 for underflowing terms."""
    raw = np.atleast_2d(np.asarray(raw, dtype=F32)).astype(np.float64)
    m = raw.max(-1, keepdims=True)
    d = raw - m
    e = np.exp(d)
    z = e.sum(-1)
    with np.errstate(invalid="ignore"):
        A = np.where(e > 0, e * np.abs(d), 0.0).sum(-1) / z          # (a -inf logit: e = 0 exactly, it adds nothing)
    rel_z = 1.01 * (U * A + E_EXP + chain * U)
    lse = m[:, 0] + np.log(z)
    return rel_z * (1.0 + rel_z) + E_LOG * np.abs(np.log(z)) + U * np.abs(lse) + 1e-30


def logprob_bound(raw, lp64, chain: int) -> np.ndarray:
    """|kernel (x_t - lse) - fp64 log_softmax(raw)[t]| for log-probabilities lp64 ([rows] or [rows, n]): lse_bound plus the rounding of
    the subtraction, U |lp|. Entries where lp64 is not finite get bound 0: -inf and NaN are compared exactly, not by distance."""
    lp64 = np.asarray(lp64, dtype=np.float64)
    b = lse_bound(raw, chain)
    b = b.reshape((-1,) + (1,) * (lp64.ndim - 1))
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(lp64), b + U * np.abs(lp64), 0.0)


def worst_ratio(got, want64, bound) -> float:
    """max |got - want| / bound over the finite entries of want64, after asserting that the others match exactly (NaN with NaN, -inf
    with -inf). 0.0 when nothing is finite."""
    got = np.asarray(got, dtype=np.float64)
    want64 = np.asarray(want64, dtype=np.float64)
    fin = np.isfinite(want64)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), "NaN pattern differs"
    assert np.array_equal(got[~fin & ~np.isnan(want64)], want64[~fin & ~np.isnan(want64)]), "infinite entries differ"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want64[fin]) / np.broadcast_to(bound, want64.shape)[fin]).max())
