"""Host restatement of the per-row sampler (vt_sample_rows, vitron_amd/csrc/vt_sample.hip) for
tests/test_sample_ref_host.py, tests/test_gpu_sample_rows.py and tests/test_gpu_sampling_requests.py: the repetition penalty in fp32
(bit for bit what the kernel computes), the warpers' keep-sets in transformers' order (4.31: RepetitionPenaltyLogitsProcessor, then
TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper), the counter-based uniform (splitmix64 of seed, counter, stream), the
inverse-CDF walk over the kept tokens in index order, and the fp64 log-probability with the bound an fp32 implementation must meet.
The keep-sets and the walk are stated in fp64: they are the RULE (the kernel's fp32 roundings are pinned by exact equality with
vt_sample_top_p / vt_argmax instead). Plain numpy / torch on the CPU; nothing here calls the library."""
import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of fp32 (half an ulp, relative)
_M64 = (1 << 64) - 1


# ---- the uniform ---------------------------------------------------------------------------------------------------------------------------
def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def uniform24(seed: int, counter: int, stream: int) -> np.float32:
    """The kernel's uniform in (0, 1): the top 24 bits of splitmix64(seed ^ splitmix64(counter * 0x632be59bd9b4e019 + stream)), centred
    (+ 0.5), as fp32. vt_sample_top_p draws the same number from (seed, step, row index)."""
    r = splitmix64((seed & _M64) ^ splitmix64((counter * 0x632BE59BD9B4E019 + stream) & _M64))
    return F32(float(r >> 40) + 0.5) * F32(1.0 / 16777216.0)


# ---- RepetitionPenaltyLogitsProcessor ----------------------------------------------------------------------------------------------------
def repetition_penalty(logits, history, penalty) -> np.ndarray:
    """fp32 row(s) [..., V] with every DISTINCT id of `history` in [0, V) penalised: x < 0 ? x * p : x / p, the product and the correctly
    rounded quotient in fp32 (numpy's and torch's fp32 arithmetic; the kernel's __fdiv_rn). Ids outside [0, V) are skipped."""
    out = np.array(logits, dtype=F32, copy=True)
    V = out.shape[-1]
    ids = np.unique(np.asarray(history, dtype=np.int64).reshape(-1))
    ids = ids[(ids >= 0) & (ids < V)]
    if ids.size:
        x = out[..., ids]
        p = F32(penalty)
        with np.errstate(all="ignore"):
            out[..., ids] = np.where(x < 0, x * p, x / p).astype(F32)
    return out


# ---- the warpers' keep-sets --------------------------------------------------------------------------------------------------------------
def top_k_keep(scores, k: int) -> np.ndarray:
    """TopKLogitsWarper: scores < (k-th largest score) leave; ties with the k-th value stay. k <= 0 or k >= V: everything stays."""
    s = np.asarray(scores, dtype=np.float64)
    if k <= 0 or k >= s.shape[-1]:
        return np.ones(s.shape, dtype=bool)
    kth = np.sort(s, axis=-1)[..., -k][..., None]
    return s >= kth


def top_p_keep(scores, top_p: float) -> np.ndarray:
    """TopPLogitsWarper (min_tokens_to_keep = 1): sort ascending, drop while the cumulative softmax mass is <= 1 - top_p, always keep
    the last (largest). `scores` may hold -inf (what TopK removed). top_p >= 1 keeps every finite score. fp64. Among scores that TIE at
    the boundary the stable sort drops the lower indices first."""
    s = np.asarray(scores, dtype=np.float64)
    if top_p >= 1.0:
        return s > -np.inf
    order = np.argsort(s, axis=-1, kind="stable")
    ss = np.take_along_axis(s, order, -1)
    e = np.exp(ss - ss[..., -1:])
    cum = np.cumsum(e / e.sum(-1, keepdims=True), axis=-1)
    remove = cum <= (1.0 - top_p)
    remove[..., -1] = False
    keep = np.zeros(s.shape, dtype=bool)
    np.put_along_axis(keep, order, ~remove, -1)
    return keep


def keep_set(row, temperature, top_k, top_p, penalty=1.0, history=()) -> np.ndarray:
    """The tokens a sampled row can return: penalty (fp32), / temperature, top-k, top-p over what top-k left -- transformers' order."""
    x = repetition_penalty(row, history, penalty).astype(np.float64) / float(temperature)
    kk = top_k_keep(x, int(top_k))
    return top_p_keep(np.where(kk, x, -np.inf), float(top_p)) & kk


def sample_row(row, temperature, top_k, top_p, penalty, history, seed, counter, stream):
    """(id, keep mask) of one row under the whole rule. temperature 0: the first index of the maximum of the penalised row (keep mask:
    that one token). Otherwise the inverse-CDF walk: u * (kept mass) against the running sum of the kept probabilities in INDEX order,
    the first token whose running sum exceeds it."""
    pen = repetition_penalty(row, history, penalty)
    if not temperature > 0:
        i = int(np.argmax(pen))                      # numpy: first index of the maximum
        keep = np.zeros(pen.shape, dtype=bool)
        keep[i] = True
        return i, keep
    keep = keep_set(row, temperature, top_k, top_p, penalty, history)
    x = pen.astype(np.float64) / float(temperature)
    p = np.where(keep, np.exp(x - x[keep].max()), 0.0)
    c = np.cumsum(p)
    u = float(uniform24(seed, counter, stream)) * c[-1]
    i = int(np.searchsorted(c, u, side="right"))
    kept_ids = np.flatnonzero(keep)
    return (i if i < len(c) and keep[i] else int(kept_ids[-1])), keep


# ---- the chosen token's log-probability ----------------------------------------------------------------------------------------------------
# expf / logf of the device math library: the HIP documentation states 1 ulp for each; taken as 2 ulp (= 4 U relative) here.
E_EXP = 4.0 * U
E_LOG = 4.0 * U


def logprob_ref(raw) -> np.ndarray:
    """fp64 log_softmax of fp32 row(s)"""
    return torch.log_softmax(torch.as_tensor(np.asarray(raw, dtype=F32)).double(), -1).numpy()


def lse_chain(V: int) -> int:
    """Longest chain of fp32 additions behind the sum of the exponentials: a thread adds its own terms serially (32 in the register form,
    ceil(V / 1024) in the streaming form), 6 shuffle levels add the wave, 16 serial additions the wave totals."""
    return max(32, -(-V // 1024)) + 6 + 16


def logprob_bound(raw, ids) -> np.ndarray:
    """|kernel logprob - fp64 log_softmax(raw)[id]| per row, for  lp = raw[id] - (m + logf(sum_i expf(raw_i - m))),  m = max(raw) (exact):
    * d_i = raw_i - m rounds once: expf's argument is off by U |d_i|, its value by that relatively; expf itself adds E_EXP. Weighted by
      the term's share e_i / z of the sum that is  U A + E_EXP  with  A = sum_i e_i |d_i| / z  (computed here in fp64 from the data);
    * any order of lse_chain(V) additions of positive terms: (chain) U relative to z; 1 % on top covers every second-order product;
    * log(z (1 + r)) - log z <= r (1 + r); logf adds E_LOG |log z|;
    * m + logf(z) rounds once: U |lse|; raw[id] - lse rounds once: U |lp|;
    * an exponential that underflows is off by at most 2^-126 absolutely: V 2^-126 / z < 1e-30, added as a constant.
    Derived from the operation counts alone; DESIGN.md 9.3 records how much of it the kernel uses."""
    raw = np.atleast_2d(np.asarray(raw, dtype=F32)).astype(np.float64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    V = raw.shape[-1]
    m = raw.max(-1, keepdims=True)
    d = raw - m
    e = np.exp(d)
    z = e.sum(-1)
    A = (e * np.abs(d)).sum(-1) / z
    rel_z = 1.01 * (U * A + E_EXP + lse_chain(V) * U)
    lse = m[:, 0] + np.log(z)
    lp = raw[np.arange(raw.shape[0]), ids] - lse
    return rel_z * (1.0 + rel_z) + E_LOG * np.abs(np.log(z)) + U * np.abs(lse) + U * np.abs(lp) + 1e-30


def logprob_f32_emulation(raw, idx, order=None) -> np.float32:
    """fp32 emulation of the kernel's logprob arithmetic on one row (serial sum in `order`, numpy's expf / logf): what the bound must
    admit whatever the order."""
    raw = np.asarray(raw, dtype=F32)
    m = raw.max()
    e = np.exp((raw - m).astype(F32)).astype(F32)
    z = F32(0)
    for v in (e if order is None else e[order]):
        z = F32(z + v)
    return F32(raw[idx] - F32(m + np.log(z).astype(F32)))
