"""Host restatement of vt_sample_rows_wm's watermark (include/vitron_hip.h) for tests/test_synthid_ref_host.py,
tests/test_gpu_sample_wm.py and tests/test_gpu_wm_requests.py: transformers' SynthIDTextWatermarkLogitsProcessor with the hashes in
numpy uint64 (the bits of its wrapping int64), the tournament in fp64, and the sequence's cell as the header lays it out.

The keys are computed the way transformers states them -- ((H + v) * M + 1 + k_i) * M + 1 -- not the way the kernel does (a per-token
part plus a per-layer part, low 32 bits only), so the two meet only in the g-values. The tournament is ill-conditioned in log space
(fp32 rounds sum(g p) to exactly 1 once the mass sits on g = 1 tokens, which zeroes tokens whose fp64 probability is 1e-17 and less)
but not in probability: everything here is compared as probabilities and cumulative mass, never as logarithms, and nothing requires a
token to stay non-zero. Plain numpy (and torch.randint for the table, as transformers draws it); nothing here calls the library."""
import numpy as np

M = np.uint64(6364136223846793005)
ONE = np.uint64(1)
HEADER = 12                      # cell words in front of the history ring
WATERMARKED, REPEATED, SKIPPED = 1, 2, 4
KEYS30 = (654, 400, 836, 123, 340, 443, 597, 160, 57, 29, 590, 639, 13, 715, 468, 990, 966, 226, 324, 585, 118, 504, 421, 521, 129, 669,
          732, 225, 90, 960)     # the 30 keys of transformers' documentation example


def u64(x):
    return np.asarray(x).astype(np.int64).astype(np.uint64)


def accumulate(h, data):
    """h <- (h + d) * M + 1 over the last axis of data, wrapping"""
    h = np.asarray(h, dtype=np.uint64)
    data = u64(data)
    with np.errstate(over="ignore"):
        for i in range(data.shape[-1]):
            h = (h + data[..., i]) * M + ONE
    return h


def make_table(size, seed):
    import torch
    return torch.randint(0, 2, (int(size),), generator=torch.Generator("cpu").manual_seed(int(seed))).numpy().astype(np.uint8)


class Config:
    def __init__(self, ngram_len, keys, table_size=65536, table_seed=0, history_size=1024, skip_first=False):
        self.ngram_len, self.keys, self.history_size, self.skip_first = int(ngram_len), tuple(int(k) for k in keys), int(history_size), bool(skip_first)
        self.table_size, self.table_seed = int(table_size), int(table_seed)
        self.table = make_table(table_size, table_seed)
        self.depth = len(self.keys)

    def as_dict(self):
        return dict(ngram_len=self.ngram_len, keys=list(self.keys), sampling_table_size=self.table_size, sampling_table_seed=self.table_seed,
                    context_history_size=self.history_size, skip_first_ngram_calls=self.skip_first)

    def context_hash(self, context):
        return accumulate(np.ones(np.shape(context)[:-1], dtype=np.uint64), context)

    def g_next(self, H, V):
        """uint8 [V, depth]: g of every continuation behind a context with hash H, by transformers' statement"""
        with np.errstate(over="ignore"):
            h = (np.uint64(H) + np.arange(V, dtype=np.uint64)) * M + ONE
            keys = (h[:, None] + u64(self.keys)[None, :]) * M + ONE
        return self.table[(keys % np.uint64(self.table_size)).astype(np.int64)]


def tournament(q, g):
    """fp64: q *= 1 + g_i - sum(g_i q), layer by layer. q [V] sums to 1, g [V, depth] of 0 / 1."""
    q = np.array(q, dtype=np.float64, copy=True)
    for i in range(g.shape[1]):
        gi = g[:, i].astype(np.float64)
        q = q * (1.0 + gi - float((gi * q).sum()))
    return q


class Cell:
    """One sequence's state, word for word the device cell: [0] num_calls, [1] ring head, [2] the last call's context hash, [3] its
    flags, [4..11) the context ids (ngram_len - 1 used), [12..) the history ring. A fresh one is all zero."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.w = np.zeros((HEADER + cfg.history_size,), dtype=np.uint64)

    def words(self):
        return self.w.copy()

    def begin(self):
        """The part of a call in front of the draw: returns (H, flags)"""
        c, w = self.cfg, self.w
        w[0] += ONE
        H = c.context_hash(w[4:4 + c.ngram_len - 1].astype(np.int64))
        w[2] = H
        if c.skip_first and int(w[0]) < c.ngram_len:
            w[3] = SKIPPED
            return H, SKIPPED
        ring = w[HEADER:]
        rep = bool((ring == H).any())              # ALL entries, the zero ones of a fresh ring included
        head = int(w[1]) % c.history_size
        ring[head] = H
        w[1] = (head + 1) % c.history_size
        w[3] = REPEATED if rep else WATERMARKED
        return H, int(w[3])

    def finish(self, token):
        """The part behind the draw: an id >= 0 is shifted into the context"""
        n1 = self.cfg.ngram_len - 1
        if token >= 0:
            self.w[4:4 + n1 - 1] = self.w[5:4 + n1]
            self.w[4 + n1 - 1] = np.uint64(token)

    def call(self, p):
        """One call on the kept probabilities p (fp64 [V], 0 outside the keep-set, any positive mass): the distribution the draw is
        made over (sums to 1) and the flags. finish(token) must follow."""
        p = np.asarray(p, dtype=np.float64)
        q = p / p.sum()
        H, flags = self.begin()
        if flags == WATERMARKED:
            q = tournament(q, self.cfg.g_next(H, len(q)))
        return q, flags


def pick(q, u01):
    """(id, seam distance, (excl, incl)): the inverse-CDF walk over q in index order for the uniform u01 of (0, 1); the distance of
    u01 * mass from the nearest edge of the chosen token's interval, as a share of the mass; and that interval."""
    c = np.cumsum(q)
    u = float(u01) * c[-1]
    i = int(np.searchsorted(c, u, side="right"))
    if i >= len(c) or not q[i] > 0:
        i = int(np.flatnonzero(q > 0)[-1])
    lo = c[i] - q[i]
    return i, float(min(u - lo, c[i] - u) / c[-1]), (float(lo / c[-1]), float(c[i] / c[-1]))
