"""Host restatement of vt_sample_rows_miro's Mirostat v2 stage (include/vitron_hip.h; Basu et al., "Mirostat: A Neural
Text Decoding Algorithm that Directly Controls Perplexity", ICLR 2021; llama.cpp's mirostat_v2) for tests/test_miro_ref_host.py,
tests/test_gpu_sample_miro.py and tests/test_gpu_miro_requests.py.

The rule, in fp64, on the scores `s` and the survivors `A` that tests/trunc_ref.py states for vt_sample_rows_trunc (after penalty,
adjustment, allow mask, temperature, top-k, top-p and the four truncation stages):
  1. q_v = p_v / kept over A, s_v = -log2(q_v).
  2. v survives iff s_v <= mu; the most probable kept token always survives (the first index on a tie) -- alone when its own surprise
     exceeds mu.
  3. kept2 = the sum of the surviving q_v; the draw is the inverse CDF over the survivors in index order for the uniform u01 * kept2.
  4. e = -log2(q_x / kept2) for the drawn id x; mu <- mu - eta * (e - tau); the cell becomes {mu, e}.
  5. kept_count = the number of survivors of step 2.
`step` is that statement without a sort. `llama_step` is a second, independent one written literally after llama.cpp's
llama_sampler_mirostat_v2 (softmax, sort by probability, truncate at the first candidate whose surprise exceeds mu keeping at least
one, softmax again, sample by the CDF, update mu): the two must agree (tests/test_miro_ref_host.py). llama.cpp walks its CDF in
sorted order with a random number of its own; the sampler here walks in index order with the row's uniform, so `llama_step` takes the
index-order walk over its truncated candidates -- the one place where it follows this project rather than llama.cpp.

The bounds an fp32 implementation must meet (`surprise_bound`, `mu_bound`) are derived below from the kernel's arithmetic, the way
sample_ref.logprob_bound is. Plain numpy on the CPU; nothing here calls the library."""
import numpy as np

from tests import trunc_ref as T

F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of fp32
LN2 = float(np.log(2.0))


def fresh_cell(tau):
    """{mu, last_surprise} of a sequence that has not picked yet: what the host writes once"""
    return np.array([2.0 * float(tau), 0.0], dtype=F32)


# ---- the five steps -------------------------------------------------------------------------------------------------------------------------
def surprises(s, A):
    """(q over A as fp64 (0 elsewhere), s_v = -log2 q_v (inf elsewhere))"""
    q = T.softmax(np.asarray(s, dtype=np.float64), np.asarray(A, dtype=bool))
    sv = np.full(q.shape, np.inf)
    sv[A] = -np.log2(q[A])
    return q, sv


def keep(s, A, mu):
    """The survivors of step 2 (bool [V]). A NaN mu keeps the arg-max alone."""
    q, sv = surprises(s, A)
    K = np.asarray(A, dtype=bool) & (sv <= mu)
    first = int(np.flatnonzero(q == q.max())[0])
    if not K[first]:               # the maximum's own surprise exceeds mu: nothing else can survive
        K = np.zeros(q.shape, dtype=bool)
    K[first] = True
    return K


def draw(q, K, u01):
    """The inverse-CDF walk over the survivors K in index order for the uniform u01 of (0, 1): (id, distance of u01 * kept2 from the
    nearest edge of the chosen interval, as a share of kept2)"""
    p = np.where(K, q, 0.0)
    c = np.cumsum(p)
    u = float(u01) * c[-1]
    i = int(np.searchsorted(c, u, side="right"))
    i = i if i < len(c) and K[i] else int(np.flatnonzero(K)[-1])
    return i, float(min(u - (c[i] - p[i]), c[i] - u) / c[-1])


def observed(q, K, x):
    """e = -log2(q_x / kept2): the surprise of x under the distribution it was drawn from"""
    return float(-np.log2(q[x] / q[K].sum()))


def step(s, A, mu, tau, eta, u01=None, x=None):
    """One pick: dict(K, count, id, seam, e, mu). tau and eta are taken as the fp32 values the kernel reads. Give u01 (the id is
    drawn) or x (the id is given: a replay with the kernel's ids)."""
    q, _ = surprises(s, A)
    K = keep(s, A, mu)
    seam = np.inf
    if x is None:
        x, seam = draw(q, K, u01)
    e = observed(q, K | (np.arange(q.size) == x), x)
    return dict(K=K, count=int(K.sum()), id=int(x), seam=seam, e=e, mu=float(mu) - float(F32(eta)) * (e - float(F32(tau))))


# ---- llama.cpp's mirostat_v2, literally -----------------------------------------------------------------------------------------------------
def llama_step(s, A, mu, tau, eta, u01):
    """llama_sampler_mirostat_v2_apply over the candidates A with logits s: softmax; sort by probability, descending (stable: the lower
    index first among equals); find the first candidate whose surprise -log2(p) exceeds mu, truncate there, keep at least one; softmax
    over what is left; sample by the CDF; observed surprise of the sampled candidate; mu -= eta * (observed - tau).
    Returns dict(K, count, id, e, mu)."""
    s = np.asarray(s, dtype=np.float64)
    ids = np.flatnonzero(np.asarray(A, dtype=bool))
    logit = s[ids]
    p = np.exp(logit - logit.max())
    p = p / p.sum()                                              # llama_sampler_softmax_impl
    order = np.argsort(-p, kind="stable")
    ids, p, logit = ids[order], p[order], logit[order]
    size = len(ids)
    for i in range(len(ids)):                                    # std::find_if(... -log2f(candidate.p) > mu)
        if -np.log2(p[i]) > mu:
            size = i
            break
    size = max(size, 1)                                          # cur_p->size = std::max(..., 1). (A NaN mu compares false everywhere:
    #                                                              llama.cpp keeps all, the kernel one; no test of agreement uses a NaN)
    ids, p = ids[:size], p[:size]
    p2 = p / p.sum()                                             # the softmax over the truncated candidates (same logits, same ratios)
    by_index = np.argsort(ids, kind="stable")                    # this project's walk: index order, the row's own uniform
    c = np.cumsum(p2[by_index])
    j = int(np.searchsorted(c, float(u01) * c[-1], side="right"))
    j = min(j, size - 1)
    x = int(ids[by_index][j])
    e = float(-np.log2(p2[by_index][j]))
    K = np.zeros(s.shape, dtype=bool)
    K[ids] = True
    return dict(K=K, count=size, id=x, e=e, mu=float(mu) - float(F32(eta)) * (e - float(F32(tau))))


def trajectory(fn, s, A, tau, eta, uniforms, mu0=None):
    """n picks on ONE row (the chat loop's logits change, the rule does not): [(K.sum(), id, e, mu after)]"""
    mu = 2.0 * float(F32(tau)) if mu0 is None else float(mu0)
    out = []
    for u in uniforms:
        r = fn(s, A, mu, tau, eta, u)
        mu = r["mu"]
        out.append((r["count"], r["id"], r["e"], mu))
    return out


# ---- what fp32 may cost ---------------------------------------------------------------------------------------------------------------------
# The kernel's q_v, factor by factor (U = 2^-24, M = the largest |scaled logit| among the kept tokens, so every x_v - max is within 2 M):
#   x_v = l_v * fl(1 / T)                      two roundings, against the reference's l_v / T:      |dx| <= 2 U |x_v|
#   x_v - max                                  both operands and the difference:                    <= (2 + 2 + 2) U M = 6 U M
#   __expf = v_exp_f32(d * log2 e)             the product moves the exponent by U |d| log2 e, i.e. the value by U |d| relative; 1 ulp of its own
#                                                                                                   <= 2 U M + 2 U
#   so p_v carries a relative error            E_p <= U (8 M + 2)
#   * inv_z, the keep test's kept p, * 1/kept  three more roundings each and the common factors 1/z, 1/kept with theirs   <= 5 U
#   kept = a tree sum of <= 32768 terms        32 serial + 6 + 16 serial additions: <= 54 U, on top of the terms' E_p
#   q_v = p_v / kept                           E_q <= 2 E_p + 59 U
#   s_v = -log2f(q_v)                          |ds| <= E_q / ln 2 + 2 ulp(s_v)  (ocml's log2f: 1 ulp; 2 is taken)
# e = -log2f(fdiv(q_x, kept2)): kept2 is one more such tree sum over the q (54 U + E_q), the divide one rounding.
SUM_CHAIN = 54


def q_rel_err(max_abs_scaled):
    return (2.0 * (8.0 * float(max_abs_scaled) + 2.0) + 5.0 + SUM_CHAIN) * U


def surprise_bound(max_abs_scaled, surprise, observed_e=False):
    """Upper bound of |fp32 - fp64| for a token's surprise s_v (observed_e=False) or for the observed surprise e of the drawn token
    (True), from the derivation above. max_abs_scaled: the largest |score| among the kept tokens after the temperature;
    surprise: the fp64 value (its ulp enters)."""
    eq = q_rel_err(max_abs_scaled)
    if observed_e:
        eq = 2.0 * eq + (SUM_CHAIN + 1) * U
    return eq / LN2 + 4.0 * U * abs(float(surprise)) + 2.0 ** -126


def mu_step_bound(eta, e_err, e, tau, mu):
    """One update mu - eta * (e - tau) in fp32 against fp64 with an e that is off by e_err: the difference, the product and the last
    difference round once each."""
    d = abs(float(e) - float(tau)) + e_err
    return float(eta) * (e_err + U * d) + U * float(eta) * d + U * (abs(float(mu)) + float(eta) * d)


def mu_bound(n, eta, e_err, e_span, mu_max):
    """After n steps whose observed surprises are each off by at most e_err, with |e - tau| <= e_span and |mu| <= mu_max throughout"""
    return n * mu_step_bound(eta, e_err, e_span, 0.0, mu_max)


# ---- placement ------------------------------------------------------------------------------------------------------------------------------
def place_mu(s, A, want_count, max_abs_scaled=None):
    """A mu at the midpoint of a gap of the fp64 surprises so that about want_count tokens survive, the gap wider than 4 surprise
    bounds -- asserted here, on the CPU, before anything is launched. Returns (mu as an exact fp32 value, the survivors)."""
    _, sv = surprises(s, A)
    v = np.unique(sv[np.asarray(A, dtype=bool)])
    M = float(np.abs(np.asarray(s)[np.asarray(A, dtype=bool)]).max()) if max_abs_scaled is None else float(max_abs_scaled)
    k0 = min(max(int(want_count), 1), v.size - 1)
    for k in list(range(k0, v.size)) + list(range(k0 - 1, 0, -1)):           # the nearest gap that is wide enough
        lo, hi = v[k - 1], v[k]
        mu = float(F32(0.5 * (lo + hi)))
        if min(mu - lo, hi - mu) > 2.0 * surprise_bound(M, hi):
            K = keep(s, A, mu)
            assert hi - lo > 4.0 * surprise_bound(M, hi) * 0.999 and K.sum() == (sv <= lo).sum()
            return mu, K
    raise AssertionError("no gap of the surprises is wider than four bounds")


def zipf_row(V, exponent=1.1):
    """Scores of a Zipf(exponent) distribution over V tokens in a fixed shuffled order: fp64 of fp32 values"""
    p = 1.0 / np.arange(1, V + 1, dtype=np.float64) ** exponent
    x = np.log(p / p.sum()).astype(F32)
    return x[np.random.default_rng(V).permutation(V)].astype(np.float64)
