"""Host restatement of vt_sample_rows_trunc's truncation stages (include/vitron_hip.h) for tests/test_trunc_ref_host.py,
tests/test_gpu_sample_trunc.py and tests/test_gpu_trunc_requests.py: transformers' MinPLogitsWarper, TypicalLogitsWarper,
EpsilonLogitsWarper and EtaLogitsWarper stated in fp64 on the survivors of top-k and top-p, the inverse-CDF walk over the final set, and
`place()`.

A comparison at a threshold cannot be pinned across fp32 and fp64, so a test never uses a parameter as drawn: `place()` moves it, stage by
stage, to the middle of the nearest gap of the stage's statistic and asserts the margin in fp64 before anything runs:
  min_p, epsilon, eta  the geometric mean of two adjacent distinct values of q / q_max (min_p) or q (epsilon, eta) that are at least a
                       factor 1 + 4e-3 apart; for eta the threshold is solved back to eta_cutoff;
  typical              the midpoint of two adjacent prefix sums in d order; the gap token's q is at least 8e-3 of the mass and its d at
                       least 1e-3 nats from both neighbours.
Every margin is >= 1e-3 (relative for a probability, absolute nats for d); the kernel's fp32 statistics (one fast exponential and one
fast logarithm per token, tree sums of <= 32768 terms) err below about 1e-5. A row that cannot be placed (place() returns None) is
replaced by the next drawn row; no case is ever skipped. The top-p step in front gets the same treatment (`top_p_margin`).
Plain numpy on the CPU; nothing here calls the library."""
import numpy as np

from tests import sample_ref as S

F32 = np.float32
GAP = 1.0 + 4e-3          # least ratio of the two values a probability threshold is placed between
MARGIN = 1e-3             # what place() asserts for every comparison
TYP_Q = 8e-3              # least q of the typical stage's gap token, as a share of the placed mass
OFF = (0.0, 1.0, 0.0, 0.0)
STAGES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def on(trunc):
    """Which of the four stages the kernel runs: min_p > 0, the others inside (0, 1); NaN is off."""
    mp, ty, ep, et = (float(x) for x in trunc)
    return (mp > 0, 0 < ty < 1, 0 < ep < 1, 0 < et < 1)


# ---- the row the stages see ---------------------------------------------------------------------------------------------------------------
def scaled(row, temperature, allow=None, penalty=1.0, history=()):
    """fp64 scores after the allow mask (-inf), the repetition penalty (fp32, sample_ref) and the temperature"""
    x = np.array(row, dtype=F32, copy=True)
    if allow is not None:
        x[~np.asarray(allow, dtype=bool)] = -np.inf
    if penalty != 1.0:
        x = S.repetition_penalty(x, history, penalty)
    return x.astype(np.float64) / float(temperature)


def base_keep(s, top_k, top_p):
    """The survivors of TopK and TopP (sample_ref's rules) on scaled scores"""
    kk = S.top_k_keep(s, int(top_k)) & (s > -np.inf)
    return S.top_p_keep(np.where(kk, s, -np.inf), float(top_p)) & kk


def top_p_margin(s, top_k, top_p):
    """Distance of 1 - top_p from the nearest cumulative mass of the ascending sort, i.e. how far the top-p step is from keeping one
    token more or less (inf when top_p >= 1)."""
    if top_p >= 1.0:
        return np.inf
    kk = S.top_k_keep(s, int(top_k)) & (s > -np.inf)
    v = np.sort(s[kk])
    e = np.exp(v - v[-1])
    cum = np.cumsum(e / e.sum())
    return float(np.abs(cum - (1.0 - top_p)).min())


def softmax(s, A):
    """q over the survivors A (0 elsewhere), fp64"""
    e = np.where(A, np.exp(np.where(A, s, 0.0) - s[A].max()), 0.0)
    return e / e.sum()


def entropy(q, A):
    return float(-(q[A] * np.log(q[A])).sum())


# ---- the four stages ------------------------------------------------------------------------------------------------------------------------
def min_p_stage(s, A, min_p):
    q = softmax(s, A)
    return A & ((q >= min_p * q[A].max()) | (q == q[A].max()))


def typical_groups(s, A):
    """(d per token (inf outside A), the distinct d values ascending, their cumulative masses)"""
    q = softmax(s, A)
    d = np.full(s.shape, np.inf)
    d[A] = np.abs(-np.log(q[A]) - entropy(q, A))
    uniq, inv = np.unique(d[A], return_inverse=True)
    return d, uniq, np.cumsum(np.bincount(inv, weights=q[A]))


def typical_stage(s, A, mass):
    d, uniq, cum = typical_groups(s, A)
    k = int(np.searchsorted(cum, mass, side="left"))          # the first d whose tokens reach the mass
    return A.copy() if k >= len(uniq) else A & (d <= uniq[k])


def epsilon_stage(s, A, eps):
    q = softmax(s, A)
    return A & ((q >= eps) | (q == q[A].max()))


def eta_threshold(s, A, eta_cutoff):
    return min(eta_cutoff, np.sqrt(eta_cutoff) * np.exp(-entropy(softmax(s, A), A)))


def eta_stage(s, A, eta_cutoff):
    q = softmax(s, A)
    return A & ((q >= eta_threshold(s, A, eta_cutoff)) | (q == q[A].max()))


def apply(s, A, trunc):
    """The final survivors: the active stages of `trunc` = (min_p, typical_p, epsilon_cutoff, eta_cutoff) in transformers' order, each on
    the softmax renormalised over what is left."""
    A = np.array(A, dtype=bool, copy=True)
    act = on(trunc)
    for stage, active, value in zip((min_p_stage, typical_stage, epsilon_stage, eta_stage), act, trunc):
        if active:
            A = stage(s, A, float(value))
    return A


# ---- placement ------------------------------------------------------------------------------------------------------------------------------
def _gap(values, x):
    """The geometric mean of the two adjacent distinct `values` nearest to x, as fp32, or None when they are closer than GAP"""
    v = np.unique(values)
    if v.size < 2:
        return None
    k = min(max(int(np.searchsorted(v, x)), 1), v.size - 1)
    lo, hi = v[k - 1], v[k]
    if not (lo > 0 and hi / lo >= GAP):
        return None
    t = float(F32(np.sqrt(lo * hi)))
    assert min(t / lo, hi / t) - 1.0 >= MARGIN
    return t


def place(s, A, trunc):
    """`trunc` with every active parameter moved to the middle of the nearest gap of its stage's statistic (module docstring), the
    stages applied one after the other in fp64. Returns (placed trunc as four Python floats that are exact fp32 values, the final
    survivors), or None when a stage has no gap wide enough."""
    A = np.array(A, dtype=bool, copy=True)
    out = list(float(x) for x in trunc)
    act = on(trunc)
    if act[0]:
        q = softmax(s, A)
        t = _gap(q[A] / q[A].max(), out[0])
        if t is None or not 0 < t <= 1:
            return None
        out[0] = t
        A = min_p_stage(s, A, t)
    if act[1]:
        d, uniq, cum = typical_groups(s, A)
        if uniq.size < 3:
            return None
        k = min(max(int(np.searchsorted(cum, out[1], side="left")), 1), uniq.size - 2)     # the gap token has a neighbour on both sides
        m = float(F32(0.5 * (cum[k - 1] + cum[k])))
        if not 0 < m < 1 or cum[k] - cum[k - 1] < TYP_Q * m or min(uniq[k] - uniq[k - 1], uniq[k + 1] - uniq[k]) < MARGIN:
            return None
        assert min(m - cum[k - 1], cum[k] - m) / m >= MARGIN
        out[1] = m
        A = typical_stage(s, A, m)
    if act[2]:
        t = _gap(softmax(s, A)[A], out[2])
        if t is None or not 0 < t < 1:
            return None
        out[2] = t
        A = epsilon_stage(s, A, t)
    if act[3]:
        q = softmax(s, A)
        t = _gap(q[A], eta_threshold(s, A, out[3]))
        if t is None:
            return None
        k = np.exp(-entropy(q, A))                       # eta = min(e, sqrt(e) k): e for e <= k^2, else sqrt(e) k
        e = float(F32(t if t <= k * k else (t / k) ** 2))
        if not 0 < e < 1:
            return None
        v = np.unique(q[A])
        eta = eta_threshold(s, A, e)
        below, above = v[v < eta], v[v >= eta]
        if below.size == 0 or above.size == 0 or min(eta / below.max(), above.min() / eta) - 1.0 < MARGIN:
            return None
        out[3] = e
        A = eta_stage(s, A, e)
    return tuple(out), A


# ---- the draw -------------------------------------------------------------------------------------------------------------------------------
def pick(s, A, u01):
    """(id, seam distance): the inverse-CDF walk over the survivors in index order for the uniform u01 of (0, 1), and how far
    u01 * (kept mass) lies from the nearest edge of the chosen token's interval, as a share of the kept mass."""
    p = np.where(A, np.exp(np.where(A, s, 0.0) - s[A].max()), 0.0)
    c = np.cumsum(p)
    u = float(u01) * c[-1]
    i = int(np.searchsorted(c, u, side="right"))
    i = i if i < len(c) and A[i] else int(np.flatnonzero(A)[-1])
    lo = c[i] - p[i]
    return i, float(min(u - lo, c[i] - u) / c[-1])


# ---- the constructed row ------------------------------------------------------------------------------------------------------------------
ARGMAX_REMOVED_TOP_K = 61


def argmax_removed_case(V):
    """(scores as fp64 of fp32 values, the survivors of top_k = 61, trunc): token 7 holds about 0.4 of the mass, 60 tokens about 0.01
    each (their logits 0.006 apart, so their d are too), the rest lies 30 below and outside the top-k set. The entropy is near 3.1, so
    the big token's d (2.2) is larger than every small token's (< 1.7): typical sampling with a mass near 0.5 keeps small tokens only
    and REMOVES the arg-max. epsilon_cutoff = 0.5 then exceeds every q (< 0.05): all leave but the maximum of the CURRENT survivors.
    The typical mass is placed; epsilon is a factor 10 from every q."""
    x = np.full((V,), np.log(0.01) - 30.0, dtype=F32)
    small = 100 + 3 * np.arange(60)
    x[small] = (np.log(0.01) + 0.006 * (np.arange(60) - 30)).astype(F32)
    x[7] = F32(np.log(0.4))
    s = x.astype(np.float64)
    A0 = base_keep(s, ARGMAX_REMOVED_TOP_K, 1.0)
    assert A0.sum() == 61
    (_, m, _, _), _ = place(s, A0, (0.0, 0.5, 0.0, 0.0))
    return s, A0, (0.0, m, 0.5, 0.0)


# ---- drawn cases ----------------------------------------------------------------------------------------------------------------------------
SIGMAS = (0.5, 1.5, 3.0, 6.0)
TEMPS = (0.7, 1.0, 1.3)
TOP_KS = (0, 50, 200)
TOP_PS = (1.0, 0.95)
COMBOS = ((0,), (1,), (2,), (3,), (0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2, 3), (0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3),
          (0, 1, 2, 3))


def draw_row(g, V):
    """One drawn row: fp32 N(0, sigma) logits, a temperature, top_k and top_p; the spread of the logits stays under 80 after the
    temperature, so that no kept token's exponential underflows."""
    sigma = SIGMAS[int(g.integers(len(SIGMAS)))]
    x = (g.standard_normal(V) * sigma).astype(F32)
    T = TEMPS[int(g.integers(len(TEMPS)))]
    return x, T, TOP_KS[int(g.integers(len(TOP_KS)))], TOP_PS[int(g.integers(len(TOP_PS)))]


def draw_trunc(g, combo):
    """Drawn parameters for the stages of `combo` (indices into STAGES), the rest off"""
    drawn = (float(g.uniform(0.02, 0.3)), float(g.uniform(0.2, 0.95)), float(10.0 ** g.uniform(-5.0, -2.0)), float(10.0 ** g.uniform(-5.0, -2.0)))
    return tuple(drawn[i] if i in combo else OFF[i] for i in range(4))


def placed_cases(V, combos=COMBOS, seed=0, allow_every=0, penalty_every=0, history=()):
    """len(combos) placed cases at vocabulary V, in order: dicts with the fp32 `row`, T, top_k, top_p, `allow` (bool [V] or None), penalty,
    the placed `trunc`, the fp64 scores `s`, the survivors of top-k / top-p `A0` and the final ones `A`. Rows are drawn from one
    generator; a row that cannot be placed -- or whose top-p step sits within 1e-4 of another keep-set -- is replaced by the next drawn
    row, so the list always has its full length. allow_every / penalty_every = n > 0: every n-th case carries a random allow mask of
    60 % of the ids / the repetition penalty 1.3 over `history`."""
    g = np.random.default_rng(seed * 1000003 + V)
    cases = []
    for n, combo in enumerate(combos):
        for attempt in range(200):
            row, T, k, p = draw_row(g, V)
            allow = (g.random(V) < 0.6) if (allow_every and n % allow_every == allow_every - 1) else None
            pen = 1.3 if (penalty_every and n % penalty_every == penalty_every - 1) else 1.0
            s = scaled(row, T, allow, pen, history)
            A0 = base_keep(s, k, p)
            ok = top_p_margin(s, k, p) >= 1e-4 and np.ptp(s[np.isfinite(s)]) < 80.0
            got = place(s, A0, draw_trunc(g, combo)) if ok else None
            if got is not None:
                cases.append(dict(row=row, T=T, top_k=k, top_p=p, allow=allow, penalty=pen, trunc=got[0], s=s, A0=A0, A=got[1], combo=combo))
                break
        else:
            raise AssertionError(f"no placeable row for stages {combo} at V = {V} in 200 draws")
    return cases
