"""Host restatement of vt_dola_rows (vitron_amd/csrc/vt_dola.hip, include/vitron_hip.h) and of the dola_layers rule for
tests/test_dola_ref_host.py, tests/test_gpu_dola_rows.py and tests/test_gpu_dola_requests.py. transformers 5.x no longer ships
_dola_decoding / _dola_select_contrast / _relative_top_filter, so this module is the statement (tests/test_dola_ref_host.py checks it
against a literal torch port of the two functions of transformers 4.4x).

Per row, f = the final layer's logit row, x_j = candidate j (an early layer's stream through the bare lm_head), lp = log_softmax:
    div_j = 0.5 * sum_v [ M (log M - lp_f) + M (log M - lp_j) ],  M = 0.5 (exp(lp_f) + exp(lp_j)),  a term with M == 0 counting 0
    j*    = 0; for j = 1 .. n - 1: if div_j > div_j*: j* = j              (the largest; exact ties and NaNs go to the lower j)
    keep  = f >= max(f) + log(relative_top)                               (in fp32, the maximum over the values that are not NaN)
    out   = keep ? lp_f - lp_j* : -inf
One candidate: j* = 0 and div = [0]. `row64` is that in fp64; `out32` is the fp32 restatement of `out` from GIVEN lse values and j in
numpy float32 operations, each rounded on its own -- the kernel's contract, bit for bit; `div32` restates the divergence the same way
(not bit for bit: expf / logf differ).

div_bound, derived (U = 2^-24, E_EXP = E_LOG = 4 U: tests/sample_ref.py's stated assumption of 2 ulp for the device's expf / logf):
  lp_f~ = f - lse_f~ is off by at most d_f = lse_bound(f) + U |lp_f| (tests/logprob_ref.logprob_bound), lp_j~ by d_j likewise;
  p~ = expf(lp~) has relative error r = 1.01 (d + E_EXP); M~ = 0.5 (p_f~ + p_j~) -- a sum of two non-negative numbers, the half exact --
  has r_M = max(r_f, r_j) + U; logf(M~) is off by at most l = r_M (1 + r_M) + E_LOG |log M|; a difference (log M - lp) by l + d + U |log M
  - lp|; a product M (log M - lp) by M [l + d + (r_M + U) |log M - lp|]; the sum of the two products adds U (|a| + |b|). Per term
      e_v = 1.01 M [ 2 l + d_f + d_j + (r_M + 3 U) (|log M - lp_f| + |log M - lp_j|) ]
  and the reduction -- this kernel's chain: a thread's own terms (32 in the register form, ceil(V / 1024) in the re-read form), 6
  shuffle levels, 16 wave totals -- adds chain U sum_v (|a_v| + |b_v|). The final 0.5 is exact. A denormal or underflowing M loses at
  most 2^-149 against factors below 2^8: V 2^-141 in all.
Plain numpy / torch on the CPU; nothing here calls the library."""
import numpy as np

from tests.cfg_ref import row_max, same_bits  # noqa: F401  (same_bits: used by the GPU tests through this module)
from tests.logprob_ref import log_softmax64, lse64, lse_bound  # noqa: F401
from tests.sample_ref import E_EXP, E_LOG, F32, U

MAX_LAYERS = 16


# ---- the layer rule ----------------------------------------------------------------------------------------------------------------------
def candidate_layers(dola_layers, N: int, tied: bool = False) -> list:
    """transformers 4.4x' rule, restated independently of vitron_amd.sampling.dola_candidate_layers."""
    start = 2 if tied else 0
    if dola_layers == "low":
        return list(range(start, N // 2, 2)) if N <= 40 else list(range(start, 20, 2))
    if dola_layers == "high":
        return list(range(N // 2, N, 2)) if N <= 40 else list(range(N - 20, N, 2))
    return [int(l) for l in dola_layers]


# ---- the row in fp64 -----------------------------------------------------------------------------------------------------------------------
def divergences64(final, prem) -> np.ndarray:
    """fp64 [n_cand]: div_j of every candidate row of prem [n_cand, V] against final [V]; [0.] for one candidate."""
    prem = np.atleast_2d(np.asarray(prem, dtype=F32))
    if prem.shape[0] == 1:
        return np.zeros((1,))
    lpf = log_softmax64(final)
    out = np.empty((prem.shape[0],))
    with np.errstate(all="ignore"):
        pf = np.exp(lpf)
        for j in range(prem.shape[0]):
            lpj = log_softmax64(prem[j])
            M = 0.5 * (pf + np.exp(lpj))
            lm = np.log(M)
            out[j] = 0.5 * np.where(M == 0, 0.0, M * (lm - lpf) + M * (lm - lpj)).sum()
    return out


def choose(div) -> int:
    """The largest divergence; exact ties and NaNs go to the lower j (a NaN never beats an earlier candidate, and nothing beats a NaN)."""
    jb = 0
    for j in range(1, len(div)):
        if div[j] > div[jb]:
            jb = j
    return jb


def log_rt(relative_top: float) -> np.float32:
    return F32(np.log(relative_top))


def keep(final, relative_top: float) -> np.ndarray:
    """bool [V]: f >= max(f) + log(relative_top), one fp32 addition and an fp32 comparison; a NaN fails."""
    f = np.asarray(final, dtype=F32)
    with np.errstate(all="ignore"):
        return f >= F32(row_max(f) + log_rt(relative_top))


def mask(final, relative_top: float, base=None) -> np.ndarray:
    """uint32 [ceil(V / 32)]: bit i = base bit i AND keep_i; bits at positions >= V are base's own there, or clear without a base."""
    k = keep(final, relative_top)
    V = k.size
    W = (V + 31) // 32
    ok = np.ones((W * 32,), dtype=bool)
    ok[:V] = k
    words = np.packbits(ok, bitorder="little").view("<u4").astype(np.uint32)
    if base is None:
        start = np.zeros((W * 32,), dtype=bool)
        start[:V] = True
        base = np.packbits(start, bitorder="little").view("<u4")
    return words & np.asarray(base, dtype=np.uint32)


def row64(final, prem, relative_top: float = 0.1, base=None) -> dict:
    """The whole row in fp64: {"div" [n_cand], "j", "out" fp64 [V], "keep" bool [V], "mask" uint32 [ceil(V / 32)]}."""
    final = np.asarray(final, dtype=F32)
    prem = np.atleast_2d(np.asarray(prem, dtype=F32))
    div = divergences64(final, prem)
    j = choose(div)
    k = keep(final, relative_top)
    with np.errstate(all="ignore"):
        out = np.where(k, log_softmax64(final) - log_softmax64(prem[j]), -np.inf)
    return {"div": div, "j": j, "out": out, "keep": k, "mask": mask(final, relative_top, base)}


# ---- fp32 restatements -------------------------------------------------------------------------------------------------------------------
def out32(final, prem_j, lse_f, lse_j, relative_top: float) -> np.ndarray:
    """fp32 `out` from the given lse values and the chosen candidate row: a = f - lse_f; b = x - lse_j; out = keep ? a - b : -inf, every
    operation a numpy float32 operation (round to nearest, nothing fused): the kernel's contract, bit for bit."""
    f, x = np.asarray(final, dtype=F32), np.asarray(prem_j, dtype=F32)
    with np.errstate(all="ignore"):
        a = (f - F32(lse_f)).astype(F32)
        b = (x - F32(lse_j)).astype(F32)
        r = (a - b).astype(F32)
        return np.where(keep(f, relative_top), r, F32(-np.inf)).astype(F32)


def lse32(row) -> np.float32:
    """m + log(sum exp(x - m)) in numpy float32 operations (pairwise summation: not the kernel's order, inside the same bound)."""
    x = np.asarray(row, dtype=F32)
    with np.errstate(all="ignore"):
        m = row_max(x)
        return F32(m + np.log(np.exp((x - m).astype(F32)).astype(F32).sum(dtype=F32)))


def div32(final, prem_j) -> np.float32:
    """div_j in numpy float32 operations, the kernel's expression term by term."""
    f, x = np.asarray(final, dtype=F32), np.asarray(prem_j, dtype=F32)
    with np.errstate(all="ignore"):
        lpf = (f - lse32(f)).astype(F32)
        lpj = (x - lse32(x)).astype(F32)
        M = (F32(0.5) * (np.exp(lpf).astype(F32) + np.exp(lpj).astype(F32)).astype(F32)).astype(F32)
        lm = np.log(M).astype(F32)
        t = ((M * (lm - lpf).astype(F32)).astype(F32) + (M * (lm - lpj).astype(F32)).astype(F32)).astype(F32)
        return F32(F32(0.5) * np.where(M == 0, F32(0), t).sum(dtype=F32))


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------------
def register_form(V: int, offsets_bytes=(0, 0, 0), prem_stride: int = 0) -> bool:
    """The kernel's choice per row: V <= 32 * 1024, final / prem / out 16-byte aligned and a candidate stride that is a multiple of 4."""
    return V <= 32 * 1024 and all(o % 16 == 0 for o in offsets_bytes) and prem_stride % 4 == 0


def chain(V: int, reg: bool) -> int:
    """Longest chain of fp32 additions behind one of vt_dola_rows' block sums (the lse sums and the divergence alike), read off
    dola_rows_kernel: a thread's own terms, 6 shuffle levels, the 16 wave totals."""
    return (32 if reg else -(-V // 1024)) + 6 + 16


def div_bound(final, prem_j, reg: bool = True) -> float:
    """|kernel div_j - fp64 div_j| for finite rows; the derivation is in the module docstring."""
    f, x = np.asarray(final, dtype=F32), np.asarray(prem_j, dtype=F32)
    V = f.size
    c = chain(V, reg)
    lpf, lpj = log_softmax64(f), log_softmax64(x)
    d_f = float(lse_bound(f, c)[0]) + U * np.abs(lpf)
    d_j = float(lse_bound(x, c)[0]) + U * np.abs(lpj)
    r_M = np.maximum(1.01 * (d_f + E_EXP), 1.01 * (d_j + E_EXP)) + U
    M = 0.5 * (np.exp(lpf) + np.exp(lpj))
    with np.errstate(all="ignore"):
        lm = np.where(M > 0, np.log(M), 0.0)
        da, db = np.where(M > 0, np.abs(lm - lpf), 0.0), np.where(M > 0, np.abs(lm - lpj), 0.0)
    ell = r_M * (1.0 + r_M) + E_LOG * np.abs(lm)
    e = 1.01 * M * (2.0 * ell + d_f + d_j + (r_M + 3.0 * U) * (da + db))
    return float(0.5 * (e.sum() + 1.01 * c * U * (M * (da + db)).sum()) + V * 2.0 ** -141)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def ladder_case(V: int, n_cand: int, seed: int, reg: bool = True, furthest_at=None):
    """(final fp32 [V], prem fp32 [n_cand, V], j): final = 4 N(0, 1), prem_j = (1 - w_j) final + w_j 4 N(0, 1) with the w_j a shuffled
    ladder 0.1 .. 1.0 (furthest_at: the position the row with the largest divergence is moved to). j is the fp64 choice. Asserts
    what makes the choice testable exactly: the fp64 gap between the best and the second divergence is at least 4 x the larger
    div_bound of the two. A case that fails it is an error of this builder, never a skip."""
    g = np.random.default_rng([seed, V, n_cand])
    final = (4.0 * g.standard_normal(V)).astype(F32)
    w = np.linspace(0.1, 1.0, n_cand) if n_cand > 1 else np.array([1.0])
    g.shuffle(w)
    prem = np.stack([((1.0 - wj) * final + wj * 4.0 * g.standard_normal(V)).astype(F32) for wj in w])
    div = divergences64(final, prem)
    j = choose(div)
    if furthest_at is not None and furthest_at != j:     # a row's divergence does not depend on where it stands: swap two rows
        prem[[j, furthest_at]] = prem[[furthest_at, j]]
        div[[j, furthest_at]] = div[[furthest_at, j]]
        j = choose(div)
    if n_cand > 1:
        order = np.argsort(-div, kind="stable")
        gap = div[order[0]] - div[order[1]]
        worst = max(div_bound(final, prem[order[0]], reg), div_bound(final, prem[order[1]], reg))
        assert gap >= 4.0 * worst, f"ladder_case(V={V}, n_cand={n_cand}, seed={seed}): gap {gap:.3e} < 4 x bound {worst:.3e}"
        assert furthest_at is None or j == furthest_at, (j, furthest_at)
    return final, prem, j
