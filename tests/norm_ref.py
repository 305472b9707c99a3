"""Host restatement of the normalisations (vt_rmsnorm / vt_layernorm, vitron_amd/csrc/vt_norm.hip) and of the RMSNorm folded into the
16-bit GEMMs (vt_gemm_bf16_norm, vt_gemm_bf16_resid_norm, vt_rowscale_finalize; vt_gemm.hip, vt_gemm8.hip) for tests/test_gpu_norm.py
and tests/test_norm_ref_host.py: fp64 references, the per-element bounds an fp32 implementation of them must meet (derived from the
kernels' longest summation chains, DESIGN.md "Norm pinning"), data whose results are exact in fp32 whatever the summation order
(one-hot rows, small integers with power-of-two weights), and float32 emulations of the kernels with the faults the bounds must catch.
The 16-bit store, the half ulp and the integer operands come from tests/gemm_ref.py. Plain numpy / torch on the CPU; nothing here calls
the library."""
import numpy as np
import torch

from tests import gemm_ref as G
from tests.gemm_ref import U

F32 = np.float32
# every NCH of VT_NORM_DISPATCH full and ragged: 1 (4, 256), 2 (320, 512), 4 (772, 1024), 8 (1028, 2048), 16 (4092, 4096); none divisible by 7
D_SET = (4, 256, 320, 512, 772, 1024, 1028, 2048, 4092, 4096)
# |rsqrtf(x) - x^-1/2| / x^-1/2 in units of 2^-23 (one fp32 ulp at the top of a binade). The HIP math documentation installed with the
# toolchain states no figure; measured on an MI355X through vt_rowscale_finalize over 2^16 log-spaced arguments in [1e-6, 1e6]
# (tests/test_gpu_norm.py::test_rsqrt_error_is_inside_the_constant records it; EXPERIMENTS.md): 0.773. The constant is that, rounded up to
# 0.8, + 1.
RSQRT_ULPS = 1.8
E_RSQRT = RSQRT_ULPS * 2.0 * U

# longest chain of fp32 additions behind one sum of a row: the one-wave-per-row kernels add up to NCH * 4 = 64 terms serially per lane and
# then run 6 shuffle levels (70); the 256-thread row-block kernel 16 terms + 6 levels + 3 adds of the wave sums (25)
CHAIN_WAVE = 64 + 6
CHAIN_ROW_BLOCK = 16 + 6 + 3
CHAIN = max(CHAIN_WAVE, CHAIN_ROW_BLOCK)


def rstd_rel(chain, term=1, tail=3):
    """Relative error of rstd = rsqrtf(sum * inv_dim + eps) when `sum` is an fp32 sum of non-negative terms: each term carries `term`
    roundings (x * x: 1), any order of `chain` additions at most chain more ((1 + u)^n - 1 <= n u (1 + n u), n <= 600: one more u covers the
    second order), the scaling by 1 / D (a division, or a rounded reciprocal and a product) and the addition of eps `tail` = 3. eps >= 0
    only shrinks the relative error of the argument. An argument off by r moves its inverse square root by r / 2; the device rsqrtf adds
    E_RSQRT."""
    return ((term + chain + tail) / 2.0 + 1.0) * U + E_RSQRT


E_RSTD_RMS = rstd_rel(CHAIN)


# ---- RMSNorm -----------------------------------------------------------------------------------------------------------------------------
def rms_ref(x, g, eps):
    """y64 [R][D] = x g / sqrt(mean(x^2) + eps) of fp32 x, g (eps as the kernel receives it: an fp32 number)"""
    x, g = torch.as_tensor(x).double(), torch.as_tensor(g).double()
    return x * g / torch.sqrt((x * x).mean(-1, keepdim=True) + float(F32(eps)))


def rms_bound(y64, dtype):
    """half an ulp of the store + |y| (E_RSTD_RMS + 2 U): the kernel forms (x * rstd) * g in fp32 (two roundings) and stores once. A result
    pushed over a binade boundary by the fp32 error still rounds onto that boundary, so the half ulp at |y64| holds."""
    return G.store_half_ulp(y64, dtype) + y64.abs() * (E_RSTD_RMS + 2 * U)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
C_MEAN = CHAIN_WAVE + 1                                  # the row sum's chain and the division by D
E_RSTD_LN = rstd_rel(CHAIN_WAVE, term=3)                 # a term (x - mean)^2: the difference rounds once (twice in the square), the square once


def ln_ref(x, g, b, eps):
    """(y64, d64 rstd64 g, rstd64 [R][1]) of LayerNorm in fp64"""
    x, g, b = torch.as_tensor(x).double(), torch.as_tensor(g).double(), torch.as_tensor(b).double()
    d = x - x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + float(F32(eps)))
    return d * rstd * g + b, d * rstd * g, rstd


def ln_bound(x, g, y64, t64, rstd64, dtype):
    """Per element, with t = (x - mean) rstd g and y = t + beta:
    * the fp32 mean is off by dm <= C_MEAN U mean|x| (a sum of mixed signs: the chain's error is relative to sum |x|). It shifts every
      difference by the same dm: |g| rstd dm on the output, the term  C_MEAN U mean|x| rstd |g|;
    * the deviations sum to zero, so the common shift reaches the variance in second order only: var + dm^2, i.e. rstd off by
      dm^2 rstd^2 / 2 relative (noticeable for rows far from zero: mean 1000, std 1), beside E_RSTD_LN of the chain itself;
    * x - mean, * rstd, * g: 3 U of |t|; the addition of beta: U of |y|; one store."""
    x, g = torch.as_tensor(x).double(), torch.as_tensor(g).double()
    dm = C_MEAN * U * x.abs().mean(-1, keepdim=True)
    e_rstd = E_RSTD_LN + 0.5 * (dm * rstd64) ** 2
    return G.store_half_ulp(y64, dtype) + t64.abs() * (e_rstd + 3 * U) + dm * rstd64 * g.abs() + U * y64.abs()


# ---- the folded RMSNorm ------------------------------------------------------------------------------------------------------------------
def rms_f32_part(y64, chain=CHAIN):
    """the fp32 part of rms_bound (no store) for a kernel whose longest chain of additions is `chain`: |y| (rstd_rel(chain) + 2 U)"""
    return y64.abs() * (rstd_rel(chain) + 2 * U)


def ln_f32_part(x, g, y64, t64, rstd64, chain=CHAIN_WAVE):
    """the fp32 part of ln_bound (no store) for a kernel whose longest chain of additions is `chain` (the mean's constant is chain + 1)"""
    x, g = torch.as_tensor(x).double(), torch.as_tensor(g).double()
    dm = (chain + 1) * U * x.abs().mean(-1, keepdim=True)
    e_rstd = rstd_rel(chain, term=3) + 0.5 * (dm * rstd64) ** 2
    return t64.abs() * (e_rstd + 3 * U) + dm * rstd64 * g.abs() + U * y64.abs()


def fold_rstd_rel(chain, partial_chain=0):
    """rstd of a folded-norm consumer against the fp64 rstd of the SAME x: `chain` additions over the partial sums (decode flavour: in_n / 16
    per thread + 4 shuffle levels; vt_rowscale_finalize: np / 16 per thread + 16 over the block's LDS column), `partial_chain` additions
    inside one partial (0 when the partials are given exactly; 16 for the decode producer's 16-column blocks, 32 for the tile producers'
    32-column groups: loose, any order), one rounding per square. The form of tests/test_gpu_nf4.py's rstd_rel, with the halving written out."""
    return rstd_rel(chain + partial_chain, term=1 if partial_chain else 0)


def fold_rstd64(ss64, inv_dim, eps):
    """fp64 rsqrt(ss * inv_dim + eps) with inv_dim and eps as the kernel receives them (fp32 numbers)"""
    return 1.0 / torch.sqrt(torch.as_tensor(ss64).double() * float(F32(inv_dim)) + float(F32(eps)))


def block_sums(x, width):
    """[M][N] -> fp64 [M][N / width] sums of x^2 over consecutive `width` columns"""
    x = torch.as_tensor(x).double()
    M, N = x.shape
    return (x * x).reshape(M, N // width, width).sum(-1)


def consumer_bound(acc64, r64, e_r, epi, dtype, resid64=None, e_acc=None):
    """(ref64, bound) of a folded-norm consumer whose accumulator is within e_acc of acc64 [M][N] (None: exact, integer operands) and whose
    row factor r64 [M] is held to e_r relative: acc * rstd costs one more rounding. EPI_F32: |acc r| (e_r + U). EPI_BF16: + half an ulp of the store.
    EPI_SWIGLU: gate and up errors carried through silu(g) * u (|silu'| <= 1.1) + gemm_ref.e_swiglu + the store. EPI_F32_RESID: + U of the sum."""
    y = acc64 * r64[:, None]
    e = y.abs() * (e_r + U)
    if e_acc is not None:
        e = e + e_acc * r64[:, None] * (1 + e_r + U)
    if epi == G.EPI_SWIGLU:
        g, u = G.swiglu_split(y)
        eg, eu = G.swiglu_split(e)
        s = torch.from_numpy(G.silu64(g.numpy()))
        ref = s * u
        e = 1.1 * u.abs() * eg + s.abs() * eu + eg * eu + torch.from_numpy(G.e_swiglu(g.numpy(), u.numpy()))
        return ref, e + G.store_half_ulp(ref, dtype)
    if epi == G.EPI_F32_RESID:
        ref = y + resid64
        return ref, e + U * ref.abs()
    if epi == G.EPI_BF16:
        return y, e + G.store_half_ulp(y, dtype)
    assert epi == G.EPI_F32
    return y, e


# ---- data whose results are exact -------------------------------------------------------------------------------------------------------
def onehot_rows(R, D, seed):
    """x fp32 [R][D]: row r is zero but for c_r = +-j 2^(k - 23) (j odd with bit 23 set: all 24 significand bits of fp32 in use, k in -3 .. 3)
    at column (7 r + 5) mod D -> (x, cols int64 [R], c fp64 [R]). Every other output of a norm of such a row is exactly +-0."""
    rng = np.random.default_rng(seed)
    j = (rng.integers(2 ** 22, 2 ** 23, size=R, dtype=np.int64) * 2 + 1) * (rng.integers(0, 2, size=R) * 2 - 1)
    c = j.astype(np.float64) * np.exp2(rng.integers(-3, 4, size=R) - 23.0)
    assert (c.astype(F32).astype(np.float64) == c).all()
    cols = (np.arange(R, dtype=np.int64) * 7 + 5) % D
    x = torch.zeros((R, D))
    x[torch.arange(R), torch.from_numpy(cols)] = torch.from_numpy(c.astype(F32))
    return x, cols, torch.from_numpy(c)


def onehot_want(c64, g_hit64, D, eps):
    """fp64 value of the hit column: g c / sqrt(c^2 / D + eps) (a kernel that left c out of its sum would return g c / sqrt(eps))"""
    return g_hit64 * c64 / torch.sqrt(c64 * c64 / D + float(F32(eps)))


def fold_producer_ints(M, N, K, seed, width, amax=4, span=300, bias=False):
    """Integer operands of a folded-norm producer: a [M][K], w [N][K] integers of |.| <= amax, an integer residual (and bias) of |.| <= span,
    w_next [N] powers of two 2^-2 .. 2^2 -> dict with the fp64 x_new = resid + a w^T (+ bias), xw64 = x_new * w_next and the block sums
    of x_new^2 over `width` columns (16: decode flavour, 32: tile flavour). ASSERTS the preconditions under which an fp32 kernel returns all
    three bit for bit whatever its order: width * max(x_new^2) < 2^24 (every partial sum of squares is an integer below 2^24), x_new an
    integer below 2^24 (gemm_ref.int_operands), products with powers of two exact."""
    a, w = G.int_operands(M, N, K, seed, amax=amax)
    resid = G.frac_vector(M * N, seed + 1, span=span, frac=False).reshape(M, N)
    b = G.frac_vector(N, seed + 2, span=span, frac=False) if bias else None
    wn = G.pow2_scales(N, seed + 3)
    x64, ok = G.exact_epilogue(a, w, b, resid)
    assert ok
    assert width * float((x64 * x64).max()) < 2 ** 24, (M, N, K, float(x64.abs().max()))
    xw64 = x64 * wn.double()
    assert bool((xw64.float().double() == xw64).all())
    part = block_sums(x64, width)
    assert bool((part.float().double() == part).all()) and float(part.max()) < 2 ** 24
    nb = part.shape[1]
    assert nb < 2 or bool((part[:, 1:] != part[:, :-1]).float().mean() > 0.9), "neighbouring blocks must differ"
    return dict(a=a, w=w, resid=resid, bias=b, wn=wn, x64=x64, xw64=xw64, part=part)


def distinct_partials(M, in_n, seed):
    """fp32 [M][in_n] of distinct positive integers whose row sums stay below 2^24: exact in any order of additions"""
    rng = np.random.default_rng(seed)
    v = rng.permutation(M * in_n).reshape(M, in_n).astype(np.float64) * 3 + 1
    assert v.sum(-1).max() < 2 ** 24
    return torch.from_numpy(v.astype(F32))


# ---- float32 emulations of the kernels (and of the faults the bounds must catch) ---------------------------------------------------------
def _tree(s):
    """[R][L] float32, L a power of two -> [R]: log2 L levels of pairwise additions (the depth of the shuffle reduction)"""
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
    return s[:, 0]


def _lane_sums(t, lanes):
    """t float32 [R][D] terms -> [R]: lane l adds the terms of its float4 chunks (columns 4 (l + i lanes) .. + 3, i = 0, 1, ..) serially, then
    the tree over the lanes: the order of the norm kernels (lanes = 64: one wave per row; 256: the row-block kernel, whose last two
    levels stand for the three additions of the wave sums)"""
    R, D = t.shape
    nch = -(-D // (lanes * 4))
    p = np.zeros((R, nch * lanes * 4), F32)
    p[:, :D] = t
    p = p.reshape(R, nch, lanes, 4)
    s = np.zeros((R, lanes), F32)
    for i in range(nch):
        for r in range(4):
            s = s + p[:, i, :, r]
    return _tree(s)


def _rsqrt32(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(F32)


FAULTS = ("missing", "twice", "stale")


def _faulty_terms(t, fault, col):
    """terms of the row sums with one emulated fault: the element at column `col` left out / counted twice; 'stale': the second half of
    every row's terms taken from the previous row (a prefetched row not handed over). Returns (terms, extra, affected rows)."""
    t = t.copy()
    extra = np.zeros(t.shape[0], F32)
    rows = np.arange(t.shape[0])
    if fault == "missing":
        t[:, col] = 0
    elif fault == "twice":
        extra = t[:, col].copy()
    elif fault == "stale":
        h = t.shape[1] // 2
        t[1:, h:] = t[:-1, h:].copy()
        rows = rows[1:]
    elif fault is not None:
        raise ValueError(fault)
    return t, extra, rows


def rms_f32(x, g, eps, dtype, lanes=64, fault=None, col=1):
    """vt_rmsnorm in float32 -> (y as the store leaves it, affected rows of `fault`)"""
    x, g = np.asarray(x, F32), np.asarray(g, F32)
    t, extra, rows = _faulty_terms(x * x, fault, col)
    ss = _lane_sums(t, lanes) + extra
    rstd = _rsqrt32(ss / F32(x.shape[1]) + F32(eps))
    return G.rne_op(torch.from_numpy(x * rstd[:, None] * g), dtype), rows


def ln_f32(x, g, b, eps, dtype, fault=None, col=1):
    """vt_layernorm in float32 (two passes over the row held in registers); the faults hit the sum of squared deviations"""
    x, g, b = np.asarray(x, F32), np.asarray(g, F32), np.asarray(b, F32)
    D = F32(x.shape[1])
    mean = _lane_sums(x, 64) / D
    d = x - mean[:, None]
    t, extra, rows = _faulty_terms(d * d, fault, col)
    rstd = _rsqrt32((_lane_sums(t, 64) + extra) / D + F32(eps))
    return G.rne_op(torch.from_numpy(d * rstd[:, None] * g + b), dtype), rows


def partials_f32(x, width):
    """producer side in float32: [M][N] -> [M][N / width] sums of x^2 (one term per lane, then the tree)"""
    x = np.asarray(x, F32)
    M, N = x.shape
    sq = (x * x).reshape(M * (N // width), width)
    return _tree(sq).reshape(M, N // width)


FOLD_FAULTS = ("missing", "twice", "neighbour")


def consumer_rstd_f32(part, inv_dim, eps, parts=16, fault=None, j=3):
    """consumer side in float32: `parts` threads per row add len / parts partial sums each, serially, then the tree, then rsqrtf(ss * inv_dim +
    eps). Faults: partial j left out / counted twice / taken from the neighbouring block j + 1."""
    p = np.asarray(part, F32).copy()
    M, n = p.shape
    extra = np.zeros(M, F32)
    if fault == "missing":
        p[:, j] = 0
    elif fault == "twice":
        extra = p[:, j].copy()
    elif fault == "neighbour":
        p[:, j] = p[:, j + 1]
    elif fault is not None:
        raise ValueError(fault)
    cnt = -(-n // parts)
    q = np.zeros((M, parts * cnt), F32)
    q[:, :n] = p
    q = q.reshape(M, parts, cnt)
    s = np.zeros((M, parts), F32)
    for i in range(cnt):
        s = s + q[:, :, i]
    return _rsqrt32((_tree(s) + extra) * F32(inv_dim) + F32(eps))
