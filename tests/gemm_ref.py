"""Host restatement of the 16-bit GEMM family (vt_gemm_bf16 / vt_gemm_bf16_resid_splitk, include/vitron_hip.h; vitron_amd/csrc/vt_gemm.hip,
vt_gemm8.hip) for tests/test_gpu_gemm.py and tests/test_gemm_ref_host.py: the store of both operand builds (rne_op: round to nearest even,
fp16 saturating at +-65504 with NaN kept, as vt_common.h documents f32_to_op), the data families whose results are EXACT in fp32 whatever
the kernel's summation order (small integers; one-hot probes with full-mantissa values), the order-independent per-element bound of an
fp32 accumulation for random data (sum_bound), the activation epilogues in fp64 with the error e(x) that vt_common.h's own statements about
vt_gelu_erf / vt_silu / vt_quick_gelu allow, float32 restatements of those three (same constants, same operation order), and the shape
lists both test files walk. Plain numpy / torch on the CPU; nothing here calls the library."""
import math

import numpy as np
import torch

from tests.attn_ref import fma32
from tests.nf4_ref import half_ulp

DTYPES = [torch.bfloat16, torch.float16]
FMT = {torch.bfloat16: "bf16", torch.float16: "fp16"}
MANT = {torch.bfloat16: 8, torch.float16: 11}          # significand bits, hidden bit included
U = 2.0 ** -24                                         # fp32 unit roundoff
TINY = 2.0 ** -126                                     # results below the fp32 normal range may flush
# epilogues (include/vitron_hip.h VT_EPI_*)
EPI_BF16, EPI_GELU, EPI_QGELU, EPI_RELU, EPI_F32_RESID, EPI_F32, EPI_SWIGLU = 0, 1, 2, 3, 4, 5, 6


# ---- the 16-bit store ------------------------------------------------------------------------------------------------------------------
def rne_op(x, dtype) -> torch.Tensor:
    """fp32 values -> the operand dtype as f32_to_op stores them. bf16: the bit formula of f32_to_bf16_bits (add 0x7fff + the kept LSB,
    drop 16 bits; NaN kept); fp16: clamp to +-65504 (NaN kept), then numpy's own float16 cast (round to nearest even). A float64 argument
    is rounded to fp32 first, as the kernels hold it."""
    x = np.ascontiguousarray(torch.as_tensor(x).to(torch.float32).numpy())
    if dtype == torch.float16:
        with np.errstate(invalid="ignore"):
            c = np.where(np.isnan(x), x, np.clip(x, -65504.0, 65504.0)).astype(np.float16)
        return torch.from_numpy(c)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r = np.where(np.isnan(x), np.uint16(0x7FC0), r).astype(np.uint16)
    return torch.from_numpy(r.view(np.int16)).view(torch.bfloat16)


def representable(x, dtype) -> bool:
    x = torch.as_tensor(x, dtype=torch.float32)
    return bool((x.to(dtype).float() == x).all())


# ---- a. dense small integers ------------------------------------------------------------------------------------------------------------
AMAX = 4                                               # |a|, |w| <= 4: 16 K < 2^24 up to K = 2^20


def int_operands(M, N, K, seed, amax=AMAX):
    """A [M][K], W [N][K] fp32 holding integers in [-amax, amax] (exact in bf16 and fp16). amax^2 K < 2^24, so every partial sum of every
    product, in any order and over any split of K, is an integer below 2^24: exact in fp32."""
    assert amax * amax * K < 2 ** 24
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.integers(-amax, amax + 1, size=(M, K), dtype=np.int8)).float()
    w = torch.from_numpy(rng.integers(-amax, amax + 1, size=(N, K), dtype=np.int8)).float()
    return a, w


def frac_vector(n, seed, span=600, frac=True):
    """fp32 [n]: an integer in [-span, span] (+ j / 64, j in 0..63, with frac): bias / residual values. With the integer products above
    they put the results past 256 (bf16: odd integers are ties of the store) and on odd multiples of 2^-6 (ties from 4 up in bf16, from 32
    up in fp16)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-span, span + 1, size=n).astype(np.float64)
    if frac:
        v = v + rng.integers(0, 64, size=n) / 64.0
    return torch.from_numpy(v.astype(np.float32))


def pow2_scales(M, seed, lo=-2, hi=2, big=None):
    """fp32 [M] powers of two 2^lo .. 2^hi (row_scale); `big`: every 7th row gets 2^big instead (results past fp16's 65504)."""
    rng = np.random.default_rng(seed)
    e = rng.integers(lo, hi + 1, size=M).astype(np.float64)
    if big is not None:
        e[3::7] = big
    return torch.from_numpy(np.exp2(e).astype(np.float32))


def exact_epilogue(a, w, bias=None, resid=None, rs=None):
    """(y fp64 [M][N], exact) of rs[:, None] * (a w^T) + bias (+ resid): the fp64 value, and whether every value an fp32 epilogue passes
    through on the way (the accumulator, its scaled value, the sum with the bias, the sum with the residual) is an fp32 number, so that the
    kernel's fp32 result is this value bit for bit. The matrix product runs in fp32 (exact by int_operands' condition; the host tests
    check it against fp64)."""
    acc = (a @ w.t()).double()
    steps = [acc]
    y = acc
    if rs is not None:
        y = y * rs.double()[:, None]
        steps.append(y)
    if bias is not None:
        y = y + bias.double()
        steps.append(y)
    if resid is not None:
        y = y + resid.double()
        steps.append(y)
    exact = all(bool((s.float().double() == s).all()) and bool(s.abs().max() < 2.0 ** 60) for s in steps)
    return y, exact


def swiglu_split(y):
    """[M][N] pre-activations on the interleaved-16 layout (W rows [gate 16 | up 16 | ...]) -> (gate, up), each [M][N/2]."""
    M, N = y.shape
    y4 = y.reshape(M, N // 32, 2, 16)
    return y4[:, :, 0].reshape(M, N // 2), y4[:, :, 1].reshape(M, N // 2)


# ---- b. one-hot, full-mantissa probes ----------------------------------------------------------------------------------------------------
def coprime_step(K, start=7):
    p = start
    while math.gcd(p, K) != 1:
        p += 2
    return p


def onehot_k(M, K, c=5):
    """k(m) = (m p + c) mod K with p coprime to K (odd, so that with 64 | K any 64 consecutive rows also hit every position of a 64-wide K
    step): int64 [M]."""
    return (np.arange(M, dtype=np.int64) * coprime_step(K) + c) % K


def full_mantissa(shape, dtype, seed, emin=-2, emax=1):
    """fp32 values +-j 2^(e - (p - 1)): j an ODD integer with its top bit set (all p significand bits of `dtype` in use, first and last one
    set), e in [emin, emax]. A product of two of them has at most 2 p <= 22 significant bits: exact in fp32."""
    p = MANT[dtype]
    rng = np.random.default_rng(seed)
    j = rng.integers(2 ** (p - 2), 2 ** (p - 1), size=shape, dtype=np.int32) * 2 + 1          # odd, in [2^(p-1) + 1, 2^p - 1]
    j *= rng.integers(0, 2, size=shape, dtype=np.int32) * 2 - 1
    scale = np.exp2(np.arange(emin, emax + 1) - (p - 1.0)).astype(np.float32)
    return torch.from_numpy(j.astype(np.float32) * scale[rng.integers(0, emax - emin + 1, size=shape, dtype=np.int8)])


def onehot_problem(M, N, K, dtype, seed, mirrored=False):
    """(a, w, want fp32 [M][N]): row m of A (mirrored: row n of W) is zero except one full-mantissa value at k(m), the other operand is
    dense full-mantissa, and want[m][n] = a[m][k(m)] * w[n][k(m)] (mirrored: a[m][k(n)] * w[n][k(n)]): one exact product per element."""
    rows = N if mirrored else M
    k = torch.from_numpy(onehot_k(rows, K))
    hot = torch.zeros((rows, K))
    vals = full_mantissa((rows,), dtype, seed)
    hot[torch.arange(rows), k] = vals
    dense = full_mantissa((M if mirrored else N, K), dtype, seed + 1)
    if mirrored:
        want = dense[:, k].double() * vals.double()[None, :]
        return dense, hot, want.float()
    want = vals.double()[:, None] * dense[:, k].double().t()
    return hot, dense, want.float()


# ---- c. random data: the per-element bound -----------------------------------------------------------------------------------------------
def gauss_operands(M, N, K, dtype, seed):
    """A ~ N(0, 1), W ~ N(0, 0.05^2) rounded to `dtype` (fp32 holders), bias ~ N(0, 1) fp32, resid ~ N(0, 1) fp32: the existing tests' scales"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((M, K), generator=g).to(dtype).float()
    w = (torch.randn((N, K), generator=g) * 0.05).to(dtype).float()
    return a, w, torch.randn((N,), generator=g), torch.randn((M, N), generator=g)


def sum_bound(a, w):
    """K 2^-23 sum_k |a_k w_k| [M][N] fp64: every product of two 16-bit values is exact in fp32, and K - 1 fp32 additions in ANY order are off
    by at most (K - 1) u sum|a w| (1 + O(K u)) with u = 2^-24. Taking the unit as 2^-23 covers an MFMA that truncates inside its dot product
    and leaves (K + 1) u sum|a w| for the epilogue's one or two further fp32 additions (bias, residual), which cost u |result| each: covered
    while |bias| + |resid| <= (K - 1) / 2 * sum|a w| (checked by the caller through bound_covers_epilogue)."""
    K = a.shape[1]
    return K * 2.0 ** -23 * (a.double().abs() @ w.double().abs().t())


def bound_covers_epilogue(a, w, bias=None, resid=None) -> bool:
    K = a.shape[1]
    s = a.double().abs() @ w.double().abs().t()
    extra = torch.zeros_like(s)
    if bias is not None:
        extra = extra + bias.double().abs()
    if resid is not None:
        extra = extra + resid.double().abs()
    return bool((extra <= (K - 1) / 2 * s).all())


def store_half_ulp(ref64, dtype):
    """half an ulp of `dtype` at |ref64| (fp64 tensor), as an fp64 tensor"""
    return torch.from_numpy(half_ulp(ref64.numpy(), FMT[dtype]))


# ---- d. activation epilogues --------------------------------------------------------------------------------------------------------------
XMAX = 128.0                                           # |pre-activation| of every activation test (act_operands asserts it)


def act_operands(M, N, K, seed):
    """Integers for the activation tests: A in {-2 .. 2} with about 32 non-zeros per row whatever K, W in {-1, 0, 1}: the accumulator has a
    standard deviation of about 7, so with a bias of multiples of 2^-6 in [-2, 2] the pre-activations x lie densely over [-10, 10], with
    tails to about +-30, and are exact fp32 numbers."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 3, size=(M, K)) * (rng.integers(0, 2, size=(M, K)) * 2 - 1) * (rng.random((M, K)) < min(1.0, 32.0 / K))
    w = rng.integers(-1, 2, size=(N, K))
    bias = rng.integers(-128, 129, size=N) / 64.0
    a, w, bias = torch.from_numpy(a.astype(np.float32)), torch.from_numpy(w.astype(np.float32)), torch.from_numpy(bias.astype(np.float32))
    assert float((a.abs() @ w.abs().t()).max()) + 2.0 <= XMAX
    return a, w, bias


def _np64(x):
    return np.asarray(x, dtype=np.float64)


def _erfc(z):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(_np64(z)))).numpy()


def gelu64(x):
    """x Phi(x) = 0.5 x erfc(-x / sqrt 2): the exact-erf GELU without cancellation in the negative tail"""
    x = _np64(x)
    return 0.5 * x * _erfc(-x / math.sqrt(2.0))


def silu64(x):
    x = _np64(x)
    return x / (1.0 + np.exp(-x))


def qgelu64(x):
    x = _np64(x)
    return x / (1.0 + np.exp(-1.702 * x))


def _flush(x):
    """A factor below the fp32 normal range (q, or the reciprocal of 1 + exp once the exponential passes 2^126 or overflows) may flush to
    zero: the result is then 0 where the true one is at most |x| 2^-126."""
    return (1.0 + np.abs(_np64(x))) * TINY


def e_gelu(x):
    """|vt_gelu_erf(x) - gelu64(x)| allowed by vt_common.h's statements: the kernel forms q ~ erfc(z), z = |x| / sqrt 2, from Abramowitz & Stegun
    7.1.26 (|error| <= 1.5e-7 on erf) and returns 0.5 x (2 - q) or 0.5 x q. In fp32, with u = 2^-24:
    * z: the rounded constant and one product, 2 u; t = rcp(fma(p, z, 1)): 2 u from z (p z / (1 + p z) < 1), 1 u the fma, 2 u the 1-ulp
      reciprocal: 5 u.
    * the degree-4 Horner form P(t), t in (0, 1]: sum |c_i| = 4.475, P >= 0.2548; an error of 5 u in t moves t^i by 5 i u, four fmas round once
      each: |dP| <= 4.475 (20 + 4) u = 107.4 u, relative 421.5 u.
    * exp2(w'), w' = (z z) (-log2 e) held to 2 u + 2 u + 1 u + 2 u = 7 u relative, so the exponential moves by 7 |w'| ln 2 u = 4.86 |w'| u, plus
      2 u for the 1-ulp hardware exp2.
    * the two products that join P, t and the exponential: 2 u. Together q is within rho = (421.5 + 5 + 2 + 2 + 4.86 |w'|) u < (431 + 4.9 |w'|) u
      of the formula, relative; and the final 2 - q and two products: 3 u of the result.
    e(x) = 0.5 |x| (1.5e-7 + rho erfc(z)) + 3 u |gelu(x)| + _flush(x)."""
    x = _np64(x)
    z = np.abs(x) / math.sqrt(2.0)
    wp = z * z * 1.4426950408889634
    rho = (431.0 + 4.9 * wp) * U
    return 0.5 * np.abs(x) * (1.5e-7 + rho * _erfc(z)) + 3 * U * np.abs(gelu64(x)) + _flush(x)


def e_silu(x):
    """|vt_silu(x) - silu64(x)|: x * rcp(1 + __expf(-x)), __expf(y) = exp2(y log2 e) in hardware: the argument's product rounds (2 u with its
    constant, i.e. 2 |x| log2 e ln 2 u = 2 |x| u on the exponential), 2 u the 1-ulp exp2; 1 + s: the error of s passes at most unchanged, 1 u
    the add; 2 u the 1-ulp reciprocal; 1 u the product: (2 |x| + 6) u relative, taken as (2 |x| + 8) u."""
    x = _np64(x)
    return (2.0 * np.abs(x) + 8.0) * U * np.abs(silu64(x)) + _flush(x)


def e_qgelu(x):
    """|vt_quick_gelu(x) - qgelu64(x)|: as e_silu with the argument -1.702f x: the fp32 constant (1 u), its product (1 u) and the product with
    log2 e (2 u): 4 * 1.702 |x| u on the exponential, taken as 7 |x| u; the rest as in e_silu."""
    x = _np64(x)
    return (7.0 * np.abs(x) + 8.0) * U * np.abs(qgelu64(x)) + _flush(x)


def e_swiglu(g, up):
    """silu(g) * up with exact g, up: e_silu(g) |up| and one more product"""
    g, up = _np64(g), _np64(up)
    return e_silu(g) * np.abs(up) + U * np.abs(silu64(g) * up) + _flush(up)


F32 = np.float32


def _exp2_32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(x.astype(np.float64)).astype(F32)


def _rcp32(x):
    with np.errstate(divide="ignore", over="ignore"):
        return (1.0 / x.astype(np.float64)).astype(F32)


def gelu_f32(x):
    """vt_gelu_erf in numpy float32: the same constants, fmas and order"""
    x = np.asarray(x, F32)
    z = np.abs(x) * F32(0.70710678118654752)
    t = _rcp32(fma32(F32(0.3275911), z, F32(1.0)))
    q = fma32(F32(1.061405429), t, F32(-1.453152027))
    q = fma32(q, t, F32(1.421413741))
    q = fma32(q, t, F32(-0.284496736))
    q = fma32(q, t, F32(0.254829592))
    q = q * (t * _exp2_32(z * z * F32(-1.4426950408889634)))
    return (F32(0.5) * x) * np.where(x >= 0, F32(2.0) - q, q)


def _expf32(y):
    """__expf: exp2(y * log2 e) on the hardware exponential"""
    return _exp2_32(np.asarray(y, F32) * F32(1.4426950408889634))


def silu_f32(x):
    x = np.asarray(x, F32)
    return x * _rcp32(F32(1.0) + _expf32(-x))


def qgelu_f32(x):
    x = np.asarray(x, F32)
    return x * _rcp32(F32(1.0) + _expf32(F32(-1.702) * x))


# ---- the shapes --------------------------------------------------------------------------------------------------------------------------
TILE_ROWS = {2: 128, 3: 256, 4: 256, 5: 64, 6: 256, 8: 256, 10: 256, 13: 256, 14: 320, 15: 160, 16: 224}
CLASSIC = (2, 3, 4, 5)                                 # launch_tile: N % 4 == 0 is enough
ROW_SCALE_CFGS = (0, 2, 3, 4, 5, 6, 10)                # `tile_cfg` of vt_gemm_launch's norm-fold branch
N_RAGGED = 288                                         # a multiple of 32, not of 128 or 256: two or three column tiles, the last one ragged
N_MULT4 = 268                                          # a multiple of 4 only


def k_rule(cfg):
    """(shortest K, K multiple) the configuration documents"""
    if cfg in (6, 10, 13, 14, 16):
        return 256, 128
    if cfg == 15:
        return 256, 256
    if cfg == 9:
        return 8, 8
    return 64, 64


def legal(cfg, M, N, K, epi=EPI_BF16, row_scale=False) -> bool:
    """the documented constraints of an explicit configuration (include/vitron_hip.h, the VT_REQUIREs of vt_gemm_launch)"""
    kmin, kmult = k_rule(cfg)
    if K < kmin or K % kmult or N % 4:
        return False
    if cfg in (1, 9):
        if M > (32 if cfg == 1 else 16) or (cfg == 1 and M > 16 and K % 64):
            return False
    elif cfg not in CLASSIC and N % 32:
        return False
    if epi == EPI_SWIGLU and N % 32:
        return False
    if row_scale and (cfg not in ROW_SCALE_CFGS or N % 32 or K % 64):
        return False
    return True


def tile_ks(cfg):
    kmin, kmult = k_rule(cfg)
    long_k = {64: 2112, 128: 2176, 256: 2304}[kmult]   # 33 / 17 / 9 steps
    return [kmin, 3 * kmult, long_k]


def cfg_cases(full=True):
    """(cfg, M, N, K) of every explicit configuration: M = tile rows - 1, tile rows, tile rows + 1 and one and a half tiles + 5; K = the
    shortest legal loop, three steps, a long odd loop (>= 2048); N ragged against the tile; the classic tiles also at an N that is a
    multiple of 4 only. full=False: the subset the slower families walk (M = tile rows + 1 and the ragged two-tile M; the shortest and the
    long loop)."""
    out = []
    for cfg, tr in TILE_ROWS.items():
        ks = tile_ks(cfg)
        for M in (tr - 1, tr, tr + 1, tr + tr // 2 + 5):
            for K in ks:
                if K == ks[2] and M in (tr - 1, tr):
                    continue
                if not full and (M in (tr - 1, tr) or K == ks[1]):
                    continue
                out.append((cfg, M, N_RAGGED, K))
        if cfg in CLASSIC:
            out.append((cfg, tr + 1, N_MULT4, ks[1]))
    for cfg in (1, 9):
        ks = [64, 192, 2112] + ([8, 200] if cfg == 9 else [])
        for M in (1, 8, 9, 16):
            for K in ks:
                if not full and (M in (1, 8) or K in (192, 8)):
                    continue
                out.append((cfg, M, N_RAGGED, K))
        out.append((cfg, 9, N_MULT4, 192 if cfg == 1 else 200))
    out += [(1, 17, N_RAGGED, 64), (1, 32, N_RAGGED, 192)]        # cfg 1 above 16 rows: the 32-row weight-streaming kernel
    assert all(legal(*c) for c in out)
    return out


AUTO_MS = (1, 16, 17, 32, 33, 48, 64, 65)


def auto_cases(full=True):
    """(0, M, N, K): AUTO at every dispatch class of M (M <= 8 / <= 16 weight-streaming kernels, the 32-row kernel, two groups of 32, the
    first tile grid), the ragged-K fallback (K % 64 != 0, K % 8 == 0: M <= 16 only), the 32-row kernel's wide variant (N >= 8192) and the
    33..64-row tile grid behind N > 16384."""
    out = [(0, M, N_RAGGED, K) for M in AUTO_MS for K in ((64, 192, 2112) if full else (64, 2112))]
    out += [(0, 5, N_RAGGED, 200), (0, 16, N_MULT4, 72), (0, 24, 8192 + 32, 128), (0, 40, 16384 + 32, 64)]
    return out


def all_cases(full=True):
    return cfg_cases(full) + auto_cases(full)


def case_id(c):
    return "cfg%d-%dx%dx%d" % c
