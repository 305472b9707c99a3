"""Host restatement of the MX-FP4 operand images of precise level 3 (vt_mx4_quant_lo, vt_rmsnorm_mx, vt_layernorm_mx and the SwiGLU / GELU /
quick-GELU operand-out epilogues of vt_gemm8x.inc; vitron_amd/csrc/vt_mx4.hip, vt_mx4.h) for tests/test_gpu_mx4.py,
tests/test_gpu_mx4_image.py and tests/test_mx4_ref_host.py: the image's storage (nibble order, the lane-ordered scale array), the
per-element contract of an operand-out producer against an fp64 value and a derived bound (image_check), data whose fp32 value is known
exactly whatever the summation order (so that the whole image must equal the oracle's mx4_quant bit for bit), float32 emulations of the
producers with the faults the checks must catch, and the shape lists both test files walk. The quantisation rule itself is the oracle's
(oracle/vitron_oracle.py mx4_exponent / mx4_round / mx4_codes); the bounds come from tests/norm_ref.py and tests/gemm_ref.py (DESIGN.md
"MX image pinning"). Plain numpy / torch on the CPU; nothing here calls the library."""
import numpy as np
import torch

from oracle import vitron_oracle as O
from tests import gemm_ref as G
from tests import norm_ref as NR
from tests.gemm_ref import U

F32 = np.float32
BLOCK = 32
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
FILL = 0xA5                                              # what the guarded buffers hold before a launch


# ---- storage ---------------------------------------------------------------------------------------------------------------------------------
def _unpack(codes_u8):
    """uint8 [R][K/2] -> int codes [R][K] (even k in bits 3:0)."""
    c = codes_u8.cpu().to(torch.int32)
    return torch.stack([c & 15, c >> 4], dim=-1).reshape(c.shape[0], -1)


def _aexp_rows(aexp, M, K):
    """the GEMM-order scale array -> biased exponents [M][K/32]"""
    KB = K // 32
    a = aexp.cpu().to(torch.int32)[: ((M + 63) // 64) * KB * 64].view(-1, KB, 16, 4)      # [m / 64][kb][m % 16][(m % 64) / 16]
    m = torch.arange(M)
    return a[m // 64, :, m % 16, (m % 64) // 16]


def _deq(codes, exps_biased, block):
    v = E2M1[codes & 7] * torch.where((codes & 8) != 0, -1.0, 1.0)
    sc = torch.ldexp(torch.ones(exps_biased.shape), exps_biased - 127)
    return (v.view(codes.shape[0], -1, block) * sc.view(codes.shape[0], -1, 1)).reshape(codes.shape)


def aexp_bytes(M, K):
    """vt_mx4_aexp_bytes restated: rows padded to whole 256-row tiles, one byte per (row, 32 k)"""
    return -(-M // 256) * 256 * (K // 32)


def pack_codes(codes):
    """int codes [R][K] -> uint8 [R][K/2] (the inverse of _unpack)"""
    c = codes.to(torch.int32).view(codes.shape[0], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8)


def aexp_pack(exps_biased, K, fill=0, pad=0, swapped=False):
    """biased exponents [M][K/32] -> the scale array uint8 [aexp_bytes(M, K)]: `pad` in the rows of the last 64-row group past M (the norm
    producers store 0 there), `fill` in the row groups nobody writes. swapped: the fault m % 16 <-> (m % 64) / 16."""
    M, KB = exps_biased.shape
    groups = -(-M // 64)
    out = torch.full((aexp_bytes(M, K),), fill, dtype=torch.uint8)
    body = torch.full((groups, KB, 64), pad, dtype=torch.uint8)
    m = torch.arange(M)
    pos = ((m % 64) // 16) * 16 + m % 16 if swapped else (m % 16) * 4 + (m % 64) // 16
    body[m // 64, :, pos] = exps_biased.to(torch.uint8)
    out[: groups * KB * 64] = body.view(-1)
    return out


def code_values(codes):
    """4-bit codes -> the e2m1 values they stand for (fp64)"""
    return (E2M1[codes & 7] * torch.where((codes & 8) != 0, -1.0, 1.0)).double()


# ---- the per-element contract ----------------------------------------------------------------------------------------------------------------
def _bmax(a):
    return a.reshape(a.shape[0], -1, BLOCK).amax(-1)


def _wide(b):
    return b.repeat_interleave(BLOCK, dim=1)


def _intervals(v64, delta, y_got, exps):
    """(lo, e_min, e_max, q_lo, q_hi): the kernel's remainder is lo_k = v_k - y with |v_k - v64| <= delta, an fp32 number, so |lo_k| lies in
    [|lo| - delta, |lo| + delta]; mx4_exponent is monotone in the block maximum and mx4_round is monotone in its argument."""
    v64 = torch.as_tensor(v64).double()
    delta = torch.as_tensor(delta).double().expand_as(v64)
    lo = v64 - y_got.double()
    e_min = O.mx4_exponent(_bmax((lo.abs() - delta).clamp(min=0.0)))
    e_max = O.mx4_exponent(_bmax(lo.abs() + delta))
    sc = _wide(torch.ldexp(torch.ones(exps.shape, dtype=torch.float64), exps.to(torch.int32) - 127))
    return lo, e_min, e_max, O.mx4_round((lo - delta) / sc), O.mx4_round((lo + delta) / sc)


def image_check(v64, delta, y_got, codes, exps, dtype):
    """The contract of an operand-out producer whose fp32 value v_k is within `delta` of the fp64 value v64 [M][K]; y_got the 16-bit output,
    codes int [M][K], exps biased [M][K/32] -> four boolean masks:
      hi ok [M][K]       |v64 - y_got| <= half an ulp of the store at v64 + delta;
      exponent ok [M][K/32]  with lo = v64 - f64(y_got), the stored exponent lies in [mx4_exponent(max_block(|lo| - delta)),
                         mx4_exponent(max_block(|lo| + delta))];
      code ok [M][K]     the stored e2m1 value lies between mx4_round((lo - delta) / 2^e_got) and mx4_round((lo + delta) / 2^e_got) -- against
                         the STORED exponent, so that a block whose exponent is in doubt still pins its codes (the sign of a zero is not
                         compared: -0 == 0);
      ambiguous [M][K]   the code interval holds more than one value, or the block's exponent interval does."""
    v64 = torch.as_tensor(v64).double()
    delta = torch.as_tensor(delta).double().expand_as(v64)
    lo, e_min, e_max, q_lo, q_hi = _intervals(v64, delta, y_got, exps)
    hi_ok = (v64 - y_got.double()).abs() <= G.store_half_ulp(v64.contiguous(), dtype) + delta
    e_got = exps.to(torch.int32) - 127
    exp_ok = (e_got >= e_min) & (e_got <= e_max)
    q_got = code_values(codes)
    code_ok = (q_got >= q_lo) & (q_got <= q_hi)
    return hi_ok, exp_ok, code_ok, (q_lo != q_hi) | _wide(e_min != e_max)


def ambiguous_shares(v64, delta, y, exps):
    """(share of elements whose code interval holds more than one value, share of blocks whose exponent interval does)"""
    _, e_min, e_max, q_lo, q_hi = _intervals(v64, delta, y, exps)
    return float((q_lo != q_hi).double().mean()), float((e_min != e_max).double().mean())


def reference_shares(v64, delta, dtype):
    """ambiguous_shares of the reference alone: hi = op16(v64), the exponents of its own remainder"""
    y = G.rne_op(v64, dtype)
    e = O.mx4_quant((torch.as_tensor(v64).double() - y.double()).float(), BLOCK)[2] + 127
    return ambiguous_shares(v64, delta, y, e)


_EDGE_LO = torch.tensor([-0.25, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=torch.float64)
_EDGE_HI = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, float("inf")], dtype=torch.float64)


def implied_ratio(v64, delta, y_got, codes, exps, dtype):
    """The largest |v_implied - v64| / delta: how far, in units of its bound, the fp64 value has to move before the stored 16-bit value is
    its rounding and the stored code is the rounding of its remainder at the stored exponent (0: the image is the reference's own)."""
    v64 = torch.as_tensor(v64).double()
    delta = torch.as_tensor(delta).double().expand_as(v64)
    lo = v64 - y_got.double()
    sc = _wide(torch.ldexp(torch.ones(exps.shape, dtype=torch.float64), exps.to(torch.int32) - 127))
    mag = (codes & 7).long()
    sign = torch.where(mag == 0, torch.sign(lo), torch.where((codes & 8) != 0, -1.0, 1.0).double())
    t = lo / sc * torch.where(sign == 0, torch.ones_like(sign), sign)
    need = torch.maximum((_EDGE_LO[mag] - t).clamp(min=0.0), (t - _EDGE_HI[mag]).clamp(min=0.0)) * sc
    need = torch.maximum(need, ((v64 - y_got.double()).abs() - G.store_half_ulp(v64.contiguous(), dtype)).clamp(min=0.0))
    ok = delta > 0
    return float((need[ok] / delta[ok]).max()) if bool(ok.any()) else 0.0


def assert_image(v64, delta, y_got, codes, exps, dtype, what):
    """every mask of image_check true everywhere, and the nearest code wherever the element is not ambiguous -> (worst implied ratio, code
    share, exponent share) for the record"""
    hi_ok, exp_ok, code_ok, amb = image_check(v64, delta, y_got, codes, exps, dtype)
    assert bool(hi_ok.all()), f"{what}: {int((~hi_ok).sum())} 16-bit values outside the bound, first at {(~hi_ok).nonzero()[0].tolist()}"
    assert bool(exp_ok.all()), f"{what}: {int((~exp_ok).sum())} block exponents outside their interval, first at (row, block) {(~exp_ok).nonzero()[0].tolist()}"
    assert bool(code_ok.all()), f"{what}: {int((~code_ok).sum())} codes outside their interval, first at {(~code_ok).nonzero()[0].tolist()}"
    lo = torch.as_tensor(v64).double() - y_got.double()
    sc = _wide(torch.ldexp(torch.ones(exps.shape, dtype=torch.float64), exps.to(torch.int32) - 127))
    off = (code_values(codes) != O.mx4_round(lo / sc)) & ~amb
    assert not bool(off.any()), f"{what}: {int(off.sum())} unambiguous codes are not the nearest code, first at {off.nonzero()[0].tolist()}"
    return (implied_ratio(v64, delta, y_got, codes, exps, dtype),) + ambiguous_shares(v64, delta, y_got, exps)


def exact_image(v32, dtype):
    """fp32 values [M][K] -> (y as the store leaves it, codes int [M][K], biased exponents [M][K/32]) of the oracle"""
    v32 = torch.as_tensor(v32, dtype=torch.float32)
    y = G.rne_op(v32, dtype)
    _, q, e = O.mx4_quant(v32 - y.float(), BLOCK)          # (the difference of an fp32 number and its 16-bit rounding is an fp32 number)
    return y, O.mx4_codes(q), e + 127


def assert_exact(v32, dtype, y_got, codes, exps, what):
    """the whole output equals the oracle's image of the known fp32 value bit for bit (the sign of a zero code is not compared)"""
    y, c, e = exact_image(v32, dtype)
    bad = y_got.view(torch.int16) != y.view(torch.int16)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} 16-bit values differ, first at {bad.nonzero()[0].tolist()}"
    bad = exps.to(torch.int32) != e
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} block exponents differ, first at (row, block) {bad.nonzero()[0].tolist()}: got {int(exps[bad][0])}, want {int(e[bad][0])}"
    bad = ((codes & 7) != (c & 7)) | (((codes & 8) != (c & 8)) & ((c & 7) != 0))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} codes differ, first at {bad.nonzero()[0].tolist()}"


def assert_pad_rows(aexp, M, K, what, fill=FILL):
    """the norm producers store exponent byte 0 for the rows of the last 64-row group past M and nothing behind that group"""
    KB = K // 32
    groups = -(-M // 64)
    a = aexp.cpu().to(torch.int32)
    body = a[: groups * KB * 64].view(groups, KB, 16, 4)
    m = torch.arange(M, groups * 64)
    if len(m):
        pad = body[m // 64, :, m % 16, (m % 64) // 16]
        assert bool((pad == 0).all()), f"{what}: {int((pad != 0).sum())} exponent bytes of the rows past {M} are not 0"
    rest = a[groups * KB * 64:]
    assert bool((rest == fill).all()), f"{what}: {int((rest != fill).sum())} bytes written behind the last row group"


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------------
CHAIN_RMS_MX = 16 * 8 + 6                                # rmsnorm_mx_kernel<16>: eight squares per chunk and lane, 16 chunks, 6 shuffle levels
CHAIN_LN_MX = NR.CHAIN_WAVE                              # layernorm_mx_kernel<16>: four terms per chunk and lane, 16 chunks, 6 shuffle levels


def rms_delta(v64):
    return NR.rms_f32_part(v64, CHAIN_RMS_MX)


def ln_delta(x, g, y64, t64, rstd64):
    return NR.ln_f32_part(x, g, y64, t64, rstd64, CHAIN_LN_MX)


ACT64 = {"gelu": G.gelu64, "qgelu": G.qgelu64}
ACT_E = {"gelu": G.e_gelu, "qgelu": G.e_qgelu}
ACT_F32 = {"gelu": G.gelu_f32, "qgelu": G.qgelu_f32}
ACT_FLOOR = {"gelu": 8.0, "qgelu": 12.0, "swiglu": 20.0}     # from here up the activation is the identity in fp32 (test_mx4_ref_host.py)


def act_ref(pre32, kind):
    """(v64, delta) of an activation epilogue on the fp32 pre-activations [M][N] the kernel holds (swiglu: the interleaved-16 layout)"""
    p = torch.as_tensor(pre32).double()
    if kind == "swiglu":
        g, u = G.swiglu_split(p)
        g, u = g.numpy(), u.numpy()
        return torch.from_numpy(G.silu64(g) * u), torch.from_numpy(G.e_swiglu(g, u))
    return torch.from_numpy(ACT64[kind](p.numpy())), torch.from_numpy(ACT_E[kind](p.numpy()))


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 17, 64, 65, 130)
RMS_D = (512, 1024, 1536, 4096, 4608, 8192)              # rmsnorm_mx_kernel<2> / <8> / <16>, each full and with ragged chunks
LN_D = (256, 768, 1024, 1280, 4096)                      # layernorm_mx_kernel<4> / <16>
K_SET = (-3, 0, 5)                                       # x = +-2^k of the exact norm probes


def norm_cases(ds):
    """(rows, D): every row count at every width"""
    return [(rows, D) for D in ds for rows in ROWS]


SWIGLU_N = (128, 384, 640)
GELU_N = (64, 192, 320)
GEMM_M = (1, 63, 65, 257, 300)
GEMM_K = (256, 384)


def gemm_cases(ns):
    """(M, N, K): every (M, N) pair at one K"""
    return [(M, N, GEMM_K[(i + j) % 2]) for i, M in enumerate(GEMM_M) for j, N in enumerate(ns)]


def gemm_seed(M, N, K):
    """the seed of both data families of a GEMM case. One row gives an epilogue two to ten blocks: with the plain seed some of those cases
    hold no tie or no pair of neighbouring blocks with different exponents; SEED_SALT is the first salt with which every M = 1 case shows
    every fault (tests/test_mx4_ref_host.py proves it for the salt in use)"""
    return M + N + K + SEED_SALT


SEED_SALT = 19
ZERO_TILE_N = 384                                        # the SwiGLU variant whose second column tile has up == 0


# ---- data whose image is known exactly ---------------------------------------------------------------------------------------------------------
def full_mantissa32(shape, rng, emin=-2, emax=1):
    """fp32 +-j 2^(e - 23), j odd with bit 23 set (all 24 significand bits in use), e in [emin, emax]"""
    j = (rng.integers(2 ** 22, 2 ** 23, size=shape, dtype=np.int64) * 2 + 1) * (rng.integers(0, 2, size=shape) * 2 - 1)
    v = j.astype(np.float64) * np.exp2(rng.integers(emin, emax + 1, size=shape) - 23.0)
    assert (v.astype(F32).astype(np.float64) == v).all()
    return v.astype(F32)


TIES = (6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)       # in units of the block scale: the block maximum 6 (mantissa exactly 1.5), then every tie


def _plant_ties(g):
    """g[0:8] = 1 + TIES 2^-15: op16 rounds them to 1 in both formats, the remainders are 6 2^-15 (the block's maximum: exponent -15, nothing
    above it in the block) and the seven ties of e2m1 at that scale; the rest of the first block stays below the maximum"""
    g[:BLOCK] = 1.0 + np.abs(g[:BLOCK] - np.round(g[:BLOCK])) * 2.0 ** -15
    g[:8] = 1.0 + np.asarray(TIES) * 2.0 ** -15
    return g


def rms_exact(rows, D, seed, ks=K_SET):
    """x[r][c] = +-2^k_r (random signs), eps = 0: mean square 4^k, rstd 2^-k, v = +-g[c] exactly -> (x, g, v32)"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, size=(rows, D)) * 2.0 - 1.0
    k = np.asarray(ks)[np.arange(rows) % len(ks)]
    g = _plant_ties(full_mantissa32(D, rng))
    x = (s * np.exp2(k)[:, None]).astype(F32)
    return torch.from_numpy(x), torch.from_numpy(g), torch.from_numpy((s * g.astype(np.float64)).astype(F32))


def ln_exact(rows, D, seed, ks=K_SET):
    """x = +-2^k_r with exactly D / 2 of each sign in a shuffled order, eps = 0: mean 0, rstd 2^-k, v = fl32(+-g + b) -> (x, g, b, v32)"""
    rng = np.random.default_rng(seed)
    s = np.stack([rng.permutation(D) for _ in range(rows)]) % 2 * 2.0 - 1.0
    k = np.asarray(ks)[np.arange(rows) % len(ks)]
    g = _plant_ties(full_mantissa32(D, rng))
    b = full_mantissa32(D, rng, emin=-3, emax=0)
    b[:BLOCK] = 0.0
    x = (s * np.exp2(k)[:, None]).astype(F32)
    v = (s * g.astype(np.float64) + b.astype(np.float64)).astype(F32)      # (the fp64 sum of two fp32 numbers this close is exact: one rounding)
    return torch.from_numpy(x), torch.from_numpy(g), torch.from_numpy(b), torch.from_numpy(v)


N_FIXED = 12


def mx_gemm_ints(M, N, K, seed, kind, dtype, zero_tile=False):
    """Integer operands of an operand-out GEMM whose activation saturates to the identity. A: integers -3 .. 3, arbitrary 4-bit codes, block
    exponents 126 .. 128, and N_FIXED columns spread over K that hold 2 or 3. An activated row of W (every row for gelu / qgelu, the gate
    rows for swiglu) holds 2 in the fixed columns (48 .. 72), two more entries of |.| <= 2 (|.| <= 12) and ONE 4-bit code of |value| <= 1
    (|.| <= 12): its accumulators lie in [24, 96] whatever A's random part is. The up rows of swiglu are free: integers -2 .. 2, arbitrary
    codes in one position of eight, exponents 126 / 127. The bias (gelu / qgelu) has a full random mantissa below 4, but every fourth
    column a multiple of 2^-6 (bf16) / 2^-9 (fp16): remainders on the ties of e2m1. zero_tile: the up rows of the second 256-column tile
    are zero in both images -> dict(a, a4, ea, w, w4, ew, bias, pre64 [M][N], v32 [M][outputs], zero (a column slice or None))."""
    rng = np.random.default_rng(seed)
    KB = K // 32
    a = rng.integers(-3, 4, size=(M, K)).astype(np.float64)
    kf = np.arange(N_FIXED) * (K // N_FIXED) + 5
    a[:, kf] = rng.integers(2, 4, size=(M, N_FIXED))
    a4 = rng.integers(0, 256, size=(M, K // 2)).astype(np.uint8)
    ea = rng.integers(126, 129, size=(M, KB))
    free = np.setdiff1d(np.arange(K), kf)
    w = np.zeros((N, K))
    w4c = np.zeros((N, K), np.int64)
    ew = rng.integers(126, 128, size=N)
    act_row = np.ones(N, bool) if kind != "swiglu" else (np.arange(N) % 32) < 16
    for n in range(N):
        if act_row[n]:
            w[n, kf] = 2
            w[n, rng.choice(free, 2, replace=False)] = rng.choice([-2, -1, 1, 2], 2)
            w4c[n, rng.integers(0, K)] = rng.integers(1, 3) | (rng.integers(0, 2) << 3)
        else:
            w[n] = rng.integers(-2, 3, size=K)
            w4c[n] = rng.integers(0, 16, size=K) * (rng.random(K) < 0.125)
    zero = None
    if zero_tile:
        assert kind == "swiglu" and N > 256
        w[256:][~act_row[256:]] = 0
        w4c[256:][~act_row[256:]] = 0
        zero = slice(128, N // 2)
    bias = None
    if kind != "swiglu":
        bias = full_mantissa32(N, rng, emin=-2, emax=1).astype(np.float64)
        frac = 2.0 ** (-6 if dtype == torch.bfloat16 else -9)
        bias[1::4] = np.round(bias[1::4] / frac) * frac
        bias = torch.from_numpy(bias.astype(F32))
    a, w = torch.from_numpy(a).float(), torch.from_numpy(w).float()
    a4 = torch.from_numpy(a4)
    ea, ew = torch.from_numpy(ea), torch.from_numpy(ew)
    w4 = pack_codes(torch.from_numpy(w4c))
    acc = a.double() @ w.double().t() + _deq(_unpack(a4), ea, BLOCK).double() @ _deq(_unpack(w4), ew.view(-1, 1), K).double().t()
    assert float(acc.abs().max()) * 16 < 2 ** 24 and torch.equal(acc * 16, (acc * 16).round())      # every partial sum is an fp32 number
    pre = acc if bias is None else (acc + bias.double()).float().double()
    if kind == "swiglu":
        g, up = G.swiglu_split(pre)
        v = (g * up).float()
        gate = g
    else:
        v = pre.float()
        gate = pre
    assert float(gate.min()) >= ACT_FLOOR[kind] and float(gate.max()) <= G.XMAX, (float(gate.min()), float(gate.max()))
    assert float(v.abs().max()) < 60000.0
    return dict(a=a, a4=a4, ea=ea, aexp=aexp_pack(ea, K), w=w, w4=w4, ew=ew.to(torch.uint8), bias=bias, pre64=pre, v32=v, zero=zero)


def resid_ints(M, N, K, seed):
    """the operands of test_gemm_mx_exact_on_integers with an integer residual |.| <= 300 -> dict with ref64 = resid + both products"""
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.integers(-3, 4, size=(M, K))).float()
    w = torch.from_numpy(rng.integers(-2, 3, size=(N, K))).float()
    a4 = torch.from_numpy(rng.integers(0, 256, size=(M, K // 2)).astype(np.uint8))
    w4 = torch.from_numpy(rng.integers(0, 256, size=(N, K // 2)).astype(np.uint8))
    ea = torch.from_numpy(rng.integers(126, 129, size=(M, K // 32)))
    ew = torch.from_numpy(rng.integers(126, 128, size=N))
    resid = torch.from_numpy(rng.integers(-300, 301, size=(M, N))).float()
    acc = a.double() @ w.double().t() + _deq(_unpack(a4), ea, BLOCK).double() @ _deq(_unpack(w4), ew.view(-1, 1), K).double().t()
    ref = acc + resid.double()
    for s in (acc, ref):
        assert float(s.abs().max()) * 16 < 2 ** 24 and torch.equal(s * 16, (s * 16).round())
    return dict(a=a, a4=a4, aexp=aexp_pack(ea, K), w=w, w4=w4, ew=ew.to(torch.uint8), resid=resid, ref64=ref)


def quant_lo_probes(dtype, M=70, K=128, seed=11):
    """16-bit remainders [M][K] (fp32 holders) for vt_mx4_quant_lo, and the blocks [M][K/32] planted in them -> (lo, dict of masks):
    'm15'  block 0 of rows 0, 3, ..: one value 1.5 2^e, the rest at most 0.25 2^e (the mantissa test of mx4_exponent sits on its edge);
    'six'  block 1 of rows 1, 4, ..: the maximum 6 2^e with every tie of e2m1 at that scale beside it;
    'sub'  block 2 of rows 2, 5, .. (fp16 only): nothing but fp16 subnormals, multiples of 2^-24 below 2^-14."""
    rng = np.random.default_rng(seed)
    v = torch.from_numpy(rng.standard_normal((M, K)).astype(F32)) * 4
    lo = G.rne_op(v - G.rne_op(v, dtype).float(), dtype).float()
    masks = {k: torch.zeros((M, K // BLOCK), dtype=torch.bool) for k in ("m15", "six", "sub")}
    for r in range(M):
        e = -3 - r % 8
        s = torch.from_numpy(rng.integers(0, 2, size=BLOCK) * 2.0 - 1.0).float()
        if r % 3 == 0:
            blk = torch.from_numpy(rng.integers(-8, 9, size=BLOCK)).float() * 2.0 ** (e - 5)
            blk[int(rng.integers(0, BLOCK))] = 1.5 * 2.0 ** e * float(s[0])
            lo[r, :BLOCK] = blk
            masks["m15"][r, 0] = True
        elif r % 3 == 1:
            blk = torch.from_numpy(rng.integers(-8, 9, size=BLOCK)).float() * 2.0 ** (e - 3)
            blk[:8] = torch.tensor(TIES) * 2.0 ** e
            lo[r, BLOCK:2 * BLOCK] = (blk * s)[torch.from_numpy(rng.permutation(BLOCK))]
            masks["six"][r, 1] = True
        elif dtype == torch.float16:
            blk = torch.from_numpy(rng.integers(-1023, 1024, size=BLOCK)).float() * 2.0 ** -24
            blk[0] = 1023 * 2.0 ** -24
            lo[r, 2 * BLOCK:3 * BLOCK] = blk
            masks["sub"][r, 2] = True
    return lo + 0.0, masks                               # (-0 + 0 = +0: no negative zeros, whose code the comparison would have to exempt)


# ---- Gaussian data -------------------------------------------------------------------------------------------------------------------------------
EPS = 1e-5


def rms_gauss(rows, D, seed):
    """Gaussian rows, three in ten scaled x 60 (the data of test_rmsnorm_mx), g = 1 + 0.1 N(0, 1) -> (x, g)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, D), generator=gen) * (1 + 59 * (torch.rand((rows, 1), generator=gen) < 0.3))
    return x, 1 + 0.1 * torch.randn((D,), generator=gen)


def ln_gauss(rows, D, seed):
    """Gaussian rows (scale 3, the towers' residual stream) plus a per-row offset N(0, 0.3^2), gamma = 1 + 0.1 N, beta = 2 + 0.5 N -> (x, g, b).
    The offset in beta is a condition of the check, not of the kernel: ln_f32_part has an ABSOLUTE term (the mean's error times rstd |gamma|,
    about 57 u) that does not shrink with |y|, so with beta around 0 the outputs near zero -- whose fp16 remainders are a few hundred u -- put
    13 % of the codes in doubt (cap 10 %); with |y| around 2 it is 7 % (tests/test_mx4_ref_host.py holds every case to the caps)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, D), generator=gen) * 3 + 0.3 * torch.randn((rows, 1), generator=gen)
    return x, 1 + 0.1 * torch.randn((D,), generator=gen), 2 + 0.5 * torch.randn((D,), generator=gen)


def gemm_gauss(M, N, K, seed, dtype, kind):
    """v ~ N(0, 1) fp32 [M][K] (hi = op16(v), lo = op16(v - hi): the operand pair the quantisers take), W ~ N(0, s^2) in `dtype`, bias ~ N(1, 1)
    for gelu / qgelu -> dict(hi, lo, w, bias) (fp32 holders of 16-bit values). The bias is centred at 1 as a condition of the check: e_gelu is
    relative to |x|, not to gelu(x), so in the negative tail (gelu -> 0) the bound exceeds the fp16 remainder; with a bias around 0 that
    puts 11.7 % of the fp16 codes in doubt (cap 10 %), around 1 it is 5.6 % (tests/test_mx4_ref_host.py holds every case to the caps)."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn((M, K), generator=gen)
    w = (torch.randn((N, K), generator=gen) * (0.05 if kind == "swiglu" else 0.03)).to(torch.bfloat16).to(dtype).float()
    bias = None if kind == "swiglu" else 1 + torch.randn((N,), generator=gen)
    hi = G.rne_op(v, dtype).float()
    lo = G.rne_op(v - hi, dtype).float()
    return dict(hi=hi, lo=lo, w=w, bias=bias)


def gemm_gauss_pre32(p):
    """the fp32 pre-activations of gemm_gauss' operands as a host stand-in for the kernel's accumulators: both products in fp64, one rounding"""
    y = p["hi"].double() @ p["w"].double().t() + O.mx4_quant(p["lo"], BLOCK)[0].double() @ O.mx4_quant(p["w"], None)[0].double().t()
    return (y if p["bias"] is None else y + p["bias"].double()).float()


# ---- float32 emulations of the producers (and of the faults the checks must catch) -------------------------------------------------------------
FAULTS = ("exp+1", "halfmax", "ties_away", "nibble", "scale_index", "kb_shift", "stale_group", "idx_ignored")


def _round_away(t):
    a = t.abs()
    q = torch.where(a < 2.0, torch.floor(a * 2.0 + 0.5) * 0.5, torch.where(a < 4.0, torch.floor(a + 0.5), torch.floor(a * 0.5 + 0.5) * 2.0))
    return torch.copysign(q.clamp(max=6.0), t)


def emit_image(v32, dtype, fault=None, wrong=None, pad=0):
    """what a producer holding the fp32 values v32 [M][K] stores -> (y, codes int [M][K], scale array uint8). Faults: 'exp+1' the stored
    exponent of one block one too high; 'halfmax' the block maximum over the first 16 values only (the others clip at 6); 'ties_away';
    'nibble' the two codes of a byte exchanged; 'scale_index' m % 16 <-> (m % 64) / 16 in the scale array; 'kb_shift' the exponent of block kb
    stored at kb + 1; 'stale_group' the image of the last 64-row group never written; 'idx_ignored' the image taken from `wrong` (the
    fp32 values of the row the gather should not have read), y from v32."""
    v32 = torch.as_tensor(v32, dtype=torch.float32)
    M, K = v32.shape
    y = G.rne_op(v32, dtype)
    lo = v32 - y.float()
    if fault == "idx_ignored":
        wrong = torch.as_tensor(wrong, dtype=torch.float32)
        lo = wrong - G.rne_op(wrong, dtype).float()
    xb = lo.view(M, K // BLOCK, BLOCK)
    e = O.mx4_exponent((xb[..., :16] if fault == "halfmax" else xb).abs().amax(-1))
    t = xb / torch.ldexp(torch.ones_like(e, dtype=torch.float32), e).unsqueeze(-1)
    q = _round_away(t) if fault == "ties_away" else O.mx4_round(t)
    codes = O.mx4_codes(q.reshape(M, K))
    eb = e + 127
    if fault == "nibble":
        codes = codes.view(M, K // 2, 2).flip(-1).reshape(M, K)
    elif fault == "exp+1":
        eb[M // 2, (K // BLOCK) // 2] += 1
    elif fault == "kb_shift":
        eb = eb.roll(1, dims=1)
    elif fault == "stale_group":
        m0 = (M - 1) // 64 * 64
        codes[m0:] = torch.tensor([FILL & 15, FILL >> 4]).repeat(K // 2)
        eb[m0:] = FILL
    elif fault not in (None, "halfmax", "ties_away", "scale_index", "idx_ignored"):
        raise ValueError(fault)
    return y, codes, aexp_pack(eb, K, fill=FILL, pad=pad, swapped=fault == "scale_index")


def _lane_sums8(t):
    """t float32 [R][D] -> [R]: lane l adds the eight terms of its chunks (columns 8 (l + 64 i) .. + 7) serially, then the tree over 64 lanes"""
    R, D = t.shape
    nch = -(-D // 512)
    p = np.zeros((R, nch * 512), F32)
    p[:, :D] = t
    p = p.reshape(R, nch, 64, 8)
    s = np.zeros((R, 64), F32)
    for i in range(nch):
        for r in range(8):
            s = s + p[:, i, :, r]
    return NR._tree(s)


def rms_mx_f32(x, g, eps, dtype, idx=None, fault=None):
    """vt_rmsnorm_mx in float32 -> emit_image of (x[idx] * rstd) * g ('idx_ignored': the image of row r of x instead of row idx[r])"""
    x, g = np.asarray(x, F32), np.asarray(g, F32)

    def val(rows):
        xr = x[rows]
        rstd = NR._rsqrt32(_lane_sums8(xr * xr) / F32(x.shape[1]) + F32(eps))
        return xr * rstd[:, None] * g

    rows = np.arange(x.shape[0]) if idx is None else np.asarray(idx)
    return emit_image(val(rows), dtype, fault, wrong=val(np.arange(len(rows))) if fault == "idx_ignored" else None)


def ln_mx_f32(x, g, b, eps, dtype, fault=None):
    """vt_layernorm_mx in float32 (two passes over the row held in registers)"""
    x, g, b = np.asarray(x, F32), np.asarray(g, F32), np.asarray(b, F32)
    D = F32(x.shape[1])
    d = x - (NR._lane_sums(x, 64) / D)[:, None]
    rstd = NR._rsqrt32(NR._lane_sums(d * d, 64) / D + F32(eps))
    return emit_image(d * rstd[:, None] * g + b, dtype, fault)


def act_mx_f32(pre32, kind, dtype, fault=None):
    """an operand-out epilogue in float32 on the fp32 pre-activations (gemm_ref's restatements of vt_gelu_erf / vt_quick_gelu / vt_silu). The
    epilogues write whole exponent dwords: the rows past M of the last group hold whatever their accumulators gave (taken as FILL here)."""
    pre32 = np.asarray(pre32, F32)
    if kind == "swiglu":
        g, u = G.swiglu_split(torch.from_numpy(pre32))
        v = G.silu_f32(g.numpy()) * u.numpy()
    else:
        v = ACT_F32[kind](pre32)
    return emit_image(v, dtype, fault, pad=FILL)
