"""numpy restatement of the NF4 format of load_4bit (bitsandbytes load_in_4bit, bnb_4bit_quant_type="nf4"; include/vitron_hip.h
vt_nf4_quant): the weight as fp16, blocks of 64 consecutive elements, absmax = fp32 max |x|, x * (1.0f / absmax) in fp32 to the code whose
fp32 midpoint (bitsandbytes dQuantizeNF4) it lies strictly above, element 2j in the high nibble, dequantised = fp32(code) * absmax.
Also the GPU GEMM tests' input and limit: random_nf4 (code bytes and block scales no quantiser produced) and gemm_ref / gemm_bound (fp64
result and per-element error limit of vt_gemm_nf4 on exact operand values)."""
import numpy as np

CODEBOOK = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
                     -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
                     0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0], dtype=np.float32)
# dQuantizeNF4's thresholds as its source spells them (ascending here): code = how many of them the value is strictly above
MIDPOINTS = np.array([-0.8480964004993439, -0.6106329262256622, -0.4599952697753906, -0.33967943489551544, -0.23460740596055984,
                      -0.13791173323988914, -0.045525018125772476, 0.03979014977812767, 0.1202552504837513, 0.2035212516784668,
                      0.2920137718319893, 0.3893125355243683, 0.5016634166240692, 0.6427869200706482, 0.8614784181118011], dtype=np.float32)
BLOCK = 64


def quantize(w) -> tuple:
    """(codes uint8 [N*K/2], absmax fp32 [N*K/64]) of a [N][K] array (any float dtype: cast to fp16 first, as the 4-bit load does)."""
    x = np.asarray(w).astype(np.float16).astype(np.float32)
    N, K = x.shape
    assert K % BLOCK == 0
    blocks = x.reshape(-1, BLOCK)
    absmax = np.abs(blocks).max(axis=1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):      # all-zero blocks: 0 * inf, overwritten with code 7 below
        inv = (np.float32(1.0) / absmax).astype(np.float32)
        y = (blocks * inv[:, None]).astype(np.float32)
    codes = np.zeros(blocks.shape, dtype=np.uint8)
    for t in MIDPOINTS:
        codes += (y > t).astype(np.uint8)
    codes[absmax == 0] = 7
    flat = codes.reshape(-1)
    packed = ((flat[0::2] << 4) | flat[1::2]).astype(np.uint8)
    return packed, absmax


def unpack(codes) -> np.ndarray:
    """uint8 [n/2] -> code per element [n] (element 2j from the high nibble)."""
    codes = np.asarray(codes, dtype=np.uint8)
    out = np.empty(codes.size * 2, dtype=np.uint8)
    out[0::2] = codes >> 4
    out[1::2] = codes & 15
    return out


def dequantize_f32(codes, absmax, N: int, K: int) -> np.ndarray:
    """fp32 [N][K] = fp32(code) * absmax -- the value the operand format then rounds (op16)."""
    c = CODEBOOK[unpack(codes)].reshape(-1, BLOCK)
    return (c * np.asarray(absmax, dtype=np.float32)[:, None]).astype(np.float32).reshape(N, K)


def random_nf4(N: int, K: int, seed: int, log2_range=(-12, 4)) -> tuple:
    """(codes uint8 [N*K/2], absmax fp32 [N*K/64]) of a random NF4 matrix [N][K] that no quantiser produced: uniformly random code bytes
    (all 256 byte values, so every code in both nibbles), and per 64-block an absmax 2^e * (1 + u), e uniform over the integers
    [log2_range[0], log2_range[1]) and u uniform in [0, 1), rounded to fp16 as a real absmax is (the weight is fp16). Neighbouring blocks,
    rows and K steps differ by up to 2^16 in scale, so reading the wrong block's absmax is an O(1) error in the elements it touches. The
    low end reaches fp16 subnormal weights (2^-12 * 0.0796 < 2^-14)."""
    assert K % BLOCK == 0
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=N * K // 2, dtype=np.uint8)
    nb = N * K // BLOCK
    e = rng.integers(log2_range[0], log2_range[1], size=nb).astype(np.float64)
    absmax = (np.exp2(e) * (1.0 + rng.random(nb))).astype(np.float16).astype(np.float32)
    return codes, absmax


U32 = 2.0 ** -24     # unit roundoff of fp32
_MANT = {"bf16": 8, "fp16": 11}


def half_ulp(x, fmt: str) -> np.ndarray:
    """half a unit in the last place of the 16-bit format `fmt` ('bf16' / 'fp16') at |x| (fp16: subnormal spacing 2^-24 below 2^-14)."""
    p = _MANT[fmt]
    ax = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    ex = np.floor(np.log2(ax))
    if fmt == "fp16":
        ex = np.maximum(ex, -14.0)
    return np.exp2(ex - (p - 1)) / 2


def silu(x):
    x = np.asarray(x, dtype=np.float64)
    return x / (1.0 + np.exp(-np.clip(x, -700, 700)))


def gemm_ref(a, wd, rscale=None, resid=None, swiglu: bool = False, y=None) -> np.ndarray:
    """fp64 epi(rscale[:, None] * (a @ wd^T)) of the exact operand values a [M][K], wd [N][K]: the vt_gemm_nf4 epilogues before their store
    (swiglu: silu(gate) * up on the interleaved layout -- 32-row blocks of 16 gate rows, then their 16 up rows -- [M][N/2]). `y`: a @ wd^T
    in fp64 when the caller has it already."""
    y = np.asarray(a, np.float64) @ np.asarray(wd, np.float64).T if y is None else y
    if rscale is not None:
        y = y * np.asarray(rscale, np.float64)[:, None]
    if swiglu:
        M, N = y.shape
        y4 = y.reshape(M, N // 32, 2, 16)
        y = (silu(y4[:, :, 0]) * y4[:, :, 1]).reshape(M, N // 2)
    if resid is not None:
        y = y + np.asarray(resid, np.float64)
    return y


def gemm_bound(a, wd, K: int, rscale=None, rscale_rel: float = 0.0, resid=None, swiglu: bool = False, store=None, y=None) -> np.ndarray:
    """Per-element limit of |got - gemm_ref(...)| for vt_gemm_nf4 on the same exact operands (same arguments; `y`: a @ wd^T in fp64).
    * Every product of two 16-bit values is exact in fp32; the accumulation (MFMA chains, then the 8-way split-K reduce) adds at most K + 8
      times, so (K + 16) * 2^-24 * sum |a||w| covers it in any order.
    * rscale (folded RMSNorm, consumer side): that bound scales with rscale, and the kernel's own rstd, which it computes from fp32 partial
      sums, is off from the fp64 one by rscale_rel (relative): + rscale_rel * |y|.
    * swiglu: the gate error e_g and the up error e_u carried through silu(g) * u (|silu'| <= 1.1): 1.1 |u| e_g + |silu(g)| e_u + e_g e_u,
      plus the epilogue's own fp32 rounding: __expf(-g) is off by about |g| ulps (its argument x * log2(e) is rounded), the hardware
      reciprocal, the add and the two products by one each: (|g| + 8) * 2^-24 * |silu(g) u|.
    * resid (EPI_F32_RESID): one more fp32 rounding, of the sum.
    * store ('bf16' / 'fp16'): half an output ulp for the 16-bit store."""
    a, wd = np.asarray(a, np.float64), np.asarray(wd, np.float64)
    y = a @ wd.T if y is None else y
    e = (K + 16) * U32 * (np.abs(a) @ np.abs(wd).T)
    if rscale is not None:
        r = np.asarray(rscale, np.float64)[:, None]
        y, e = y * r, e * r
        e = e + rscale_rel * np.abs(y)
    if swiglu:
        M, N = y.shape
        y4, e4 = y.reshape(M, N // 32, 2, 16), e.reshape(M, N // 32, 2, 16)
        g, u, eg, eu = y4[:, :, 0], y4[:, :, 1], e4[:, :, 0], e4[:, :, 1]
        s = silu(g)
        y = (s * u).reshape(M, N // 2)
        e = (1.1 * np.abs(u) * eg + np.abs(s) * eu + eg * eu + (np.abs(g) + 8) * U32 * np.abs(s * u)).reshape(M, N // 2)
    if resid is not None:
        y = y + np.asarray(resid, np.float64)
        e = e + U32 * (np.abs(y) + e)
    if store is not None:
        e = e + half_ulp(np.abs(y) + e, store)
    return e
