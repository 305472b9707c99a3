"""numpy restatement of the NF4 format of load_4bit (bitsandbytes load_in_4bit, bnb_4bit_quant_type="nf4"; include/vitron_hip.h
vt_nf4_quant): the weight as fp16, blocks of 64 consecutive elements, absmax = fp32 max |x|, x * (1.0f / absmax) in fp32 to the code whose
fp32 midpoint (bitsandbytes dQuantizeNF4) it lies strictly above, element 2j in the high nibble, dequantised = fp32(code) * absmax."""
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
