"""Host restatement of the FP8 (OCP e4m3fn) paged KV cache (vitron_amd/csrc/vt_kv8.hip, its decode kernels being the shared bodies of
vitron_amd/csrc/vt_attn_decode.h with the e4m3 page format; include/vitron_hip.h "FP8 KV CACHE"): the
element format from its definition (E4M3 table), the canonical byte quant(x) = e4m3_rne(clamp(x, -448, +448)) and its exact inverse,
the page layout (pack_pages8 / unpack_pages8 = the 16-bit layouts of tests/attn_ref.py with 1-byte elements), and the fp64 reference +
per-element error limit of the fp8 decode kernels (decode_ref / decode_bound over the DEQUANTISED pages: the quantisation itself is
not part of the kernels' error). CPU only."""
import numpy as np
import torch

from tests import attn_ref as R
from tests.nf4_ref import U32, half_ulp

PAGE = R.PAGE
E4M3_MAX = 448.0


def _e4m3_value(code: int) -> float:
    """One e4m3fn code from the format's definition: 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 0 = subnormal (m / 8 * 2^-6);
    no infinity; exponent 15 with mantissa 7 is NaN, every other exponent-15 code is a normal number (up to 1.75 * 2^8 = 448)."""
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return float("nan")
    v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


E4M3 = np.array([_e4m3_value(c) for c in range(256)], np.float64)          # code -> value (0x7f, 0xff: NaN)
FINITE_CODES = np.array([c for c in range(256) if c & 0x7f != 0x7f], np.uint8)   # the 254 finite codes


def quant_table(x) -> np.ndarray:
    """quant() restated from the table alone (the oracle of quant in the host tests): clamp to +-448, the nearest non-negative code value,
    ties to the even code, the sign bit kept (-0 and negative values that round to zero give 0x80); NaN -> 0x7f | sign."""
    x = np.asarray(x, np.float64)
    pos = E4M3[:127]                                                         # codes 0x00 .. 0x7e, ascending
    a = np.minimum(np.abs(x), E4M3_MAX)
    a = np.where(np.isnan(a), 0.0, a)
    hi = np.clip(np.searchsorted(pos, a, side="left"), 0, 126)               # first code value >= a
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - pos[lo], pos[hi] - a
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(np.isnan(x), 0x7f, code).astype(np.uint8)
    return code | (np.signbit(x).astype(np.uint8) << 7)


def quant(x) -> torch.Tensor:
    """The canonical byte of 16-bit cache values x (any float dtype): e4m3_rne(clamp(x, -448, +448)) as uint8 -- torch's float8_e4m3fn
    conversion behind the clamp (without it an overflow becomes NaN: e4m3fn has no infinity). NaN stays NaN."""
    x = torch.as_tensor(x).to(torch.float32)
    return x.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def dequant(b, dtype=torch.float32) -> torch.Tensor:
    """bytes -> values in `dtype` (exact: every finite e4m3 value is a bf16 and an fp16 value)."""
    return torch.as_tensor(b).contiguous().view(torch.float8_e4m3fn).to(torch.float32).to(dtype)


def pack_pages8(k, v, table, heads: int, hd: int, dtype, npages: int = None, fill: int = 0, out=None):
    """attn_ref.pack_pages with 1-byte elements: k is rounded to the operand `dtype`, v to the fp16 page value, then both to their canonical
    bytes. Tile i of head h starts at byte (table[i] * heads + h) * 64 * hd; K is [64 keys][hd], V^T is [hd][64 keys]; rows / columns past
    L are 0x00; pages outside `table` hold `fill`. Returns flat uint8 (k8, vt8)."""
    k, v = torch.as_tensor(k), torch.as_tensor(v)
    L = k.shape[0]
    table = torch.as_tensor(table, dtype=torch.long).reshape(-1)
    nt = (L + PAGE - 1) // PAGE
    assert table.numel() == nt and k.shape == (L, heads, hd) and v.shape == (L, heads, hd)
    if out is None:
        n = int(table.max()) + 1 if npages is None else npages
        out = (torch.full((n * heads * PAGE * hd,), fill, dtype=torch.uint8), torch.full((n * heads * PAGE * hd,), fill, dtype=torch.uint8))
    kp, vp = out
    kx = torch.zeros((nt * PAGE, heads, hd), dtype=torch.uint8)
    kx[:L] = quant(R.to_op(k, dtype))
    vx = torch.zeros((nt * PAGE, heads, hd), dtype=torch.uint8)
    vx[:L] = quant(R.to_f16_page(v))
    kp.view(-1, heads, PAGE, hd)[table] = kx.view(nt, PAGE, heads, hd).permute(0, 2, 1, 3)
    vp.view(-1, heads, hd, PAGE)[table] = vx.view(nt, PAGE, heads, hd).permute(0, 2, 3, 1)
    return kp, vp


def unpack_pages8(k8, vt8, table, L: int, heads: int, hd: int):
    """Inverse of pack_pages8: (k bytes [L][heads][hd], v bytes [L][heads][hd])."""
    return R.unpack_pages(torch.as_tensor(k8), torch.as_tensor(vt8), table, L, heads, hd)


def decode_ref(q, k8, v8, scale: float) -> torch.Tensor:
    """fp64 single-query attention over e4m3 bytes: q [heads][hd] (the rotated, rounded operand values), k8 / v8 uint8 [L][heads][hd]."""
    return R.decode_ref(q, dequant(k8, torch.float64), dequant(v8, torch.float64), scale)


def decode_bound(q, k8, v8, scale: float, store: str, exact_scores: bool = False) -> torch.Tensor:
    """Per-element limit of |got - decode_ref| for attn_decode_kv8_kernel / attn_decode_fused_kv8_kernel: attn_ref.decode_bound's terms with
    the operation counts of the fp8 kernels (vt_attn_decode.h header comments with EPC = 16), every constant as there:
    * scores: the product of an e4m3 value (4 significant bits) and a 16-bit operand value is exact in fp32; a lane chains 16 fmaf (one
      16-byte chunk = 16 elements of a key) and the hd / 16 <= 8 lanes of a key meet in <= 3 adds -- <= 19 roundings on any path, inside the
      (hd + 16) u sum |q k| of the 16-bit bound, which holds for any summation order. Unchanged.
    * exp2 and weights: unchanged -- the waves own the same tiles (fused: w, w + 8, ...; split: 4 waves x <= 32 splits), T = ceil(ntiles / 4).
    * accumulation: a V^T row is 64 bytes = 4 lanes x 16 keys, so an accumulator passes through 17 roundings per tile (the alpha product and
      16 fmaf; the 16-bit kernels: 9), then the 4-lane reduction (2 adds; 16-bit: 3), the new token's fmaf (fused), <= 8 wave-combine and <= 32
      split-combine products and adds; l passes through 8 per tile. n = 17 T + 96 (16-bit: 9 T + 96; the constant covers 2 + 1 + 6 + 80).
    * division, flushes, store: unchanged."""
    q = torch.as_tensor(q).to(torch.float64)
    k, v = dequant(k8, torch.float64), dequant(v8, torch.float64)
    L, heads, hd = k.shape
    ntiles = (L + PAGE - 1) // PAGE
    T = (ntiles + 3) // 4
    sl2 = scale * R.LOG2E
    s = torch.einsum("hd,lhd->hl", q, k)
    t = s * sl2
    tmax = t.max(dim=-1, keepdim=True).values
    p = torch.softmax(s * scale, dim=-1)
    o = torch.einsum("hl,lhd->hd", p, v)
    dt = U32 * t.abs() + 6 * U32 * (tmax - t)
    if not exact_scores:
        dt = dt + sl2 * (hd + 16) * U32 * torch.einsum("hd,lhd->hl", q.abs(), k.abs())
    d = torch.exp2(dt) * (1 + (T + 3) * R.EXP2_REL) - 1
    vo = (v.permute(1, 0, 2) - o[:, None, :]).abs()
    w = torch.einsum("hl,hld->hd", p * d, vo) / (1 - d.max(dim=-1, keepdim=True).values)
    n = 17 * T + 96
    pv = torch.einsum("hl,lhd->hd", p, v.abs())
    e = w + 1.01 * n * U32 * (pv + o.abs() + w) + 2 * U32 * o.abs()
    e = e + L * 2.0 ** -125 * (v.abs().amax(dim=0) + o.abs())
    return e + torch.from_numpy(half_ulp((o.abs() + e).numpy(), store))


def attend_f32(q, k8, v8, scale: float, drop=None, extra_pad: int = 0, swap_tile=None) -> torch.Tensor:
    """A plain fp32 single-query attention over e4m3-valued operands, tile by tile with an online softmax (what the kernels compute, in
    numpy): the subject of the host test of decode_bound. Mutants: drop = a key index left out; extra_pad = padding keys (zero rows)
    counted as valid; swap_tile = (a, b): tile a's keys scored against tile b's K rows."""
    q = torch.as_tensor(q).to(torch.float32).numpy()
    k = dequant(k8, torch.float32).numpy().copy()
    v = dequant(v8, torch.float32).numpy().copy()
    L, heads, hd = k.shape
    nt = (L + PAGE - 1) // PAGE
    kk = np.zeros((nt * PAGE, heads, hd), np.float32)
    vv = np.zeros((nt * PAGE, heads, hd), np.float32)
    kk[:L], vv[:L] = k, v
    valid = np.arange(nt * PAGE) < L + extra_pad
    if drop is not None:
        valid[drop] = False
    if swap_tile is not None:
        a, b = swap_tile
        kk[a * PAGE:(a + 1) * PAGE] = kk[b * PAGE:(b + 1) * PAGE].copy()
    sl2 = np.float32(scale * R.LOG2E)
    out = np.zeros((heads, hd), np.float32)
    for h in range(heads):
        m, l, acc = np.float32(-np.inf), np.float32(0), np.zeros(hd, np.float32)
        for t in range(nt):
            sl = slice(t * PAGE, (t + 1) * PAGE)
            s = (kk[sl, h] @ q[h]).astype(np.float32) * sl2
            s = np.where(valid[sl], s, -np.inf).astype(np.float32)
            mn = max(m, s.max())
            if mn == -np.inf:
                continue
            alpha = np.exp2(np.float32(m - mn)).astype(np.float32)
            p = np.exp2(s - mn).astype(np.float32)
            l = np.float32(l * alpha + p.sum(dtype=np.float32))
            acc = (acc * alpha + p @ vv[sl, h]).astype(np.float32)
            m = mn
        out[h] = acc / l
    return torch.from_numpy(out)
