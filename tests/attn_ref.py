"""Host restatement of the decode attention kernels (vitron_amd/csrc/vt_attn.hip attn_decode_fused_kernel, attn_decode_kernel +
attn_decode_combine_kernel, whose arithmetic is the shared bodies of vitron_amd/csrc/vt_attn_decode.h with the 16-bit page format;
include/vitron_hip.h vt_attn_decode_fused / vt_attn_decode): the paged K / V^T layout (pack_pages /
unpack_pages, written here without vt_kv_tiles so that a layout slip in that kernel cannot hide a matching one in the decode kernels),
the kernels' half-split rotary embedding rounded exactly as they round it (rope_ref), and fp64 single-query attention with a per-element
error limit for the kernels' fp32 arithmetic (decode_ref / decode_bound). The prefill kernels (flash_attn_kernel, vt_attn_w4.hip
flash_attn_w4_kernel; vt_flash_attn) read the same pages: prefill_ref / prefill_bound restate them the same way. Plain torch, no kernel
of the project: the functions run on the device of their arguments (the CPU in the host tests)."""
import math

import numpy as np
import torch

from tests.nf4_ref import U32, half_ulp

PAGE = 64                       # keys per K / V^T tile
LOG2E = 1.4426950408889634
EXP2_REL = 2.0 ** -22           # v_exp_f32 (fast_exp2): 1 ulp per the CDNA3/CDNA4 ISA guides' transcendental accuracy; taken as 2 ulp
FMT = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def to_op(x, dtype) -> torch.Tensor:
    """fp32 / fp64 values -> the operand dtype, round to nearest even (fp16: saturating at +-65504, as pack_op2 / f32_to_op clamp first).
    The float64 argument is first rounded to fp32, as the kernels hold it."""
    x = torch.as_tensor(x).to(torch.float32)
    if dtype == torch.float16:
        x = x.clamp(-65504.0, 65504.0)
    return x.to(dtype)


def to_f16_page(v) -> torch.Tensor:
    """operand values -> the fp16 the V^T pages hold: exact in fp16's normal range, RNE below it, saturating at +-65504."""
    return torch.as_tensor(v).to(torch.float32).clamp(-65504.0, 65504.0).to(torch.float16)


def pack_pages(k, v, table, heads: int, hd: int, dtype, npages: int = None, fill: float = 0.0, out=None):
    """K and V^T pages of ONE sequence: k, v [L][heads][hd] (any float; k is rounded to `dtype`, v to the fp16 page format), table =
    its page indices (ceil(L / 64) of them). Tile i of head h starts at (table[i] * heads + h) * 64 * hd; K is [64 keys][hd] in the
    operand dtype, V^T is [hd][64 keys] in fp16; rows / columns past L are zero. Returns flat (k_pages `dtype`, vt_pages fp16) of
    npages (default max(table) + 1) pages, pages outside `table` holding `fill` -- or writes into out = (k_pages, vt_pages)."""
    k, v = torch.as_tensor(k), torch.as_tensor(v)
    L = k.shape[0]
    table = torch.as_tensor(table, dtype=torch.long).reshape(-1)
    nt = (L + PAGE - 1) // PAGE
    assert table.numel() == nt and k.shape == (L, heads, hd) and v.shape == (L, heads, hd)
    if out is None:
        n = int(table.max()) + 1 if npages is None else npages
        out = (torch.full((n * heads * PAGE * hd,), fill, dtype=dtype), torch.full((n * heads * PAGE * hd,), fill, dtype=torch.float16))
    kp, vp = out
    kx = torch.zeros((nt * PAGE, heads, hd), dtype=dtype)
    kx[:L] = to_op(k, dtype)
    vx = torch.zeros((nt * PAGE, heads, hd), dtype=torch.float16)
    vx[:L] = to_f16_page(v)
    kp.view(-1, heads, PAGE, hd)[table] = kx.view(nt, PAGE, heads, hd).permute(0, 2, 1, 3)
    vp.view(-1, heads, hd, PAGE)[table] = vx.view(nt, PAGE, heads, hd).permute(0, 2, 3, 1)
    return kp, vp


def unpack_pages(k_pages, vt_pages, table, L: int, heads: int, hd: int):
    """Inverse of pack_pages: (k [L][heads][hd] in the K pages' dtype, v [L][heads][hd] fp16)."""
    table = torch.as_tensor(table, dtype=torch.long).reshape(-1)
    nt = table.numel()
    k = torch.as_tensor(k_pages).view(-1, heads, PAGE, hd)[table].permute(0, 2, 1, 3).reshape(nt * PAGE, heads, hd)
    v = torch.as_tensor(vt_pages).view(-1, heads, hd, PAGE)[table].permute(0, 3, 1, 2).reshape(nt * PAGE, heads, hd)
    return k[:L], v[:L]


def fma32(a, b, c) -> np.ndarray:
    """fp32 fmaf(a, b, c) of fp32 values, without math.fma: a * b is exact in fp64 (2 x 24 bits); the sum a * b + c is taken in fp64
    rounded to ODD (TwoSum gives the exact remainder; an inexact sum whose last bit is even moves one fp64 ulp towards the exact value),
    and a round-to-odd result with 53 >= 24 + 2 bits rounds to fp32 exactly as the exact sum would (no double-rounding error)."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bp = s - c
    err = (p - bp) + (c - (s - bp))
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def rope_ref(x, cos, sin, pos, dtype) -> torch.Tensor:
    """The kernels' half-split rotary embedding (vt_common.h rope_lo / rope_hi) of operand values x [n][..][hd] at positions pos [n]
    (tables cos / sin fp32 [P][hd / 2]): lo = fmaf(a, c, -(b * s)), hi = fmaf(b, c, a * s) in fp32, each rounded once to `dtype`."""
    x = torch.as_tensor(x).to(torch.float32).numpy()
    h = x.shape[-1] // 2
    pos = np.asarray(pos, np.int64)
    shape = (pos.size,) + (1,) * (x.ndim - 2) + (h,)
    c = np.asarray(cos, np.float32)[pos].reshape(shape)
    s = np.asarray(sin, np.float32)[pos].reshape(shape)
    a, b = x[..., :h], x[..., h:]
    lo = fma32(a, c, -(b * s))             # b * s: an fp32 product, rounded, as the kernel forms it
    hi = fma32(b, c, a * s)
    return to_op(torch.from_numpy(np.concatenate([lo, hi], axis=-1)), dtype)


def decode_ref(q, k, v, scale: float) -> torch.Tensor:
    """fp64 single-query attention of one sequence: q [heads][hd], k / v [L][heads][hd] -- the exact operand values the kernel sees
    (q and k rotated and rounded to the operand, v as the fp16 of the pages). Returns [heads][hd] float64."""
    q, k, v = (torch.as_tensor(x).to(torch.float64) for x in (q, k, v))
    s = torch.einsum("hd,lhd->hl", q, k) * scale
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hl,lhd->hd", p, v)


def decode_bound(q, k, v, scale: float, store: str, exact_scores: bool = False) -> torch.Tensor:
    """Per-element limit of |got - decode_ref(q, k, v, scale)| for either decode kernel on the same operands; store = 'bf16' / 'fp16'
    (the output's format). u = 2^-24, t_j = s_j * scale * log2(e) the exact score of key j in log2 units, p_j its fp64 softmax weight,
    o the fp64 output, T = ceil(ntiles / 4) the most tiles one wave accumulates in either kernel (fused: ntiles / 8; split: 1 until
    the split count is clamped at 32, then ntiles / 128). The sum of:
    * scores (fp32): products of two 16-bit values are exact, each lane chains 8 fmaf and the CH <= 16 lanes of a key meet in <= 4 adds,
      so |ds_j| <= (hd + 16) u sum_d |q_d k_jd| in any order (dropped when exact_scores: integer operands, every partial sum < 2^24).
      Then t_j = fl(s_j * sl2): + u |t_j|; sl2 = fl(fl(scale) * fl(log2 e)) is off by <= 3u relatively, a common factor that only
      moves the weights through t_j - t_max; the subtraction t_j - m and the running-max differences of the alpha rescales are
      <= t_max - t_j in sum and each rounds once: together <= 6u (t_max - t_j). dt_j = sl2 (hd + 16) u sum|q k_j| + u |t_j| + 6u (t_max - t_j).
    * exp2: v_exp_f32 has 1 ulp (2^-23) relative error (ISA guide); EXP2_REL takes 2 ulp. Key j's weight passes through its own exp2,
      <= T - 1 later per-tile alpha rescales, the wave combine and the split combine: <= (T + 3) evaluations.
      The relative weight error is d_j = 2^dt_j (1 + (T + 3) EXP2_REL) - 1, and sum p_j (1 + d_j) v_j / sum p_j (1 + d_j) - o is at
      most W = sum_j p_j d_j |v_j - o| / (1 - max d).
    * accumulation (fp32): sum p v and sum p each pass through <= 9T lane operations (8 fmaf and one alpha product per tile), the 8-lane
      and 64-lane reductions, <= 8 wave-combine and <= 32 split-combine products and adds: n = 9T + 96 roundings, a relative error
      <= n u on sum p|v| and on l, so + 1.01 n u (sum p |v| + |o| + W).
    * the final division o / l (fused) or o * (1 / l) (split): + 2u |o|.
    * flushes: v_exp_f32 flushes results below 2^-126 to zero, and the largest weight is 1: + L 2^-125 (max |v| + |o|).
    * the store: half an ulp of `store` at |o| + the sum above."""
    q, k, v = (torch.as_tensor(x).to(torch.float64) for x in (q, k, v))
    L, heads, hd = k.shape
    ntiles = (L + PAGE - 1) // PAGE
    T = (ntiles + 3) // 4
    sl2 = scale * LOG2E
    s = torch.einsum("hd,lhd->hl", q, k)
    t = s * sl2
    tmax = t.max(dim=-1, keepdim=True).values
    p = torch.softmax(s * scale, dim=-1)
    o = torch.einsum("hl,lhd->hd", p, v)
    dt = U32 * t.abs() + 6 * U32 * (tmax - t)
    if not exact_scores:
        dt = dt + sl2 * (hd + 16) * U32 * torch.einsum("hd,lhd->hl", q.abs(), k.abs())
    d = torch.exp2(dt) * (1 + (T + 3) * EXP2_REL) - 1
    vo = (v.permute(1, 0, 2) - o[:, None, :]).abs()                      # [heads][L][hd]
    w = torch.einsum("hl,hld->hd", p * d, vo) / (1 - d.max(dim=-1, keepdim=True).values)
    n = 9 * T + 96
    pv = torch.einsum("hl,lhd->hd", p, v.abs())
    e = w + 1.01 * n * U32 * (pv + o.abs() + w) + 2 * U32 * o.abs()
    e = e + L * 2.0 ** -125 * (v.abs().amax(dim=0) + o.abs())
    return e + torch.from_numpy(half_ulp((o.abs() + e).numpy(), store))


# ---- prefill ------------------------------------------------------------------------------------------------------------------------
P_BIAS = 7.0                    # vt_attn.hip P_BIAS / vt_attn_w4.hip W4A_BIAS: the softmax weights are 2^(t - m_run + 7)
RESCALE_THR = 8.0               # RESCALE_THR / W4A_THR: m_run only moves when a tile's maximum exceeds it by more than this


def half_ulp_t(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """tests.nf4_ref.half_ulp in torch (fp64, on x's device)"""
    p = {"bf16": 8, "fp16": 11}[fmt]
    ex = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    if fmt == "fp16":
        ex = ex.clamp_min(-14.0)
    return torch.exp2(ex - (p - 1)) / 2


W_ELEMS = 1 << 24               # prefill_bound's largest fp64 temporary, in elements (a test on a GPU may raise it)


def _prefill(q, k, v, scale, past, causal, store, rows, want_bound):
    q, k, v = (torch.as_tensor(x).to(torch.float64) for x in (q, k, v))
    dev = q.device
    Lq, heads, hd = q.shape
    Lk = k.shape[0]
    rows = torch.arange(Lq, device=dev) if rows is None else torch.as_tensor(rows, dtype=torch.long, device=dev)
    assert rows.numel() == Lq and k.shape == v.shape == (Lk, heads, hd) and int(rows.max()) + past < Lk
    kh, vh = k.permute(1, 0, 2), v.permute(1, 0, 2)                       # [heads][Lk][hd]
    sl2 = scale * LOG2E
    ref = torch.empty((heads, Lq, hd), dtype=torch.float64, device=dev)
    bound = torch.empty_like(ref) if want_bound else None
    vmax = vh.abs().amax(dim=1, keepdim=True)                             # [heads][1][hd]
    R = 64
    for r0 in range(0, Lq, R):
        lim = (past + rows[r0:r0 + R]) if causal else torch.full((min(R, Lq - r0),), Lk - 1, device=dev)   # last visible key
        K = int(lim.max()) + 1
        qc = q[r0:r0 + R].permute(1, 0, 2)                                # [heads][R][hd]
        vis = torch.arange(K, device=dev)[None, :] <= lim[:, None]        # [R][K]
        t = (qc @ kh[:, :K].transpose(1, 2) * sl2).masked_fill(~vis, -math.inf)
        tmax = t.amax(dim=-1, keepdim=True)
        p = torch.exp2(t - tmax)
        p = p / p.sum(dim=-1, keepdim=True)
        o = p @ vh[:, :K]                                                 # [heads][R][hd]
        ref[:, r0:r0 + R] = o
        if not want_bound:
            continue
        n = vis.sum(dim=1).to(torch.float64)[None, :, None]               # visible keys        [1][R][1]
        T = (torch.div(lim, PAGE, rounding_mode="floor") + 1).to(torch.float64)[None, :, None]
        sabs = qc.abs() @ kh[:, :K].abs().transpose(1, 2)
        tf = t.masked_fill(~vis, 0.0)
        dt = U32 * (sl2 * (hd + 16) * sabs + 2 * tf.abs() + 2 * tmax.abs() + 6 * (tmax - tf) + 64.0)
        d = (torch.exp2(dt) * (1 + (2 * T + 1) * EXP2_REL) - 1).masked_fill(~vis, 0.0)
        dmax = d.amax(dim=-1, keepdim=True)
        pd = p * d
        W = torch.zeros_like(o)
        kc = max(1, W_ELEMS // (heads * qc.shape[1] * hd))
        for j0 in range(0, K, kc):
            W += torch.einsum("hrj,hrjd->hrd", pd[:, :, j0:j0 + kc], (vh[:, None, j0:min(j0 + kc, K)] - o[:, :, None]).abs())
        W = W / (1 - dmax)
        pv = p @ vh[:, :K].abs()
        e = W + 2.0 ** -11 * (1 + dmax) * pv + 1.01 * (n + 2 * T + 16) * U32 * (pv + o.abs() + W) + 2 * U32 * o.abs()
        e = e + n * 2.0 ** -32 * (vmax + o.abs())
        bound[:, r0:r0 + R] = e + half_ulp_t(o.abs() + e, store)
    return ref.permute(1, 0, 2), (bound.permute(1, 0, 2) if want_bound else None)


def prefill_ref(q, k, v, scale: float, past: int, causal: bool, rows=None) -> torch.Tensor:
    """fp64 attention of one sequence: q [Lq][heads][hd], k / v [past + Lq][heads][hd] -- the exact operand values the kernel sees (q and
    k rotated and rounded to the operand, v as the fp16 of the pages). Query i sees keys <= past + i when causal, all kv_len keys
    otherwise. rows (optional): q holds only these query indices of the sequence (a subset of a long prefill). [Lq][heads][hd] float64."""
    return _prefill(q, k, v, scale, past, causal, None, rows, False)[0]


def prefill_bound(q, k, v, scale: float, past: int, causal: bool, store: str, rows=None) -> torch.Tensor:
    """Per-element limit of |got - prefill_ref(...)| for flash_attn_kernel<HD, CAUSAL, 4, 2> (vt_attn.hip) and flash_attn_w4_kernel
    (vt_attn_w4.hip) on the same operands; store = 'bf16' / 'fp16' (the output's format). u = 2^-24; t_j = s_j * scale * log2(e) the
    exact score of key j in log2 units, p_j its fp64 softmax weight over the row's n visible keys, o the fp64 output, T the row's count
    of 64-key tiles (one wave walks all of them: nothing is combined across waves). The kernels keep a running maximum m_run per row
    that only moves when some row of the wave sees a tile (vt_attn.hip) or 32-key sub tile (w4) maximum more than RESCALE_THR = 8 above
    it ("deferred rescale": ballot, then m_new = max(m_run, m_tile), l and O scaled by alpha = exp2(m_run - m_new)), and form the weight
    of key j as e_j = exp2(fma(s_j, sl2, P_BIAS - m_run)), P_BIAS = 7. The sum of:
    * weights (fp32), as a relative error d_j of e_j against the other keys of the row:
      - scores: v_mfma_f32_32x32x16 on 16-bit operands, products exact, fp32 accumulation over hd terms, one rounding per product taken
        as the worst case: |ds_j| <= (hd + 16) u sum_d |q_d k_jd| (the + 16 as in decode_bound);
      - the fma rounds once, at |y| = |t_j - m_run + 7| <= (t_max - t_j) + 15; its addend fl(7 - m_run) rounds at |m_run| + 7 <=
        |t_j| + |t_max| + 15 (m_run lies between t_j - 8 and t_max); sl2 = fl(fl(scale) * fl(log2 e)) is off by <= 3u relatively, a
        common factor that only acts through t_j - t_max; the alpha of every later rescale rounds its difference once, and the
        differences add up to <= t_max - (t_j - 8). The value of m_run itself (fl(max * sl2)) enters numerator and row sum alike and
        cancels. Together dt_j <= u (sl2 (hd + 16) sum|q k_j| + 2|t_j| + 2|t_max| + 6 (t_max - t_j) + 64);
      - exp2: v_exp_f32, EXP2_REL (2 ulp) per evaluation: the key's own and one alpha per later softmax step, of which the w4 kernel has
        two per tile: <= 2T + 1. d_j = 2^dt_j (1 + (2T + 1) EXP2_REL) - 1.
      The row sum l adds the same fp32 e_j, so these errors act on numerator and denominator alike:
      |sum p_j (1 + d_j) v_j / sum p_j (1 + d_j) - o| <= W = sum_j p_j d_j |v_j - o| / (1 - max d).
    * the fp16 weights: e_j reaches the P.V MFMA through pack_f16x2 (round to nearest even, relative 2^-11 in fp16's normal range) while
      l adds the unrounded value -- an error of the numerator alone: 2^-11 (1 + max d) sum_j p_j |v_j|. (Not |v_j - o|: nothing cancels.)
    * fp16's range: e_j <= 2^(8 + 7) never overflows; below 2^-14 the rounding is absolute, <= 2^-25 per key, against a row sum of at
      least 2^7 (the largest weight is >= 2^(7 - 0): m_run never exceeds the true maximum); v_exp_f32's own flush below 2^-126 is far
      smaller: + n 2^-32 (max|v| + |o|).
    * accumulation (fp32): O gathers n products in the MFMA's accumulator (fp16 x fp16 products are exact in fp32; one rounding per
      product as the worst case) and <= 2T alpha products; l gathers n terms in lane sums, the two half-waves' sum and <= 2T alpha
      products: a relative error <= (n + 2T + 16) u on sum p |v| and on l: + 1.01 (n + 2T + 16) u (sum p |v| + |o| + W).
    * the epilogue o * (1 / l): + 2u |o|.
    * the store: half an ulp of `store` at |o| + the sum above."""
    return _prefill(q, k, v, scale, past, causal, store, rows, True)[1]


def prefill_ref_and_bound(q, k, v, scale: float, past: int, causal: bool, store: str, rows=None):
    """(prefill_ref, prefill_bound) in one pass"""
    return _prefill(q, k, v, scale, past, causal, store, rows, True)
