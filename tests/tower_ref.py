"""Host restatement of the tower kernels for tests/test_gpu_tower_kernels.py and tests/test_tower_ref_host.py: temporal attention
(vitron_amd/csrc/vt_attn.hip attn_temporal8_kernel, attn_temporal_kernel<T>, attn_temporal_f32_kernel<T>), the ViT embedding assembly +
pre-LayerNorm (vt_vit.hip vit_embed_kernel<NCH>) and the region extractor's pooling launch (vt_region.hip region_pool_kernel: cell mask,
count, masked mean, LocationEncoder layer 0). For each: an fp64 reference, the per-element bound an fp32 implementation of it must meet
(derived below from the kernels' summation chains, DESIGN.md "Tower-kernel pinning"), inputs whose results are exact in fp32 whatever the
summation order, the inputs of the GPU tests (built here so that the host tests judge the same numbers), and float32 emulations of the
kernels with the faults the checks must catch. Plain numpy / torch on the CPU; nothing here calls the library."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

from tests import gemm_ref as G
from tests import norm_ref as NR
from tests.attn_ref import EXP2_REL, U32, fma32
from tests.nf4_ref import half_ulp

F32 = np.float32
HD = 64                          # head dim of the temporal kernels (one lane per dim / eight 16-byte chunks)
FMT = G.FMT


def _half_ulp_t(x64, dtype):
    return torch.from_numpy(half_ulp(torch.as_tensor(x64).numpy(), FMT[dtype]))


# ==== temporal attention ================================================================================================================
# (B, T, N, heads): 15 items for every T (the last workgroup holds 3 waves), two ragged multi-clip shapes, the video tower's width
TEMPORAL_SHAPES = tuple((1, T, 5, 3) for T in range(1, 9)) + ((2, 8, 33, 2), (2, 4, 17, 2), (1, 8, 257, 16))
SCORE_STDS = (1.0, 11.0)
TEMPORAL_FAULTS = ("drop_last", "transpose", "weight", "row_shift", "head")


def split_qkv(qkv, B, T, N, heads):
    """qkv [B*T*N][>= 3 D] (row (b T + t) N + n, columns q | k | v) -> q, k, v [I][T][64], item i = (b N + n) heads + head: the kernels'
    wave index"""
    D = heads * HD
    x = torch.as_tensor(qkv)[:, :3 * D].reshape(B, T, N, 3, heads, HD).permute(3, 0, 2, 4, 1, 5).reshape(3, B * N * heads, T, HD)
    return x[0], x[1], x[2]


def merge_qkv(q, k, v, B, T, N, heads):
    """inverse of split_qkv -> [B*T*N][3 D]"""
    x = torch.stack([torch.as_tensor(t) for t in (q, k, v)]).reshape(3, B, N, heads, T, HD)
    return x.permute(1, 4, 2, 0, 3, 5).reshape(B * T * N, 3 * heads * HD).contiguous()


def merge_out(o, B, T, N, heads):
    """o [I][T][64] -> [B*T*N][D], the layout of the kernels' output"""
    return torch.as_tensor(o).reshape(B, N, heads, T, HD).permute(0, 3, 1, 2, 4).reshape(B * T * N, heads * HD).contiguous()


def temporal_ref(q, k, v):
    """fp64 softmax(q k^T) v per item over the T frames: q, k, v [I][T][64], the exact values the kernel reads (q arrives pre-scaled: no
    scale here) -> [I][T][64] float64"""
    q, k, v = (torch.as_tensor(x).double() for x in (q, k, v))
    p = torch.softmax(torch.einsum("itd,iud->itu", q, k), dim=-1)
    return torch.einsum("itu,iud->itd", p, v)


def temporal_bound(q, k, v, store, prod_round):
    """Per-element limit of |got - temporal_ref(q, k, v)| for the three temporal kernels on the same operands. store: torch.bfloat16 /
    torch.float16 (the output's format) or None (the fp32 value before the store: the pair kernel's test adds its own store term);
    prod_round: roundings of one product q_d k_d (0 for 16-bit operands, whose products are exact in fp32; 1 for the f32 kernel).
    u = 2^-24, s_j the exact score of frame j in a row, x_j = s_max - s_j, p_j its fp64 softmax weight, o the fp64 output. The sum of:
    * scores (fp32): attn_temporal8_kernel chains 64 fmaf, the other two add 64 products in the 6 levels of wave_sum; (1 + u)^n - 1 <=
      1.01 n u up to n = 64 + 1, so in any order |ds_j| <= (64 + prod_round) u sum_d |q_d k_jd| (the 1.01 is carried by the + 4 ds_max below
      and by EXP2_REL's spare ulp: both are orders above it).
    * weights: the kernel forms e_j = __expf(fl(s_j - mx)) with mx the largest COMPUTED score. __expf lowers to v_mul_f32 by fl(log2 e) and
      a bare v_exp_f32 (read from the gfx950 ISA of both operand builds: no range scaling, no denormal fix-up), so the exponent carries
      the rounding of the difference, of the constant and of the product: 3 u |s_j - s_mx|, and |s_j - s_mx| <= x_j + 4 ds_max because
      the computed maximum is within 2 ds_max of the true one. The score error of the maximum itself is common to the row and cancels
      in the normalisation. In natural-log units dx_j = ds_j + 3 u (x_j + 4 ds_max), and the relative weight error is
      d_j = exp(dx_j) (1 + EXP2_REL) - 1 with attn_ref.EXP2_REL = 2 ulp for v_exp_f32 (1 ulp per the ISA guide). Numerator and
      denominator use the same e_j: |sum p_j (1 + d_j) v_j / sum p_j (1 + d_j) - o| <= W = sum_j p_j d_j |v_j - o| / (1 - max d).
    * accumulation (fp32): the denominator passes through T adds (3 shuffle adds at T = 8), the numerator through T fmaf / rounded
      products and adds, and there is one division (p / den at T = 8, acc / den otherwise): <= 2 T + 4 roundings, relative to
      sum p |v| and to the denominator: + 1.01 (2 T + 4) u (sum p |v| + |o| + W) + 2 u |o|.
    * flushes: v_exp_f32 returns zero below 2^-126 while the largest weight is 1: + T 2^-125 (max |v| + |o|).
    * the store: half an ulp of `store` at |o| + the sum above."""
    q, k, v = (torch.as_tensor(x).double() for x in (q, k, v))
    T = q.shape[1]
    s = torch.einsum("itd,iud->itu", q, k)
    ds = (HD + prod_round) * U32 * torch.einsum("itd,iud->itu", q.abs(), k.abs())
    x = s.max(dim=-1, keepdim=True).values - s
    dx = ds + 3 * U32 * (x + 4 * ds.max(dim=-1, keepdim=True).values)
    d = torch.exp(dx) * (1 + EXP2_REL) - 1
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("itu,iud->itd", p, v)
    W = torch.zeros_like(o)
    for j in range(T):                                                    # per frame: no [I][T][T][64] temporary
        W += (p[:, :, j] * d[:, :, j])[:, :, None] * (v[:, None, j, :] - o).abs()
    W = W / (1 - d.max(dim=-1, keepdim=True).values)
    pv = torch.einsum("itu,iud->itd", p, v.abs())
    e = W + 1.01 * (2 * T + 4) * U32 * (pv + o.abs() + W) + 2 * U32 * o.abs()
    e = e + T * 2.0 ** -125 * (v.abs().amax(dim=1, keepdim=True) + o.abs())
    return e if store is None else e + _half_ulp_t(o.abs() + e, store)


def pair_bound(o64, e, hi, dtype):
    """the f32 kernel's (hi, lo): hi + lo against o64 -- the arithmetic bound e + half an ulp of lo's format at |o - hi| (+ e: lo is the
    rounding of the kernel's fp32 value minus hi, and that difference is exact in fp32)"""
    return e + _half_ulp_t((o64 - hi.double()).abs() + e, dtype)


def temporal_kind(T, f32):
    """which summation a launch runs: 'chain' = attn_temporal8_kernel, 'tree' = attn_temporal_kernel<T> / attn_temporal_f32_kernel<T>"""
    return "chain" if T == 8 and not f32 else "tree"


def _tree_last(s):
    """[..][L], L a power of two -> [..]: log2 L levels of additions, partner at distance L / 2 first (wave_sum's order)"""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., :h] + s[..., h:]
    return s[..., 0]


def _tree_adjacent(s):
    """[..][L] -> [..]: partner at distance 1 first (xor-shuffles 1, 2, 4)"""
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def temporal_f32(q, k, v, kind, dtype, heads, fault=None, pair=False):
    """The temporal kernels in numpy float32: q, k, v float32 [I][T][64] -> the output [I][T][64] as the store leaves it (pair: (hi, lo) of
    attn_temporal_f32_kernel). kind 'chain': 64 fmaf per score, P = e / den normalised before the 8 fmaf of the output; 'tree': rounded
    products through wave_sum, den and acc serially, one division at the end. Faults: 'drop_last' frame T - 1 left out of the softmax;
    'transpose' S[t1][t2] <-> S[t2][t1]; 'weight' the weight of (t1, t2) = (0, 0) times 1 + 2^-9 in the numerator; 'row_shift' the output
    of frame t1 written to frame t1 + 1; 'head' written at the next head's offset."""
    q, k, v = (np.asarray(x, F32) for x in (q, k, v))
    I, T, _ = q.shape
    if kind == "chain":
        s = np.zeros((I, T, T), F32)
        for d in range(HD):
            s = fma32(q[:, :, None, d], k[:, None, :, d], s)
    else:
        s = _tree_last(q[:, :, None, :] * k[:, None, :, :])
    if fault == "transpose":
        s = np.ascontiguousarray(s.transpose(0, 2, 1))
    if fault == "drop_last":
        s, v = s[:, :, :T - 1], v[:, :T - 1]
    Tk = s.shape[-1]
    e = G._expf32(s - s.max(-1, keepdims=True))
    bump = F32(1.0 + 2.0 ** -9) if fault == "weight" else F32(1.0)
    acc = np.zeros((I, T, HD), F32)
    if kind == "chain":
        ep = np.zeros((I, T, 8), F32)
        ep[:, :, :Tk] = e
        p = e / _tree_adjacent(ep)[:, :, None]
        p[:, 0, 0] *= bump
        for j in range(Tk):
            acc = fma32(p[:, :, j, None], v[:, None, j, :], acc)
        o = acc
    else:
        den = np.zeros((I, T), F32)
        for j in range(Tk):
            den = den + e[:, :, j]
            w = e[:, :, j].copy()
            if j == 0:
                w[:, 0] *= bump
            acc = fma32(w[:, :, None], v[:, None, j, :], acc)
        o = acc / den[:, :, None]
    if fault == "row_shift":
        o = np.roll(o, 1, axis=1)
    if fault == "head":
        o = np.roll(o.reshape(-1, heads, T, HD), 1, axis=1).reshape(I, T, HD)
    hi = G.rne_op(torch.from_numpy(np.ascontiguousarray(o)), dtype)
    if not pair:
        return hi
    return hi, G.rne_op(torch.from_numpy(o - hi.float().numpy()), dtype)


def temporal_gauss(B, T, N, heads, dtype, std):
    """Gaussian qkv fp32 [B*T*N][3 D] of values `dtype` holds (None: plain fp32, the f32 kernel's operands): v ~ N(0, 1), q and k scaled so
    that a score q . k over 64 dims has standard deviation `std`"""
    gen = torch.Generator().manual_seed(1000 * T + 10 * N + heads + int(std))
    D = heads * HD
    x = torch.randn((B * T * N, 3, D), generator=gen)
    x[:, :2] *= math.sqrt(std / 8.0)
    x = x.reshape(B * T * N, 3 * D)
    return x if dtype is None else x.to(dtype).float()


def temporal_uniform(B, T, N, heads):
    """k = 0 and v = T m with integers |m| <= 16 that change with the item, the lane and the frame, q small integers -> (qkv fp32, want
    fp64 [B*T*N][D]). Every score is 0, every weight 1 / T, every output sum_t m_t: an integer of |.| <= 128, exact in fp32 in any order
    (all partial sums are integers below 2^11, or multiples of 1 / 8 at T = 8) and in both 16-bit formats."""
    I = B * N * heads
    i = torch.arange(I)[:, None, None]
    t = torch.arange(T)[None, :, None]
    d = torch.arange(HD)[None, None, :]
    m = (i * 37 + d * 11 + t * (2 * d + 1) + (i // heads) * 5) % 33 - 16
    q = ((i * 5 + d * 3 + t) % 7 - 3).expand(I, T, HD)
    qkv = merge_qkv(q.float(), torch.zeros((I, T, HD)), (T * m).float(), B, T, N, heads)
    want = m.sum(dim=1, keepdim=True).expand(I, T, HD).double()
    return qkv, merge_out(want, B, T, N, heads)


def temporal_onehot(B, T, N, heads, dtype):
    """q[t1] = 16 e_t1, k[t2] = 16 e_sigma(t2) with a permutation sigma per item, Gaussian v of values `dtype` holds (None: fp32) ->
    (qkv fp32, want fp32 [B*T*N][D], sigma [I][T]). A row's peak score is 256 and every other score 0: the off-peak weights are
    exp(-256) = 2^-369.3, zero in fp32 under any rounding, the denominator is exactly 1 and out[t1] = v[sigma^-1(t1)] unrounded."""
    I = B * N * heads
    rng = np.random.default_rng(77 * T + N + heads)
    sigma = torch.from_numpy(np.argsort(rng.random((I, T)), axis=1))
    q = torch.zeros((I, T, HD))
    k = torch.zeros((I, T, HD))
    ar = torch.arange(T)
    q[:, ar, ar] = 16.0
    k[torch.arange(I)[:, None], ar[None, :], sigma] = 16.0
    v = torch.randn((I, T, HD), generator=torch.Generator().manual_seed(5 * T + N))
    v = v if dtype is None else v.to(dtype).float()
    inv = torch.empty_like(sigma)
    inv[torch.arange(I)[:, None], sigma] = ar[None, :].expand(I, T)
    want = v[torch.arange(I)[:, None], inv]
    return merge_qkv(q, k, v, B, T, N, heads), merge_out(want, B, T, N, heads), sigma


# ==== ViT embed =========================================================================================================================
EMBED_F, EMBED_G2 = 3, 5          # 18 rows: the last workgroup holds 2 waves
EMBED_KINDS = ("gauss", "offset")
EMBED_FAULTS = ("pos_prev", "cls_nopos", "patch_stride", "ragged", "var_padded")
EMBED_EPS = 1e-5


def embed_problem(D, kind):
    """fp32 operands of one vit_embed launch: patch_out [F G2][D], cls [D], pos [G2 + 1][D], g, b [D]. 'gauss': rows of std ~2 around 0;
    'offset': rows of mean 1000 and std 1 (the mean's error reaches the variance); 'const': integers whose sums cls + pos[0] and
    patch_out + pos are constant along every row while each operand varies -- the row mean is that integer exactly (D |x| < 2^24), every
    deviation +-0 and the output beta bit for bit."""
    gen = torch.Generator().manual_seed(D + 17 * len(kind))
    F, G2 = EMBED_F, EMBED_G2
    g, b = 1.0 + torch.randn((D,), generator=gen), torch.randn((D,), generator=gen)
    if kind == "const":
        pos = torch.randint(-500, 501, (G2 + 1, D), generator=gen).float()
        c = torch.randint(-1000, 1001, (F, G2 + 1), generator=gen).float()
        cls = c[0, 0] - pos[0]
        patch = (c[:, 1:, None] - pos[None, 1:, :]).reshape(F * G2, D)
        assert D * 1000 < 2 ** 24
    elif kind == "offset":
        pos = torch.randn((G2 + 1, D), generator=gen) * 0.1
        cls = 1000.0 + torch.randn((D,), generator=gen)
        patch = 1000.0 + torch.randn((F * G2, D), generator=gen)
    else:
        pos = torch.randn((G2 + 1, D), generator=gen) * 0.5
        cls = torch.randn((D,), generator=gen)
        patch = torch.randn((F * G2, D), generator=gen) * 2.0
    return dict(patch_out=patch.contiguous(), cls=cls.contiguous(), pos=pos, g=g, b=b)


def embed_rows(patch_out, cls, pos, F, G2, fault=None):
    """the rows before the LayerNorm, each sum rounded once to fp32 as the kernel holds it: row f (G2 + 1) = cls + pos[0], row
    f (G2 + 1) + 1 + p = patch_out[f G2 + p] + pos[1 + p] -> float32 [F (G2 + 1)][D]"""
    patch_out, cls, pos = (torch.as_tensor(t).float() for t in (patch_out, cls, pos))
    N = G2 + 1
    rows = []
    for f in range(F):
        for n in range(N):
            pr = pos[n - 1 if fault == "pos_prev" and n > 0 else n]
            if n == 0:
                rows.append(cls.clone() if fault == "cls_nopos" else cls + pr)
            else:
                src = (f * N + n - 1) % (F * G2) if fault == "patch_stride" else f * G2 + n - 1
                rows.append(patch_out[src] + pr)
    return torch.stack(rows)


def embed_bound(x, g, y64, t64, rstd64):
    """norm_ref.ln_bound with an fp32 store: the same terms from the same constants (C_MEAN, E_RSTD_LN: a lane of vit_embed_kernel adds at
    most NCH 4 = 64 terms and wave_sum has 6 levels, norm_ref.CHAIN_WAVE), with u |y| of the fp32 store in place of the 16-bit half ulp"""
    x, g = torch.as_tensor(x).double(), torch.as_tensor(g).double()
    dm = NR.C_MEAN * U32 * x.abs().mean(-1, keepdim=True)
    e_rstd = NR.E_RSTD_LN + 0.5 * (dm * rstd64) ** 2
    return t64.abs() * (e_rstd + 3 * U32) + dm * rstd64 * g.abs() + U32 * y64.abs() + U32 * y64.abs()


def embed_ref(p, F=EMBED_F, G2=EMBED_G2, eps=EMBED_EPS):
    """(y64, bound, x32) of one launch: the fp32 rows of embed_rows, LayerNorm in fp64 (norm_ref.ln_ref)"""
    x = embed_rows(p["patch_out"], p["cls"], p["pos"], F, G2)
    y64, t64, rstd64 = NR.ln_ref(x, p["g"], p["b"], eps)
    return y64, embed_bound(x, p["g"], y64, t64, rstd64), x


def embed_f32(p, F=EMBED_F, G2=EMBED_G2, eps=EMBED_EPS, fault=None):
    """vit_embed_kernel in numpy float32 (lane sums over the float4 chunks, then the tree) -> (y float32 [rows][D], affected rows).
    Faults: 'pos_prev' position row n - 1 used for row n; 'cls_nopos' the CLS row without pos[0]; 'patch_stride' patch row f N + n - 1
    in place of f G2 + n - 1; 'ragged' the last, partly filled 256-column chunk left out of the mean; 'var_padded' the variance divided
    by the width padded to whole chunks."""
    N = G2 + 1
    x = embed_rows(p["patch_out"], p["cls"], p["pos"], F, G2, fault=fault).numpy()
    g, b = p["g"].numpy(), p["b"].numpy()
    R, D = x.shape
    n_of = np.arange(R) % N
    rows = {"pos_prev": n_of > 0, "cls_nopos": n_of == 0, "patch_stride": (np.arange(R) // N > 0) & (n_of > 0)}.get(fault, np.ones(R, bool))
    padded = -(-D // 256) * 256
    xs = x.copy()
    if fault == "ragged":
        xs[:, padded - 256:] = 0
    mean = NR._lane_sums(xs, 64) / F32(D)
    d = x - mean[:, None]
    var = NR._lane_sums(d * d, 64) / F32(padded if fault == "var_padded" else D)
    rstd = NR._rsqrt32(var + F32(eps))
    return d * rstd[:, None] * g + b, np.nonzero(rows)[0]


# ==== region pooling ====================================================================================================================
# (G, image_size, D, boxes): the slice sweep on a small canvas; 64 boxes at the image tower's grid (24, 224), at an integer scale (16, 224:
# every tap weight 1 / 2), at the widest grid (64 lines: the whole ballot) on a fractional scale, and at scale 1 (64, 64: the second tap of
# every line has weight zero); 16 channel slabs
REGION_SHAPES = ((6, 28, 64, "sweep"), (24, 224, 128, "boxes"), (16, 224, 64, "boxes"), (64, 100, 64, "boxes"), (64, 64, 64, "boxes"),
                 (24, 224, 1024, "four"))
SWEEP_GRIDS = ((6, 28), (24, 224), (16, 224), (64, 100), (64, 64), (1, 7), (5, 5))
MASK_FAULTS = ("swap", "inclusive", "zero_tap")
# loc_n of the launches that also run LocationEncoder layer 0, by (G, image_size, D): 2 outputs over 16 slabs (per = 1: most slabs own
# nothing), 100 over 2 slabs, 600 over one slab (3 passes of the 256 threads)
LOC_N = {(24, 224, 1024): 2, (24, 224, 128): 100, (16, 224, 64): 600}


def line_taps(G, image):
    """the source taps of grid line 0 .. G - 1 (rows and columns alike) as upsample_bilinear2d with align_corners=False takes them, in
    float32: src = max(scale (dst + 0.5) - 0.5, 0) -> (i0, i1 int64 [G], w0 > 0, w1 > 0 bool [G])"""
    scale = F32(image) / F32(G)
    src = scale * (np.arange(G).astype(F32) + F32(0.5)) - F32(0.5)
    src = np.maximum(src, F32(0))
    i0 = np.minimum(src.astype(np.int64), image - 1)
    i1 = np.where(i0 < image - 1, i0 + 1, i0)
    w1 = src - i0.astype(F32)
    return i0, i1, (F32(1) - w1) > 0, w1 > 0


def lines_on(lo, hi, G, image, fault=None):
    """bool [B][G]: line g touches [lo, hi) when one of its taps with non-zero weight lies inside (the kernel's integer rule). Faults:
    'inclusive' the upper bound taken inclusive; 'zero_tap' a tap of weight zero counted."""
    i0, i1, p0, p1 = line_taps(G, image)
    lo, hi = np.asarray(lo, np.int64)[:, None], np.asarray(hi, np.int64)[:, None]
    if fault == "inclusive":
        hi = hi + 1
    if fault == "zero_tap":
        p0, p1 = np.ones_like(p0), np.ones_like(p1)
    return (p0 & (i0 >= lo) & (i0 < hi)) | (p1 & (i1 >= lo) & (i1 < hi))


def region_lines(slices, G, image, fault=None):
    """(rows_on, cols_on) bool [B][G] of the integer rule; slices int [B][4] = {r0, r1, c0, c1}. 'swap': rows and columns exchanged."""
    s = np.asarray(slices, np.int64)
    if fault == "swap":
        s = s[:, [2, 3, 0, 1]]
    f = fault if fault in ("inclusive", "zero_tap") else None
    return lines_on(s[:, 0], s[:, 1], G, image, f), lines_on(s[:, 2], s[:, 3], G, image, f)


def lines_mask(rows_on, cols_on):
    return rows_on[:, :, None] & cols_on[:, None, :]


def region_mask_ref(slices, G, image_size):
    """The reference, literally: a {0, 1} canvas with [r0:r1, c0:c1] = 1 (x indexes rows), F.interpolate(size=(G, G), mode='bilinear',
    align_corners=False) > 0, on the CPU -> bool [B][G][G]"""
    s = np.asarray(slices, np.int64)
    canvas = torch.zeros((s.shape[0], 1, image_size, image_size))
    for b, (r0, r1, c0, c1) in enumerate(s.tolist()):
        canvas[b, 0, r0:r1, c0:c1] = 1.0
    return (Fn.interpolate(canvas, size=(G, G), mode="bilinear", align_corners=False) > 0)[:, 0].numpy()


def sweep_boxes(image):
    """every slice pair r0 <= r1 as rows against full columns, then the same as columns against full rows (the empty boxes included)"""
    pairs = [(a, b) for a in range(image + 1) for b in range(a, image + 1)]
    return np.array([[a, b, 0, image] for a, b in pairs] + [[0, image, a, b] for a, b in pairs], np.int32)


def region_boxes(G, image, n=64):
    """n = 64 boxes: the full canvas; 7 single pixels (two corners and the centre, which may touch no cell at all, and four that light
    exactly one cell); 40 tap-boundary boxes -- box t puts a row edge on a tap of line t mod G and a column
    edge on a tap of line (t + 40) mod G (every grid line gets one: 80 edges >= 64 lines), even t starting the rows AT the line's second tap
    and ending the columns just after the line's first tap, odd t ending the rows just BEFORE the second tap and starting the columns just after
    the first; the rest seeded random boxes, one of them empty."""
    rng = np.random.default_rng(1000 * G + image)
    i0, i1, _, _ = line_taps(G, image)
    out = [[0, image, 0, image]]
    pix = np.arange(image)
    single = pix[lines_on(pix, pix + 1, G, image).sum(1) == 1]           # pixels that are a live tap of exactly one grid line
    px = [(0, 0), (image - 1, image - 1), (image // 2, image // 2)] + [tuple(rng.choice(single, 2)) for _ in range(4)]
    out += [[int(r), int(r) + 1, int(c), int(c) + 1] for r, c in px]
    for t in range(40):
        a, b = int(i1[t % G]), int(i0[(t + 40) % G])
        span = int(rng.integers(1, image))
        if t % 2 == 0:
            out.append([a, min(image, a + span), max(0, b + 1 - span), b + 1])
        else:
            out.append([max(0, a - span), a, min(image, b + 1), min(image, b + 1 + span)])
    while len(out) < n - 1:
        r = np.sort(rng.integers(0, image + 1, 2))
        c = np.sort(rng.integers(0, image + 1, 2))
        out.append([int(r[0]), int(r[1]), int(c[0]), int(c[1])])
    out.append([image // 3, image // 3, 0, image])
    return np.array(out[:n], np.int32)


def region_slices(G, image, boxes):
    if boxes == "sweep":
        return sweep_boxes(image)
    if boxes == "four":
        return np.array([[0, image, 0, image], [image // 2, image // 2 + 1, 5, 6], [17, 140, 60, 61], [9, 9, 0, image]], np.int32)
    return region_boxes(G, image)


def region_feats(B, G, D, dtype, kind):
    """feats fp32 [B][G G][D] of values `dtype` holds: 'gauss' N(0, 1); 'int' integers |x| <= 8"""
    gen = torch.Generator().manual_seed(B + 7 * G + D)
    if kind == "int":
        return torch.randint(-8, 9, (B, G * G, D), generator=gen).float()
    return torch.randn((B, G * G, D), generator=gen).to(dtype).float()


def pool_inv(count):
    """fl32(1 / (fl32(count) + 1e-8f)) as float64 [B] (0 for an empty box: the kernel adds nothing). fl32(count + 1e-8) == count for every
    count >= 1 (1e-8 is below half an ulp of 1), so this is the rounded reciprocal of the count."""
    c = np.asarray(count).astype(F32)
    with np.errstate(divide="ignore"):
        inv = (F32(1.0) / (c + F32(1e-8))).astype(np.float64)
    return np.where(np.asarray(count) > 0, inv, 0.0)


def region_pool_ref(feats, mask, dtype):
    """(ref64 [B][D], bound): the masked mean sum_cells x * inv in fp64 with inv = pool_inv(count). The kernel walks the bounding rectangle
    of the on-cells (= the on-cells: the on-lines of a box are contiguous), 32 cells per step, so a lane chains ceil(cells / 32) fmaf /
    rounded products and adds; then 3 shuffle adds and the 4 waves' partial sums (3 adds): (ceil(cells / 32) + 9) u sum |x| inv with the
    product's rounding and two to spare, + half an ulp of the store."""
    x = torch.as_tensor(feats).double()
    B = x.shape[0]
    m = torch.from_numpy(np.asarray(mask)).reshape(B, -1).double()
    cnt = m.sum(-1)
    inv = torch.from_numpy(pool_inv(cnt.numpy()))[:, None]
    ref = torch.einsum("bc,bcd->bd", m, x) * inv
    e = (torch.ceil(cnt / 32) + 9)[:, None] * U32 * torch.einsum("bc,bcd->bd", m, x.abs()) * inv
    return ref, e + _half_ulp_t(ref.abs() + e, dtype)


def region_pool_f32(feats, rows_on, cols_on, G, dtype, fault=None):
    """region_pool_kernel's masked mean in numpy float32: cell k of the bounding rectangle goes to (wave, cell lane) = k mod 32, each adds
    its cells serially (fmaf), the 8 cell lanes meet in 3 xor-shuffles and the 4 waves as (0 + 1) + (2 + 3). Faults: 'count_plus1' the
    divisor count + 1; 'rect' every cell of the rectangle summed, the mask ignored."""
    x = np.asarray(feats, F32)
    B, _, D = x.shape
    out = np.zeros((B, D), F32)
    for b in range(B):
        rm, cm = rows_on[b], cols_on[b]
        cnt = int(rm.sum()) * int(cm.sum())
        if cnt == 0:
            continue
        ri, ci = np.nonzero(rm)[0], np.nonzero(cm)[0]
        i0, j0, nj = ri[0], ci[0], ci[-1] - ci[0] + 1
        total = (ri[-1] - ri[0] + 1) * nj
        inv = F32(1.0) / (F32(cnt + (fault == "count_plus1")) + F32(1e-8))
        ks = np.arange(total)
        i, j = i0 + ks // nj, j0 + ks % nj
        on = np.ones(total, bool) if fault == "rect" else rm[i] & cm[j]
        steps = -(-total // 32)
        xs = np.zeros((steps * 32, D), F32)
        xs[:total][on] = x[b, (i * G + j)[on]]
        xs = xs.reshape(steps, 32, D)
        acc = np.zeros((32, D), F32)
        for st in range(steps):
            acc = fma32(xs[st], inv, acc)
        w = _tree_adjacent(np.ascontiguousarray(acc.reshape(4, 8, D).transpose(0, 2, 1)))           # [4 waves][D]
        out[b] = (w[0] + w[1]) + (w[2] + w[3])
    return G_rne(out, dtype)


def G_rne(x, dtype):
    return G.rne_op(torch.from_numpy(np.ascontiguousarray(x, F32)), dtype)


def lines_contiguous(on):
    """bool [B]: the on-lines of every box form one run (what lets the kernel walk a rectangle)"""
    on = np.asarray(on, bool)
    edges = np.diff(np.concatenate([np.zeros((on.shape[0], 1), np.int8), on.astype(np.int8), np.zeros((on.shape[0], 1), np.int8)], 1), axis=1)
    return (edges == 1).sum(1) <= 1


def loc_problem(B, loc_n, dtype, kind):
    """LocationEncoder layer 0 operands: coords fp32 [B][4], w0 fp32 [loc_n][8] of values `dtype` holds (columns 4 .. 7 zero: the packed
    layout), b0 fp32 [loc_n]. 'int': integer coords in 0 .. 336, weights |w| <= 4, bias |b| <= 64 -- every partial sum is an integer below
    2^24; 'gauss': coords uniform in [0, 336), w ~ N(0, 0.05), b ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(31 * loc_n + B)
    w = torch.zeros((loc_n, 8))
    if kind == "int":
        coords = torch.randint(0, 337, (B, 4), generator=gen).float()
        w[:, :4] = torch.randint(-4, 5, (loc_n, 4), generator=gen).float()
        b = torch.randint(-64, 65, (loc_n,), generator=gen).float()
    else:
        coords = torch.rand((B, 4), generator=gen) * 336.0
        w[:, :4] = (torch.randn((loc_n, 4), generator=gen) * 0.05).to(dtype).float()
        w[::2] = w[::2].abs()                                             # the coords are positive: every other output is above the relu's knee
        b = torch.randn((loc_n,), generator=gen)
    return coords, w, b


def loc_ref(coords, w, b, dtype):
    """(ref64 [B][loc_n], bound): relu(coords . w[:, :4] + b) in fp64; the kernel rounds one product, three fmaf and the addition of the
    bias: 5 u (sum |c w| + |b|), + half an ulp of the store"""
    c, w, b = torch.as_tensor(coords).double(), torch.as_tensor(w).double()[:, :4], torch.as_tensor(b).double()
    ref = torch.relu(c @ w.T + b)
    e = 5 * U32 * (c.abs() @ w.abs().T + b.abs())
    return ref, e + _half_ulp_t(ref + e, dtype)


def loc_f32(coords, w, b, dtype, slabs, fault=None):
    """the kernel's layer 0 in numpy float32 -> [B][loc_n] as stored, NaN where no block writes. Slab s owns outputs s per .. s per + per - 1,
    per = ceil(loc_n / slabs); fault 'per_floor': per rounded down (the tail, or with loc_n < slabs everything, is never written)."""
    c, w, b = np.asarray(coords, F32), np.asarray(w, F32), np.asarray(b, F32)
    loc_n = w.shape[0]
    v = c[:, None, 0] * w[None, :, 0]
    for i in (1, 2, 3):
        v = fma32(c[:, None, i], w[None, :, i], v)
    v = np.maximum(v + b[None, :], F32(0))
    per = loc_n // slabs if fault == "per_floor" else -(-loc_n // slabs)
    written = np.zeros(loc_n, bool)
    for s in range(slabs):
        written[s * per:min(loc_n, s * per + per)] = True
    out = G_rne(v, dtype).float()
    out[:, torch.from_numpy(~written)] = float("nan")
    return out
