"""The tower kernels on the GPU against tests/tower_ref.py, element by element, in both operand builds: temporal attention
(attn_temporal8_kernel, attn_temporal_kernel<T> through ops.attn_temporal; attn_temporal_f32_kernel<T> through ops.attn_temporal_f32 with
ld = 3 D + 8), the ViT embedding assembly + pre-LayerNorm (vit_embed_kernel<NCH> at every chunk count, full and ragged) and the region
extractor's pooling launch (cell mask, count, masked mean, LocationEncoder layer 0). Exact probes are compared bit for bit, Gaussian data
inside the derived bounds with no element exempt. Every output is the head of a buffer of NaN bits whose other rows -- and, where the
leading dimension exceeds the width, whose gap -- must come back untouched; every input must come back unchanged. The inputs are built
by tests/tower_ref.py, where tests/test_tower_ref_host.py shows that they flag every emulated fault. DESIGN.md "Tower-kernel pinning"."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests import norm_ref as NR
from tests import tower_ref as TR
from tests.test_gpu_gemm import _bits, _exact, _where

pytestmark = pytest.mark.gpu
DT_IDS = ["bf16", "fp16"]
SHAPE_IDS = ["x".join(map(str, s)) for s in TR.TEMPORAL_SHAPES]
NAN_I32 = 0x7FC00000


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


class Guard:
    """out = buf[:rows, :cols] of a buffer of NaN bits 3 rows taller and `ld` wide; check(): every bit outside the window as before, no NaN
    inside -> the window on the host"""

    def __init__(self, dev, rows, cols, dtype, ld=None):
        self.rows, self.cols = rows, cols
        fill = NAN_I32 if dtype == torch.int32 else float("nan")
        self.buf = torch.full((rows + 3, cols if ld is None else ld), fill, dtype=dtype, device=dev)
        self.view = self.buf[:rows, :cols]
        self.before = _bits(self.buf).clone()

    def check(self, what):
        torch.cuda.synchronize()
        same = _bits(self.buf) == self.before
        same[:self.rows, :self.cols] = True
        assert bool(same.all()), f"{what}: {int((~same).sum())} elements written outside the {self.rows} x {self.cols} window, first at {(~same).nonzero()[0].tolist()}"
        got = self.view.cpu()
        if got.dtype != torch.int32:
            assert not bool(torch.isnan(got.float()).any()), f"{what}: NaN in the result"
        return got


class Inputs:
    """device copies of the operands; unchanged(): their bits as uploaded"""

    def __init__(self, dev, **tensors):
        self.t = {k: v.to(dev) for k, v in tensors.items()}
        self.before = {k: _bits(v).clone() for k, v in self.t.items()}

    def __getitem__(self, k):
        return self.t[k]

    def unchanged(self, what):
        torch.cuda.synchronize()
        for k, v in self.t.items():
            assert torch.equal(_bits(v), self.before[k]), f"{what}: input {k} changed"


def _within(got64, ref64, bound, what, record_property=None):
    """|got - ref64| <= bound element by element, no element exempt -> the worst err / bound"""
    err = (got64 - ref64).abs()
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    worst = float(ratio.max())
    print(f"[{what}] worst err / bound {worst:.3f}")                    # shown with -s: the figures EXPERIMENTS.md records
    if record_property is not None:
        record_property(what, round(worst, 4))
    assert not bool(bad.any()), _where(bad, got64, ref64, what) + f"; worst err / bound {worst:.3f}"
    return worst


# ---- temporal attention ----------------------------------------------------------------------------------------------------------------
def _temporal16(dev, qkv, shape, dtype, what):
    """one ops.attn_temporal launch on qkv (fp32 holder of operand values) -> the output on the host, [B T N][D] in `dtype`"""
    from vitron_amd import ops
    B, T, N, heads = shape
    assert G.representable(qkv, dtype)
    inp = Inputs(dev, qkv=qkv.to(dtype))
    g = Guard(dev, B * T * N, heads * TR.HD, dtype)
    ops.attn_temporal(inp["qkv"], B, T, N, heads, out=g.buf)
    got = g.check(what)
    inp.unchanged(what)
    return got


def _temporal32(dev, qkv, shape, dtype, what):
    """one ops.attn_temporal_f32 launch on the fp32 qkv, rows ld = 3 D + 8 apart inside NaN -> (hi, lo) on the host"""
    from vitron_amd import ops
    B, T, N, heads = shape
    rows, D = B * T * N, heads * TR.HD
    buf = torch.full((rows + 2, 3 * D + 8), float("nan"))
    buf[:rows, :3 * D] = qkv
    inp = Inputs(dev, qkv=buf)
    hi, lo = Guard(dev, rows, D, dtype), Guard(dev, rows, D, dtype)
    ops.attn_temporal_f32(inp["qkv"][:rows, :3 * D], B, T, N, heads, out=hi.buf, out_lo=lo.buf)
    got = hi.check(what + " hi"), lo.check(what + " lo")
    inp.unchanged(what)
    return got


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", TR.TEMPORAL_SHAPES, ids=SHAPE_IDS)
def test_temporal_uniform_probe_is_the_integer_mean(dev, shape, dtype):
    """k = 0, v = T m: every output is sum_t m_t bit for bit, in all three kernels -- which rows, heads and lanes each item reads and
    writes, the partly filled last workgroup included. The pair kernel's lo is exactly zero."""
    qkv, want = TR.temporal_uniform(*shape)
    _exact(_temporal16(dev, qkv, shape, dtype, "uniform").double(), want, f"temporal uniform {shape}")
    hi, lo = _temporal32(dev, qkv, shape, dtype, "uniform f32")
    _exact(hi.double(), want, f"temporal f32 uniform {shape} hi")
    _exact(lo.double(), torch.zeros_like(want), f"temporal f32 uniform {shape} lo")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", TR.TEMPORAL_SHAPES, ids=SHAPE_IDS)
def test_temporal_onehot_probe_selects_the_permuted_frame(dev, shape, dtype):
    """q[t1] = 16 e_t1, k[t2] = 16 e_sigma(t2): the off-peak weights are exactly 0 and out[t1] = v[sigma^-1(t1)] bit for bit (the pair
    kernel on fp32 v: hi the rounding of v, lo the rounding of the rest)"""
    qkv, want, _ = TR.temporal_onehot(*shape, dtype)
    _exact(_temporal16(dev, qkv, shape, dtype, "one-hot"), want.to(dtype), f"temporal one-hot {shape}")
    qkv, want, _ = TR.temporal_onehot(*shape, None)
    hi, lo = _temporal32(dev, qkv, shape, dtype, "one-hot f32")
    want_hi = G.rne_op(want, dtype)
    _exact(hi, want_hi, f"temporal f32 one-hot {shape} hi")
    _exact(lo, G.rne_op(want - want_hi.float(), dtype), f"temporal f32 one-hot {shape} lo")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", TR.TEMPORAL_SHAPES, ids=SHAPE_IDS)
def test_temporal_random_data_is_inside_the_bound_everywhere(dev, shape, dtype, record_property):
    """Gaussian operands at two score widths: every element of the 16-bit kernels within temporal_bound of the fp64 reference; the pair
    kernel's hi + lo within the arithmetic bound + half an ulp of lo's format at |o - hi|, |lo| <= half an ulp of hi, and hi the 16-bit
    rounding of hi + lo (where |lo| is exactly half an ulp of hi the sum is a tie, which lo's own rounding can create: either neighbour is
    the kernel's correct hi there). A second launch returns the same bits."""
    B, T, N, heads = shape
    fmt = TR.FMT[dtype]
    for std in TR.SCORE_STDS:
        qkv = TR.temporal_gauss(B, T, N, heads, dtype, std)
        q, k, v = TR.split_qkv(qkv, B, T, N, heads)
        got = _temporal16(dev, qkv, shape, dtype, "gauss")
        o64 = TR.merge_out(TR.temporal_ref(q, k, v), B, T, N, heads)
        bound = TR.merge_out(TR.temporal_bound(q, k, v, dtype, 0), B, T, N, heads)
        _within(got.double(), o64, bound, f"temporal {TR.temporal_kind(T, False)} {shape} {fmt} std {std:g}", record_property)
        assert torch.equal(_bits(got), _bits(_temporal16(dev, qkv, shape, dtype, "gauss again"))), "two launches differ"

        qkv = TR.temporal_gauss(B, T, N, heads, None, std)
        q, k, v = TR.split_qkv(qkv, B, T, N, heads)
        hi, lo = _temporal32(dev, qkv, shape, dtype, "gauss f32")
        o64 = TR.merge_out(TR.temporal_ref(q, k, v), B, T, N, heads)
        e = TR.merge_out(TR.temporal_bound(q, k, v, None, 1), B, T, N, heads)
        s = hi.double() + lo.double()
        _within(s, o64, TR.pair_bound(o64, e, hi, dtype), f"temporal f32 pair {shape} {fmt} std {std:g}", record_property)
        half = TR._half_ulp_t(hi.double().abs(), dtype)
        assert bool((lo.double().abs() <= half).all()), "|lo| above half an ulp of hi"
        assert bool((s.float().double() == s).all())                                        # hi + lo is an fp32 number: the kernel's o up to lo's rounding
        wrong = (G.rne_op(s, dtype) != hi) & (lo.double().abs() != half)
        assert not bool(wrong.any()), _where(wrong, hi, G.rne_op(s, dtype), f"temporal f32 {shape}: hi is not the rounding of hi + lo")
        hi2, lo2 = _temporal32(dev, qkv, shape, dtype, "gauss f32 again")
        assert torch.equal(_bits(hi), _bits(hi2)) and torch.equal(_bits(lo), _bits(lo2)), "two launches differ"


# ---- ViT embed -------------------------------------------------------------------------------------------------------------------------
def _embed(dev, p, lib, what):
    from vitron_amd import ops
    F, G2 = TR.EMBED_F, TR.EMBED_G2
    inp = Inputs(dev, **p)
    g = Guard(dev, F * (G2 + 1), p["pos"].shape[1], torch.float32)
    ops.vit_embed(inp["patch_out"], inp["cls"], inp["pos"], inp["g"], inp["b"], F, G2, TR.EMBED_EPS, out=g.buf, lib=lib)
    got = g.check(what)
    inp.unchanged(what)
    N = G2 + 1
    assert torch.equal(_bits(got[0]), _bits(got[N])) and torch.equal(_bits(got[0]), _bits(got[2 * N])), f"{what}: the frames' CLS rows differ"
    return got


@pytest.mark.parametrize("operand", DT_IDS)
@pytest.mark.parametrize("D", NR.D_SET)
def test_vit_embed_is_inside_the_bound_everywhere(dev, D, operand, record_property):
    """18 rows (3 frames of CLS + 5 patches: the last workgroup holds 2 waves) at every chunk count, full and ragged: Gaussian rows and
    rows of mean 1000, std 1 against the fp64 LayerNorm of the fp32 sums; the three CLS rows bit-identical. The kernel has no 16-bit
    operand: both builds of the library must give the same bits."""
    from vitron_amd import _lib
    lib = _lib.load(operand=operand)
    for kind in TR.EMBED_KINDS:
        p = TR.embed_problem(D, kind)
        y64, bound, _ = TR.embed_ref(p)
        got = _embed(dev, p, lib, f"embed D={D} {kind}")
        _within(got.double(), y64, bound, f"vit_embed D={D} {kind} ({operand} build)", record_property)
        other = _embed(dev, p, _lib.load(operand="fp16" if operand == "bf16" else "bf16"), f"embed D={D} {kind} other build")
        assert torch.equal(_bits(got), _bits(other)), "the two builds differ"


@pytest.mark.parametrize("D", [d for d in NR.D_SET if d & (d - 1) == 0])
def test_vit_embed_constant_rows_give_beta(dev, D):
    """integer patch_out / cls / pos whose sums are constant along a row: mean exact, every deviation zero, the output beta bit for bit"""
    from vitron_amd import _lib
    p = TR.embed_problem(D, "const")
    for operand in DT_IDS:
        got = _embed(dev, p, _lib.load(operand=operand), f"embed const D={D}")
        _exact(got, p["b"][None, :].expand_as(got).contiguous(), f"vit_embed const D={D} ({operand} build)")


# ---- region pooling --------------------------------------------------------------------------------------------------------------------
REGION_IDS = ["x".join(map(str, s[:3])) for s in TR.REGION_SHAPES]
_mask_cache = {}


def _mask_ref(shape):
    if shape not in _mask_cache:
        G_, image, D, boxes = shape
        sl = TR.region_slices(G_, image, boxes)
        _mask_cache[shape] = (sl, TR.region_mask_ref(sl, G_, image))
    return _mask_cache[shape]


def _pool(dev, shape, dtype, x, sl, loc, what, want_mask=True):
    """one ops.region_pool launch -> (pooled, mask | None, count | None, loc_out | None) on the host; loc = (coords, w0, b0) or None"""
    from vitron_amd import ops
    G_, image, D, _ = shape
    B = len(sl)
    t = dict(feats=x.to(dtype), slices=torch.from_numpy(sl))
    if loc is not None:
        t.update(coords=loc[0], w0=loc[1].to(dtype), b0=loc[2])
    inp = Inputs(dev, **t)
    gp = Guard(dev, B, D, dtype)
    gm = Guard(dev, B, G_ * G_, torch.int32) if want_mask else None
    gc = Guard(dev, B, 1, torch.int32) if want_mask else None
    gl = None
    kw = {}
    if loc is not None:
        loc_n = loc[2].numel()
        gl = Guard(dev, B, loc_n, dtype, ld=loc_n + 8)
        kw = dict(coords=inp["coords"], loc_w0=inp["w0"], loc_b0=inp["b0"], loc_out=gl.view)
    ops.region_pool(inp["feats"], inp["slices"], G_, image, pooled=gp.buf, want_mask=want_mask,
                    cell_mask=gm.buf if gm else None, cell_count=gc.buf if gc else None, **kw)
    out = (gp.check(what + " pooled"), gm.check(what + " mask") if gm else None, gc.check(what + " count")[:, 0] if gc else None,
           gl.check(what + " loc") if gl else None)
    inp.unchanged(what)
    return out


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", TR.REGION_SHAPES, ids=REGION_IDS)
def test_region_pool_mask_mean_and_location_layer(dev, shape, dtype, record_property):
    """One launch over all boxes of the shape, Gaussian features (and Gaussian location weights where the shape runs the layer), then
    one with integer features and operands:
    * cell_mask and cell_count equal the literal reference (canvas, bilinear resize, > 0) bit for bit;
    * an empty box pools to exact zeros; a single-cell box returns that cell's features bit for bit (row / column orientation, slab and
      channel mapping); Gaussian features within the bound; integers |x| <= 8 over a power-of-two count give the exact mean, rounded once;
    * LocationEncoder layer 0 into a row-strided view (ld = loc_n + 8): Gaussian weights within loc_ref's bound, integer operands the
      exact relu rounded once; the same launch without loc_out, and without the optional outputs, returns the same pooled bits."""
    G_, image, D, boxes = shape
    fmt = TR.FMT[dtype]
    sl, mask = _mask_ref(shape)
    B = len(sl)
    cnt = mask.reshape(B, -1).sum(-1)
    loc_n = TR.LOC_N.get(shape[:3])
    for kind in ("gauss", "int"):
        x = TR.region_feats(B, G_, D, dtype, kind)
        loc = TR.loc_problem(B, loc_n, dtype, kind) if loc_n else None
        what = f"region_pool {shape[:3]} {fmt} {kind}"
        pooled, gmask, gcount, gloc = _pool(dev, shape, dtype, x, sl, loc, what)
        _exact(gmask, torch.from_numpy(mask.reshape(B, -1).astype(np.int32)), what + " cell_mask")
        _exact(gcount[:, None], torch.from_numpy(cnt.astype(np.int32))[:, None], what + " cell_count")
        ref, bound = TR.region_pool_ref(x, mask, dtype)
        _within(pooled.double(), ref, bound, what, record_property)
        empty = torch.from_numpy(cnt == 0)
        assert bool(empty.any()) and not bool(pooled[empty].float().any()), what + ": an empty box did not pool to zeros"
        for b in np.nonzero(cnt == 1)[0]:
            cell = int(np.argmax(mask[b].reshape(-1)))
            assert torch.equal(_bits(pooled[b]), _bits(x[b, cell].to(dtype))), f"{what}: box {b} (cell {divmod(cell, G_)}) is not that cell's features"
        if boxes == "boxes":
            assert int((cnt == 1).sum()) >= 3
        if kind == "int":
            p2 = torch.from_numpy((cnt > 0) & ((cnt & (cnt - 1)) == 0))
            assert bool(p2.any()) or boxes != "boxes"
            _exact(pooled[p2], G.rne_op(ref[p2], dtype), what + " power-of-two counts")
        if loc is not None:
            lref, lbound = TR.loc_ref(*loc, dtype)
            if kind == "int":
                _exact(gloc, G.rne_op(lref, dtype), what + f" loc_n={loc_n}")
            else:
                _within(gloc.double(), lref, lbound, f"location layer loc_n={loc_n} slabs={D // 64} {fmt}", record_property)
            p2_, m2, c2, _ = _pool(dev, shape, dtype, x, sl, None, what + " without loc_out")
            assert torch.equal(_bits(p2_), _bits(pooled)) and torch.equal(m2, gmask) and torch.equal(c2, gcount), what + ": the NULL-loc_out launch differs"
        p3, _, _, _ = _pool(dev, shape, dtype, x, sl, None, what + " without mask", want_mask=False)
        assert torch.equal(_bits(p3), _bits(pooled)), what + ": the launch without the optional outputs differs"
