"""The tower references without a GPU (tests/tower_ref.py), on the very inputs tests/test_gpu_tower_kernels.py launches: the float32
emulations of the temporal-attention, ViT-embed and region-pooling kernels stay inside their per-element bounds with NO element exempt,
every emulated fault is flagged, the literal torch form of the region mask equals the kernel's integer line rule over a box sweep, and the
exact probes meet the preconditions under which fp32 returns them bit for bit."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests import norm_ref as NR
from tests import tower_ref as TR

DT_IDS = ["bf16", "fp16"]
SHAPE_IDS = ["x".join(map(str, s)) for s in TR.TEMPORAL_SHAPES]
FMTS = ("bf16", "fp16", "f32")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _ratio(got64, ref64, bound):
    err = (got64 - ref64).abs()
    return err / bound, ~(err <= bound)


def _temporal_case(shape, fmt, std):
    """(q, k, v, kind, operand dtype | None, prod_round) of one GPU launch"""
    B, T, N, heads = shape
    dt = DT.get(fmt)
    q, k, v = TR.split_qkv(TR.temporal_gauss(B, T, N, heads, dt, std), B, T, N, heads)
    return q, k, v, TR.temporal_kind(T, dt is None), dt, int(dt is None)


def _temporal_judge(q, k, v, kind, dt, prod_round, heads, fault=None):
    """-> (worst err / bound, any element outside) over every store the launch has (the pair kernel: both pair formats, hi + lo)"""
    o64 = TR.temporal_ref(q, k, v)
    worst, outside = 0.0, False
    if dt is not None:
        got = TR.temporal_f32(q.numpy(), k.numpy(), v.numpy(), kind, dt, heads, fault=fault)
        r, bad = _ratio(got.double(), o64, TR.temporal_bound(q, k, v, dt, prod_round))
        return float(r.max()), bool(bad.any())
    e = TR.temporal_bound(q, k, v, None, prod_round)
    for pdt in G.DTYPES:
        hi, lo = TR.temporal_f32(q.numpy(), k.numpy(), v.numpy(), kind, pdt, heads, fault=fault, pair=True)
        r, bad = _ratio(hi.double() + lo.double(), o64, TR.pair_bound(o64, e, hi, pdt))
        worst, outside = max(worst, float(r.max())), outside or bool(bad.any())
        if fault is None:
            assert bool((lo.double().abs() <= TR._half_ulp_t(hi.double().abs(), pdt)).all()), "|lo| above half an ulp of hi"
    return worst, outside


# ---- temporal attention ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", TR.TEMPORAL_SHAPES, ids=SHAPE_IDS)
def test_temporal_emulations_are_inside_the_bound_everywhere(shape, fmt):
    for std in TR.SCORE_STDS:
        worst, outside = _temporal_judge(*_temporal_case(shape, fmt, std), shape[3])
        print(f"[temporal emulation {shape} {fmt} score std {std}] worst err / bound {worst:.3f}")
        assert not outside and worst <= 1.0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", TR.TEMPORAL_SHAPES[:10], ids=SHAPE_IDS[:10])
def test_temporal_faults_are_flagged(shape, fmt):
    """every fault, at both score widths, puts at least one element outside the bound (T = 1 has one frame and one weight, identically 1:
    nothing to drop, transpose, shift or scale -- only the head offset). The tower-width shape adds no path to these: left to the
    emulation test."""
    T = shape[1]
    for std in TR.SCORE_STDS:
        case = _temporal_case(shape, fmt, std)
        for fault in TR.TEMPORAL_FAULTS:
            if T == 1 and fault != "head":
                continue
            worst, outside = _temporal_judge(*case, shape[3], fault=fault)
            print(f"[temporal fault {fault} {shape} {fmt} score std {std}] worst err / bound {worst:.1f}")
            assert outside, (fault, shape, fmt, std, worst)


@pytest.mark.parametrize("shape", TR.TEMPORAL_SHAPES, ids=SHAPE_IDS)
def test_temporal_probes_are_exact_in_fp32(shape):
    """uniform probe: every partial sum of either summation is an integer (a multiple of 1 / 8 at T = 8) far below 2^24 and the output an
    integer both 16-bit formats hold; neighbouring items, heads and lanes expect different values. One-hot probe: scores are 0 or 256,
    exp(-256) is zero in fp32, the peak's weight exactly 1. Both emulations return the expected bits."""
    B, T, N, heads = shape
    qkv, want = TR.temporal_uniform(B, T, N, heads)
    q, k, v = TR.split_qkv(qkv, B, T, N, heads)
    assert not bool(k.any()) and bool((v == v.round()).all()) and float(v.abs().max()) <= 16 * T and float(v.abs().sum(1).max()) * 8 < 2 ** 24
    assert bool((want == want.round()).all()) and float(want.abs().max()) <= 128
    for dt in G.DTYPES:
        assert G.representable(qkv, dt) and G.representable(want, dt)
    w = want.reshape(B, T, N, heads, TR.HD)
    assert float((w[:, :, :, 1:] != w[:, :, :, :-1]).float().mean()) > 0.9 and float((w[..., 1:] != w[..., :-1]).float().mean()) > 0.9
    assert float((w[:, :, 1:] != w[:, :, :-1]).float().mean()) > 0.9
    assert float((v[:, 1:] != v[:, :-1]).float().mean()) > 0.9 if T > 1 else True
    for kind in ("chain", "tree") if T == 8 else ("tree",):
        for dt in G.DTYPES:
            got = TR.merge_out(TR.temporal_f32(q.numpy(), k.numpy(), v.numpy(), kind, dt, heads).double(), B, T, N, heads)
            assert torch.equal(got, want)
    assert float(G._expf32(np.float32(-256.0))) == 0.0 and -256.0 * 1.4426950408889634 < -150
    for dt in (torch.bfloat16, torch.float16, None):
        qkv, want, sigma = TR.temporal_onehot(B, T, N, heads, dt)
        q, k, v = TR.split_qkv(qkv, B, T, N, heads)
        s = torch.einsum("itd,iud->itu", q, k)
        assert bool(((s == 0) | (s == 256)).all()) and bool(((s == 256).sum(-1) == 1).all()) and bool(((q != 0).sum(-1) == 1).all())
        assert bool((torch.sort(sigma, dim=1).values == torch.arange(T)).all())
        assert T == 1 or bool((sigma != torch.arange(T)).any())
        for kind in ("chain", "tree") if T == 8 else ("tree",):
            pdt = dt or torch.bfloat16
            hi, lo = TR.temporal_f32(q.numpy(), k.numpy(), v.numpy(), kind, pdt, heads, pair=True)
            want_hi = G.rne_op(want, pdt)
            assert torch.equal(TR.merge_out(hi, B, T, N, heads), want_hi)
            assert torch.equal(TR.merge_out(lo, B, T, N, heads), G.rne_op(want - want_hi.float(), pdt))
            if dt is not None:
                assert not bool(lo.float().any())


# ---- ViT embed -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", NR.D_SET)
def test_embed_emulation_is_inside_the_bound_everywhere(D):
    for kind in TR.EMBED_KINDS:
        p = TR.embed_problem(D, kind)
        y64, bound, _ = TR.embed_ref(p)
        got, _ = TR.embed_f32(p)
        r, bad = _ratio(torch.from_numpy(got).double(), y64, bound)
        print(f"[embed emulation D={D} {kind}] worst err / bound {float(r.max()):.3f}")
        assert not bool(bad.any())
        N = TR.EMBED_G2 + 1
        assert np.array_equal(got[0], got[N]) and np.array_equal(got[0], got[2 * N])


@pytest.mark.parametrize("D", NR.D_SET)
def test_embed_faults_are_flagged(D):
    """every fault puts at least one element of EVERY row it touches outside the bound on the Gaussian rows (the two chunk faults exist
    only at a ragged width). The rows of mean 1000 allow the mean's own error, C_MEAN u 1000 rstd |g| = 4e-3 absolute, so a fault below
    that (the variance over 4096 instead of 4092 columns: 5e-4 |t|) passes there: those rows are there for the bound's second-order
    term, and their count is only printed."""
    for kind in TR.EMBED_KINDS:
        p = TR.embed_problem(D, kind)
        y64, bound, _ = TR.embed_ref(p)
        for fault in TR.EMBED_FAULTS:
            if fault in ("ragged", "var_padded") and D % 256 == 0:
                continue
            got, rows = TR.embed_f32(p, fault=fault)
            _, bad = _ratio(torch.from_numpy(got).double(), y64, bound)
            hit = bad.any(-1).numpy()[rows]
            print(f"[embed fault {fault} D={D} {kind}] {int(hit.sum())} of {len(rows)} rows flagged")
            assert len(rows) and (kind != "gauss" or bool(hit.all())), f"{fault} D={D} {kind}: {int(hit.sum())} of {len(rows)} rows flagged"


@pytest.mark.parametrize("D", [d for d in NR.D_SET if d & (d - 1) == 0])
def test_embed_constant_rows_are_exact(D):
    p = TR.embed_problem(D, "const")
    x = TR.embed_rows(p["patch_out"], p["cls"], p["pos"], TR.EMBED_F, TR.EMBED_G2)
    for t in (p["patch_out"], p["cls"], p["pos"]):
        assert bool((t == t.round()).all()) and float(t.std()) > 100                  # integers, none constant on its own
    assert bool((x == x[:, :1]).all()) and float(x.abs().max()) * D < 2 ** 24          # constant rows; any partial sum is an exact integer
    assert len(set(x[:, 0].tolist())) > x.shape[0] // 2
    got, _ = TR.embed_f32(p)
    assert np.array_equal(got, np.broadcast_to(p["b"].numpy(), got.shape))


# ---- region pooling --------------------------------------------------------------------------------------------------------------------
def _sweep(G_, image):
    if image <= 28:
        return TR.sweep_boxes(image)
    rng = np.random.default_rng(G_ + image)
    r, c = np.sort(rng.integers(0, image + 1, (300, 2)), 1), np.sort(rng.integers(0, image + 1, (300, 2)), 1)
    return np.concatenate([TR.region_boxes(G_, image), np.concatenate([r, c], 1).astype(np.int32)])


@pytest.mark.parametrize("grid", TR.SWEEP_GRIDS, ids=[f"{g}x{i}" for g, i in TR.SWEEP_GRIDS])
def test_region_mask_reference_equals_the_integer_rule(grid):
    G_, image = grid
    sl = _sweep(G_, image)
    ro, co = TR.region_lines(sl, G_, image)
    assert np.array_equal(TR.region_mask_ref(sl, G_, image), TR.lines_mask(ro, co)), grid
    assert bool(TR.lines_contiguous(ro).all()) and bool(TR.lines_contiguous(co).all())      # a box's cells fill their bounding rectangle
    print(f"[mask sweep {grid}] {len(sl)} boxes")


def _region_case(shape):
    G_, image, D, boxes = shape
    sl = TR.region_slices(G_, image, boxes)
    return sl, TR.region_mask_ref(sl, G_, image)


REGION_IDS = ["x".join(map(str, s[:3])) for s in TR.REGION_SHAPES]


def test_region_mask_faults_are_flagged_by_the_gpu_boxes():
    """each mask fault changes the mask of at least one box of the GPU tests (the zero-weight tap exists only at scale 1: the 64 x 64
    shape), and the boxes hold what the other checks need: empty boxes, single cells, power-of-two counts"""
    caught = {f: [] for f in TR.MASK_FAULTS}
    for shape in TR.REGION_SHAPES:
        G_, image, D, boxes = shape
        sl, ref = _region_case(shape)
        ro, co = TR.region_lines(sl, G_, image)
        assert np.array_equal(ref, TR.lines_mask(ro, co))
        assert bool(TR.lines_contiguous(ro).all()) and bool(TR.lines_contiguous(co).all())
        got = TR.region_pool_f32(TR.region_feats(min(len(sl), 8), G_, 64, torch.float16, "gauss").numpy(), ro[:8], co[:8], G_, torch.float16)
        rect = TR.region_pool_f32(TR.region_feats(min(len(sl), 8), G_, 64, torch.float16, "gauss").numpy(), ro[:8], co[:8], G_, torch.float16, fault="rect")
        assert torch.equal(got, rect)                       # the mask test inside the rectangle never rejects a cell
        cnt = ref.reshape(len(sl), -1).sum(-1)
        assert (cnt == 0).any()
        if boxes == "boxes":
            assert (cnt == 1).sum() >= 3 and (cnt == G_ * G_).any()
            assert len({int(c) for c in cnt if c > 1 and (c & (c - 1)) == 0}) >= 2, sorted(set(cnt.tolist()))
        for f in TR.MASK_FAULTS:
            fr, fc = TR.region_lines(sl, G_, image, fault=f)
            if not np.array_equal(TR.lines_mask(fr, fc), ref):
                caught[f].append(shape[:3])
    print(caught)
    assert all(caught.values()), caught
    assert (64, 64, 64) in caught["zero_tap"] and (6, 28, 64) in caught["swap"] and (6, 28, 64) in caught["inclusive"]


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", TR.REGION_SHAPES, ids=REGION_IDS)
def test_region_pool_emulation_bound_and_faults(shape, dtype):
    G_, image, D, boxes = shape
    sl, mask = _region_case(shape)
    ro, co = TR.region_lines(sl, G_, image)
    cnt = mask.reshape(len(sl), -1).sum(-1)
    for kind in ("gauss", "int"):
        x = TR.region_feats(len(sl), G_, D, dtype, kind)
        assert G.representable(x, dtype)
        ref, bound = TR.region_pool_ref(x, mask, dtype)
        got = TR.region_pool_f32(x.numpy(), ro, co, G_, dtype)
        r, bad = _ratio(got.double(), ref, bound)
        print(f"[pool emulation {shape[:3]} {kind}] worst err / bound {float(r.max()):.3f}")
        assert not bool(bad.any())
        assert not bool(got[torch.from_numpy(cnt == 0)].float().any())                              # an empty box: exactly zero
        one = np.nonzero(cnt == 1)[0]
        for b in one:
            assert torch.equal(got[b], G.rne_op(x[b, int(np.argmax(mask[b].reshape(-1)))], dtype))
        if kind == "int":
            p2 = torch.from_numpy((cnt > 0) & ((cnt & (cnt - 1)) == 0))
            assert (bool(p2.any()) or boxes != "boxes") and float(x.abs().max()) <= 8 and bool((x == x.round()).all())
            assert 8 * int(cnt.max()) < 2 ** 24             # x 2^-k is exact and every partial sum a multiple of 2^-k below 8: any order gives the mean
            assert torch.equal(got[p2], G.rne_op(ref[p2], dtype))                                    # exact mean, one store rounding
        bad_b = _ratio(TR.region_pool_f32(x.numpy(), ro, co, G_, dtype, fault="count_plus1").double(), ref, bound)[1].any(-1).numpy()
        live = cnt > 0                                      # count / (count + 1) is within the store's half ulp once count is in the hundreds
        print(f"[pool fault count + 1 {shape[:3]} {kind}] {int(bad_b[live].sum())} of {int(live.sum())} boxes flagged")
        assert int(bad_b[live].sum()) * 2 >= int(live.sum()), "divisor count + 1 not flagged in half of the boxes"
        fr, fc = TR.region_lines(sl, G_, image, fault="swap")
        swapped = _ratio(TR.region_pool_f32(x.numpy(), fr, fc, G_, dtype).double(), ref, bound)[1]
        assert bool(swapped.any())


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("key", sorted(TR.LOC_N), ids=lambda k: "x".join(map(str, k)))
def test_location_layer_emulation_bound_and_split(key, dtype):
    G_, image, D = key
    loc_n, slabs = TR.LOC_N[key], D // 64
    B = len(TR.region_slices(G_, image, [s[3] for s in TR.REGION_SHAPES if s[:3] == key][0]))
    for kind in ("int", "gauss"):
        c, w, b = TR.loc_problem(B, loc_n, dtype, kind)
        assert G.representable(w, dtype) and not bool(w[:, 4:].any())
        ref, bound = TR.loc_ref(c, w, b, dtype)
        got = TR.loc_f32(c.numpy(), w.numpy(), b.numpy(), dtype, slabs)
        r, bad = _ratio(got.double(), ref, bound)
        print(f"[loc emulation loc_n={loc_n} slabs={slabs} {kind}] worst err / bound {float(r.max()):.3f}")
        assert not bool(bad.any())
        if kind == "int":
            pre = (c.double().abs() @ w.double().abs()[:, :4].T + b.double().abs())
            assert float(pre.max()) < 2 ** 24 and bool((c == c.round()).all()) and float(c.max()) <= 336 and float(c.max()) > 256
            assert torch.equal(got, G.rne_op(ref, dtype).float()) and bool((ref > 0).any()) and bool((ref == 0).any())
        floor = _ratio(TR.loc_f32(c.numpy(), w.numpy(), b.numpy(), dtype, slabs, fault="per_floor").double(), ref, bound)[1]
        assert bool(floor.any()) == (loc_n % slabs != 0)
    assert any(TR.LOC_N[k] % (k[2] // 64) for k in TR.LOC_N)                                       # one launch has a split that does not divide
