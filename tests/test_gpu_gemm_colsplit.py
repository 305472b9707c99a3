"""One GEMM as two launches over column ranges (vt_gemm_bf16_colsplit through ops.gemm(colsplit=...); vitron_amd/csrc/vt_gemm.hip
vt_gemm_colsplit_launch -- the code the planner's own column splits run through), forced at small shapes in both operand builds:

  M in {320, 640, 700}: one 320-row block, two, and a ragged last block;  N = 1024 split at 256, 512 and 768;
  first range on the 320-row or the 224-row four-wave tile, second range on the 256-row tile;
  bf16 store with a bias, SwiGLU, fp32 residual into a pre-filled C.

Each split result is compared BIT FOR BIT with the single launch of the same call on 256-row tiles (tile height changes neither the K order
nor the epilogue), held to the per-element bound of tests/gemm_ref.py against the fp64 reference, and written into a window of a NaN-filled
buffer whose every other bit must survive while the window -- the seam column included -- holds no NaN.

K: the four-wave tiles document K % 128 == 0 and K >= 256 (include/vitron_hip.h; gemm_ref.k_rule), so the shortest loop and a three-step one
are K = 256 and 384. K = 128 and 192 are not legal for them: there the forced split must refuse before any launch and leave C untouched
(test_short_k_is_refused_before_any_launch).

test_planned_split_at_the_gate_up_shape: plain AUTO at 5120 x 22016, where the planner splits (K = 4096, the measured shape) and where it
does not (K = 2048: only measured shapes change plans), against the forced single-grid launch."""
import functools

import pytest
import torch

from tests import gemm_ref as G
from tests.gemm_ref import EPI_BF16, EPI_F32_RESID, EPI_SWIGLU
from tests.test_gpu_gemm import COL0, DT_IDS, GAP, NAN, Problem, _bits, _exact, _within

pytestmark = pytest.mark.gpu
W4, W4_320, W4_224 = 13, 14, 16
N = 1024
MS, N1S, KS, FIRSTS = (320, 640, 700), (256, 512, 768), (256, 384), (W4_320, W4_224)


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


def _run(dev, pb, epi, cfg, colsplit=None, bias=True):
    """as test_gpu_gemm._launch, with the forced split: C = a window of a NaN-filled buffer (EPI_F32_RESID: holding the residual); every bit
    outside the window must survive and the window must hold no NaN"""
    from vitron_amd import ops
    n_out = pb.N // 2 if epi == EPI_SWIGLU else pb.N
    odt = torch.float32 if epi == EPI_F32_RESID else pb.dtype
    cbuf = torch.full((GAP + pb.M + 3, COL0 + n_out + 12), NAN, dtype=odt, device=dev)
    win = cbuf[GAP:GAP + pb.M, COL0:COL0 + n_out]
    if epi == EPI_F32_RESID:
        win.copy_(pb.resid)
    before = _bits(cbuf).clone()
    ops.gemm(pb.a, pb.w, pb.bias if bias else None, epi, out=win, cfg=cfg, colsplit=colsplit)
    torch.cuda.synchronize()
    same = _bits(cbuf) == before
    same[GAP:GAP + pb.M, COL0:COL0 + n_out] = True
    if not bool(same.all()):
        r, c = (~same).nonzero()[0].tolist()
        raise AssertionError(f"written outside the {pb.M} x {n_out} window: {int((~same).sum())} elements, first at window row {r - GAP}, column {c - COL0}")
    got = win.cpu()
    nan = torch.isnan(got.float())
    if bool(nan.any()):
        r, c = nan.nonzero()[0].tolist()
        raise AssertionError(f"{int(nan.sum())} NaN in the window (never written, or padding leaked in), first at ({r}, {c})")
    return got


@functools.lru_cache(maxsize=None)
def _gauss(dtype, M, K):
    """(a, w, bias, resid, fp64 reference without the residual, summation bound): computed once per shape and build, read only"""
    a, w, bias, resid = G.gauss_operands(M, N, K, dtype, M * 7 + K)
    assert G.bound_covers_epilogue(a, w, bias, resid)
    return a, w, bias, resid, a.double() @ w.double().t() + bias.double(), G.sum_bound(a, w)


@functools.lru_cache(maxsize=None)
def _swiglu(M, K):
    """(a, w, fp64 reference, bound): integer operands, so gate and up are exact fp32 numbers and the only errors are the SiLU's and the store's"""
    a, w, _ = G.act_operands(M, N, K, M + 3 * K)
    g, up = G.swiglu_split(G.exact_epilogue(a, w)[0])
    return a, w, torch.from_numpy(G.silu64(g.numpy()) * up.numpy()), torch.from_numpy(G.e_swiglu(g.numpy(), up.numpy()))


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_forced_split_equals_the_single_launch(dev, dtype, M, K):
    assert all(G.legal(c, M, n, K, EPI_SWIGLU) for c in (W4, W4_320, W4_224) for n in (256, 512, 768, N))
    a, w, bias, resid, ref, sb = _gauss(dtype, M, K)
    pb = Problem(dev, dtype, a, w, bias, resid)
    ai, wi, ref_s, e_s = _swiglu(M, K)
    pbs = Problem(dev, dtype, ai, wi)
    single = {EPI_BF16: _run(dev, pb, EPI_BF16, W4), EPI_F32_RESID: _run(dev, pb, EPI_F32_RESID, W4), EPI_SWIGLU: _run(dev, pbs, EPI_SWIGLU, W4, bias=False)}
    _within(single[EPI_BF16], ref, sb + G.store_half_ulp(ref, dtype), "single, EPI_BF16 + bias")
    _within(single[EPI_F32_RESID], ref + resid.double(), sb, "single, EPI_F32_RESID")
    _within(single[EPI_SWIGLU], ref_s, e_s + G.store_half_ulp(ref_s, dtype), "single, SwiGLU")
    for first in FIRSTS:
        for N1 in N1S:
            what = f"{M}x{N}x{K}: columns [0, {N1}) on cfg {first}, the rest on cfg {W4}"
            got = _run(dev, pb, EPI_BF16, first, (N1, W4))
            _exact(got, single[EPI_BF16], what + ", EPI_BF16 + bias")
            _within(got, ref, sb + G.store_half_ulp(ref, dtype), what + ", EPI_BF16 + bias")
            got = _run(dev, pb, EPI_F32_RESID, first, (N1, W4))
            _exact(got, single[EPI_F32_RESID], what + ", EPI_F32_RESID")
            _within(got, ref + resid.double(), sb, what + ", EPI_F32_RESID")
            got = _run(dev, pbs, EPI_SWIGLU, first, (N1, W4), bias=False)                  # the output seam is column N1 / 2
            _exact(got, single[EPI_SWIGLU], what + ", SwiGLU")
            _within(got, ref_s, e_s + G.store_half_ulp(ref_s, dtype), what + ", SwiGLU")


def test_rest_planned_again_equals_the_single_launch(dev):
    """cfg_rest = AUTO: the remaining columns go through the planner as a GEMM of their own"""
    dtype, M, K = torch.bfloat16, 700, 384
    a, w, bias, resid, ref, sb = _gauss(dtype, M, K)
    pb = Problem(dev, dtype, a, w, bias, resid)
    _exact(_run(dev, pb, EPI_BF16, W4_320, (512, 0)), _run(dev, pb, EPI_BF16, W4), "rest on AUTO, EPI_BF16 + bias")
    _exact(_run(dev, pb, EPI_F32_RESID, W4_224, (768, 0)), _run(dev, pb, EPI_F32_RESID, W4), "rest on AUTO, EPI_F32_RESID")


@pytest.mark.parametrize("K", (128, 192))
def test_short_k_is_refused_before_any_launch(dev, K):
    """K = 128 / 192 with a four-wave first range (K % 128 == 0 and K >= 256 documented), and column counts that are no split at all: an error
    before the first launch, C keeps its bits"""
    from vitron_amd import ops
    from vitron_amd._lib import VitronHipError
    dtype, M = torch.bfloat16, 320
    a, w = torch.ones((M, K), dtype=dtype, device=dev), torch.ones((N, K), dtype=dtype, device=dev)
    c = torch.full((M, N), NAN, dtype=dtype, device=dev)
    for first in FIRSTS:
        for N1 in N1S:
            with pytest.raises(VitronHipError):
                ops.gemm(a, w, None, EPI_BF16, out=c, cfg=first, colsplit=(N1, W4))
    for N1 in (0, 128, N, N + 256, -256):
        with pytest.raises(VitronHipError):
            ops.gemm(a, w, None, EPI_BF16, out=c, cfg=5, colsplit=(N1, 5))
    torch.cuda.synchronize()
    assert bool(torch.isnan(c.float()).all()), "C was written"


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_planned_split_at_the_gate_up_shape(dev, dtype):
    """gate/up of the headline prefill (5120 x 22016, SwiGLU) through plain AUTO: at K = 4096 the planner runs 48 column tiles on 320-row tiles
    + 38 on 256-row tiles, at K = 2048 (not a measured shape) the single grid of 256-row tiles; both are the forced single-grid launch bit for
    bit. Operands are drawn on the device (small integers: every sum exact) and compared there."""
    from vitron_amd import ops
    M, NN = 5120, 22016
    assert ops.gemm_plan_split(M, NN, 4096, EPI_SWIGLU) == (W4_320, 0, 12288, W4) and ops.gemm_plan_split(M, NN, 2048, EPI_SWIGLU) == (W4, 0, 0, 0)
    g = torch.Generator(device=dev).manual_seed(11)
    a = torch.randint(-2, 3, (M, 4096), generator=g, device=dev).to(dtype)
    w = torch.randint(-1, 2, (NN, 4096), generator=g, device=dev).to(dtype)
    a[:, ::3] = 0                                                        # keeps |gate|, |up| small enough for a SiLU away from saturation
    for K in (2048, 4096):
        got = ops.gemm(a[:, :K], w[:, :K], None, EPI_SWIGLU)
        want = ops.gemm(a[:, :K], w[:, :K], None, EPI_SWIGLU, cfg=W4)
        forced = ops.gemm(a[:, :K], w[:, :K], None, EPI_SWIGLU, cfg=W4_320, colsplit=(12288, W4))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(want.float()).any()) and float(want.float().abs().max()) > 0
        assert torch.equal(_bits(got), _bits(want)), f"AUTO differs from the single grid at K = {K}"
        assert torch.equal(_bits(forced), _bits(want)), f"the forced split differs from the single grid at K = {K}"
