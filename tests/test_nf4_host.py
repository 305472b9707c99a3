"""NF4 (load_4bit) on the host: the numpy restatement of the format (tests/nf4_ref.py) against bitsandbytes' constants, and the ABI that
carries the 4-bit kernels (include/vitron_hip.h vt_nf4_*), in both operand builds. No GPU needed."""
import os
import re

import numpy as np
import pytest

from tests import nf4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_midpoints_are_the_fp32_midpoints_of_the_codebook():
    mids = ((R.CODEBOOK[:-1].astype(np.float64) + R.CODEBOOK[1:].astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mids, R.MIDPOINTS)
    assert np.all(np.diff(R.CODEBOOK) > 0) and R.CODEBOOK[7] == 0.0 and R.CODEBOOK[0] == -1.0 and R.CODEBOOK[15] == 1.0


def test_packing_order_and_exact_codebook_values():
    # a row whose absmax is 1 and whose elements are the codebook values themselves: codes 0..15, twice, then reversed
    vals = np.concatenate([R.CODEBOOK, R.CODEBOOK, R.CODEBOOK[::-1], R.CODEBOOK[::-1]]).astype(np.float16).astype(np.float32)
    codes, absmax = R.quantize(vals[None, :])
    assert absmax.tolist() == [1.0]
    got = R.unpack(codes)
    want = np.concatenate([np.arange(16), np.arange(16), np.arange(15, -1, -1), np.arange(15, -1, -1)])
    # fp16 rounding of the codebook values can only move a value onto the nearer side of its own interval, never past a midpoint
    assert np.array_equal(got, want)
    assert codes[0] == (0 << 4) | 1 and codes[8] == (0 << 4) | 1 and codes[16] == (15 << 4) | 14   # element 2j in the HIGH nibble


def test_zero_block_and_mixed_rows():
    w = np.zeros((2, 128), np.float32)
    w[1, 64:] = np.linspace(-2, 3, 64)
    codes, absmax = R.quantize(w)
    assert absmax.tolist()[:3] == [0.0, 0.0, 0.0] and absmax[3] == np.float32(3.0)
    u = R.unpack(codes).reshape(2, 128)
    assert np.all(u[0] == 7) and np.all(u[1, :64] == 7)
    d = R.dequantize_f32(codes, absmax, 2, 128)
    assert np.all(np.isfinite(d)) and np.all(d[0] == 0) and d[1, 127] == 3.0 and d[1, 64] == R.CODEBOOK[1] * np.float32(3.0)   # -2/3 -> code 1


@pytest.mark.parametrize("i", range(15))
def test_values_at_midpoints_and_one_ulp_around(i):
    """strict '>': a normalised value exactly on a midpoint goes DOWN, one fp32 ulp above goes up, one below stays down. absmax = 1 (the
    block's first element is 1.0), so the normalised value is the element itself -- elements are given as fp32 that fp16 represents."""
    t = R.MIDPOINTS[i]
    # pick fp16-representable values around the midpoint: the fp16 grid is what the quantiser sees
    h = np.float16(t)
    lo = np.nextafter(h, np.float16(-2)) if np.float32(h) > t else h
    while np.float32(lo) > t:
        lo = np.nextafter(lo, np.float16(-2))
    hi = np.nextafter(lo, np.float16(2))
    row = np.zeros(64, np.float32)
    row[0] = 1.0
    row[1], row[2] = np.float32(lo), np.float32(hi)
    codes, absmax = R.quantize(row[None, :])
    u = R.unpack(codes)
    assert np.float32(lo) <= t < np.float32(hi)
    assert u[1] == i and u[2] == i + 1
    # the comparison itself, in fp32, at the midpoint and one fp32 ulp on each side
    for v, want in ((t, i), (np.nextafter(t, np.float32(2)), i + 1), (np.nextafter(t, np.float32(-2)), i)):
        assert int(np.sum(np.float32(v) > R.MIDPOINTS)) == want


def test_signatures_carry_the_nf4_entry_points():
    from vitron_amd import _lib
    for name in ("vt_nf4_quant", "vt_nf4_dequant", "vt_gemm_nf4"):
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 114
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr)
    names = [f[0] for f in _lib.VtLlamaLayer._fields_]
    assert names[-8:] == ["wqkv_nf4", "wqkv_absmax", "wo_nf4", "wo_absmax", "wgu_nf4", "wgu_absmax", "wdown_nf4", "wdown_absmax"]


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_libraries_export_the_nf4_entry_points_and_check_arguments(operand):
    from vitron_amd import _lib
    lib = _lib.load(operand=operand)
    for name in ("vt_nf4_quant", "vt_nf4_dequant", "vt_gemm_nf4"):
        assert hasattr(lib, name), name
    # argument errors come back as status -1 + message, without touching the GPU
    assert lib.vt_gemm_nf4(None, 64, None, None, None, 64, 1, 32, 128, 0, None, 0, 0.0, 0.0, None, None, 0, None, None) == -1
    assert "null" in _lib.last_error(lib)
    assert lib.vt_gemm_nf4(8, 64, 8, 8, 8, 64, 33, 32, 128, 0, None, 0, 0.0, 0.0, None, None, 0, None, None) == -1   # M > 32
    assert "M <= 32" in _lib.last_error(lib)
    assert lib.vt_nf4_quant(8, 1, 96, 4, 96, 8, 8, None) == -1                                                     # K % 64 != 0
    assert lib.vt_nf4_dequant(8, 8, 4, 100, 8, 100, None) == -1


def test_load_8bit_still_refused_and_4bit_flag_reaches_the_model():
    import inspect

    from vitron_amd.model import builder
    with pytest.raises(NotImplementedError):
        builder.load_pretrained_model("synthetic", None, "x", load_8bit=True)
    assert "load_4bit" in inspect.signature(builder.load_pretrained_model).parameters
    from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    assert LlavaLlamaForCausalLM(LlavaConfig()).weight_format == "16bit"


# ---- nf4_ref.random_nf4 and nf4_ref.gemm_bound (the GPU GEMM tests' input and limit) -------------------------------------------------
def test_random_nf4_covers_every_byte_and_spreads_fp16_scales():
    codes, absmax = R.random_nf4(64, 1024, 3)
    assert codes.dtype == np.uint8 and codes.size == 64 * 512 and absmax.dtype == np.float32 and absmax.size == 64 * 16
    assert np.unique(codes).size == 256                                       # every (high, low) code pair
    assert np.array_equal(absmax, absmax.astype(np.float16).astype(np.float32))  # fp16 values, as a real absmax
    e = np.floor(np.log2(absmax))
    assert e.min() == -12 and e.max() == 3 and np.unique(e).size == 16
    assert np.abs(np.diff(e)).max() >= 10                                     # neighbouring blocks far apart in scale
    d = R.dequantize_f32(codes, absmax, 64, 1024)
    assert np.any((d != 0) & (np.abs(d) < 2.0 ** -14))                         # fp16 subnormal weights at the low end
    c2, a2 = R.random_nf4(64, 1024, 3)
    assert np.array_equal(codes, c2) and np.array_equal(absmax, a2)


def test_half_ulp():
    assert R.half_ulp(np.array([1.0]), "bf16")[0] == 2.0 ** -8 and R.half_ulp(np.array([1.0]), "fp16")[0] == 2.0 ** -11
    assert R.half_ulp(np.array([3.0]), "bf16")[0] == 2.0 ** -7 and R.half_ulp(np.array([2.0 ** -20]), "fp16")[0] == 2.0 ** -25


def _op16(x, fmt):
    import torch
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[fmt]
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).double().numpy()


def _bound_case(fmt, K, N=96, M=8, seed=5, log2_range=(-12, 4)):
    codes, absmax = R.random_nf4(N, K, seed, log2_range)
    wd = _op16(R.dequantize_f32(codes, absmax, N, K), fmt)
    a = _op16(np.random.default_rng(seed + 1).standard_normal((M, K)), fmt)
    return codes, absmax, wd, a


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("K", [128, 1152, 4096])
def test_gemm_bound_holds_for_a_cpu_fp32_gemm(fmt, K):
    """an fp32 product of the same operands (another summation order, then the kernels' epilogue arithmetic in fp32) stays inside the bound,
    in every epilogue; the bound is far below the values, and the 16-bit store term dominates it"""
    _, _, wd, a = _bound_case(fmt, K)
    y32 = a.astype(np.float32) @ wd.astype(np.float32).T
    # EPI_F32
    ref = R.gemm_ref(a, wd)
    bnd = R.gemm_bound(a, wd, K)
    assert np.all(np.abs(y32 - ref) <= bnd) and np.all(bnd <= 1e-3 * (np.abs(a) @ np.abs(wd).T))
    # EPI_BF16 (operand out)
    assert np.all(np.abs(_op16(y32, fmt) - ref) <= R.gemm_bound(a, wd, K, store=fmt))
    # EPI_F32_RESID
    r = np.random.default_rng(9).standard_normal(ref.shape).astype(np.float32) * 4
    assert np.all(np.abs((r + y32) - R.gemm_ref(a, wd, resid=r)) <= R.gemm_bound(a, wd, K, resid=r))
    # folded RMSNorm consumer: an fp32 rstd one part in 2^20 off the fp64 one
    rs = np.linspace(0.01, 3.0, a.shape[0])
    rs32 = (rs * (1 + 2.0 ** -20)).astype(np.float32)
    assert np.all(np.abs(_op16(y32 * rs32[:, None], fmt) - R.gemm_ref(a, wd, rscale=rs)) <=
                  R.gemm_bound(a, wd, K, rscale=rs, rscale_rel=2.0 ** -19, store=fmt))
    # SwiGLU (gate / up scales below 1, as the GPU test's, so that silu(g) * u stays inside fp16)
    _, _, wd, a = _bound_case(fmt, K, log2_range=(-12, 0))
    y32 = a.astype(np.float32) @ wd.astype(np.float32).T
    g32 = y32.reshape(a.shape[0], -1, 2, 16)
    with np.errstate(over="ignore"):                                           # exp(-g) = inf -> silu = -0, as on the GPU
        s32 = g32[:, :, 0] * (np.float32(1) / (np.float32(1) + np.exp(-g32[:, :, 0])))
    sw = _op16((s32 * g32[:, :, 1]).reshape(a.shape[0], -1), fmt)
    assert np.all(np.abs(sw - R.gemm_ref(a, wd, swiglu=True)) <= R.gemm_bound(a, wd, K, swiglu=True, store=fmt))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_gemm_bound_catches_one_wrong_block_scale(fmt):
    """the weights the kernel would use if it read one block's absmax twice as large, or its neighbour's, fall outside the bound in that
    block's column -- and only there. (The row's largest block: an error confined to a block 2^16 below its row's largest is inside the
    accumulation bound of that row; the GPU tests' exact unit probes see every element on its own.)"""
    K, N = 1152, 96
    codes, absmax, wd, a = _bound_case(fmt, K)
    ref, bnd = R.gemm_ref(a, wd), R.gemm_bound(a, wd, K, store=fmt)
    kpr = K // 64
    for n in (0, 37, 95):
        row = absmax[n * kpr:(n + 1) * kpr]
        b = int(np.argmax(row))
        for wrong in (row[b] * 2, row[b - 1] if b else row[b + 1]):
            if wrong == row[b]:
                continue
            bad = absmax.copy()
            bad[n * kpr + b] = wrong
            got = _op16(R.gemm_ref(a, _op16(R.dequantize_f32(codes, bad, N, K), fmt)), fmt)
            out = np.abs(got - ref) > bnd
            assert out[:, n].any(), (n, b)
            assert not np.delete(out, n, axis=1).any()
