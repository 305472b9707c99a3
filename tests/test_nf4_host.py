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
