"""The FP8 (e4m3) KV cache without a GPU: the host restatement tests/kv8_ref.py against the format's definition (round to nearest even at
every code midpoint, subnormals, saturation), the exact inverse, the page layout, the fp64 bound of the fp8 decode kernels on an fp32
attention over e4m3 operands (and the three mutants it must catch), the C ABI's six new entry points (header, SIGNATURES, both libraries,
argument errors as status -1), and the Python switch (config.kv_cache_dtype parsing, refusals that need no device)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import attn_ref as R
from tests import kv8_ref as K8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = {"vt_kv8_quant", "vt_kv8_dequant", "vt_attn_decode_kv8", "vt_attn_decode_fused_kv8", "vt_llama_workspace_bytes_kv8",
                    "vt_llama_forward_kv8"}


def _f32_neighbours(x):
    x = np.asarray(x, np.float32)
    return np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))


def test_e4m3_table_is_the_ocp_format():
    v = K8.E4M3
    assert v[0x00] == 0.0 and v[0x80] == 0.0 and np.signbit(v[0x80])
    assert v[0x01] == 2.0 ** -9 and v[0x07] == 7 * 2.0 ** -9 and v[0x08] == 2.0 ** -6          # subnormals, smallest normal
    assert v[0x38] == 1.0 and v[0x7e] == 448.0 and v[0xfe] == -448.0
    assert np.isnan(v[0x7f]) and np.isnan(v[0xff]) and np.isfinite(v).sum() == 254 and K8.FINITE_CODES.size == 254
    assert (np.diff(v[:127]) > 0).all()                                                       # codes order like their values
    # every finite value is a bf16 and an fp16 value: dequantisation is exact in both operand formats
    t = torch.from_numpy(v[K8.FINITE_CODES.astype(np.int64)])
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(t.to(dt).to(torch.float64), t)


def test_quant_rounds_to_nearest_even_at_every_midpoint():
    """kv8_ref.quant (torch float8_e4m3fn behind the +-448 clamp) against the table: at every code value, at the midpoint of every pair of
    neighbouring codes (exact in fp32) and one fp32 ulp to each side, both signs."""
    pos = K8.E4M3[:127]
    mids = (pos[:-1] + pos[1:]) / 2
    pts = np.concatenate([pos, mids]).astype(np.float32)
    assert (pts.astype(np.float64) == np.concatenate([pos, mids])).all()
    xs = np.concatenate(_f32_neighbours(pts))
    xs = np.concatenate([xs, -xs])
    got = K8.quant(torch.from_numpy(xs)).numpy()
    want = K8.quant_table(xs)
    assert (got == want).all(), [(float(x), hex(g), hex(w)) for x, g, w in zip(xs[got != want][:5], got[got != want], want[got != want])]
    # ties go to the even code
    assert K8.quant(torch.tensor([mids[0], mids[1], mids[8]])).tolist() == [0x00, 0x02, 0x08]
    assert K8.quant(torch.tensor([2.0 ** -10])).item() == 0x00                        # the tie between 0 and 2^-9 goes to 0
    assert K8.quant(torch.tensor([float(np.nextafter(np.float32(2.0 ** -10), np.float32(1)))])).item() == 0x01
    assert K8.quant(torch.tensor([-2.0 ** -10])).item() == 0x80


def test_quant_saturates_and_never_makes_a_nan_from_a_number():
    x = torch.tensor([448.0, 449.0, 464.0, 465.0, 1e4, 65504.0, float("inf"), 3e38])
    assert K8.quant(x).tolist() == [0x7e] * 8 and K8.quant(-x).tolist() == [0xfe] * 8
    assert (K8.quant_table(x.numpy()) == 0x7e).all()
    assert K8.quant(torch.tensor([float("nan")])).item() & 0x7f == 0x7f
    # through both 16-bit formats (the values a cache can hold)
    for dt in (torch.bfloat16, torch.float16):
        assert K8.quant(torch.tensor([464.0, 65504.0, float("inf")]).to(dt)).tolist() == [0x7e] * 3
    assert K8.quant(torch.tensor([0.0])).item() == 0x00


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_dequant_then_quant_is_the_identity_on_all_finite_codes(dtype):
    codes = torch.from_numpy(K8.FINITE_CODES.copy())
    vals = K8.dequant(codes, dtype)
    assert torch.equal(vals.to(torch.float64), torch.from_numpy(K8.E4M3[K8.FINITE_CODES.astype(np.int64)]))
    assert torch.equal(K8.quant(vals), codes)
    assert (K8.quant_table(vals.to(torch.float64).numpy()) == K8.FINITE_CODES).all()


def test_quant_matches_the_table_on_every_16_bit_pattern():
    """every bf16 and fp16 bit pattern (NaNs left out): the torch conversion equals the table restatement"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    for dt in (torch.bfloat16, torch.float16):
        x = bits.view(dt)
        keep = ~torch.isnan(x)
        got = K8.quant(x[keep]).numpy()
        want = K8.quant_table(x[keep].to(torch.float64).numpy())
        assert (got == want).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hd", [64, 128])
def test_page_layout_round_trips_and_is_the_quantised_16_bit_layout(dtype, hd):
    g = torch.Generator().manual_seed(hd)
    heads, L = 3, 150
    k = torch.randn((L, heads, hd), generator=g) * 3
    v = torch.randn((L, heads, hd), generator=g) * 3
    table = [4, 0, 2]
    k8, v8 = K8.pack_pages8(k, v, table, heads, hd, dtype, npages=6, fill=0x55)
    kb, vb = K8.unpack_pages8(k8, v8, table, L, heads, hd)
    assert torch.equal(kb, K8.quant(R.to_op(k, dtype))) and torch.equal(vb, K8.quant(R.to_f16_page(v)))
    # == quant(pack_pages) on the table's pages, padding (zero) included; other pages keep the fill
    kp, vp = R.pack_pages(k, v, table, heads, hd, dtype, npages=6)
    used = torch.zeros(6, dtype=torch.bool)
    used[table] = True
    assert torch.equal(k8.view(6, -1)[used], K8.quant(kp).view(6, -1)[used])
    assert torch.equal(v8.view(6, -1)[used], K8.quant(vp).view(6, -1)[used])
    assert (k8.view(6, -1)[~used] == 0x55).all() and (v8.view(6, -1)[~used] == 0x55).all()
    # element addresses: key j, head h, element d
    j, h, d = 70, 1, 5
    assert k8[(table[1] * heads + h) * 64 * hd + (j - 64) * hd + d] == kb[j, h, d]
    assert v8[(table[1] * heads + h) * 64 * hd + d * 64 + (j - 64)] == vb[j, h, d]
    tail = k8.view(6, heads, 64, hd)[table[2], :, L - 128:]
    assert (tail == 0).all()


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 700, 2049, 8192])
def test_fp32_attention_over_e4m3_operands_stays_inside_the_bound(L):
    """An fp32 tile-by-tile attention over e4m3-valued K / V is inside kv8_ref.decode_bound of the fp64 reference (N(0,1) data, both
    output formats); prints the highest error-to-bound ratio."""
    hd, heads = 128, 2
    g = torch.Generator().manual_seed(L)
    q = R.to_op(torch.randn((heads, hd), generator=g), torch.float16)
    k8 = K8.quant(torch.randn((L, heads, hd), generator=g))
    v8 = K8.quant(torch.randn((L, heads, hd), generator=g))
    scale = 1 / math.sqrt(hd)
    ref = K8.decode_ref(q, k8, v8, scale)
    got = K8.attend_f32(q, k8, v8, scale)
    worst = 0.0
    for store, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        bound = K8.decode_bound(q, k8, v8, scale, store)
        err = (got.to(dt).to(torch.float64) - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"L={L} {store}: ratio {float((err / bound).max()):.3f}"
    print(f"kv8 bound, L={L}: highest error / bound {worst:.3f}")


@pytest.mark.parametrize("mutant", ["dropped_key", "padding_key", "wrong_tile"])
def test_the_bound_catches_a_dropped_a_padding_and_a_wrong_tile_key(mutant):
    hd, heads, L = 128, 2, 200
    g = torch.Generator().manual_seed(7)
    q = R.to_op(torch.randn((heads, hd), generator=g), torch.float16)
    k8 = K8.quant(torch.randn((L, heads, hd), generator=g))
    v8 = K8.quant(torch.randn((L, heads, hd), generator=g))
    scale = 1 / math.sqrt(hd)
    ref = K8.decode_ref(q, k8, v8, scale)
    bound = K8.decode_bound(q, k8, v8, scale, "fp16")
    kw = {"dropped_key": dict(drop=137), "padding_key": dict(extra_pad=1), "wrong_tile": dict(swap_tile=(1, 2))}[mutant]
    got = K8.attend_f32(q, k8, v8, scale, **kw).to(torch.float16).to(torch.float64)
    assert ((got - ref).abs() > bound).any()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_the_six_entry_points_are_declared_bound_and_exported(operand):
    from vitron_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(vt_\w+)\s*\(", hdr, flags=re.M))
    assert NEW_ENTRY_POINTS <= declared and NEW_ENTRY_POINTS <= set(_lib.SIGNATURES)
    assert "typedef struct vt_kv_cache8" in hdr
    lib = _lib.load(operand=operand)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 114 and lib.vt_version() == 114 and "#define VT_ABI_VERSION 114" in hdr
    assert [f[0] for f in _lib.VtKvCache8._fields_] == ["k", "vt", "num_pages"]


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_argument_errors_come_back_as_status_minus_one_without_a_gpu(operand):
    from vitron_amd import _lib
    lib = _lib.load(operand=operand)
    one = C.c_void_p(64)      # a non-null pointer that is never dereferenced: every check below fails before a launch
    assert lib.vt_kv8_quant(None, None, None, None, None, None, 1, 2, 128, None) == -1 and "null" in _lib.last_error(lib)
    assert lib.vt_kv8_dequant(None, None, None, None, None, None, 1, 2, 128, None) == -1 and "null" in _lib.last_error(lib)
    assert lib.vt_kv8_quant(one, one, one, one, one, one, 1, 2, 48, None) == -1 and "head_dim 48" in _lib.last_error(lib)
    assert lib.vt_kv8_dequant(one, one, one, one, one, one, 1, 2, 48, None) == -1 and "head_dim 48" in _lib.last_error(lib)
    assert lib.vt_attn_decode_kv8(None, 128, None, None, None, None, 1, None, 128, 1, 128, 0.1, 64, None, 0, None) == -1
    assert "null" in _lib.last_error(lib)
    assert lib.vt_attn_decode_kv8(one, 48, one, one, one, one, 1, one, 48, 1, 48, 0.1, 64, one, 1 << 20, None) == -1
    assert "head_dim 48" in _lib.last_error(lib)
    assert lib.vt_attn_decode_fused_kv8(None, 384, 0, 128, 256, None, None, None, None, 1, None, 128, 1, 128, 0.1, None, None, None, None) == -1
    assert "null" in _lib.last_error(lib)
    assert lib.vt_attn_decode_fused_kv8(one, 144, 0, 48, 96, one, one, one, one, 1, one, 48, 1, 48, 0.1, None, None, None, None) == -1
    assert "head_dim 48" in _lib.last_error(lib)
    # the decoder pass: a null pool, and the modes that read or write 16-bit pages
    m = _lib.VtLlamaModel()
    m.hidden, m.heads, m.head_dim, m.intermediate, m.num_layers, m.vocab = 256, 2, 128, 512, 1, 64
    kv = _lib.VtKvCache8()
    kv.k, kv.vt, kv.num_pages = 64, 64, 4
    args = (one, 1, one, one, 1, 1, 1, 1, one, 1, one, 1, one, None, one, 1 << 20, None)
    assert lib.vt_llama_forward_kv8(C.byref(m), None, *args) == -1 and "null" in _lib.last_error(lib)
    for field, word in (("precise_qk", "precise level 1"), ("qkv_fuse", "qkv_fuse")):
        setattr(m, field, 1)
        assert lib.vt_llama_forward_kv8(C.byref(m), C.byref(kv), *args) == -1
        assert word in _lib.last_error(lib) and "fp8" in _lib.last_error(lib)
        setattr(m, field, 0)
    m.head_dim, m.heads = 48, 2
    m.hidden = 96
    m.rope_cos = m.rope_sin = 64
    assert lib.vt_llama_forward_kv8(C.byref(m), C.byref(kv), *args) == -1 and "head_dim 48" in _lib.last_error(lib)
    # the staging pool is part of the fp8 workspace of a prefill, and of nothing else
    m.hidden, m.heads, m.head_dim = 256, 2, 128
    tile = 2 * 64 * 128 * 2
    base = lib.vt_llama_workspace_bytes(C.byref(m), 100, 1, 1, 100)
    assert lib.vt_llama_workspace_bytes_kv8(C.byref(m), 100, 1, 1, 100, 2) >= base + 2 * 2 * tile
    assert lib.vt_llama_workspace_bytes_kv8(C.byref(m), 4, 4, 4, 100, 8) == lib.vt_llama_workspace_bytes(C.byref(m), 4, 4, 4, 100)


# ---- Python switch ---------------------------------------------------------------------------------------------------------------------
def test_kv_cache_dtype_parsing_and_refusals_before_any_device_work():
    from vitron_amd.engine import parse_kv_cache_dtype
    from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    for x, want in ((None, "16bit"), ("auto", "16bit"), ("16bit", "16bit"), ("fp8", "fp8"), ("fp8_e4m3", "fp8"), ("FP8", "fp8")):
        assert parse_kv_cache_dtype(x) == want
    for bad in ("fp8_e5m2", "int8", 8, ""):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            parse_kv_cache_dtype(bad)
    small = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, vocab_size=64)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        LlavaLlamaForCausalLM(LlavaConfig(**small, kv_cache_dtype="fp4"))
    assert LlavaLlamaForCausalLM(LlavaConfig(**small)).kv_cache_dtype == "16bit"
    model = LlavaLlamaForCausalLM(LlavaConfig(**small, kv_cache_dtype="fp8"))
    assert model.kv_cache_dtype == "fp8"
    with pytest.raises(RuntimeError, match="fp8 KV cache"):
        model.set_precise(1)
    with pytest.raises(NotImplementedError, match="fp8 KV cache"):
        model.generate(torch.ones((2, 4), dtype=torch.long), padded_batch=True, max_new_tokens=1)
    model.set_kv_cache_dtype("16bit")
    assert model.kv_cache_dtype == "16bit" and model.config.kv_cache_dtype is None
    # the reverse order: a precise mode first, the fp8 cache refused
    model.precise_level = 1
    with pytest.raises(RuntimeError, match="precise"):
        model.set_kv_cache_dtype("fp8")
    model.precise_level = 0
    assert model.set_kv_cache_dtype("fp8_e4m3").kv_cache_dtype == "fp8"
    from vitron_amd.model.builder import load_pretrained_model
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        load_pretrained_model("synthetic", None, "x", kv_cache_dtype="e5m2")
