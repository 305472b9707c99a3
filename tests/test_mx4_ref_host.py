"""The MX-FP4 image reference without a GPU (tests/mx4_ref.py): on every dataset and shape tests/test_gpu_mx4_image.py walks, float32
emulations of the operand-out producers pass the per-element contract (image_check, no element exempt) and the exact builders' bit-for-bit
equality, and each emulated fault -- a block exponent one too high, the block maximum over half the block, ties rounded away, the nibbles
of a byte exchanged, the scale array indexed m % 16 <-> (m % 64) / 16, an exponent stored one block further, a last row group never
written, the image of the row the gather should not have read -- fails at least one of those assertions. Also here: the conditions the
GPU tests rest on (the activations are the identity from 8 / 12 / 20 up, the exact builders' accumulators are fp32 numbers inside the
saturated range, the ambiguous shares of the chosen inputs stay under the caps)."""
import numpy as np
import pytest
import torch

from oracle import vitron_oracle as O
from tests import gemm_ref as G
from tests import mx4_ref as X
from tests import norm_ref as NR
from tests.gemm_ref import U

DT_IDS = ["bf16", "fp16"]
# ambiguous shares allowed on the reference alone (hi = op16(v64)): codes, exponents. Past them a check of the image says too little.
CAPS = {torch.bfloat16: (0.02, 0.01), torch.float16: (0.10, 0.05)}


def _flagged(run, faults, what):
    run(None)
    for f in faults:
        try:
            run(f)
        except AssertionError:
            continue
        raise AssertionError(f"{what}: the fault '{f}' passed every assertion")


def _under_caps(v64, delta, dtype, what):
    codes, exps = X.reference_shares(v64, delta, dtype)
    assert codes <= CAPS[dtype][0] and exps <= CAPS[dtype][1], f"{what}: ambiguous shares {codes:.4f} of the codes, {exps:.4f} of the exponents"
    return codes, exps


def _faults(M, idx=False):
    """one row sits at m % 16 == (m % 64) / 16 == 0: the exchanged scale index cannot show; only the gather can ignore idx"""
    return [f for f in X.FAULTS if not (f == "scale_index" and M == 1) and (idx or f != "idx_ignored")]


def test_constants_follow_the_chains():
    assert X.CHAIN_RMS_MX == 134 and X.CHAIN_LN_MX == NR.CHAIN_WAVE == 70
    rel = NR.rstd_rel(X.CHAIN_RMS_MX) + 2 * U
    assert rel == ((1 + 134 + 3) / 2 + 1) * U + NR.E_RSQRT + 2 * U and 75 * U < rel < 76 * U
    y = torch.tensor([[-3.0, 0.5]], dtype=torch.float64)
    assert torch.equal(NR.rms_f32_part(y) + G.store_half_ulp(y, torch.bfloat16), NR.rms_bound(y, torch.bfloat16))
    x, g, b = X.ln_gauss(4, 256, 1)
    y64, t64, r64 = NR.ln_ref(x, g, b, X.EPS)
    part = NR.ln_f32_part(x, g, y64, t64, r64) + G.store_half_ulp(y64, torch.float16)       # (the same terms in another order of additions)
    assert torch.allclose(part, NR.ln_bound(x, g, y64, t64, r64, torch.float16), rtol=1e-14, atol=0.0)


def test_storage_helpers_invert_each_other():
    rng = np.random.default_rng(0)
    for M, K in ((1, 64), (65, 96), (300, 512)):
        e = torch.from_numpy(rng.integers(1, 255, size=(M, K // 32)))
        arr = X.aexp_pack(e, K, fill=X.FILL)
        assert arr.numel() == X.aexp_bytes(M, K) and torch.equal(X._aexp_rows(arr, M, K), e.to(torch.int32))
        X.assert_pad_rows(arr, M, K, "pack")
        c = torch.from_numpy(rng.integers(0, 16, size=(M, K))).to(torch.int32)
        assert torch.equal(X._unpack(X.pack_codes(c)), c)
        assert torch.equal(X.code_values(c).float(), X._deq(c, torch.full((M, K // 32), 127), 32))
    # the kernels' index formula, byte by byte
    arr = X.aexp_pack(torch.arange(70 * 2).view(70, 2) % 251, 64)
    for m, kb in ((0, 0), (17, 1), (63, 0), (69, 1)):
        assert int(arr[((m >> 6) * 2 + kb) * 64 + (m & 15) * 4 + ((m & 63) >> 4)]) == (m * 2 + kb) % 251


def test_activations_are_the_identity_from_their_floor_up():
    """the saturation the exact GEMM probes rest on: vt_gelu_erf from 8, vt_quick_gelu from 12, vt_silu from 20 return x itself up to XMAX"""
    for f, kind in ((G.gelu_f32, "gelu"), (G.qgelu_f32, "qgelu"), (G.silu_f32, "swiglu")):
        x = np.linspace(X.ACT_FLOOR[kind], G.XMAX, 100001).astype(np.float32)
        assert np.array_equal(f(x), x), kind


def test_image_check_flags_single_faults():
    """one exponent + 1, one flipped code bit, a nibble swap, rows 0 and 16 exchanged in the scale array"""
    dtype = torch.bfloat16
    x, g = X.rms_gauss(65, 1024, 3)
    v64 = NR.rms_ref(x, g, X.EPS)
    delta = X.rms_delta(v64)
    y, c, arr = X.rms_mx_f32(x.numpy(), g.numpy(), X.EPS, dtype)
    e = X._aexp_rows(arr, 65, 1024)
    assert all(bool(m.all()) for m in X.image_check(v64, delta, y, c, e, dtype)[:3])
    e1 = e.clone()
    e1[7, 5] += 1
    ok = X.image_check(v64, delta, y, c, e1, dtype)[1]
    assert not bool(ok[7, 5]) and int((~ok).sum()) == 1
    flipped = 0
    for bit in (1, 2, 4):
        c1 = c.clone()
        c1[9, 100:132] ^= bit
        flipped += int((~X.image_check(v64, delta, y, c1, e, dtype)[2]).sum())
    assert flipped >= 90                                              # 96 flips, the ambiguous elements may absorb a few
    ok = X.image_check(v64, delta, y, c.view(65, -1, 2).flip(-1).reshape(65, -1), e, dtype)[2]
    assert 0.3 < float((~ok).double().mean()) < 0.9
    e2 = e.clone()
    e2[[0, 16]] = e[[16, 0]]
    assert not bool(X.image_check(v64, delta, y, c, e2, dtype)[1].all())


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rows,D", X.norm_cases(X.RMS_D))
def test_rmsnorm_mx_emulation_passes_and_every_fault_fails(dtype, rows, D):
    src = rows + 7
    xg, g = X.rms_gauss(src, D, D + rows)
    xe, ge, ve = X.rms_exact(src, D, D + rows)
    v64 = NR.rms_ref(xg, g, X.EPS)
    delta = X.rms_delta(v64)
    _under_caps(v64, delta, dtype, f"rmsnorm {rows}x{D}")
    idx = (torch.arange(rows) * 5 + 3) % src
    idx[rows // 2] = idx[0]

    def run(fault, ix=None):
        sel = torch.arange(rows) if ix is None else ix
        y, c, arr = X.rms_mx_f32(xe.numpy()[:src if ix is not None else rows], ge.numpy(), 0.0, dtype, idx=None if ix is None else ix.numpy(), fault=fault)
        X.assert_exact(ve[sel], dtype, y, c, X._aexp_rows(arr, rows, D), "exact")
        X.assert_pad_rows(arr, rows, D, "exact")
        y, c, arr = X.rms_mx_f32(xg.numpy()[:src if ix is not None else rows], g.numpy(), X.EPS, dtype, idx=None if ix is None else ix.numpy(), fault=fault)
        X.assert_image(v64[sel], delta[sel], y, c, X._aexp_rows(arr, rows, D), dtype, "gauss")

    _flagged(run, _faults(rows), f"rmsnorm {rows}x{D}")
    _flagged(lambda f: run(f, idx), ["idx_ignored"], f"rmsnorm {rows}x{D} through idx")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rows,D", X.norm_cases(X.LN_D))
def test_layernorm_mx_emulation_passes_and_every_fault_fails(dtype, rows, D):
    xg, g, b = X.ln_gauss(rows, D, D + rows)
    xe, ge, be, ve = X.ln_exact(rows, D, D + rows)
    assert bool((xe.double().sum(-1) == 0).all())
    y64, t64, r64 = NR.ln_ref(xg, g, b, X.EPS)
    delta = X.ln_delta(xg, g, y64, t64, r64)
    _under_caps(y64, delta, dtype, f"layernorm {rows}x{D}")

    def run(fault):
        y, c, arr = X.ln_mx_f32(xe.numpy(), ge.numpy(), be.numpy(), 0.0, dtype, fault=fault)
        X.assert_exact(ve, dtype, y, c, X._aexp_rows(arr, rows, D), "exact")
        X.assert_pad_rows(arr, rows, D, "exact")
        y, c, arr = X.ln_mx_f32(xg.numpy(), g.numpy(), b.numpy(), X.EPS, dtype, fault=fault)
        X.assert_image(y64, delta, y, c, X._aexp_rows(arr, rows, D), dtype, "gauss")

    _flagged(run, _faults(rows), f"layernorm {rows}x{D}")


def _gemm_case(dtype, kind, M, N, K):
    nout = N // 2 if kind == "swiglu" else N
    q = X.mx_gemm_ints(M, N, K, X.gemm_seed(M, N, K), kind, dtype, zero_tile=kind == "swiglu" and N == X.ZERO_TILE_N)
    p = X.gemm_gauss(M, N, K, X.gemm_seed(M, N, K), dtype, kind)
    pre = X.gemm_gauss_pre32(p)
    assert float(pre.abs().max()) <= G.XMAX
    v64, delta = X.act_ref(pre, kind)
    if M > 1:                                                          # (one row of 64 .. 320 outputs is too few to estimate a share of 2 %)
        _under_caps(v64, delta, dtype, f"{kind} {M}x{N}x{K}")

    def run(fault):
        y, c, arr = X.act_mx_f32(q["pre64"].float().numpy(), kind, dtype, fault=fault)
        e = X._aexp_rows(arr, M, nout)
        X.assert_exact(q["v32"], dtype, y, c, e, "exact")
        if q["zero"] is not None:
            zb = slice(q["zero"].start // 32, q["zero"].stop // 32)
            assert bool((e[:, zb] == 1).all()) and bool(((c[:, q["zero"]] & 7) == 0).all()) and bool((y[:, q["zero"]].float() == 0).all())
        y, c, arr = X.act_mx_f32(pre.numpy(), kind, dtype, fault=fault)
        X.assert_image(v64, delta, y, c, X._aexp_rows(arr, M, nout), dtype, "gauss")

    _flagged(run, _faults(M), f"{kind} {M}x{N}x{K}")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K", X.gemm_cases(X.SWIGLU_N))
def test_swiglu_epilogue_emulation_passes_and_every_fault_fails(dtype, M, N, K):
    _gemm_case(dtype, "swiglu", M, N, K)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["gelu", "qgelu"])
@pytest.mark.parametrize("M,N,K", X.gemm_cases(X.GELU_N))
def test_gelu_epilogue_emulation_passes_and_every_fault_fails(dtype, kind, M, N, K):
    _gemm_case(dtype, kind, M, N, K)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_quant_lo_probes_hold_what_they_claim(dtype):
    lo, want = X.quant_lo_probes(dtype)
    assert G.representable(lo, dtype)
    _, q, e = O.mx4_quant(lo, 32)
    amax = lo.view(lo.shape[0], -1, 32).abs().amax(-1)
    mant = amax / torch.exp2(torch.floor(torch.log2(amax.clamp(min=2.0 ** -30))))
    assert bool((mant[want["m15"]] == 1.5).all()) and bool((q.view(lo.shape[0], -1, 32).abs().amax(-1)[want["m15"]] == 6).all())
    assert bool((amax[want["six"]] * torch.exp2(-e[want["six"]].float()) == 6).all())
    if dtype == torch.float16:
        assert bool((amax[want["sub"]] < 2.0 ** -14).all()) and bool((amax[want["sub"]] > 0).all())


@pytest.mark.parametrize("M,N,K", [(300, 512, 1024), (1300, 1024, 768)])
def test_resid_ints_are_fp32_exact(M, N, K):
    p = X.resid_ints(M, N, K, M + N)
    assert bool((p["ref64"].float().double() == p["ref64"]).all())
