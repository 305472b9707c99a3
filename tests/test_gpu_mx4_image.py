"""The MX-FP4 operand images of precise level 3, producer by producer, per element and bit for bit (vt_mx4_quant_lo, vt_rmsnorm_mx,
vt_layernorm_mx, the SwiGLU / GELU / quick-GELU operand-out epilogues of vt_gemm_mx, vt_gemm_mx_resid) against tests/mx4_ref.py, whose
checks tests/test_mx4_ref_host.py proves on the CPU to catch a wrong exponent, a clipped block, ties rounded away, exchanged nibbles, a
permuted or shifted scale array, a stale row group and an ignored gather. Exact probes -- data whose fp32 value is known whatever the
summation order -- must come back as the oracle's image bit for bit; Gaussian data must meet image_check with no element exempt, the
bound derived from the kernels' summation chains and vt_common.h's statements about the activations (DESIGN.md "MX image pinning"). Every
producer is launched through the C ABI into over-allocated buffers filled with 0xA5 whose spare bytes must still hold 0xA5 afterwards."""
import pytest
import torch

from oracle import vitron_oracle as O
from tests import gemm_ref as G
from tests import mx4_ref as X
from tests import norm_ref as NR

pytestmark = pytest.mark.gpu
DT_IDS = ["bf16", "fp16"]
GUARD_ROWS = 3
GUARD_COLS = 8
GUARD_BYTES = 64


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


def _filled(dev, shape, dtype=torch.uint8):
    """a tensor of `dtype` whose every byte is FILL"""
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), X.FILL, dtype=torch.uint8, device=dev).view(dtype).view(*shape)


def _untouched(t, what):
    b = t.contiguous().view(torch.uint8)
    assert bool((b == X.FILL).all()), f"{what}: {int((b != X.FILL).sum())} guard bytes written"


def _record(record_property, what, ratio, codes, exps):
    print(f"[mx4 image] {what}: worst |v_implied - v64| / delta {ratio:.4f}, ambiguous codes {codes:.4f}, exponents {exps:.4f}")
    record_property("worst_implied_over_delta", round(ratio, 4))
    record_property("ambiguous_codes", round(codes, 4))
    record_property("ambiguous_exponents", round(exps, 4))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- rsqrtf(4^k) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_ks(dev):
    """the k of mx4_ref.K_SET for which the device returns rsqrtf(4^k) == 2^-k exactly, read through vt_rowscale_finalize (one group,
    inv_dim 1, eps 0: out = rsqrtf(x * 1 + 0)): the exact norm probes use these and no other"""
    from vitron_amd import ops
    x = torch.tensor([[4.0 ** k for k in X.K_SET]], device=dev)
    got = ops.rowscale_finalize(x, len(X.K_SET), 1.0, 0.0).cpu()
    return tuple(k for k, r in zip(X.K_SET, got.tolist()) if r == 2.0 ** -k)


def test_rsqrt_of_a_power_of_four(dev, exact_ks, record_property):
    """the exact norm probes rest on rsqrtf(4^k) == 2^-k: k = 0 must be exact; which of k = -12 .. 12 are is recorded (EXPERIMENTS.md)"""
    from vitron_amd import ops
    ks = list(range(-12, 13))
    x = torch.tensor([[4.0 ** k for k in ks]], device=dev)
    got = ops.rowscale_finalize(x, len(ks), 1.0, 0.0).cpu().tolist()
    inexact = [k for k, r in zip(ks, got) if r != 2.0 ** -k]
    print(f"[mx4 image] rsqrtf(4^k) != 2^-k for k in {inexact} of -12 .. 12; probes use k in {exact_ks}")
    record_property("rsqrt_inexact_k", str(inexact))
    record_property("probe_k", str(exact_ks))
    assert 0 in exact_ks


# ---- the norms -----------------------------------------------------------------------------------------------------------------------------------
def _norm_launch(dev, dtype, name, x, g, b, eps, rows, idx=None):
    """vt_rmsnorm_mx (b None) / vt_layernorm_mx through the C ABI into FILL-ed y, codes and scale array with spare rows / bytes behind them
    -> (y cpu, codes int [rows][D], scale array uint8 cpu [aexp_bytes]); the spare rows and bytes must come back untouched"""
    from vitron_amd import _lib
    lib = _lib.load(operand=_lib.operand_of(dtype))
    D = x.shape[1]
    nb = X.aexp_bytes(rows, D)
    assert nb == lib.vt_mx4_aexp_bytes(rows, D)
    y = _filled(dev, (rows + GUARD_ROWS, D), dtype)
    a4 = _filled(dev, (rows + GUARD_ROWS, D // 2))
    aexp = _filled(dev, (nb + GUARD_BYTES,))
    xd, gd = x.to(dev).contiguous(), g.to(dev).contiguous()
    if b is None:
        ix = None if idx is None else idx.to(torch.int32).to(dev)
        st = lib.vt_rmsnorm_mx(xd.data_ptr(), None if ix is None else ix.data_ptr(), gd.data_ptr(), y.data_ptr(), a4.data_ptr(), aexp.data_ptr(),
                               rows, D, eps, _stream())
    else:
        bd = b.to(dev).contiguous()
        st = lib.vt_layernorm_mx(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), a4.data_ptr(), aexp.data_ptr(), rows, D, eps, _stream())
    _lib.check(st, name, lib)
    torch.cuda.synchronize()
    _untouched(y[rows:], name + " y rows past the last")
    _untouched(a4[rows:], name + " code rows past the last")
    _untouched(aexp[nb:], name + " bytes behind the scale array")
    return y[:rows].cpu(), X._unpack(a4[:rows]), aexp[:nb].cpu()


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rows,D", X.norm_cases(X.RMS_D))
def test_rmsnorm_mx_image(dev, dtype, rows, D, exact_ks, record_property):
    """D = 512 .. 8192 reaches rmsnorm_mx_kernel<2> / <8> / <16>, each with full and with ragged chunks; rows 1 .. 130 one to three row groups,
    the last one ragged. Exact probe: y, codes and exponents bit for bit, exponent byte 0 for the rows past the last, nothing behind the
    last row group. Gaussian rows, three in ten x 60: image_check everywhere."""
    what = f"vt_rmsnorm_mx {rows}x{D}"
    x, g, v32 = X.rms_exact(rows, D, D + rows, ks=exact_ks)
    y, c, arr = _norm_launch(dev, dtype, what, x, g, None, 0.0, rows)
    X.assert_exact(v32, dtype, y, c, X._aexp_rows(arr, rows, D), what + " exact")
    X.assert_pad_rows(arr, rows, D, what + " exact")
    x, g = X.rms_gauss(rows, D, D + rows)
    v64 = NR.rms_ref(x, g, X.EPS)
    y, c, arr = _norm_launch(dev, dtype, what, x, g, None, X.EPS, rows)
    X.assert_pad_rows(arr, rows, D, what)
    _record(record_property, what, *X.assert_image(v64, X.rms_delta(v64), y, c, X._aexp_rows(arr, rows, D), dtype, what))


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_rmsnorm_mx_image_through_idx(dev, dtype, exact_ks, record_property):
    """the gather: 65 rows picked, permuted and one repeated, from a source of 72"""
    rows, D, src = 65, 4608, 72
    what = f"vt_rmsnorm_mx {rows}x{D} through idx"
    idx = (torch.arange(rows) * 5 + 3) % src
    idx[rows // 2] = idx[0]
    x, g, v32 = X.rms_exact(src, D, 1, ks=exact_ks)
    y, c, arr = _norm_launch(dev, dtype, what, x, g, None, 0.0, rows, idx=idx)
    X.assert_exact(v32[idx], dtype, y, c, X._aexp_rows(arr, rows, D), what + " exact")
    x, g = X.rms_gauss(src, D, 2)
    v64 = NR.rms_ref(x, g, X.EPS)[idx]
    y, c, arr = _norm_launch(dev, dtype, what, x, g, None, X.EPS, rows, idx=idx)
    X.assert_pad_rows(arr, rows, D, what)
    _record(record_property, what, *X.assert_image(v64, X.rms_delta(v64), y, c, X._aexp_rows(arr, rows, D), dtype, what))


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rows,D", X.norm_cases(X.LN_D))
def test_layernorm_mx_image(dev, dtype, rows, D, exact_ks, record_property):
    """D = 256 .. 1024: layernorm_mx_kernel<4>, 1280 and 4096: <16>. Exact probe (as many +2^k as -2^k in a row: mean 0) and Gaussian rows
    with a per-row offset."""
    what = f"vt_layernorm_mx {rows}x{D}"
    x, g, b, v32 = X.ln_exact(rows, D, D + rows, ks=exact_ks)
    y, c, arr = _norm_launch(dev, dtype, what, x, g, b, 0.0, rows)
    X.assert_exact(v32, dtype, y, c, X._aexp_rows(arr, rows, D), what + " exact")
    X.assert_pad_rows(arr, rows, D, what + " exact")
    x, g, b = X.ln_gauss(rows, D, D + rows)
    y64, t64, r64 = NR.ln_ref(x, g, b, X.EPS)
    y, c, arr = _norm_launch(dev, dtype, what, x, g, b, X.EPS, rows)
    X.assert_pad_rows(arr, rows, D, what)
    _record(record_property, what, *X.assert_image(y64, X.ln_delta(x, g, y64, t64, r64), y, c, X._aexp_rows(arr, rows, D), dtype, what))


# ---- vt_mx4_quant_lo -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_quant_lo_strided_edges_and_subnormals(dev, dtype):
    """a column slice of a wider buffer (ld = K + 64, 32 columns in), with blocks whose maximum has the mantissa 1.5 exactly, blocks whose
    maximum is 6 2^e beside every tie of e2m1, and (fp16) blocks of subnormals only: codes and exponents bit for bit"""
    from vitron_amd import _lib
    lib = _lib.load(operand=_lib.operand_of(dtype))
    lo, _ = X.quant_lo_probes(dtype)
    M, K = lo.shape
    buf = torch.full((M + GUARD_ROWS, K + 64), 3.0, dtype=dtype, device=dev)
    buf[:M, 32:32 + K] = lo.to(dtype).to(dev)
    nb = X.aexp_bytes(M, K)
    a4 = _filled(dev, (M + GUARD_ROWS, K // 2))
    aexp = _filled(dev, (nb + GUARD_BYTES,))
    view = buf[:, 32:32 + K]
    _lib.check(lib.vt_mx4_quant_lo(view.data_ptr(), buf.stride(0), M, K, a4.data_ptr(), aexp.data_ptr(), _stream()), "vt_mx4_quant_lo", lib)
    torch.cuda.synchronize()
    _untouched(a4[M:], "vt_mx4_quant_lo code rows past the last")
    _untouched(aexp[nb:], "vt_mx4_quant_lo bytes behind the scale array")
    _, q, e = O.mx4_quant(lo, 32)
    assert torch.equal(X._aexp_rows(aexp[:nb], M, K), e + 127)
    assert torch.equal(X._unpack(a4[:M]), O.mx4_codes(q))


# ---- the operand-out epilogues -------------------------------------------------------------------------------------------------------------------
def _act_launch(dev, dtype, kind, a, a4, aexp, w, w4, wexp, bias, M, N, K):
    """vt_gemm_mx_swiglu / vt_gemm_mx_gelu through the C ABI (device operands) into FILL-ed C (ldc = outputs + 8, three spare rows), codes
    (three spare rows) and scale array (64 spare bytes) -> (C cpu [M][outputs], codes int, biased exponents [M][outputs / 32])"""
    from vitron_amd import _lib
    lib = _lib.load(operand=_lib.operand_of(dtype))
    nout = N // 2 if kind == "swiglu" else N
    nb = X.aexp_bytes(M, nout)
    assert nb == lib.vt_mx4_aexp_bytes(M, nout)
    c = _filled(dev, (M + GUARD_ROWS, nout + GUARD_COLS), dtype)
    h4 = _filled(dev, (M + GUARD_ROWS, nout // 2))
    hexp = _filled(dev, (nb + GUARD_BYTES,))
    args = (a.data_ptr(), K, a4.data_ptr(), aexp.data_ptr(), w.data_ptr(), K, w4.data_ptr(), wexp.data_ptr())
    if kind == "swiglu":
        st = lib.vt_gemm_mx_swiglu(*args, c.data_ptr(), c.stride(0), h4.data_ptr(), hexp.data_ptr(), M, N, K, _stream())
    else:
        st = lib.vt_gemm_mx_gelu(*args, None if bias is None else bias.data_ptr(), c.data_ptr(), c.stride(0), h4.data_ptr(), hexp.data_ptr(), M, N, K,
                                 int(kind == "qgelu"), _stream())
    what = f"vt_gemm_mx_{kind} {M}x{N}x{K}"
    _lib.check(st, what, lib)
    torch.cuda.synchronize()
    _untouched(c[M:], what + " C rows past M")
    _untouched(c[:M, nout:], what + " C columns past N")
    _untouched(h4[M:], what + " code rows past M")
    _untouched(hexp[nb:], what + " bytes behind the scale array")
    return c[:M, :nout].cpu().contiguous(), X._unpack(h4[:M]), X._aexp_rows(hexp[:nb], M, nout)


def _act_case(dev, dtype, kind, M, N, K, record_property):
    from vitron_amd import ops
    what = f"vt_gemm_mx_{kind} {M}x{N}x{K}"
    seed = X.gemm_seed(M, N, K)
    # the saturated probe: integers, every accumulator exact, the activation the identity
    q = X.mx_gemm_ints(M, N, K, seed, kind, dtype, zero_tile=kind == "swiglu" and N == X.ZERO_TILE_N)
    bias = None if q["bias"] is None else q["bias"].to(dev)
    y, c, e = _act_launch(dev, dtype, kind, q["a"].to(dtype).to(dev), q["a4"].to(dev), q["aexp"].to(dev), q["w"].to(dtype).to(dev), q["w4"].to(dev),
                          q["ew"].to(dev), bias, M, N, K)
    X.assert_exact(q["v32"], dtype, y, c, e, what + " exact")
    if q["zero"] is not None:
        z = q["zero"]
        assert bool((y[:, z].float() == 0).all()) and bool(((c[:, z] & 7) == 0).all()), what + ": the zero tile's outputs and codes"
        assert bool((e[:, z.start // 32: z.stop // 32] == 1).all()), what + ": the zero tile's exponent bytes"
    # Gaussian operands through the project's own quantisers; the fp32 pre-activations are the fp32-out epilogue's of the same operands
    p = X.gemm_gauss(M, N, K, seed, dtype, kind)
    a, w = p["hi"].to(dtype).to(dev), p["w"].to(dtype).to(dev)
    a4, aexp = ops.mx4_quant_lo(p["lo"].to(dtype).to(dev))
    w4, wexp = ops.mx4_quant_weights(w)
    bias = None if p["bias"] is None else p["bias"].to(dev)
    pre32 = ops.gemm_mx(a, a4, aexp, w, w4, wexp, bias, ops.EPI_F32).cpu()
    host = X.gemm_gauss_pre32(p).double()                # (both products in fp64, rounded once)
    loose = G.sum_bound(p["hi"], p["w"]) + G.sum_bound(O.mx4_quant(p["lo"], 32)[0], O.mx4_quant(p["w"], None)[0]) + 3 * G.U * host.abs()
    assert bool(((pre32.double() - host).abs() <= loose).all()), what + ": the fp32-out launch the reference is taken from"
    assert float(pre32.abs().max()) <= G.XMAX
    v64, delta = X.act_ref(pre32, kind)
    y, c, e = _act_launch(dev, dtype, kind, a, a4, aexp, w, w4, wexp, bias, M, N, K)
    _record(record_property, what, *X.assert_image(v64, delta, y, c, e, dtype, what))


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K", X.gemm_cases(X.SWIGLU_N))
def test_gemm_mx_swiglu_image(dev, dtype, M, N, K, record_property):
    """N = 128, 384, 640: the last (or only) 256-column tile holds 64 outputs of 128; M = 1 .. 300 under one row group, around it and a
    ragged second 256-row tile. The saturated probe at N = 384 carries the tile whose up accumulators are exactly 0: exponent byte 1, zero
    codes."""
    _act_case(dev, dtype, "swiglu", M, N, K, record_property)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["gelu", "qgelu"])
@pytest.mark.parametrize("M,N,K", X.gemm_cases(X.GELU_N))
def test_gemm_mx_gelu_image(dev, dtype, kind, M, N, K, record_property):
    """N = 64, 192, 320: a last column tile of 64 outputs (half a wave's 128), alone and behind a full one"""
    _act_case(dev, dtype, kind, M, N, K, record_property)


# ---- vt_gemm_mx_resid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K", [(300, 512, 1024), (1300, 1024, 768)])
def test_gemm_mx_resid_exact_on_both_paths(dev, dtype, M, N, K):
    """integer operands and an integer residual: every partial sum over every K range is an fp32 number, so the one-launch path and the
    split path (K ranges into fp32 slabs + the ordered reduce) must both return the fp64 result bit for bit"""
    from vitron_amd import ops
    p = X.resid_ints(M, N, K, M + N + K)
    a, w = p["a"].to(dtype).to(dev), p["w"].to(dtype).to(dev)
    a4, aexp, w4, ew = p["a4"].to(dev), p["aexp"].to(dev), p["w4"].to(dev), p["ew"].to(dev)
    plain = ops.gemm_mx_resid(a, a4, aexp, w, w4, ew, p["resid"].to(dev).clone())
    assert torch.equal(plain.cpu().double(), p["ref64"]), "the one-launch path"
    part = torch.empty((8 * M * N,), device=dev, dtype=torch.float32)
    split = ops.gemm_mx_resid(a, a4, aexp, w, w4, ew, p["resid"].to(dev).clone(), part)
    assert torch.equal(split.cpu().double(), p["ref64"]), "the split path"
