"""The 16-bit GEMM family on the GPU (vt_gemm_bf16 / vt_gemm_bf16_resid_splitk through ops.gemm / ops.gemm_resid_splitk: the tile kernels of
vitron_amd/csrc/vt_gemm.hip and vt_gemm8.hip in every explicit configuration, the weight-streaming kernels, the planner's row and column
splits, the two-pass split-K) against the host restatement in tests/gemm_ref.py, in both operand builds: small integers and one-hot
full-mantissa probes whose results are exact in fp32 whatever the summation order (compared bit for bit, the 16-bit stores against
round-to-nearest-even), random data inside the per-element bound of an fp32 accumulation, the activation epilogues inside the error their
documentation allows. Every launch reads A and W as views into wider, taller NaN-filled buffers and writes C as a view into a NaN-filled
buffer (_launch): everything outside the M x N window must keep its bits and the window must hold no NaN."""
import pytest
import torch

from tests import gemm_ref as G
from tests.gemm_ref import EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_GELU, EPI_QGELU, EPI_RELU, EPI_SWIGLU

pytestmark = pytest.mark.gpu
NAN = float("nan")
ROW0, COL0, GAP = 2, 8, 2                                # A / W rows in front, columns in front (16 bytes); C rows in front (even: 16 bytes)
DT_IDS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _padded(x, dtype, dev, row0, col0, rows_after, cols_after):
    """x [R][C] -> the view [row0 : row0 + R, col0 : col0 + C] of a NaN-filled device buffer"""
    R, C = x.shape
    buf = torch.full((row0 + R + rows_after, col0 + C + cols_after), NAN, dtype=dtype, device=dev)
    view = buf[row0:row0 + R, col0:col0 + C]
    view.copy_(x.to(dtype))
    return view


def _padded_vec(v, dev):
    buf = torch.full((v.numel() + 12,), NAN, dtype=torch.float32, device=dev)
    buf[4:4 + v.numel()] = v
    return buf[4:4 + v.numel()]


class Problem:
    """One GEMM's operands on the device, each inside NaN: A = abuf[2 : 2 + M, 8 : 8 + K] of a buffer 5 rows taller and 24 columns wider
    (lda = K + 24), W the same view of a buffer 4 rows taller and 16 columns wider, bias / row_scale 4 floats into buffers 12 floats longer.
    a, w: fp32 holders of values the operand dtype represents (asserted)."""

    def __init__(self, dev, dtype, a, w, bias=None, resid=None, rs=None):
        assert G.representable(a, dtype) and G.representable(w, dtype)
        self.dtype, self.M, self.K, self.N = dtype, a.shape[0], a.shape[1], w.shape[0]
        self.a = _padded(a, dtype, dev, ROW0, COL0, 3, 16)
        self.w = _padded(w, dtype, dev, ROW0, COL0, 2, 8)
        self.bias = None if bias is None else _padded_vec(bias, dev)
        self.rs = None if rs is None else _padded_vec(rs, dev)
        self.resid = resid
        assert self.a.stride(0) == self.K + 24 and self.w.stride(0) == self.K + 16 and not (self.M > 1 and self.a.is_contiguous())


def _launch(dev, pb: Problem, epi, cfg=0, bias=True, rs=True, splitk=None, work=None):
    """One launch into C = cbuf[2 : 2 + M, 8 : 8 + n_out] of a NaN buffer 5 rows taller and 20 columns wider than the result (ldc =
    n_out + 20); EPI_F32_RESID: the window holds the residual. Afterwards every bit outside the window is as before and the window holds
    no NaN. splitk = ksplit: through ops.gemm_resid_splitk with the workspace `work`. Returns the window on the host."""
    from vitron_amd import ops
    n_out = pb.N // 2 if epi == EPI_SWIGLU else pb.N
    odt = torch.float32 if epi in (EPI_F32, EPI_F32_RESID) else pb.dtype
    cbuf = torch.full((GAP + pb.M + 3, COL0 + n_out + 12), NAN, dtype=odt, device=dev)
    win = cbuf[GAP:GAP + pb.M, COL0:COL0 + n_out]
    if epi == EPI_F32_RESID:
        win.copy_(pb.resid)
    before = _bits(cbuf).clone()
    b = pb.bias if bias else None
    if splitk is None:
        ops.gemm(pb.a, pb.w, b, epi, out=win, cfg=cfg, row_scale=pb.rs if rs else None)
    else:
        ops.gemm_resid_splitk(pb.a, pb.w, win, b, splitk, work)
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
        raise AssertionError(f"{int(nan.sum())} NaN in the result (padding leaked in, or elements never written), first at ({r}, {c})")
    return got


def _where(bad, got, want, what):
    idx = bad.nonzero()
    rows, cols = idx[:, 0], idx[:, 1]
    first = ", ".join(f"({r}, {c}): got {float(got[r, c])!r} want {float(want[r, c])!r}" for r, c in idx[:4].tolist())
    return (f"{what}: {idx.shape[0]} of {bad.numel()} elements differ, rows {int(rows.min())}..{int(rows.max())}, columns "
            f"{int(cols.min())}..{int(cols.max())}; first {first}")


def _exact(got, want, what):
    """bit for bit, but for the sign of a zero"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), _where(bad, got, want, what)


def _within(got, ref64, bound, what):
    """|got - ref64| <= bound element by element -> the worst err / bound"""
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound)
    worst = float((err / bound).max())
    print(f"[{what}] worst err / bound {worst:.3f}")                    # shown with -s: the figures EXPERIMENTS.md records
    assert not bool(bad.any()), _where(bad, got, ref64, what) + f"; worst err / bound {worst:.3f}"
    return worst


CASES = G.all_cases()
CASES_SLOW = G.all_cases(full=False)


def _ids(cases):
    return [G.case_id(c) for c in cases]


# ---- a. small integers: every epilogue exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_integers_are_exact_in_every_plain_epilogue(dev, dtype, case):
    """Integers of |a|, |w| <= 4, a bias and a residual of integers + j / 64: every partial sum is exact in fp32 in any order, so EPI_F32 and
    EPI_F32_RESID return the fp64 result itself and EPI_BF16 / EPI_BF16_RELU that result rounded to nearest even (fp16: clamped first). The
    results lie past 256 and on odd multiples of 2^-6: ties of both stores (tests/test_gemm_ref_host.py)."""
    cfg, M, N, K = case
    a, w = G.int_operands(M, N, K, M + N + K)
    bias, resid = G.frac_vector(N, K), G.frac_vector(M * N, K + 1).reshape(M, N)
    pb = Problem(dev, dtype, a, w, bias, resid)
    y, ok = G.exact_epilogue(a, w, bias)
    y0, ok0 = G.exact_epilogue(a, w)
    yr, okr = G.exact_epilogue(a, w, bias, resid)
    assert ok and ok0 and okr
    _exact(_launch(dev, pb, EPI_F32, cfg), y.float(), "EPI_F32 + bias")
    _exact(_launch(dev, pb, EPI_F32, cfg, bias=False), y0.float(), "EPI_F32")
    _exact(_launch(dev, pb, EPI_F32_RESID, cfg), yr.float(), "EPI_F32_RESID + bias")
    _exact(_launch(dev, pb, EPI_BF16, cfg), G.rne_op(y, dtype), "EPI_BF16 + bias")
    _exact(_launch(dev, pb, EPI_BF16, cfg, bias=False), G.rne_op(y0, dtype), "EPI_BF16")
    _exact(_launch(dev, pb, EPI_RELU, cfg), G.rne_op(y.clamp_min(0.0), dtype), "EPI_BF16_RELU + bias")


# ---- b. one-hot probes: k addressing and operand bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_one_hot_probes_return_single_products(dev, dtype, case):
    """Row m of A is zero but for one value at k(m) = (7 m + 5) mod K (mirrored: row n of W), every value uses all significand bits of the
    operand type (first and last bit set): out[m][n] is ONE product of at most 22 bits, exact in fp32 -- a wrong k, a dropped K step or an
    operand that lost a low bit changes it. EPI_F32 returns the product, EPI_BF16 the product rounded to nearest even."""
    cfg, M, N, K = case
    for mirrored in (False, True):
        a, w, want = G.onehot_problem(M, N, K, dtype, M + K, mirrored)
        pb = Problem(dev, dtype, a, w)
        tag = "W one-hot" if mirrored else "A one-hot"
        _exact(_launch(dev, pb, EPI_F32, cfg), want, tag + ", EPI_F32")
        _exact(_launch(dev, pb, EPI_BF16, cfg), G.rne_op(want, dtype), tag + ", EPI_BF16")


# ---- c. random data: the per-element bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES_SLOW, ids=_ids(CASES_SLOW))
def test_gaussian_data_within_the_summation_bound(dev, dtype, case):
    """A ~ N(0, 1), W ~ N(0, 0.05^2), bias and residual ~ N(0, 1): |got - fp64| <= K 2^-23 sum_k |a_k w_k| + half an ulp of the output type at
    |fp64| (gemm_ref.sum_bound: derived, order independent), element by element."""
    cfg, M, N, K = case
    a, w, bias, resid = G.gauss_operands(M, N, K, dtype, M * 7 + K)
    assert G.bound_covers_epilogue(a, w, bias, resid)
    pb = Problem(dev, dtype, a, w, bias, resid)
    ref = a.double() @ w.double().t() + bias.double()
    sb = G.sum_bound(a, w)
    # worst err / bound measured on an MI355X over every case of both builds: EPI_F32 0.025, EPI_F32_RESID 0.037, 16-bit store 0.998 (the
    # half ulp of a value next to a tie); EXPERIMENTS.md, GEMM pinning
    _within(_launch(dev, pb, EPI_F32, cfg), ref, sb, "EPI_F32")
    _within(_launch(dev, pb, EPI_F32_RESID, cfg), ref + resid.double(), sb, "EPI_F32_RESID")
    _within(_launch(dev, pb, EPI_BF16, cfg), ref, sb + G.store_half_ulp(ref, dtype), "EPI_BF16")


# ---- d. activation epilogues ------------------------------------------------------------------------------------------------------------------------
def _check_activations(dev, dtype, cfg, M, N, K, seed, rs=None, what=""):
    a, w, bias = G.act_operands(M, N, K, seed)
    pb = Problem(dev, dtype, a, w, bias, rs=rs)
    x0, ok = G.exact_epilogue(a, w, None, None, rs)
    x, okb = G.exact_epilogue(a, w, bias, None, rs)
    assert ok and okb and float(x.abs().max()) <= G.XMAX
    xn = x.numpy()
    for epi, f64, e, name in ((EPI_GELU, G.gelu64, G.e_gelu, "GELU"), (EPI_QGELU, G.qgelu64, G.e_qgelu, "quick-GELU")):
        ref = torch.from_numpy(f64(xn))
        # worst err / bound measured on an MI355X: GELU 1.000, quick-GELU 0.999, SwiGLU 0.999 (values next to a tie of the store)
        _within(_launch(dev, pb, epi, cfg), ref, torch.from_numpy(e(xn)) + G.store_half_ulp(ref, dtype), what + name)
    if N % 32 == 0:
        g, up = G.swiglu_split(x0)                       # no bias in the SwiGLU epilogue
        ref = torch.from_numpy(G.silu64(g.numpy()) * up.numpy())
        _within(_launch(dev, pb, EPI_SWIGLU, cfg, bias=False), ref, torch.from_numpy(G.e_swiglu(g.numpy(), up.numpy())) + G.store_half_ulp(ref, dtype),
                what + "SwiGLU")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES_SLOW, ids=_ids(CASES_SLOW))
def test_activation_epilogues_within_their_documented_error(dev, dtype, case):
    """Integer operands and a bias of multiples of 2^-6: the pre-activation x is an exact fp32 number, dense over [-10, 10] with the GELU tail
    below -3.5, so the only errors are the activation's own (gemm_ref.e_gelu / e_qgelu / e_swiglu, from what vt_common.h documents; the host
    tests hold float32 restatements of the three to it) and one store: |got - f64(x)| <= e(x) + half an ulp of the output type."""
    cfg, M, N, K = case
    _check_activations(dev, dtype, cfg, M, N, K, M + 3 * K)


# ---- row_scale ---------------------------------------------------------------------------------------------------------------------------------------
RS_CASES = [(cfg, M, G.N_RAGGED, max(G.k_rule(cfg)[0], 128)) for cfg in G.ROW_SCALE_CFGS for M in (37, 64, G.TILE_ROWS.get(cfg, 64) + 37)]
assert all(G.legal(*c, row_scale=True) for c in RS_CASES)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", RS_CASES, ids=_ids(RS_CASES))
def test_row_scale_by_powers_of_two_is_exact(dev, dtype, case):
    """epi(row_scale[m] * (a w^T) + bias) with factors 2^-2 .. 2^2 and every 7th row 2^10 on every configuration that takes a row scale, at
    M <= 64 (which stays on the tile kernels) and on a ragged second tile row: scaling by a power of two is exact, so the integer family
    stays exact; the 2^10 rows pass 65504, where the fp16 build must saturate and the bf16 build must not. SwiGLU, GELU: within e(x)."""
    cfg, M, N, K = case
    a, w = G.int_operands(M, N, K, M + K)
    bias, rs = G.frac_vector(N, K, frac=False), G.pow2_scales(M, M, big=10)
    pb = Problem(dev, dtype, a, w, bias, rs=rs)
    y, ok = G.exact_epilogue(a, w, bias, None, rs)
    assert ok and float(y.abs().max()) > 65504.0
    _exact(_launch(dev, pb, EPI_F32, cfg), y.float(), "EPI_F32")
    want = G.rne_op(y, dtype)
    assert (float(want.float().abs().max()) == 65504.0) == (dtype == torch.float16)
    _exact(_launch(dev, pb, EPI_BF16, cfg), want, "EPI_BF16")
    _check_activations(dev, dtype, cfg, M, N, K, M, rs=G.pow2_scales(M, M + 1, lo=-1, hi=0), what="row_scale, ")


# ---- planner seams -----------------------------------------------------------------------------------------------------------------------------------
def _smallest(pred, Ms, Ns, Ks, epi):
    from vitron_amd import ops
    best = None
    for M in Ms:
        for N in Ns:
            for K in Ks:
                plan = ops.gemm_plan_cols(M, N, K, epi)
                if pred(plan) and (best is None or M * N * K < best[0] * best[1] * best[2]):
                    best = (M, N, K, plan)
    return best


# candidate grid of the seam searches: row counts just past whole tile rows; N up to 128 / 129 column tiles of 256, every N ragged (N % 256 =
# 32: the last column tile holds 32 columns) so that W stays under 150 MB; the shortest K at which the planner splits (K >= 2048)
SEAM_MS = (65, 129, 200, 257, 321, 513, 577, 641, 769)
SEAM_NS = tuple(256 * t - 224 for t in (16, 32, 64, 86, 87, 128, 129))


def _seam_checks(dev, dtype, M, N, K, what):
    """families a and b across a split: the second launch's A / W / C / bias offsets must land exactly where the first launch stopped"""
    a, w = G.int_operands(M, N, K, 5)
    bias = G.frac_vector(N, 6)
    pb = Problem(dev, dtype, a, w, bias)
    y, ok = G.exact_epilogue(a, w, bias)
    assert ok
    _exact(_launch(dev, pb, EPI_F32), y.float(), what + ", integers, EPI_F32 + bias")
    _exact(_launch(dev, pb, EPI_BF16), G.rne_op(y, dtype), what + ", integers, EPI_BF16 + bias")
    del pb
    for mirrored in (False, True):
        a, w, want = G.onehot_problem(M, N, K, dtype, 7, mirrored)
        _exact(_launch(dev, Problem(dev, dtype, a, w), EPI_F32), want, what + (", W" if mirrored else ", A") + " one-hot, EPI_F32")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_row_split_seam_is_exact(dev, dtype):
    """the smallest shape of the grid whose AUTO plan runs rows [0, rows_first) on whole rounds of big tiles and plans the rest again"""
    found = _smallest(lambda p: p[1] > 0, SEAM_MS, SEAM_NS, (2048,), EPI_BF16)
    assert found is not None, "no shape of the grid takes the planner's row split any more: widen SEAM_MS / SEAM_NS"
    M, N, K, plan = found
    from vitron_amd import ops
    assert 0 < plan[1] < M and ops.gemm_plan_cols(M, N, K, EPI_F32)[1] == plan[1]
    _seam_checks(dev, dtype, M, N, K, f"row split {M}x{N}x{K} at row {plan[1]}")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_column_split_seam_is_exact(dev, dtype):
    """the smallest shape of the grid whose AUTO plan runs columns [0, cols_first) on whole rounds of big tiles and plans the tail columns
    again: W, C and the bias move by cols_first, a SwiGLU output by cols_first / 2"""
    from vitron_amd import ops
    found = _smallest(lambda p: p[2] > 0, SEAM_MS, SEAM_NS, (2048,), EPI_BF16)
    assert found is not None, "no shape of the grid takes the planner's column split any more: widen SEAM_MS / SEAM_NS"
    M, N, K, plan = found
    assert 0 < plan[2] < N and plan[1] == 0
    for epi in (EPI_F32, EPI_SWIGLU):
        assert ops.gemm_plan_cols(M, N, K, epi)[2] == plan[2]
    what = f"column split {M}x{N}x{K} at column {plan[2]}"
    _seam_checks(dev, dtype, M, N, K, what)
    # SwiGLU across the seam: integers again (exact gate and up), the output column of the tail starts at cols_first / 2
    a, w, _ = G.act_operands(M, N, K, 8)
    g, up = G.swiglu_split(G.exact_epilogue(a, w)[0])
    ref = torch.from_numpy(G.silu64(g.numpy()) * up.numpy())
    got = _launch(dev, Problem(dev, dtype, a, w), EPI_SWIGLU)
    _within(got, ref, torch.from_numpy(G.e_swiglu(g.numpy(), up.numpy())) + G.store_half_ulp(ref, dtype), what + ", SwiGLU")


VARIANT_MS = (65, 129, 161, 225, 257, 321, 449, 513)
VARIANT_NS = (288, 1056, 4128, 8224, 16416, 22048)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("variant", [13, 14, 15, 16, 2, 5])
def test_auto_reaches_every_planned_kernel(dev, dtype, variant):
    """the smallest shape of the grid for which the AUTO plan is this configuration in one launch: exact there through AUTO itself"""
    found = _smallest(lambda p: p == (variant, 0, 0), VARIANT_MS, VARIANT_NS, (256, 2048, 4096), EPI_BF16)
    assert found is not None, f"no shape of the grid plans configuration {variant} any more: widen VARIANT_MS / VARIANT_NS"
    M, N, K, _ = found
    a, w = G.int_operands(M, N, K, variant)
    bias = G.frac_vector(N, variant + 1)
    pb = Problem(dev, dtype, a, w, bias)
    y, ok = G.exact_epilogue(a, w, bias)
    assert ok
    _exact(_launch(dev, pb, EPI_BF16), G.rne_op(y, dtype), f"AUTO -> cfg {variant} at {M}x{N}x{K}, EPI_BF16 + bias")
    a, w, want = G.onehot_problem(M, N, K, dtype, variant)
    _exact(_launch(dev, Problem(dev, dtype, a, w), EPI_F32), want, f"AUTO -> cfg {variant} at {M}x{N}x{K}, A one-hot, EPI_F32")


# ---- split-K -----------------------------------------------------------------------------------------------------------------------------------------
def _splitk(dev, pb, ks, work_floats, want, what, expect_ks):
    """one vt_gemm_bf16_resid_splitk launch into a NaN workspace `work_floats` + 1024 floats long: the result exact, the partial sums of
    expect_ks K ranges -- and nothing else -- written (expect_ks = 0: the workspace untouched)"""
    work = None if work_floats is None else torch.full((work_floats + 1024,), NAN, dtype=torch.float32, device=dev)
    _exact(_launch(dev, pb, EPI_F32_RESID, splitk=ks, work=work), want, what)
    if work is not None:
        used = int((~torch.isnan(work)).sum())
        assert used == expect_ks * pb.M * pb.N and bool(torch.isnan(work[expect_ks * pb.M * pb.N:]).all()), \
            f"{what}: {used} workspace floats written, expected the first {expect_ks} x {pb.M} x {pb.N}"


SPLITK_CASES = [(M, G.N_RAGGED, K, ks) for M, K in ((300, 2176), (250, 1024), (65, 2304)) for ks in range(2, 9) if (K >> 7) // ks >= 2]


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K,ks", SPLITK_CASES)
def test_forced_split_k_is_exact(dev, dtype, M, N, K, ks):
    """ksplit = 2 .. 8 (K / 128 = 17 and 18 steps: divisible by few of them), on the 224-row (M = 300) and the 256-row (M = 250, 65) first pass, a
    ragged N: the integer family makes partial sums and their ordered reduce exact, so C + A W^T + bias comes back bit for bit"""
    a, w = G.int_operands(M, N, K, ks)
    bias, resid = G.frac_vector(N, K), G.frac_vector(M * N, K + 1).reshape(M, N)
    pb = Problem(dev, dtype, a, w, bias, resid)
    y, ok = G.exact_epilogue(a, w, bias, resid)
    assert ok
    _splitk(dev, pb, ks, ks * M * N, y.float(), f"ksplit {ks}", ks)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_dispatched_split_k_is_exact(dev, dtype):
    """ksplit = 0: with a workspace the dispatcher splits 300 x 1024 x 4096 (8 tiles of 256 x 256, a long K loop) eight ways; without one, or
    with one that is too small for its choice, it never splits and touches no workspace"""
    M, N, K = 300, 1024, 4096
    a, w = G.int_operands(M, N, K, 1)
    bias, resid = G.frac_vector(N, 2), G.frac_vector(M * N, 3).reshape(M, N)
    pb = Problem(dev, dtype, a, w, bias, resid)
    y, ok = G.exact_epilogue(a, w, bias, resid)
    assert ok
    _splitk(dev, pb, 0, 8 * M * N, y.float(), "ksplit 0 with a workspace", 8)
    _splitk(dev, pb, 0, None, y.float(), "ksplit 0 without a workspace", 0)
    _splitk(dev, pb, 0, 8 * M * N - 2048, y.float(), "ksplit 0 with a workspace one KiB-block short", 0)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_row_split_remainder_splits_k(dev, dtype):
    """ksplit = 0 on the smallest shape of the grid whose residual plan runs whole rounds of big tiles first and whose remaining rows (few
    tiles, K = 4096) then split K eight ways: the recursion's A / C offsets and the remainder's partial sums, exact"""
    from vitron_amd import ops
    found = _smallest(lambda p: p[1] > 0, (4161, 4225, 4353), (8192 - 224, 8192), (4096,), EPI_F32_RESID)
    assert found is not None, "no shape of the grid takes the residual GEMM's row split any more"
    M, N, K, plan = found
    R = M - plan[1]
    tiles = -(-R // 256) * -(-N // 256)
    assert 64 < R <= 256 and tiles <= 32 and tiles * 8 >= 128 and N % 32 == 0      # the dispatcher's own conditions for 8 splits of the remainder
    a, w = G.int_operands(M, N, K, 4)
    bias, resid = G.frac_vector(N, 5), G.frac_vector(M * N, 6).reshape(M, N)
    pb = Problem(dev, dtype, a, w, bias, resid)
    y, ok = G.exact_epilogue(a, w, bias, resid)
    assert ok
    work = torch.full((8 * R * N + 1024,), NAN, dtype=torch.float32, device=dev)
    _exact(_launch(dev, pb, EPI_F32_RESID, splitk=0, work=work), y.float(), f"ksplit 0, {M}x{N}x{K}, rows [0, {plan[1]}) first")
    used = int((~torch.isnan(work)).sum())
    assert used == 8 * R * N and bool(torch.isnan(work[8 * R * N:]).all()), f"{used} workspace floats written, expected 8 x {R} x {N}: the remainder did not split K"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_c_untouched(dev):
    """Arguments the C ABI documents as unsupported raise before any launch: C keeps its bits."""
    from vitron_amd import ops
    from vitron_amd._lib import VitronHipError
    dtype = torch.bfloat16
    M, N, K = 70, 64, 128
    abuf = torch.ones((M + 2, K + 24), dtype=dtype, device=dev)
    wbuf = torch.ones((N + 2, K + 24), dtype=dtype, device=dev)
    cbuf = torch.full((M, N + 8), NAN, dtype=dtype, device=dev)
    c32 = torch.full((M, N + 8), NAN, dtype=torch.float32, device=dev)
    ok_a, ok_w = abuf[:M, 8:8 + K], wbuf[:N, 8:8 + K]

    def refused(what, fn):
        with pytest.raises(VitronHipError):
            fn()
        torch.cuda.synchronize()
        assert bool(torch.isnan(cbuf.float()).all()) and bool(torch.isnan(c32).all()), what + ": C was written"

    lda4 = torch.ones((M + 2, K + 28), dtype=dtype, device=dev)[:M, 8:8 + K]                    # lda = K + 28: a multiple of 4, not of 8
    assert lda4.stride(0) % 8 == 4
    refused("lda % 8 != 0", lambda: ops.gemm(lda4, ok_w, None, EPI_BF16, out=cbuf[:, :N]))
    refused("ldw % 8 != 0", lambda: ops.gemm(ok_a, torch.ones((N, K + 28), dtype=dtype, device=dev)[:, :K], None, EPI_BF16, out=cbuf[:, :N]))
    refused("A 8 bytes off", lambda: ops.gemm(abuf[:M, 4:4 + K], ok_w, None, EPI_BF16, out=cbuf[:, :N]))
    refused("C 8 bytes off", lambda: ops.gemm(ok_a, ok_w, None, EPI_BF16, out=cbuf[:, 4:4 + N]))
    refused("ldc % 4 != 0", lambda: ops.gemm(ok_a, ok_w, None, EPI_BF16, out=torch.full((M, N + 2), NAN, dtype=dtype, device=dev)[:, :N]))
    for cfg in (2, 5, 10, 13):
        refused(f"K % 64 != 0 on cfg {cfg}", lambda: ops.gemm(abuf[:M, 8:8 + 72], wbuf[:N, 8:8 + 72], None, EPI_BF16, out=cbuf[:, :N], cfg=cfg))
    refused("N % 4 != 0", lambda: ops.gemm(ok_a, wbuf[:N - 2, 8:8 + K], None, EPI_BF16, out=cbuf[:, :N - 2]))
    K2 = 1024
    a2, w2 = torch.ones((M, K2), dtype=dtype, device=dev), torch.ones((N, K2), dtype=dtype, device=dev)
    small = torch.full((2 * M * N - 1,), NAN, dtype=torch.float32, device=dev)
    refused("split-K workspace too small", lambda: ops.gemm_resid_splitk(a2, w2, c32[:, :N], None, 2, small))
    assert bool(torch.isnan(small).all())
    refused("split-K without a workspace", lambda: ops.gemm_resid_splitk(a2, w2, c32[:, :N], None, 2, None))
    # layouts ops refuses itself: a transposed view, overlapping rows, a wrong dtype, a view of the wrong shape
    refused("transposed A", lambda: ops.gemm(torch.ones((K, M), dtype=dtype, device=dev).t(), ok_w, None, EPI_BF16, out=cbuf[:, :N]))
    refused("overlapping rows", lambda: ops.gemm(ok_a, ok_w, None, EPI_BF16, out=cbuf[0, :N].expand(M, N)))
    refused("column-strided C", lambda: ops.gemm(ok_a, wbuf[:4, 8:8 + K], None, EPI_BF16, out=cbuf[:, 0:8:2]))
    refused("C view of the wrong shape", lambda: ops.gemm(ok_a, ok_w, None, EPI_BF16, out=cbuf[:M - 1, :N]))
    refused("fp32 C for a 16-bit epilogue", lambda: ops.gemm(ok_a, ok_w, None, EPI_BF16, out=c32[:, :N]))
    # and the same views, aligned, are accepted
    got = ops.gemm(ok_a, ok_w, None, EPI_BF16, out=cbuf[:, :N])
    torch.cuda.synchronize()
    assert bool((got.float() == K).all()) and bool(torch.isnan(cbuf[:, N:].float()).all())
    # an epilogue id outside the seven public values is refused for every configuration (K = 256: nothing else is wrong for any of them);
    # 0x1000 .. 0x10000 used to select a kernel family by accident, 0x4005 stored fp32 into a C laid out for 16 bits
    K3 = 256
    a3, w3 = torch.ones((M, K3), dtype=dtype, device=dev), torch.ones((N, K3), dtype=dtype, device=dev)
    cbuf.fill_(NAN)
    for cfg in (0, 5, 6, 10, 13, 15):
        for e in (7, 11, -1, 0x1000, 0x4000, 0x4005, 0x10000):
            refused(f"epilogue id {e:#x} on cfg {cfg}", lambda: ops.gemm(a3, w3, None, e, out=cbuf[:, :N], cfg=cfg))
    for cfg in (0, 5, 6, 10, 13, 15):
        cbuf.fill_(NAN)
        got = ops.gemm(a3, w3, None, EPI_BF16, out=cbuf[:, :N], cfg=cfg)
        torch.cuda.synchronize()
        assert bool((got.float() == K3).all()) and bool(torch.isnan(cbuf[:, N:].float()).all()), f"EPI_BF16 on cfg {cfg}"
