"""The normalisations on the GPU against tests/norm_ref.py, element by element, in both operand builds: vt_rmsnorm on each of its three
kernels (rmsnorm_row_block_kernel below 2048 rows, rmsnorm_stream_kernel from 2048 rows, rmsnorm_kernel from 2048 rows with a row index)
and vt_layernorm at every chunk count of their dispatch, full and ragged; the RMSNorm folded into the 16-bit GEMMs: the decode flavour
(ops.gemm_norm: producer and consumer side of gemm_skinny_dma_kernel) and the tile flavour (ops.gemm_resid_norm: the producers in
launch_tile, the 256x256 kernels and the split-K reduce pass; ops.rowscale_finalize; the row_scale consumer). One-hot rows and small
integers with power-of-two weights are compared bit for bit, Gaussian data inside the derived bounds with no element exempt. Every output
is a view inside a NaN-filled buffer whose guards must still be NaN afterwards (vt_rmsnorm / vt_layernorm take no row stride: guard rows
only). DESIGN.md "Norm pinning" says which shape reaches which path."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests import norm_ref as NR
from tests.gemm_ref import EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_GELU, EPI_SWIGLU, U
from tests.test_gpu_gemm import COL0, GAP, NAN, Problem, _bits, _exact, _padded, _where

pytestmark = pytest.mark.gpu
DT_IDS = ["bf16", "fp16"]
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


def _within(got, ref64, bound, what):
    """|got - ref64| <= bound element by element, no element exempt (a zero bound asks for the exact value) -> the worst err / bound"""
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    worst = float(ratio.max())
    print(f"[{what}] worst err / bound {worst:.3f}")                    # shown with -s: the figures EXPERIMENTS.md records
    assert not bool(bad.any()), _where(bad, got, ref64, what) + f"; worst err / bound {worst:.3f}"
    return worst


class Window:
    """out = buf[2 : 2 + M, 8 : 8 + N] of a NaN buffer 5 rows taller and 24 columns wider (`init`: the window's content before the launch);
    check(): every bit outside the window as before, no NaN inside -> the window on the host"""

    def __init__(self, dev, M, N, dtype, init=None):
        self.M, self.N = M, N
        self.buf = torch.full((GAP + M + 3, COL0 + N + 16), NAN, dtype=dtype, device=dev)
        self.win = self.buf[GAP:GAP + M, COL0:COL0 + N]
        if init is not None:
            self.win.copy_(init)
        self.before = _bits(self.buf).clone()

    def check(self, what):
        torch.cuda.synchronize()
        same = _bits(self.buf) == self.before
        same[GAP:GAP + self.M, COL0:COL0 + self.N] = True
        assert bool(same.all()), f"{what}: {int((~same).sum())} elements written outside the {self.M} x {self.N} window, first at {(~same).nonzero()[0].tolist()}"
        got = self.win.cpu()
        assert not bool(torch.isnan(got.float()).any()), f"{what}: NaN in the result"
        return got


def _guarded_rows(dev, rows, D, dtype):
    buf = torch.full((2 + rows + 3, D), NAN, dtype=dtype, device=dev)
    return buf, buf[2:2 + rows]


def _guards_are_nan(buf, rows, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:2].float()).all()) and bool(torch.isnan(buf[2 + rows:].float()).all()), what + ": guard rows written"


def _record(record_property, name, worst):
    record_property(name, round(float(worst), 4))


# ---- the device rsqrtf ------------------------------------------------------------------------------------------------------------------------
def test_rsqrt_error_is_inside_the_constant(dev, record_property):
    """norm_ref.RSQRT_ULPS is the measured error of the device rsqrtf + 1 ulp: 2^16 log-spaced arguments in [1e-6, 1e6] through
    vt_rowscale_finalize (one group, inv_dim 1, eps 0: out = rsqrtf(x * 1 + 0)), against fp64, in units of 2^-23 relative."""
    from vitron_amd import ops
    x = torch.from_numpy(np.logspace(-6, 6, 2 ** 16).astype(np.float32))
    got = ops.rowscale_finalize(x.to(dev).reshape(1, -1), x.numel(), 1.0, 0.0).cpu().double()
    ref = 1.0 / torch.sqrt(x.double())
    worst = float(((got - ref).abs() / ref).max()) / 2.0 ** -23
    print(f"[rsqrtf] worst relative error {worst:.3f} x 2^-23")
    _record(record_property, "rsqrtf_rel_err_in_2^-23", worst)
    assert worst + 1.0 <= NR.RSQRT_ULPS


# ---- vt_rmsnorm ----------------------------------------------------------------------------------------------------------------------------------
SRC_ROWS = 4097
# (rows, with idx): 1, 5, 2047 rows: rmsnorm_row_block_kernel; 2048, 2049, 4097: rmsnorm_stream_kernel, 2048 waves, wave 0 walks 1, 2, 3 rows;
# 2048, 2051 rows through an index: rmsnorm_kernel; 5 rows through an index: the row-block kernel's gather
RMS_LAUNCHES = [(1, False), (5, False), (2047, False), (2048, False), (2049, False), (4097, False), (5, True), (2048, True), (2051, True)]
_rms_cache = {}


def _rms_problem(dev, D):
    """one Gaussian source of 4097 rows per width (scale 2, g = 1 + N(0, 1)), its fp64 reference and both bounds, shared by every launch"""
    if D not in _rms_cache:
        _rms_cache.clear()
        gen = torch.Generator().manual_seed(D)
        x = torch.randn((SRC_ROWS, D), generator=gen) * 2.0
        g = 1.0 + torch.randn((D,), generator=gen)
        y64 = NR.rms_ref(x, g, EPS)
        _rms_cache[D] = dict(x=x.to(dev), g=g.to(dev), y64=y64, bound={dt: NR.rms_bound(y64, dt) for dt in G.DTYPES})
    return _rms_cache[D]


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", NR.D_SET)
def test_rmsnorm_gaussian_rows_within_the_bound_on_every_kernel(dev, dtype, D, record_property):
    """every element of every launch within half an ulp of the store + |y| (E_RSTD_RMS + 2 u) of fp64. The first 2047 rows go through the
    row-block kernel and again inside the 2049- and 4097-row launches of the stream kernel: each is held to the bound on its own."""
    from vitron_amd import ops
    pb = _rms_problem(dev, D)
    worst = 0.0
    for rows, with_idx in RMS_LAUNCHES:
        idx = None
        if with_idx:                                     # a permutation of the first `rows` source rows with repeats and rows past `rows`
            rng = np.random.default_rng(rows + D)
            sel = rng.permutation(rows)
            sel[::7] = rng.integers(0, SRC_ROWS, size=sel[::7].shape)
            idx = torch.from_numpy(sel.astype(np.int32))
        buf, y = _guarded_rows(dev, rows, D, dtype)
        ops.rmsnorm(pb["x"] if with_idx else pb["x"][:rows], pb["g"], EPS, idx=None if idx is None else idx.to(dev), dtype=dtype, out=y)
        what = f"rmsnorm {rows} x {D}" + (" idx" if with_idx else "")
        _guards_are_nan(buf, rows, what)
        pick = idx.long() if with_idx else slice(0, rows)
        worst = max(worst, _within(y.cpu(), pb["y64"][pick], pb["bound"][dtype][pick], what))
    _record(record_property, "worst_err_over_bound", worst)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", NR.D_SET)
def test_rmsnorm_one_hot_rows(dev, dtype, D, record_property):
    """Row r holds one full-mantissa fp32 value c at column (7 r + 5) mod D: every other output is exactly +-0 and the hit column is
    g c / sqrt(c^2 / D + eps) within the bound (a kernel that left c out of its sum returns g c / sqrt(eps)). max(D, 2049) rows, so that
    every column is hit on the row-block kernel (launches of at most 2047 rows), on the stream kernel (one launch) and on the indexed kernel."""
    from vitron_amd import ops
    R = max(D, 2049)
    x, cols, c = NR.onehot_rows(R, D, D + 1)
    g = 1.0 + torch.randn((D,), generator=torch.Generator().manual_seed(D))
    want = NR.onehot_want(c, g.double()[torch.from_numpy(cols)], D, EPS)
    bound = G.store_half_ulp(want, dtype) + want.abs() * (NR.E_RSTD_RMS + 2 * U)
    xd, gd = x.to(dev), g.to(dev)
    rng = np.random.default_rng(D)
    sel = np.concatenate([rng.permutation(R), rng.integers(0, R, size=3)])
    launches = [(f"row-block rows {s}..", torch.arange(s, min(s + 2047, R)), False) for s in range(0, R, 2047)]
    launches += [("stream", torch.arange(R), False), ("indexed", torch.from_numpy(sel), True)]
    worst = 0.0
    for what, rows_idx, with_idx in launches:
        n = rows_idx.numel()
        assert (n < 2048) == what.startswith("row-block")
        buf, y = _guarded_rows(dev, n, D, dtype)
        if with_idx:
            ops.rmsnorm(xd, gd, EPS, idx=rows_idx.to(torch.int32).to(dev), dtype=dtype, out=y)
        else:
            ops.rmsnorm(xd[int(rows_idx[0]):int(rows_idx[-1]) + 1], gd, EPS, dtype=dtype, out=y)
        _guards_are_nan(buf, n, what)
        got = y.cpu().double()
        hit_cols = torch.from_numpy(cols)[rows_idx]
        hit = got[torch.arange(n), hit_cols]
        err = (hit - want[rows_idx]).abs()
        ratio = err / bound[rows_idx]
        assert bool((ratio <= 1.0).all()), f"{what}, D={D}: {int((ratio > 1).sum())} hit columns off, first row {int((ratio > 1).nonzero()[0])}, worst {float(ratio.max()):.3f}"
        worst = max(worst, float(ratio.max()))
        got[torch.arange(n), hit_cols] = 0.0
        assert bool((got == 0).all()), f"{what}, D={D}: {int((got != 0).sum())} elements of all-zero columns are not +-0"
    _record(record_property, "worst_err_over_bound", worst)


# ---- vt_layernorm -------------------------------------------------------------------------------------------------------------------------------
LN_ROWS = 37                                             # ten blocks of four waves, the last one ragged


def _ln_check(dev, dtype, x, g, b, what):
    from vitron_amd import ops
    rows, D = x.shape
    buf, y = _guarded_rows(dev, rows, D, dtype)
    xd = x.to(dev)
    ops.layernorm(xd, g.to(dev), b.to(dev), EPS, dtype=dtype, out=y)
    _guards_are_nan(buf, rows, what)
    assert torch.equal(xd.cpu(), x), what + ": x changed without a temporal embedding"
    y64, t64, r64 = NR.ln_ref(x, g, b, EPS)
    return _within(y.cpu(), y64, NR.ln_bound(x, g, y64, t64, r64, dtype), what)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", NR.D_SET)
def test_layernorm_gaussian_and_offset_rows_within_the_bound(dev, dtype, D, record_property):
    """Gaussian rows of scale 2, and rows 1000 + N(0, 1) whose variance a one-pass E[x^2] - E[x]^2 would cancel away: every element inside
    norm_ref.ln_bound"""
    gen = torch.Generator().manual_seed(D + 11)
    g, b = 1.0 + torch.randn((D,), generator=gen), torch.randn((D,), generator=gen)
    w0 = _ln_check(dev, dtype, torch.randn((LN_ROWS, D), generator=gen) * 2.0, g, b, f"layernorm {LN_ROWS} x {D}")
    w1 = _ln_check(dev, dtype, 1000.0 + torch.randn((LN_ROWS, D), generator=gen), g, b, f"layernorm {LN_ROWS} x {D}, rows 1000 + N(0, 1)")
    _record(record_property, "worst_err_over_bound", w0)
    _record(record_property, "worst_err_over_bound_offset_rows", w1)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", [d for d in NR.D_SET if d & (d - 1) == 0])
def test_layernorm_of_constant_rows_is_beta(dev, dtype, D):
    """rows of one power of two, D a power of two: the sum, the mean and every difference are exact, so y == op16(beta) bit for bit"""
    from vitron_amd import ops
    gen = torch.Generator().manual_seed(D)
    g, b = 1.0 + torch.randn((D,), generator=gen), torch.randn((D,), generator=gen)
    x = torch.exp2(torch.arange(LN_ROWS).float() % 9 - 4)[:, None].expand(LN_ROWS, D).contiguous()
    buf, y = _guarded_rows(dev, LN_ROWS, D, dtype)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), EPS, dtype=dtype, out=y)
    _guards_are_nan(buf, LN_ROWS, "constant rows")
    _exact(y.cpu(), G.rne_op(b, dtype)[None, :].expand(LN_ROWS, D), f"layernorm of constant rows, D={D}")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", [4, 320, 4096])
def test_layernorm_temporal_embedding_add_is_one_fp32_add(dev, dtype, D):
    """x[row] += temb[(row // 5) % 3] for the first 37 rows, written back: torch.equal to the fp32 sum; the rows of x behind them keep their
    bits; y is the LayerNorm of the sum"""
    from vitron_amd import ops
    T, tpf, spare = 3, 5, 3
    gen = torch.Generator().manual_seed(D + 5)
    x = torch.randn((LN_ROWS + spare, D), generator=gen) * 2.0
    temb = torch.randn((T, D), generator=gen)
    g, b = 1.0 + torch.randn((D,), generator=gen), torch.randn((D,), generator=gen)
    want_x = x.clone()
    want_x[:LN_ROWS] = x[:LN_ROWS] + temb[(torch.arange(LN_ROWS) // tpf) % T]
    xd = x.to(dev)
    buf, y = _guarded_rows(dev, LN_ROWS, D, dtype)
    ops.layernorm(xd, g.to(dev), b.to(dev), EPS, temb=temb.to(dev), tokens_per_frame=tpf, dtype=dtype, out=y, rows=LN_ROWS)
    _guards_are_nan(buf, LN_ROWS, "temb")
    assert torch.equal(xd.cpu(), want_x)
    y64, t64, r64 = NR.ln_ref(want_x[:LN_ROWS], g, b, EPS)
    _within(y.cpu(), y64, NR.ln_bound(want_x[:LN_ROWS], g, y64, t64, r64, dtype), f"layernorm after the temb add, D={D}")


# ---- the decode flavour of the fold: ops.gemm_norm ------------------------------------------------------------------------------------------
DECODE_MS = (1, 7, 8, 9, 16)                            # <= 8 rows: XI = 1; 9 .. 16: XI = 2


def _nan_partials(dev, M, n, spare_rows=2):
    buf = torch.full((M + spare_rows, n), NAN, device=dev)
    return buf, buf[:M]


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M", DECODE_MS)
def test_decode_producer_is_exact(dev, dtype, M):
    """x += a w^T of small integers, w_next powers of two: C, xw = op16(x w_next) and the per-16-column sums of x^2 come back bit for bit
    (16 max(x^2) < 2^24: asserted by fold_producer_ints); nothing behind row M of C, xw or the partial sums is written"""
    from vitron_amd import ops
    for N in (32, 96, 1024):                             # 96: a multiple of 32, not of 64
        for K in (64, 192):
            p = NR.fold_producer_ints(M, N, K, M + N + K, 16)
            pb = Problem(dev, dtype, p["a"], p["w"])
            c = Window(dev, M, N, torch.float32, init=p["resid"])
            xw = Window(dev, M, N, dtype)
            pbuf, part = _nan_partials(dev, M, N // 16)
            ops.gemm_norm(pb.a, pb.w, EPI_F32_RESID, out=c.win, norm_out=(p["wn"].to(dev), xw.win, part))
            what = f"decode producer {M}x{N}x{K}"
            _exact(c.check(what), p["x64"].float(), what + ", C")
            _exact(xw.check(what), G.rne_op(p["xw64"], dtype), what + ", xw")
            _exact(part.cpu(), p["part"].float(), what + ", partial sums")
            assert bool(torch.isnan(pbuf[M:]).all()), what + ": partial sums written behind row M"


CONSUMER_EPIS = ((EPI_F32, "EPI_F32"), (EPI_BF16, "EPI_BF16"), (EPI_SWIGLU, "EPI_SWIGLU_BF16"), (EPI_F32_RESID, "EPI_F32_RESID"))


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M", DECODE_MS)
def test_decode_consumer_at_every_partial_count(dev, dtype, M, record_property):
    """in_n = 64, 128, 448, 512: 4, 8, 28, 32 partial sums per thread, i.e. 1, 2, 7, 8 of the 8 clamped 16-byte loads kept by the mask. The
    partial sums are distinct integers (their sum is exact in any order: a dropped, doubled or foreign one moves rstd by far more than
    fold_rstd_rel), the accumulator is an exact integer; everything behind row M of the partial sums is NaN and must never be read."""
    from vitron_amd import ops
    N, K = 64, 64
    a, w = G.int_operands(M, N, K, M)
    pb = Problem(dev, dtype, a, w)
    acc = (a @ w.t()).double()
    resid = G.frac_vector(M * N, M + 1, frac=False).reshape(M, N)
    worst = 0.0
    for in_n in (64, 128, 448, 512):
        part = NR.distinct_partials(M, in_n, in_n + M)
        flat = torch.full((M * in_n + 64,), NAN, device=dev)
        flat[:M * in_n] = part.reshape(-1).to(dev)
        pin = flat[:M * in_n].view(M, in_n)
        inv_dim = 1.0 / (16 * in_n)
        r64 = NR.fold_rstd64(part.double().sum(-1), inv_dim, EPS)
        e_r = NR.fold_rstd_rel(in_n // 16 + 4)
        for epi, name in CONSUMER_EPIS:
            n_out = N // 2 if epi == EPI_SWIGLU else N
            odt = torch.float32 if epi in (EPI_F32, EPI_F32_RESID) else dtype
            c = Window(dev, M, n_out, odt, init=resid if epi == EPI_F32_RESID else None)
            ops.gemm_norm(pb.a, pb.w, epi, out=c.win, norm_in=(pin, inv_dim, EPS))
            what = f"decode consumer {name} M={M} in_n={in_n}"
            ref, bound = NR.consumer_bound(acc, r64, e_r, epi, dtype, resid64=resid.double())
            worst = max(worst, _within(c.check(what), ref, bound, what))
    _record(record_property, "worst_err_over_bound", worst)


def _gauss_w(N, K, dtype, gen, std=0.05):
    return (torch.randn((N, K), generator=gen) * std).to(dtype).float()


def _producer_checks(x_got, xw_got, part_got, x64, sb, wn, width, dtype, what):
    """a Gaussian producer: x within the summation bound of fp64; xw and the partial sums against the x the GPU produced (xw: two roundings;
    a partial sum: one rounding per square and at most `width` additions, all terms non-negative)"""
    w0 = _within(x_got, x64, sb, what + ", x")
    xg = x_got.double()
    p = xg * wn.double()
    _within(xw_got, p, U * p.abs() + G.store_half_ulp(p, dtype), what + ", xw")
    ps = NR.block_sums(xg, width)
    _within(part_got, ps, (width + 2) * U * ps, what + ", partial sums")
    return w0, xg


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_decode_chain_at_the_smallest_folded_width(dev, dtype, record_property):
    """H = 1024 (the smallest width the engine folds: H % 1024 == 0), I = 192, Gaussian data, every row count: o_proj producer -> SwiGLU
    consumer (N = 2 I) -> down_proj producer (K = I) -> qkv consumer (N = 3 H), every stage element by element against fp64 of the operands
    the GPU handed on (sum_bound + the rstd term, as tests/test_gpu_nf4.py does for the 4-bit twin)"""
    from vitron_amd import ops
    H, I = 1024, 192
    gen = torch.Generator().manual_seed(7)
    wo, wgu, wd, wqkv = _gauss_w(H, H, dtype, gen), _gauss_w(2 * I, H, dtype, gen), _gauss_w(H, I, dtype, gen), _gauss_w(3 * H, H, dtype, gen)
    wo_d, wgu_d, wd_d, wqkv_d = (_padded(t, dtype, dev, 2, 8, 2, 8) for t in (wo, wgu, wd, wqkv))
    att = torch.randn((16, H), generator=gen).to(dtype).float()
    x0 = torch.randn((16, H), generator=gen)
    wn2, wn1 = 1.0 + 0.1 * torch.randn((H,), generator=gen), 1.0 + 0.1 * torch.randn((H,), generator=gen)
    e_r = NR.fold_rstd_rel(H // 256 + 4, 16)
    worst = {"producer": 0.0, "swiglu": 0.0, "qkv": 0.0}

    def producer(a_dev, a_host, w_dev, w_host, x_init, wn, M, what):
        c = Window(dev, M, H, torch.float32, init=x_init)
        xw = Window(dev, M, H, dtype)
        pbuf, part = _nan_partials(dev, M, H // 16)
        ops.gemm_norm(a_dev, w_dev, EPI_F32_RESID, out=c.win, norm_out=(wn.to(dev), xw.win, part))
        assert G.bound_covers_epilogue(a_host, w_host, None, x_init)
        x64 = a_host.double() @ w_host.double().t() + x_init.double()
        w0, xg = _producer_checks(c.check(what), xw.check(what), part.cpu(), x64, G.sum_bound(a_host, w_host), wn, 16, dtype, what)
        assert bool(torch.isnan(pbuf[M:]).all())
        worst["producer"] = max(worst["producer"], w0)
        return c, xw, part, xg

    def consumer(xw, part, xg, w_dev, w_host, epi, M, key, what):
        a_host = xw.win.cpu().float()
        r64 = NR.fold_rstd64((xg * xg).sum(-1), 1.0 / H, EPS)
        n_out = w_host.shape[0] // 2 if epi == EPI_SWIGLU else w_host.shape[0]
        c = Window(dev, M, n_out, dtype)
        ops.gemm_norm(xw.win, w_dev, epi, out=c.win, norm_in=(part, 1.0 / H, EPS))
        ref, bound = NR.consumer_bound(a_host.double() @ w_host.double().t(), r64, e_r, epi, dtype, e_acc=G.sum_bound(a_host, w_host))
        worst[key] = max(worst[key], _within(c.check(what), ref, bound, what))
        return c

    for M in DECODE_MS:
        a = _padded(att[:M], dtype, dev, 2, 8, 3, 16)
        c1, xw1, part1, xg1 = producer(a, att[:M], wo_d, wo, x0[:M], wn2, M, f"o_proj producer M={M}")
        h = consumer(xw1, part1, xg1, wgu_d, wgu, EPI_SWIGLU, M, "swiglu", f"gate/up consumer M={M}")
        c2, xw2, part2, xg2 = producer(h.win, h.win.cpu().float(), wd_d, wd, c1.win.cpu(), wn1, M, f"down_proj producer M={M}")
        consumer(xw2, part2, xg2, wqkv_d, wqkv, EPI_BF16, M, "qkv", f"qkv consumer M={M}")
    for k, v in worst.items():
        _record(record_property, "worst_err_over_bound_" + k, v)


def test_decode_fold_refusals_leave_c_untouched(dev):
    """what vt_gemm_bf16_norm documents as unsupported raises before any launch: C, xw and the partial sums keep their bits"""
    from vitron_amd import _lib, ops
    from vitron_amd._lib import VitronHipError
    dtype = torch.bfloat16
    a = torch.ones((17, 136), dtype=dtype, device=dev)
    w = torch.ones((72, 136), dtype=dtype, device=dev)
    c32 = torch.full((17, 64), NAN, device=dev)
    c16 = torch.full((17, 64), NAN, dtype=dtype, device=dev)
    xw = torch.full((17, 64), NAN, dtype=dtype, device=dev)
    part = torch.full((17, 4), NAN, device=dev)
    wn = torch.ones((64,), device=dev)
    wn40 = torch.ones((40,), device=dev)

    def refused(what, fn):
        with pytest.raises(VitronHipError):
            fn()
        torch.cuda.synchronize()
        for t in (c32, c16, xw, part):
            assert bool(torch.isnan(t.float()).all()), what + ": an output was written"

    A, W = a[:16, :128], w[:64, :128]
    pin = lambda n: torch.ones((16, n), device=dev)   # noqa: E731
    refused("M = 17", lambda: ops.gemm_norm(a[:, :128], W, EPI_F32, out=c32, norm_in=(torch.ones((17, 64), device=dev), 1 / 64, EPS)))
    refused("K % 64 != 0", lambda: ops.gemm_norm(a[:16, :72], w[:64, :72], EPI_F32, out=c32[:16], norm_in=(pin(64), 1 / 64, EPS)))
    refused("N % 32 != 0", lambda: ops.gemm_norm(A, w[:40, :128], EPI_F32, out=c32[:16, :40], norm_in=(pin(64), 1 / 64, EPS)))
    refused("in_n = 576", lambda: ops.gemm_norm(A, W, EPI_F32, out=c32[:16], norm_in=(pin(576), 1 / 576, EPS)))
    refused("in_n = 96", lambda: ops.gemm_norm(A, W, EPI_F32, out=c32[:16], norm_in=(pin(96), 1 / 96, EPS)))
    refused("producer on EPI_F32", lambda: ops.gemm_norm(A, W, EPI_F32, out=c32[:16], norm_out=(wn, xw[:16], part[:16])))
    refused("producer on EPI_BF16", lambda: ops.gemm_norm(A, W, EPI_BF16, out=c16[:16], norm_out=(wn, xw[:16], part[:16])))
    refused("unsupported epilogue", lambda: ops.gemm_norm(A, W, EPI_GELU, out=c16[:16], norm_in=(pin(64), 1 / 64, EPS)))
    lib = _lib.lib_for(dtype)                          # ops cannot express a producer without its weights: straight through the C ABI
    st = lib.vt_gemm_bf16_norm(A.data_ptr(), 136, W.data_ptr(), 136, c32.data_ptr(), 64, 16, 64, 128, EPI_F32_RESID, None, 0, 0.0, 0.0, None,
                               xw.data_ptr(), 64, part.data_ptr(), None)
    refused("producer without out_w", lambda: _lib.check(st, "vt_gemm_bf16_norm", lib))
    refused("norm_out.w of the wrong length", lambda: ops.gemm_norm(A, W, EPI_F32_RESID, out=c32[:16], norm_out=(wn40, xw[:16], part[:16])))
    # and the same views are accepted
    c32[:16] = 1.0
    ops.gemm_norm(A, W, EPI_F32_RESID, out=c32[:16], norm_out=(wn, xw[:16], part[:16]))
    torch.cuda.synchronize()
    assert bool((c32[:16] == 129.0).all()) and bool((xw[:16].float() == 129.0).all()) and bool((part[:16] == 16 * 129.0 ** 2).all())
    assert bool(torch.isnan(c32[16]).all()) and bool(torch.isnan(xw[16].float()).all()) and bool(torch.isnan(part[16]).all())


# ---- the tile flavour of the fold: ops.gemm_resid_norm, ops.rowscale_finalize ------------------------------------------------------------------
def _tile_producer(dev, dtype, p, what, **route):
    """one producer launch of integer data into NaN-guarded C, xw and partial sums [N / 32 + 2][M + 3]: all three bit for bit, the spare groups
    and the spare columns of every group still NaN"""
    from vitron_amd import ops
    M, N = p["x64"].shape
    pb = Problem(dev, dtype, p["a"], p["w"], bias=p["bias"])
    c = Window(dev, M, N, torch.float32, init=p["resid"])
    xw = Window(dev, M, N, dtype)
    part = torch.full((N // 32 + 2, M + 3), NAN, device=dev)
    ops.gemm_resid_norm(pb.a, pb.w, c.win, (p["wn"].to(dev), xw.win, part), bias=pb.bias, **route)
    _exact(c.check(what), p["x64"].float(), what + ", C")
    _exact(xw.check(what), G.rne_op(p["xw64"], dtype), what + ", xw")
    got = part.cpu()
    _exact(got[:N // 32, :M], p["part"].float().t().contiguous(), what + ", partial sums")
    got[:N // 32, :M] = NAN
    assert bool(torch.isnan(got).all()), f"{what}: {int((~torch.isnan(got)).sum())} spare partial sums written, first at {(~torch.isnan(got)).nonzero()[0].tolist()}"


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cfg", G.ROW_SCALE_CFGS)
def test_tile_producer_is_exact_on_every_configuration(dev, dtype, cfg):
    """every configuration that carries the fold (AUTO, the launch_tile grids, the 256x256 kernels) at its shortest K; M = 1 (the height of an
    M-split's remainder), 65, 300; N = 288 (a ragged last column tile) and 512"""
    K = G.k_rule(cfg)[0]
    for M in (1, 65, 300):
        for N in (G.N_RAGGED, 512):
            assert G.legal(cfg, M, N, K, EPI_F32_RESID, row_scale=True)
            p = NR.fold_producer_ints(M, N, K, M + N + K, 32, amax=2, span=200, bias=True)
            _tile_producer(dev, dtype, p, f"tile producer cfg {cfg} {M}x{N}x{K}", cfg=cfg)


def _nf_plan_rows_first(M, N, K):
    """vt_gemm_plan's verdict for a launch that carries the fold (vt_gemm.hip vt_gemm_plan_cost: with a fold only the 64x128 tiles, the
    256-row tiles and the M-split are priced; K % 128 == 0, K >= 256, N % 32 == 0 assumed): rows_first, 0 without a split. The public plan
    query prices a launch WITHOUT a fold, which has more candidates."""
    cdiv = lambda a, b: -(-a // b)   # noqa: E731
    tiles_n = cdiv(N, 256)

    def cost(m):
        small = cdiv(cdiv(m, 64) * cdiv(N, 128), 512) * (512.0 * 64 * 128 / 65536.0 / 256.0 / 0.55)
        return small if m <= 64 else min(small, float(cdiv(cdiv(m, 256) * tiles_n, 256)))

    unit = 256 * (256 // int(np.gcd(tiles_n, 256)))
    M1 = M // unit * unit
    if K >= 2048 and M > 256 and unit <= M1 < M and M1 // 256 * tiles_n // 256 + cost(M - M1) + 0.02 < cost(M):
        return M1
    return 0


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_tile_producer_across_the_row_split(dev, dtype):
    """AUTO on the smallest shape of test_gpu_gemm's seam grid whose plan WITH a fold runs whole rounds of big tiles first: the remainder's
    launch gets xw, the partial sums and C re-based by vt_nf_rows. Through vt_gemm_bf16's dispatcher and through the residual GEMM's own row
    split (ksplit = 0 with a workspace too small to split K)."""
    from tests.test_gpu_gemm import SEAM_MS, SEAM_NS
    K = 2048
    shapes = sorted((M * N, M, N) for M in SEAM_MS for N in SEAM_NS if _nf_plan_rows_first(M, N, K) > 0)
    assert shapes, "no shape of the grid takes the planner's row split with a fold any more"
    _, M, N = shapes[0]
    M1 = _nf_plan_rows_first(M, N, K)
    p = NR.fold_producer_ints(M, N, K, 3, 32, amax=1, span=200, bias=True)
    _tile_producer(dev, dtype, p, f"tile producer AUTO {M}x{N}x{K}, rows [0, {M1}) first")
    small = torch.full((1024,), NAN, device=dev)
    _tile_producer(dev, dtype, p, f"residual route {M}x{N}x{K}, rows [0, {M1}) first", ksplit=0, workspace=small)
    assert bool(torch.isnan(small).all())


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_tile_producer_through_the_split_k_reduce(dev, dtype):
    """the engine's route: forced ksplit 2 and 3 at 300 x 288 (M N / 4 = 21600 is no multiple of 64: the last wave of the reduce pass is
    ragged), and ksplit = 0 with a workspace at 300 x 992 x 4096, which the dispatcher splits eight ways (the whole workspace is written):
    the reduce pass writes C, xw and the partial sums"""
    M = 300
    for N, K, ks, amax in ((G.N_RAGGED, 1024, 2, 2), (G.N_RAGGED, 1024, 3, 2), (992, 4096, 0, 1)):
        assert (M * N // 4) % 64 != 0
        p = NR.fold_producer_ints(M, N, K, M + N + K, 32, amax=amax, span=200, bias=True)
        parts = ks or 8
        work = torch.full((parts * M * N + 1024,), NAN, device=dev)
        _tile_producer(dev, dtype, p, f"split-K producer {M}x{N}x{K} ksplit {ks}", ksplit=ks, workspace=work)
        used = int((~torch.isnan(work)).sum())
        assert used == parts * M * N and bool(torch.isnan(work[parts * M * N:]).all()), f"ksplit {ks}: {used} workspace floats written, expected {parts} x {M} x {N}"


def _int_groups(rows, np_, seed):
    """fp32 [np][rows] of integers, distinct within a row (column here) and with distinct row sums below 2^24"""
    rng = np.random.default_rng(seed)
    v = np.stack([rng.permutation(np_) for _ in range(rows)], 1).astype(np.float64) * 37 + np.arange(rows)[None, :]
    assert v.sum(0).max() < 2 ** 24
    return torch.from_numpy(v.astype(np.float32))


def test_rowscale_finalize_with_exact_partials(dev, record_property):
    """rows 1, 16, 17, 333 (one block, a full block, a second ragged one, 21 blocks), 1 .. 256 groups (under 16: some of the 16 threads of a
    row add nothing), ldp = rows + 5 with NaN in the spare columns: out within fold_rstd_rel(np / 16 + 16) of fp64, out[rows ..] untouched"""
    from vitron_amd import ops
    worst = 0.0
    for rows in (1, 16, 17, 333):
        for np_ in (1, 15, 17, 128, 256):
            v = _int_groups(rows, np_, rows + np_)
            part = torch.full((np_, rows + 5), NAN, device=dev)
            part[:, :rows] = v.to(dev)
            obuf = torch.full((rows + 8,), NAN, device=dev)
            inv_dim = 1.0 / (32 * np_)
            ops.rowscale_finalize(part, rows, inv_dim, EPS, out=obuf)
            torch.cuda.synchronize()
            assert bool(torch.isnan(obuf[rows:]).all()), f"rows={rows} np={np_}: written behind out[rows]"
            r64 = NR.fold_rstd64(v.double().sum(0), inv_dim, EPS)
            worst = max(worst, _within(obuf[:rows].cpu()[None, :], r64[None, :], NR.fold_rstd_rel(np_ // 16 + 16) * r64[None, :], f"finalize rows={rows} np={np_}"))
    _record(record_property, "worst_err_over_bound", worst)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
def test_tile_chain_producer_finalize_consumer(dev, dtype, record_property):
    """M = 300, H = 256, I = 192, Gaussian: o_proj producer -> vt_rowscale_finalize -> ops.gemm(row_scale = rstd) with SwiGLU (N = 2 I) and
    EPI_BF16 (N = 3 H), each stage per element against fp64 of what the GPU handed on"""
    from vitron_amd import ops
    M, H, I = 300, 256, 192
    gen = torch.Generator().manual_seed(11)
    wo, wgu, wqkv = _gauss_w(H, H, dtype, gen), _gauss_w(2 * I, H, dtype, gen), _gauss_w(3 * H, H, dtype, gen)
    att = torch.randn((M, H), generator=gen).to(dtype).float()
    x0 = torch.randn((M, H), generator=gen)
    wn = 1.0 + 0.1 * torch.randn((H,), generator=gen)
    pb = Problem(dev, dtype, att, wo)
    c = Window(dev, M, H, torch.float32, init=x0)
    xw = Window(dev, M, H, dtype)
    part = torch.full((H // 32 + 2, M + 3), NAN, device=dev)
    ops.gemm_resid_norm(pb.a, pb.w, c.win, (wn.to(dev), xw.win, part))
    assert G.bound_covers_epilogue(att, wo, None, x0)
    x64 = att.double() @ wo.double().t() + x0.double()
    w0, xg = _producer_checks(c.check("producer"), xw.check("producer"), part[:H // 32, :M].t().cpu(), x64, G.sum_bound(att, wo), wn, 32, dtype, "tile chain producer")
    _record(record_property, "worst_err_over_bound_producer", w0)
    rbuf = torch.full((M + 8,), NAN, device=dev)
    ops.rowscale_finalize(part[:H // 32], M, 1.0 / H, EPS, out=rbuf)
    torch.cuda.synchronize()
    assert bool(torch.isnan(rbuf[M:]).all())
    r64 = NR.fold_rstd64((xg * xg).sum(-1), 1.0 / H, EPS)
    e_r = NR.fold_rstd_rel(H // 32 // 16 + 16, 32)
    w1 = _within(rbuf[:M].cpu()[None, :], r64[None, :], e_r * r64[None, :], "tile chain rstd")
    _record(record_property, "worst_err_over_bound_rstd", w1)
    rstd = rbuf[:M].clone()
    a_host = xw.win.cpu().float()
    for w_host, epi, name in ((wgu, EPI_SWIGLU, "swiglu"), (wqkv, EPI_BF16, "qkv")):
        n_out = w_host.shape[0] // 2 if epi == EPI_SWIGLU else w_host.shape[0]
        out = Window(dev, M, n_out, dtype)
        ops.gemm(xw.win, _padded(w_host, dtype, dev, 2, 8, 2, 8), None, epi, out=out.win, row_scale=rstd)
        ref, bound = NR.consumer_bound(a_host.double() @ w_host.double().t(), r64, e_r, epi, dtype, e_acc=G.sum_bound(a_host, w_host))
        _record(record_property, "worst_err_over_bound_" + name, _within(out.check(name), ref, bound, "tile chain " + name))
