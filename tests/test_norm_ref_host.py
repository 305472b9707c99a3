"""The norm references without a GPU (tests/norm_ref.py): float32 emulations of vt_rmsnorm, vt_layernorm and of the folded RMSNorm's
consumer stay inside the per-element bounds with NO element exempt, every emulated fault (an element missing from the sum, one counted
twice, a partial sum taken from the neighbouring block, the previous row's data used for the current row) is flagged in at least half of
the rows it touches, and the integer probes of tests/test_gpu_norm.py meet the preconditions under which fp32 returns them bit for bit."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests import norm_ref as NR
from tests.gemm_ref import U

DT_IDS = ["bf16", "fp16"]
DS = (4, 128, 320, 1028, 4096)
ROWS = 64
EPS = 1e-5


def _gauss(D, seed, offset=0.0, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((ROWS, D), generator=g) * scale + offset
    return x, 1.0 + torch.randn((D,), generator=g), torch.randn((D,), generator=g)


def _violating_rows(got, ref64, bound):
    return ((got.double() - ref64).abs() > bound).any(-1)


def test_constants_follow_the_chains():
    assert NR.CHAIN == 70 and NR.CHAIN_ROW_BLOCK == 25
    assert NR.E_RSTD_RMS == ((1 + 70 + 3) / 2 + 1) * U + NR.RSQRT_ULPS * 2 * U
    assert NR.RSQRT_ULPS == 1.8 and NR.E_RSTD_RMS < 42 * U                                        # far below half an ulp of either store (2^-9, 2^-12 relative)
    assert NR.fold_rstd_rel(32 + 4) < NR.fold_rstd_rel(32 + 4, 16) < 40 * U


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("lanes", [64, 256])
def test_rmsnorm_emulation_is_inside_the_bound_everywhere(dtype, D, lanes):
    x, g, _ = _gauss(D, D + lanes)
    y64 = NR.rms_ref(x, g, EPS)
    got, _ = NR.rms_f32(x.numpy(), g.numpy(), EPS, dtype, lanes=lanes)
    assert not bool(_violating_rows(got, y64, NR.rms_bound(y64, dtype)).any())


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fault", NR.FAULTS)
def test_rmsnorm_faults_are_flagged(dtype, D, fault):
    """a fault moves rstd by about x_j^2 / (2 sum x^2) ~ 1 / (2 D): far below the store's half ulp, yet every element next to a rounding
    boundary flips, and a row has D of them"""
    x, g, _ = _gauss(D, 3 * D)
    y64 = NR.rms_ref(x, g, EPS)
    got, rows = NR.rms_f32(x.numpy(), g.numpy(), EPS, dtype, fault=fault)
    bad = _violating_rows(got, y64, NR.rms_bound(y64, dtype))[rows]
    assert int(bad.sum()) * 2 >= len(rows), f"{fault}: {int(bad.sum())} of {len(rows)} rows flagged"


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_layernorm_emulation_is_inside_the_bound_everywhere(dtype, D, offset):
    x, g, b = _gauss(D, D + 7, offset=offset, scale=1.0 if offset else 2.0)
    y64, t64, r64 = NR.ln_ref(x, g, b, EPS)
    got, _ = NR.ln_f32(x.numpy(), g.numpy(), b.numpy(), EPS, dtype)
    assert not bool(_violating_rows(got, y64, NR.ln_bound(x, g, y64, t64, r64, dtype)).any())


@pytest.mark.parametrize("dtype", G.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fault", NR.FAULTS)
def test_layernorm_faults_are_flagged(dtype, D, fault):
    x, g, b = _gauss(D, 5 * D)
    y64, t64, r64 = NR.ln_ref(x, g, b, EPS)
    got, rows = NR.ln_f32(x.numpy(), g.numpy(), b.numpy(), EPS, dtype, fault=fault)
    bad = _violating_rows(got, y64, NR.ln_bound(x, g, y64, t64, r64, dtype))[rows]
    assert int(bad.sum()) * 2 >= len(rows), f"{fault}: {int(bad.sum())} of {len(rows)} rows flagged"


def test_onehot_rows_are_exact_probes():
    for D in NR.D_SET:
        R = max(D, 64)
        x, cols, c = NR.onehot_rows(R, D, D)
        assert int((x != 0).sum()) == R and set(cols[:D].tolist()) == set(range(D))          # D rows hit every column
        g = torch.ones(D)
        got, _ = NR.rms_f32(x.numpy(), g.numpy(), EPS, torch.bfloat16)
        hit = torch.zeros((R, D), dtype=torch.bool)
        hit[torch.arange(R), torch.from_numpy(cols)] = True
        assert bool((got.float()[~hit] == 0).all())
        want = NR.onehot_want(c, torch.ones(R, dtype=torch.float64), D, EPS)
        err = (got.double()[hit] - want).abs()
        assert bool((err <= G.store_half_ulp(want, torch.bfloat16) + want.abs() * (NR.E_RSTD_RMS + 2 * U)).all())
        # the value a kernel returns that left the element out of its sum, c / sqrt(eps), is far outside the bound (but for the rare c
        # next to sqrt(D eps), where the two coincide)
        bnd = G.store_half_ulp(want, torch.bfloat16) + want.abs() * (NR.E_RSTD_RMS + 2 * U)
        assert float(((c / np.sqrt(float(np.float32(EPS))) - want).abs() > 4 * bnd).float().mean()) > 0.98


# ---- the folded norm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_n", [64, 128, 448, 512])
def test_consumer_emulation_and_its_faults(in_n):
    """Gaussian x of in_n * 16 columns: the emulated producer + consumer pair is inside fold_rstd_rel of the fp64 rstd of the same x in every
    row; each fault moves rstd by about 1 / (2 in_n) of itself and is flagged in every row (EPI_F32 has no store to hide behind)."""
    M, H = 16, in_n * 16
    g = torch.Generator().manual_seed(in_n)
    x = (torch.randn((M, H), generator=g) * 2).numpy()
    inv_dim = 1.0 / H
    r64 = NR.fold_rstd64(NR.block_sums(x, 16).sum(-1), inv_dim, EPS)
    e_r = NR.fold_rstd_rel(in_n // 16 + 4, 16)
    part = NR.partials_f32(x, 16)
    ok = NR.consumer_rstd_f32(part, inv_dim, EPS)
    assert bool(((torch.from_numpy(ok).double() - r64).abs() <= e_r * r64).all())
    for fault in NR.FOLD_FAULTS:
        got = NR.consumer_rstd_f32(part, inv_dim, EPS, fault=fault)
        bad = (torch.from_numpy(got).double() - r64).abs() > (e_r + U) * r64
        assert int(bad.sum()) * 2 >= M, f"{fault}: {int(bad.sum())} of {M} rows flagged"


@pytest.mark.parametrize("np_", [1, 15, 17, 128, 256])
def test_finalize_emulation_with_exact_partials(np_):
    part = NR.distinct_partials(20, np_, np_)
    r64 = NR.fold_rstd64(part.double().sum(-1), 1.0 / (32 * np_), EPS)
    got = NR.consumer_rstd_f32(part.numpy(), 1.0 / (32 * np_), EPS)
    assert bool(((torch.from_numpy(got).double() - r64).abs() <= NR.fold_rstd_rel(np_ // 16 + 16) * r64).all())


DECODE_PRODUCER = [(M, N, K) for M in (1, 7, 8, 9, 16) for N in (32, 96, 1024) for K in (64, 192)]
TILE_PRODUCER = [(M, N, K, 2) for M in (1, 65, 300) for N in (G.N_RAGGED, 512) for K in (64, 256)] + \
                [(300, G.N_RAGGED, 1024, 2), (300, 992, 4096, 1)]


def test_integer_probe_preconditions_hold():
    """16 max(x^2) < 2^24 (decode flavour), 32 max(x^2) < 2^24 (tile flavour), power-of-two weights: asserted inside fold_producer_ints for
    every shape the GPU tests use; and the float32 emulation of the producer then returns the block sums bit for bit."""
    for M, N, K in DECODE_PRODUCER:
        p = NR.fold_producer_ints(M, N, K, M + N + K, 16)
        assert 16 * float((p["x64"] ** 2).max()) < 2 ** 24
        assert np.array_equal(NR.partials_f32(p["x64"].numpy(), 16).astype(np.float64), p["part"].numpy())
        assert bool((G.rne_op(p["xw64"], torch.float16).double() - p["xw64"]).abs().max() <= G.store_half_ulp(p["xw64"], torch.float16).max())
    for M, N, K, amax in TILE_PRODUCER:
        p = NR.fold_producer_ints(M, N, K, M + N + K, 32, amax=amax, span=200, bias=True)
        assert 32 * float((p["x64"] ** 2).max()) < 2 ** 24
        assert np.array_equal(NR.partials_f32(p["x64"].numpy(), 32).astype(np.float64), p["part"].numpy())
    with pytest.raises(AssertionError):
        NR.fold_producer_ints(16, 1024, 2112, 1, 16, span=2000)          # the precondition is a real check
    for in_n in (64, 128, 448, 512):
        v = NR.distinct_partials(17, in_n, in_n)
        assert v.unique().numel() == v.numel() and float(v.double().sum(-1).max()) < 2 ** 24
