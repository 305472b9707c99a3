"""tests/gemm_ref.py without a GPU: the generators keep the conditions that make tests/test_gpu_gemm.py's references exact, the store
restatement agrees with torch's own casts, the activation error e(x) holds for float32 restatements of the kernels' three activations, and the
per-element bound of the random family holds for a plain float32 product of the same operands."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as G

SHAPES = sorted({(M, N, K) for _, M, N, K in G.all_cases()})


def test_shape_lists_cover_the_axes():
    """every explicit configuration at tile rows - 1 / tile rows / + 1 / a ragged second tile row, its shortest, a three-step and a long
    (>= 2048) K loop, a ragged N; the classic tiles at an N that is a multiple of 4 only; AUTO at every dispatch class of M and on the
    ragged-K fallback; the reduced list is a subset"""
    cases = G.cfg_cases()
    assert len(set(cases)) == len(cases) and set(G.all_cases(False)) <= set(G.all_cases())
    for cfg, tr in G.TILE_ROWS.items():
        mine = [c for c in cases if c[0] == cfg]
        kmin, kmult = G.k_rule(cfg)
        assert {tr - 1, tr, tr + 1} <= {c[1] for c in mine} and any(tr + 1 < c[1] < 2 * tr for c in mine)
        ks = {c[3] for c in mine}
        assert kmin in ks and 3 * kmult in ks and max(ks) >= 2048 and (max(ks) // kmult) % 2 == 1
        assert all(c[2] % 32 == 0 and c[2] % 128 for c in mine if c[2] != G.N_MULT4)
        assert (cfg in G.CLASSIC) == any(c[2] == G.N_MULT4 for c in mine)
    assert G.N_MULT4 % 4 == 0 and G.N_MULT4 % 8 and G.N_RAGGED % 32 == 0 and G.N_RAGGED % 128
    assert {c[1] for c in cases if c[0] == 1} >= {1, 8, 9, 16, 17, 32} and {c[1] for c in cases if c[0] == 9} >= {1, 8, 9, 16}
    auto = G.auto_cases()
    assert {c[1] for c in auto} >= set(G.AUTO_MS) and any(c[3] % 64 and c[3] % 8 == 0 for c in auto)
    # illegal pairs are filtered by the documented constraints
    assert not G.legal(6, 300, 288, 192) and not G.legal(15, 300, 288, 384) and not G.legal(13, 300, G.N_MULT4, 256)
    assert not G.legal(9, 17, 288, 64) and G.legal(5, 65, 288, 64, G.EPI_SWIGLU) and not G.legal(5, 65, 268, 64, G.EPI_SWIGLU) and not G.legal(8, 65, 288, 64, row_scale=True)


@pytest.mark.parametrize("M,N,K", SHAPES + [(300, 512, 11008)], ids=lambda v: str(v))
def test_integer_family_is_exact_in_fp32(M, N, K):
    """sum |a||w| < 2^24 on the data itself, both 16-bit types hold the operands unchanged, the fp32 product equals the fp64 one, and every
    epilogue value on the way to bias / residual / row scale is an fp32 number"""
    M = min(M, 96)                                      # rows are independent draws: a slice shows the same thing
    a, w = G.int_operands(M, N, K, 1)
    assert float((a.abs() @ w.abs().t()).max()) < 2 ** 24 and G.AMAX * G.AMAX * K < 2 ** 24
    for dt in G.DTYPES:
        assert G.representable(a, dt) and G.representable(w, dt)
    assert torch.equal((a @ w.t()).double(), a.double() @ w.double().t())
    bias, resid = G.frac_vector(N, 2), G.frac_vector(M * N, 3).reshape(M, N)
    y, exact = G.exact_epilogue(a, w, bias, resid)
    assert exact and torch.equal(y, a.double() @ w.double().t() + bias.double() + resid.double())
    assert G.exact_epilogue(a, w, G.frac_vector(N, 2, frac=False), None, G.pow2_scales(M, 4, big=10))[1]
    # the family does reach the ties of both stores (bf16: odd integers past 256, odd multiples of 2^-6 in [4, 8), ...; fp16: odd multiples
    # of 2^-6 in [32, 64), ...)
    if M >= 16 and K >= 64:
        v = (a @ w.t()).double() + bias.double()
        for dt in G.DTYPES:
            ties = (G.rne_op(v, dt).double() - v).abs() == G.store_half_ulp(v, dt)
            assert int(ties.sum()) >= 8, (dt, int(ties.sum()))
    assert not G.exact_epilogue(a, w, torch.full((N,), 1.0 / 3.0))[1]                # the check can fail


@pytest.mark.parametrize("dtype", G.DTYPES, ids=["bf16", "fp16"])
def test_one_hot_probes_cover_every_k_with_every_mantissa_bit(dtype):
    for K in sorted({K for _, _, K in SHAPES} | {11008}):
        p = G.coprime_step(K)
        assert np.gcd(p, K) == 1 and p % 2 == 1
        assert sorted(G.onehot_k(K, K).tolist()) == list(range(K))                          # K rows: every k once
        if K % 64 == 0:
            for m0 in (0, 37):
                assert sorted((G.onehot_k(m0 + 64, K)[m0:] % 64).tolist()) == list(range(64))   # any 64 rows: every position of a K step
    v = G.full_mantissa((4096,), dtype, 3)
    assert G.representable(v, dtype)
    p = G.MANT[dtype]
    frac, _ = np.frexp(v.double().numpy())
    j = np.abs(frac) * 2.0 ** p                                                             # the significand as an integer of p bits
    assert (j == np.round(j)).all() and (j.astype(np.int64) % 2 == 1).all() and (j >= 2 ** (p - 1)).all()
    assert len(set(j.astype(np.int64).tolist())) >= min(2 ** (p - 2), 64)
    for mirrored in (False, True):
        a, w, want = G.onehot_problem(70, 96, 192, dtype, 5, mirrored)
        assert G.representable(a, dtype) and G.representable(w, dtype)
        y = a.double() @ w.double().t()
        assert torch.equal(y, want.double()) and torch.equal((a @ w.t()), want)             # one exact fp32 product per element
        assert int(((a if not mirrored else w) != 0).sum()) == (70 if not mirrored else 96)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=["bf16", "fp16"])
def test_store_restatement_agrees_with_torch(dtype):
    """every 16-bit pattern, its midpoints to both neighbours (the ties) and values one fp32 ulp to either side of them, +-65504 and what
    lies beyond, infinities and NaN"""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype).float()
    v = v[torch.isfinite(v)]
    nxt = torch.sort(v).values
    mid = ((nxt[1:].double() + nxt[:-1].double()) / 2).float()                              # exact in fp32: 9 / 12 significand bits
    pts = torch.cat([v, mid, torch.nextafter(mid, torch.tensor(float("inf"))), torch.nextafter(mid, torch.tensor(float("-inf"))),
                     torch.tensor([65504.0, -65504.0, 65519.9, 65520.0, 65536.0, -65520.0, 1e9, -1e9, 3e38, float("inf"), float("-inf"),
                                   float("nan"), 0.0, -0.0, 1e-30, 2.0 ** -25, 3 * 2.0 ** -26])])
    got = G.rne_op(pts, dtype)
    want = (pts.clamp(-65504.0, 65504.0) if dtype == torch.float16 else pts).to(dtype)      # clamp keeps NaN
    assert got.dtype == dtype
    nan = torch.isnan(pts)
    assert torch.isnan(got.float()[nan]).all() and torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))
    if dtype == torch.float16:
        assert float(G.rne_op(torch.tensor([1e9]), dtype)) == 65504.0 and float(G.rne_op(torch.tensor([float("-inf")]), dtype)) == -65504.0
    # ties go to even: 257 -> 256, 259 -> 260 in bf16; 2049 -> 2048, 2051 -> 2052 in fp16
    t = torch.tensor([257.0, 259.0] if dtype == torch.bfloat16 else [2049.0, 2051.0])
    assert G.rne_op(t, dtype).float().tolist() == ([256.0, 260.0] if dtype == torch.bfloat16 else [2048.0, 2052.0])


def test_activation_restatements_stay_inside_e():
    """float32 restatements of vt_gelu_erf / vt_silu / vt_quick_gelu (same constants, same order) against fp64 at every multiple of 2^-6 in
    [-XMAX, XMAX] -- every pre-activation the GPU tests can produce -- and at random points between them"""
    x = np.arange(-int(G.XMAX) * 64, int(G.XMAX) * 64 + 1) / 64.0
    x = np.concatenate([x, np.random.default_rng(0).uniform(-G.XMAX, G.XMAX, 20000).astype(np.float32).astype(np.float64)])
    worst = {}
    for name, f32, f64, e in (("gelu", G.gelu_f32, G.gelu64, G.e_gelu), ("silu", G.silu_f32, G.silu64, G.e_silu), ("qgelu", G.qgelu_f32, G.qgelu64, G.e_qgelu)):
        with np.errstate(over="ignore"):
            err = np.abs(f32(x).astype(np.float64) - f64(x))
            ratio = err / e(x)
        worst[name] = float(ratio.max())
        assert ratio.max() <= 1.0, (name, float(x[ratio.argmax()]), worst[name])
        print(name, 'worst err / e(x)', worst[name])
        # the allowance is small against the 16-bit store that follows (2^-9 / 2^-12 relative) but for A&S's absolute 1.5e-7 * |x| / 2
        near = np.abs(x) <= 3.0
        assert (e(x)[near] <= 2.0 ** -13 * np.abs(f64(x))[near] + 2.5e-7).all()
    # the references themselves: torch's fp64 activations
    t = torch.from_numpy(x)
    assert np.allclose(G.gelu64(x), torch.nn.functional.gelu(t).numpy(), rtol=1e-12, atol=1e-13)       # torch's 1 + erf cancels in the tail
    assert np.allclose(G.silu64(x), torch.nn.functional.silu(t).numpy(), rtol=1e-12, atol=1e-300)
    assert np.allclose(G.qgelu64(x), (t * torch.sigmoid(1.702 * t)).numpy(), rtol=1e-12, atol=1e-300)
    g, up = np.meshgrid(np.arange(-40, 41) / 2.0, np.arange(-12, 13) * 1.0)
    err = np.abs((G.silu_f32(g) * up.astype(np.float32)).astype(np.float64) - G.silu64(g) * up)
    assert (err <= G.e_swiglu(g, up)).all()


def test_activation_operands_cover_the_range_exactly():
    for K in (64, 256, 2304, 8):
        a, w, bias = G.act_operands(161, 288, K, K)
        for dt in G.DTYPES:
            assert G.representable(a, dt) and G.representable(w, dt)
        x = (a @ w.t()).double() + bias.double()
        assert torch.equal(x, a.double() @ w.double().t() + bias.double()) and torch.equal(x.float().double(), x)
        assert float(x.abs().max()) <= G.XMAX and bool(((x * 64) == (x * 64).round()).all())
        if K >= 64:
            hist = torch.histc(x.float(), bins=40, min=-10, max=10)
            assert int(hist.min()) > 0 and float(x.min()) < -3.5 and int((x < -3.5).sum()) > 100   # dense over [-10, 10], the GELU tail included


@pytest.mark.parametrize("dtype", G.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", [(65, 288, 64), (33, 288, 2112), (16, 268, 200), (40, 160, 11008)])
def test_sum_bound_holds_for_a_float32_product(dtype, M, N, K):
    """a plain float32 matmul of the random family (another summation order than any kernel's), then the epilogue in fp32 and the store:
    inside the bound in every epilogue"""
    a, w, bias, resid = G.gauss_operands(M, N, K, dtype, K)
    assert G.representable(a, dtype) and G.representable(w, dtype) and G.bound_covers_epilogue(a, w, bias, resid)
    acc = a @ w.t()
    sb = G.sum_bound(a, w)
    ref = a.double() @ w.double().t() + bias.double()
    got32 = acc + bias
    assert bool(((got32.double() - ref).abs() <= sb).all())
    got16 = G.rne_op(got32, dtype).double()
    assert bool(((got16 - ref).abs() <= sb + G.store_half_ulp(ref, dtype)).all())
    refr = ref + resid.double()
    assert bool((((resid + got32).double() - refr).abs() <= sb).all())
    # The bound grows like K^2 (K terms, K roundings): far below the values on a short loop, about 1 % of a typical value at K = 2112; there
    # the exact families carry the long loops and this one only excludes gross errors
    if K <= 256:
        assert float((sb / ref.abs().clamp_min(1e-3)).median()) < 1e-3
        bad = got16.clone()                             # one element off by 2 % of its value leaves the bound
        i = int(ref.abs().flatten().argmax())
        bad.view(-1)[i] *= 1.02
        assert not bool(((bad - ref).abs() <= sb + G.store_half_ulp(ref, dtype)).all())
