"""load_4bit on the GPU: the NF4 kernels (vitron_amd/csrc/vt_nf4.hip) against the numpy restatement (tests/nf4_ref.py) and fp64, the 4-bit
decoder against a 16-bit decoder built from its dequantised weights, and the public surface (load_pretrained_model(..., load_4bit=True),
generate, ServingEngine, padded batches)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import nf4_ref as R
from tests.golden import cases
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-3            # what test_gemm_skinny_kernels / test_gemm_skinny_32_row_kernel allow the 16-bit weight-streaming kernels
DECODE_TOL = 1e-2     # decode-step logits of the 4-bit vs the dequantised 16-bit decoder: same weights, other kernels' summation order
LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


def _w(shape, seed, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * std


def _edge_matrix():
    """zero blocks, a block of one value, a block holding the codebook exactly, values one fp16 ulp around every midpoint, huge / tiny scales"""
    rows = [np.zeros(256, np.float32)]
    r = np.zeros(256, np.float32)
    r[64:128] = 0.5
    r[128:192] = R.CODEBOOK.repeat(4) * 3.0
    r[192] = 1.0
    for i, t in enumerate(R.MIDPOINTS):
        h = np.float16(t)
        while np.float32(h) > t:
            h = np.nextafter(h, np.float16(-2))
        r[193 + 2 * i], r[194 + 2 * i] = np.float32(h), np.float32(np.nextafter(h, np.float16(2)))
    rows.append(r)
    rows.append(np.linspace(-60000, 60000, 256).astype(np.float32))
    rows.append((np.arange(256, dtype=np.float32) - 128) * np.float32(2 ** -20))
    return torch.from_numpy(np.stack(rows))


@pytest.mark.parametrize("shape,seed", [((12288, 4096), 1), ((4096, 11008), 2), ((22016, 4096), 3), ("edge", 0)])
def test_nf4_quant_bytes_equal_the_restatement(dev, shape, seed):
    from vitron_amd import ops
    w = _edge_matrix() if shape == "edge" else _w(shape, seed)
    want_c, want_a = R.quantize(w.numpy())
    srcs = [(w, torch.bfloat16), (w, torch.float16), (w.half(), None), (w.bfloat16(), None)]
    for src, dt in srcs:
        codes, absmax = ops.nf4_quant(src.to(dev), dtype=dt)
        ref_c, ref_a = (want_c, want_a) if src.dtype == torch.float32 else R.quantize(src.float().numpy())
        assert np.array_equal(codes.cpu().numpy(), ref_c), (src.dtype, dt)
        assert np.array_equal(absmax.cpu().numpy().view(np.uint32), ref_a.view(np.uint32)), (src.dtype, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(4096, 4096), "edge"])
def test_nf4_dequant_bit_equal(dev, dt, shape):
    from vitron_amd import ops
    w = _edge_matrix() if shape == "edge" else _w(shape, 7)
    N, K = w.shape
    codes, absmax = ops.nf4_quant(w.to(dev), dtype=dt)
    got = ops.nf4_dequant(codes, absmax, K, dt)
    want = torch.from_numpy(R.dequantize_f32(codes.cpu().numpy(), absmax.cpu().numpy(), N, K)).to(dt)
    assert got.dtype == dt and torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.isfinite(got).all()


def _ref(a, wd, epi, resid=None, rscale=None, dt=None):
    """fp64 product, then the epilogue's store (the 16-bit epilogues round to `dt`, as _gemm_ref of test_gpu_kernels.py does)"""
    from vitron_amd import ops
    y = a.double() @ wd.double().t()
    if rscale is not None:
        y = y * rscale.double()[:, None]
    if epi == ops.EPI_SWIGLU_BF16:
        M, N = y.shape
        y4 = y.view(M, N // 32, 2, 16)
        y = torch.nn.functional.silu(y4[:, :, 0]) * y4[:, :, 1]
        y = y.reshape(M, N // 2)
    if epi == ops.EPI_F32_RESID:
        y = y + resid.double()
    if dt is not None and epi in (ops.EPI_BF16, ops.EPI_SWIGLU_BF16):
        return y.float().to(dt).float()
    return y.float()


GEMM_SHAPES = [(12288, 4096, "EPI_BF16"), (4096, 4096, "EPI_F32_RESID"), (22016, 4096, "EPI_SWIGLU_BF16"), (4096, 11008, "EPI_F32_RESID"),
               (4096, 4096, "EPI_F32"), (4096, 4096, "EPI_BF16")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [1, 4, 16, 17, 32])
@pytest.mark.parametrize("N,K,epi_name", GEMM_SHAPES)
def test_gemm_nf4_against_fp64(dev, dt, M, N, K, epi_name):
    from vitron_amd import ops
    epi = getattr(ops, epi_name)
    codes, absmax = ops.nf4_quant(_w((N, K), 100 + N % 97 + K % 89).to(dev), dtype=dt)
    wd = ops.nf4_dequant(codes, absmax, K, dt).float().cpu()
    a = _w((M, K), 200 + M, 1.0).to(dt)
    resid = _w((M, N), 300 + M, 1.0)
    out = resid.to(dev).clone() if epi == ops.EPI_F32_RESID else None
    got = ops.gemm_nf4(a.to(dev), codes, absmax, epi, out=out)
    ref = _ref(a.float(), wd, epi, resid, dt=dt)
    assert got.shape == ref.shape
    assert rel_l2(got.float(), ref) <= TOL, (M, N, K, epi_name)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [1, 16, 32])
def test_gemm_nf4_folded_norm_both_roles(dev, dt, M):
    """producer (o_proj / down_proj): x += A W^T, y = op16(x .* w_next), partial sums of x^2 per 16 columns; consumer (gate/up, qkv): rows
    scaled by rsqrt(mean(x^2) + eps) from those partials -- the decode step's 4-launch layer."""
    from vitron_amd import ops
    H, I = 4096, 11008
    eps = 1e-5
    c_o, s_o = ops.nf4_quant(_w((H, I), 11).to(dev), dtype=dt)
    c_gu, s_gu = ops.nf4_quant(_w((2 * I, H), 12).to(dev), dtype=dt)
    h = _w((M, I), 13, 1.0).to(dt)
    x0 = _w((M, H), 14, 1.0)
    wn = 1.0 + _w((H,), 15, 0.1)
    x = x0.to(dev).clone()
    xw = torch.empty((M, H), device=dev, dtype=dt)
    part = torch.empty((M, H // 16), device=dev)
    ops.gemm_nf4(h.to(dev), c_o, s_o, ops.EPI_F32_RESID, out=x, norm_out=(wn.to(dev), xw, part))
    x_ref = _ref(h.float(), ops.nf4_dequant(c_o, s_o, I, dt).float().cpu(), ops.EPI_F32_RESID, x0)
    assert rel_l2(x, x_ref) <= TOL
    xg = x.cpu().double()
    assert rel_l2(xw.float(), (xg * wn.double()).float().to(dt).float()) <= TOL
    assert rel_l2(part.cpu(), (xg * xg).view(M, H // 16, 16).sum(-1)) <= 1e-6
    g = ops.gemm_nf4(xw, c_gu, s_gu, ops.EPI_SWIGLU_BF16, norm_in=(part, 1.0 / H, eps))
    rstd = 1.0 / torch.sqrt((xg * xg).mean(-1) + eps)
    ref = _ref(xw.float().cpu(), ops.nf4_dequant(c_gu, s_gu, H, dt).float().cpu(), ops.EPI_SWIGLU_BF16, rscale=rstd, dt=dt)
    assert rel_l2(g.float(), ref) <= TOL


# ---- the GEMM against the CPU dequantisation of random NF4 matrices (nf4_ref.random_nf4: no GPU quantiser in the reference) ------------
FMT = {torch.bfloat16: "bf16", torch.float16: "fp16"}
PROBE_EPIS = ("EPI_F32", "EPI_BF16", "EPI_F32_RESID")
BOUND_M = (1, 2, 3, 8, 15, 16, 17, 24, 31, 32)
BOUND_K = (128, 256, 384, 1024 + 128, 4096, 11008)     # 128: one K step, seven of the eight waves idle; 384, 1152: uneven splits
SWIGLU_RANGE = (-12, 0)   # gate / up scales small enough that silu(g) * u stays inside fp16 at K = 11008


@functools.lru_cache(maxsize=6)
def _rnd(N, K, seed, log2_range=(-12, 4)):
    """(codes, absmax, fp32 CPU dequantisation [N][K]) of nf4_ref.random_nf4"""
    codes, absmax = R.random_nf4(N, K, seed, log2_range)
    return codes, absmax, R.dequantize_f32(codes, absmax, N, K)


def _rnd_dev(N, K, seed, dt, dev, log2_range=(-12, 4)):
    """(codes, absmax on the GPU, the weight's exact operand values op16(CPU dequantisation) as fp64 numpy [N][K])"""
    codes, absmax, deq = _rnd(N, K, seed, log2_range)
    wd = torch.from_numpy(deq).to(dt).double().numpy()
    return torch.from_numpy(codes).to(dev), torch.from_numpy(absmax).to(dev), wd


def _within(got, ref, bound, what):
    """|got - ref| <= bound element by element (NaN fails); the largest error / bound ratio goes to VT_TOL_REPORT when that is set"""
    g = got.detach().double().cpu().numpy()
    err = np.abs(g - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {i}: got {g[i]!r} ref {ref[i]!r} "
                             f"bound {bound[i]!r}")
    out = os.environ.get("VT_TOL_REPORT")
    if out:
        with open(out, "a") as fh:
            fh.write(f"bound {what}\t{float((err / np.maximum(bound, 1e-300)).max()):.6e}\n")


def _probe_ks(K):
    """k = 0, 1, 63, 64, 127, 128 (nibble order, 64-blocks, the first K steps), each wave's first and last k, and K - 1"""
    steps = K // 128
    ks = {0, 1, 63, 64, 127, 128, K - 1}
    for w in range(8):                          # gemm_nf4_kernel: wave w walks steps [steps * w / 8, steps * (w + 1) / 8)
        s0, s1 = steps * w // 8, steps * (w + 1) // 8
        if s0 < s1:
            ks |= {128 * s0, 128 * s1 - 1}
    return sorted(k for k in ks if k < K)


def _probe(a_rows, codes, absmax, epi, N):
    """C = epi(a W^T) for unit rows a, as fp32 [M][N] (EPI_F32_RESID onto a zero residual)"""
    from vitron_amd import ops
    if epi == ops.EPI_F32_RESID:
        out = torch.zeros((a_rows.shape[0], N), device=a_rows.device)
        return ops.gemm_nf4(a_rows, codes, absmax, epi, out=out)
    return ops.gemm_nf4(a_rows, codes, absmax, epi).float()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [4096, 11008])
def test_gemm_nf4_unit_probes_reconstruct_every_weight_exactly(dev, dt, K):
    """row m of A = e_k: C[m][n] = deq(W)[n][k] is one exact product, so every epilogue must return the CPU dequantisation itself. 32 probe
    rows per launch, ceil(K / 32) launches: every weight element passes through the kernel's load, LDS table, nibble split and scale."""
    from vitron_amd import ops
    N = 64
    codes, absmax, wd = _rnd_dev(N, K, 400 + K % 97, dt, dev)
    want = torch.from_numpy(wd.T.copy()).float()
    eye = torch.eye(K, dtype=dt, device=dev)
    for epi_name in PROBE_EPIS:
        epi = getattr(ops, epi_name)
        got = torch.empty((K, N), device=dev)
        for k0 in range(0, K, 32):
            k1 = min(K, k0 + 32)
            got[k0:k1] = _probe(eye[k0:k1], codes, absmax, epi, N)
        bad = got.cpu() != want                 # as values: +0 == -0
        assert not bad.any(), (epi_name, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("K", BOUND_K)
def test_gemm_nf4_unit_probes_at_edge_shapes(dev, dt, N, K):
    """the exact probes at the k that split K among the waves and steps, in every row-count instantiation and tail (M = 1 .. 32)"""
    from vitron_amd import ops
    codes, absmax, wd = _rnd_dev(N, K, 500 + K % 89 + N, dt, dev)
    want = torch.from_numpy(wd).float()
    ks = _probe_ks(K)
    eye = torch.eye(K, dtype=dt, device=dev)
    for M in (1, 15, 16, 17, 31, 32):
        for i0 in range(0, len(ks), M):
            sel = [ks[(i0 + j) % len(ks)] for j in range(M)]
            a = eye[sel].contiguous()
            for epi_name in PROBE_EPIS:
                got = _probe(a, codes, absmax, getattr(ops, epi_name), N).cpu()
                bad = got != want[:, sel].t()
                assert not bad.any(), (epi_name, M, sel, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("epi_name", ["EPI_F32", "EPI_BF16", "EPI_F32_RESID", "EPI_SWIGLU_BF16"])
@pytest.mark.parametrize("K", BOUND_K)
def test_gemm_nf4_within_per_element_bound_of_fp64(dev, dt, epi_name, K):
    """random NF4 weights against fp64 on their CPU dequantisation, element by element under nf4_ref.gemm_bound, at every row count
    1 .. 32 (both instantiations, their tails), K from one step to 86 (uneven splits), N from one block to 4096 + 32 and 2 I for SwiGLU"""
    from vitron_amd import ops
    epi = getattr(ops, epi_name)
    swiglu, resid = epi == ops.EPI_SWIGLU_BF16, epi == ops.EPI_F32_RESID
    store = FMT[dt] if epi in (ops.EPI_BF16, ops.EPI_SWIGLU_BF16) else None
    Ns = (32, 96, 4096 + 32) + ((2 * 11008,) if swiglu and K <= 4096 else ())
    a = _w((32, K), 600 + K % 83, 1.0).to(dt)
    a64 = a.double().numpy()
    a_dev = a.to(dev)
    for N in Ns:
        codes, absmax, wd = _rnd_dev(N, K, 700 + K % 79 + N % 71, dt, dev, SWIGLU_RANGE if swiglu else (-12, 4))
        r = _w((32, N), 800 + N % 67, 4.0) if resid else None
        r64 = r.double().numpy() if resid else None
        y = a64 @ wd.T
        ref = R.gemm_ref(a64, wd, resid=r64, swiglu=swiglu, y=y)
        bnd = R.gemm_bound(a64, wd, K, resid=r64, swiglu=swiglu, store=store, y=y)
        for M in BOUND_M:
            out = r[:M].to(dev).clone() if resid else None
            got = ops.gemm_nf4(a_dev[:M], codes, absmax, epi, out=out)
            _within(got, ref[:M], bnd[:M], f"{epi_name} {FMT[dt]} M={M} N={N} K={K}")
            ref_t = torch.from_numpy(ref[:M]).float()
            assert rel_l2(got.float(), ref_t.to(dt).float() if store else ref_t) <= TOL, (M, N)


@pytest.mark.parametrize("dt", DTYPES)
def test_gemm_nf4_folded_norm_every_role_within_bound(dev, dt):
    """the decode step's folded RMSNorm at 7B width, every row count of both instantiations: producer (down_proj: x += h Wdown^T,
    xw = op16(x .* w_next), partial sums of x^2) and both consumers of its output (qkv: EPI_BF16 at N = 3 H; gate/up: SwiGLU), each element
    against fp64 scaled by the fp64 rstd of the produced x"""
    from vitron_amd import ops
    H, I, eps = 4096, 11008, 1e-5
    fmt = FMT[dt]
    c_o, s_o, w_o = _rnd_dev(H, I, 21, dt, dev)
    consumers = [("qkv", ops.EPI_BF16, _rnd_dev(3 * H, H, 22, dt, dev)), ("gate_up", ops.EPI_SWIGLU_BF16, _rnd_dev(2 * I, H, 23, dt, dev, SWIGLU_RANGE))]
    h = _w((32, I), 24, 1.0).to(dt)
    x0 = _w((32, H), 25, 4.0)
    wn = 1.0 + _w((H,), 26, 0.1)
    h64, x064, wn64 = h.double().numpy(), x0.double().numpy(), wn.double().numpy()
    y_o = h64 @ w_o.T
    # the kernel's rstd comes from fp32 sums: 16 squares per partial, H / 256 partials per thread, 16 threads; then * 1/H, + eps, rsqrt
    rstd_rel = (H // 256 + 16 + 4 + 8) * R.U32
    for M in (1, 2, 16, 17, 31, 32):
        x = x0[:M].to(dev).clone()
        xw = torch.empty((M, H), device=dev, dtype=dt)
        part = torch.empty((M, H // 16), device=dev)
        ops.gemm_nf4(h[:M].to(dev), c_o, s_o, ops.EPI_F32_RESID, out=x, norm_out=(wn.to(dev), xw, part))
        _within(x, R.gemm_ref(h64[:M], w_o, resid=x064[:M], y=y_o[:M]), R.gemm_bound(h64[:M], w_o, I, resid=x064[:M], y=y_o[:M]), f"producer x M={M}")
        xg = x.cpu().double()
        p = xg.numpy() * wn64                                # xw = op16(fp32(x * w)): two roundings
        _within(xw, p, R.U32 * np.abs(p) + R.half_ulp(np.abs(p) * (1 + R.U32), fmt), f"producer xw M={M}")
        assert rel_l2(part.cpu(), (xg * xg).view(M, H // 16, 16).sum(-1)) <= 1e-6
        rstd = (1.0 / torch.sqrt((xg * xg).mean(-1) + eps)).numpy()
        a64 = xw.cpu().double().numpy()
        for name, epi, (c, s, wd) in consumers:
            swiglu = epi == ops.EPI_SWIGLU_BF16
            got = ops.gemm_nf4(xw, c, s, epi, norm_in=(part, 1.0 / H, eps))
            y = a64 @ wd.T
            ref = R.gemm_ref(a64, wd, rscale=rstd, swiglu=swiglu, y=y)
            _within(got, ref, R.gemm_bound(a64, wd, H, rscale=rstd, rscale_rel=rstd_rel, swiglu=swiglu, store=fmt, y=y), f"{name} {fmt} M={M}")
            assert rel_l2(got.float(), torch.from_numpy(ref).float().to(dt).float()) <= TOL, (name, M)


# ---- the 4-bit decoder against the 16-bit decoder of its dequantised weights ------------------------------------------------------------
def _llama_sd(cfg, seed):
    from vitron_amd import synth
    return synth.llama_state(cfg, synth.make_generator(seed), w_std=0.02)


def _dequantised(sd, dt, dev):
    """the state dict with every decoder Linear replaced by op16(dequant(nf4(W))) (per matrix: NF4 blocks never leave a row, so this equals
    the quantisation of the packed q|k|v and interleaved gate/up matrices)"""
    from vitron_amd import ops
    out = dict(sd)
    for k, v in sd.items():
        if k.startswith("model.layers.") and any(k.endswith(n + ".weight") for n in LINEARS):
            c, a = ops.nf4_quant(v.float().to(dev), dtype=dt)
            out[k] = ops.nf4_dequant(c, a, v.shape[1], dt)
    return out


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp16"])
def pair7b(dev, request):
    """a 2-layer decoder at 7B width, 4-bit, and the 16-bit one of its dequantised weights"""
    from vitron_amd.engine import PackedLlama
    dt = request.param
    cfg = dict(hidden_size=4096, intermediate_size=11008, num_attention_heads=32, num_hidden_layers=2, vocab_size=1024, rms_norm_eps=1e-5,
               rope_theta=10000.0, max_position_embeddings=4096)
    sd = _llama_sd(cfg, 5)
    q = PackedLlama(sd, cfg, dev, dtype=dt, weight_format="nf4")
    p16 = PackedLlama(_dequantised(sd, dt, dev), cfg, dev, dtype=dt)
    return dt, cfg, q, p16


def test_nf4_decoder_holds_no_16bit_matrix_and_is_small(pair7b):
    dt, cfg, q, p16 = pair7b
    for t in q.layer_tensors:
        assert not any(k in t for k in ("wqkv", "wo", "wgu", "wdown"))
        assert all(v.dtype in (torch.uint8, torch.float32) for v in t.values())
    assert q.decoder_weight_bytes() <= 0.30 * p16.decoder_weight_bytes()
    for level in (1, 2, 3):
        with pytest.raises(Exception):
            q.set_precise(level)
    with pytest.raises(Exception):
        q.set_precise_qk(True)


def _run(pl, emb_rows, n_steps, pages=16):
    """prefill `emb_rows` then n_steps greedy decode steps: (prefill logits [rows][V], [step logits [V]])"""
    from vitron_amd.engine import PagedKVCache, SequenceState, llama_forward
    kv = PagedKVCache(pl, pages)
    seq = SequenceState()
    n = emb_rows.shape[0]
    pre = llama_forward(pl, kv, [seq], emb_rows, [n], logit_rows=list(range(n))).float()
    steps, ids = [pre[-1].clone()], []
    for _ in range(n_steps):
        t = int(steps[-1].argmax())
        ids.append(t)
        lg = llama_forward(pl, kv, [seq], pl.embed[t:t + 1].contiguous(), [1]).float()[0]
        steps.append(lg)
    kv.release(seq.pages)
    return pre, steps, ids


def test_nf4_prefill_bitwise_equals_dequantised_16bit_and_decode_agrees(dev, pair7b):
    dt, cfg, q, p16 = pair7b
    g = torch.Generator().manual_seed(9)
    emb = (torch.randn((200, cfg["hidden_size"]), generator=g) * 0.5).to(dt).to(dev)
    pre4, st4, ids4 = _run(q, emb, 16)
    pre16, st16, ids16 = _run(p16, emb, 16)
    assert torch.equal(pre4, pre16)        # > 32 rows: dequantised weights on the same tile GEMMs
    for t in range(16):
        assert rel_l2(st4[t], st16[t]) <= DECODE_TOL, t
        if ids4[t] != ids16[t]:             # a flip only where the 16-bit run's top-2 margin is inside the noise of the bound
            top2 = st16[t].topk(2).values
            assert float(top2[0] - top2[1]) <= 2 * DECODE_TOL * float(st16[t].pow(2).mean().sqrt()), t
            break
    # a short follow-up prefill (<= 32 rows, norms as launches) on both
    g2 = torch.Generator().manual_seed(10)
    emb2 = (torch.randn((20, cfg["hidden_size"]), generator=g2) * 0.5).to(dt).to(dev)
    a, _, _ = _run(q, emb2, 0)
    b, _, _ = _run(p16, emb2, 0)
    assert rel_l2(a, b) <= DECODE_TOL


def _emb(rows, H, dt, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, H), generator=g) * 0.5).to(dt).to(dev)


def _pasts_on_both(q, p16, pasts, pages, seed):
    """both decoders prefill the same pasts in one batch (> 32 rows: dequantised weights on the tile GEMMs, so bit-equal caches)"""
    from vitron_amd.engine import PagedKVCache, SequenceState, llama_forward
    emb = _emb(sum(pasts), q.H, q.dtype, q.device, seed)
    out = []
    for pl in (q, p16):
        kv = PagedKVCache(pl, pages)
        seqs = [SequenceState() for _ in pasts]
        lg = llama_forward(pl, kv, seqs, emb, list(pasts)).float()
        out.append((kv, seqs, lg))
    assert torch.equal(out[0][2], out[1][2])
    return out


def _decode_steps(q, p16, state, n_steps):
    """n_steps decode steps of every sequence on both decoders, both fed the 16-bit decoder's greedy tokens: [(logits4, logits16)] on the CPU"""
    from vitron_amd.engine import llama_forward
    (kv4, s4, _), (kv16, s16, last) = state
    steps = []
    for _ in range(n_steps):
        e = p16.embed[last.argmax(-1)].contiguous()
        a = llama_forward(q, kv4, s4, e, [1] * len(s4)).float()
        b = llama_forward(p16, kv16, s16, e, [1] * len(s16)).float()
        steps.append((a.cpu(), b.cpu()))
        last = b
    return steps


def _agree(a, b, what):
    """one sequence's logits: DECODE_TOL, and an arg-max flip only where the 16-bit top-2 margin is inside the noise of that bound"""
    assert rel_l2(a, b) <= DECODE_TOL, what
    if int(a.argmax()) != int(b.argmax()):
        top2 = b.topk(2).values
        assert float(top2[0] - top2[1]) <= 2 * DECODE_TOL * float(b.pow(2).mean().sqrt()), what


def _pasts(B):
    """1, 63, 64, 65 tokens (page edges) and 128 .. 134 (a page edge inside the second page), cycling"""
    return [(1, 63, 64, 65)[i % 5] if i % 5 < 4 else 128 + i // 5 for i in range(B)]


@pytest.mark.parametrize("B", [20, 32])
def test_nf4_decode_17_to_32_sequences_agree(dev, pair7b, B):
    """17 .. 32 sequences decoding at once: the NF4 branch without the norm fold (norms as launches, gemm_nf4, fused decode attention)"""
    dt, cfg, q, p16 = pair7b
    state = _pasts_on_both(q, p16, _pasts(B), 3 * B + 4, 40 + B)
    for t, (a, b) in enumerate(_decode_steps(q, p16, state, 4)):
        for i in range(B):
            _agree(a[i], b[i], (B, t, i))


def test_nf4_decode_40_sequences_bitwise_equals_dequantised_16bit(dev, pair7b):
    """> 32 decode rows: every Linear dequantised into the workspace in front of the same tile GEMMs the 16-bit decoder runs"""
    dt, cfg, q, p16 = pair7b
    state = _pasts_on_both(q, p16, _pasts(40), 124, 80)
    for t, (a, b) in enumerate(_decode_steps(q, p16, state, 4)):
        assert torch.equal(a, b), t


@pytest.mark.parametrize("n", [40, 64])
def test_nf4_prefill_33_to_64_rows_bitwise_equals_dequantised_16bit(dev, pair7b, n):
    dt, cfg, q, p16 = pair7b
    emb = _emb(n, cfg["hidden_size"], dt, dev, 90 + n)
    a, _, _ = _run(q, emb, 0)
    b, _, _ = _run(p16, emb, 0)
    assert torch.equal(a, b)


def test_nf4_chunk_after_a_past_next_to_decodes_agrees(dev, pair7b):
    """one launch of <= 32 rows mixing a 12-row chunk that goes on from a 200-token past with 3 single-token decodes: the NF4 branch's
    kv_tiles + flash_attn; then one decode step of all four (the folded 4-launch layer) on the cache that launch wrote"""
    from vitron_amd.engine import llama_forward
    dt, cfg, q, p16 = pair7b
    state = _pasts_on_both(q, p16, [200, 1, 64, 129], 16, 100)
    emb = _emb(15, cfg["hidden_size"], dt, dev, 101)
    (kv4, s4, _), (kv16, s16, _) = state
    a = llama_forward(q, kv4, s4, emb, [12, 1, 1, 1], logit_rows=list(range(15))).float().cpu()
    b = llama_forward(p16, kv16, s16, emb, [12, 1, 1, 1], logit_rows=list(range(15))).float().cpu()
    for r in range(15):
        _agree(a[r], b[r], ("chunk", r))
    last = b[[11, 12, 13, 14]].to(dev)
    for t, (a, b) in enumerate(_decode_steps(q, p16, ((kv4, s4, None), (kv16, s16, last)), 1)):
        for i in range(4):
            _agree(a[i], b[i], ("after", t, i))


# ---- public surface ---------------------------------------------------------------------------------------------------------------
def _spec(seed=31):
    return dict(llm=dict(cases.LLM, eos_token_id=2, bos_token_id=1, pad_token_id=0), image=cases.VIT_IMAGE, video=cases.VIT_VIDEO, seed=seed,
                w_std=0.05)


def test_load_4bit_synthetic_generates_and_refuses_precise_and_8bit(dev):
    from vitron_amd.model.builder import load_pretrained_model
    _, model, _, _ = load_pretrained_model("synthetic", None, "vitron-llava-7b", load_4bit=True, device="cuda", synthetic=_spec())
    assert model.weight_format == "nf4" and model.model.llama.weight_format == "nf4"
    ids = torch.tensor([[1, 5, 6, 7, 8, 9]], device=dev)
    out = model.generate(ids, do_sample=False, max_new_tokens=6, eos_token_id=-1)
    assert out.shape == (1, 12) and int(out.min()) >= 0
    for level in (1, 2, 3):
        with pytest.raises(Exception):
            model.set_precise(level)
    with pytest.raises(NotImplementedError):
        load_pretrained_model("synthetic", None, "x", load_8bit=True, synthetic=_spec())


def test_load_4bit_checkpoint_equals_synthetic_construction(dev, tmp_path):
    import json
    import os

    from safetensors.torch import save_file

    from vitron_amd import synth
    from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    from vitron_amd.model.builder import load_pretrained_model
    cfg = dict(cases.LLM)
    sd = {k: v.half().contiguous() for k, v in synth.llama_state(cfg, synth.make_generator(44), w_std=0.05).items()}
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file(sd, os.path.join(ck, "model.safetensors"))
    json.dump(dict(cfg, mm_hidden_size=cases.MM_HIDDEN), open(os.path.join(ck, "config.json"), "w"))
    _, m1, _, _ = load_pretrained_model(str(ck), None, "vitron-llava-7b", load_4bit=True, device="cuda", tokenizer=object())
    m2 = LlavaLlamaForCausalLM(LlavaConfig(**cfg, mm_hidden_size=cases.MM_HIDDEN))
    m2.weight_format = "nf4"
    m2.load_state_dict(sd, strict=False)
    m2.to(dev, dtype=torch.float16)
    for t1, t2 in zip(m1.model.llama.layer_tensors, m2.model.llama.layer_tensors):
        assert t1.keys() == t2.keys()
        for k in t1:
            assert torch.equal(t1[k], t2[k]), k
    ids = torch.tensor([[1, 11, 12, 13, 14]], device=dev)
    o1 = m1.generate(ids, do_sample=False, max_new_tokens=5, eos_token_id=-1)
    o2 = m2.generate(ids, do_sample=False, max_new_tokens=5, eos_token_id=-1)
    assert torch.equal(o1, o2)


def test_serving_engine_on_4bit_matches_solo_runs(dev):
    from vitron_amd.model.builder import load_pretrained_model
    from vitron_amd.serving import ServingEngine
    _, model, _, _ = load_pretrained_model("synthetic", None, "vitron-llava-7b", load_4bit=True, device="cuda", synthetic=_spec(32))
    g = torch.Generator().manual_seed(21)
    V = cases.LLM["vocab_size"]
    img = torch.randn((3, 56, 56), generator=g).bfloat16().to(dev)
    rnd = lambda n: torch.randint(3, V, (n,), generator=g).tolist()                     # noqa: E731
    reqs = [dict(input_ids=torch.tensor([[1] + rnd(23)]), images=None, max_new_tokens=9),
            dict(input_ids=torch.tensor([[1, -200] + rnd(11)]), images=[img], max_new_tokens=12),
            dict(input_ids=torch.tensor([[1] + rnd(70)]), images=None, max_new_tokens=5)]
    model.config.kv_prefix_reuse = False
    solo = []
    for r in reqs:
        o = model.generate(r["input_ids"].to(dev), images=r["images"], do_sample=False, max_new_tokens=r["max_new_tokens"], eos_token_id=-1)
        solo.append(o[0, r["input_ids"].shape[1]:].cpu().tolist())
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    seen = {}
    rid0 = eng.submit(reqs[0]["input_ids"], reqs[0]["images"], None, reqs[0]["max_new_tokens"], eos_token_id=-1)
    seen[rid0] = []
    steps = 0
    while eng.pending():
        if steps == 2:
            for r in reqs[1:]:
                seen[eng.submit(r["input_ids"], r["images"], None, r["max_new_tokens"], eos_token_id=-1)] = []
        for rid, t in eng.step():
            seen[rid].append(t)
        steps += 1
        assert steps < 200
    assert [seen[i] for i in sorted(seen)] == solo


def test_padded_batch_on_4bit_runs_fixup_through_gemm_nf4(dev, monkeypatch):
    from vitron_amd import ops
    from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    from vitron_amd import synth
    case = cases.glue_cases()["batch_pad"]
    st = {"image_tower": synth.vit_state(cases.VIT_IMAGE, synth.make_generator(cases.SEED_VIT), w_std=0.05),
          "video_tower": synth.vit_state(cases.VIT_VIDEO, synth.make_generator(cases.SEED_VIT), w_std=0.05),
          "projector": synth.projector_state(cases.MM_HIDDEN, cases.LLM["hidden_size"], synth.make_generator(cases.SEED_PROJ), w_std=0.05),
          "region": synth.region_state(cases.MM_HIDDEN, cases.LLM["hidden_size"], synth.make_generator(cases.SEED_REGION), w_std=0.05),
          "llama": synth.llama_state(cases.LLM, synth.make_generator(cases.SEED_LLM), w_std=0.05)}

    def build(fmt, llama_sd):
        m = LlavaLlamaForCausalLM(LlavaConfig(**cases.LLM, mm_hidden_size=cases.MM_HIDDEN, mm_image_tower="golden/LanguageBind_Image",
                                              mm_video_tower="golden/LanguageBind_Video_merge"))
        m.weight_format = fmt
        m.get_image_tower().load_state(cases.VIT_IMAGE, st["image_tower"])
        m.get_video_tower().load_state(cases.VIT_VIDEO, st["video_tower"])
        sd = dict(llama_sd)
        sd.update({"model.mm_projector." + k: v for k, v in st["projector"].items()})
        sd.update({"model.region_extractor." + k: v for k, v in st["region"].items()})
        m.load_state_dict(sd)
        return m.to(dev, dtype=torch.float16)

    m4 = build("nf4", st["llama"])
    m16 = build("16bit", {k: v.cpu() for k, v in _dequantised(st["llama"], torch.float16, dev).items()})
    calls = []
    real = ops.gemm_nf4
    monkeypatch.setattr(ops, "gemm_nf4", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    ids, am = case["input_ids"].to(dev), case["attention_mask"].to(dev)
    images = [im.to(dev).half() for im in case["images"]]
    n_new = 8
    o4, l4 = m4.generate(ids, images=images, regions=case["regions"], attention_mask=am, do_sample=False, max_new_tokens=n_new, eos_token_id=-1,
                         return_logits=True, padded_batch=True)
    assert calls and max(calls) <= 32          # the fix-up rows went through the 4-bit GEMM
    monkeypatch.setattr(ops, "gemm_nf4", real)
    o16, l16 = m16.generate(ids, images=images, regions=case["regions"], attention_mask=am, do_sample=False, max_new_tokens=n_new, eos_token_id=-1,
                            return_logits=True, padded_batch=True)
    new4, new16 = o4[:, ids.shape[1]:].cpu(), o16[:, ids.shape[1]:].cpu()
    for b in range(ids.shape[0]):
        for t in range(n_new):
            if int(new4[b, t]) != int(new16[b, t]):
                row = l16[t][b].float()
                top2 = row.topk(2).values
                assert float(top2[0] - top2[1]) <= 2 * DECODE_TOL * float(row.pow(2).mean().sqrt()), (b, t)
                break
            assert rel_l2(l4[t][b].float(), l16[t][b].float()) <= DECODE_TOL, (b, t)
