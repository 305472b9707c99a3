"""Decode attention on the GPU (vitron_amd/csrc/vt_attn.hip: attn_decode_fused_kernel through ops.attn_decode_fused, the split-K
attn_decode_kernel + attn_decode_combine_kernel through ops.attn_decode) against the host restatement in tests/attn_ref.py, in both
operand builds at head_dim 64 and 128: exact one-hot and uniform probes over every page position and wave / split layout, a per-element
fp64 bound on random data at long ragged contexts with rope, the score-range edges, and the fused kernel's page invariants. Caches are
packed on the host (pack_pages) unless a test is about vt_kv_tiles writing them."""
import math

import numpy as np
import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
KERNELS = ["fused", "split"]
PROBE_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 1024, 1089]
NB = 14                 # bits of the one-hot probes' key codes: positions < 2^14
A_CODE = 32.0           # key code entries +-A, query +-B: the target scores NB * A * B, every other key at least 2 A B lower,
B_CODE = 32.0           # 2 A B * scale * log2(e) >= 261 (hd 128) -- every other weight is below 2^-150 and v_exp_f32 returns 0
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- cache layouts -----------------------------------------------------------------------------------------------------------------
class Batch:
    """Sequences over a shuffled pool of pages with spare pages; every page no table names holds NaN. groups = [(kv_len, n)]: n sequences
    of one context length. Under the split kernel they share their pages (read only); under the fused kernel the pages before the new
    token's are shared and every sequence gets its own copy of the page the step writes (a fresh one stays NaN: the kernel must zero
    it). keys(j) / vals(j) -> [len(j)][heads][hd]: the cache contents at positions j (before the step, for the fused kernel)."""

    def __init__(self, groups, heads, hd, dtype, fused, keys, vals, seed, spare=5):
        rng = np.random.default_rng(seed)
        need = sum((L - 1 if fused else L) // 64 + 1 + (n if fused else 0) for L, n in groups)
        self.npages = need + spare
        it = iter(rng.permutation(self.npages).tolist())
        size = self.npages * heads * 64 * hd
        self.kp, self.vp = torch.full((size,), NAN, dtype=dtype), torch.full((size,), NAN, dtype=torch.float16)
        self.table, self.seqs = [], []           # seqs: (kv_len, table_off)
        src, dst = [], []
        for L, n in groups:
            nk = L - 1 if fused else L
            pages = [next(it) for _ in range((nk + 63) // 64)]
            if nk:
                j = np.arange(nk)
                R.pack_pages(keys(j), vals(j), pages, heads, hd, dtype, out=(self.kp, self.vp))
            if not fused:
                off = len(self.table)
                self.table += pages
                self.seqs += [(L, off)] * n
                continue
            t_last, r_new = (L - 1) // 64, (L - 1) % 64
            for _ in range(n):
                priv = next(it)
                if r_new:
                    src.append(pages[t_last])
                    dst.append(priv)
                self.seqs.append((L, len(self.table)))
                self.table += pages[:t_last] + [priv]
        if src:
            for p in (self.kp, self.vp):
                v = p.view(self.npages, -1)
                v[dst] = v[src]
        self.heads, self.hd, self.dtype, self.fused = heads, hd, dtype, fused
        self.rows = rng.permutation(len(self.seqs))            # q_row0 of sequence i

    def used(self):
        u = torch.zeros(self.npages, dtype=torch.bool)
        u[self.table] = True
        return u


def _qkv(b: Batch, q, knew=None, vnew=None):
    """the decode step's fused-QKV buffer: row b.rows[i] holds sequence i; a row stride beyond 3 D and permuted column blocks (k, v, q)"""
    D = b.heads * b.hd
    ld = 3 * D + 192
    cols = dict(k=0, v=D + 64, q=2 * D + 128)
    x = torch.zeros((len(b.seqs), ld), dtype=b.dtype)
    x[:, D:D + 64] = NAN                                     # the gaps between the blocks are never read
    for name, t in (("q", q), ("k", knew), ("v", vnew)):
        if t is not None:
            x[b.rows, cols[name]:cols[name] + D] = torch.as_tensor(t).reshape(len(b.seqs), D).to(b.dtype)
    return x, cols


def _launch(dev, kernel, b: Batch, q, knew=None, vnew=None, max_kv=None, rope=None, positions=None, pages=None):
    """one decode step over `b` -> (out [nseq][heads][hd] on the host in sequence order, k_pages, vt_pages, qkv) on the device"""
    from vitron_amd import ops
    x, cols = _qkv(b, q, knew, vnew)
    x = x.to(dev)
    kp, vp = pages if pages is not None else (b.kp.to(dev), b.vp.to(dev))
    table = torch.tensor(b.table, dtype=torch.int32, device=dev)
    desc = ops.seq_desc_tensor([(int(b.rows[i]), 1, L, off) for i, (L, off) in enumerate(b.seqs)], dev)
    D, hd, scale = b.heads * b.hd, b.hd, 1.0 / math.sqrt(b.hd)
    cs = (None, None, None) if rope is None else (rope[0].to(dev), rope[1].to(dev), torch.as_tensor(positions, dtype=torch.int32).to(dev))
    if kernel == "fused":
        out = ops.attn_decode_fused(x, cols["q"], cols["k"], cols["v"], kp, vp, table, desc, b.heads, hd, scale, *cs)
    else:
        q = x[:, cols["q"]:cols["q"] + D]                      # a view: ldq = the qkv row stride
        out = ops.attn_decode(q, kp, vp, table, desc, b.heads, hd, scale, max_kv or max(L for L, _ in b.seqs))
    torch.cuda.synchronize()
    return out.cpu()[torch.as_tensor(b.rows)].view(len(b.seqs), b.heads, hd), kp, vp, x


# ---- probe data --------------------------------------------------------------------------------------------------------------------
def _code(j, heads, hd, amp):
    """[len(j)][heads][hd]: +-amp on the first NB dimensions by the bits of position j, zero elsewhere"""
    j = np.asarray(j, np.int64)
    c = np.zeros((j.size, heads, hd), np.float32)
    c[:, :, :NB] = (((j[:, None] >> np.arange(NB)) & 1) * 2 - 1)[:, None, :] * amp
    return torch.from_numpy(c)


def _venc(j, heads, hd):
    """an injective small-integer encoding of (position, head) in every V row: d0 = j % 128 + 1, d1 = j // 128 + 1, d2 = head + 1, the
    rest (j + 3 d + 5 head) % 31 - 15 -- exact in bf16 and fp16"""
    j = np.asarray(j, np.int64)[:, None, None]
    h = np.arange(heads)[None, :, None]
    d = np.arange(hd)[None, None, :]
    v = (j + 3 * d + 5 * h) % 31 - 15
    v = np.broadcast_to(v, (j.shape[0], heads, hd)).copy()
    v[:, :, 0] = (j[:, :, 0] % 128 + 1)
    v[:, :, 1] = (j[:, :, 0] // 128 + 1)
    v[:, :, 2] = h[:, :, 0] + 1
    return torch.from_numpy(v.astype(np.float32))


def _one_hot(dev, kernel, dtype, hd, groups, targets_of, seed, vals=None):
    """targets_of(L, n, heads) -> [n][heads] key positions; returns (got, want) as int16 bits"""
    heads = 32
    vals = vals or (lambda j: _venc(j, heads, hd))
    fused = kernel == "fused"
    b = Batch(groups, heads, hd, dtype, fused, lambda j: _code(j, heads, hd, A_CODE), vals, seed)
    tg = np.concatenate([targets_of(L, n, heads) for L, n in groups])           # [nseq][heads]
    q = torch.stack([_code(tg[i], heads, hd, B_CODE)[np.arange(heads), np.arange(heads)] for i in range(len(tg))])
    last = np.array([L - 1 for L, _ in b.seqs])
    knew = _code(last, heads, hd, A_CODE) if fused else None
    vnew = vals(last) if fused else None
    got, *_ = _launch(dev, kernel, b, q, knew, vnew)
    want = torch.stack([vals(tg[i])[np.arange(heads), np.arange(heads)] for i in range(len(tg))])
    return _bits(got), _bits(R.to_op(R.to_f16_page(want.to(dtype)), dtype)), tg


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_probes_address_every_key_exactly(dev, dtype, hd, kernel):
    """One key per (sequence, head) dominates by >= 2^150: the output is exactly its V row. Every position of every context in
    PROBE_LENS is a target once (32 heads x ceil(L / 32) sequences sharing pages); for the fused kernel that includes the new token, in
    a page (L = 2, 64, ...) and as the first key of a fresh page (L = 1, 65, 129, 513, 577, 1089). At 4097 and 8193: every position
    = 0, 1, 62, 63 (mod 64), the new token and a seeded sample."""
    def sweep(L, n, heads):
        return (np.arange(n * heads) % L).reshape(n, heads)
    got, want, tg = _one_hot(dev, kernel, dtype, hd, [(L, (L + 31) // 32) for L in PROBE_LENS], sweep, 1)
    bad = (got != want).any(dim=-1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} probes wrong, e.g. target {tg[bad.numpy()][:4]}"

    rng = np.random.default_rng(2)
    sets = {}
    for L in (4097, 8193):
        j = np.arange(L)
        pick = np.union1d(j[np.isin(j % 64, (0, 1, 62, 63))], rng.choice(L, 64, replace=False))
        pick = np.union1d(pick, [L - 1])
        sets[L] = np.resize(pick, ((pick.size + 31) // 32) * 32)
    got, want, tg = _one_hot(dev, kernel, dtype, hd, [(L, s.size // 32) for L, s in sets.items()],
                             lambda L, n, heads: sets[L].reshape(n, heads), 3)
    bad = (got != want).any(dim=-1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} long-context probes wrong, e.g. target {tg[bad.numpy()][:4]}"


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_probes_combine_waves_and_splits_exactly(dev, dtype, hd, kernel):
    """q = 0: every weight is exp2(0) = 1 and every partial sum of small-integer V is exact in fp32, so the output is the kernel's own
    final expression bit for bit -- o / l (fused) or o * (1 / l) (split) -- whatever the tiles' distribution over waves and splits. One
    launch holds every context (the split count comes from the longest: 32 with 8193 and 12345, the clamp, where waves run 2 rounds)."""
    heads = 32
    lens = PROBE_LENS + ([8193, 12345] if kernel == "split" else [])
    fused = kernel == "fused"

    def vals(j):
        j = np.asarray(j, np.int64)[:, None, None]
        return torch.from_numpy(((j * 7 + np.arange(heads)[None, :, None] * 3 + np.arange(hd)[None, None, :] * 5) % 17 - 8).astype(np.float32))
    b = Batch([(L, 1) for L in lens], heads, hd, dtype, fused, lambda j: _code(j, heads, hd, 1.0), vals, 4)
    last = np.array(lens) - 1
    got, *_ = _launch(dev, kernel, b, torch.zeros((len(lens), heads, hd)),
                      _code(last, heads, hd, 1.0) if fused else None, vals(last) if fused else None)
    for i, L in enumerate(lens):
        o = vals(np.arange(L)).double().sum(dim=0).float()     # exact
        l = torch.tensor(float(L), dtype=torch.float32)
        want = o / l if fused else o * (1.0 / l)
        assert torch.equal(_bits(got[i]), _bits(R.to_op(want, dtype))), (L, (got[i].float() - want).abs().max())


# ---- random data: the per-element bound ----------------------------------------------------------------------------------------------
def _rope_tables(hd):
    from oracle import vitron_oracle as O
    return O.rope_tables(hd, 8192 + 128)


def _check_bound(name, got, q, k, v, scale, dtype, exact_scores=False, ref=None):
    """|got - fp64| <= decode_bound, element by element; returns the largest error-to-bound ratio"""
    ref = R.decode_ref(q, k, v, scale) if ref is None else ref
    bound = R.decode_bound(q, k, v, scale, R.FMT[dtype], exact_scores)
    err = (got.double() - ref).abs()
    ratio = float((err / bound).max())
    assert torch.isfinite(got.float()).all() and (err <= bound).all(), f"{name}: error / bound up to {ratio:.3g}"
    return ratio


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_data_within_the_fp64_bound_at_long_ragged_contexts(dev, dtype, hd):
    """The engine's way: vt_kv_tiles writes the cache with rope (its K / V^T pages are checked bit for bit against pack_pages of
    rope_ref), then one step through the fused kernel, and through vt_kv_tiles + the split kernel with max_kv_len at the true maximum
    and above it. Positions differ from kv_len - 1 (a per-sequence offset), q_row0 is permuted, qkv has a wide row and permuted column
    blocks. 32 heads at hd 128, 8 at hd 64."""
    from vitron_amd import ops
    heads = 32 if hd == 128 else 8
    D, scale = heads * hd, 1.0 / math.sqrt(hd)
    cos, sin = _rope_tables(hd)
    gen = torch.Generator(device=dev).manual_seed(hd + (dtype == torch.float16))
    report = {}
    for batch_i, (lens, offs) in enumerate([([1, 64, 65, 513, 2047, 2048, 2049, 5121, 8192], [0, 5, 100, 0, 1, 64, 3, 0, 17]),
                                            ([1, 65, 5121, 700, 64], [9, 0, 1, 31, 0])]):
        # the whole context of every sequence (the past and the new token) at once, drawn on the device
        tot = sum(lens)
        kv = (torch.randn((tot, 2, heads, hd), generator=gen, device=dev)).to(dtype)
        qn = (torch.randn((len(lens), heads, hd), generator=gen, device=dev)).to(dtype).cpu()
        kv_h = kv.cpu()
        starts = np.cumsum([0] + lens[:-1])
        pos = np.concatenate([np.arange(L) + o for L, o in zip(lens, offs)])
        b = Batch([(L, 1) for L in lens], heads, hd, dtype, False, lambda j: torch.zeros((len(j), heads, hd)),
                  lambda j: torch.zeros((len(j), heads, hd)), 10 + batch_i)
        # b's pages: kv_len = L each, holding zeros; the prefill below overwrites the first L - 1 keys (and zero-fills padding)
        kp, vp = torch.full_like(b.kp, NAN).to(dev), torch.full_like(b.vp, NAN).to(dev)
        table = torch.tensor(b.table, dtype=torch.int32, device=dev)
        past = [(int(s), L - 1, L - 1, off) for s, (L, off) in zip(starts, b.seqs) if L > 1]
        pre = torch.zeros((tot, 3 * D + 192), dtype=dtype, device=dev)
        pre[:, 0:D] = kv[:, 0].reshape(tot, D)
        pre[:, D + 64:2 * D + 64] = kv[:, 1].reshape(tot, D)
        ops.kv_tiles(pre, 2 * D + 128, 0, D + 64, kp, vp, table, ops.seq_desc_tensor(past, dev), max(L - 1 for L in lens) // 64 + 1,
                     heads, hd, cos.to(dev), sin.to(dev), torch.as_tensor(pos, dtype=torch.int32, device=dev))
        # host: every key rotated at its position; the pages vt_kv_tiles wrote == pack_pages of them, NaN pages untouched
        k_rot = R.rope_ref(kv_h[:, 0], cos, sin, pos, dtype)
        want_k, want_v = torch.full_like(b.kp, NAN), torch.full_like(b.vp, NAN)
        for s, (L, off) in zip(starts, b.seqs):
            if L > 1:
                tb = b.table[off:off + (L - 2) // 64 + 1]
                R.pack_pages(k_rot[s:s + L - 1], kv_h[s:s + L - 1, 1], tb, heads, hd, dtype, out=(want_k, want_v))
        assert torch.equal(_bits(kp.cpu()), _bits(want_k)) and torch.equal(_bits(vp.cpu()), _bits(want_v)), "vt_kv_tiles pages"
        # the step: the new token is key L - 1 at position L - 1 + offset
        last = starts + np.array(lens) - 1
        knew, vnew = kv_h[last, 0], kv_h[last, 1]
        rope = (cos, sin)
        pos_new = np.zeros(len(lens), np.int64)
        pos_new[b.rows] = pos[last]                                   # positions[] is indexed by qkv row
        q_rot = R.rope_ref(qn, cos, sin, pos[last], dtype)
        fused_out, kf, vf, x = _launch(dev, "fused", b, qn, knew, vnew, rope=rope, positions=pos_new, pages=(kp.clone(), vp.clone()))
        x0, _ = _qkv(b, qn, knew, vnew)
        assert torch.equal(_bits(x.cpu()), _bits(x0)), "the fused kernel must not modify qkv"
        # split path: vt_kv_tiles appends the token and rotates q in place, then the split kernel reads the q columns
        cols = dict(k=0, v=D + 64, q=2 * D + 128)
        step = ops.seq_desc_tensor([(int(b.rows[i]), 1, L, off) for i, (L, off) in enumerate(b.seqs)], dev)
        ops.kv_tiles(x, cols["q"], cols["k"], cols["v"], kp, vp, table, step, 1, heads, hd, cos.to(dev), sin.to(dev),
                     torch.as_tensor(pos_new, dtype=torch.int32, device=dev))
        assert torch.equal(_bits(kf.cpu()), _bits(kp.cpu())) and torch.equal(_bits(vf.cpu()), _bits(vp.cpu())), "fused vs kv_tiles pages"
        assert torch.equal(_bits(x[:, cols["q"]:cols["q"] + D].cpu()[torch.as_tensor(b.rows)].view(-1, heads, hd)), _bits(q_rot))
        outs = {"fused": fused_out}
        for extra in (0, 1000):
            q = x[:, cols["q"]:cols["q"] + D]
            o = ops.attn_decode(q, kp, vp, table, step, heads, hd, scale, max(lens) + extra)
            torch.cuda.synchronize()
            outs[f"split(max_kv_len +{extra})"] = o.cpu()[torch.as_tensor(b.rows)].view(len(lens), heads, hd)
        for i, (s, L) in enumerate(zip(starts, lens)):
            kk, vv = k_rot[s:s + L], R.to_f16_page(kv_h[s:s + L, 1])
            ref = R.decode_ref(q_rot[i], kk, vv, scale)
            for name, o in outs.items():
                r = _check_bound(f"{name} L={L}", o[i], q_rot[i], kk, vv, scale, dtype, ref=ref)
                report[name.split("(")[0]] = max(report.get(name.split("(")[0], 0.0), r)
    print(f"\n[decode attn bound] {R.FMT[dtype]} hd {hd}: highest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))


# ---- score-range edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_score_range_edges(dev, dtype, hd, kernel):
    """(1) Every score shifted by +-A B with |s * scale * log2 e| ~ 2^11 (a shared component on the last dimension; integer operands,
    so the fp32 scores are exact): the output matches the unshifted problem's fp64 result within the bound of the shifted operands
    (whose only offset-dependent term is the rounding of s * scale * log2 e). (2) A softmax peaked by >= 200 (log2) or by 12 on one key
    in the first tile, in a middle wave's tile and as the last key (a fresh page's first: for the fused kernel the new token)."""
    heads, L = 8, 5121
    fused = kernel == "fused"
    scale = 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(hd * 7 + len(kernel))
    ints = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    q0, k0, v = ints(3, heads, hd), ints(L, heads, hd), torch.randn((L, heads, hd), generator=g).to(dtype).float()
    q0[:, :, -1] = 0
    k0[:, :, -1] = 0
    qs, ks = q0.clone(), k0.clone()
    qs[1, :, -1], qs[2, :, -1] = 128.0, -128.0             # scores shifted by +-128 * 128: |s * scale * log2 e| 2089 (hd 128), 2954
    ks[:, :, -1] = 128.0

    def run(qq, kk, n_seq):
        b = Batch([(L, n_seq)], heads, hd, dtype, fused, lambda j: kk[j], lambda j: v[j], 20)
        last = [L - 1] * n_seq
        got, *_ = _launch(dev, kernel, b, qq, kk[last] if fused else None, v[last] if fused else None)
        return got

    got = run(qs, ks, 3)
    vv = R.to_f16_page(v.to(dtype))
    ratios = []
    for i in range(3):
        ref = R.decode_ref(q0[i], k0, vv, scale)
        ratios.append(_check_bound(f"shift {i}", got[i], qs[i], ks, vv, scale, dtype, exact_scores=True, ref=ref))
    # (2) peaked
    qp = torch.randn((6, heads, hd), generator=g).to(dtype).float()
    kp = torch.randn((L, heads, hd), generator=g).to(dtype).float()
    where = [5, 20 * 64 + 33, 43 * 64 + 7, L - 1, 20 * 64 + 33, L - 1]
    gaps = [200, 200, 200, 200, 12, 12]
    outs = []
    for i, (j, gap) in enumerate(zip(where, gaps)):
        k_i = kp.clone()
        c = gap / (scale * R.LOG2E) + 4 * math.sqrt(hd)           # score of key j above 4 sigma of the others by `gap` in log2 units
        k_i[j] = (qp[i] * (c / float((qp[i] * qp[i]).sum(-1).mean()))).to(dtype).float()
        b = Batch([(L, 1)], heads, hd, dtype, fused, lambda jj: k_i[jj], lambda jj: v[jj], 30 + i)
        got_i, *_ = _launch(dev, kernel, b, qp[i:i + 1], k_i[[L - 1]] if fused else None, v[[L - 1]] if fused else None)
        ratios.append(_check_bound(f"peak at {j}, gap {gap}", got_i[0], qp[i].to(dtype), k_i.to(dtype), vv, scale, dtype))
    print(f"\n[decode attn edges] {kernel} {R.FMT[dtype]} hd {hd}: highest error / bound {max(ratios):.3f}")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("hd", [64, 128])
def test_bf16_values_beyond_fp16_range_saturate(dev, hd, kernel):
    """bf16 V above 65504 lands in the fp16 V^T pages (and the fused kernel's LDS copy of the new one) as +-65504: the one-hot output is
    bf16(+-65504) = +-65536, finite. Every key of a 130-key context, the new token included, is a target once."""
    def vals(j):
        return _venc(j, 32, hd) * 4096.0                      # |v| up to 2^7 * 2^12 > 65504, mixed signs; exact in bf16
    got, want, tg = _one_hot(dev, kernel, torch.bfloat16, hd, [(130, 5)], lambda L, n, heads: (np.arange(n * heads) % L).reshape(n, heads),
                             40, vals=vals)
    assert torch.isfinite(got.view(torch.bfloat16).float()).all()
    assert (want.view(torch.bfloat16).float().abs() == 65536.0).any()
    assert torch.equal(got, want)


# ---- the fused kernel's page invariants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_is_idempotent_and_touches_only_its_slot(dev, dtype, hd):
    """One step with rope over contexts 1, 64, 65, 700, 2049 (pages packed on the host, NaN everywhere else). Then: qkv unchanged; pages
    outside the tables bit-identical; in the written page only key r_new (K row, V^T column) changes, or, on a fresh page, the rest is
    zero; the step run again on its own output gives the same bits everywhere; stale finite values past kv_len in the last page (a page
    reused or rolled back) change no output bit, in the split kernel either."""
    from vitron_amd import ops
    heads = 32 if hd == 128 else 8
    lens = [1, 64, 65, 700, 2049]
    scale = 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(50 + hd)
    kc = torch.randn((max(lens), heads, hd), generator=g).to(dtype)
    vc = torch.randn((max(lens), heads, hd), generator=g).to(dtype)
    b = Batch([(L, 1) for L in lens], heads, hd, dtype, True, lambda j: kc[j], lambda j: vc[j], 60)
    qn = torch.randn((len(lens), heads, hd), generator=g).to(dtype)
    knew = torch.randn((len(lens), heads, hd), generator=g).to(dtype)
    vnew = torch.randn((len(lens), heads, hd), generator=g).to(dtype)
    cos, sin = _rope_tables(hd)
    pos = np.zeros(len(lens), np.int64)
    pos[b.rows] = np.array(lens) - 1 + 40                   # positions[] by qkv row, 40 past kv_len - 1
    kw = dict(rope=(cos, sin), positions=pos)
    out1, k1, v1, x1 = _launch(dev, "fused", b, qn, knew, vnew, **kw)
    x0, _ = _qkv(b, qn, knew, vnew)
    assert torch.equal(_bits(x1.cpu()), _bits(x0)), "qkv modified"
    k1h, v1h = k1.cpu().view(b.npages, heads, 64, hd), v1.cpu().view(b.npages, heads, hd, 64)
    k0h, v0h = b.kp.view(b.npages, heads, 64, hd), b.vp.view(b.npages, heads, hd, 64)
    used = b.used()
    assert torch.equal(_bits(k1h[~used]), _bits(k0h[~used])) and torch.equal(_bits(v1h[~used]), _bits(v0h[~used])), "untouched pages"
    k_rot = R.rope_ref(knew, cos, sin, np.array(lens) - 1 + 40, dtype)
    for i, (L, off) in enumerate(b.seqs):
        t_last, r = (L - 1) // 64, (L - 1) % 64
        for t in range(t_last + 1):
            p = b.table[off + t]
            kw_, vw_ = k0h[p].clone(), v0h[p].clone()
            if t == t_last:
                if r == 0:
                    kw_.zero_()
                    vw_.zero_()
                kw_[:, r] = k_rot[i]
                vw_[:, :, r] = R.to_f16_page(vnew[i])
            assert torch.equal(_bits(k1h[p]), _bits(kw_)) and torch.equal(_bits(v1h[p]), _bits(vw_)), (L, t)
        q_rot = R.rope_ref(qn[i:i + 1], cos, sin, [L - 1 + 40], dtype)[0]
        kk = torch.cat([R.unpack_pages(b.kp, b.vp, b.table[off:off + t_last + 1], L - 1, heads, hd)[0], k_rot[i:i + 1]])
        vv = torch.cat([R.unpack_pages(b.kp, b.vp, b.table[off:off + t_last + 1], L - 1, heads, hd)[1], R.to_f16_page(vnew[i:i + 1])])
        _check_bound(f"fused L={L}", out1[i], q_rot, kk, vv, scale, dtype)
    # the same step again, on the pages it wrote
    out2, k2, v2, _ = _launch(dev, "fused", b, qn, knew, vnew, pages=(k1.clone(), v1.clone()), **kw)
    assert torch.equal(_bits(out2), _bits(out1)) and torch.equal(_bits(k2.cpu()), _bits(k1.cpu())) and torch.equal(_bits(v2.cpu()), _bits(v1.cpu()))
    # stale values past kv_len (and in the new token's own slot, before the step) of every last page that holds older keys
    ks, vs = b.kp.clone().view(b.npages, heads, 64, hd), b.vp.clone().view(b.npages, heads, hd, 64)
    k1s, v1s = k1.cpu().view(b.npages, heads, 64, hd).clone(), v1.cpu().view(b.npages, heads, hd, 64).clone()
    for L, off in b.seqs:
        r = (L - 1) % 64
        if r:
            p = b.table[off + (L - 1) // 64]
            junk_k = torch.randn((heads, 64 - r, hd), generator=g).to(dtype) * 3
            junk_v = torch.randn((heads, hd, 64 - r), generator=g).half() * 3
            ks[p, :, r:], vs[p, :, :, r:] = junk_k, junk_v
            k1s[p, :, r + 1:], v1s[p, :, :, r + 1:] = junk_k[:, 1:], junk_v[:, :, 1:]
    out3, *_ = _launch(dev, "fused", b, qn, knew, vnew, pages=(ks.reshape(-1).to(dev), vs.reshape(-1).to(dev)), **kw)
    assert torch.equal(_bits(out3), _bits(out1)), "stale values past kv_len changed the fused output"
    # the split kernel on the pages after the step, with and without stale values past kv_len
    D = heads * hd
    q = torch.zeros((len(lens), D), dtype=dtype)
    q[torch.as_tensor(b.rows)] = R.rope_ref(qn, cos, sin, np.array(lens) - 1 + 40, dtype).reshape(len(lens), D)
    q = q.to(dev)
    table = torch.tensor(b.table, dtype=torch.int32, device=dev)
    desc = ops.seq_desc_tensor([(int(b.rows[i]), 1, L, off) for i, (L, off) in enumerate(b.seqs)], dev)
    a = ops.attn_decode(q, k1, v1, table, desc, heads, hd, scale, max(lens))
    s = ops.attn_decode(q, k1s.reshape(-1).to(dev), v1s.reshape(-1).to(dev), table, desc, heads, hd, scale, max(lens))
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.cpu()), _bits(s.cpu())), "stale values past kv_len changed the split output"
