"""Prefill attention on the GPU (vt_flash_attn through ops.flash_attn: flash_attn_kernel<HD, CAUSAL, 4, 2> of vitron_amd/csrc/vt_attn.hip at
head_dim 64 and 128, flash_attn_w4_kernel of vt_attn_w4.hip in its placed, unplaced, persistent and natural-order forms) against the host
restatement in tests/attn_ref.py, in both operand builds: uniform probes that pin every row's key count exactly, one-hot probes that pin
the addressing of every key relative to the row's own position, random data inside a per-element fp64 bound (prefill_bound), and the
contract edges. Pages are packed on the host (pack_pages) over a shuffled pool whose spare pages hold NaN unless a test is about
vt_kv_tiles writing them; Q is a view into a wider buffer, the sequences' rows are permuted, and the output buffer starts as NaN: rows no
sequence owns and the columns beside the output must stay NaN (checked on every launch)."""
import math

import numpy as np
import pytest
import torch

from tests import attn_ref as R
from tests.test_gpu_decode_attn import A_CODE, B_CODE, NAN, NB, _bits, _code, _rope_tables, _venc

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
PERSIST8 = 4 | (8 << 8)          # the persistent form with at most 8 workgroups: every workgroup walks many blocks
# the kernel axis: head_dim 64 has the one kernel; head_dim 128 the selectors of vt_flash_attn_select
KAXIS = [pytest.param(64, None, id="hd64")] + [pytest.param(128, s, id=f"hd128-sel{n}") for s, n in
                                               ((1, "1"), (2, "2"), (3, "3"), (PERSIST8, "4x8"), (5, "5"), (0, "0"))]


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    _lib.load(operand="fp16")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _auto_kernel_afterwards():
    yield
    from vitron_amd import ops
    ops.flash_attn_select(0)


_CACHE = {}


def _cached(key, build):
    """the problem of the last key only: the kernel axis varies fastest, so one host packing serves every selector"""
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = build()
    return _CACHE[key]


# ---- problems packed on the host ------------------------------------------------------------------------------------------------------
class Problem:
    """seqs = [(q_len, past)]. k_of(si, j) / v_of(si, j) -> [len(j)][heads][hd]: the cache of sequence si at positions j;
    q_of(si) -> [q_len][heads][hd]. Pages: a shuffled pool with `spare` pages more than the tables name, NaN wherever no key lives (the
    padding of a last page is zero, as vt_kv_tiles leaves it). Rows: the sequences in a permuted order with `gap` rows nobody owns in
    front, between and behind; Q = x[:, 8 : 8 + D] of a buffer D + 72 wide (NaN elsewhere), O = o[:, :D] of a NaN buffer D + 8 wide."""

    def __init__(self, seqs, heads, hd, dtype, q_of, k_of, v_of, seed, spare=3, gap=3):
        rng = np.random.default_rng(seed)
        D = heads * hd
        ntl = [(q + p + 63) // 64 for q, p in seqs]
        self.npages = sum(ntl) + spare
        it = iter(rng.permutation(self.npages).tolist())
        size = self.npages * heads * 64 * hd
        self.kp, self.vp = torch.full((size,), NAN, dtype=dtype), torch.full((size,), NAN, dtype=torch.float16)
        row0, r = {}, gap
        for si in rng.permutation(len(seqs)).tolist():
            row0[si] = r
            r += seqs[si][0] + gap
        self.rows = r
        self.x = torch.full((self.rows, D + 72), NAN, dtype=dtype)
        self.owned = torch.zeros(self.rows, dtype=torch.bool)
        self.table, self.desc = [], []
        for si, (ql, past) in enumerate(seqs):
            pages = [next(it) for _ in range(ntl[si])]
            R.pack_pages(k_of(si, np.arange(past + ql)), v_of(si, np.arange(past + ql)), pages, heads, hd, dtype, out=(self.kp, self.vp))
            self.x[row0[si]:row0[si] + ql, 8:8 + D] = torch.as_tensor(q_of(si)).reshape(ql, D).to(dtype)
            self.owned[row0[si]:row0[si] + ql] = True
            self.desc.append((row0[si], ql, past + ql, len(self.table)))
            self.table += pages
        self.table += [next(it)] * 4             # entries no sequence owns, naming a NaN page
        self.seqs, self.heads, self.hd, self.dtype, self.D = seqs, heads, hd, dtype, D
        self._dev = None

    def on(self, dev):
        from vitron_amd import ops
        if self._dev is None:
            self._dev = (self.x.to(dev), self.kp.to(dev), self.vp.to(dev), torch.tensor(self.table, dtype=torch.int32, device=dev),
                         ops.seq_desc_tensor(self.desc, dev))
        return self._dev


def _launch(dev, pb: Problem, sel, causal, raw=False):
    """one vt_flash_attn launch -> [per sequence [q_len][heads][hd]] on the host (raw: the whole output buffer's bits instead)"""
    from vitron_amd import ops
    if sel is not None:
        ops.flash_attn_select(sel)
    x, kp, vp, table, desc = pb.on(dev)
    D = pb.D
    obuf = torch.full((pb.rows, D + 8), NAN, dtype=pb.dtype, device=dev)
    ops.flash_attn(x[:, 8:8 + D], kp, vp, table, desc, max(q for q, _ in pb.seqs), pb.heads, pb.hd, causal, 1.0 / math.sqrt(pb.hd), out=obuf[:, :D])
    torch.cuda.synchronize()
    o = obuf.cpu()
    assert torch.isnan(o[~pb.owned].float()).all(), "rows no sequence owns were written"
    assert torch.isnan(o[:, D:].float()).all(), "columns beside the output were written"
    if raw:
        return _bits(o)
    return [o[r0:r0 + ql, :D].reshape(ql, pb.heads, pb.hd) for r0, ql, _, _ in pb.desc]


# ---- a. uniform probes: every row's key count exact --------------------------------------------------------------------------------------
UNIFORM_PAST0 = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 577, 1089, 2304]
# chunks behind a past: past % 64 in {0, 1, 31, 32, 33, 63}, past up to 4096, lengths that are no multiples of 32, kv_len = 0, 1, 62, 63
# (mod 64) among them
UNIFORM_CHUNKS = [(40, 4096), (33, 1), (95, 31), (31, 32), (31, 33), (66, 63), (257, 1000), (300, 2047), (130, 4033), (513, 1056),
                  (70, 3999), (100, 2081), (1, 64), (1, 63), (2, 4094)]


def _uniform_vals(j, heads, hd):
    j = np.asarray(j, np.int64)[:, None, None]
    return torch.from_numpy(((j * 7 + np.arange(heads)[None, :, None] * 3 + np.arange(hd)[None, None, :] * 5) % 17 - 8).astype(np.float32))


def _uniform_problem(dtype, hd):
    heads = 8
    seqs = [(L, 0) for L in UNIFORM_PAST0 + ([5120] if hd == 128 else [])] + UNIFORM_CHUNKS
    assert {p % 64 for _, p in UNIFORM_CHUNKS} >= {0, 1, 31, 32, 33, 63} and {(q + p) % 64 for q, p in UNIFORM_CHUNKS} >= {0, 1, 62, 63}
    pb = Problem(seqs, heads, hd, dtype, lambda si: torch.zeros((seqs[si][0], heads, hd)), lambda si, j: _code(j + si, heads, hd, 3.0),
                 lambda si, j: _uniform_vals(j + 11 * si, heads, hd), 100 + hd)
    want = {True: [], False: []}
    for si, (ql, past) in enumerate(seqs):
        cs = torch.cumsum(_uniform_vals(np.arange(past + ql) + 11 * si, heads, hd).double(), dim=0)       # exact: small integers
        for causal in (True, False):
            S = cs[past:] if causal else cs[-1:].expand(ql, heads, hd)
            n = torch.arange(past + 1, past + ql + 1, dtype=torch.float32) if causal else torch.full((ql,), float(past + ql))
            assert float(S.abs().max()) * 128 < 2 ** 24
            # the kernels' own final expression: oacc * (1 / l) with a weight of 2^7 on every visible key
            want[causal].append(_bits(R.to_op((S.float() * 128.0) * (1.0 / (n * 128.0))[:, None, None], dtype)))
    return pb, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd,sel", KAXIS)
def test_uniform_probes_pin_every_rows_key_count(dev, dtype, causal, hd, sel):
    """q = 0: every visible key weighs exactly 2^(0 + P_BIAS) = 128 and V holds integers of |v| <= 8, so every partial sum is exact in fp32
    and row i is the kernels' final expression bit for bit, fl(128 S_i) * fl(1 / fl(128 n_i)) rounded to the operand, with S_i the sum of V
    over the n_i visible keys (past + i + 1 causal, kv_len otherwise). One key too many or too few changes n_i and S_i of that row. One
    launch holds sequences of 1 .. 2304 rows (5120 at head_dim 128: 20 blocks of 256 rows, warm seams of the persistent form) and
    chunks behind a past of up to 4096 keys (cold seams), so short sequences skip most of the grid's blocks."""
    pb, want = _cached(("uniform", dtype, hd), lambda: _uniform_problem(dtype, hd))
    got = _launch(dev, pb, sel, causal)
    bad = []
    for (ql, past), g, w in zip(pb.seqs, got, want[causal]):
        rows = (_bits(g) != w).flatten(1).any(dim=1).nonzero().flatten().tolist()
        if rows:
            bad.append(f"(q_len {ql}, past {past}): {len(rows)} rows, first {rows[:6]}")
    assert not bad, "; ".join(bad)


# ---- b. one-hot probes: addressing exact -------------------------------------------------------------------------------------------------
def _one_hot(dev, dtype, hd, sel, causal, seqs, targets, seed, name):
    """Keys carry the +-A code of their position on NB dimensions and -NB A on dimension NB; the query of (row, head) carries the +-B code of
    its target and B on dimension NB: the target scores NB A B - NB A B = 0 EXACTLY (all partial sums are integers below 2^24), every
    other key at least 2 A B lower (261 in log2 units at head_dim 128, 369 at 64). So the running maximum is 0 from the target's tile on,
    whatever came before is scaled by exp2(<= -261) = 0, the target's weight is exp2(7) in the fp16 that feeds the MFMA and in the fp32
    that feeds l alike, every other weight is exp2(<= -254) = 0, and the row is fl(128 v) * fl(1 / 128) = v: the target's V row (_venc,
    8-bit integers) bit for bit. targets(si) -> [q_len][heads] key positions, each visible to its row."""
    heads = 32 if hd == 128 else 8

    def build():
        def keys(si, j):
            k = _code(j, heads, hd, A_CODE)
            k[:, :, NB] = -NB * A_CODE
            return k

        tgs = [np.asarray(targets(si), np.int64) for si in range(len(seqs))]
        for (ql, past), tg in zip(seqs, tgs):
            assert tg.shape == (ql, heads) and (tg >= 0).all() and (tg <= ((past + np.arange(ql))[:, None] if causal else past + ql - 1)).all()

        def query(si):
            q = _code(tgs[si].reshape(-1), 1, hd, B_CODE).reshape(seqs[si][0], heads, hd)
            q[:, :, NB] = B_CODE
            return q

        pb = Problem(seqs, heads, hd, dtype, query, keys, lambda si, j: _venc(j + si, heads, hd), seed)
        want = [_bits(R.to_op(_venc(np.arange(past + ql) + si, heads, hd)[torch.from_numpy(tg), torch.arange(heads)[None, :]], dtype))
                for si, ((ql, past), tg) in enumerate(zip(seqs, tgs))]
        return pb, want, tgs

    pb, want, tgs = _cached((name, dtype, hd, causal), build)
    got = _launch(dev, pb, sel, causal)
    bad = []
    for (ql, past), g, w, tg in zip(seqs, got, want, tgs):
        wrong = (_bits(g) != w).any(dim=-1)
        if wrong.any():
            i, h = wrong.nonzero()[0].tolist()
            bad.append(f"(q_len {ql}, past {past}): {int(wrong.sum())} of {wrong.numel()} probes, first row {i} head {h} target {tg[i, h]}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,sel", KAXIS)
def test_one_hot_diagonal_band(dev, dtype, hd, sel):
    """target = past + i - delta for every delta in 0 .. 159 the row allows (key 0 otherwise): the heads carry different deltas and the
    delta group advances with the row's 256-row block (128-row block at head_dim 64), so that every row position inside a block meets
    every delta: every position of a key in its 64-key tile and 32-key sub tile relative to the row, where need_mask, lim, the
    per-wave skip of the mask and the w4 kernel's sub tile pipeline live. With pasts of 0, 63 and 1033 (mod 64: 0, 63, 9)."""
    heads, blk = (32, 256) if hd == 128 else (8, 128)
    seqs = [(160 // heads * blk, 0), (160 // heads * blk, 1033), (160 // heads * blk + 5, 63), (700, 4000)]

    def targets(si):
        ql, past = seqs[si]
        i = np.arange(ql)[:, None]
        delta = (np.arange(heads)[None, :] + heads * (i // blk)) % 160
        return np.maximum(past + i - delta, 0)
    _one_hot(dev, dtype, hd, sel, True, seqs, targets, 200 + hd, "band")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,sel", KAXIS)
def test_one_hot_fixed_columns(dev, dtype, hd, sel):
    """target = a fixed key for every row that sees it (its own diagonal key otherwise): 0, 1, 31, 32, 63, 64, past - 1, past, past + 1 and
    a seeded sample, spread over the heads."""
    heads = 32 if hd == 128 else 8
    seqs = [(300, 0), (257, 100), (40, 1000), (130, 4033), (1100, 0)]
    rng = np.random.default_rng(7)

    def targets(si):
        ql, past = seqs[si]
        cols = [0, 1, 31, 32, 63, 64, past - 1, past, past + 1] + rng.integers(0, past + ql, 23).tolist()
        col = np.array([cols[(h + si) % len(cols)] for h in range(heads)])[None, :]
        diag = (past + np.arange(ql))[:, None]
        return np.where((col >= 0) & (col <= diag), col, diag)
    _one_hot(dev, dtype, hd, sel, True, seqs, targets, 300 + hd, "columns")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,sel", KAXIS)
def test_one_hot_non_causal_every_key(dev, dtype, hd, sel):
    """Non-causal: every key of L = 257 and 577 (the towers' sequence lengths) and of 700 is the target of some row (head 0 of row i
    targets key i; the other heads are 37 h further on)."""
    heads = 32 if hd == 128 else 8
    seqs = [(257, 0), (577, 0), (700, 0)]
    _one_hot(dev, dtype, hd, sel, False, seqs, lambda si: (np.arange(seqs[si][0])[:, None] + 37 * np.arange(heads)[None, :]) % seqs[si][0],
             400 + hd, "full")


def _ramp_problem(dtype, hd):
    heads, beta = (32 if hd == 128 else 8), 2048.0
    seqs = [(300, 0), (257, 100), (70, 4000), (33, 31)]

    def keys(si, j):
        j = np.asarray(j, np.int64)
        k = torch.zeros((j.size, heads, hd))
        k[:, :, 0] = torch.from_numpy((64 * (j // 64)).astype(np.float32))[:, None]
        k[:, :, 1] = torch.from_numpy((j % 64).astype(np.float32))[:, None]
        k[:, :, 2:4] = beta
        return k

    def query(si):
        ql, past = seqs[si]
        r = past + np.arange(ql)
        q = torch.zeros((ql, heads, hd))
        q[:, :, 0:2] = beta
        q[:, :, 2] = torch.from_numpy((-64 * (r // 64)).astype(np.float32))[:, None]
        q[:, :, 3] = torch.from_numpy((-(r % 64)).astype(np.float32))[:, None]
        return q

    vals = lambda si, j: _venc(j + si, heads, hd) * 256.0
    pb = Problem(seqs, heads, hd, dtype, query, keys, vals, 500 + hd)
    want = [_bits(R.to_op(vals(si, past + np.arange(ql)), dtype)) for si, (ql, past) in enumerate(seqs)]
    return pb, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,sel", KAXIS)
def test_keys_above_the_diagonal_never_reach_a_row(dev, dtype, hd, sel):
    """The reverse probe: key j scores beta (j - (past + i)) for row i, beta = 2048 (built from four dimensions holding 64 (j // 64), j % 64
    and the row's own two digits: 8-bit integers times powers of two, every partial sum a multiple of 2^11 below 2^35, exact) -- 0 on the
    row's diagonal key, 261 (369) log2 units lower per key below it, and HIGHER by as much per key above it: the strongest scores of
    every row sit only on keys it must not see, next to V rows of up to 33024. One admitted key gives exp2(>= 268) = inf; a dropped
    diagonal gives the row below. The row must return V[past + i] exactly."""
    pb, want = _cached(("ramp", dtype, hd), lambda: _ramp_problem(dtype, hd))
    got = _launch(dev, pb, sel, True)
    for (ql, past), g, w in zip(pb.seqs, got, want):
        assert torch.isfinite(g.float()).all(), (ql, past)
        rows = (_bits(g) != w).flatten(1).any(dim=1).nonzero().flatten().tolist()
        assert not rows, f"(q_len {ql}, past {past}): {len(rows)} rows wrong, first {rows[:6]}"


# ---- c. random data inside prefill_bound, element by element ---------------------------------------------------------------------------
SELS = {64: [None], 128: [1, 2, 3, PERSIST8, 5, 0]}
SEL_NAME = {None: "hd64", 1: "sel1", 2: "sel2", 3: "sel3", PERSIST8: "sel4x8", 5: "sel5", 0: "sel0"}


def _random_case(dev, dtype, hd, heads, causal, lens, pasts, seed, rope=True, data=None, amp=(1.0, 1.0, 1.0), subset=None):
    """The engine's way: vt_kv_tiles (with rope) writes the pages from a fused QKV buffer (wide rows, column blocks k | v | q, the
    sequences in a permuted row order, positions offset per sequence) and rotates q in place; its pages are checked bit for bit against
    pack_pages(rope_ref(...)) and its q against rope_ref. Then every kernel of the head_dim, each output element against the fp64
    reference within prefill_bound (both computed on the device from the host restatement's operands). data: [sum kv][3][heads][hd]
    host values instead of N(0, amp^2) draws. subset(si) -> [(head indices, row indices)] to check instead of every element.
    Returns {kernel name: largest error / bound}."""
    from vitron_amd import ops
    D, scale, store = heads * hd, 1.0 / math.sqrt(hd), R.FMT[dtype]
    kv = [p + q for p, q in zip(pasts, lens)]
    ntl = [(n + 63) // 64 for n in kv]
    rng = np.random.default_rng(seed)
    npages = sum(ntl) + 3
    it = iter(rng.permutation(npages).tolist())
    gen = torch.Generator(device=dev).manual_seed(seed)
    tot, gap = sum(kv), 2
    if data is None:
        data = torch.randn((tot, 3, heads, hd), generator=gen, device=dev) * torch.tensor(amp, device=dev).view(1, 3, 1, 1)
    data = data.to(dev).to(dtype)
    row0, r = {}, gap
    for si in rng.permutation(len(lens)).tolist():
        row0[si] = r
        r += kv[si] + gap
    rows, ld = r, 3 * D + 192
    cols = dict(k=0, v=D + 64, q=2 * D + 128)
    x = torch.full((rows, ld), NAN, dtype=dtype, device=dev)
    pos = np.zeros(rows, np.int64)
    table, desc_kv, desc, src0 = [], [], [], np.cumsum([0] + kv[:-1])
    for si in range(len(lens)):
        sl = slice(row0[si], row0[si] + kv[si])
        for c, name in enumerate("qkv"):
            x[sl, cols[name]:cols[name] + D] = data[src0[si]:src0[si] + kv[si], c].reshape(kv[si], D)
        pos[sl] = np.arange(kv[si]) + 5 * si
        desc_kv.append((row0[si], kv[si], kv[si], len(table)))
        desc.append((row0[si] + pasts[si], lens[si], kv[si], len(table)))
        table += [next(it) for _ in range(ntl[si])]
    kp = torch.full((npages * heads * 64 * hd,), NAN, dtype=dtype, device=dev)
    vp = torch.full((npages * heads * 64 * hd,), NAN, dtype=torch.float16, device=dev)
    table_t = torch.tensor(table, dtype=torch.int32, device=dev)
    cos, sin = _rope_tables(hd)
    cs = (cos.to(dev), sin.to(dev), torch.as_tensor(pos, dtype=torch.int32, device=dev)) if rope else (None, None, None)
    ops.kv_tiles(x, cols["q"], cols["k"], cols["v"], kp, vp, table_t, ops.seq_desc_tensor(desc_kv, dev), max(ntl), heads, hd, *cs)
    torch.cuda.synchronize()
    # host: the operands the kernels see
    dh, xq = data.cpu(), x[:, cols["q"]:cols["q"] + D].cpu()
    want_k, want_v = torch.full((kp.numel(),), NAN, dtype=dtype), torch.full((kp.numel(),), NAN, dtype=torch.float16)
    ops_h = []
    for si in range(len(lens)):
        d = dh[src0[si]:src0[si] + kv[si]]
        p_si = np.arange(kv[si]) + 5 * si
        k_rot = R.rope_ref(d[:, 1], cos, sin, p_si, dtype) if rope else d[:, 1]
        q_rot = R.rope_ref(d[pasts[si]:, 0], cos, sin, p_si[pasts[si]:], dtype) if rope else d[pasts[si]:, 0]
        toff = desc[si][3]
        R.pack_pages(k_rot, d[:, 2], table[toff:toff + ntl[si]], heads, hd, dtype, out=(want_k, want_v))
        assert torch.equal(_bits(xq[desc[si][0]:desc[si][0] + lens[si]].reshape(lens[si], heads, hd)), _bits(q_rot)), "q after vt_kv_tiles"
        ops_h.append((q_rot, k_rot, R.to_f16_page(d[:, 2])))
    assert torch.equal(_bits(kp.cpu()), _bits(want_k)) and torch.equal(_bits(vp.cpu()), _bits(want_v)), "vt_kv_tiles pages"
    owned = torch.zeros(rows, dtype=torch.bool)
    for r0, ql, _, _ in desc:
        owned[r0:r0 + ql] = True
    # reference and bound, on the device
    R.W_ELEMS, keep = 1 << 26, R.W_ELEMS
    try:
        checks = []
        for si, (q_rot, k_rot, v16) in enumerate(ops_h):
            qd, kd, vd = q_rot.to(dev).double(), k_rot.to(dev).double(), v16.to(dev).double()
            parts = subset(si) if subset else [(np.arange(heads), np.arange(lens[si]))]
            for hs, rs in parts:
                hs, rs = torch.as_tensor(hs, device=dev), torch.as_tensor(rs, device=dev)
                ref, bound = R.prefill_ref_and_bound(qd[rs][:, hs], kd[:, hs], vd[:, hs], scale, pasts[si], causal, store, rows=rs)
                checks.append((si, hs, rs, ref, bound))
    finally:
        R.W_ELEMS = keep
    desc_t = ops.seq_desc_tensor(desc, dev)
    report = {}
    for sel in SELS[hd]:
        if sel is not None:
            ops.flash_attn_select(sel)
        obuf = torch.full((rows, D + 8), NAN, dtype=dtype, device=dev)
        ops.flash_attn(x[:, cols["q"]:cols["q"] + D], kp, vp, table_t, desc_t, max(lens), heads, hd, causal, scale, out=obuf[:, :D])
        torch.cuda.synchronize()
        assert torch.isnan(obuf[~owned.to(dev)].float()).all() and torch.isnan(obuf[:, D:].float()).all(), "wrote outside its rows / columns"
        worst = 0.0
        for si, hs, rs, ref, bound in checks:
            got = obuf[desc[si][0]:desc[si][0] + lens[si], :D].reshape(lens[si], heads, hd)[rs][:, hs].double()
            assert torch.isfinite(got).all(), (SEL_NAME[sel], lens[si], pasts[si])
            ratio = (got - ref).abs() / bound
            if not bool((ratio <= 1).all()):
                i, h, dd = (ratio == ratio.max()).nonzero()[0].tolist()
                raise AssertionError(f"{SEL_NAME[sel]} {store} (q_len {lens[si]}, past {pasts[si]}): error / bound up to {float(ratio.max()):.3g} at row "
                                     f"{int(rs[i])} head {int(hs[h])} d {dd} ({int((ratio > 1).sum())} of {ratio.numel()} elements outside)")
            worst = max(worst, float(ratio.max()))
        report[SEL_NAME[sel]] = worst
    return report


def _say(what, dtype, hd, report):
    print(f"\n[prefill attn bound] {what} {R.FMT[dtype]} hd {hd}: highest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))


# the ragged multi-sequence and chunked cases of tests/test_gpu_attn_w4.py::CASES, and a 40-row chunk behind 4000 keys
RAGGED = [(True, [700, 300, 64, 1], [0, 0, 0, 0]), (False, [577, 130], [0, 0]), (True, [257, 40], [100, 1000]), (True, [2304], [0]),
          (True, [256, 255, 257], [0, 31, 64]), (False, [64], [0]), (True, [1], [0]), (True, [40], [4000])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_random_data_within_the_fp64_bound_ragged_and_chunked(dev, dtype, hd):
    from tests.test_gpu_attn_w4 import CASES
    assert all(c in RAGGED for c in CASES)
    total = {}
    for n, (causal, lens, pasts) in enumerate(RAGGED):
        rep = _random_case(dev, dtype, hd, 3, causal, lens, pasts, 600 + n)
        total = {k: max(v, total.get(k, 0.0)) for k, v in rep.items()}
    _say("ragged / chunked", dtype, hd, total)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [577, 257])
def test_random_data_within_the_fp64_bound_tower_shapes(dev, dtype, L):
    """both towers' spatial attention: 8 frames of L tokens, 16 heads of 64, non-causal (no rope in the towers)"""
    _say(f"towers [{L}] * 8", dtype, 64, _random_case(dev, dtype, 64, 16, False, [L] * 8, [0] * 8, 700 + L, rope=False))


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_data_within_the_fp64_bound_at_s5120(dev, dtype):
    """The headline prefill: one causal sequence of 5120 rows on 32 heads. The fp64 reference of all of it is too heavy, so a subset fixed
    here, before any run: for heads 0, 9, 22, 31 every row of 0 .. 63, of 224 .. 287 (a 256-row block seam of the w4 kernel, a 128-row
    seam of the other) and of the last 64, plus 256 seeded rows on all heads. (The uniform probes check every row of S = 5120 exactly.)"""
    S = 5120
    rows_a = np.concatenate([np.arange(0, 64), np.arange(224, 288), np.arange(S - 64, S)])
    rows_b = np.sort(np.random.default_rng(5120).choice(S, 256, replace=False))
    rep = _random_case(dev, dtype, 128, 32, True, [S], [0], 800, subset=lambda si: [(np.array([0, 9, 22, 31]), rows_a), (np.arange(32), rows_b)])
    _say("S = 5120 x 32 heads (subset)", dtype, 128, rep)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("variant", ["wide", "ascending"])
def test_score_range_edges_within_the_fp64_bound(dev, dtype, hd, variant):
    """The score-range cases of tests/test_gpu_attn_w4.py::test_w4_kernel_score_range_edges, per element: rows whose scores span more than
    60 (q, k scaled by 3: the fp16 weights' subnormal tail) and rows whose running maximum moves at every sub tile (keys ascending in
    score: the deferred rescale and the w4 kernel's pending O rescale between sub-iterations). No rope: it would undo the ordering."""
    heads, L = 2, 700
    D = heads * hd
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn((L, 3 * D), generator=g)
    if variant == "wide":
        qkv[:, :2 * D] *= 3.0
    else:
        u = torch.sign(torch.randn((1, D), generator=g))
        qkv[:, D:2 * D] = torch.linspace(-3.0, 3.0, L).view(L, 1) * u + 0.05 * qkv[:, D:2 * D]
        qkv[:, :D] = (1.0 + torch.rand((L, 1), generator=g)) * u + 0.05 * qkv[:, :D]
    data = qkv.view(L, 3, heads, hd)
    s = torch.einsum("qhd,khd->hqk", data[:, 0].to(dtype).double(), data[:, 1].to(dtype).double()) / math.sqrt(hd)
    assert float(s.max() - s.min()) > 60.0
    _say(f"edges: {variant}", dtype, hd, _random_case(dev, dtype, hd, heads, True, [L], [0], 900, rope=False, data=data))


@pytest.mark.parametrize("hd", [64, 128])
def test_bf16_values_beyond_fp16_range_within_the_fp64_bound(dev, hd):
    """bf16 V of N(0, 30000^2): about 3 % of the entries exceed 65504 and land in the fp16 V^T pages as +-65504 (the reference takes the
    pages' values); outputs stay finite and inside the bound."""
    rep = _random_case(dev, torch.bfloat16, hd, 3, True, [300, 70], [0, 200], 950, amp=(1.0, 1.0, 30000.0))
    _say("V beyond fp16's range", torch.bfloat16, hd, rep)


# ---- d. contract edges -------------------------------------------------------------------------------------------------------------
def _random_problem(dtype, hd, heads, seqs, seed):
    g = torch.Generator().manual_seed(seed)
    draw = lambda n: torch.randn((n, heads, hd), generator=g)
    data = [(draw(q), draw(q + p), draw(q + p)) for q, p in seqs]
    return Problem(seqs, heads, hd, dtype, lambda si: data[si][0], lambda si, j: data[si][1][j], lambda si, j: data[si][2][j], seed)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,sel", KAXIS)
def test_repeated_launches_are_bit_identical(dev, dtype, hd, sel):
    """three launches of a ragged causal problem (and one non-causal pair) give the same bits everywhere, NaN rows and columns included"""
    pb = _cached(("repeat", dtype, hd), lambda: _random_problem(dtype, hd, 8, [(700, 0), (300, 100), (64, 0), (1, 0), (257, 1000)], 960 + hd))
    first = _launch(dev, pb, sel, True, raw=True)
    assert all(torch.equal(_launch(dev, pb, sel, True, raw=True), first) for _ in range(2))
    assert torch.equal(_launch(dev, pb, sel, False, raw=True), _launch(dev, pb, sel, False, raw=True))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,forced", [(2304, 2), (1088, 1), (1024, 1)])
def test_selector_0_is_the_forced_selector_it_documents(dev, dtype, S, forced):
    """vt_flash_attn_select(0) at head_dim 128: the one-wave-per-SIMD kernel (selector 2) once heads x sequences x 256-row blocks fill 256
    workgroups and max_q_len >= 1024 (32 heads x 2304 rows: 288), the two-waves-per-SIMD kernel (selector 1) below that (32 x 1088 rows:
    160; 8 heads x 4 sequences of 1024: 128)."""
    heads, seqs = (32, [(S, 0)]) if S != 1024 else (8, [(1024, 0)] * 4)
    pb = _random_problem(dtype, 128, heads, seqs, 970 + S)
    assert torch.equal(_launch(dev, pb, 0, True, raw=True), _launch(dev, pb, forced, True, raw=True))
