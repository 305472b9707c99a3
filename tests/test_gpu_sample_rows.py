"""vt_sample_rows (ops.sample_rows): one token per row with per-row parameters. Pinned EXACTLY against the launch-uniform kernels it shares
its bodies with (vt_sample_top_p: ids and keep-set sizes; vt_argmax), against itself on host-penalised logits (the repetition penalty, bit
for bit), and per row against the fp64 log_softmax inside the bound tests/sample_ref.py derives. 8 rows; V = 32000 (rows in registers),
32003 (odd stride: the ragged tail, the streaming form) and 40000 (the streaming form, aligned)."""
import numpy as np
import pytest
import torch

from tests import sample_ref as R

pytestmark = pytest.mark.gpu
ROWS = 8
VS = (32000, 32003, 40000)
TKP = ((0.7, 0, 0.9), (1.0, 0, 0.5), (0.2, 0, 0.95), (1.3, 0, 1.0), (1.0, 7, 1.0), (0.3, 50, 1.0), (1.0, 50, 0.6))   # from tests/test_gpu_kernels.py


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_cache = {}


def _logits(V):
    """fp32 [8][V] on the host, computed once per V and never modified: both signs, a zero, ties, one dominant and one near-uniform row"""
    if V not in _cache:
        g = torch.Generator().manual_seed(1000 + V)
        x = torch.randn((ROWS, V), generator=g) * 3.0
        x[0, 123] = 40.0                                   # dominant: logprob near 0, keep-set of one
        x[1] = torch.randn((V,), generator=g) * 1e-3       # near uniform
        x[2, 777] = x[2, V - 1] = 50.0                     # tie for the maximum: the first index wins
        x[2, 100] = 20.0
        x[3] = x[3].round()                                # ties everywhere
        x[:, 5] = 0.0
        x[4, 0], x[4, 31], x[4, 32], x[4, V - 1] = 13.0, -13.0, 14.0, 15.0      # the mask's word boundaries carry the row's extremes
        _cache[V] = x
    return _cache[V]


def _pack(rows, dev):
    from vitron_amd.sampling import pack_sample_rows
    return pack_sample_rows(rows, dev)


def _row(T=0.0, k=0, p=1.0, pen=1.0, seed=0, counter=0, stream=0, hist=None, hlen=None):
    return (T, k, p, pen, seed, counter, stream, 0 if hist is None else hist.data_ptr(), 0 if hist is None else (hist.numel() if hlen is None else hlen))


@pytest.mark.parametrize("V", VS)
def test_equals_the_launch_uniform_kernels(dev, V):
    from vitron_amd import ops
    x = _logits(V)
    ld = x.to(dev)
    assert (ld.stride(0) % 4 == 0) == (V % 4 == 0)
    am = ops.argmax(ld)
    assert am.cpu().tolist() == x.argmax(-1).tolist() and int(am[2]) == 777
    seed, s = 5, 3
    for T, k, p in TKP:                                   # (T, k, p, seed, counter = s, stream = r) is sample_top_p(seed, step = s) at row r
        want, want_kept = ops.sample_top_p(ld, T, p, seed, s, return_kept=True, top_k=k)
        got, kept = ops.sample_rows(ld, _pack([_row(T, k, p, 1.0, seed, s, r) for r in range(ROWS)], dev), return_kept=True)
        assert torch.equal(got, want) and torch.equal(kept, want_kept), (T, k, p, got.tolist(), want.tolist(), kept.tolist(), want_kept.tolist())
    assert int(want_kept.max()) > 1
    got, kept = ops.sample_rows(ld, _pack([_row() for _ in range(ROWS)], dev), return_kept=True)        # all greedy
    assert torch.equal(got, am) and kept.cpu().tolist() == [1] * ROWS
    # a mixed batch: every row its own parameters, rows 1, 4 and 6 greedy; each row's answer is the launch-uniform kernel's at that row
    per_row = [TKP[r % len(TKP)] + (11 + r, 2 * r + 1) for r in range(ROWS)]
    greedy = (1, 4, 6)
    rows = [_row() if r in greedy else _row(*per_row[r][:3], 1.0, per_row[r][3], per_row[r][4], r) for r in range(ROWS)]
    got, kept = ops.sample_rows(ld, _pack(rows, dev), return_kept=True)
    for r in range(ROWS):
        if r in greedy:
            assert int(got[r]) == int(am[r]) and int(kept[r]) == 1
        else:
            T, k, p, sd, st = per_row[r]
            w, wk = ops.sample_top_p(ld, T, p, sd, st, return_kept=True, top_k=k)
            assert int(got[r]) == int(w[r]) and int(kept[r]) == int(wk[r]), (r, per_row[r])
    # the draw belongs to (seed, counter, stream), not to the row's place in the batch: permuted rows give permuted outputs
    perm = [3, 7, 0, 5, 1, 6, 2, 4]
    got_p, kept_p = ops.sample_rows(ld[perm].contiguous(), _pack([rows[i] for i in perm], dev), return_kept=True)
    assert got_p.tolist() == got[perm].tolist() and kept_p.tolist() == kept[perm].tolist()
    uni = [_row(1.0, 0, 1.0, 1.0, 9, 4, r) for r in range(ROWS)]                                        # sampled rows only, broad keep-sets
    a = ops.sample_rows(ld, _pack(uni, dev))
    b = ops.sample_rows(ld[perm].contiguous(), _pack([uni[i] for i in perm], dev))
    assert b.tolist() == a[perm].tolist() and a.tolist() == ops.sample_top_p(ld, 1.0, 1.0, 9, 4).tolist()


def _order_probe(p, T):
    """fp32 x > 0 for which penalising BEFORE the temperature and after it round differently: (x / p) * (1 / T) != (x * (1 / T)) / p"""
    it = np.float32(1.0) / np.float32(T)
    g = np.random.default_rng(17)
    for x in (g.random(4096, dtype=np.float32) * 8 + 1):
        if np.float32(np.float32(x / np.float32(p)) * it) != np.float32(np.float32(x * it) / np.float32(p)):
            return np.float32(x)
    raise AssertionError("no probe value found")


@pytest.mark.parametrize("V", VS)
def test_penalty_equals_host_penalised_logits(dev, V):
    """sample_rows(logits, penalty p, history) == sample_rows(host-penalised logits, penalty 1) in ids and keep-set sizes: greedy rows
    (0-3) and sampled rows (4-7); histories of 0, 1 and 1500 ids (the 1024-stride fill loop wraps) with duplicates, the ids 0, 31, 32 and
    V - 1, negative sentinels and ids >= V. Row 7 is a probe of the ORDER (penalty, then temperature): its two largest logits tie exactly
    only when the penalised value is the one that gets scaled, and top_k = 1 counts the tie."""
    from vitron_amd import ops
    g = torch.Generator().manual_seed(V)
    special = [0, 31, 32, V - 1, 0, 31, -200, -300, V, V + 7, 2 ** 31 - 1, 5, 777, 123]
    rnd = torch.randint(2, V, (1500 - len(special),), generator=g).tolist()
    rnd = [i + 1 if i == 1 else i for i in rnd]                                  # id 1 stays out: the probe's unpenalised twin
    long_hist = special + rnd[:700] + rnd[:100] + rnd[700:1500 - len(special) - 100]
    assert len(long_hist) == 1500
    for pen in (1.3, 0.8):
        x = _logits(V).clone()
        px = _order_probe(pen, 0.7)
        x[7] = -5.0
        x[7, 0], x[7, 1] = float(px), float(np.float32(px / np.float32(pen)))
        ld = x.to(dev)
        for hist in ([], [0], long_hist):
            h = torch.tensor(hist + [0], dtype=torch.int32, device=dev)          # (+ a spare so the empty history still has a buffer)
            def rows(p, hd):
                return [_row(0.0, 0, 1.0, p, 0, 0, r, hd, len(hist) if hd is not None else None) for r in range(4)] + \
                       [_row(0.7, 0, 0.9, p, 3, 1, 4, hd, len(hist) if hd is not None else None),
                        _row(1.0, 50, 1.0, p, 3, 2, 5, hd, len(hist) if hd is not None else None),
                        _row(1.3, 7, 0.8, p, 3, 3, 6, hd, len(hist) if hd is not None else None),
                        _row(0.7, 1, 1.0, p, 3, 4, 7, hd, len(hist) if hd is not None else None)]
            got, kept = ops.sample_rows(ld, _pack(rows(pen, h), dev), return_kept=True)
            host = torch.from_numpy(R.repetition_penalty(x.numpy(), hist, pen))
            want, want_kept = ops.sample_rows(host.to(dev), _pack(rows(1.0, None), dev), return_kept=True)
            assert got.tolist() == want.tolist() and kept.tolist() == want_kept.tolist(), (pen, len(hist), got.tolist(), want.tolist(),
                                                                                          kept.tolist(), want_kept.tolist())
            assert got.tolist()[:4] == host.argmax(-1).tolist()[:4]              # greedy rows: the first maximum of the penalised row
            if hist:
                assert int(kept[7]) == 2 and int(got[7]) in (0, 1)               # the probe's tie
            else:
                assert int(kept[7]) == 1 and int(got[7]) == (0 if pen > 1 else 1)
            assert int(got[2]) == 777                                            # 777 and its twin at V - 1 are penalised together or not at all


@pytest.mark.parametrize("V", VS)
def test_logprob_inside_the_fp64_bound(dev, V, record_property):
    """logprob[r] = log_softmax(RAW row)[id] -- before penalty and temperature -- inside the bound tests/sample_ref.py derives from the
    operation counts; greedy and sampled rows, with and without a penalty whose history holds the row's best tokens."""
    from vitron_amd import ops
    x = _logits(V)
    ld = x.to(dev)
    ref = R.logprob_ref(x.numpy())
    top = x.topk(3, -1).indices.to(torch.int32).to(dev)                           # every row's history: its own three best tokens
    worst = 0.0
    for pen in (1.0, 1.3):
        rows = [_row(0.0 if r % 2 == 0 else 0.9, 0, 0.95, pen, 21, 6, r, top[r]) for r in range(ROWS)]
        ids, lp = ops.sample_rows(ld, _pack(rows, dev), return_logprob=True)
        ids2, kept, lp2 = ops.sample_rows(ld, _pack(rows, dev), return_kept=True, return_logprob=True)
        assert torch.equal(ids, ops.sample_rows(ld, _pack(rows, dev))) and torch.equal(ids, ids2) and torch.equal(lp, lp2)
        idl = ids.cpu().long().numpy()
        bound = R.logprob_bound(x.numpy(), idl)
        err = np.abs(lp.cpu().double().numpy() - ref[np.arange(ROWS), idl])
        ratio = err / bound
        print(f"V={V} penalty={pen} logprob err/bound per row: {[f'{v:.3f}' for v in ratio]} (bound {bound.min():.2e}..{bound.max():.2e})")
        assert (ratio <= 1.0).all(), (pen, err.tolist(), bound.tolist())
        worst = max(worst, float(ratio.max()))
        assert int(ids[0]) == 123 and abs(float(lp[0])) < 1e-6                    # the dominant row
        assert abs(float(lp[1]) + np.log(V)) < 0.02                               # the near-uniform row
        assert int(ids[2]) == 777                                                 # penalised or not, with its twin at V - 1: still the first maximum
        if pen != 1.0:            # row 4's three best tokens are pushed below the rest: another token wins, its logprob is still the raw row's
            assert int(ids[4]) not in top[4].tolist() and int(ids[4]) == int(R.repetition_penalty(x[4].numpy(), top[4].tolist(), pen).argmax())
    record_property("logprob_err_over_bound", worst)


@pytest.mark.parametrize("V,ldl", ((1000, 1000), (1001, 1001)))          # the register form; the streaming form by misalignment
def test_every_entry_point_without_its_arrays_is_vt_sample_rows(dev, V, ldl):
    """The library picks the kernel by the highest array it is given, whichever entry point carries it. Four rows (greedy; sampled;
    sampled with a 5-id history under a penalty of 1.3; greedy), once with ids alone and once with kept_count and logprob, through raw
    ctypes: each wider entry point returns the bits of vt_sample_rows with every added array NULL, and with neutral arrays -- all-ones
    masks, all-zero [V][2] adjustments, all-inactive vt_trunc_row, vt_wm_row without a cell -- each together with the neutral arrays
    below it. vt_sample_rows_wm with an array keeps its refusal in the streaming form.
    Left out, asserted elsewhere in both forms: vt_sample_rows_allow with allow == NULL (test_gpu_sample_allow.py's
    test_allow_none_is_sample_rows); an all-inactive trunc array or a cell-less wm array ALONE, behind NULL arrays
    (test_gpu_sample_trunc.py's and test_gpu_sample_wm.py's bit-equality tests, through ops.sample_rows)."""
    from vitron_amd import _lib
    from vitron_amd.sampling import pack_trunc_rows
    from vitron_amd.watermark import pack_wm_rows
    lib = _lib.load()
    n = 4
    buf = torch.zeros((n, ldl), dtype=torch.float32)
    buf[:, :V] = _logits(V)[:n]
    x = buf.to(dev)[:, :V]
    hist = torch.tensor([0, 31, 32, 123, V - 1], dtype=torch.int32, device=dev)
    pr = _pack([_row(), _row(0.7, 0, 0.9, 1.0, 5, 3, 1), _row(0.7, 20, 0.9, 1.3, 5, 3, 2, hist), _row()], dev)
    ones = torch.full(((V + 31) // 32,), -1, dtype=torch.int32, device=dev)
    zeros = torch.zeros((V, 2), dtype=torch.float32, device=dev)
    allow = torch.tensor([ones.data_ptr()] * n, dtype=torch.int64, device=dev)
    adjust = torch.tensor([zeros.data_ptr()] * n, dtype=torch.int64, device=dev)
    trunc, wm = pack_trunc_rows([None] * n, dev), pack_wm_rows([None] * n, dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(name, *arrays, outputs):
        out = torch.full((n,), -7, dtype=torch.int32, device=dev)
        kept = torch.full((n,), -7, dtype=torch.int32, device=dev) if outputs else None
        lp = torch.full((n,), 7.0, dtype=torch.float32, device=dev) if outputs else None
        st = getattr(lib, name)(x.data_ptr(), n, V, ldl, pr.data_ptr(), *(None if a is None else a.data_ptr() for a in arrays), out.data_ptr(),
                                None if kept is None else kept.data_ptr(), None if lp is None else lp.data_ptr(), stream)
        assert st == 0, (name, _lib.last_error(lib))
        return [out.cpu().tolist()] + ([kept.cpu().tolist(), lp.cpu().numpy().view(np.uint32).tolist()] if outputs else [])

    wide = (("vt_sample_rows_allow", (allow,)), ("vt_sample_rows_adj", (allow, adjust)), ("vt_sample_rows_trunc", (allow, adjust, trunc)),
            ("vt_sample_rows_wm", (allow, adjust, trunc, wm)))
    for outputs in (False, True):
        base = call("vt_sample_rows", outputs=outputs)
        assert all(0 <= i < V for i in base[0]) and [base[0][0], base[0][3]] == _logits(V)[[0, 3]].argmax(-1).tolist(), base
        for name, neutral in wide:
            if name != "vt_sample_rows_allow":
                assert call(name, *[None] * len(neutral), outputs=outputs) == base, (name, "NULL arrays", outputs)
            if name == "vt_sample_rows_wm" and ldl % 4:
                continue                                                         # refused below
            assert call(name, *neutral, outputs=outputs) == base, (name, "neutral arrays", outputs)
    if ldl % 4:
        out = torch.empty((n,), dtype=torch.int32, device=dev)
        st = lib.vt_sample_rows_wm(x.data_ptr(), n, V, ldl, pr.data_ptr(), None, None, None, wm.data_ptr(), out.data_ptr(), None, None, stream)
        assert st < 0 and (f"vt_sample_rows_wm: V={V} ldl={ldl}: the watermark runs in the register form only (V <= 32768, ldl % 4 == 0, "
                           "logits 16-byte aligned)") in _lib.last_error(lib), (st, _lib.last_error(lib))


def test_bad_calls_return_errors(dev):
    from vitron_amd import _lib, ops
    lib = _lib.load()
    ld = torch.zeros((2, 64), device=dev)
    pr = _pack([_row(), _row()], dev)
    out = torch.empty((2,), dtype=torch.int32, device=dev)
    L, Pp, Op = ld.data_ptr(), pr.data_ptr(), out.data_ptr()

    def bad(status, needle):
        msg = _lib.last_error(lib)
        assert status < 0 and needle in msg, (status, msg)

    bad(lib.vt_sample_rows(None, 2, 64, 64, Pp, Op, None, None, None), "null")
    bad(lib.vt_sample_rows(L, 2, 64, 64, None, Op, None, None, None), "null")
    bad(lib.vt_sample_rows(L, 2, 64, 64, Pp, None, None, None, None), "null")
    bad(lib.vt_sample_rows(L, 0, 64, 64, Pp, Op, None, None, None), "rows=0")
    bad(lib.vt_sample_rows(L, 2, 0, 64, Pp, Op, None, None, None), "V=0")
    bad(lib.vt_sample_rows(L, 2, 64, 32, Pp, Op, None, None, None), "ldl")
    bad(lib.vt_sample_rows(L, 2, 262145, 262145, Pp, Op, None, None, None), "beyond the history mask")      # refused before any launch
    bad(lib.vt_sample_rows(L, 2, 300000, 300000, Pp, Op, None, None, None), "beyond the history mask")
    bad(lib.vt_sample_rows(L, 2, 64, 64, Pp + 4, Op, None, None, None), "aligned")
    with pytest.raises(_lib.VitronHipError):
        ops.sample_rows(ld, pr[:1])
    with pytest.raises(_lib.VitronHipError):
        ops.sample_rows(ld, pr.cpu())
    with pytest.raises(_lib.VitronHipError):
        ops.sample_rows(torch.zeros((0, 64), device=dev), pr[:0])
    torch.cuda.synchronize()


def test_the_kernel_is_total(dev):
    """Field values Python would have refused, written straight into the struct: the launch completes and every id is inside the row (or -1
    where NaNs leave nothing to choose): greedy for a temperature that is not > 0, top_k < 0 off, a NULL history or a negative length empty."""
    from vitron_amd import ops
    from vitron_amd.sampling import ROW_DTYPE
    for V in (32000, 32003):
        x = _logits(V)
        ld = x.to(dev)
        hist = torch.tensor([0, 5, V - 1, V, -1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=dev)
        arr = np.zeros((ROWS,), dtype=ROW_DTYPE)
        arr["temperature"] = [-1.0, np.nan, 1.0, 1.0, 1.0, 0.0, 1.0, np.inf]
        arr["top_p"] = [1.0, 1.0, -1.0, np.nan, 0.0, 1.0, 0.5, 0.5]
        arr["top_k"] = [0, 0, -5, 2 ** 31 - 1, -2 ** 31, 3, 1, 1]
        arr["repetition_penalty"] = [1.0, 1.0, 1.0, 1.3, 1.3, -1.0, 1.3, 1.3]
        arr["history"] = [0, 0, 0, 0, hist.data_ptr(), hist.data_ptr(), hist.data_ptr(), hist.data_ptr()]
        arr["history_len"] = [0, 0, 0, 100, -7, 7, 7, 7]                          # row 3: a length without a buffer
        arr["stream"] = 2 ** 32 - 1
        arr["seed"] = 2 ** 64 - 1
        arr["counter"] = 2 ** 64 - 1
        pr = torch.from_numpy(arr.view(np.uint8).reshape(ROWS, 48)).to(dev)
        ids, kept, lp = ops.sample_rows(ld, pr, return_kept=True, return_logprob=True)
        torch.cuda.synchronize()
        ids = ids.cpu().tolist()
        assert all(-1 <= i < V for i in ids), ids
        am = x.argmax(-1).tolist()
        assert ids[0] == am[0] and ids[1] == am[1] and ids[6] == am[6]           # not > 0: greedy; top_k = 1: the maximum (0 / 1.3 stays 0)
