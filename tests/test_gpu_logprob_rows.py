"""vt_logprob_rows (ops.logprob_rows) against tests/logprob_ref.py: top_ids and target_rank EXACTLY, top_lp, target_lp and
lse inside the fp64 bound. rows in {1, 3, 8}; V in {7 (V < n_top), 512 (the tiny model), 1000, 32000 and 32768 (the register form and its
edge), 32003 (no 16-byte rows: the streaming form with single loads), 40000 (the streaming form with 16-byte loads)}; n_top in {0, 1, 5,
20}; a row stride > V and a base pointer offset by one float once each. Per V one 8-row matrix, built and scored on the host once:
  row 0  seeded normal logits (spread 3) with one dominant token      row 4  a run of -inf
  row 1  one value tied across slots, threads and waves               row 5  one NaN (its own index is the target)
  row 2  the maximum at index 0                                       row 6  all equal (the target V - 1 has rank V)
  row 3  the maximum at V - 1                                         row 7  rounded normals: ties everywhere
The 1-row launch takes row 1, the 3-row launch rows 4 - 6, the 8-row launch everything. Further: agreement with vt_sample_rows' logprob
on the sampler's picks inside the sum of the two bounds, the logits bit-unchanged, the argument refusals."""
import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import sample_ref as R

pytestmark = pytest.mark.gpu
VS = (7, 512, 1000, 32000, 32003, 32768, 40000)
NTOPS = (0, 1, 5, 20)
PICK = {1: slice(1, 2), 3: slice(4, 7), 8: slice(0, 8)}


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_cache = {}


def _case(V):
    """(logits fp32 [8, V], targets int32 [8], reference dict) on the host, computed once per V and never modified"""
    if V in _cache:
        return _cache[V]
    g = torch.Generator().manual_seed(4000 + V)
    x = (torch.randn((8, V), generator=g) * 3.0).numpy().astype(np.float32)
    at = lambda i: min(int(i), V - 1)         # noqa: E731
    x[0, at(123)] = 25.0
    # row 1, register form: thread t owns the floats 4 (t + 1024 j) + k. Ties inside one thread's 16-byte load (1, 2), in its next slot
    # group (4096 + 1), in another lane (4 * 5 + 1), in another wave (4 * 64 + 2, 4 * 1000 + 3) and at the end of the row
    tie = sorted({at(i) for i in (1, 2, 21, 258, 4003, 4097, V - 1)})
    x[1, tie] = 11.5
    x[1, at(3)] = 12.0
    x[2, 0] = 30.0
    x[3, V - 1] = 30.0
    x[4, at(2):at(300)] = -np.inf
    nan_at = V // 2
    x[5, nan_at] = np.nan
    x[6] = 0.25
    x[7] = np.round(x[7])
    targets = np.array([LR.order(x[0])[min(3, V - 1)], tie[len(tie) // 2], 0, 0, at(2), nan_at, V - 1, -1], dtype=np.int32)
    top_ids, top_lp = LR.top(x, LR.MAX_TOP)
    ref = {"top_ids": top_ids, "top_lp": top_lp, "rank": LR.rank(x, targets), "tlp": LR.target_lp(x, targets), "lse": LR.lse64(x)}
    _cache[V] = (x, targets, ref)
    return _cache[V]


def _check(got, x, targets, ref, sel, n_top, reg, worst):
    """One launch's outputs against the reference rows `sel`; returns the highest error / bound ratio seen."""
    V = x.shape[1]
    chain = LR.lse_chain(V, reg)
    xs = x[sel]
    rank = got["rank"].cpu().numpy()
    assert rank.dtype == np.int32 and np.array_equal(rank, ref["rank"][sel]), (V, n_top, rank.tolist(), ref["rank"][sel].tolist())
    tlp = got["logprob"].cpu().numpy()
    worst = max(worst, LR.worst_ratio(tlp, ref["tlp"][sel], LR.logprob_bound(xs, ref["tlp"][sel], chain)))
    lse = got["lse"].cpu().numpy()
    worst = max(worst, LR.worst_ratio(lse, ref["lse"][sel], LR.lse_bound(xs, chain)))
    if n_top:
        ids = got["top_ids"].cpu().numpy()
        assert ids.shape == (xs.shape[0], n_top) and np.array_equal(ids, ref["top_ids"][sel, :n_top]), (V, n_top)
        want = ref["top_lp"][sel, :n_top]
        worst = max(worst, LR.worst_ratio(got["top_logprobs"].cpu().numpy(), want, LR.logprob_bound(xs, want, chain)))
    else:
        assert "top_ids" not in got and "top_logprobs" not in got
    return worst


@pytest.mark.parametrize("V", VS)
def test_equals_the_host_reference(dev, V, record_property):
    from vitron_amd import ops
    x, targets, ref = _case(V)
    worst = 0.0
    for rows, sel in PICK.items():
        ld = torch.from_numpy(x[sel].copy()).to(dev)
        before = ld.clone()
        tg = torch.from_numpy(targets[sel].copy()).to(dev)
        reg = LR.register_form(V, ld.stride(0), ld.data_ptr() % 16)
        assert reg == (V <= 32768 and V % 4 == 0)
        for n_top in NTOPS:
            got = ops.logprob_rows(ld, tg, n_top, return_rank=True, return_lse=True)
            worst = _check(got, x, targets, ref, sel, n_top, reg, worst)
        assert torch.equal(ld.view(torch.int32), before.view(torch.int32))          # the logits are only read
    # the hand-made rows say what they were made for
    assert ref["rank"][2] == 1 and ref["top_ids"][3, 0] == V - 1 and ref["rank"][6] == V and ref["rank"][7] == 0
    assert ref["rank"][5] == V and np.isnan(ref["tlp"][5]) and np.isnan(ref["top_lp"][5]).all() and ref["top_ids"][5, 0] >= 0
    if V < LR.MAX_TOP:
        assert (ref["top_ids"][0, V:] == -1).all() and np.isnan(ref["top_lp"][0, V:]).all() and ref["top_ids"][5, V - 1] == -1
    print(f"vt_logprob_rows V={V}: highest error / bound = {worst:.4f}")
    record_property("logprob_err_over_bound", worst)
    assert worst <= 1.0, worst


def test_row_stride_and_unaligned_base(dev):
    """ldl > V (1000 in rows of 1008 floats, and 7 in rows of 8 -- V < n_top in the register form) and a base offset by one float
    (32000: the streaming form with single loads), the same references."""
    from vitron_amd import ops
    for V, ldl, off in ((1000, 1008, 0), (7, 8, 0), (32000, 32000, 1)):
        x, targets, ref = _case(V)
        flat = torch.full((8 * ldl + off + 3,), 7.0, dtype=torch.float32, device=dev)
        ld = flat[off:off + 8 * ldl].view(8, ldl)[:, :V]
        ld.copy_(torch.from_numpy(x))
        before = flat.clone()
        reg = LR.register_form(V, ldl, ld.data_ptr() % 16)
        assert reg == (off == 0) and ld.stride(0) == ldl
        got = ops.logprob_rows(ld, torch.from_numpy(targets).to(dev), 20, return_rank=True, return_lse=True)
        assert _check(got, x, targets, ref, slice(0, 8), 20, reg, 0.0) <= 1.0
        assert torch.equal(flat.view(torch.int32), before.view(torch.int32))        # the padding columns too


def test_targets_none_out_of_range_and_out_buffers(dev):
    """No targets at all; targets outside [0, V) on both sides; out= views of [T, rows, N] step buffers are written in place."""
    from vitron_amd import ops
    V = 1000
    x, targets, ref = _case(V)
    ld = torch.from_numpy(x).to(dev)
    got = ops.logprob_rows(ld, None, 5)
    assert set(got) == {"top_ids", "top_logprobs", "packed"} and np.array_equal(got["top_ids"].cpu().numpy(), ref["top_ids"][:, :5])
    tg = torch.tensor([V, -1, 2 ** 31 - 1, -2 ** 31, V + 5, -7, V, V], dtype=torch.int32, device=dev)
    got = ops.logprob_rows(ld, tg, 0, return_rank=True)
    assert np.isnan(got["logprob"].cpu().numpy()).all() and (got["rank"].cpu().numpy() == 0).all()
    T = 3
    ids = torch.full((T, 8, 5), -9, dtype=torch.int32, device=dev)
    lps = torch.full((T, 8, 5), -9.0, dtype=torch.float32, device=dev)
    rk = torch.full((T, 8), -9, dtype=torch.int32, device=dev)
    tl = torch.full((T, 8), -9.0, dtype=torch.float32, device=dev)
    res = ops.logprob_rows(ld, torch.from_numpy(targets).to(dev), 5, out={"top_ids": ids[1], "top_logprobs": lps[1], "rank": rk[1], "logprob": tl[1]})
    assert res["top_ids"].data_ptr() == ids[1].data_ptr() and "packed" not in res
    assert np.array_equal(ids[1].cpu().numpy(), ref["top_ids"][:, :5]) and np.array_equal(rk[1].cpu().numpy(), ref["rank"])
    assert (ids[0] == -9).all() and (ids[2] == -9).all() and (rk[0] == -9).all() and (tl[2] == -9.0).all() and (lps[0] == -9.0).all()
    chain = LR.lse_chain(V, True)
    assert LR.worst_ratio(tl[1].cpu().numpy(), ref["tlp"], LR.logprob_bound(x, ref["tlp"], chain)) <= 1.0
    # the keys of out= say what is computed: no target log-probability here, and nothing is allocated
    res = ops.logprob_rows(ld, torch.from_numpy(targets).to(dev), 5, out={"top_ids": ids[2], "top_logprobs": lps[2], "rank": rk[2]})
    assert set(res) == {"top_ids", "top_logprobs", "rank"} and np.array_equal(rk[2].cpu().numpy(), ref["rank"])
    assert np.array_equal(ids[2].cpu().numpy(), ref["top_ids"][:, :5]) and (tl[2] == -9.0).all()
    assert LR.worst_ratio(lps[1].cpu().numpy(), ref["top_lp"][:, :5], LR.logprob_bound(x, ref["top_lp"][:, :5], chain)) <= 1.0


@pytest.mark.parametrize("V", (32000, 32003, 40000))
def test_agrees_with_the_samplers_logprob(dev, V):
    """target_lp at the ids vt_sample_rows picked (greedy and sampled rows) against the sampler's own logprob: inside the SUM of the two
    kernels' bounds (their summation orders differ, so bit equality is not asked for)."""
    from vitron_amd import ops
    from vitron_amd.sampling import pack_sample_rows
    g = torch.Generator().manual_seed(77 + V)
    x = torch.randn((4, V), generator=g) * 3.0
    ld = x.to(dev)
    pr = pack_sample_rows([(0.0, 0, 1.0, 1.0, 0, 0, 0, 0, 0), (1.0, 0, 1.0, 1.0, 5, 0, 1, 0, 0), (0.7, 50, 0.9, 1.0, 5, 1, 2, 0, 0),
                           (1.5, 0, 1.0, 1.0, 6, 2, 3, 0, 0)], dev)
    ids, lp_s = ops.sample_rows(ld, pr, return_logprob=True)
    got = ops.logprob_rows(ld, ids, 0, return_rank=True)
    ids_h = ids.cpu().numpy()
    want = LR.target_lp(x.numpy(), ids_h)
    reg = LR.register_form(V, ld.stride(0), ld.data_ptr() % 16)
    mine = LR.logprob_bound(x.numpy(), want, LR.lse_chain(V, reg))
    theirs = R.logprob_bound(x.numpy(), ids_h)
    diff = np.abs(got["logprob"].cpu().numpy().astype(np.float64) - lp_s.cpu().numpy().astype(np.float64))
    assert (diff <= mine + theirs).all(), (diff.tolist(), (mine + theirs).tolist())
    assert np.array_equal(got["rank"].cpu().numpy(), LR.rank(x.numpy(), ids_h)) and int(got["rank"][0]) == 1      # the greedy row


def test_bad_calls_return_errors(dev):
    from vitron_amd import _lib, ops
    lib = _lib.load()
    ld = torch.zeros((2, 64), device=dev)
    tg = torch.zeros((2,), dtype=torch.int32, device=dev)
    lp = torch.full((2,), -9.0, device=dev)
    rk = torch.full((2,), -9, dtype=torch.int32, device=dev)
    ti = torch.full((2, 20), -9, dtype=torch.int32, device=dev)
    tl = torch.full((2, 20), -9.0, device=dev)
    L, T, P, K, I, Q = (t.data_ptr() for t in (ld, tg, lp, rk, ti, tl))

    def bad(status, needle):
        msg = _lib.last_error(lib)
        assert status == -1 and needle in msg, (status, msg)               # VT_STATUS_ARG

    bad(lib.vt_logprob_rows(None, 2, 64, 64, T, 5, None, P, K, I, Q, None), "null")
    bad(lib.vt_logprob_rows(L, 0, 64, 64, T, 5, None, P, K, I, Q, None), "rows=0")
    bad(lib.vt_logprob_rows(L, 2, 0, 64, T, 5, None, P, K, I, Q, None), "V=0")
    bad(lib.vt_logprob_rows(L, 2, 64, 32, T, 5, None, P, K, I, Q, None), "ldl")
    bad(lib.vt_logprob_rows(L, 2, 64, 64, T, -1, None, P, K, I, Q, None), "n_top=-1")
    bad(lib.vt_logprob_rows(L, 2, 64, 64, T, 21, None, P, K, I, Q, None), "n_top=21")
    bad(lib.vt_logprob_rows(L, 2, 64, 64, T, 5, None, P, K, None, Q, None), "top_ids")
    bad(lib.vt_logprob_rows(L, 2, 64, 64, T, 5, None, P, K, I, None, None), "top_ids")
    bad(lib.vt_logprob_rows(L, 2, 64, 64, T, 0, None, None, None, None, None, None), "no output")
    bad(lib.vt_logprob_rows(L, 2, 64, 64, T + 2, 5, None, P, K, I, Q, None), "aligned")
    bad(lib.vt_logprob_rows(L, 2, 2 ** 30 + 1, 2 ** 30 + 1, T, 5, None, P, K, I, Q, None), "V=")
    torch.cuda.synchronize()
    assert (lp == -9.0).all() and (rk == -9).all() and (ti == -9).all() and (tl == -9.0).all()       # nothing was launched
    for kw in (dict(n_top=21), dict(n_top=-1), dict(targets=tg.cpu()), dict(targets=tg[:1]), dict(targets=tg.long()), dict(),
               dict(n_top=5, out={"top_ids": ti}), dict(n_top=5, out={"bogus": ti}), dict(n_top=5, targets=tg, out={"rank": rk})):
        with pytest.raises(_lib.VitronHipError):
            ops.logprob_rows(ld, **kw)
    with pytest.raises(_lib.VitronHipError):
        ops.logprob_rows(ld.cpu(), None, 5)
