"""vt_sample_rows_allow (ops.sample_rows(..., allow=)): per-row allow masks in the per-row sampler. The defining contract is EXACT: ids
and keep-set sizes equal vt_sample_rows on a copy of the logits with -inf written at the banned positions (tests/allow_ref.py), for
every mask shape, at the mask's word boundaries, with garbage in the bits past V, before the top-k threshold; the log-probability stays
the RAW row's, inside the fp64 bound of tests/sample_ref.py. 8 rows mixing greedy and sampled rows, with and without a penalty history;
V = 32000 (rows in registers), 32003 (odd stride: the ragged tail, the streaming form) and 40000 (the streaming form, aligned)."""
import numpy as np
import pytest
import torch

from tests import allow_ref as A
from tests import sample_ref as R
from tests.allow_cases import ROWS, VS, logits as _logits, pack as _pack, row as _row

pytestmark = pytest.mark.gpu
PEN = (1.0, 1.3, 1.0, 1.3, 1.0, 1.3, 1.0, 1.3)                 # odd rows carry a penalty history
TKP = ((0.0, 0, 1.0),) * 4 + ((0.7, 0, 0.9), (1.0, 50, 1.0), (1.3, 7, 0.8), (0.9, 20, 0.95))      # rows 0-3 greedy, 4-7 sampled


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _hist(V):
    g = torch.Generator().manual_seed(7 + V)
    return [0, 31, 32, V - 1, 123, 777, -200, V + 3] + torch.randint(0, V, (300,), generator=g).tolist()


def _params(dev, V, hist_dev, seed=5, tkp=TKP):
    return _pack([_row(*tkp[r], PEN[r], seed, 2 * r + 1, r, hist_dev if PEN[r] != 1.0 else None) for r in range(ROWS)], dev)


def _mask(V, allowed=None, banned=None, tail=True):
    """allow_mask with every bit >= V of the last word SET (the kernel must ignore them)"""
    from vitron_amd.sampling import allow_mask
    m = allow_mask(V, allowed, banned)
    if tail and V % 32:
        m[-1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    return m


def _up(masks, dev):
    return [None if m is None else torch.from_numpy(m.view(np.int32)).to(dev) for m in masks]


def _both(dev, x, pr, masks):
    """(ids, kept) with the masks, and of vt_sample_rows on the host-masked logits"""
    from vitron_amd import ops
    got = ops.sample_rows(x.to(dev), pr, return_kept=True, allow=_up(masks, dev))
    want = ops.sample_rows(A.masked_logits(x, masks).to(dev), pr, return_kept=True)
    return [t.cpu().tolist() for t in got], [t.cpu().tolist() for t in want]


def _shapes(V, x):
    g = np.random.default_rng(V)
    probes = [0, 31, 32, 1023, 1024, V - 1, 12345, 5]
    top = x.argmax(-1).tolist()
    half = [np.flatnonzero(g.random(V) < 0.5) for _ in range(ROWS)]
    return {
        "one allowed token (the boundary probes)": [_mask(V, [probes[r]]) for r in range(ROWS)],
        "two allowed tokens": [_mask(V, [probes[r], probes[(r + 3) % ROWS]]) for r in range(ROWS)],
        "about half the vocabulary": [_mask(V, half[r]) for r in range(ROWS)],
        "all but one (the row's maximum)": [_mask(V, None, [top[r]]) for r in range(ROWS)],
        "all bits set": [np.full((A.words(V),), 0xFFFFFFFF, dtype=np.uint32) for _ in range(ROWS)],
        "NULL entries among masked rows": [None if r % 3 == 0 else (_mask(V, half[r]) if r % 3 == 1 else _mask(V, [probes[r]])) for r in range(ROWS)],
        "bits past V clear": [_mask(V, half[r], tail=False) for r in range(ROWS)],
    }


@pytest.mark.parametrize("V", VS)
def test_equals_sample_rows_on_host_masked_logits(dev, V):
    x = _logits(V)
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    pr = _params(dev, V, h)
    for name, masks in _shapes(V, x).items():
        (ids, kept), (wids, wkept) = _both(dev, x, pr, masks)
        assert ids == wids and kept == wkept, (V, name, ids, wids, kept, wkept)
        for r, m in enumerate(masks):
            if m is not None:
                assert A.mask_bool(m, V)[ids[r]], (V, name, r, ids[r])
        if name.startswith("one allowed"):
            assert ids == [0, 31, 32, 1023, 1024, V - 1, 12345, 5]        # (kept_count is the -inf row's: top_k = 50 of one finite logit keeps V)
        if name.startswith("all bits set"):
            from vitron_amd import ops
            assert ids == ops.sample_rows(x.to(dev), pr).cpu().tolist()


@pytest.mark.parametrize("V", VS)
def test_the_mask_matters_in_every_masked_row(dev, V):
    """Every row's raw top 64 (by value: ties with the 64th included) is banned and top_k <= 50: the unconstrained launch necessarily
    returns a banned id, the constrained one cannot -- the two differ on EVERY row. The histories hold none of the banned ids and the
    penalty is > 1, so the penalised top 50 are the raw top 50. The reference alone (tests/sample_ref.py, fp64) says so first."""
    from vitron_amd import ops
    x = _logits(V)
    kth = x.topk(64, -1).values[:, -1:]
    banned = [np.flatnonzero((x[r] >= kth[r]).numpy()) for r in range(ROWS)]
    masks = [_mask(V, None, banned[r]) for r in range(ROWS)]
    ban_all = set(np.concatenate(banned).tolist())
    hist = [i for i in _hist(V) if i not in ban_all]
    tkp = ((0.0, 0, 1.0),) * 4 + ((0.7, 50, 0.9), (1.0, 50, 1.0), (1.3, 7, 0.8), (0.9, 20, 0.95))
    xm = A.masked_logits(x, masks)
    for r in range(ROWS):                       # the reference: unconstrained lands in the banned set, constrained cannot
        args = (*tkp[r], PEN[r], hist if PEN[r] != 1.0 else [], 5, 2 * r + 1, r)
        free, _ = R.sample_row(x[r].numpy(), *args)
        held, keep = R.sample_row(xm[r].numpy(), *args)
        assert free in banned[r] and held not in banned[r] and not keep[banned[r]].any(), (V, r, free, held)
    h = torch.tensor(hist, dtype=torch.int32, device=dev)
    pr = _params(dev, V, h, tkp=tkp)
    ld = x.to(dev)
    free = ops.sample_rows(ld, pr).cpu().tolist()
    held, kept = [t.cpu().tolist() for t in ops.sample_rows(ld, pr, return_kept=True, allow=_up(masks, dev))]
    want, wkept = [t.cpu().tolist() for t in ops.sample_rows(xm.to(dev), pr, return_kept=True)]
    for r in range(ROWS):
        assert free[r] in banned[r] and held[r] not in banned[r] and free[r] != held[r], (V, r, free[r], held[r])
    assert held == want and kept == wkept
    assert held[0] == int(xm[0].argmax()) and held[2] == int(xm[2].argmax())     # greedy rows without a penalty: the masked row's first maximum


@pytest.mark.parametrize("V", VS)
def test_mask_applies_before_the_top_k_threshold(dev, V):
    """Rows whose 5 largest logits include 3 banned ones: top_k = 5 keeps the 5 largest ALLOWED tokens -- the two that are left and the
    next three, which sit close below so that top_p = 0.999 still needs all five. A mask applied after the threshold would keep 2 (at
    top_p = 1 it would count the three banned tokens with probability 0 as kept: 5 for the wrong reason, hence the second top_p)."""
    from vitron_amd import ops
    g = torch.Generator().manual_seed(V)
    x = torch.randn((ROWS, V), generator=g)
    masks = []
    for r in range(ROWS):
        pos = [(31 + 1000 * r) % V, (32 + 1000 * r) % V, V - 1 - r, 5 + r, 20000 + r, 64 + r, 9000 + r, 30000 + r]
        for j, p in enumerate(pos):
            x[r, p] = 10.0 - 0.1 * j
        masks.append(_mask(V, None, [pos[0], pos[2], pos[3]]))
    xm = A.masked_logits(x, masks)
    for top_p in (1.0, 0.999):
        pr = _pack([_row(1.0, 5, top_p, 1.0, 9, r, r) for r in range(ROWS)], dev)
        (ids, kept), (wids, wkept) = _both(dev, x, pr, masks)
        ref = [int(R.keep_set(xm[r].numpy(), 1.0, 5, top_p).sum()) for r in range(ROWS)]
        assert ref == [5] * ROWS and kept == wkept == ref and ids == wids, (top_p, kept, wkept, ref)
        _, kfree = ops.sample_rows(x.to(dev), pr, return_kept=True)
        assert kfree.cpu().tolist() == [5] * ROWS


@pytest.mark.parametrize("V", VS)
def test_allow_none_is_sample_rows(dev, V):
    from vitron_amd import _lib, ops
    lib = _lib.load()
    x = _logits(V)
    ld = x.to(dev)
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    pr = _params(dev, V, h)
    base = ops.sample_rows(ld, pr, return_kept=True, return_logprob=True)
    for allow in (None, [None] * ROWS):                                          # today's call; the new kernel with NULL entries only
        got = ops.sample_rows(ld, pr, return_kept=True, return_logprob=True, allow=allow)
        assert all(torch.equal(a, b) for a, b in zip(got, base))
    out = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)                 # the C entry point with allow == NULL
    kept = torch.empty((ROWS,), dtype=torch.int32, device=dev)
    lp = torch.empty((ROWS,), dtype=torch.float32, device=dev)
    st = lib.vt_sample_rows_allow(ld.data_ptr(), ROWS, V, ld.stride(0), pr.data_ptr(), None, out.data_ptr(), kept.data_ptr(), lp.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert st == 0, _lib.last_error(lib)
    assert torch.equal(out, base[0]) and torch.equal(kept, base[1]) and torch.equal(lp, base[2])
    if hasattr(torch, "uint32"):                                                 # masks may be uint32 tensors as well
        m = _mask(V, None, [int(base[0][0])])
        a = ops.sample_rows(ld, pr, allow=[torch.from_numpy(m.view(np.int32)).to(dev)] + [None] * (ROWS - 1))
        b = ops.sample_rows(ld, pr, allow=[torch.from_numpy(m.view(np.int32)).to(dev).view(torch.uint32)] + [None] * (ROWS - 1))
        assert torch.equal(a, b) and int(a[0]) != int(base[0][0])


@pytest.mark.parametrize("V", VS)
def test_logprob_stays_the_raw_rows(dev, V, record_property):
    """logprob[r] = log_softmax(RAW row)[id] with banned positions INCLUDED in the sum, inside the bound tests/sample_ref.py derives; the
    masks ban each row's maximum (so the chosen ids are not the unconstrained ones) or allow half the row."""
    from vitron_amd import ops
    x = _logits(V)
    ld = x.to(dev)
    ref = R.logprob_ref(x.numpy())
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    pr = _params(dev, V, h)
    shapes = _shapes(V, x)
    worst = 0.0
    for name in ("all but one (the row's maximum)", "about half the vocabulary", "one allowed token (the boundary probes)"):
        masks = shapes[name]
        ids, lp = ops.sample_rows(ld, pr, return_logprob=True, allow=_up(masks, dev))
        idl = ids.cpu().long().numpy()
        assert idl.tolist() == ops.sample_rows(A.masked_logits(x, masks).to(dev), pr).cpu().tolist()
        bound = R.logprob_bound(x.numpy(), idl)
        ratio = np.abs(lp.cpu().double().numpy() - ref[np.arange(ROWS), idl]) / bound
        print(f"V={V} {name}: logprob err/bound per row {[f'{v:.3f}' for v in ratio]}")
        assert (ratio <= 1.0).all(), (name, ratio.tolist())
        worst = max(worst, float(ratio.max()))
    assert int(ids[0]) == 0 and float(lp[0]) < -20.0          # row 0 holds a dominant token at 123: the forced token 0 is improbable, and says so
    record_property("logprob_err_over_bound", worst)


def test_bad_calls_and_the_empty_mask(dev):
    from vitron_amd import _lib, ops
    lib = _lib.load()
    V = 64
    x = torch.randn((2, V), generator=torch.Generator().manual_seed(1))
    ld = x.to(dev)
    pr = _pack([_row(), _row(0.8, 5, 0.9, 1.0, 3, 1, 1)], dev)
    out = torch.empty((2,), dtype=torch.int32, device=dev)
    ok = torch.from_numpy(_mask(V).view(np.int32)).to(dev)
    ptrs = ops.allow_pointers([ok, None], 2, V, dev)
    assert ptrs.dtype == torch.int64 and ptrs.cpu().tolist() == [ok.data_ptr(), 0]
    L, Pp, Ap, Op = ld.data_ptr(), pr.data_ptr(), ptrs.data_ptr(), out.data_ptr()

    def bad(status, needle):
        msg = _lib.last_error(lib)
        assert status < 0 and needle in msg, (status, msg)

    bad(lib.vt_sample_rows_allow(None, 2, V, V, Pp, Ap, Op, None, None, None), "null")
    bad(lib.vt_sample_rows_allow(L, 2, V, V, None, Ap, Op, None, None, None), "null")
    bad(lib.vt_sample_rows_allow(L, 2, V, V, Pp, Ap, None, None, None, None), "null")
    bad(lib.vt_sample_rows_allow(L, 0, V, V, Pp, Ap, Op, None, None, None), "rows=0")
    bad(lib.vt_sample_rows_allow(L, 2, 0, V, Pp, Ap, Op, None, None, None), "V=0")
    bad(lib.vt_sample_rows_allow(L, 2, V, 32, Pp, Ap, Op, None, None, None), "ldl")
    bad(lib.vt_sample_rows_allow(L, 2, 262145, 262145, Pp, Ap, Op, None, None, None), "beyond the history mask")     # refused before any launch
    bad(lib.vt_sample_rows_allow(L, 2, V, V, Pp + 4, Ap, Op, None, None, None), "aligned")
    bad(lib.vt_sample_rows_allow(L, 2, V, V, Pp, Ap + 4, Op, None, None, None), "aligned")
    base = ops.sample_rows(ld, pr, allow=[ok, None])
    assert torch.equal(ops.sample_rows(ld, pr, _allow_ptrs=ptrs), base)          # the private form: a pointer array built earlier
    for kw in (dict(_allow_ptrs=ptrs[:1]), dict(_allow_ptrs=ptrs.cpu()), dict(_allow_ptrs=ptrs.int()), dict(_allow_ptrs=[ok, None]),
               dict(allow=[ok, None], _allow_ptrs=ptrs)):
        with pytest.raises(_lib.VitronHipError):
            ops.sample_rows(ld, pr, **kw)
    for allow in ([ok], [ok, ok, ok], [ok, ok.float()], [ok, ok.long()], [ok, ok.cpu()], [ok, torch.zeros((3,), dtype=torch.int32, device=dev)],
                  [ok, torch.zeros((4,), dtype=torch.int32, device=dev)[::2]], [ok, 5], ok, ptrs[:1], ptrs.cpu(), 7):
        with pytest.raises(_lib.VitronHipError):
            ops.sample_rows(ld, pr, allow=allow)
    # a row with nothing allowed is the all -inf row of vt_sample_rows; its neighbour is untouched
    for V2 in (64, 32003):
        x2 = torch.randn((2, V2), generator=torch.Generator().manual_seed(2))
        none = torch.zeros((A.words(V2),), dtype=torch.int32, device=dev)
        for greedy_first in (True, False):
            pr2 = _pack([_row(), _row(0.8, 5, 0.9, 1.0, 3, 1, 1)] if greedy_first else [_row(0.8, 5, 0.9, 1.0, 3, 1, 1), _row()], dev)
            dead = x2.clone()
            dead[0] = -float("inf")
            got = ops.sample_rows(x2.to(dev), pr2, return_kept=True, allow=[none, None])
            want = ops.sample_rows(dead.to(dev), pr2, return_kept=True)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (V2, greedy_first, got, want)
            assert -1 <= int(got[0][0]) < V2
    torch.cuda.synchronize()
