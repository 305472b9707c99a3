"""vt_sample_rows_trunc (ops.sample_rows(..., trunc=)): min_p, typical_p, epsilon_cutoff and eta_cutoff in the per-row sampler (DESIGN.md
9.9). Two kinds of check:
  EXACT   trunc=None, all-inactive rows and rows whose fields are NaN / negative / >= 1 return the ids, kept_count and logprob of
          vt_sample_rows_adj bit for bit, with and without allow masks, adjustments and a penalty history; greedy rows ignore active
          fields; a row's result does not depend on its neighbours.
  PLACED  16 cases per shape from tests/trunc_ref.py (each stage alone, the pairs, triples and all four, after top-k and top-p, every
          fourth with an allow mask, every third with a penalty history), their parameters placed in the middle of a gap with an fp64
          margin >= 1e-3: kept_count equals the fp64 keep-set size, the id lies in the keep-set and equals the fp64 inverse-CDF answer;
          the counter of every row is chosen so that its uniform is at least 1e-4 of the kept mass from a seam, and that is asserted.
Shapes (V, row stride): 1000 and 32768 (rows in registers), 32003 / 32004 (registers, ragged tail), 1001 / 1001 (the streaming form by
misalignment), 33000 (the streaming form by size). 16 rows."""
import numpy as np
import pytest
import torch

from tests import sample_ref as S
from tests import trunc_ref as R
from tests.allow_cases import pack as _pack, row as _row

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = ((1000, 1000), (32768, 32768), (32003, 32004), (1001, 1001), (33000, 33000))
ROWS = 16
SEED = 11
SEAM = 1e-4


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _hist(V):
    g = torch.Generator().manual_seed(23 + V)
    return [0, 31, 32, V - 1, 123, 777, -200, V + 3] + torch.randint(0, V, (300,), generator=g).tolist()


_built = {}


def _cases(V):
    """The 16 placed cases of vocabulary V with a counter per row that keeps its uniform off the seams; built once, never modified"""
    if V not in _built:
        cases = R.placed_cases(V, seed=7, allow_every=4, penalty_every=3, history=_hist(V))
        for n, c in enumerate(cases):
            for counter in range(64):
                want, dist = R.pick(c["s"], c["A"], S.uniform24(SEED, counter, n))
                if dist >= SEAM:
                    break
            c.update(counter=counter, want=want, seam=dist)
        _built[V] = cases
    return _built[V]


def _logits(cases, V, ldl, dev):
    buf = torch.zeros((ROWS, ldl), dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(np.stack([c["row"] for c in cases]))
    return buf.to(dev)[:, :V]


def _masks(cases, V, dev):
    from vitron_amd.sampling import allow_mask
    return [None if c["allow"] is None else torch.from_numpy(allow_mask(V, np.flatnonzero(c["allow"])).view(np.int32)).to(dev) for c in cases]


def _params(cases, hist_dev, dev, order=None, greedy=()):
    order = range(len(cases)) if order is None else order
    return _pack([_row(0.0 if n in greedy else cases[n]["T"], cases[n]["top_k"], cases[n]["top_p"], cases[n]["penalty"], SEED,
                       cases[n]["counter"], n, hist_dev if cases[n]["penalty"] != 1.0 else None) for n in order], dev)


def _bits(res):
    ids, kept, lp = res
    return ids.cpu().tolist(), kept.cpu().tolist(), lp.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("V,ldl", SHAPES)
def test_placed_cases_match_the_fp64_keep_sets_and_draws(dev, V, ldl):
    from vitron_amd import ops
    from vitron_amd.sampling import pack_trunc_rows
    cases = _cases(V)
    assert len(cases) == ROWS and [c["combo"] for c in cases] == list(R.COMBOS)       # fixed length, nothing skipped
    assert all(c["seam"] >= SEAM for c in cases), [c["seam"] for c in cases]
    x = _logits(cases, V, ldl, dev)
    assert x.stride(0) == ldl
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    masks = _masks(cases, V, dev)
    trunc = pack_trunc_rows([c["trunc"] for c in cases], dev)
    ids, kept, lp = ops.sample_rows(x, _params(cases, h, dev), return_kept=True, return_logprob=True, allow=masks, trunc=trunc)
    ids, kept, lp = ids.cpu().tolist(), kept.cpu().tolist(), lp.cpu().numpy()
    for n, c in enumerate(cases):
        print(f"V={V} row {n} stages {c['combo']} trunc {c['trunc']} kept {kept[n]} / fp64 {int(c['A'].sum())} of {int(c['A0'].sum())} "
              f"id {ids[n]} / fp64 {c['want']} seam {c['seam']:.2e}")
    for n, c in enumerate(cases):
        assert kept[n] == int(c["A"].sum()), (V, n, c["combo"], c["trunc"], kept[n], int(c["A"].sum()), int(c["A0"].sum()))
        assert 0 <= ids[n] < V and c["A"][ids[n]], (V, n, ids[n])
        assert ids[n] == c["want"], (V, n, c["combo"], ids[n], c["want"], c["seam"])
    assert sum(int(c["A"].sum()) < int(c["A0"].sum()) for c in cases) >= 12            # the stages removed something
    # logprob stays over the RAW row
    raw = np.stack([c["row"] for c in cases])
    ref = S.logprob_ref(raw)[np.arange(ROWS), ids]
    assert np.all(np.abs(lp.astype(np.float64) - ref) <= S.logprob_bound(raw, ids)), (V, lp, ref)
    # a row's result does not depend on its neighbours: the same rows in reverse order, every row with its own stream
    order = list(range(ROWS))[::-1]
    y = _logits([cases[n] for n in order], V, ldl, dev)
    rev = ops.sample_rows(y, _params(cases, h, dev, order), return_kept=True, return_logprob=True, allow=[masks[n] for n in order],
                          trunc=pack_trunc_rows([cases[n]["trunc"] for n in order], dev))
    assert [t[::-1] for t in _bits(rev)] == [ids, kept, lp.view(np.uint32).tolist()]


def _junk_rows(dev):
    """16 vt_trunc_row whose four fields are all inactive, written as raw floats (pack_trunc_rows validates what it packs): zeros, NaN,
    negative values, -inf, and for the three fields whose range is (0, 1) also 1, values above 1 and +inf."""
    nan, inf = float("nan"), float("inf")
    rows = [(0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (nan, nan, nan, nan), (-0.5, -0.5, -0.5, -0.5), (-inf, -inf, -inf, -inf),
            (0.0, 1.0, 1.0, 1.0), (0.0, 1.5, 2.0, 7.0), (0.0, inf, inf, inf), (nan, 1.0, 0.0, -1.0), (-1e-30, 3.0, nan, 1.0),
            (0.0, nan, 1.0, inf), (-2.0, 1.0, -0.0, 0.0), (-0.0, -0.0, -0.0, -0.0), (nan, 2.0, -3.0, nan), (0.0, 1.0, nan, 0.0),
            (-1.0, inf, 1.0, -inf)]
    assert len(rows) == ROWS and not any(any(R.on(t)) for t in rows)
    return torch.from_numpy(np.asarray(rows, dtype="<f4").view(np.uint8).reshape(ROWS, 16).copy()).to(dev)


@pytest.mark.parametrize("V,ldl", SHAPES)
def test_inactive_rows_are_bit_equal_to_the_adjusted_sampler(dev, V, ldl):
    from vitron_amd import ops
    from vitron_amd.sampling import pack_trunc_rows
    cases = _cases(V)
    x = _logits(cases, V, ldl, dev)
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    greedy = tuple(range(0, ROWS, 5))                                               # rows 0, 5, 10, 15 are greedy
    pr = _params(cases, h, dev, greedy=greedy)
    masks = _masks(cases, V, dev)
    g = torch.Generator().manual_seed(5 + V)
    adj = [None if n % 3 == 0 else (torch.randn((V, 2), generator=g) * 2.0).to(dev) for n in range(ROWS)]
    off, junk = pack_trunc_rows([None] * ROWS, dev), _junk_rows(dev)
    active = pack_trunc_rows([c["trunc"] for c in cases], dev)
    for allow, adjust in ((None, None), (masks, None), (None, adj), (masks, adj)):
        kw = dict(return_kept=True, return_logprob=True, allow=allow, adjust=adjust)
        base = _bits(ops.sample_rows(x, pr, **kw))                                  # vt_sample_rows / _allow / _adj
        if adjust is None:                                                          # vt_sample_rows_adj itself, NULL adjustments
            assert _bits(ops.sample_rows(x, pr, adjust=[None] * ROWS, **{k: v for k, v in kw.items() if k != "adjust"})) == base
        assert _bits(ops.sample_rows(x, pr, trunc=None, **kw)) == base
        assert _bits(ops.sample_rows(x, pr, trunc=off, **kw)) == base
        assert _bits(ops.sample_rows(x, pr, trunc=junk, **kw)) == base
        got = _bits(ops.sample_rows(x, pr, trunc=active, **kw))                     # greedy rows ignore active fields
        for part, want in zip(got, base):
            assert [part[n] for n in greedy] == [want[n] for n in greedy]
        assert all(base[1][n] == 1 for n in greedy)
        assert any(got[1][n] != base[1][n] for n in range(ROWS) if n not in greedy)     # ... the sampled rows do not


@pytest.mark.parametrize("V,ldl", ((1000, 1000), (1001, 1001), (33000, 33000)))
def test_one_allowed_token_with_every_stage_active(dev, V, ldl):
    from vitron_amd import ops
    from vitron_amd.sampling import allow_mask, pack_trunc_rows
    cases = _cases(V)
    x = _logits(cases, V, ldl, dev)
    only = [0, 31, 32, V - 1, V // 2, 7, 999, 500, 64, 63, 1, 2, 3, 100, 200, 300]
    masks = [torch.from_numpy(allow_mask(V, [t]).view(np.int32)).to(dev) for t in only]
    pr = _pack([_row(c["T"], c["top_k"], c["top_p"], 1.0, SEED, n, n) for n, c in enumerate(cases)], dev)
    trunc = pack_trunc_rows([(0.3, 0.5, 1e-2, 1e-2), (1.0, 0.01, 0.9, 0.9), (0.05, 0.99, 1e-4, 0.5), (0.5, 0.5, 0.5, 0.5)] * 4, dev)
    ids, kept = ops.sample_rows(x, pr, return_kept=True, allow=masks, trunc=trunc)
    assert ids.cpu().tolist() == only and kept.cpu().tolist() == [1] * ROWS


@pytest.mark.parametrize("V,ldl", ((1000, 1000), (1001, 1001)))
def test_typical_removes_the_arg_max_and_epsilon_protects_the_new_maximum(dev, V, ldl):
    """The constructed row of tests/trunc_ref.py in both forms: the survivor is the maximum of what typical sampling left, not the row's
    arg-max."""
    from vitron_amd import ops
    from vitron_amd.sampling import pack_trunc_rows
    s, A0, trunc = R.argmax_removed_case(V)
    A = R.apply(s, A0, trunc)
    new_top = int(np.flatnonzero(A)[0])
    assert A.sum() == 1 and new_top != int(np.argmax(s))
    buf = torch.zeros((4, ldl), dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(s.astype(F32))
    x = buf.to(dev)[:, :V]
    pr = _pack([_row(1.0, R.ARGMAX_REMOVED_TOP_K, 1.0, 1.0, SEED, n, n) for n in range(4)], dev)
    ids, kept = ops.sample_rows(x, pr, return_kept=True, trunc=pack_trunc_rows([trunc] * 4, dev))
    assert ids.cpu().tolist() == [new_top] * 4 and kept.cpu().tolist() == [1] * 4
    # typical alone: the arg-max is gone, the others stay
    alone = (0.0, trunc[1], 0.0, 0.0)
    ids, kept = ops.sample_rows(x, pr, return_kept=True, trunc=pack_trunc_rows([alone] * 4, dev))
    after = R.apply(s, A0, alone)
    assert kept.cpu().tolist() == [int(after.sum())] * 4 and all(after[i] for i in ids.cpu().tolist()) and not after[int(np.argmax(s))]


def test_bad_calls(dev):
    from vitron_amd import _lib, ops
    from vitron_amd.sampling import pack_trunc_rows
    V = 64
    x = torch.zeros((2, V), dtype=torch.float32, device=dev)
    pr = _pack([_row(), _row()], dev)
    good = pack_trunc_rows([None, (0.1, 0.9, 0.0, 0.0)], dev)
    assert ops.sample_rows(x, pr, trunc=good).cpu().tolist() == [0, 0]
    for bad in (good.cpu(), good[:1], good.to(torch.int32), good.t(), torch.zeros((2, 4), dtype=torch.float32, device=dev),
                np.zeros((2, 16), np.uint8), [None, None]):
        with pytest.raises(_lib.VitronHipError, match="trunc"):
            ops.sample_rows(x, pr, trunc=bad)
