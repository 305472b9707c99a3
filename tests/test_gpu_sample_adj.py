"""vt_sample_rows_adj (ops.sample_rows(..., adjust=)): per-row additive adjustments in the per-row sampler. The defining
contract is EXACT: ids and keep-set sizes equal the EXISTING ops.sample_rows(allow=...) on logits adjusted on the host by
tests/bias_ref.py (mask, + pre, repetition penalty, + post, each step one fp32 operation), with penalty 1 and no history in its
parameters -- no new code on the reference side. 8 rows of tests/allow_cases.py's logits: 4 greedy, 4 sampled, odd rows with a penalty
history, some rows with an allow mask, rows 0 and 4 with a NULL adjust entry; V = 32000 (rows in registers), 32003 (odd stride: the
streaming form, ragged) and 40000 (the streaming form, aligned)."""
import numpy as np
import pytest
import torch

from tests import allow_ref as A
from tests import bias_ref as R
from tests import sample_ref as S
from tests.allow_cases import ROWS, VS, logits as _logits, pack as _pack, row as _row

pytestmark = pytest.mark.gpu
F32 = np.float32
PEN = (1.0, 1.3, 1.0, 1.3, 1.0, 1.3, 1.0, 1.3)                 # odd rows carry a penalty history
TKP = ((0.0, 0, 1.0),) * 4 + ((0.7, 0, 0.9), (1.0, 50, 1.0), (1.3, 7, 0.8), (0.9, 20, 0.95))      # rows 0-3 greedy, 4-7 sampled
NULL_ADJ = (0, 4)
MASKED = (2, 3, 6, 7)


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _hist(V):
    g = torch.Generator().manual_seed(17 + V)
    return [0, 31, 32, V - 1, 123, 777, -200, V + 3] + torch.randint(0, V, (300,), generator=g).tolist()


def _params(dev, hist_dev, pen=PEN, tkp=TKP, seed=5):
    return _pack([_row(*tkp[r], pen[r], seed, 2 * r + 1, r, hist_dev if pen[r] != 1.0 else None) for r in range(len(tkp))], dev)


def _host_row(raw, allow_bool, adj, penalty, hist):
    """The row the sampler works on. adj None (a NULL entry): the mask and the penalty alone, nothing is added."""
    if adj is not None:
        return R.adjusted(raw, allow_bool, adj[0], adj[1], penalty, hist)
    x = np.array(raw, dtype=F32, copy=True)
    if allow_bool is not None:
        x[~allow_bool] = -np.inf
    return S.repetition_penalty(x, hist, penalty) if penalty != 1.0 else x


_built = {}


def _inputs(V):
    """(masks, mask bools, adjustments, host-adjusted logits, unadjusted host logits), built once per V and never modified. Every
    adjusted row: a bias on 300 ids (ids 0, 31, 32, V - 1 among them), a count penalty on 200 ids, and -1000 behind the id the row
    would pick greedily without the adjustment."""
    if V in _built:
        return _built[V]
    from vitron_amd.sampling import allow_mask
    x = _logits(V).numpy()
    hist = _hist(V)
    g = np.random.default_rng(40 + V)
    masks, bools, adjs = [], [], []
    for r in range(ROWS):
        m = None
        if r in MASKED:
            m = allow_mask(V, np.flatnonzero(g.random(V) < 0.6))
            if V % 32:
                m[-1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)          # garbage past V: ignored
        masks.append(m)
        bools.append(None if m is None else A.mask_bool(m, V))
    plain = np.stack([_host_row(x[r], bools[r], None, PEN[r], hist) for r in range(ROWS)])
    for r in range(ROWS):
        if r in NULL_ADJ:
            adjs.append(None)
            continue
        ids = np.unique(np.concatenate([[0, 31, 32, V - 1], g.choice(V, size=296, replace=False)]))
        counted = g.choice(V, size=200, replace=False)
        pre, post = R.bias_rows(V, np.repeat(counted, g.integers(1, 6, size=200)), ids, g.standard_normal(ids.size) * 4, 0.3, 0.5)
        post[int(np.argmax(plain[r]))] = F32(-1000.0)
        adjs.append((pre, post))
    host = np.stack([_host_row(x[r], bools[r], adjs[r], PEN[r], hist) for r in range(ROWS)])
    _built[V] = (masks, bools, adjs, host, plain)
    return _built[V]


def _up_masks(masks, dev):
    return [None if m is None else torch.from_numpy(m.view(np.int32)).to(dev) for m in masks]


def _up_adj(adjs, dev, odd=False):
    """[V][2] device tensors; odd: 8 bytes behind a 16-byte boundary (the sampler's 8-byte loads instead of its 16-byte ones)"""
    out = []
    for a in adjs:
        if a is None:
            out.append(None)
            continue
        t = torch.from_numpy(np.stack(a, 1).copy())
        if odd:
            buf = torch.zeros((t.numel() + 4,), dtype=torch.float32, device=dev)
            t = buf[2:2 + t.numel()].view(t.shape).copy_(t)
        out.append(t.to(dev))
        assert out[-1].data_ptr() % 16 == (8 if odd else 0)
    return out


def _lists(res):
    return [t.cpu().tolist() for t in res]


@pytest.mark.parametrize("V", VS)
def test_equals_the_existing_sampler_on_host_adjusted_logits(dev, V):
    from vitron_amd import ops
    masks, bools, adjs, host, plain = _inputs(V)
    # the premise, on the host alone: every adjusted greedy row picks another id than it would unadjusted
    for r in range(4):
        if r not in NULL_ADJ:
            assert int(np.argmax(host[r])) != int(np.argmax(plain[r])), (V, r)
    x = _logits(V).to(dev)
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    pr = _params(dev, h)
    no_pen = _params(dev, None, pen=(1.0,) * ROWS)
    dm, da = _up_masks(masks, dev), _up_adj(adjs, dev)
    ids, kept, lp = _lists(ops.sample_rows(x, pr, return_kept=True, return_logprob=True, allow=dm, adjust=da))
    wids, wkept = _lists(ops.sample_rows(torch.from_numpy(host).to(dev), no_pen, return_kept=True))
    assert ids == wids and kept == wkept, (V, ids, wids, kept, wkept)
    for r in range(4):
        assert ids[r] == int(np.argmax(host[r]))
        if r not in NULL_ADJ:
            assert ids[r] != int(np.argmax(plain[r]))
    for r in MASKED:
        assert bools[r][ids[r]]
    odd = _lists(ops.sample_rows(x, pr, return_kept=True, return_logprob=True, allow=dm, adjust=_up_adj(adjs, dev, odd=True)))
    assert odd[0] == ids and odd[1] == kept and odd[2] == lp                     # adjustments that are 8-byte aligned only
    # without masks: the allow ARRAY is NULL, the adjustments stay
    host_free = np.stack([_host_row(_logits(V).numpy()[r], None, adjs[r], PEN[r], _hist(V)) for r in range(ROWS)])
    got = _lists(ops.sample_rows(x, pr, return_kept=True, adjust=da))
    assert got == _lists(ops.sample_rows(torch.from_numpy(host_free).to(dev), no_pen, return_kept=True))
    # adjust=None is the allow launch; all entries None changes nothing either
    base = _lists(ops.sample_rows(x, pr, return_kept=True, return_logprob=True, allow=dm))
    assert _lists(ops.sample_rows(x, pr, return_kept=True, return_logprob=True, allow=dm, adjust=None)) == base
    assert _lists(ops.sample_rows(x, pr, return_kept=True, return_logprob=True, allow=dm, adjust=[None] * ROWS)) == base
    assert base[0] != ids
    # logprob stays the RAW row's: vt_sample_rows_allow held to the chosen id returns the same float, bit for bit
    from vitron_amd.sampling import allow_mask
    one = [torch.from_numpy(allow_mask(V, [i]).view(np.int32)).to(dev) for i in ids]
    greedy = _params(dev, None, pen=(1.0,) * ROWS, tkp=((0.0, 0, 1.0),) * ROWS)
    rid, rlp = ops.sample_rows(x, greedy, return_logprob=True, allow=one)
    assert rid.cpu().tolist() == ids
    assert np.array_equal(np.asarray(lp, dtype=F32).view(np.uint32), rlp.cpu().numpy().view(np.uint32)), (V, lp, rlp.cpu().tolist())


def _order_rows(V):
    """Four greedy rows over a floor of -10. Row 0: the biased token is in the penalty history (raw 1, bias +3, penalty 2, rival 3.0):
    (1 + 3) / 2 = 2 loses; the penalty first would give 1 / 2 + 3 = 3.5. Row 1: a counted token is penalised (raw 4, penalty 2, post
    -1.5, rival 1.0): 4 / 2 - 1.5 = 0.5 loses; post first would give (4 - 1.5) / 2 = 1.25. Rows 2 and 3: a masked token under a bias
    of +1e30 stays -inf (greedy; sampled below with the same rows)."""
    a, rival, c, m = 700, V - 1, 31, 32
    x = np.full((4, V), -10.0, dtype=F32)
    pre, post = np.zeros((4, V), dtype=F32), np.zeros((4, V), dtype=F32)
    x[0, a], x[0, rival], pre[0, a] = 1.0, 3.0, 3.0
    x[1, c], x[1, rival], post[1, c] = 4.0, 1.0, -1.5
    x[2, m], x[2, rival], pre[2, m] = 5.0, 1.0, 1e30
    x[3, m], x[3, rival], pre[3, m] = 5.0, 1.0, 1e30
    hist = [[a], [c], [], []]
    return x, pre, post, hist, (a, rival, c, m)


@pytest.mark.parametrize("V", VS)
def test_the_order_of_the_steps_and_a_masked_token_under_a_huge_bias(dev, V):
    from vitron_amd import ops
    from vitron_amd.sampling import allow_mask
    x, pre, post, hist, (a, rival, c, m) = _order_rows(V)
    # on the host: the right order picks the rival, either wrong order picks the other token
    assert int(np.argmax(R.adjusted(x[0], None, pre[0], post[0], 2.0, hist[0]))) == rival
    assert int(np.argmax(S.repetition_penalty(x[0], hist[0], 2.0) + pre[0])) == a
    assert int(np.argmax(R.adjusted(x[1], None, pre[1], post[1], 2.0, hist[1]))) == rival
    assert int(np.argmax(S.repetition_penalty(x[1] + post[1], hist[1], 2.0))) == c
    hd = [torch.tensor(h or [0], dtype=torch.int32, device=dev) for h in hist]
    masks = [None, None] + [torch.from_numpy(allow_mask(V, None, [m]).view(np.int32)).to(dev)] * 2
    adj = [torch.from_numpy(np.stack([pre[r], post[r]], 1).copy()).to(dev) for r in range(4)]
    for T in (0.0, 1.0):
        pr = _pack([_row(0.0, 0, 1.0, 2.0, 0, 0, 0, hd[0]), _row(0.0, 0, 1.0, 2.0, 0, 0, 1, hd[1]),
                    _row(T, 0, 1.0, 1.0, 3, 1, 2), _row(T, 5, 0.9, 1.0, 3, 2, 3)], dev)
        ids = ops.sample_rows(torch.from_numpy(x).to(dev), pr, allow=masks, adjust=adj).cpu().tolist()
        assert ids[:2] == [rival, rival], (V, ids)
        assert m not in ids[2:] and all(0 <= i < V for i in ids), (V, T, ids)
        if T == 0.0:
            assert ids[2:] == [rival, rival]                                     # the only value above the floor that is left


def test_bad_calls(dev):
    from vitron_amd import _lib, ops
    V = 64
    x = torch.zeros((2, V), dtype=torch.float32, device=dev)
    pr = _pack([_row(), _row()], dev)
    good = torch.zeros((V, 2), dtype=torch.float32, device=dev)
    assert ops.sample_rows(x, pr, adjust=[good, None]).cpu().tolist() == [0, 0]
    for bad in ([good.double(), None], [good.to(torch.bfloat16), None], [good[:-1], None], [torch.zeros((V, 3), device=dev), None],
                [good.cpu(), None], [good.t(), None], [good], good, [np.zeros((V, 2), np.float32), None]):
        with pytest.raises(_lib.VitronHipError, match="adjust"):
            ops.sample_rows(x, pr, adjust=bad)
    ptrs = torch.tensor([good.data_ptr(), 0], dtype=torch.int64, device=dev)
    assert ops.sample_rows(x, pr, _adjust_ptrs=ptrs).cpu().tolist() == [0, 0]
    with pytest.raises(_lib.VitronHipError, match="not both"):
        ops.sample_rows(x, pr, adjust=[good, None], _adjust_ptrs=ptrs)
    for bad in (ptrs.to(torch.int32), ptrs[:1], ptrs.cpu()):
        with pytest.raises(_lib.VitronHipError, match="_adjust_ptrs"):
            ops.sample_rows(x, pr, _adjust_ptrs=bad)
