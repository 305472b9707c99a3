"""vt_sample_rows_wm (ops.sample_rows(..., watermark=)): the SynthID text watermark inside the per-row sampler. Checks:
  EXACT     watermark=None, all-NULL cells and greedy rows with live cells return the ids, kept_count and logprob of vt_sample_rows_trunc
            bit for bit, with and without allow masks, adjustments and truncation; the greedy rows' cells stay all zero.
  STATE     12 launches on the same cells, the kernel's ids fed back into tests/synthid_ref.py's cell, repeats forced through one-token
            allow masks: every cell word equals the restatement's after every launch (ngram_len 2 and 5, history 2 and 1024, skip_first
            both ways).
  PLACED    16 cases per shape built like tests/trunc_ref.py's (8 to 64 survivors behind top-k / top-p / the truncation stages, depth 1,
            9 and 30, every third with a penalty history, every fourth with an allow mask): the id equals the fp64 inverse-CDF answer
            over the fp64 tournament, kept_count the truncation's fp64 keep-set size; every row's counter keeps its uniform at least 1e-4
            of the mass from a seam of the fp64 CDF (the kernel's fp32 tournament stays within 3e-7 of it), and that is asserted; a
            row's result does not depend on its neighbours.
  FULL ROW  no truncation, near-uniform rows at V = 32003, depth 9: the id's fp64 interval contains the uniform within 1e-4 (a wrong g
            for a sizeable share of the vocabulary moves the CDF by about 0.1).
  PROBES    equal logits on two or four survivors, depth 1: the tournament's probabilities (0.75, 0.25), (0.5, 0.5), (0.4375, 0.1875 x 3)
            are exact in fp32, and the uniform is taken where they give different ids; survivor ids 0, 31, 32 and V - 1.
  BAD CALLS every refusal returns -1 with a message; junk in a cell never leaves the ring; junk fields are refused before the launch.
Shapes (V, row stride): (1000, 1000), (32768, 32768), (32003, 32004). 16 rows."""
import numpy as np
import pytest
import torch

from tests import sample_ref as S
from tests import synthid_ref as W
from tests import trunc_ref as R
from tests.allow_cases import pack as _pack, row as _row

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = ((1000, 1000), (32768, 32768), (32003, 32004))
ROWS = 16
SEED = 29
SEAM = 1e-4
DEPTHS = (1, 9, 30)


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _hist(V):
    g = torch.Generator().manual_seed(41 + V)
    return [0, 31, 32, V - 1, 123, 777, -200, V + 3] + torch.randint(0, V, (300,), generator=g).tolist()


def _cfg(n, **kw):
    """The configuration of case n: depth 1 / 9 / 30 in turn, ngram_len 5 / 2 / 3"""
    return W.Config((5, 2, 3)[n % 3], W.KEYS30[:DEPTHS[n % 3]], **kw)


def _wm(cfg):
    from vitron_amd.watermark import SynthIDWatermark
    return SynthIDWatermark(cfg.as_dict())


def _seed_cell(cell, ref, context, calls=0):
    """Write a context (and a call count) into a device cell and its restatement: the cell is plain data"""
    n1 = ref.cfg.ngram_len - 1
    ref.w[0] = calls
    ref.w[4:4 + n1] = np.asarray(context[:n1], dtype=np.uint64)
    cell.copy_(torch.from_numpy(ref.w.view(np.int64).copy()))


def _words(cell):
    return cell.cpu().numpy().view(np.uint64)


_built = {}


def _cases(V):
    """16 placed cases at vocabulary V, built once and never modified: trunc_ref's placement with 8 to 64 final survivors, then the fp64
    tournament of case n's configuration behind the context (3 n + 1, ...) and a counter that keeps the uniform off the seams."""
    if V in _built:
        return _built[V]
    g = np.random.default_rng(5 * 1000003 + V)
    hist = _hist(V)
    cases = []
    for n, combo in enumerate(R.COMBOS):
        for attempt in range(400):
            row, T, _, p = R.draw_row(g, V)
            k = (24, 50, 64)[int(g.integers(3))]
            allow = (g.random(V) < 0.6) if n % 4 == 3 else None
            pen = 1.3 if n % 3 == 2 else 1.0
            s = R.scaled(row, T, allow, pen, hist)
            A0 = R.base_keep(s, k, p)
            ok = R.top_p_margin(s, k, p) >= 1e-4 and np.ptp(s[np.isfinite(s)]) < 80.0
            got = R.place(s, A0, R.draw_trunc(g, combo)) if ok else None
            if got is not None and 8 <= int(got[1].sum()) <= 64:
                break
        else:
            raise AssertionError(f"no placeable row with 8..64 survivors for stages {combo} at V = {V} in 400 draws")
        A = got[1]
        cfg = _cfg(n)
        context = [(3 * n + 1 + 7 * i) % V for i in range(cfg.ngram_len - 1)]
        ref = W.Cell(cfg)
        ref.w[4:4 + cfg.ngram_len - 1] = np.asarray(context, dtype=np.uint64)
        q, flags = ref.call(np.where(A, np.exp(np.where(A, s, 0.0) - s[A].max()), 0.0))
        assert flags == W.WATERMARKED
        for counter in range(64):
            want, dist, _ = W.pick(q, S.uniform24(SEED, counter, n))
            if dist >= SEAM:
                break
        ref.finish(want)
        cases.append(dict(row=row, T=T, top_k=k, top_p=p, allow=allow, penalty=pen, trunc=got[0], s=s, A=A, combo=combo, cfg=cfg,
                          context=context, q=q, counter=counter, want=want, seam=dist, after=ref.words()))
    _built[V] = cases
    return cases


def _logits(rows, V, ldl, dev):
    buf = torch.zeros((len(rows), ldl), dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(np.stack(rows))
    return buf.to(dev)[:, :V]


def _masks(cases, V, dev):
    from vitron_amd.sampling import allow_mask
    return [None if c["allow"] is None else torch.from_numpy(allow_mask(V, np.flatnonzero(c["allow"])).view(np.int32)).to(dev) for c in cases]


def _params(cases, hist_dev, dev, order=None, greedy=()):
    order = range(len(cases)) if order is None else order
    return _pack([_row(0.0 if n in greedy else cases[n]["T"], cases[n]["top_k"], cases[n]["top_p"], cases[n]["penalty"], SEED,
                       cases[n]["counter"], n, hist_dev if cases[n]["penalty"] != 1.0 else None) for n in order], dev)


def _live(cases, dev, order=None):
    """(the watermarks, fresh cells holding the cases' contexts, the packed vt_wm_row array) in `order`"""
    from vitron_amd.watermark import pack_wm_rows
    order = range(len(cases)) if order is None else order
    wms, cells = [], []
    for n in order:
        wm = _wm(cases[n]["cfg"])
        cell = wm.new_cell(dev)
        _seed_cell(cell, W.Cell(cases[n]["cfg"]), cases[n]["context"])
        wms.append(wm)
        cells.append(cell)
    return wms, cells, pack_wm_rows(list(zip(wms, cells)), dev)


def _bits(res):
    ids, kept, lp = res
    return ids.cpu().tolist(), kept.cpu().tolist(), lp.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("V,ldl", SHAPES)
def test_placed_cases_match_the_fp64_tournament(dev, V, ldl):
    from vitron_amd import ops
    from vitron_amd.sampling import pack_trunc_rows
    cases = _cases(V)
    assert len(cases) == ROWS and all(8 <= int(c["A"].sum()) <= 64 for c in cases)
    assert all(c["seam"] >= SEAM for c in cases), [c["seam"] for c in cases]             # such a counter exists for every row
    assert sorted({c["cfg"].depth for c in cases}) == list(DEPTHS)
    x = _logits([c["row"] for c in cases], V, ldl, dev)
    assert x.stride(0) == ldl
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    masks = _masks(cases, V, dev)
    trunc = pack_trunc_rows([c["trunc"] for c in cases], dev)
    wms, cells, wm_rows = _live(cases, dev)
    ids, kept, lp = ops.sample_rows(x, _params(cases, h, dev), return_kept=True, return_logprob=True, allow=masks, trunc=trunc,
                                    watermark=wm_rows)
    ids, kept, lp = ids.cpu().tolist(), kept.cpu().tolist(), lp.cpu().numpy()
    for n, c in enumerate(cases):
        print(f"V={V} row {n} stages {c['combo']} depth {c['cfg'].depth} ngram {c['cfg'].ngram_len} kept {kept[n]} / fp64 {int(c['A'].sum())} "
              f"id {ids[n]} / fp64 {c['want']} seam {c['seam']:.2e} q[want] {c['q'][c['want']]:.3e}")
    for n, c in enumerate(cases):
        assert kept[n] == int(c["A"].sum()), (V, n, kept[n], int(c["A"].sum()))          # the truncation's survivors
        assert 0 <= ids[n] < V and c["A"][ids[n]], (V, n, ids[n])
        assert ids[n] == c["want"], (V, n, c["combo"], ids[n], c["want"], c["seam"])
        assert np.array_equal(_words(cells[n]), c["after"]), (V, n)
    # the tournament moved the draw: the plain inverse CDF over the same survivors gives other ids for many rows
    plain = [W.pick(np.where(c["A"], np.exp(np.where(c["A"], c["s"], 0.0) - c["s"][c["A"]].max()), 0.0), S.uniform24(SEED, c["counter"], n))[0]
             for n, c in enumerate(cases)]
    assert sum(a != b for a, b in zip(plain, ids)) >= 4, (plain, ids)
    # logprob stays over the RAW row
    raw = np.stack([c["row"] for c in cases])
    ref = S.logprob_ref(raw)[np.arange(ROWS), ids]
    assert np.all(np.abs(lp.astype(np.float64) - ref) <= S.logprob_bound(raw, ids)), (V, lp, ref)
    # a row's result does not depend on its neighbours: the same rows in reverse order on fresh cells, every row with its own stream
    order = list(range(ROWS))[::-1]
    y = _logits([cases[n]["row"] for n in order], V, ldl, dev)
    _, cells2, wm_rows2 = _live(cases, dev, order)
    rev = ops.sample_rows(y, _params(cases, h, dev, order), return_kept=True, return_logprob=True, allow=[masks[n] for n in order],
                          trunc=pack_trunc_rows([cases[n]["trunc"] for n in order], dev), watermark=wm_rows2)
    assert [t[::-1] for t in _bits(rev)] == [ids, kept, lp.view(np.uint32).tolist()]
    assert all(np.array_equal(_words(cells2[i]), cases[n]["after"]) for i, n in enumerate(order))


@pytest.mark.parametrize("V,ldl", SHAPES)
def test_rows_without_a_watermark_are_bit_equal_to_the_truncating_sampler(dev, V, ldl):
    from vitron_amd import ops
    from vitron_amd.sampling import pack_trunc_rows
    from vitron_amd.watermark import pack_wm_rows
    cases = _cases(V)
    x = _logits([c["row"] for c in cases], V, ldl, dev)
    h = torch.tensor(_hist(V), dtype=torch.int32, device=dev)
    greedy = tuple(range(0, ROWS, 5))                                               # rows 0, 5, 10, 15 are greedy
    pr_all = _params(cases, h, dev, greedy=tuple(range(ROWS)))
    pr = _params(cases, h, dev, greedy=greedy)
    masks = _masks(cases, V, dev)
    g = torch.Generator().manual_seed(5 + V)
    adj = [None if n % 3 == 0 else (torch.randn((V, 2), generator=g) * 2.0).to(dev) for n in range(ROWS)]
    active = pack_trunc_rows([c["trunc"] for c in cases], dev)
    null = pack_wm_rows([None] * ROWS, dev)
    for allow, adjust, trunc in ((None, None, None), (masks, None, None), (None, adj, None), (masks, adj, active), (None, None, active)):
        kw = dict(return_kept=True, return_logprob=True, allow=allow, adjust=adjust, trunc=trunc)
        base = _bits(ops.sample_rows(x, pr, **kw))
        assert _bits(ops.sample_rows(x, pr, watermark=None, **kw)) == base
        assert _bits(ops.sample_rows(x, pr, watermark=null, **kw)) == base              # all-NULL cells
        # live cells on every row: the greedy rows ignore them and do not touch them, the sampled rows are watermarked
        _, cells, wm_rows = _live(cases, dev)
        for c in cells:
            c.zero_()
        got = _bits(ops.sample_rows(x, pr, watermark=wm_rows, **kw))
        for part, want in zip(got, base):
            assert [part[n] for n in greedy] == [want[n] for n in greedy]
        assert got[1] == base[1]                                                       # kept_count: the truncation's survivors
        assert all(not _words(cells[n]).any() for n in greedy)
        assert all(int(_words(cells[n])[0]) == 1 for n in range(ROWS) if n not in greedy)
        # every row greedy: the trunc launch's bits, every cell untouched
        base_g = _bits(ops.sample_rows(x, pr_all, **kw))
        _, cells, wm_rows = _live(cases, dev)
        for c in cells:
            c.zero_()
        assert _bits(ops.sample_rows(x, pr_all, watermark=wm_rows, **kw)) == base_g
        assert all(not _words(c).any() for c in cells)


STATE_COMBOS = [(ng, hs, skip) for ng in (2, 5) for hs in (2, 1024) for skip in (False, True)]


@pytest.mark.parametrize("V,ldl", ((1000, 1000), (32003, 32004)))
def test_cell_state_follows_the_restatement_over_twelve_launches(dev, V, ldl):
    """Row r runs combination r % 8 of (ngram_len, history size, skip_first). Rows 0..7 are forced to one token by a one-token allow mask
    (the context repeats as soon as it is full of it), rows 8, 10, .. to a cycle of three tokens (their contexts come back behind two
    others: found by the history of 1024, evicted from the history of 2), rows 9, 11, .. are free (top_k = 40)."""
    from vitron_amd import ops
    from vitron_amd.sampling import allow_mask
    from vitron_amd.watermark import pack_wm_rows
    g = torch.Generator().manual_seed(3 + V)
    x = (torch.randn((ROWS, ldl), generator=g) * 2.0).to(dev)[:, :V]
    cfgs = [W.Config(ng, W.KEYS30[:4], history_size=hs, skip_first=skip) for ng, hs, skip in (STATE_COMBOS[r % 8] for r in range(ROWS))]
    kinds = [0 if r < 8 else 1 + r % 2 for r in range(ROWS)]                       # 0: one token, 1: a cycle of three, 2: free
    wms = [_wm(c) for c in cfgs]
    cells = [w.new_cell(dev) for w in wms]
    refs = [W.Cell(c) for c in cfgs]
    wm_rows = pack_wm_rows(list(zip(wms, cells)), dev)
    forced = [None if kinds[r] == 2 else ([(17 * r + 5) % V] if kinds[r] == 0 else [(17 * r + 5) % V, 31, V - 1]) for r in range(ROWS)]
    one = {t: torch.from_numpy(allow_mask(V, [t]).view(np.int32)).to(dev) for f in forced if f is not None for t in f}
    seen_flags = set()
    for step in range(12):
        masks, want_tok = [], []
        for r in range(ROWS):
            t = forced[r]
            tok = None if t is None else t[step % len(t)]
            want_tok.append(tok)
            masks.append(None if tok is None else one[tok])
        pr = _pack([_row(1.0, 40, 1.0, 1.0, SEED, step, r) for r in range(ROWS)], dev)
        ids = ops.sample_rows(x, pr, allow=masks, watermark=wm_rows).cpu().tolist()
        for r in range(ROWS):
            assert 0 <= ids[r] < V and (want_tok[r] is None or ids[r] == want_tok[r]), (step, r, ids[r], want_tok[r])
            _, flags = refs[r].begin()
            refs[r].finish(ids[r])
            seen_flags.add((STATE_COMBOS[r % 8], flags))
            got = _words(cells[r])
            assert np.array_equal(got, refs[r].w), (step, r, STATE_COMBOS[r % 8], kinds[r], got[:12], refs[r].w[:12])
    for ng, hs, skip in STATE_COMBOS:                                               # every combination repeated and watermarked; skipped when asked
        assert ((ng, hs, skip), W.REPEATED) in seen_flags and ((ng, hs, skip), W.WATERMARKED) in seen_flags
        assert (((ng, hs, skip), W.SKIPPED) in seen_flags) == skip


def test_full_rows_land_in_the_fp64_interval(dev):
    """No truncation at V = 32003 (row stride 32004), depth 9, 16 streams on near-uniform rows"""
    from vitron_amd import ops
    from vitron_amd.watermark import pack_wm_rows
    V, ldl = 32003, 32004
    g = torch.Generator().manual_seed(77)
    rows = (torch.randn((ROWS, V), generator=g) * 0.1).numpy().astype(F32)
    x = _logits(list(rows), V, ldl, dev)
    cfg = W.Config(5, W.KEYS30[:9])
    wm = _wm(cfg)
    cells, refs = [wm.new_cell(dev) for _ in range(ROWS)], [W.Cell(cfg) for _ in range(ROWS)]
    for r in range(ROWS):
        _seed_cell(cells[r], refs[r], [(101 * r + 13 * i) % V for i in range(4)])
    pr = _pack([_row(1.0, 0, 1.0, 1.0, SEED, 3, r) for r in range(ROWS)], dev)
    ids, kept = ops.sample_rows(x, pr, return_kept=True, watermark=pack_wm_rows([(wm, c) for c in cells], dev))
    ids, kept = ids.cpu().tolist(), kept.cpu().tolist()
    assert kept == [V] * ROWS
    for r in range(ROWS):
        s = rows[r].astype(np.float64)
        q, flags = refs[r].call(np.exp(s - s.max()))
        assert flags == W.WATERMARKED
        c = np.cumsum(q) / q.sum()
        u = float(S.uniform24(SEED, 3, r))
        excl, incl = c[ids[r]] - q[ids[r]] / q.sum(), c[ids[r]]
        print(f"row {r}: id {ids[r]} interval [{excl:.6f}, {incl:.6f}] uniform {u:.6f} fp64 id {W.pick(q, u)[0]}")
        assert excl - SEAM <= u <= incl + SEAM, (r, ids[r], excl, incl, u)
        refs[r].finish(ids[r])
        assert np.array_equal(_words(cells[r]), refs[r].w)


def _find_context(cfg, V, ids, wanted):
    """A one-token-varied context whose g-values at `ids` are `wanted` (layer 0), found by search on the host"""
    n1 = cfg.ngram_len - 1
    for t in range(4096):
        context = [t % V] + [5] * (n1 - 1)
        if tuple(int(v) for v in cfg.g_next(cfg.context_hash(context), V)[list(ids), 0]) == tuple(wanted):
            return context
    raise AssertionError(f"no context gives g = {wanted} at {ids}")


def _counter_with_uniform(stream, lo, hi):
    for counter in range(4096):
        if lo < float(S.uniform24(SEED, counter, stream)) < hi:
            return counter
    raise AssertionError("no counter")


@pytest.mark.parametrize("V,ldl", ((1000, 1000), (32003, 32004)))
def test_exact_probes(dev, V, ldl):
    """Equal logits on the survivors, depth 1: (g, the uniform's window, the survivor the fp32-exact probabilities give there, and the
    one another g would give). (1, 0): (0.75, 0.25); (0, 1): (0.25, 0.75); equal g: (0.5, 0.5); (1, 0, 0, 0): (0.4375, 0.1875 x 3)."""
    from vitron_amd import ops
    from vitron_amd.watermark import pack_wm_rows
    probes = [((0, 31), (1, 0), (0.52, 0.73), 0), ((0, 31), (1, 1), (0.52, 0.73), 1), ((0, 31), (0, 0), (0.52, 0.73), 1),
              ((0, 31), (0, 1), (0.27, 0.48), 1), ((32, V - 1), (1, 0), (0.52, 0.73), 0), ((32, V - 1), (0, 1), (0.27, 0.48), 1),
              ((32, V - 1), (1, 1), (0.27, 0.48), 0), ((31, 32), (1, 0), (0.77, 0.98), 1), ((31, 32), (1, 0), (0.52, 0.73), 0),
              ((31, 32), (0, 1), (0.02, 0.23), 0), ((0, 31, 32, V - 1), (1, 0, 0, 0), (0.27, 0.42), 0),
              ((0, 31, 32, V - 1), (0, 0, 0, 1), (0.58, 0.73), 3), ((0, 31, 32, V - 1), (0, 0, 0, 0), (0.27, 0.48), 1),
              ((0, 31, 32, V - 1), (0, 1, 1, 0), (0.14, 0.235), 1), ((0, V - 1), (1, 0), (0.52, 0.73), 0), ((0, V - 1), (0, 1), (0.27, 0.48), 1)]
    assert len(probes) == ROWS
    cfg = W.Config(3, (654,))
    wm = _wm(cfg)
    rows, cells, params, want = [], [], [], []
    for r, (ids, gwant, (lo, hi), which) in enumerate(probes):
        row = np.full((V,), -20.0, dtype=F32)
        row[list(ids)] = 1.5
        rows.append(row)
        ref = W.Cell(cfg)
        cell = wm.new_cell(dev)
        _seed_cell(cell, ref, _find_context(cfg, V, ids, gwant))
        cells.append(cell)
        counter = _counter_with_uniform(r, lo, hi)
        params.append(_row(1.0, len(ids), 1.0, 1.0, SEED, counter, r))
        p = np.zeros((V,))
        p[list(ids)] = 1.0
        q, _ = ref.call(p)
        got, dist, _ = W.pick(q, S.uniform24(SEED, counter, r))
        assert got == ids[which] and dist >= 0.015, (r, got, ids, dist)           # the window is what the docstring says it is
        want.append(ids[which])
    out, kept = ops.sample_rows(_logits(rows, V, ldl, dev), _pack(params, dev), return_kept=True,
                                watermark=pack_wm_rows([(wm, c) for c in cells], dev))
    assert kept.cpu().tolist() == [len(p[0]) for p in probes]
    assert out.cpu().tolist() == want


def test_bad_calls(dev):
    from vitron_amd import _lib, ops
    from vitron_amd.sampling import _upload_rows
    from vitron_amd.watermark import WM_ROW_DTYPE, pack_wm_rows, wm_rows_array
    V = 64
    x = torch.zeros((2, V), dtype=torch.float32, device=dev)
    pr = _pack([_row(1.0, 0, 1.0, 1.0, 1, 0, 0), _row(1.0, 0, 1.0, 1.0, 1, 0, 1)], dev)
    cfg = W.Config(5, W.KEYS30[:9], history_size=8)
    wm = _wm(cfg)
    cells = [wm.new_cell(dev), wm.new_cell(dev)]
    good = pack_wm_rows([None, (wm, cells[1])], dev)
    ids = ops.sample_rows(x, pr, watermark=good).cpu().tolist()
    assert all(0 <= i < V for i in ids) and int(_words(cells[1])[0]) == 1 and not _words(cells[0]).any()
    # the tensor itself
    for bad in (good.cpu(), good[:1], good.to(torch.int32), good.t(), torch.zeros((2, 12), dtype=torch.float32, device=dev),
                np.zeros((2, 48), np.uint8), [None, None]):
        with pytest.raises(_lib.VitronHipError, match="watermark"):
            ops.sample_rows(x, pr, watermark=bad)
    # a misaligned array; the streaming form by size, by stride and by alignment
    shifted = torch.zeros((2 * 48 + 8,), dtype=torch.uint8, device=dev)[4:4 + 96]
    shifted.copy_(good.reshape(-1))
    with pytest.raises(_lib.VitronHipError, match="8-byte aligned"):
        ops.sample_rows(x, pr, watermark=shifted)
    with pytest.raises(_lib.VitronHipError, match="register form"):
        ops.sample_rows(torch.zeros((2, 33000), dtype=torch.float32, device=dev), pr, watermark=good)
    with pytest.raises(_lib.VitronHipError, match="register form"):
        ops.sample_rows(torch.zeros((2, 63), dtype=torch.float32, device=dev), pr, watermark=good)
    with pytest.raises(_lib.VitronHipError, match="register form"):
        ops.sample_rows(torch.zeros((2, 65), dtype=torch.float32, device=dev)[:, 1:], pr, watermark=good)
    # junk fields on a row with a cell are refused by name before the launch: the cell is not touched
    fields = wm.row_fields(cells[1])
    names = list(WM_ROW_DTYPE.names)
    for name, values in (("depth", (0, -1, 33, 2 ** 31 - 1)), ("table_size", (0, 16, 1000, 65537, 131072, -65536)),
                         ("ngram_len", (0, 1, 9, -5)), ("history_size", (0, -1, 4097, 2 ** 31 - 1)), ("reserved", (1, -1)),
                         ("layer_add", (0, fields[1] + 4)), ("table", (0, fields[2] + 2)), ("cell", (fields[0] + 4,))):
        for v in values:
            junk = list(fields)
            junk[names.index(name)] = v
            arr = _upload_rows(wm_rows_array([None, tuple(junk)]), dev)
            before = _words(cells[1]).copy()
            with pytest.raises(_lib.VitronHipError, match="vt_sample_rows_wm: wm\\[1\\]"):
                ops.sample_rows(x, pr, watermark=arr)
            assert np.array_equal(_words(cells[1]), before)
    # the same junk on a row WITHOUT a cell is not looked at: the bits of the plain launch
    base = ops.sample_rows(x, pr).cpu().tolist()
    arr = _upload_rows(wm_rows_array([(0, 0, 0, -7, 1000, 77, -1, 5, 9), (0, 123456, 8, 99, 3, 0, 0, 0, 1)]), dev)
    assert ops.sample_rows(x, pr, watermark=arr).cpu().tolist() == base
    # whatever a cell holds stays inside it: a head, a call count and context ids of random bits; any non-zero skip_first is on
    g = np.random.default_rng(9)
    for trial in range(4):
        junk_cell = g.integers(0, 2 ** 63, size=(wm.cell_words,), dtype=np.int64) * (1 if trial % 2 else -1)
        cells[1].copy_(torch.from_numpy(junk_cell))
        f = list(fields)
        f[names.index("skip_first")] = (0, 12345, -7, 1)[trial]
        ids = ops.sample_rows(x, pr, watermark=_upload_rows(wm_rows_array([None, tuple(f)]), dev)).cpu().tolist()
        w = _words(cells[1])
        assert 0 <= ids[1] < V and int(w[1]) < 8 and int(w[3]) in (1, 2, 4) and int(w[4 + 3]) == ids[1]
        assert int(w[0]) == (int(junk_cell.view(np.uint64)[0]) + 1) % 2 ** 64
