"""vt_sample_rows_miro through the C ABI of both builds' libraries: Mirostat v2 inside the per-row sampler. Checks:
  OFF       rows with tau <= 0, with a NULL cell and greedy rows with live cells return the ids, kept_count and logprob of
            vt_sample_rows_trunc bit for bit beside live rows; their cells keep every byte.
  KEEP-SET  every row's mu stands at the midpoint of a gap of the fp64 surprises wider than 4 surprise bounds (asserted on the CPU before
            the launch, no case skipped): kept_count and the id equal tests/miro_ref.py's, which takes the same uniform; the uniform is
            kept 1e-4 of the mass from a seam of the fp64 CDF. The cell: e within surprise_bound of fp64, mu' bit for bit
            mu - eta * (e - tau) in unfused fp32 from the kernel's own e.
  PROBES    mu below every surprise (and -inf, NaN): the arg-max alone, the first index on a tie; mu above every surprise (and +inf):
            vt_sample_rows_trunc's id and kept_count; plateaus of equal logits leave or stay together.
  TRAJECTORY 64 launches, 4 + 4 rows, V = 4096, the cell carried by the kernel alone. Step by step, from the kernel's own mu: kept_count
            between the fp64 counts at mu -/+ bound, the id inside the fp64 keep-set at mu + bound, e and mu' inside the bounds of the
            fp64 update. Over the whole run: the fp64 trajectory replayed with the kernel's ids, kept as an interval (a step at which a
            token's surprise lies within the bound of the cutoff has two fp64 answers, and both are followed), contains the kernel's mu
            after every step; where no token ever straddled, its width is the steps' mu_bound and nothing else.
  STAGES    allow mask, adjustment and truncation in front, each alone and all together.
  BAD CALLS the streaming-form refusal and the argument refusals, each with its message, nothing launched.
  CAPTURE   one launch captured into a graph and replayed once: the array is not read back there, so the entries the launcher would have
            refused (a NaN tau, an infinite or negative eta, a misaligned cell) reach the kernel, which returns vt_sample_rows_trunc's
            bits for them and leaves their cells alone; the good rows beside them are the restatement's.
Shapes (V, row stride, rows): (64, 64, 1), (1000, 1004, 5), (4096, 4096, 16), (32000, 32004, 5), (32768, 32768, 16)."""
import numpy as np
import pytest
import torch

from tests import miro_ref as M
from tests import sample_ref as S
from tests import trunc_ref as R
from tests.allow_cases import pack as _pack, row as _row

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = ((64, 64, 1), (1000, 1004, 5), (4096, 4096, 16), (32000, 32004, 5), (32768, 32768, 16))
SEED = 31
SEAM = 1e-4
TAUS = (3.0, 5.0, 2.5, 4.0)
ETAS = (0.1, 0.25, 0.05, 1.0)


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def lib(request):
    from vitron_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load(operand=request.param)


DEV = torch.device("cuda:0")


def _logits(rows, V, ldl):
    buf = torch.zeros((len(rows), ldl), dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(np.stack(rows).astype(F32))
    return buf.to(DEV)[:, :V]


def _miro_array(entries):
    """The device vt_miro_row array from raw (cell address, tau, eta) triples, unvalidated (the bad calls need bad values)"""
    from vitron_amd.sampling import MIRO_ROW_DTYPE, _upload_rows
    a = np.zeros((len(entries),), dtype=MIRO_ROW_DTYPE)
    for i, (c, tau, eta) in enumerate(entries):
        a[i] = (int(c), F32(tau), F32(eta))
    return _upload_rows(a, DEV)


def _call(lib, x, params, miro=None, allow=None, adjust=None, trunc=None, status=0):
    """One launch through the C ABI: vt_sample_rows_miro with `miro`, else vt_sample_rows_trunc. Returns (ids, kept, logprob bits), or
    the library's message when `status` is the refusal that is expected."""
    from vitron_amd import _lib, ops
    rows, V = x.shape
    ids = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lp = torch.zeros((rows,), dtype=torch.float32, device=DEV)
    ap = None if allow is None else ops.allow_pointers(allow, rows, V, DEV)
    jp = None if adjust is None else ops.adjust_pointers(adjust, rows, V, DEV)
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    if miro is None:
        got = lib.vt_sample_rows_trunc(p(x), rows, V, x.stride(0), p(params), p(ap), p(jp), p(trunc), p(ids), p(kept), p(lp), st)
    else:
        got = lib.vt_sample_rows_miro(p(x), rows, V, x.stride(0), p(params), p(ap), p(jp), p(trunc), p(miro), p(ids), p(kept), p(lp), st)
    torch.cuda.synchronize()
    assert got == status, (got, _lib.last_error(lib))
    if status != 0:
        assert ids.cpu().tolist() == [-7] * rows and kept.cpu().tolist() == [-7] * rows            # nothing was launched
        return _lib.last_error(lib)
    return ids.cpu().tolist(), kept.cpu().tolist(), lp.cpu().numpy().view(np.uint32).tolist()


def _step_f32(mu, eta, e, tau):
    """mu - eta * (e - tau) with every operation rounded to fp32 on its own"""
    with np.errstate(all="ignore"):
        d = F32(F32(e) - F32(tau))
        return F32(F32(mu) - F32(F32(eta) * d))


_built = {}


def _cases(V, rows, stages=False):
    """`rows` placed cases at vocabulary V, built once and never modified. Every case: a drawn row behind top-k / top-p (stages=True: an
    allow mask, an adjustment and truncation stages in front, each alone and all together, case by case), mu at the midpoint of a gap of
    the fp64 surprises wider than four bounds (miro_ref.place_mu asserts it), and a counter whose uniform stays SEAM off the seams."""
    key = (V, rows, stages)
    if key in _built:
        return _built[key]
    g = np.random.default_rng(11 * 1000003 + V + 17 * stages)
    hist = [0, 31, 32, V - 1, 7, 5, -200, V + 3] + g.integers(0, V, 100).tolist()
    cases = []
    for n in range(rows):
        kind = ("allow", "adjust", "trunc", "all")[n % 4] if stages else "plain"
        for attempt in range(400):
            row, T, k, p = R.draw_row(g, V)
            allow = (g.random(V) < 0.6) if kind in ("allow", "all") else None
            pen = 1.3 if (kind == "all" or (not stages and n % 3 == 2)) else 1.0
            adj = None
            x = row
            if kind in ("adjust", "all"):            # (pre, post): pre before the penalty, post behind it, each addition rounded to fp32
                adj = np.zeros((V, 2), dtype=F32)
                at = g.integers(0, V, 40)
                adj[at, 0] = g.normal(0, 2, 40).astype(F32)
                adj[g.integers(0, V, 40), 1] = -g.uniform(0.1, 2, 40).astype(F32)
                x = (row + adj[:, 0]).astype(F32)
                if pen != 1.0:
                    x = S.repetition_penalty(x, hist, pen)
                x = (x + adj[:, 1]).astype(F32)
                s = R.scaled(x, T, allow)
            else:
                s = R.scaled(row, T, allow, pen, hist)
            A = R.base_keep(s, k, p)
            ok = R.top_p_margin(s, k, p) >= 1e-4 and np.ptp(s[np.isfinite(s)]) < 80.0
            trunc = R.OFF
            if ok and kind in ("trunc", "all"):
                got = R.place(s, A, R.draw_trunc(g, R.COMBOS[(n // 4) % len(R.COMBOS)]))
                ok = got is not None
                if ok:
                    trunc, A = got
            if ok and int(A.sum()) >= 4:
                break
        else:
            raise AssertionError(f"no placeable row for case {n} at V = {V}")
        mu, K = M.place_mu(s, A, int(g.integers(1, min(40, int(A.sum()) - 1) + 1)))
        tau, eta = TAUS[n % 4], ETAS[n % 4]
        for counter in range(64):
            r = M.step(s, A, mu, tau, eta, float(S.uniform24(SEED, counter, n)))
            if r["seam"] >= SEAM:
                break
        assert r["seam"] >= SEAM and np.array_equal(r["K"], K)
        cases.append(dict(row=row, T=T, top_k=k, top_p=p, allow=allow, penalty=pen, adj=adj, trunc=trunc, s=s, A=A, mu=mu, K=K, tau=tau,
                          eta=eta, counter=counter, want=r, kind=kind, M=float(np.abs(s[A]).max())))
    _built[key] = (cases, hist)
    return _built[key]


def _inputs(cases, hist, V, ldl, greedy=()):
    from vitron_amd.sampling import allow_mask, pack_trunc_rows
    x = _logits([c["row"] for c in cases], V, ldl)
    h = torch.tensor(hist, dtype=torch.int32, device=DEV)
    params = _pack([_row(0.0 if n in greedy else c["T"], c["top_k"], c["top_p"], c["penalty"], SEED, c["counter"], n,
                         h if c["penalty"] != 1.0 else None) for n, c in enumerate(cases)], DEV)
    allow = [None if c["allow"] is None else torch.from_numpy(allow_mask(V, np.flatnonzero(c["allow"])).view(np.int32)).to(DEV) for c in cases]
    adjust = [None if c["adj"] is None else torch.from_numpy(c["adj"]).to(DEV).contiguous() for c in cases]
    trunc = pack_trunc_rows([c["trunc"] for c in cases], DEV)
    extra = dict(allow=allow if any(a is not None for a in allow) else None, adjust=adjust if any(a is not None for a in adjust) else None,
                 trunc=trunc if any(c["trunc"] != R.OFF for c in cases) else None)
    return x, params, extra, h


def _cells(cases):
    return torch.tensor([[c["mu"], 0.25] for c in cases], dtype=torch.float32).to(DEV)


def _check_live(cases, got, cells_after, V, rows_live=None):
    ids, kept, _ = got
    after = cells_after.cpu().numpy()
    for n, c in enumerate(cases):
        if rows_live is not None and n not in rows_live:
            continue
        w = c["want"]
        print(f"V={V} row {n} {c['kind']} kept {kept[n]} / fp64 {w['count']} of {int(c['A'].sum())} id {ids[n]} / fp64 {w['id']} mu {c['mu']:.5f} "
              f"e {after[n, 1]:.6f} / fp64 {w['e']:.6f} (bound {M.surprise_bound(c['M'], w['e'], True):.2e}) seam {w['seam']:.1e}")
    for n, c in enumerate(cases):
        if rows_live is not None and n not in rows_live:
            continue
        w = c["want"]
        assert kept[n] == w["count"], (V, n, kept[n], w["count"])
        assert ids[n] == w["id"], (V, n, ids[n], w["id"])
        assert abs(float(after[n, 1]) - w["e"]) <= M.surprise_bound(c["M"], w["e"], observed_e=True), (V, n, after[n, 1], w["e"])
        want_mu = _step_f32(c["mu"], c["eta"], after[n, 1], c["tau"])
        assert after[n, 0].view(np.uint32) == want_mu.view(np.uint32), (V, n, after[n, 0], want_mu)


# ---- KEEP-SET and the cell ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl,rows", SHAPES)
def test_placed_cutoffs_match_the_restatement(lib, V, ldl, rows):
    cases, hist = _cases(V, rows)
    x, params, extra, h = _inputs(cases, hist, V, ldl)
    assert x.stride(0) == ldl
    cells = _cells(cases)
    miro = _miro_array([(cells[n].data_ptr(), c["tau"], c["eta"]) for n, c in enumerate(cases)])
    got = _call(lib, x, params, miro, **extra)
    _check_live(cases, got, cells, V)
    # logprob stays over the RAW row: the one vt_sample_rows_trunc reports for the same id would be the same expression; hold it to fp64
    lp = np.asarray(got[2], dtype=np.uint32).view(F32)
    for n, c in enumerate(cases):
        raw = c["row"].astype(np.float64)
        want = raw[got[0][n]] - (raw.max() + np.log(np.exp(raw - raw.max()).sum()))
        assert abs(float(lp[n]) - want) <= 1e-4, (V, n, lp[n], want)


# ---- OFF ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl,rows", SHAPES[1:])
def test_off_rows_are_the_trunc_launch_bit_for_bit(lib, V, ldl, rows):
    """Row n: n % 5 == 0 live; 1 tau = 0 with a cell; 2 a NULL cell; 3 greedy with a live cell; 4 tau < 0 with a cell"""
    cases, hist = _cases(V, rows)
    greedy = {n for n in range(rows) if n % 5 == 3}
    x, params, extra, h = _inputs(cases, hist, V, ldl, greedy=greedy)
    cells = _cells(cases)
    before = cells.cpu().numpy().tobytes()
    entries = []
    for n, c in enumerate(cases):
        tau = {0: c["tau"], 1: 0.0, 2: c["tau"], 3: c["tau"], 4: -1.0}[n % 5]
        entries.append((0 if n % 5 == 2 else cells[n].data_ptr(), tau, c["eta"]))
    plain = _call(lib, x, params, None, **dict(extra, trunc=extra["trunc"]))
    got = _call(lib, x, params, _miro_array(entries), **extra)
    after = cells.cpu().numpy()
    off = [n for n in range(rows) if n % 5 != 0]
    for n in off:
        assert (got[0][n], got[1][n], got[2][n]) == (plain[0][n], plain[1][n], plain[2][n]), (V, n)
        assert after[n].tobytes() == np.frombuffer(before, F32).reshape(rows, 2)[n].tobytes(), (V, n)      # untouched, byte for byte
    assert all(plain[1][n] == 1 for n in greedy)
    _check_live(cases, got, cells, V, rows_live={n for n in range(rows) if n % 5 == 0})
    # all rows off: the whole launch equals the trunc launch
    allnull = _call(lib, x, params, _miro_array([(0, c["tau"], c["eta"]) for c in cases]), **extra)
    assert allnull == plain


# ---- PROBES -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl", [(1000, 1004), (32768, 32768)])
def test_probes(lib, V, ldl):
    g = np.random.default_rng(V)
    tie = (g.standard_normal(V) * 2).astype(F32)
    hi = float(tie.max()) + 3.0
    a, b = sorted(g.choice(V, 2, replace=False).tolist())
    tie[[a, b]] = hi                                   # two equal maxima: the first index survives alone
    plateau = np.full((V,), -30.0, dtype=F32)          # plateaus of 1, 2 and 3 equal logits, then far below
    where = g.choice(V, 6, replace=False)
    plateau[where] = np.asarray([5, 4, 4, 2, 2, 2], dtype=F32)
    s_pl = plateau.astype(np.float64)
    A_pl = np.ones(V, dtype=bool)
    _, sv = M.surprises(s_pl, A_pl)
    lv = np.unique(sv[where])                          # the three plateau surprises
    far = float(np.unique(sv)[-1])
    mus_pl = [float(F32(0.5 * (lv[0] + lv[1]))), float(F32(0.5 * (lv[1] + lv[2]))), float(F32(0.5 * (lv[2] + far)))]
    rows = [tie] * 8 + [plateau] * 6
    mus = [-1.0, -np.inf, np.nan, 0.0, 1e9, np.inf, 1e9, np.inf] + mus_pl + mus_pl
    x = _logits(rows, V, ldl)
    params = _pack([_row(1.0, 0, 1.0, 1.0, SEED, n, n, None) for n in range(len(rows))], DEV)
    cells = torch.tensor([[m, 0.0] for m in mus], dtype=torch.float32).to(DEV)
    miro = _miro_array([(cells[n].data_ptr(), 3.0, 0.1) for n in range(len(rows))])
    plain = _call(lib, x, params, None)
    ids, kept, lp = _call(lib, x, params, miro)
    after = cells.cpu().numpy()
    for n in range(4):                                 # below every surprise, -inf, NaN, 0 (< the maxima's surprise of >= 1 bit)
        assert (ids[n], kept[n]) == (a, 1), (n, ids[n], kept[n], a, b)
        assert after[n, 1] == 0.0                      # alone: q_x / kept2 = 1, e = 0 exactly
        assert after[n, 0].view(np.uint32) == _step_f32(mus[n], 0.1, 0.0, 3.0).view(np.uint32) or (np.isnan(after[n, 0]) and np.isnan(mus[n]))
    for n in range(4, 8):                              # above every surprise: the trunc launch's id and kept_count
        assert (ids[n], kept[n]) == (plain[0][n], plain[1][n]) and kept[n] == V, (n, ids[n], kept[n])
        assert lp[n] == plain[2][n]
    for n, want in zip(range(8, 14), (1, 3, 6, 1, 3, 6)):     # equal probabilities leave or stay together
        assert kept[n] == want and ids[n] in set(where[:want].tolist()), (n, kept[n], want, ids[n])
    assert np.isfinite(after[8:, :]).all()


# ---- TRAJECTORY ---------------------------------------------------------------------------------------------------------------------------
def test_trajectory_the_cell_carried_by_the_kernel(lib):
    V, steps = 4096, 64
    cases, hist = _cases(V, 16)
    # four rows as they come (the step-by-step checks) and the first four with at most 200 survivors behind top-k / top-p: there the
    # fp64 surprises lie about 0.05 bit apart, a cutoff within a bound of one is rare, and the whole-run interval below stays narrow
    # (with all 4096 tokens alive a token straddles mu every few steps and the interval only says so)
    sparse = [c for c in cases[4:] if int(c["A"].sum()) <= 200][:4]
    assert len(sparse) == 4
    cases = cases[:4] + sparse
    rows = len(cases)
    x, _, extra, h = _inputs(cases, hist, V, V)
    cells = torch.tensor([[2.0 * c["tau"], 0.0] for c in cases], dtype=torch.float32).to(DEV)
    miro = _miro_array([(cells[n].data_ptr(), c["tau"], c["eta"]) for n, c in enumerate(cases)])
    surp = [M.surprises(c["s"], c["A"]) for c in cases]
    lo = [2.0 * c["tau"] for c in cases]               # the fp64 trajectory replayed with the kernel's ids, as an interval
    hi = list(lo)
    straddles = [0] * rows
    r_sum = [0.0] * rows
    for st in range(steps):
        params = _pack([_row(c["T"], c["top_k"], c["top_p"], c["penalty"], SEED, st, n, h if c["penalty"] != 1.0 else None)
                        for n, c in enumerate(cases)], DEV)
        before = cells.cpu().numpy().copy()
        ids, kept, _ = _call(lib, x, params, miro, **extra)
        after = cells.cpu().numpy()
        for n, c in enumerate(cases):
            q, sv = surp[n]
            mu_k, xk, tau, eta = float(before[n, 0]), ids[n], float(F32(c["tau"])), float(F32(c["eta"]))
            sb = M.surprise_bound(c["M"], abs(mu_k) + 1.0)
            K_lo, K_hi = M.keep(c["s"], c["A"], mu_k - sb), M.keep(c["s"], c["A"], mu_k + sb)
            assert K_lo.sum() <= kept[n] <= K_hi.sum(), (st, n, int(K_lo.sum()), kept[n], int(K_hi.sum()))
            assert K_hi[xk], (st, n, xk)
            me = np.arange(V) == xk
            e_lo, e_hi = M.observed(q, K_lo | me, xk), M.observed(q, K_hi, xk)
            eb = M.surprise_bound(c["M"], e_hi, observed_e=True)
            e_k = float(after[n, 1])
            assert e_lo - eb <= e_k <= e_hi + eb, (st, n, e_lo, e_k, e_hi, eb)
            assert after[n, 0].view(np.uint32) == _step_f32(before[n, 0], c["eta"], after[n, 1], c["tau"]).view(np.uint32), (st, n)
            r = M.mu_step_bound(eta, eb, max(abs(e_lo - tau), abs(e_hi - tau)), 0.0, max(abs(mu_k), abs(float(after[n, 0]))))
            assert mu_k - eta * (e_hi - tau) - r <= float(after[n, 0]) <= mu_k - eta * (e_lo - tau) + r, (st, n)
            # the whole run: the cutoffs of the fp64 replay (kept as an interval where a token straddles mu) contain the kernel's
            J_lo, J_hi = M.keep(c["s"], c["A"], lo[n] - sb) | me, M.keep(c["s"], c["A"], hi[n] + sb) | me
            straddles[n] += int(J_lo.sum() != J_hi.sum())
            f_lo, f_hi = M.observed(q, J_lo, xk), M.observed(q, J_hi, xk)
            rr = M.mu_step_bound(eta, eb, max(abs(f_lo - tau), abs(f_hi - tau)), 0.0, max(abs(lo[n]), abs(hi[n])))
            r_sum[n] += rr
            lo[n], hi[n] = lo[n] - eta * (f_hi - tau) - rr, hi[n] - eta * (f_lo - tau) + rr
            assert lo[n] <= float(after[n, 0]) <= hi[n], (st, n, lo[n], float(after[n, 0]), hi[n])
    width = [hi[n] - lo[n] for n in range(rows)]
    print(f"trajectory: {steps} steps, final mu {cells.cpu().numpy()[:, 0].tolist()}, interval widths {width}, straddling steps {straddles}, "
          f"the steps' rounding bounds summed {r_sum}, survivors {[int(c['A'].sum()) for c in cases]}")
    for n in range(rows):          # where no token ever straddled the cutoff the interval is the n steps' mu_bound and nothing else
        if straddles[n] == 0:
            assert width[n] <= 2.0 * r_sum[n] * (1 + 1e-9) and r_sum[n] <= M.mu_bound(steps, 1.0, 2e-4, 64.0, 200.0), (n, width[n], r_sum[n])


# ---- STAGES -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl", [(1000, 1004), (32768, 32768)])
def test_with_allow_adjust_and_trunc_in_front(lib, V, ldl):
    cases, hist = _cases(V, 8, stages=True)
    assert [c["kind"] for c in cases[:4]] == ["allow", "adjust", "trunc", "all"]
    x, params, extra, h = _inputs(cases, hist, V, ldl)
    assert all(v is not None for v in extra.values())
    cells = _cells(cases)
    miro = _miro_array([(cells[n].data_ptr(), c["tau"], c["eta"]) for n, c in enumerate(cases)])
    _check_live(cases, _call(lib, x, params, miro, **extra), cells, V)
    for only in ("allow", "adjust", "trunc"):          # each array alone with the rows it shapes (the others NULL)
        sub = [n for n, c in enumerate(cases) if c["kind"] == only]
        subcases = [cases[n] for n in sub]
        xs, _, ex, _ = _inputs(subcases, hist, V, ldl)
        ps = _pack([_row(c["T"], c["top_k"], c["top_p"], c["penalty"], SEED, c["counter"], n, None) for n, c in zip(sub, subcases)], DEV)
        assert [k for k, v in ex.items() if v is not None] == [only]
        cs = _cells(subcases)
        ms = _miro_array([(cs[i].data_ptr(), c["tau"], c["eta"]) for i, c in enumerate(subcases)])
        got = _call(lib, xs, ps, ms, **ex)
        after = cs.cpu().numpy()
        for i, c in enumerate(subcases):
            assert (got[0][i], got[1][i]) == (c["want"]["id"], c["want"]["count"]), (only, i)
            assert abs(float(after[i, 1]) - c["want"]["e"]) <= M.surprise_bound(c["M"], c["want"]["e"], True)


# ---- CAPTURE ------------------------------------------------------------------------------------------------------------------------------
def test_captured_launch_treats_a_bad_entry_as_a_row_without_mirostat(lib):
    """Rows 0 and 5 good; 1 tau = NaN; 2 eta = inf; 3 eta < 0; 4 the cell 4 bytes off its alignment. Everything is allocated in front of
    the capture; the graph is one kernel node."""
    from vitron_amd import _lib
    V, ldl, rows = 1000, 1004, 6
    cases, hist = _cases(V, 5)
    cases = list(cases) + [cases[0]]
    x, params, extra, h = _inputs(cases, hist, V, ldl)
    assert extra["allow"] is None and extra["adjust"] is None and extra["trunc"] is None
    plain = _call(lib, x, params, None)
    spare = torch.tensor([[c["mu"], 0.25, 7.0] for c in cases], dtype=torch.float32).to(DEV)        # row 4's cell: 12-byte rows, + 4
    cells = _cells(cases)
    before = cells.cpu().numpy().copy()
    entries = [(cells[n].data_ptr(), c["tau"], c["eta"]) for n, c in enumerate(cases)]
    entries[1] = (cells[1].data_ptr(), np.nan, 0.1)
    entries[2] = (cells[2].data_ptr(), 3.0, np.inf)
    entries[3] = (cells[3].data_ptr(), 3.0, -0.5)
    entries[4] = (spare[0].data_ptr() + 4, 3.0, 0.1)
    assert entries[4][0] % 8 == 4
    miro = _miro_array(entries)
    assert "miro[1].tau" in _call(lib, x, params, miro, status=-1)                # outside a capture the launcher refuses the array
    ids = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lp = torch.zeros((rows,), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = lib.vt_sample_rows_miro(x.data_ptr(), rows, V, ldl, params.data_ptr(), None, None, None, miro.data_ptr(), ids.data_ptr(),
                                         kept.data_ptr(), lp.data_ptr(), side.cuda_stream)
    assert st == 0, _lib.last_error(lib)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert ids.cpu().tolist() == [-7] * rows and cells.cpu().numpy().tobytes() == before.tobytes()      # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = (ids.cpu().tolist(), kept.cpu().tolist(), lp.cpu().numpy().view(np.uint32).tolist())
    after = cells.cpu().numpy()
    for n in (1, 2, 3, 4):
        assert (got[0][n], got[1][n], got[2][n]) == (plain[0][n], plain[1][n], plain[2][n]), n
        assert after[n].tobytes() == before[n].tobytes(), n
    assert spare.cpu().numpy().tobytes() == np.asarray([[c["mu"], 0.25, 7.0] for c in cases], dtype=F32).tobytes()
    cases[5] = dict(cases[5], want=M.step(cases[5]["s"], cases[5]["A"], cases[5]["mu"], cases[5]["tau"], cases[5]["eta"],
                                          float(S.uniform24(SEED, cases[5]["counter"], 5))))
    if cases[5]["want"]["seam"] >= SEAM:               # (row 5 repeats row 0's case on stream 5: its uniform is another one)
        _check_live(cases, got, cells, V, rows_live={0, 5})
    else:
        _check_live(cases, got, cells, V, rows_live={0})


# ---- BAD CALLS ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(lib):
    V = 1000
    cases, hist = _cases(V, 5)
    x, params, extra, h = _inputs(cases, hist, V, 1004)
    cells = _cells(cases)
    before = cells.cpu().numpy().tobytes()
    good = [(cells[n].data_ptr(), c["tau"], c["eta"]) for n, c in enumerate(cases)]

    def bad(row, entry):
        e = list(good)
        e[row] = entry
        return _miro_array(e)
    c2 = cells[2].data_ptr()
    for miro, needle in ((bad(2, (c2 + 4, 3.0, 0.1)), "miro[2]: cell must be 8-byte aligned"),
                         (bad(1, (cells[1].data_ptr(), np.nan, 0.1)), "miro[1].tau"),
                         (bad(1, (cells[1].data_ptr(), np.inf, 0.1)), "miro[1].tau"),
                         (bad(3, (cells[3].data_ptr(), 3.0, np.nan)), "miro[3].eta"),
                         (bad(3, (cells[3].data_ptr(), 3.0, np.inf)), "miro[3].eta"),
                         (bad(4, (cells[4].data_ptr(), 3.0, -0.5)), "miro[4].eta")):
        assert needle in _call(lib, x, params, miro, status=-1, **extra)
    spare = torch.zeros((6 * 4 + 1,), dtype=torch.int32, device=DEV)          # the array itself off its 8-byte alignment
    assert "miro must be 8-byte aligned" in _call(lib, x, params, spare.data_ptr() + 4, status=-1, **extra)
    # a NULL cell hides its other fields
    ok = _call(lib, x, params, bad(1, (0, np.nan, -1.0)), **extra)
    assert ok[0][1] >= 0
    cells = _cells(cases)
    good_miro = _miro_array([(cells[n].data_ptr(), c["tau"], c["eta"]) for n, c in enumerate(cases)])
    before = cells.cpu().numpy().tobytes()
    # the streaming form: by size, by stride, by alignment
    big = _logits([np.zeros(40000, F32)] * 5, 40000, 40000)
    assert "Mirostat runs in the register form only" in _call(lib, big, params, good_miro, status=-1)
    odd = _logits([c["row"] for c in cases], V, 1001)
    assert "Mirostat runs in the register form only" in _call(lib, odd, params, good_miro, status=-1)
    flat = torch.zeros((5 * 1004 + 4,), dtype=torch.float32, device=DEV)
    off4 = flat[1:1 + 5 * 1004].view(5, 1004)[:, :V]
    assert off4.data_ptr() % 16 == 4
    assert "Mirostat runs in the register form only" in _call(lib, off4, params, good_miro, status=-1)
    assert cells.cpu().numpy().tobytes() == before                            # no refused call touched a cell
    from vitron_amd import _lib, ops
    from vitron_amd.sampling import pack_miro_rows
    with pytest.raises(_lib.VitronHipError, match="not built"):
        ops.sample_rows(x, params, miro=pack_miro_rows([(cells[n], 3.0, 0.1) for n in range(5)], DEV),
                        watermark=torch.zeros((5, 48), dtype=torch.uint8, device=DEV))
