"""vt_unit_rows and vt_contrast_rows through ops.unit_rows / ops.contrast_rows against tests/contrast_ref.py, both
builds: unit_rows per element inside an fp64 bound; exact probes of contrast_rows (one-hot bank rows, one- or two-hot candidates: every dot
product is exact, so `d` is compared bit for bit) with the maximum planted at every bank position around the kernel's 16-row chunk; the
random cases of tests/contrast_cases.py inside their bounds with the exact selection on ALL of them (tests/test_contrast_ref_host.py
proves their gaps); ties, alpha = 0, the append, the refusals."""
import os

import numpy as np
import pytest
import torch

from tests import contrast_cases as CC
from tests import contrast_ref as R
from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
F32 = np.float32
DT = pytest.mark.parametrize("dt", CC.DTYPES, ids=["bf16", "fp16"])
NAN_BITS = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}
GUARD = -12345.5
CHUNK = 16


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _report(what, err, bound):
    out = os.environ.get("VT_TOL_REPORT")
    if out:
        with open(out, "a") as fh:
            fh.write(f"bound {what}\t{float((err / np.maximum(bound, 1e-300)).max()):.6e}\n")


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


# ---- unit_rows ---------------------------------------------------------------------------------------------------------------------------
_unit_in = {}


def _unit_inputs(H, rows):
    if (H, rows) not in _unit_in:
        g = torch.Generator().manual_seed(9100 + H + rows)
        x = torch.randn((rows, H), generator=g) * torch.exp(torch.randn((rows, 1), generator=g) * 2.0)      # rows of very different norms
        x[rows // 2] = 0.0                                                                                  # a zero row
        w = 1.0 + 0.5 * torch.randn((H,), generator=g)
        _unit_in[(H, rows)] = (x, w)
    return _unit_in[(H, rows)]


@DT
@pytest.mark.parametrize("with_w", (False, True), ids=["w_null", "w"])
@pytest.mark.parametrize("pad", (0, 12), ids=["dense", "padded_ldx"])
@pytest.mark.parametrize("H", (64, 256, 4096, 100, 4100, 8192))
def test_unit_rows_against_fp64(dev, dt, H, pad, with_w):
    """Per element within store_half_ulp(ref) + |ref| (H + 8) 2^-24: the fp32 sum of H squares, the rsqrt and two products are orders
    below an operand ulp, so only a rounding boundary can differ. H = 100 (not a multiple of 4) and H > 4096 take the re-read form."""
    from vitron_amd import ops
    rows = 5
    x, w = _unit_inputs(H, rows)
    buf = torch.full((rows, H + pad), 7.0)
    buf[:, :H] = x
    xd = buf.to(dev)[:, :H]
    wd = w.to(dev) if with_w else None
    out_buf = torch.full((rows, H + pad), 3.0, dtype=dt, device=dev)
    got = ops.unit_rows(xd, wd, out=out_buf[:, :H])
    torch.cuda.synchronize()
    assert got.data_ptr() == out_buf.data_ptr()
    ref = R.unit_rows(x.numpy(), w.numpy() if with_w else None)
    bound = G.store_half_ulp(torch.from_numpy(ref), dt).numpy() + np.abs(ref) * (H + 8) * 2.0 ** -24
    g = out_buf[:, :H].float().cpu().numpy().astype(np.float64)
    err = np.abs(g - ref)
    assert (err <= bound).all(), (H, float((err / bound).max()))
    _report(f"unit_rows {G.FMT[dt]} H={H}", err, bound)
    assert (g[rows // 2] == 0.0).all()                                                       # the zero row gives zeros, not NaN
    if pad:
        assert (out_buf[:, H:].float() == 3.0).all()                                         # nothing behind a row is written
    fresh = ops.unit_rows(xd, wd, dtype=dt)                                                  # the allocating form: the same bits
    assert np.array_equal(_bits(fresh), _bits(out_buf[:, :H].contiguous()))


# ---- contrast_rows: the harness ---------------------------------------------------------------------------------------------------------------
def launch(dev, dt, groups, H, cand_pad=0, extra_rows=2):
    """One ops.contrast_rows launch over `groups` (dicts with bank fp32 [T, H], cand fp32 [k, H], lp, alpha -- values representable in dt).
    The banks get extra_rows rows behind row T; every bank row from T on is filled with NaN bit patterns. Returns per group
    (d [16], score [16], sel, bank bits [T + 1 + extra_rows, H] after the launch) and the candidates' bits."""
    from vitron_amd import ops
    n_cand = sum(g["cand"].shape[0] for g in groups)
    cand_buf = torch.zeros((n_cand + 1, H + cand_pad), dtype=dt)
    first, at = [], 0
    for g in groups:
        k = g["cand"].shape[0]
        cand_buf[at:at + k, :H] = torch.from_numpy(g["cand"]).to(dt)
        first.append(at)
        at += k
    cand_dev = cand_buf.to(dev)[:n_cand, :H]
    specs, banks = [], []
    d = torch.full((len(groups), 16), GUARD, dtype=torch.float32, device=dev)
    sc = torch.full((len(groups), 16), GUARD, dtype=torch.float32, device=dev)
    sel = torch.full((len(groups),), -7, dtype=torch.int32, device=dev)
    for i, g in enumerate(groups):
        T, k = g["bank"].shape[0], g["cand"].shape[0]
        bank = torch.full((T + 1 + extra_rows, H), NAN_BITS[dt], dtype=torch.int16).view(dt)
        bank[:T] = torch.from_numpy(g["bank"]).to(dt)
        bank = bank.to(dev)
        banks.append(bank)
        specs.append(dict(bank=bank, bank_len=T, k=k, first=first[i], alpha=g["alpha"], lp=torch.from_numpy(np.asarray(g["lp"], F32)).to(dev),
                          d=d[i], score=sc[i], sel=sel[i:i + 1]))
    ops.contrast_rows(specs, cand_dev)
    torch.cuda.synchronize()
    dh, sh, selh = d.cpu().numpy(), sc.cpu().numpy(), sel.cpu().numpy()
    return [(dh[i], sh[i], int(selh[i]), _bits(banks[i])) for i in range(len(groups))], _bits(cand_dev.contiguous()), first


def check_own(res, cand_bits, first, groups, dt):
    """What holds for every launch: d finite, values behind k untouched, sel inside [0, k) and the arg-max of the kernel's OWN scores with
    ties to the lower c, the scores bit for bit the header's expression of the kernel's own d (up to __expf: checked against the bound
    elsewhere), bank[T] the chosen candidate's bits, the rows behind it untouched."""
    for (d, s, sel, bank), g, f0 in zip(res, groups, first):
        T, k = g["bank"].shape[0], g["cand"].shape[0]
        assert np.isfinite(d[:k]).all() and np.isfinite(s[:k]).all()
        assert (d[k:] == F32(GUARD)).all() and (s[k:] == F32(GUARD)).all()
        assert 0 <= sel < k and sel == R.select(list(s[:k]))
        assert np.array_equal(bank[T], cand_bits[f0 + sel]), "bank[T] is not the chosen candidate bit for bit"
        assert (bank[T + 1:] == NAN_BITS[dt]).all(), "a bank row behind T was written"


# ---- exact probes -----------------------------------------------------------------------------------------------------------------------------
PROBE_H = 64


def _probe_bank(T, plant, negative=False):
    """one-hot rows: -e_0 on odd rows and e_(2 + i % 62) on even rows (dot products -1 / -0.5 and 0 with the candidates below), +e_0 at
    `plant`; negative: every row is -e_0"""
    bank = np.zeros((T, PROBE_H), F32)
    for i in range(T):
        if negative or i % 2:
            bank[i, 0] = -1.0
        else:
            bank[i, 2 + i % 62] = 1.0
    if plant is not None:
        bank[plant] = 0.0
        bank[plant, 0] = 1.0
    return bank


def _probe_cand(k):
    """candidate c: e_0 (even c) or 0.5 e_0 + 0.5 e_1 (odd c)"""
    cand = np.zeros((k, PROBE_H), F32)
    for c in range(k):
        if c % 2:
            cand[c, 0] = cand[c, 1] = 0.5
        else:
            cand[c, 0] = 1.0
    return cand


def _probe_lp(k):
    return np.log(np.linspace(0.3, 0.01, k)).astype(F32)


@DT
@pytest.mark.parametrize("T", (1, CHUNK - 1, CHUNK, CHUNK + 1, 63, 64, 65, 130))
def test_probe_maximum_at_every_position(dev, dt, T):
    """The maximum planted at EVERY bank position j in turn (T groups in one call: more than one 32-group launch pair for T > 32): d is
    1.0 / 0.5 bit for bit, whatever chunk and lane the row falls into; rows >= T hold NaN patterns and d stays finite."""
    k = 3
    groups = [dict(bank=_probe_bank(T, j), cand=_probe_cand(k), lp=_probe_lp(k), alpha=0.6) for j in range(T)]
    res, cb, first = launch(dev, dt, groups, PROBE_H)
    check_own(res, cb, first, groups, dt)
    for j, (d, s, sel, _) in enumerate(res):
        assert d[:k].tobytes() == np.array([1.0, 0.5, 1.0], F32).tobytes(), (T, j, d[:k])


@DT
@pytest.mark.parametrize("k", (1, 2, 3, 15, 16))
def test_probe_candidate_counts_and_negative_maximum(dev, dt, k):
    """k = 1 ... 16: unused operand columns change nothing; an all-negative bank: the maximum is the negative value, not 0; a bank
    without a planted row: 0 against e_0, 0 against the two-hot candidate as well (the even rows miss both)."""
    T = 37
    want_pos = np.array([1.0 if c % 2 == 0 else 0.5 for c in range(k)], F32)
    groups = [dict(bank=_probe_bank(T, 20), cand=_probe_cand(k), lp=_probe_lp(k), alpha=0.6),
              dict(bank=_probe_bank(T, None, negative=True), cand=_probe_cand(k), lp=_probe_lp(k), alpha=0.6),
              dict(bank=_probe_bank(T, None), cand=_probe_cand(k), lp=_probe_lp(k), alpha=0.6),
              dict(bank=_probe_bank(1, None, negative=True), cand=_probe_cand(k), lp=_probe_lp(k), alpha=0.6)]
    res, cb, first = launch(dev, dt, groups, PROBE_H, cand_pad=8)
    check_own(res, cb, first, groups, dt)
    assert res[0][0][:k].tobytes() == want_pos.tobytes()
    assert res[1][0][:k].tobytes() == (-want_pos).tobytes()
    assert res[2][0][:k].tobytes() == np.zeros(k, F32).tobytes()
    assert res[3][0][:k].tobytes() == (-want_pos).tobytes()
    for (d, s, sel, _), g in zip(res, groups):           # the scores follow from the kernel's own d inside the bound (exact d: no d term)
        ref = R.score(0.6, g["lp"], d[:k])
        assert (np.abs(s[:k] - ref) <= R.score_bound(0.6, g["lp"], d[:k], 0.0)).all()


# ---- random cases -----------------------------------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("i", range(len(CC.LAUNCHES)))
def test_random_cases(dev, dt, i):
    """d within max_j sum_bound, score within its bound, sel the arg-max of the kernel's own scores AND the fp64 restatement's on every
    group (none skipped: the host test proves every gap)."""
    groups = CC.launch_case(i, dt)
    H = CC.LAUNCHES[i]["H"]
    res, cb, first = launch(dev, dt, groups, H)
    check_own(res, cb, first, groups, dt)
    for (d, s, sel, _), g in zip(res, groups):
        k = g["k"]
        d64, db = R.d_of(g["bank"], g["cand"])
        err = np.abs(d[:k] - d64)
        assert (err <= db).all(), (g["T"], k, float((err / db).max()))
        _report(f"contrast_rows d {G.FMT[dt]} H={H} T={g['T']} k={k}", err, db)
        s64 = R.score(g["alpha"], g["lp"], d64)
        sb = R.score_bound(g["alpha"], g["lp"], d64, db)
        serr = np.abs(s[:k] - s64)
        assert (serr <= sb).all(), (g["T"], k, float((serr / sb).max()))
        _report(f"contrast_rows score {G.FMT[dt]} H={H} T={g['T']} k={k}", serr, sb)
        assert sel == R.select(s64), (g["T"], k, sel, s64)


# ---- ties, alpha = 0 ---------------------------------------------------------------------------------------------------------------------------
@DT
def test_ties_and_alpha_zero(dev, dt):
    base = CC.launch_case(0, dt)[3]                      # T = 257, k = 16
    dup = dict(base, cand=np.repeat(base["cand"][5:6], 4, 0), lp=np.full(4, base["lp"][2], F32), k=4)      # four identical candidates
    best = R.select(R.score(base["alpha"], base["lp"], R.d_of(base["bank"], base["cand"])[0]))
    pair = np.concatenate([base["cand"][:3], base["cand"][best:best + 1], base["cand"][best:best + 1]])
    two = dict(base, cand=pair, lp=np.array([-9.0, -9.5, -10.0, -1.0, -1.0], F32), k=5)                    # the winner twice: ranks 3 and 4
    zero = dict(base, alpha=0.0)
    zero_tie = dict(base, alpha=0.0, lp=np.concatenate([base["lp"][:1], base["lp"][:1], base["lp"][2:]]))
    groups = [dup, two, zero, zero_tie]
    res, cb, first = launch(dev, dt, groups, CC.LAUNCHES[0]["H"])
    check_own(res, cb, first, groups, dt)
    assert res[0][2] == 0 and len(set(res[0][1][:4].tolist())) == 1                         # equal scores: the lower c
    assert res[1][2] == 3 and res[1][1][3] == res[1][1][4]
    assert res[2][2] == 0 and res[3][2] == 0                                                # alpha = 0: the most probable candidate, rank 0
    assert (np.abs(res[2][1][:16] - np.exp(base["lp"].astype(np.float64))) <= R.score_bound(0.0, base["lp"], 0.0, 0.0)).all()   # p itself


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
@DT
def test_refusals(dev, dt):
    from vitron_amd import _lib, ops
    H = 64
    cand = torch.zeros((20, H), dtype=dt, device=dev)
    bank = torch.zeros((8, H), dtype=dt, device=dev)
    f = lambda n, t=torch.float32: torch.zeros((n,), dtype=t, device=dev)                  # noqa: E731
    good = dict(bank=bank, bank_len=3, k=4, first=0, alpha=0.5, lp=f(16), d=f(16), score=f(16), sel=f(1, torch.int32))
    ops.contrast_rows([good], cand)
    bad = [dict(k=17), dict(k=0), dict(bank_len=0), dict(bank_len=-1), dict(bank_len=8), dict(bank_len=9), dict(first=17), dict(first=-1),
           dict(alpha=1.5), dict(alpha=-0.1), dict(alpha=float("nan")), dict(lp=f(2)), dict(sel=f(1)), dict(bank=bank[:, :32].contiguous()),
           dict(bank=torch.zeros((8, H), dtype=torch.float32, device=dev))]
    for kw in bad:
        with pytest.raises(_lib.VitronHipError):
            ops.contrast_rows([dict(good, **kw)], cand)
    with pytest.raises(_lib.VitronHipError):
        ops.contrast_rows([], cand)
    with pytest.raises(_lib.VitronHipError, match="multiple of 32"):
        ops.contrast_rows([dict(good, bank=torch.zeros((8, 48), dtype=dt, device=dev))], torch.zeros((20, 48), dtype=dt, device=dev))
    with pytest.raises(_lib.VitronHipError, match="workspace"):
        ops.contrast_rows([dict(good, bank=torch.zeros((40, H), dtype=dt, device=dev), bank_len=33)], cand, workspace=f(16))
    with pytest.raises(_lib.VitronHipError):
        ops.unit_rows(torch.zeros((2, 8), device=dev), torch.zeros((9,), device=dev), dtype=dt)
    with pytest.raises(_lib.VitronHipError):
        ops.unit_rows(torch.zeros((2, 8), device=dev), None)
    torch.cuda.synchronize()
    assert int(good["sel"].item()) == 0                  # nothing ran after the first, valid launch
