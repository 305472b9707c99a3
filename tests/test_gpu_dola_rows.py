"""vt_dola_rows through ops.dola_rows against tests/dola_ref.py: both forms (final row in registers; re-read), one and
many blocks, 1 / 2 / 8 / 16 candidates, ragged tails, in place, skipped rows, the mask with and without a base, the choice probes,
non-finite values, bad row content, the refusals.
The pins: lse inside tests/logprob_ref.lse_bound and div inside dola_ref.div_bound of fp64 (this kernel's chain length); the chosen
candidate exact on ladder cases (whose builder asserts a gap of 4 bounds); `out` bit for bit the fp32 restatement fed with the kernel's
OWN lse values and choice; the mask exact. The distance of `out` to the fp64 row is printed, not thresholded."""
import numpy as np
import pytest
import torch

from tests import dola_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD_F = -12345.5
GUARD_W = 0x5a5a5a5a
GUARD_I = -777
RT = 0.1
# (V, rows, n_cand): every V of the two forms' boundary, one and many blocks, every candidate count; the large products stay small
CASES = ((1, 2, 1), (33, 1, 2), (33, 17, 8), (1025, 2, 8), (1025, 17, 16), (4097, 1, 1), (4097, 2, 8), (32000, 1, 8), (32000, 2, 16),
         (32768, 1, 8), (32768, 2, 2), (32769, 1, 1), (32769, 2, 8), (32769, 17, 2), (50000, 1, 8), (50000, 2, 2))


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_cases = {}


def case(V, rows, n_cand, reg):
    """(final [rows, V], prem [rows, n_cand, V], j [rows]) on the host, one ladder case per row, computed once and never modified"""
    key = (V, rows, n_cand, reg)
    if key not in _cases:
        got = [R.ladder_case(V, n_cand, 100 + r, reg=reg) if V > 1 else
               (np.array([0.5 + r], dtype=F32), np.full((n_cand, 1), -1.25, dtype=F32), 0) for r in range(rows)]
        _cases[key] = (np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), [g[2] for g in got])
    return _cases[key]


class Bufs:
    """Device buffers for one launch: every row of final / out and every candidate row starts `off` bytes past a 16-byte boundary, guard
    values behind each; candidate j of row r stands `stride` floats behind candidate j - 1; masks are [rows, W + 1] words."""

    def __init__(self, dev, final, prem, off, base=None, odd_stride=False):
        rows, n_cand, V = prem.shape
        self.rows, self.n, self.V, self.W = rows, n_cand, V, (V + 31) // 32
        self.ld = ((V + 3) // 4) * 4 + 8 + (1 if odd_stride else 0)
        self.e = e = off // 4

        def place(x, lead):
            t = torch.full((lead * self.ld + 8,), GUARD_F, dtype=torch.float32)
            if x is not None:
                t[e:e + lead * self.ld].view(lead, self.ld)[:, :V] = torch.from_numpy(np.ascontiguousarray(x).reshape(lead, V))
            return t.to(dev)
        self.f = place(final, rows)
        self.p = place(prem, rows * n_cand)
        self.o = place(None, rows)
        self.mask = torch.full((rows, self.W + 1), GUARD_W, dtype=torch.int32, device=dev)
        self.lse = torch.full((rows, n_cand + 2), GUARD_F, dtype=torch.float32, device=dev)
        self.div = torch.full((rows, n_cand + 1), GUARD_F, dtype=torch.float32, device=dev)
        self.layer = torch.full((rows, 2), GUARD_I, dtype=torch.int32, device=dev)
        self.base = None if base is None else torch.from_numpy(np.concatenate([base, np.zeros((rows, 1), np.uint32)], 1).view(np.int32)).to(dev)

    def ptr(self, t, r):
        return t.data_ptr() + 4 * (self.e + r * self.ld)

    def view(self, t, lead):
        return t.cpu().numpy()[self.e:self.e + lead * self.ld].reshape(lead, self.ld)

    def launch(self, rt=RT, inplace=False, skip=(), want=True, based=(), n_cand=None):
        from vitron_amd import ops
        from vitron_amd.sampling import pack_dola_rows
        dst = self.f if inplace else self.o
        rows = []
        for r in range(self.rows):
            n = self.n if n_cand is None else n_cand[r]
            rows.append((0 if r in skip else self.ptr(self.f, r), self.ptr(self.p, r * self.n), self.ld, n, self.ptr(dst, r),
                         self.base[r].data_ptr() if r in based else 0, self.mask[r].data_ptr() if want else 0,
                         self.layer[r].data_ptr(), self.div[r].data_ptr() if want else 0, self.lse[r].data_ptr() if want else 0,
                         float(np.log(rt))))
        ops.dola_rows(pack_dola_rows(rows, self.f.device), self.rows, self.V)
        torch.cuda.synchronize()
        return {"out": self.view(dst, self.rows), "mask": self.mask.cpu().numpy().view(np.uint32), "lse": self.lse.cpu().numpy(),
                "div": self.div.cpu().numpy(), "layer": self.layer.cpu().numpy()}


def _bases(rows, V, seed):
    """Random bases whose tail bits (positions >= V of the last word) are set: they must come through as they are"""
    rng = np.random.default_rng(seed)
    W = (V + 31) // 32
    b = rng.integers(0, 2 ** 32, size=(rows, W), dtype=np.uint64).astype(np.uint32)
    b |= rng.integers(0, 2 ** 32, size=(rows, W), dtype=np.uint64).astype(np.uint32)
    if V & 31:
        b[:, -1] |= np.uint32((0xffffffff << (V & 31)) & 0xffffffff)
    return b


def _check_row(got, r, final, prem, V, n, reg, rt=RT, base=None, check_div=True):
    """One served row against the reference; returns max |out - fp64| over the kept tokens."""
    chain = R.chain(V, reg)
    lse, div, j = got["lse"][r], got["div"][r], int(got["layer"][r, 0])
    assert 0 <= j < n and got["layer"][r, 1] == GUARD_I and lse[n + 1] == F32(GUARD_F) and div[n] == F32(GUARD_F)
    for k, x in enumerate([final] + list(prem)):
        err, bound = abs(float(lse[k]) - float(R.lse64(x)[0])), float(R.lse_bound(x, chain)[0])
        assert err <= bound, ("lse", V, r, k, err, bound)
    if n == 1:
        assert div[0] == 0.0
    elif check_div:
        d64 = R.divergences64(final, prem)
        for k in range(n):
            bound = R.div_bound(final, prem[k], reg)
            assert abs(float(div[k]) - d64[k]) <= bound, ("div", V, r, k, float(div[k]), d64[k], bound)
    want = R.out32(final, prem[j], lse[0], lse[1 + j], rt)
    assert R.same_bits(got["out"][r, :V], want), (V, r, np.flatnonzero(got["out"][r, :V] != want)[:5])
    assert (got["out"][r, V:] == F32(GUARD_F)).all()
    W = (V + 31) // 32
    want_m = R.mask(final, rt, base)
    assert (got["mask"][r, :W] == want_m).all(), (V, r, np.flatnonzero(got["mask"][r, :W] != want_m)[:5])
    assert got["mask"][r, W] == GUARD_W
    k = R.keep(final, rt)
    return float(np.abs(got["out"][r, :V][k].astype(np.float64) - (R.log_softmax64(final) - R.log_softmax64(prem[j]))[k]).max())


@pytest.mark.parametrize("off", (0, 4))
@pytest.mark.parametrize("V,rows,n_cand", CASES)
def test_rows_against_the_reference(dev, V, rows, n_cand, off):
    """lse and div inside their bounds, the choice exact, out bit for bit from the kernel's own lse and j, in place == out of place, the
    mask exact (odd rows with a base, even rows without); nothing is written behind a row, a mask or the small outputs."""
    reg = R.register_form(V, (off, off, off))
    final, prem, js = case(V, rows, n_cand, reg)
    base = _bases(rows, V, 11 + V)
    based = tuple(r for r in range(rows) if r % 2 == 1)
    b = Bufs(dev, final, prem, off, base)
    got = b.launch(based=based)
    far = 0.0
    for r in range(rows):
        far = max(far, _check_row(got, r, final[r], prem[r], V, n_cand, reg, base=base[r] if r in based else None))
        assert int(got["layer"][r, 0]) == js[r], (V, rows, n_cand, off, r, got["div"][r], js[r])
    print(f"dola_rows V={V} rows={rows} n_cand={n_cand} off={off} form={'reg' if reg else 'reread'}: max |out - fp64| = {far:.3e}")
    b2 = Bufs(dev, final, prem, off, base)
    got2 = b2.launch(inplace=True, based=based)
    assert R.same_bits(got2["out"][:, :V], got["out"][:, :V]) and (got2["out"][:, V:] == F32(GUARD_F)).all()
    for name in ("mask", "layer"):
        assert (got2[name] == got[name]).all()
    assert R.same_bits(got2["lse"], got["lse"]) and R.same_bits(got2["div"], got["div"])
    assert (b2.view(b2.p, rows * n_cand)[:, :V] == prem.reshape(-1, V)).all()              # the candidate rows are only read
    assert (b.view(b.f, rows)[:, :V] == final).all()                                       # out of place: so is the final row


@pytest.mark.parametrize("V", (1025, 32768))
def test_a_candidate_stride_that_is_no_multiple_of_four_takes_the_reread_form(dev, V):
    final, prem, js = case(V, 2, 8, False)
    got = Bufs(dev, final, prem, 0, odd_stride=True).launch()
    for r in range(2):
        _check_row(got, r, final[r], prem[r], V, 8, False)
        assert int(got["layer"][r, 0]) == js[r]


@pytest.mark.parametrize("V,off", ((1025, 0), (1025, 4), (32769, 0)))
def test_choice_probes(dev, V, off):
    """Rows 0..7: the furthest candidate stands at position r and is the one chosen. Row 8: two bitwise equal candidate rows, both the
    furthest, give bitwise equal div and the lower index. Row 9: a candidate equal to the final row has a divergence of rounding size
    and is never chosen over a different one."""
    reg = R.register_form(V, (off, off, off))
    got_cases = [R.ladder_case(V, 8, 5, reg=reg, furthest_at=p) for p in range(8)]
    final = np.stack([g[0] for g in got_cases] + [got_cases[6][0], got_cases[1][0]])
    prem = np.stack([g[1] for g in got_cases] + [got_cases[6][1].copy(), got_cases[1][1].copy()])
    prem[8, 2] = prem[8, 6]
    prem[9, 0] = final[9]
    got = Bufs(dev, final, prem, off).launch()
    for r in range(8):
        assert int(got["layer"][r, 0]) == r, (V, off, r, got["div"][r])
        _check_row(got, r, final[r], prem[r], V, 8, reg)
    assert int(got["layer"][8, 0]) == 2 and got["div"][8, 2].view(np.uint32) == got["div"][8, 6].view(np.uint32)
    assert got["lse"][8, 3].view(np.uint32) == got["lse"][8, 7].view(np.uint32)
    _check_row(got, 8, final[8], prem[8], V, 8, reg)
    assert int(got["layer"][9, 0]) == 1 and abs(float(got["div"][9, 0])) <= R.div_bound(final[9], final[9], reg)
    _check_row(got, 9, final[9], prem[9], V, 8, reg)


@pytest.mark.parametrize("V,off", ((1025, 0), (1025, 4), (50000, 0)))
def test_threshold_tie_stays_and_one_ulp_below_leaves(dev, V, off):
    """One value exactly at max + log(relative_top) and one an ulp below it: the first is kept (bit set, a finite contrast), the second
    leaves (bit clear, -inf); the arg-max of final is always kept. relative_top = 1 keeps only the maxima."""
    reg = R.register_form(V, (off, off, off))
    f0, p0, _ = case(V, 2, 8, reg)
    final, prem = f0.copy(), p0[:, :1].copy()
    for r in range(2):
        final[r, 5 + r] = F32(R.row_max(final[r]) + R.log_rt(RT))
        final[r, 37 + r] = np.nextafter(final[r, 5 + r], F32(-np.inf))
    got = Bufs(dev, final, prem, off).launch()
    for r in range(2):
        _check_row(got, r, final[r], prem[r], V, 1, reg)
        top = int(np.argmax(final[r]))
        assert (got["mask"][r, 0] >> (5 + r)) & 1 == 1 and np.isfinite(got["out"][r, 5 + r])
        assert (got["mask"][r, 1] >> (5 + r)) & 1 == 0 and np.isneginf(got["out"][r, 37 + r])
        assert (got["mask"][r, top >> 5] >> (top & 31)) & 1 == 1 and np.isfinite(got["out"][r, top])
    got = Bufs(dev, final, prem, off).launch(rt=1.0)
    for r in range(2):
        _check_row(got, r, final[r], prem[r], V, 1, reg, rt=1.0)
        assert np.isfinite(got["out"][r, :V]).sum() == int((final[r] == final[r].max()).sum())


@pytest.mark.parametrize("off", (0, 4))
@pytest.mark.parametrize("V", (33, 4097, 32769))
def test_skipped_rows_and_bad_row_content(dev, V, off):
    """Rows with final = NULL keep their sentinel fill everywhere. A live row whose n_cand is outside [1, 16] writes layer_out = -1 and
    nothing else. Their neighbours are served. Without the optional outputs only out and layer_out are written."""
    rows = 9
    reg = R.register_form(V, (off, off, off))
    final, prem, js = case(V, rows, 2, reg)
    skip, bad = (1, 4), {2: 0, 5: 17, 7: -3}
    b = Bufs(dev, final, prem, off)
    got = b.launch(skip=skip, n_cand=[bad.get(r, 2) for r in range(rows)])
    for r in range(rows):
        if r in skip or r in bad:
            assert (got["out"][r] == F32(GUARD_F)).all() and (got["mask"][r] == GUARD_W).all()
            assert (got["lse"][r] == F32(GUARD_F)).all() and (got["div"][r] == F32(GUARD_F)).all()
            assert got["layer"][r].tolist() == ([GUARD_I, GUARD_I] if r in skip else [-1, GUARD_I])
        else:
            _check_row(got, r, final[r], prem[r], V, 2, reg)
            assert int(got["layer"][r, 0]) == js[r]
    got2 = Bufs(dev, final, prem, off).launch(want=False)
    assert (got2["mask"] == GUARD_W).all() and (got2["lse"] == F32(GUARD_F)).all() and (got2["div"] == F32(GUARD_F)).all()
    assert got2["layer"][:, 0].tolist() == js
    live = [r for r in range(rows) if r not in skip and r not in bad]
    assert R.same_bits(got2["out"][live][:, :V], got["out"][live][:, :V])


@pytest.mark.parametrize("off", (0, 4))
@pytest.mark.parametrize("V", (1025, 32769))
def test_non_finite_values(dev, V, off):
    """Rows that hold -inf and NaN do what the reference says: a NaN in final -- NaN lse and divergences, candidate 0, NaN where kept and
    -inf elsewhere, the NaN's own bit clear; a NaN in one candidate -- that candidate is never chosen; -inf in final only -- +inf
    divergences, candidate 0; -inf in final and in every candidate -- the term counts 0 and the row is an ordinary one."""
    reg = R.register_form(V, (off, off, off))
    f0, p0, js = case(V, 4, 8, reg)
    final, prem = f0[:4].copy(), p0[:4].copy()
    final[0, 7] = np.nan
    prem[1, js[1], V // 2] = np.nan
    final[2, 3] = -np.inf
    final[3, 9] = -np.inf
    prem[3, :, 9] = -np.inf
    got = Bufs(dev, final, prem, off).launch()
    for r in range(4):
        j = int(got["layer"][r, 0])
        want = R.out32(final[r], prem[r, j], got["lse"][r, 0], got["lse"][r, 1 + j], RT)
        assert R.same_bits(got["out"][r, :V], want), (V, off, r)
        assert (got["mask"][r, :(V + 31) // 32] == R.mask(final[r], RT)).all(), (V, off, r)
        assert j == R.row64(final[r], prem[r])["j"], (V, off, r, got["div"][r, :8])
    assert np.isnan(got["lse"][0, 0]) and np.isnan(got["div"][0, :8]).all() and got["layer"][0, 0] == 0
    keep = R.keep(final[0], RT)
    assert not keep[7] and np.isnan(got["out"][0, :V][keep]).all() and np.isneginf(got["out"][0, :V][~keep]).all()
    assert np.isnan(got["div"][1, js[1]]) and np.isfinite(np.delete(got["div"][1, :8], js[1])).all() and got["layer"][1, 0] != js[1]
    assert np.isposinf(got["div"][2, :8]).all() and got["layer"][2, 0] == 0 and np.isneginf(got["out"][2, 3])
    d64 = R.divergences64(final[3], prem[3])
    for k in range(8):       # the element that counts 0 taken out: the bound of the remaining row
        bound = R.div_bound(np.delete(final[3], 9), np.delete(prem[3, k], 9), reg)
        assert abs(float(got["div"][3, k]) - d64[k]) <= bound, (V, off, k)
    assert np.isneginf(got["out"][3, 9])


def test_refusals(dev):
    """VT_STATUS_ARG with a message before any launch: rows NULL, n_rows <= 0, V <= 0, V beyond vt_logprob_rows' bound, a misaligned row
    array; ops.dola_rows adds the size and device checks of the packed array."""
    from vitron_amd import _lib, ops
    from vitron_amd.sampling import DOLA_ROW_BYTES, pack_dola_rows
    lib = _lib.load()
    V = 64
    f = torch.zeros((V,), dtype=torch.float32, device=dev)
    p = torch.zeros((2, V), dtype=torch.float32, device=dev)
    p[1, 0] = 3.0
    o = torch.full((V,), GUARD_F, dtype=torch.float32, device=dev)
    layer = torch.full((1,), GUARD_I, dtype=torch.int32, device=dev)
    packed = pack_dola_rows([(f.data_ptr(), p.data_ptr(), V, 2, o.data_ptr(), 0, 0, layer.data_ptr(), 0, 0, float(np.log(RT)))], dev)
    shifted = torch.zeros((DOLA_ROW_BYTES + 8,), dtype=torch.uint8, device=dev)
    shifted[4:4 + DOLA_ROW_BYTES] = packed.view(-1)
    stream = torch.cuda.current_stream().cuda_stream
    for n_rows, v, ptr, needle in ((1, V, None, "NULL"), (0, V, packed.data_ptr(), "n_rows=0"), (-1, V, packed.data_ptr(), "n_rows=-1"),
                                   (1, 0, packed.data_ptr(), "V=0"), (1, -5, packed.data_ptr(), "V=-5"),
                                   (1, (1 << 30) + 1, packed.data_ptr(), f"V={(1 << 30) + 1}"), (1, V, shifted.data_ptr() + 4, "8-byte aligned")):
        assert lib.vt_dola_rows(ptr, n_rows, v, stream) == -1                              # VT_STATUS_ARG, with a message
        assert needle in _lib.last_error(lib), (needle, _lib.last_error(lib))
    with pytest.raises(_lib.VitronHipError, match="NULL"):
        ops.dola_rows(None, 1, V)
    with pytest.raises(_lib.VitronHipError, match="n_rows=0"):
        ops.dola_rows(packed, 0, V)
    with pytest.raises(_lib.VitronHipError, match="V=0"):
        ops.dola_rows(packed, 1, 0)
    with pytest.raises(_lib.VitronHipError, match="8-byte aligned"):
        ops.dola_rows(shifted[4:4 + DOLA_ROW_BYTES], 1, V)
    with pytest.raises(_lib.VitronHipError):
        ops.dola_rows(packed, 2, V)                                                        # 80 bytes are one row, not two
    with pytest.raises(_lib.VitronHipError):
        ops.dola_rows(packed.cpu(), 1, V)
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == F32(GUARD_F)).all() and layer.item() == GUARD_I             # nothing was launched
    ops.dola_rows(packed, 1, V)
    torch.cuda.synchronize()
    assert layer.item() == 1                              # a uniform final row: candidate 0 equals it, candidate 1 does not
    assert np.allclose(o.cpu().numpy(), -np.log(V) - R.log_softmax64(p[1].cpu().numpy()), atol=1e-5)
