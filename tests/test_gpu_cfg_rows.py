"""vt_cfg_rows through ops.cfg_rows against tests/cfg_ref.py: both forms (rows in registers; re-read), one and many
blocks, ragged tails, in place, skipped rows, the plausibility mask with and without a base, non-finite values, the refusals.
The pin is (b): `out` equals, bit for bit, the fp32 restatement of the blend fed with the kernel's OWN two lse values; the lse values
themselves are held to tests/logprob_ref.lse_bound with this kernel's chain length. The distance of `out` to the fp64 row is printed,
not thresholded."""
import numpy as np
import pytest
import torch

from tests import cfg_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = (1, 33, 1025, 4097, 32000, 32768, 32769, 50000)
GUARD_F = -12345.5
GUARD_W = 0x5a5a5a5a
BETA = 0.1


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_inputs = {}


def inputs(V, rows):
    """(cond, uncond) fp32 [rows, V] on the host, computed once per shape and never modified: both signs, ties for the maximum, a
    dominant entry, the row's extremes on the mask's word boundaries, and in every row one value EXACTLY at the plausibility threshold"""
    if (V, rows) not in _inputs:
        g = torch.Generator().manual_seed(7000 + 31 * V + rows)
        c = (torch.randn((rows, V), generator=g) * 3.0).numpy()
        u = (torch.randn((rows, V), generator=g) * 3.0).numpy()
        for r in range(rows):
            if V > 40:
                c[r, 31], c[r, 32], c[r, V - 1] = 9.0, 9.5, 9.5                            # a tie for the maximum across a word boundary
                u[r, 0] = 20.0 if r % 3 == 0 else u[r, 0]                                  # a dominant unconditional entry
                c[r, 5 + r] = F32(R.row_max(c[r]) + R.log_beta(BETA))                      # the tie at the threshold: it stays
                c[r, 7 + r] = np.nextafter(c[r, 5 + r], F32(-np.inf))                      # one ulp below: it leaves
        _inputs[(V, rows)] = (c, u)
    return _inputs[(V, rows)]


class Bufs:
    """Device buffers for one launch: every row of cond / uncond / out starts `off` bytes past a 16-byte boundary, with guard values
    behind each row; masks and bases are [rows, W + 1] words (one guard word)."""

    def __init__(self, dev, c, u, off, base=None):
        rows, V = c.shape
        self.rows, self.V, self.W = rows, V, (V + 31) // 32
        self.ld = ((V + 3) // 4) * 4 + 8                                                   # a multiple of 4 floats: every row has the same alignment
        e = off // 4

        def place(x):
            t = torch.full((rows * self.ld + 8,), GUARD_F, dtype=torch.float32)
            v = t[e:e + rows * self.ld].view(rows, self.ld)
            if x is not None:
                v[:, :V] = torch.from_numpy(x)
            return t.to(dev), e
        self.c, _ = place(c)
        self.u, _ = place(u)
        self.o, _ = place(None)
        self.e = e
        self.mask = torch.full((rows, self.W + 1), GUARD_W, dtype=torch.int32, device=dev)
        self.lse = torch.full((rows, 2), GUARD_F, dtype=torch.float32, device=dev)
        self.base = None if base is None else torch.from_numpy(np.concatenate([base, np.zeros((rows, 1), np.uint32)], 1).view(np.int32)).to(dev)

    def ptr(self, t, r):
        return t.data_ptr() + 4 * (self.e + r * self.ld)

    def view(self, t):
        return t.cpu().numpy()[self.e:self.e + self.rows * self.ld].reshape(self.rows, self.ld)

    def launch(self, scale, beta, inplace=False, skip=(), want_mask=True, want_lse=True, based=()):
        from vitron_amd import ops
        from vitron_amd.sampling import log_beta, pack_cfg_rows
        dst = self.c if inplace else self.o
        rows = []
        for r in range(self.rows):
            s = scale[r] if isinstance(scale, (list, tuple)) else scale
            rows.append((0 if r in skip else self.ptr(self.c, r), self.ptr(self.u, r), self.ptr(dst, r),
                         self.base[r].data_ptr() if r in based else 0, self.mask[r].data_ptr() if want_mask else 0,
                         self.lse[r].data_ptr() if want_lse else 0, s, log_beta(beta)))
        packed = pack_cfg_rows(rows, self.c.device)
        ops.cfg_rows(packed, self.rows, self.V)
        torch.cuda.synchronize()
        return self.view(dst), self.mask.cpu().numpy().view(np.uint32), self.lse.cpu().numpy()


def _bases(rows, V, seed):
    """Random bases whose tail bits (positions >= V of the last word) are set: they must come through as they are"""
    rng = np.random.default_rng(seed)
    W = (V + 31) // 32
    b = rng.integers(0, 2 ** 32, size=(rows, W), dtype=np.uint64).astype(np.uint32)
    b |= rng.integers(0, 2 ** 32, size=(rows, W), dtype=np.uint64).astype(np.uint32)       # three bits in four set
    if V & 31:
        b[:, -1] |= np.uint32((0xffffffff << (V & 31)) & 0xffffffff)
    return b


@pytest.mark.parametrize("off", (0, 4))
@pytest.mark.parametrize("rows", (1, 2, 17))
@pytest.mark.parametrize("V", VS)
def test_rows_against_the_reference(dev, V, rows, off):
    """(a) lse within the bound of fp64, (b) out bit for bit from the kernel's own lse, (c) in place == out of place, (e) the mask exact,
    odd rows with a base and even rows without; nothing is written behind a row or behind a mask."""
    c, u = inputs(V, rows)
    scale = 1.5
    reg = R.register_form(V, (off, off, off))
    base = _bases(rows, V, 11 + V)
    based = tuple(r for r in range(rows) if r % 2 == 1)
    b = Bufs(dev, c, u, off, base)
    out, mask, lse = b.launch(scale, BETA, based=based)
    chain = R.lse_chain(V, reg)
    far = 0.0
    for r in range(rows):
        for k, x in enumerate((c, u)):                                                     # (a)
            err = abs(float(lse[r, k]) - float(R.lse64(x[r])[0]))
            bound = float(R.lse_bound(x[r], chain)[0])
            assert err <= bound, (V, rows, off, r, k, err, bound)
        want = R.guided32(c[r], u[r], scale, lse[r, 0], lse[r, 1])                         # (b)
        assert R.same_bits(out[r, :V], want), (V, rows, off, r, np.flatnonzero(out[r, :V] != want)[:5])
        far = max(far, float(np.abs(out[r, :V].astype(np.float64) - R.guided64(c[r], u[r], scale)).max()))
        assert (out[r, V:] == F32(GUARD_F)).all()
        want_m = R.mask(c[r], BETA, base[r] if r in based else None)                       # (e)
        assert (mask[r, :b.W] == want_m).all(), (V, rows, off, r, np.flatnonzero(mask[r, :b.W] != want_m)[:5])
        assert mask[r, b.W] == GUARD_W
    print(f"cfg_rows V={V} rows={rows} off={off} form={'reg' if reg else 'reread'}: max |out - fp64| = {far:.3e}")
    b2 = Bufs(dev, c, u, off, base)                                                        # (c)
    out2, mask2, lse2 = b2.launch(scale, BETA, inplace=True, based=based)
    assert R.same_bits(out2[:, :V], out[:, :V]) and (mask2 == mask).all() and R.same_bits(lse2, lse)
    assert (out2[:, V:] == F32(GUARD_F)).all()
    assert (b2.view(b2.u)[:, :V] == u).all()                                               # the unconditional rows are only read


def test_threshold_tie_stays_and_one_ulp_below_leaves(dev):
    """The inputs carry, per row, one value exactly at m_c + log(beta) and one an ulp below it (inputs()): the first bit is set, the
    second clear, in both forms."""
    for V, off in ((1025, 0), (1025, 4), (50000, 0)):
        c, u = inputs(V, 2)
        _, mask, _ = Bufs(dev, c, u, off).launch(1.5, BETA)
        for r in range(2):
            assert (mask[r, 0] >> (5 + r)) & 1 == 1 and (mask[r, 0] >> (7 + r)) & 1 == 0
            top = int(np.argmax(c[r]))
            assert (mask[r, top >> 5] >> (top & 31)) & 1 == 1


@pytest.mark.parametrize("off", (0, 4))
@pytest.mark.parametrize("V", (33, 4097, 32769))
def test_skipped_rows_are_untouched(dev, V, off):
    """(d) rows with cond = NULL: out, mask_out and lse_out keep their sentinel fill; their neighbours are computed."""
    rows = 17
    c, u = inputs(V, rows)
    skip = tuple(range(1, rows, 2))
    b = Bufs(dev, c, u, off)
    out, mask, lse = b.launch(2.0, BETA, skip=skip)
    for r in range(rows):
        if r in skip:
            assert (out[r] == F32(GUARD_F)).all() and (mask[r] == GUARD_W).all() and (lse[r] == F32(GUARD_F)).all()
        else:
            assert R.same_bits(out[r, :V], R.guided32(c[r], u[r], 2.0, lse[r, 0], lse[r, 1])) and (mask[r, :b.W] == R.mask(c[r], BETA)).all()
    # no mask and no lse asked for: only out is written
    b = Bufs(dev, c, u, off)
    out2, mask2, lse2 = b.launch(2.0, BETA, want_mask=False, want_lse=False)
    assert (mask2 == GUARD_W).all() and (lse2 == F32(GUARD_F)).all()
    assert all(R.same_bits(out2[r, :V], out[r, :V]) for r in range(rows) if r not in skip)


@pytest.mark.parametrize("off", (0, 4))
@pytest.mark.parametrize("V", (1025, 32768, 32769))
def test_scales_and_non_finite_values(dev, V, off):
    """(f) scales 1.5, 0, -0.5 and 7 in one launch, then rows that hold -inf and NaN: the blend follows IEEE rules (NaN compared with NaN,
    -inf with -inf), the mask drops a NaN, beta = 0 keeps everything that is not a NaN, beta = 1 keeps the maxima."""
    c, u = inputs(V, 17)
    c, u = c[:8].copy(), u[:8].copy()
    scales = [1.5, 0.0, -0.5, 7.0, 1.5, 2.0, 2.0, 2.0]
    c[4, 3] = c[4, V - 1] = -np.inf                        # -inf in cond only: out = ul + s * (-inf - ul)
    u[5, 4] = -np.inf                                      # -inf in uncond only
    c[5, 9] = u[5, 9] = -np.inf                            # in both: -inf - -inf is a NaN, at that element alone
    c[6, 2] = np.nan                                       # a NaN in cond: lse_c is NaN, the whole guided row is
    u[7, V // 2] = np.nan                                  # a NaN in uncond
    b = Bufs(dev, c, u, off)
    out, mask, lse = b.launch(scales, BETA)
    for r in range(8):
        want = R.guided32(c[r], u[r], scales[r], lse[r, 0], lse[r, 1])
        assert R.same_bits(out[r, :V], want), (V, off, r)
        assert (mask[r, :b.W] == R.mask(c[r], BETA)).all(), (V, off, r)
    assert np.isfinite(lse[:6]).all() and np.isnan(lse[6, 0]) and np.isfinite(lse[6, 1]) and np.isnan(lse[7, 1]) and np.isfinite(lse[7, 0])
    assert np.isnan(out[6, :V]).all() and np.isnan(out[7, :V]).all()
    assert np.isnan(out[5, 9]) and np.isfinite(np.delete(out[5, :V], [4, 9])).all() and out[4, 3] == -np.inf
    assert (mask[6, 0] >> 2) & 1 == 0                      # the NaN's bit
    for beta in (0.0, 1.0):
        _, m, _ = Bufs(dev, c, u, off).launch(scales, beta)
        for r in range(8):
            assert (m[r, :b.W] == R.mask(c[r], beta)).all(), (V, off, r, beta)
        bits = np.unpackbits(m[6, :b.W].view(np.uint8), bitorder="little")[:V]
        assert bits.sum() == (V - 1 if beta == 0.0 else int((c[6] == R.row_max(c[6])).sum()))


def test_refusals(dev):
    """(g) VT_STATUS_ARG with a message before any launch: rows NULL, n_rows <= 0, V <= 0, V beyond vt_logprob_rows' bound, a misaligned
    row array; ops.cfg_rows adds the size and device checks of the packed array."""
    from vitron_amd import _lib, ops
    from vitron_amd.sampling import CFG_ROW_BYTES, pack_cfg_rows
    lib = _lib.load()
    V = 64
    c = torch.zeros((V,), dtype=torch.float32, device=dev)
    u = torch.zeros((V,), dtype=torch.float32, device=dev)
    o = torch.full((V,), GUARD_F, dtype=torch.float32, device=dev)
    packed = pack_cfg_rows([(c.data_ptr(), u.data_ptr(), o.data_ptr(), 0, 0, 0, 2.0, -np.inf)], dev)
    shifted = torch.zeros((CFG_ROW_BYTES + 8,), dtype=torch.uint8, device=dev)
    shifted[4:4 + CFG_ROW_BYTES] = packed.view(-1)
    stream = torch.cuda.current_stream().cuda_stream
    for n_rows, v, ptr, needle in ((1, V, None, "NULL"), (0, V, packed.data_ptr(), "n_rows=0"), (-1, V, packed.data_ptr(), "n_rows=-1"),
                                   (1, 0, packed.data_ptr(), "V=0"), (1, -5, packed.data_ptr(), "V=-5"),
                                   (1, (1 << 30) + 1, packed.data_ptr(), f"V={(1 << 30) + 1}"), (1, V, shifted.data_ptr() + 4, "8-byte aligned")):
        assert lib.vt_cfg_rows(ptr, n_rows, v, stream) == -1                               # VT_STATUS_ARG, with a message
        assert needle in _lib.last_error(lib), (needle, _lib.last_error(lib))
    with pytest.raises(_lib.VitronHipError, match="NULL"):
        ops.cfg_rows(None, 1, V)
    with pytest.raises(_lib.VitronHipError, match="n_rows=0"):
        ops.cfg_rows(packed, 0, V)
    with pytest.raises(_lib.VitronHipError, match="V=0"):
        ops.cfg_rows(packed, 1, 0)
    with pytest.raises(_lib.VitronHipError, match="8-byte aligned"):
        ops.cfg_rows(shifted[4:4 + CFG_ROW_BYTES], 1, V)
    with pytest.raises(_lib.VitronHipError):
        ops.cfg_rows(packed, 2, V)                                                         # 56 bytes are one row, not two
    with pytest.raises(_lib.VitronHipError):
        ops.cfg_rows(packed.cpu(), 1, V)
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == F32(GUARD_F)).all()                                         # nothing was launched
    ops.cfg_rows(packed, 1, V)
    torch.cuda.synchronize()
    assert np.allclose(o.cpu().numpy(), -np.log(V), atol=1e-6)                             # two uniform rows: the guided row is uniform
