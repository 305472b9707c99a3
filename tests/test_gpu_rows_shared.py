"""What csrc/vt_rows.h states once for the row kernels, checked ACROSS kernels on the same row, register form only
(V <= 32768, rows 16-byte aligned): the lse that vt_logprob_rows writes, lse_out[0] of vt_cfg_rows with the row as `cond` and lse_out[0]
of vt_dola_rows with it as `final` are the same fp32 bits -- same load, same slot order, same reductions -- and the plausibility mask of
vt_cfg_rows at log_beta = log(0.1) is vt_dola_rows' at log_relative_top = log(0.1) for the same `base`, NULL or given.
The streamed forms are not compared across kernels: their element orders differ by design (vt_rows.h). Each kernel's own values are
pinned in its own test file; this one only compares bits with bits."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROWS = 2
LOG_01 = math.log(0.1)


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(V):
    """(rows, other) fp32 [ROWS, V]: 4 N(0, 1); row 0 carries a tie at its maximum, row 1 one -inf"""
    rng = np.random.default_rng(V)
    x = (4.0 * rng.standard_normal((ROWS, V))).astype(np.float32)
    other = (4.0 * rng.standard_normal((ROWS, V))).astype(np.float32)
    top = np.float32(x[0].max() + 1.0)
    x[0, [V // 3, V - 1]] = top
    x[1, V // 2] = -np.inf
    return x, other


def _padded(a, dev):
    """The rows of `a` on the device, every row 16-byte aligned: the row stride is a multiple of 4 floats"""
    ld = (a.shape[1] + 3) // 4 * 4
    t = torch.zeros((a.shape[0], ld), dtype=torch.float32)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    t = t.to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def _row_ptr(t, r):
    return t.data_ptr() + 4 * r * t.stride(0)


@pytest.mark.parametrize("V", (33, 1025, 32768))
def test_lse_and_mask_agree_across_kernels(dev, V):
    from vitron_amd import ops
    from vitron_amd.sampling import pack_cfg_rows, pack_dola_rows
    W = (V + 31) // 32
    x, other = _inputs(V)
    xd, od = _padded(x, dev), _padded(other, dev)
    lse_lp = ops.logprob_rows(xd[:, :V], return_lse=True)["lse"]
    rng = np.random.default_rng(V + 1)
    given = torch.from_numpy(rng.integers(0, 2 ** 32, size=(ROWS, W), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
    for base in (None, given):
        out = torch.empty((2, ROWS, xd.shape[1]), dtype=torch.float32, device=dev)
        mask = torch.full((2, ROWS, W), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        lse = torch.full((2, ROWS, 2), -12345.5, dtype=torch.float32, device=dev)
        layer = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)
        b = [0 if base is None else _row_ptr(base, r) for r in range(ROWS)]
        ops.cfg_rows(pack_cfg_rows([(_row_ptr(xd, r), _row_ptr(od, r), _row_ptr(out[0], r), b[r], _row_ptr(mask[0], r), _row_ptr(lse[0], r),
                                     1.5, LOG_01) for r in range(ROWS)], dev), ROWS, V)
        ops.dola_rows(pack_dola_rows([(_row_ptr(xd, r), _row_ptr(od, r), xd.shape[1], 1, _row_ptr(out[1], r), b[r], _row_ptr(mask[1], r),
                                       layer[r:].data_ptr(), 0, _row_ptr(lse[1], r), LOG_01) for r in range(ROWS)], dev), ROWS, V)
        torch.cuda.synchronize()
        assert layer.tolist() == [0] * ROWS
        bits = [lse_lp.view(torch.int32).cpu().numpy(), lse[0, :, 0].contiguous().view(torch.int32).cpu().numpy(),
                lse[1, :, 0].contiguous().view(torch.int32).cpu().numpy()]
        print(f"V={V} base={'NULL' if base is None else 'given'} lse bits logprob / cfg / dola: {[list(map(hex, v)) for v in bits]}")
        assert np.isfinite(lse_lp.cpu().numpy()).all()
        assert np.array_equal(bits[0], bits[1]) and np.array_equal(bits[0], bits[2])
        m = mask.cpu().numpy().view(np.uint32)
        assert np.array_equal(m[0], m[1])
        # (the masks are not trivially equal: some token of every row is cut, and the tie at the maximum is kept)
        keep = (m[0][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
        keep = keep.reshape(ROWS, -1)[:, :V]
        if base is None:
            assert 0 < keep[0].sum() < V and keep[0, V // 3] == 1 and keep[0, V - 1] == 1 and keep[1, V // 2] == 0
