"""Host restatement of vt_cfg_rows (vitron_amd/csrc/vt_cfg.hip, include/vitron_hip.h) for tests/test_cfg_ref_host.py,
tests/test_gpu_cfg_rows.py and tests/test_gpu_cfg_requests.py: the fp64 guided row  s (log_softmax(c) - log_softmax(u)) + log_softmax(u),
its fp32 restatement from a GIVEN (lse_c, lse_u) in numpy float32 operations -- every one of them rounds to nearest on its own, exactly
as the kernel's __fsub_rn / __fmul_rn / __fadd_rn do, so the kernel's `out` must equal it bit for bit once it is fed the kernel's own
lse values -- the plausibility mask, and the bound on the two lse values.
The bound is tests/logprob_ref.lse_bound with vt_cfg_rows' own chain length: in the register form (V <= 32 * 1024, the three rows
16-byte aligned) a thread adds 32 terms, as vt_logprob_rows does; in the re-read form it adds its elements t + 1024 j one at a time,
ceil(V / 1024) terms, which is at most logprob_ref.lse_chain's 4 ceil(V / 4096) + 1 for the streaming form; then 6 shuffle levels and the
16 wave totals in both. `lse_chain` below states that. Plain numpy / torch on the CPU; nothing here calls the library."""
import numpy as np

from tests.logprob_ref import log_softmax64, lse64, lse_bound  # noqa: F401  (lse_bound, lse64: used by the GPU tests through this module)
from tests.sample_ref import F32


def register_form(V: int, offsets_bytes=(0, 0, 0)) -> bool:
    """The kernel's choice per row: V <= 32 * 1024 and cond, uncond and out all 16-byte aligned."""
    return V <= 32 * 1024 and all(o % 16 == 0 for o in offsets_bytes)


def lse_chain(V: int, reg: bool) -> int:
    """Longest chain of fp32 additions behind one of vt_cfg_rows' two sums, read off cfg_rows_kernel (see the module docstring)."""
    own = 32 if reg else -(-V // 1024)
    return own + 6 + 16


def guided64(cond, uncond, scale) -> np.ndarray:
    """fp64 guided row(s): ul + s (cl - ul) with cl, ul the fp64 log_softmax of the fp32 rows."""
    cl, ul = log_softmax64(cond), log_softmax64(uncond)
    with np.errstate(all="ignore"):
        return ul + np.float64(scale) * (cl - ul)


def guided32(cond, uncond, scale, lse_c, lse_u) -> np.ndarray:
    """fp32 guided row from the given lse values: cl = c - lse_c; ul = u - lse_u; out = ul + s * (cl - ul), every operation a numpy
    float32 operation (IEEE round to nearest, no fused multiply-add): the kernel's contract, bit for bit."""
    c, u = np.asarray(cond, dtype=F32), np.asarray(uncond, dtype=F32)
    s, lc, lu = F32(scale), F32(lse_c), F32(lse_u)
    with np.errstate(all="ignore"):
        cl = (c - lc).astype(F32)
        ul = (u - lu).astype(F32)
        d = (cl - ul).astype(F32)
        p = (s * d).astype(F32)
        return (ul + p).astype(F32)


def row_max(row) -> np.float32:
    """The kernel's m: the maximum over the values that are not NaN (fmaxf skips a NaN), -inf when there is none."""
    x = np.asarray(row, dtype=F32)
    x = x[~np.isnan(x)]
    return F32(x.max()) if x.size else F32(-np.inf)


def log_beta(beta: float) -> np.float32:
    return F32(np.log(beta)) if beta > 0 else F32(-np.inf)


def mask(cond, beta: float, base=None) -> np.ndarray:
    """uint32 [ceil(V / 32)]: bit i = base bit i AND (c_i >= m_c + log(beta)) in fp32; a NaN c_i fails. Bits at positions >= V of the
    last word are base's own there, or clear without a base (vt_ban_rows' convention)."""
    c = np.asarray(cond, dtype=F32)
    V = c.size
    W = (V + 31) // 32
    with np.errstate(all="ignore"):
        thr = F32(row_max(c) + log_beta(beta))
        ok = np.ones((W * 32,), dtype=bool)
        ok[:V] = c >= thr
    words = np.packbits(ok, bitorder="little").view("<u4").astype(np.uint32)
    if base is None:
        start = np.zeros((W * 32,), dtype=bool)
        start[:V] = True
        base = np.packbits(start, bitorder="little").view("<u4")
    return words & np.asarray(base, dtype=np.uint32)


def same_bits(a, b) -> bool:
    """fp32 arrays equal bit for bit, except that any NaN equals any NaN (the payload of a NaN is not part of the contract)."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))
