"""The contract of vt_bias_rows and of the adjusted value of vt_sample_rows_adj (include/vitron_hip.h) restated as plain
numpy fp32 loops, independent of the product's sampling.logit_adjust. Every arithmetic step is one fp32 operation: numpy rounds each,
so a kernel that fuses a product into a sum differs from this in the last bit."""
import numpy as np

from tests import sample_ref as S

F32 = np.float32
MAX_COUNT = 65535


def bias_rows(V, history, ids, vals, presence, frequency):
    """(pre, post), fp32 [V] each. pre[t] = vals[j] where ids[j] == t (ids outside [0, V) skipped), else 0. post[t] = 0 where t does not
    occur among the last 65535 ids of `history` (ids outside [0, V) skipped), else -(frequency * count + presence), the product and the
    sum rounded separately."""
    V = int(V)
    pre = np.zeros((V,), dtype=F32)
    for t, v in zip(ids, vals):
        if 0 <= int(t) < V:
            pre[int(t)] = F32(v)
    count = np.zeros((V,), dtype=np.int64)
    for t in list(history)[-MAX_COUNT:]:
        if 0 <= int(t) < V:
            count[int(t)] += 1
    post = np.zeros((V,), dtype=F32)
    f, p = F32(frequency), F32(presence)
    for t in np.flatnonzero(count):
        prod = F32(f * F32(count[t]))
        post[t] = -F32(prod + p)
    return pre, post


def adjusted(raw, allow_bool, pre, post, penalty=1.0, pen_history=()):
    """The fp32 row the sampler works on: raw, -inf where allow_bool is False (None: everything allowed), + pre, the repetition
    penalty of tests/sample_ref.py on the ids of pen_history (penalty 1: none), + post."""
    x = np.array(raw, dtype=F32, copy=True)
    if allow_bool is not None:
        x[~np.asarray(allow_bool, dtype=bool)] = -np.inf
    x = (x + np.asarray(pre, dtype=F32)).astype(F32)
    if float(penalty) != 1.0 and len(pen_history):
        x = S.repetition_penalty(x, pen_history, penalty)
    return (x + np.asarray(post, dtype=F32)).astype(F32)
