"""tests/logprob_ref.py (the host restatement of vt_logprob_rows) pinned against torch.log_softmax / torch.topk on rows
without ties and against hand-written rows with ties, NaN, -inf, V < n_top and out-of-range targets; its bound against an fp32 emulation
of the kernel's own summation; and the host pieces of the feature: SamplingParams(top_logprobs=), generate()'s refusals, the binding, and
how score() maps the positions of input_ids to spliced rows and targets. No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import sample_ref as R

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (7, 512, 4099))
def test_rows_without_ties_equal_torch(V):
    g = torch.Generator().manual_seed(V)
    x = torch.stack([(torch.randperm(V, generator=g).float() / V - 0.5) * 12.0 for _ in range(5)])      # distinct values in a row
    assert all(len(set(r.tolist())) == V for r in x)                      # no ties: torch.topk's order is defined
    n = min(LR.MAX_TOP, V)
    ids, lp = LR.top(x.numpy(), n)
    want = torch.topk(x, n, dim=-1)
    ls = torch.log_softmax(x.double(), -1)
    assert np.array_equal(ids, want.indices.numpy().astype(np.int32))
    assert np.array_equal(lp, torch.gather(ls, 1, want.indices).numpy())
    t = torch.randint(0, V, (5,), generator=g)
    assert np.array_equal(LR.target_lp(x.numpy(), t.numpy()), ls[torch.arange(5), t].numpy())
    want_rank = [(x[r] > x[r, t[r]]).sum().item() + 1 for r in range(5)]
    assert LR.rank(x.numpy(), t.numpy()).tolist() == want_rank
    assert [int(LR.rank(x[r].numpy(), [ids[r, k]])[0]) for r in range(5) for k in range(n)] == list(range(1, n + 1)) * 5
    assert np.allclose(LR.lse64(x.numpy()), torch.logsumexp(x.double(), -1).numpy(), rtol=0, atol=0)


def test_hand_written_rows():
    row = np.array([1.0, 3.0, 3.0, -INF, 2.0, 3.0, -INF, 0.5], dtype=np.float32)
    assert LR.order(row).tolist() == [1, 2, 5, 4, 0, 7, 3, 6]             # ties to the lower index; -inf is an ordinary last value
    ids, lp = LR.top(row, 10)                                             # V = 8 < n_top: (-1, NaN) padding
    assert ids[0].tolist() == [1, 2, 5, 4, 0, 7, 3, 6, -1, -1]
    assert lp[0, 6] == -INF and lp[0, 7] == -INF and np.isnan(lp[0, 8:]).all() and np.isfinite(lp[0, :6]).all()
    assert lp[0, 0] == lp[0, 1] == lp[0, 2]
    assert LR.rank(np.tile(row, (8, 1)), np.arange(8)).tolist() == [5, 1, 2, 7, 4, 3, 8, 6]
    assert LR.rank(np.tile(row, (4, 1)), [-1, 8, 2 ** 31 - 1, -2 ** 31]).tolist() == [0, 0, 0, 0]
    assert np.isnan(LR.target_lp(np.tile(row, (2, 1)), [-1, 8])).all() and LR.target_lp(row, [3])[0] == -INF
    # a NaN is never taken and never counted; the row's log-probabilities are all NaN; a NaN target stands behind everything else
    nan_row = np.array([2.0, NAN, 5.0, 2.0], dtype=np.float32)
    assert LR.order(nan_row).tolist() == [2, 0, 3]
    ids, lp = LR.top(nan_row, 4)
    assert ids[0].tolist() == [2, 0, 3, -1] and np.isnan(lp).all() and np.isnan(LR.lse64(nan_row)).all()
    assert LR.rank(np.tile(nan_row, (4, 1)), [0, 1, 2, 3]).tolist() == [2, 4, 1, 3]
    assert LR.order(np.full((4,), NAN, dtype=np.float32)).size == 0
    same = np.full((6,), 0.25, dtype=np.float32)
    assert LR.order(same).tolist() == list(range(6)) and LR.rank(np.tile(same, (2, 1)), [0, 5]).tolist() == [1, 6]
    assert np.allclose(LR.top(same, 3)[1], -np.log(6.0))
    assert LR.order(np.array([-INF, INF, 0.0], dtype=np.float32)).tolist() == [1, 2, 0]


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------------
def _kernel_sum_f32(e, V, reg):
    """fp32 emulation of logprob_rows_kernel's sum: per-thread serial sums over the slots the thread owns, a 6-level xor butterfly per wave,
    16 serial additions of the wave totals."""
    F = np.float32
    per = np.zeros((1024,), dtype=F)
    if reg:
        pad = np.zeros((32768,), dtype=F)
        pad[:V] = e
        own = pad.reshape(8, 1024, 4)                     # [j][t][k]: float 4 (t + 1024 j) + k
        for j in range(8):
            for k in range(4):
                per = (per + own[j, :, k]).astype(F)
    else:                                                 # single loads: thread t adds t, t + 1024, ...
        pad = np.zeros((-(-V // 1024) * 1024,), dtype=F)
        pad[:V] = e
        for chunk in pad.reshape(-1, 1024):
            per = (per + chunk).astype(F)
    w = per.reshape(16, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, np.arange(64) ^ o]).astype(F)
    z = F(0)
    for v in w[:, 0]:
        z = F(z + v)
    return z


@pytest.mark.parametrize("V,reg", ((512, True), (32000, True), (32003, False)))
def test_the_bound_admits_the_kernels_arithmetic_and_little_more(V, reg):
    g = torch.Generator().manual_seed(9 + V)
    x = (torch.randn((V,), generator=g) * 3.0).numpy().astype(np.float32)
    m = x.max()
    e = np.exp((x - m).astype(np.float32)).astype(np.float32)
    lse = np.float32(m + np.log(_kernel_sum_f32(e, V, reg)).astype(np.float32))
    ids = LR.order(x)[:5]
    got = (x[ids] - lse).astype(np.float32)
    want = LR.log_softmax64(x)[ids]
    chain = LR.lse_chain(V, reg)
    assert chain == (54 if reg else 4 * 8 + 1 + 22)
    bound = LR.logprob_bound(x[None], want[None], chain)[0]
    ratio = np.abs(got.astype(np.float64) - want) / bound
    assert (ratio <= 1.0).all() and LR.worst_ratio(got[None], want[None], bound[None]) == float(ratio.max())
    assert (bound < 2e-5).all()                                           # ... and it is tight enough to catch a wrong term:
    assert (np.abs((x[ids] - np.float32(lse + 1e-4)).astype(np.float64) - want) > bound).all()
    assert abs(float(lse) - LR.lse64(x)[0]) <= LR.lse_bound(x[None], chain)[0]
    # the same terms as the sampler's bound, with this kernel's chain length in place of its own
    mine = LR.logprob_bound(x[None], want[:1], R.lse_chain(V))
    assert np.allclose(mine, R.logprob_bound(x[None], ids[:1]), rtol=1e-12, atol=0)


def test_bound_of_entries_that_are_not_finite_is_zero_and_they_compare_exactly():
    x = np.array([[0.0, -INF, 1.0]], dtype=np.float32)
    want = LR.log_softmax64(x)
    b = LR.logprob_bound(x, want, 54)
    assert b[0, 1] == 0.0 and b[0, 0] > 0 and LR.worst_ratio(want.astype(np.float32), want, b) <= 1.0
    with pytest.raises(AssertionError):
        LR.worst_ratio(np.array([[want[0, 0], -1e30, want[0, 2]]]), want, b)
    with pytest.raises(AssertionError):
        LR.worst_ratio(np.array([[NAN, -INF, want[0, 2]]]), want, b)
    assert LR.register_form(32768, 32768) and not LR.register_form(32772, 32772) and not LR.register_form(1000, 1001)
    assert not LR.register_form(1000, 1000, 4)


# ---- SamplingParams(top_logprobs=) and generate()'s refusals -----------------------------------------------------------------------------------
def test_sampling_params_top_logprobs():
    from vitron_amd.sampling import SamplingParams
    d = SamplingParams()
    assert d.top_logprobs == 0 and not d.wants_logprobs and "top_logprobs" not in repr(d)
    a = SamplingParams(temperature=0.7, top_logprobs=5)
    assert a.top_logprobs == 5 and a.wants_logprobs and not a.logprobs and "top_logprobs=5" in repr(a)
    assert SamplingParams(top_logprobs=20).top_logprobs == 20 and SamplingParams(logprobs=True).wants_logprobs
    assert a != SamplingParams(temperature=0.7) and a == SamplingParams(temperature=0.7, top_logprobs=5) and hash(a) == hash(a.replace())
    assert a.replace(seed=3).top_logprobs == 5 and a.replace(top_logprobs=0) == SamplingParams(temperature=0.7)
    assert "top_logprobs" not in SamplingParams.__dataclass_fields__
    for bad in (-1, 21, 2.0, True, None, "5"):
        with pytest.raises(ValueError, match="top_logprobs"):
            SamplingParams(top_logprobs=bad)
    with pytest.raises(Exception):
        a.top_logprobs = 3


def _resolve(**kw):
    from types import SimpleNamespace

    from vitron_amd.picker import resolve_generate_args
    cfg = SimpleNamespace(eos_token_id=2, pad_token_id=0, vocab_size=512, top_k=50, kv_cache_dtype=None)
    args = dict(do_sample=False, temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=4, max_length=None, stopping_criteria=None,
                eos_token_id=None, pad_token_id=None, num_beams=1, seed=None, return_logits=False, padded_batch=False, repetition_penalty=1.0,
                return_logprobs=False, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None,
                allowed_token_ids=None, num_return_sequences=1, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None)
    args.update(kw)
    return resolve_generate_args(cfg, 8, **args)


def test_generate_arguments():
    a = _resolve()
    assert a.top_logprobs == 0 and not a.per_row
    b = _resolve(top_logprobs=5)
    assert b.top_logprobs == 5 and not b.per_row                          # the pick stays the launch it was (vt_argmax here)
    for bad in (-1, 21, 1.5, True):
        with pytest.raises(ValueError, match="top_logprobs"):
            _resolve(top_logprobs=bad)
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        _resolve(top_logprobs=5, num_beams=2)
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        _resolve(top_logprobs=5, padded_batch=True)


def test_the_entry_point_is_declared_bound_and_built():
    from vitron_amd import _lib, build
    hdr = (ROOT / "include" / "vitron_hip.h").read_text()
    m = re.search(r"int vt_logprob_rows\((.*?)\);", hdr, re.S)
    assert m is not None
    names = [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert names == ["logits", "rows", "V", "ldl", "target", "n_top", "lse", "target_lp", "target_rank", "top_ids", "top_lp", "stream"]
    assert len(_lib.SIGNATURES["vt_logprob_rows"][1]) == len(names)
    assert "vt_logprob.hip" in build.SOURCES and (ROOT / "vitron_amd" / "csrc" / "vt_logprob.hip").exists()
    assert re.search(r"#define VT_LOGPROB_MAX_TOP 20\b", hdr) and re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    for needle in ("never counted as ahead", "id -1", "ties go to the lower index", "VT_STATUS_ARG", "not read"):
        assert needle in hdr, needle
    from vitron_amd import ops
    from vitron_amd.sampling import SamplingParams
    assert ops.LOGPROB_MAX_TOP == LR.MAX_TOP == SamplingParams.TOP_LOGPROBS_MAX == 20


# ---- score(): positions -> spliced rows and targets --------------------------------------------------------------------------------------------
def test_score_targets_on_a_spliced_plan():
    from vitron_amd.constants import IMAGE_TOKEN_INDEX, OBJS_TOKEN_INDEX
    from vitron_amd.model.llava_arch import KIND_REGION, KIND_TOKEN, KIND_VISUAL, build_splice_plan_np
    from vitron_amd.scoring import score_targets
    IMG, OBJ = IMAGE_TOKEN_INDEX, OBJS_TOKEN_INDEX
    ids = [[1, 11, IMG, 12, 13, OBJ, 14, 15],            # text, an image block of 4 rows, text, a region row, text
           [IMG, 21, 22, 0, 0, 0, 0, 0],                 # a leading image: the token behind it is scored by the block's last row
           [1, 31, 32, 33, 0, 0, 0, 0]]                  # no image (it still consumes a feature slot); padded
    am = [[1] * 8, [1, 1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0]]
    plan, mask, _, lengths = build_splice_plan_np(np.array(ids), np.array(am), [(0, 4), (4, 4), (8, 4)], [0, 1, 2])
    assert lengths == [11, 6, 4]
    out = []
    for b in range(3):
        valid = [t for t, m in zip(ids[b], am[b]) if m]
        kinds = [int(k) for k, m in zip(plan[b, :, 0], mask[b]) if m]
        out.append(score_targets(valid, kinds))
    rows, targets, positions = out[0]
    assert [int(plan[0, r, 0]) for r in range(11)] == [KIND_TOKEN] * 2 + [KIND_VISUAL] * 4 + [KIND_TOKEN] * 2 + [KIND_REGION] + [KIND_TOKEN] * 2
    assert positions == [1, 3, 4, 6, 7]                  # never 0 (the first token), 2 (<image>) or 5 (<objs>)
    assert targets == [11, 12, 13, 14, 15]
    assert rows == [0, 5, 6, 8, 9]                       # 12 is scored by the image block's LAST row (5), 14 by the region row (8)
    assert out[1] == ([3, 4], [21, 22], [1, 2])          # rows 0 - 3 are the image; row 3 scores the first text token
    assert out[2] == ([0, 1, 2], [31, 32, 33], [1, 2, 3])
    # text only, and a plan that truncation cut short: the dropped tokens have no row
    assert score_targets([5, 6, 7], [0, 0, 0]) == ([0, 1], [6, 7], [1, 2])
    assert score_targets([5, 6, 7, 8], [0, 0]) == ([0], [6], [1])
    assert score_targets([5], [0]) == ([], [], [])
    with pytest.raises(ValueError):
        score_targets([5], [0, 0])


def test_option_scores_and_order():
    from vitron_amd.scoring import option_score, rank_order
    assert option_score([-1.0, -2.0, -0.5], "sum") == -3.5 and option_score([-1.0, -2.0, -0.5], "mean") == -3.5 / 3
    with pytest.raises(ValueError):
        option_score([-1.0], "median")
    assert rank_order([-3.0, -1.0, -3.0, -1.0, -0.5]) == [4, 1, 3, 0, 2]             # ties keep option order
    assert rank_order([-1.0, NAN, -0.5]) == [2, 0, 1]
