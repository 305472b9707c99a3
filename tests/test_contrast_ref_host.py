"""Contrastive search on the host: tests/contrast_ref.py on hand-computed cases, the tie rule, the decoding loop on a toy
model, contrastive.CandidateGroup's page plan against a fake pool, the selection gap of every random case of tests/contrast_cases.py (the
premise of the GPU test's exact selections), the C ABI's two new entry points, and the resolver's refusals with their order."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import contrast_cases as CC
from tests import contrast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_unit_rows_by_hand():
    got = R.unit_rows(np.array([[3.0, 4.0], [0.0, 0.0], [-2.0, 0.0]], F32))
    assert np.allclose(got, [[0.6, 0.8], [0.0, 0.0], [-1.0, 0.0]], atol=1e-15) and not np.isnan(got).any()
    got = R.unit_rows(np.array([[3.0, 2.0]], F32), np.array([1.0, 2.0], F32))              # y = (3, 4)
    assert np.allclose(got, [[0.6, 0.8]], atol=1e-15)
    x = np.random.default_rng(1).standard_normal((5, 33)).astype(F32)
    assert np.allclose((R.unit_rows(x) ** 2).sum(-1), 1.0, atol=1e-14)
    # RMSNorm's per-row scalar cancels: the direction of w * x is that of w * (x * any positive scalar)
    w = np.random.default_rng(2).standard_normal(33).astype(F32)
    assert np.allclose(R.unit_rows(x, w), R.unit_rows(x * F32(0.125), w), atol=1e-15)


def test_d_score_sel_by_hand():
    bank = np.array([[1.0, 0.0], [0.0, 1.0]])
    cand = np.array([[1.0, 0.0], [0.6, 0.8], [-1.0, 0.0]])
    d, bound = R.d_of(bank, cand)
    assert d.tolist() == [1.0, 0.8, 0.0] and (bound >= 0).all()
    assert R.d_of(bank[:1], cand)[0].tolist() == [1.0, 0.6, -1.0]                          # the maximum may be negative: it is not clamped at 0
    lp = np.log(np.array([0.5, 0.25, 0.125])).astype(F32)
    s = R.score(0.5, lp, d)
    assert np.allclose(s, [0.25 - 0.5, 0.125 - 0.4, 0.0625 - 0.0], atol=1e-7) and R.select(s) == 2
    assert R.select(R.score(0.0, lp, d)) == 0                                              # alpha = 0: the most probable candidate
    assert R.select(R.score(1.0, lp, d)) == 2                                              # alpha = 1: the least similar one
    sb = R.score_bound(0.5, lp, d, bound)
    assert (sb > 0).all() and (sb < 1e-5).all()


def test_tie_rule_and_range():
    assert R.select([1.0, 1.0, 0.5]) == 0 and R.select([0.5, 1.0, 1.0]) == 1 and R.select([3.0]) == 0
    assert R.select([float("nan"), 1.0]) == 0 and R.select([0.0, float("nan"), 1.0]) == 2  # a NaN never wins; sel stays inside [0, k)
    ids, lp = R.top_k(np.array([1.0, 3.0, 3.0, -1.0, 2.0]), 3)
    assert ids.tolist() == [1, 2, 4] and abs(float(np.exp(lp[0])) - math.exp(3) / (math.exp(1) + 2 * math.exp(3) + math.exp(-1) + math.exp(2))) < 1e-12


class ToyModel:
    """A deterministic numpy 'decoder': the hidden state of a position is tanh of a decayed sum of the embeddings before it; prone to
    repeating itself under greedy decoding, which is what the degeneration penalty acts on."""

    def __init__(self, V=24, H=16, seed=0):
        rng = np.random.default_rng(seed)
        self.E = rng.standard_normal((V, H))
        self.W = self.E.T * 0.3 + 0.1 * rng.standard_normal((H, V))

    def hidden(self, ids):
        h, out = np.zeros(self.E.shape[1]), []
        for t in ids:
            h = np.tanh(0.5 * h + self.E[t])
            out.append(h)
        return np.array(out)

    def run(self, prompts, k, alpha, max_new, eos=(), pad=0, stop=None):
        seqs = [list(p) for p in prompts]
        banks = [list(R.unit_rows(self.hidden(p))) for p in seqs]
        cur = [self.hidden(p)[-1] @ self.W for p in seqs]
        lps = {}

        def candidates(live):
            res = []
            for b in live:
                ids, lps[b] = R.top_k(cur[b], k)
                res.append(ids.tolist())
            return res

        def step(live, cands):
            sels = []
            for j, b in enumerate(live):
                hs = [self.hidden(seqs[b] + [c])[-1] for c in cands[j]]
                units = R.unit_rows(np.array(hs))
                d, _ = R.d_of(np.array(banks[b]), units)
                sel = R.select(R.score(alpha, lps[b], d))
                sels.append(sel)
                seqs[b].append(cands[j][sel])
                banks[b].append(units[sel])
                cur[b] = hs[sel] @ self.W
            return sels
        return R.contrastive_loop(len(prompts), k, max_new, eos, pad, candidates, step, stop)

    def greedy(self, prompt, max_new):
        ids = list(prompt)
        for _ in range(max_new):
            ids.append(int(R.top_k(self.hidden(ids)[-1] @ self.W, 1)[0][0]))
        return ids[len(prompt):]


def test_loop_on_a_toy_model():
    m = ToyModel()
    prompts = [[1, 2, 3], [4, 5]]
    greedy = [m.greedy(p, 8) for p in prompts]
    assert m.run(prompts, 4, 0.0, 8) == greedy                                              # alpha = 0 is greedy decoding
    assert m.run(prompts, 1, 0.6, 8) == greedy                                              # one candidate is greedy decoding
    got = m.run(prompts, 4, 0.6, 8)
    assert got != greedy and [m.run([p], 4, 0.6, 8)[0] for p in prompts] == got             # the penalty acts; rows are independent
    assert any(len(set(g)) < len(set(c)) for g, c in zip(greedy, got))                      # it breaks a repetition greedy falls into
    # EOS pads the finished row while the other goes on; everything stops when all rows have finished or the caller says so
    eos = got[0][2]
    out = m.run(prompts, 4, 0.6, 8, eos=[eos], pad=99)
    first = got[0].index(eos)
    assert out[0][:first + 1] == got[0][:first + 1] and set(out[0][first + 1:]) <= {99}
    stopped = m.run(prompts, 4, 0.6, 8, stop=lambda rows: len(rows[0]) == 3)
    assert [len(r) for r in stopped] == [3, 3] and stopped == [g[:3] for g in got]


# ---- the premise of the GPU test's exact selections ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(CC.LAUNCHES)))
def test_every_random_case_has_a_selection_gap(i, dtype):
    """For every group of every launch: the fp64 gap between the best and the second-best score exceeds GAP_FACTOR x the sum of the two
    scores' error bounds, so no admissible kernel can select another candidate. (A seed that fails this is changed, not the factor.)"""
    for g in CC.launch_case(i, dtype):
        assert g["bank"].shape == (g["T"], CC.LAUNCHES[i]["H"]) and g["cand"].shape[0] == g["k"]
        assert (np.diff(g["lp"]) <= 0).all() and float(np.exp(g["lp"].astype(np.float64)).sum()) < 1.0
        d, db = R.d_of(g["bank"], g["cand"])
        s = R.score(g["alpha"], g["lp"], d)
        sb = R.score_bound(g["alpha"], g["lp"], d, db)
        if g["k"] == 1:
            continue
        order = np.argsort(-s, kind="stable")
        a, b = order[0], order[1]
        assert s[a] - s[b] > CC.GAP_FACTOR * (sb[a] + sb[b]), (i, g["T"], g["k"], s[a] - s[b], sb[a] + sb[b])
    sels = [R.select(R.score(g["alpha"], g["lp"], R.d_of(g["bank"], g["cand"])[0])) for g in CC.launch_case(i, dtype)]
    assert any(x != 0 for x in sels)                                                        # the penalty overturns the most probable one somewhere


# ---- CandidateGroup against a fake pool -------------------------------------------------------------------------------------------------------
class FakePool:
    """alloc / release of PagedKVCache over pages that hold 64 python values each; a page is given out at most once at a time"""

    def __init__(self, n):
        self.num_pages, self.free, self.data, self.out = n, list(range(n - 1, -1, -1)), {p: [None] * 64 for p in range(n)}, set()
        self.copies = []

    def alloc(self, n):
        if n > len(self.free):
            raise RuntimeError("out of pages")
        got = [self.free.pop() for _ in range(n)]
        assert not self.out & set(got)
        self.out |= set(got)
        return got

    def release(self, pages):
        for p in pages:
            assert p in self.out, f"page {p} released twice or never taken"
            self.out.discard(p)
            self.data[p] = [None] * 64                    # whoever still reads it reads nothing
        self.free.extend(pages)

    def copy(self, kv, src, dst):
        assert kv is self and len(src) == len(dst) and not set(src) & set(dst) and len(set(dst)) == len(dst)
        for a, b in zip(src, dst):
            self.data[b] = list(self.data[a])
        self.copies.append(len(src))


def _prefilled(pool, n):
    from vitron_amd.engine import SequenceState
    s = SequenceState()
    s.pages, s.length = pool.alloc((n + 63) // 64), n
    for j in range(n):
        pool.data[s.pages[j // 64]][j % 64] = ("p", j)
    return s


def _read(pool, seq):
    return [pool.data[seq.pages[j // 64]][j % 64] for j in range(seq.length)]


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("prompt_len", [1, 63, 64, 65, 130])
def test_candidate_group_page_plan(prompt_len, k):
    from vitron_amd.contrastive import CandidateGroup
    steps = 140
    pool = FakePool(16)
    grp = CandidateGroup(None, pool, _prefilled(pool, prompt_len), k, steps, copy_pages=pool.copy)
    assert sum(pool.copies) == (k - 1 if prompt_len % 64 else 0)
    private = [("p", j) for j in range(prompt_len)]                 # the private-copy model: what every slot's cache holds
    for t in range(steps):
        L = prompt_len + t
        assert all(s.length == L and len(s.pages) == L // 64 + 1 and _read(pool, s) == private for s in grp.seqs)
        assert all(s.pages[:-1] == grp.seqs[0].pages[:-1] for s in grp.seqs)                       # the completed pages are shared
        assert len({s.pages[-1] for s in grp.seqs}) == k                                            # the current page is the slot's own
        for c, s in enumerate(grp.seqs):                            # a decode step: slot c writes its candidate at position L
            pool.data[s.pages[L // 64]][L % 64] = ("g", t, c)
            s.length += 1
        before = len(pool.copies)
        sel = (5 * t + 3) % k
        n = grp.select(sel)
        assert n == sum(pool.copies[before:]) and n <= k - 1
        assert n == (0 if (L + 1) % 64 == 0 else k - 1)             # a page that has just filled is shared, not copied
        private.append(("g", t, sel))
    assert all(_read(pool, s) == private for s in grp.seqs)
    with pytest.raises(ValueError):
        grp.select(k)
    grp.release()
    grp.release()                                                   # a second release gives nothing back twice
    assert not pool.out and sorted(pool.free) == list(range(16))


def test_candidate_group_releases_on_failure():
    from vitron_amd.contrastive import CandidateGroup

    def broken(kv, src, dst):
        raise RuntimeError("copy failed")
    pool = FakePool(8)
    with pytest.raises(RuntimeError, match="copy failed"):
        CandidateGroup(None, pool, _prefilled(pool, 70), 4, 10, copy_pages=broken)
    assert not pool.out and len(pool.free) == 8
    pool = FakePool(3)                                              # too small: the prompt's pages go back as well
    with pytest.raises(RuntimeError, match="out of pages"):
        CandidateGroup(None, pool, _prefilled(pool, 70), 4, 10, copy_pages=pool.copy)
    assert not pool.out and len(pool.free) == 3


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_entry_points():
    import ctypes as C

    from vitron_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    for sym, n_args in (("vt_unit_rows", 8), ("vt_contrast_rows", 9)):
        m = re.search(r"^int\s+" + sym + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M | re.S)
        assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == n_args
        assert len(_lib.SIGNATURES[sym][1]) == n_args
    assert "#define VT_ABI_VERSION 114" in hdr                      # additive symbols: no bump
    assert C.sizeof(_lib.VtContrastRow) == 64 and _lib.VtContrastRow.alpha.offset == 56 and _lib.VtContrastRow.bank_len.offset == 40
    assert ops.CONTRAST_MAX_K == int(re.search(r"#define VT_CONTRAST_MAX_K (\d+)", hdr).group(1))
    assert ops.CONTRAST_CHUNK == int(re.search(r"#define VT_CONTRAST_CHUNK (\d+)", hdr).group(1))
    for operand in ("bf16", "fp16"):                                # the launchers refuse before any device work: no GPU needed
        lib = _lib.load(operand=operand)
        assert lib.vt_unit_rows(None, 8, None, None, 8, 1, 8, None) == -1 and "NULL" in _lib.last_error(lib)
        row = (_lib.VtContrastRow * 1)()
        assert lib.vt_contrast_rows(row, 1, None, 4, 64, 64, None, 0, None) == -1 and "NULL" in _lib.last_error(lib)
        assert lib.vt_contrast_rows(row, 0, 16, 4, 64, 64, None, 0, None) == -1 and "n_groups" in _lib.last_error(lib)
        assert lib.vt_contrast_rows(row, 1, 16, 4, 64, 48, None, 0, None) == -1 and "multiple of 32" in _lib.last_error(lib)


# ---- the resolver ---------------------------------------------------------------------------------------------------------------------------
def _resolve(**kw):
    from vitron_amd.picker import resolve_generate_args
    cfg = types.SimpleNamespace(eos_token_id=2, pad_token_id=0, vocab_size=64, top_k=50)
    args = dict(do_sample=False, temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=4, max_length=None, stopping_criteria=None,
                eos_token_id=None, pad_token_id=None, num_beams=1, seed=None, return_logits=False, padded_batch=False, repetition_penalty=1.0,
                return_logprobs=False, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None,
                allowed_token_ids=None, num_return_sequences=1, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None,
                batch_size=2)
    args.update(kw)
    return resolve_generate_args(cfg, 5, **args)


def test_generate_arguments_resolve():
    plain = _resolve()
    assert not plain.contrastive and plain.penalty_alpha == 0.0 and plain.given == ()
    for off in (dict(penalty_alpha=None), dict(penalty_alpha=0), dict(penalty_alpha=0.0, top_k=4), dict(penalty_alpha=0.6, top_k=1)):
        a = _resolve(**off)
        assert not a.contrastive and not a.per_row, off
    assert _resolve(penalty_alpha=None, top_k=4).given == () and _resolve(penalty_alpha=0, top_k=4).given == ()
    a = _resolve(penalty_alpha=0.6, top_k=4)
    assert a.contrastive and a.penalty_alpha == 0.6 and a.top_k == 4 and not a.per_row
    assert _resolve(penalty_alpha=1, top_k=16).contrastive and _resolve(penalty_alpha=0.6, top_k=2, stopping_criteria=[lambda i, s: False]).contrastive


def test_generate_arguments_refuse_in_order():
    for bad in (float("nan"), float("inf"), -0.1, 1.5, "0.6", True):
        with pytest.raises(ValueError, match="penalty_alpha"):
            _resolve(penalty_alpha=bad, top_k=4)
    with pytest.raises(ValueError, match="do_sample"):
        _resolve(penalty_alpha=0.6, top_k=4, do_sample=True)
    with pytest.raises(ValueError, match="penalty_alpha"):                                  # the value comes before the beam refusals
        _resolve(penalty_alpha=2.0, top_k=4, num_beams=2)
    with pytest.raises(NotImplementedError, match=r"num_beams > 1, penalty_alpha"):
        _resolve(penalty_alpha=0.6, top_k=4, num_beams=2)
    with pytest.raises(NotImplementedError, match="explicit top_k"):
        _resolve(penalty_alpha=0.6)
    for k in (0, 17, 50):
        with pytest.raises(NotImplementedError, match="top_k"):
            _resolve(penalty_alpha=0.6, top_k=k)
    refused = [(dict(padded_batch=True), "padded_batch"), (dict(repetition_penalty=1.2), "repetition_penalty"),
               (dict(suppress_tokens=[5]), "suppress_tokens"), (dict(begin_suppress_tokens=[5]), "begin_suppress_tokens"),
               (dict(min_new_tokens=2), "min_new_tokens"), (dict(bad_words_ids=[[5]]), "bad_words_ids"),
               (dict(allowed_token_ids=[5, 6, 7]), "allowed_token_ids"), (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"),
               (dict(return_logits=True), "return_logits"), (dict(return_logprobs=True), "return_logprobs"),
               (dict(sequence_bias={(5,): 1.0}), "sequence_bias"), (dict(presence_penalty=0.5), "presence_penalty"),
               (dict(frequency_penalty=0.5), "frequency_penalty"), (dict(top_logprobs=3), "top_logprobs"),
               (dict(choices=[[5, 6]]), "automaton"), (dict(guidance_scale=2.0), "guidance_scale")]
    for kw, name in refused:
        with pytest.raises(NotImplementedError, match=name):
            _resolve(penalty_alpha=0.6, top_k=4, **kw)
        _resolve(penalty_alpha=0.6, top_k=1, **{k: v for k, v in kw.items() if k != "padded_batch"})     # top_k = 1: the mode is off, nothing refused
    # the order: top_k before padded_batch before repetition_penalty before the optional arguments
    with pytest.raises(NotImplementedError, match="explicit top_k"):
        _resolve(penalty_alpha=0.6, padded_batch=True, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match="padded_batch"):
        _resolve(penalty_alpha=0.6, top_k=4, padded_batch=True, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        _resolve(penalty_alpha=0.6, top_k=4, repetition_penalty=1.2, return_logits=True)
    # a sampling call does not consume the RNG for a refused contrastive call, and a greedy one never does
    state = torch.random.get_rng_state()
    with pytest.raises(NotImplementedError):
        _resolve(penalty_alpha=0.6)
    assert torch.equal(torch.random.get_rng_state(), state)
