"""tests/sample_ref.py (the host restatement of vt_sample_rows) pinned against transformers' RepetitionPenaltyLogitsProcessor,
TopKLogitsWarper and TopPLogitsWarper -- the classes themselves when `transformers` imports, and always their 4.31 rules restated in
torch as tests/test_gpu_kernels.py restates them; SamplingParams' validation, the packing of struct vt_sample_row against the header, and
ServingEngine.submit refusing bad parameters before it queues anything. No GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:                                              # the classes themselves, where the package is there and loads
    from transformers import RepetitionPenaltyLogitsProcessor, TopKLogitsWarper, TopPLogitsWarper
    HF = True
except Exception:  # noqa: BLE001
    HF = False


def _rows(V=257, n=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, V), generator=g) * 3.0
    x[0, 11] = 40.0                               # a dominant token
    x[1] = x[1].round()                           # ties everywhere
    x[2, 5] = 0.0                                 # a zero, both signs around it
    x[3, 20:24] = x[3].topk(7).values[-1]         # four more values tie with the 7th largest
    return x


# ---- the 4.31 rules, restated in torch ---------------------------------------------------------------------------------------------------
def rule_penalty(scores, input_ids, penalty):
    s = scores.clone()
    score = torch.gather(s, 1, input_ids)
    score = torch.where(score < 0, score * penalty, score / penalty)
    s.scatter_(1, input_ids, score)
    return s


def rule_top_k(scores, k):
    k = min(k, scores.size(-1))
    return scores.masked_fill(scores < torch.topk(scores, k)[0][..., -1, None], -float("inf"))


def rule_top_p(scores, top_p):
    sorted_logits, sorted_indices = torch.sort(scores, descending=False)
    cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    remove = cumulative_probs <= (1 - top_p)
    remove[..., -1:] = 0
    return scores.masked_fill(remove.scatter(1, sorted_indices, remove), -float("inf"))


def test_penalty_is_the_processor_bit_for_bit():
    x = _rows()
    hist = torch.tensor([[0, 5, 11, 31, 32, 256, 5, 5, 100, 11]] * x.shape[0])          # duplicates, the ends of the row, the zero at 5
    for p in (1.3, 0.8):
        want = rule_penalty(x, hist, p)
        got = np.stack([R.repetition_penalty(x[r].numpy(), hist[r].tolist(), p) for r in range(x.shape[0])])
        assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
        if HF:
            hf = RepetitionPenaltyLogitsProcessor(p)(hist, x.clone())
            assert np.array_equal(got.view(np.uint32), hf.numpy().view(np.uint32))
    # ids outside [0, V) -- the negative sentinels of a multimodal prompt, ids of a larger vocabulary -- are skipped, duplicates apply once
    row = x[2].numpy()
    a = R.repetition_penalty(row, [-200, -300, 5, 5, 257, 10 ** 6, 7], 1.3)
    b = R.repetition_penalty(row, [5, 7], 1.3)
    assert np.array_equal(a, b) and a[5] == 0.0 and a[7] == (row[7] * np.float32(1.3) if row[7] < 0 else row[7] / np.float32(1.3))
    assert np.array_equal(R.repetition_penalty(row, [], 1.3), row) and np.array_equal(R.repetition_penalty(row, [3], 1.0), row)


@pytest.mark.parametrize("k", [1, 7, 50, 0, 1000])
def test_top_k_keep_set(k):
    x = _rows()
    got = R.top_k_keep(x.numpy(), k)
    want = torch.isfinite(rule_top_k(x, k)).numpy() if 0 < k else np.ones_like(got)
    assert np.array_equal(got, want)
    if k == 7:
        assert got[3].sum() == 11 and got[0].sum() == 7                      # ties with the k-th value stay
    if HF and k > 0:
        assert np.array_equal(got, torch.isfinite(TopKLogitsWarper(k)(None, x.clone())).numpy())


def _same_keep_set(x, got, want):
    """Equal keep-sets; where scores TIE at the boundary the sort decides which of the tied tokens stay (torch.sort is not stable), so
    there the kept VALUES must agree, token for token everywhere else."""
    for r in range(x.shape[0]):
        if not np.array_equal(got[r], want[r]):
            diff = got[r] != want[r]
            assert len(set(x[r][diff].tolist())) == 1 and got[r].sum() == want[r].sum(), r
            assert np.array_equal(np.sort(x[r][got[r]]), np.sort(x[r][want[r]])), r


@pytest.mark.parametrize("top_p", [0.5, 0.9, 0.95, 1.0])
def test_top_p_keep_set(top_p):
    x = _rows().double()                                                      # fp64 on both sides: the rule, not a rounding
    got = R.top_p_keep(x.numpy(), top_p)
    want = torch.isfinite(rule_top_p(x, top_p)).numpy()
    _same_keep_set(x.numpy(), got, want)
    assert got[0].sum() == (x.shape[1] if top_p >= 1.0 else 1) and got[0, 11]      # the dominant token: a keep-set of one
    if top_p >= 1.0:
        assert got.all()
    if HF:
        _same_keep_set(x.numpy(), got, torch.isfinite(TopPLogitsWarper(top_p)(None, x.clone())).numpy())
    # after top-k: the nucleus is taken over what top-k left (-inf stays out)
    xk = rule_top_k(x, 7)
    got = R.top_p_keep(xk.numpy(), top_p)
    _same_keep_set(xk.numpy(), got, torch.isfinite(rule_top_p(xk, top_p)).numpy())
    assert not got[~torch.isfinite(xk).numpy()].any()


def test_whole_rule_order_uniform_and_walk():
    x = _rows()[4].numpy()
    hist = [int(np.argmax(x)), 3, 3, -200]
    keep = R.keep_set(x, 0.7, 5, 0.9, 1.3, hist)
    chain = rule_top_p(rule_top_k(rule_penalty(torch.tensor(x)[None], torch.tensor([hist[:3]]), 1.3).double() / 0.7, 5), 0.9)
    assert np.array_equal(keep, torch.isfinite(chain)[0].numpy()) and 1 <= keep.sum() <= 5
    # the uniform: a pure function of (seed, counter, stream), inside (0, 1), the roles of vt_sample_top_p's (seed, step, row)
    u = [float(R.uniform24(7, c, s)) for c in range(64) for s in range(8)]
    assert all(0.0 < v < 1.0 for v in u) and len(set(u)) == len(u) and abs(np.mean(u) - 0.5) < 0.05
    assert R.uniform24(7, 3, 2) == R.uniform24(7 + 2 ** 64, 3, 2) != R.uniform24(7, 2, 3)
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF                             # the published first output of the generator seeded 0
    # the walk: draws come from the keep-set and follow it; greedy rows take the first maximum of the PENALISED row
    toy = np.full(64, -1e4, dtype=np.float32)
    toy[:4] = np.log(np.array([0.5, 0.25, 0.15, 0.10], dtype=np.float32))
    ids = np.array([R.sample_row(toy, 1.0, 0, 1.0, 1.0, (), 11, c, 0)[0] for c in range(2000)])
    assert (ids < 4).all() and np.abs(np.bincount(ids, minlength=4) / 2000 - [0.5, 0.25, 0.15, 0.10]).max() < 0.04
    ids = np.array([R.sample_row(toy, 1.0, 0, 0.7, 1.0, (), 11, c, 0)[0] for c in range(500)])
    assert (ids < 2).all()
    t = np.array([1.0, 3.0, 3.0, -1.0], dtype=np.float32)
    assert R.sample_row(t, 0.0, 0, 1.0, 1.0, (), 0, 0, 0)[0] == 1 and R.sample_row(t, 0.0, 0, 1.0, 1.3, [1], 0, 0, 0)[0] == 2
    assert R.sample_row(t, 0.0, 0, 1.0, 4.0, [1, 2], 0, 0, 0)[0] == 0


def test_logprob_bound_admits_fp32_in_any_order_and_rejects_the_penalised_row():
    g = np.random.default_rng(5)
    rows = [g.standard_normal(4000).astype(np.float32) * 3, (g.standard_normal(4000) * 1e-3).astype(np.float32)]
    rows.append(rows[0].copy())
    rows[2][77] = 60.0
    for raw in rows:
        i = int(np.argmax(raw))
        ref, bound = R.logprob_ref(raw)[i], R.logprob_bound(raw, [i])[0]
        assert 0 < bound < 2e-5
        for order in (None, np.argsort(raw), np.argsort(-raw), g.permutation(raw.size)):
            assert abs(float(R.logprob_f32_emulation(raw, i, order)) - ref) <= bound
        if raw.max() < 50:      # the fault the bound must catch: logprob of the penalised row (a token that dominates either way hides it)
            pen = R.repetition_penalty(raw, [i], 1.3)
            assert abs(float(R.logprob_f32_emulation(pen, i)) - ref) > bound
    assert R.lse_chain(32000) == 54 and R.lse_chain(40000) == 62


# ---- SamplingParams, the struct ------------------------------------------------------------------------------------------------------------
def test_sampling_params_validation():
    from vitron_amd.sampling import SamplingParams
    sp = SamplingParams()
    assert (sp.temperature, sp.top_p, sp.top_k, sp.seed, sp.repetition_penalty, sp.logprobs) == (0.0, 1.0, None, 0, 1.0, False)
    assert sp.resolved_top_k(types.SimpleNamespace()) == 50 and sp.resolved_top_k(types.SimpleNamespace(top_k=7)) == 7
    assert SamplingParams(top_k=0).resolved_top_k(types.SimpleNamespace(top_k=7)) == 0
    with pytest.raises(Exception):
        sp.temperature = 1.0                                                  # frozen
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=-1.0), dict(top_k=-1), dict(top_k=1.5),
                dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0), dict(repetition_penalty=float("inf")), dict(seed=1.5),
                dict(logprobs=1), dict(temperature="hot")):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    SamplingParams(temperature=0.7, top_p=0.9, top_k=5, seed=-3, repetition_penalty=1.3, logprobs=True)


def test_struct_packing_matches_the_header():
    from vitron_amd import sampling as S
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    body = re.search(r"typedef struct vt_sample_row \{(.*?)\} vt_sample_row;", hdr, flags=re.S).group(1)
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "const int*": C.c_void_p}
    fields = [(m.group(2), ctype[m.group(1)]) for m in re.finditer(r"^\s*(const int\*|\w+)\s+(\w+);", body, flags=re.M)]

    class Row(C.Structure):
        _fields_ = fields

    assert C.sizeof(Row) == S.ROW_BYTES == S.ROW_DTYPE.itemsize == 48
    assert [n for n, _ in fields] == list(S.ROW_DTYPE.names)
    for name, _ in fields:
        assert getattr(Row, name).offset == S.ROW_DTYPE.fields[name][1], name
        assert getattr(Row, name).size == S.ROW_DTYPE.fields[name][0].itemsize, name
    # the header's offset table says the same
    table = dict((m.group(3), int(m.group(1))) for m in re.finditer(r"^ \*\s+(\d+) (float|int32|uint64|uint32|const int\*)\s+(\w+)", hdr, flags=re.M))
    assert table == {n: S.ROW_DTYPE.fields[n][1] for n in S.ROW_DTYPE.names}
    # round trip through the bytes the device reads
    rows = [(0.7, 5, 0.9, 1.3, -1, 3, 2, 0x7F0000001000, 1500), (0.0, 0, 1.0, 1.0, 2 ** 63 + 5, 2 ** 40, 2 ** 32 - 1, 0, 0)]
    raw = S.sample_rows_array(rows).tobytes()
    assert len(raw) == 96
    back = [Row.from_buffer_copy(raw[i * 48:(i + 1) * 48]) for i in range(2)]
    assert (back[0].temperature, back[0].top_p) == (np.float32(0.7), np.float32(0.9)) and back[0].repetition_penalty == np.float32(1.3)
    assert (back[0].top_k, back[0].seed, back[0].counter, back[0].stream, back[0].history, back[0].history_len) == \
        (5, 2 ** 64 - 1, 3, 2, 0x7F0000001000, 1500)
    assert (back[1].temperature, back[1].seed, back[1].counter, back[1].stream, back[1].history) == (0.0, 2 ** 63 + 5, 2 ** 40, 2 ** 32 - 1, None)
    for bad in ((-1.0, 0, 1.0, 1.0, 0, 0, 0, 0, 0), (1.0, -1, 1.0, 1.0, 0, 0, 0, 0, 0), (1.0, 0, 0.0, 1.0, 0, 0, 0, 0, 0), (1.0, 0, 1.0, 0.0, 0, 0, 0, 0, 0),
                (1.0, 0, 1.0, 1.0, 0, 0, 0, 0, 4), (1.0, 0, 1.0, 1.0, 0, -1, 0, 0, 0), (1.0, 0, 1.0, 1.0, 0, 0, 2 ** 32, 0, 0)):
        with pytest.raises(ValueError):
            S.sample_rows_array([bad])


def test_the_sampler_source_is_built():
    from vitron_amd import build
    assert "vt_sample.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "vitron_amd", "csrc", "vt_sample.hip"))


def test_submit_rejects_bad_sampling_before_queueing():
    from vitron_amd import serving
    from vitron_amd.sampling import SamplingParams
    model = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2), device="cpu", kv=None)
    eng = serving.ServingEngine(model, max_batch=4)
    ids = torch.ones((1, 5), dtype=torch.long)
    broken = SamplingParams()
    object.__setattr__(broken, "repetition_penalty", 0.0)                     # what the frozen dataclass would have refused
    with pytest.raises(TypeError):
        eng.submit(ids, sampling={"temperature": 0.7})
    with pytest.raises(ValueError):
        eng.submit(ids, sampling=broken)
    with pytest.raises(ValueError):
        eng.submit(ids, sampling=SamplingParams(top_p=0.0))
    assert not eng.waiting and eng.pending() == 0 and eng._next_id == 0
    rid = eng.submit(ids, sampling=SamplingParams(temperature=0.7, seed=3))
    assert rid == 0 and eng.waiting[0].sampling.seed == 3 and eng.submit(ids) == 1 and eng.waiting[1].sampling is None
    with pytest.raises(KeyError):
        eng.logprobs(rid)                                                     # nothing emitted yet
