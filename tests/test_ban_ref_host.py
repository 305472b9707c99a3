"""tests/ban_ref.py (the host restatement of vt_ban_rows' contract) and sampling.history_bans (the product's own) pinned: both against
transformers' NoRepeatNGramLogitsProcessor and NoBadWordsLogitsProcessor -- the installed classes wherever the `transformers` package is
present -- and against each other; the histories that MUST ban something; sentinels and degenerate sizes; struct vt_ban_row's packing,
the flattened sequences, SamplingParams' two arguments, the header. No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import ban_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HF = importlib.util.find_spec("transformers") is not None
if HF:
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor

VS = (31, 32, 33, 64, 1000)
NS = (1, 2, 3, 5, 64, 255, 256, 257, 700)
GS = (1, 2, 3, 4)


def _hf_banned(proc, history, V):
    """The ids the processor sets to -inf on a zero score row"""
    out = proc(torch.tensor([history], dtype=torch.long), torch.zeros((1, V)))
    return np.flatnonzero(torch.isinf(out[0]).numpy()).tolist()


def _random_case(V, n, g, a, rng):
    alphabet = rng.choice(V, size=a, replace=False).tolist()
    h = rng.choice(alphabet, size=n).tolist()
    seqs = [rng.choice(alphabet, size=int(rng.integers(1, 5))).tolist() for _ in range(4)]
    return h, seqs


@pytest.mark.parametrize("V", VS)
def test_both_restatements_are_the_processors(V):
    """ban_ref and sampling.history_bans equal the installed NoRepeatNGram / NoBadWords processors on random histories over small
    alphabets. The sequence rule is compared where n >= L for every sequence: the installed transformers ignores a sequence longer than
    the context, this contract needs only its L - 1 leading ids (pinned below)."""
    from vitron_amd.sampling import history_bans
    rng = np.random.default_rng(900 + V)
    compared = [0, 0]
    for n in NS:
        for g in GS:
            for a in (2, 3, 4):
                h, seqs = _random_case(V, n, g, a, rng)
                ng, sq = R.banned(V, h, g, ()), R.banned(V, h, 0, seqs)
                assert history_bans(V, h, g, None) == ng and history_bans(V, h, 0, seqs) == sq, (V, n, g, a)
                assert history_bans(V, h, g, seqs) == R.banned(V, h, g, seqs) == sorted(set(ng) | set(sq))
                if HF:
                    assert _hf_banned(NoRepeatNGramLogitsProcessor(g), h, V) == ng, (V, n, g, h[:8])
                    compared[0] += 1
                    if all(n >= len(s) for s in seqs):
                        assert _hf_banned(NoBadWordsLogitsProcessor(seqs, None), h, V) == sq, (V, n, seqs, h[-4:])
                        compared[1] += 1
    if HF:
        assert compared[0] == len(NS) * len(GS) * 3 and compared[1] >= len(NS) * len(GS) * 3 // 2


def test_a_sequence_needs_only_its_leading_ids():
    """h = [a], s = [a, b]: b is banned by this contract (the L - 1 = 1 leading id is the end of the history). The installed
    transformers bans nothing here (it skips a sequence longer than the context): the one place where the two differ."""
    from vitron_amd.sampling import history_bans
    a, b, V = 7, 8, 33
    assert R.banned(V, [a], 0, [[a, b]]) == [b] == history_bans(V, [a], 0, [[a, b]])
    assert R.banned(V, [b], 0, [[a, b]]) == [] == history_bans(V, [b], 0, [[a, b]])
    assert R.banned(V, [], 0, [[a, b]]) == [] == history_bans(V, [], 0, [[a, b]])
    assert R.banned(V, [9, a], 0, [[a, b]]) == [b]
    if HF:
        assert _hf_banned(NoBadWordsLogitsProcessor([[a, b]], None), [a], V) == []
        assert _hf_banned(NoBadWordsLogitsProcessor([[a, b]], None), [9, a], V) == [b]


def test_periodic_histories_must_ban():
    """The cases the GPU comparison relies on for non-vacuity: h[i] = 7 + i % p bans something for every (p, n, g) of MUST_BAN, so a
    kernel that clears nothing cannot equal the reference there."""
    from vitron_amd.sampling import history_bans
    assert len(R.MUST_BAN) == 24
    for p, n, g in R.MUST_BAN:
        h = R.periodic(n, p)
        got = R.banned(64, h, g, ())
        assert got and got == history_bans(64, h, g, None), (p, n, g)
        if g > 1:
            assert got == [7 + n % p], (p, n, g, got)            # the id that continued the same g - 1 ids one period earlier
        else:
            assert got == list(range(7, 7 + p))
        if HF:
            assert _hf_banned(NoRepeatNGramLogitsProcessor(g), h, 64) == got


def test_sentinels_and_degenerate_sizes():
    from vitron_amd.sampling import history_bans
    V = 40
    both = lambda h, g, s=(): (R.banned(V, h, g, s), history_bans(V, h, g, s))          # noqa: E731
    # a sentinel inside the window takes part in the comparison like any other id
    h = [5, -200, 6, 9, 5, -200]
    assert both(h, 3) == ([6], [6])
    assert both([5, -200, 6, 9, 5, -300], 3) == ([], [])
    assert both([5, 1000, 6, 9, 5, 1000], 3) == ([6], [6])                               # an id >= V in the window
    # a sentinel / an id >= V as the id to clear is skipped
    assert both([5, -200, 9, 5], 2) == ([], [])
    assert both([5, V, 9, 5], 2) == ([], [])
    assert both([5, V - 1, 9, 5], 2) == ([V - 1], [V - 1])
    assert both([3, -200, V, 3], 1) == ([3], [3])
    assert both([1, 2], 0, [[-200, 4], [2, V], [2, -1], [2, 39]]) == ([39], [39])
    assert both([-200], 0, [[-200, 4], [V + 5]]) == ([4], [4])
    # g > n + 1: no open n-gram fits the history; g == n + 1: the window is the whole history, nothing precedes it
    assert both([1, 1, 1], 5) == ([], []) and both([1, 1, 1], 4) == ([], [])
    assert both([1, 1, 1], 3) == ([1], [1])
    # n == 0: only single-id sequences ban; g == 1 on an empty history bans nothing
    assert both([], 1) == ([], []) and both([], 3, [[4], [5, 6], [4]]) == ([4], [4])
    # duplicate sequences are one ban
    assert both([5], 0, [[5, 6], [5, 6], [6], [6]]) == ([6], [6])
    # the whole mask: base copied word for word (a bit at a position >= V included), then cleared
    base = np.array([0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    m = R.ban_mask(V, [3, 3], 1, (), base)
    assert [int(w) for w in m] == [0xFFFFFFF7, 0xFFFFFFFF]
    assert [int(w) for w in R.ban_mask(V, [35], 1)] == [0xFFFFFFFF, 0xF7]


def test_flattened_sequences_and_their_parsing():
    from vitron_amd.sampling import flatten_ban_seqs
    seqs = [[5], [6, 7], [8, 9, 10, 11]]
    flat = flatten_ban_seqs(seqs)
    assert flat.dtype == np.int32 and flat.tolist() == [1, 5, 2, 6, 7, 4, 8, 9, 10, 11]
    assert flatten_ban_seqs(None).tolist() == [] and flatten_ban_seqs([]).dtype == np.int32
    assert R.parse_seqs(flat, 3, flat.size) == seqs
    assert R.parse_seqs(flat, 2, flat.size) == seqs[:2]
    assert R.parse_seqs(flat, 3, flat.size - 1) == seqs[:2]                              # the last entry runs past seqs_len
    assert R.parse_seqs(flat, 9, flat.size) == seqs                                       # n_seqs beyond what the buffer holds
    assert R.parse_seqs([1, 5, 0, 6, 7], 3, 5) == [[5]] and R.parse_seqs([-1, 5], 1, 2) == []
    with pytest.raises(ValueError):
        flatten_ban_seqs([[5], []])
    with pytest.raises(ValueError):
        flatten_ban_seqs([[2 ** 31]])


def test_ban_row_struct():
    from vitron_amd.sampling import BAN_ROW_BYTES, BAN_ROW_DTYPE, ban_rows_array
    assert BAN_ROW_BYTES == 48 == BAN_ROW_DTYPE.itemsize
    arr = ban_rows_array([(0x1122334455667788, 7, 0x0102030405060708, 0x1112131415161718, 3, 0x2122232425262728, 2, 9),
                          (0, 0, 0, 0x40, -1, 0, 0, 0)])
    raw = arr.view(np.uint8).reshape(2, 48)
    u64 = lambda r, o: int(raw[r, o:o + 8].view("<u8")[0])                                # noqa: E731
    i32 = lambda r, o: int(raw[r, o:o + 4].view("<i4")[0])                                # noqa: E731
    assert (u64(0, 0), u64(0, 8), u64(0, 16), u64(0, 24)) == (0x1122334455667788, 0x0102030405060708, 0x1112131415161718, 0x2122232425262728)
    assert (i32(0, 32), i32(0, 36), i32(0, 40), i32(0, 44)) == (7, 3, 2, 9)
    assert (u64(1, 0), u64(1, 16), i32(1, 36)) == (0, 0x40, -1)
    with pytest.raises(ValueError):
        ban_rows_array([(0, 5, 0, 0x40, 2, 0, 0, 0)])                                    # a history length without a history
    # the header's table names the same offsets
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    doc = hdr[hdr.index("HISTORY-DEPENDENT BANS"):hdr.index("typedef struct vt_ban_row")]
    table = {m.group(2): int(m.group(1)) for m in re.finditer(r"^ \*\s+(\d+) (?:const )?u?int32_t\*?\s+(\w+)", doc, flags=re.M)}
    assert table == {n: BAN_ROW_DTYPE.fields[n][1] for n in BAN_ROW_DTYPE.names}, table
    body = re.search(r"typedef struct vt_ban_row \{(.*?)\} vt_ban_row;", hdr, flags=re.S).group(1)
    assert [ln.split()[-1].rstrip(";") for ln in body.strip().splitlines()] == list(BAN_ROW_DTYPE.names)


def test_sampling_params_history_bans():
    from vitron_amd.sampling import SamplingParams, check_constraints
    d = SamplingParams()
    assert d.no_repeat_ngram_size == 0 and d.bad_words is None and not d.constrained and not d.device_bans
    a = SamplingParams(no_repeat_ngram_size=3)
    b = SamplingParams(bad_words=[[5, 6], np.array([7])])
    assert a.constrained and a.device_bans and b.constrained and b.bad_words == ((5, 6), (7,))
    assert not SamplingParams(bad_words=[]).constrained
    assert a != d and a == SamplingParams(no_repeat_ngram_size=3) and hash(b) == hash(SamplingParams(bad_words=((5, 6), (7,))))
    assert "no_repeat_ngram_size=3" in repr(a)
    c = a.replace(bad_words=[[1, 2]], temperature=0.5)
    assert (c.no_repeat_ngram_size, c.bad_words, c.temperature) == (3, ((1, 2),), 0.5)
    with pytest.raises(Exception):
        a.no_repeat_ngram_size = 2                                                   # frozen like the rest
    for bad in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.0), dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size=None),
                dict(bad_words=[[]]), dict(bad_words=[5]), dict(bad_words="56"), dict(bad_words=[[1.5]]), dict(bad_words=[[True]])):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    V = 64
    check_constraints(SamplingParams(no_repeat_ngram_size=2, bad_words=[[5, 63], [0]]), [2], V)
    for bad in (SamplingParams(bad_words=[[5, 64]]), SamplingParams(bad_words=[[-1, 5]]), SamplingParams(bad_words=[[64]])):
        with pytest.raises(ValueError):
            check_constraints(bad, [2], V)
    # the static constraints keep their host checks beside a device ban
    with pytest.raises(ValueError):
        check_constraints(SamplingParams(no_repeat_ngram_size=2, allowed_token_ids=[3], banned_token_ids=[3]), [2], V)


def test_submit_takes_and_refuses_history_bans():
    import types

    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    stub = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=64), device="cpu")
    eng = ServingEngine(stub)
    ids = torch.tensor([[1, 5, 6]])
    with pytest.raises(ValueError):
        eng.submit(ids, sampling=SamplingParams(bad_words=[[5, 64]]))
    assert eng.pending() == 0
    rid = eng.submit(ids, sampling=SamplingParams(no_repeat_ngram_size=2, bad_words=[[5, 6]]))
    assert eng.pending() == 1 and eng.cancel(rid) and eng.pending() == 0


def test_header_build_and_binding():
    from vitron_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_ban_rows\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_ban_rows is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["rows", "n_rows", "V", "stream"]
    assert "const vt_ban_row* rows" in args
    doc = hdr[hdr.index("HISTORY-DEPENDENT BANS"):m.start()]
    for needle in ("bit (i & 31) of word (i >> 5)", "ceil(V / 32)", "NULL", "must NOT alias", "total", "VT_SAMPLE_ROWS_MAX_V", "n_rows == 0",
                   "h[i + g - 1]", "s[L - 1]", "skipped"):
        assert needle in doc, needle
    assert "vt_ban_rows and struct vt_ban_row WITHOUT a bump" in hdr
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    assert len(_lib.SIGNATURES["vt_ban_rows"][1]) == 4
    assert "vt_ban.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "vitron_amd", "csrc", "vt_ban.hip"))
