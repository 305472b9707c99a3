"""tests/bias_ref.py (the host restatement of vt_bias_rows' contract and of the adjusted value) and sampling.logit_adjust
(the product's own) pinned against each other and, for the bias, against transformers' SequenceBiasLogitsProcessor -- the installed class
wherever the `transformers` package is present; struct vt_bias_row's packing and the header's table; the header's other parsers; the ABI
version; the new symbols' declarations, bindings and refusals (through the library, which validates before it launches); LogitAdjust's and
generate()'s argument validation. No GPU."""
import dataclasses
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import bias_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HF = importlib.util.find_spec("transformers") is not None
F32 = np.float32


def _random_case(rng, V, n):
    alphabet = np.concatenate([rng.choice(V, size=int(rng.integers(1, 5)), replace=False), [-3, V, V + 9, 0, V - 1]])
    h = rng.choice(alphabet, size=n).tolist()
    ids = np.unique(np.concatenate([rng.choice(V, size=int(rng.integers(0, 9)), replace=False), rng.choice(alphabet, size=2)])).tolist()
    vals = (rng.standard_normal(len(ids)) * 5).astype(F32).tolist()
    pres, freq = (float(F32(v)) for v in rng.standard_normal(2) * 1.7)
    return h, ids, vals, pres, freq


def test_both_restatements_agree():
    """bias_ref.bias_rows == sampling.logit_adjust bit for bit: V from 31 to 1000, histories of 0 to 700 ids over small alphabets (counts
    in the hundreds), ids outside the vocabulary in the history and in the bias."""
    from vitron_amd.sampling import logit_adjust
    rng = np.random.default_rng(981)
    big = 0
    for V in (31, 32, 33, 64, 257, 1000):
        for n in (0, 1, 2, 5, 64, 255, 256, 257, 700):
            h, ids, vals, pres, freq = _random_case(rng, V, n)
            pre, post = R.bias_rows(V, h, ids, vals, pres, freq)
            gpre, gpost = logit_adjust(V, h, dict(zip(ids, vals)), pres, freq)
            assert pre.dtype == post.dtype == gpre.dtype == gpost.dtype == F32
            assert np.array_equal(pre.view(np.uint32), gpre.view(np.uint32)), (V, n)
            assert np.array_equal(post.view(np.uint32), gpost.view(np.uint32)), (V, n)
            inside = [t for t in h if 0 <= t < V]
            assert set(np.flatnonzero(post).tolist()) <= set(inside)
            big = max(big, max((inside.count(t) for t in set(inside)), default=0))
    assert big >= 100                                                             # the counts did get large


def test_the_two_roundings_are_separate():
    """frequency * count + presence where a fused multiply-add gives another fp32 than the product rounded first: the reference is the
    two-step value (and so must the kernel be)."""
    f, c, p = F32(1.0 + 2.0 ** -12), 4097, F32(-4097.0)
    two_step = F32(F32(f * F32(c)) + p)
    fused = F32(np.float64(f) * np.float64(c) + np.float64(p))                    # exact in fp64: what one rounding at the end gives
    assert two_step != fused
    pre, post = R.bias_rows(8, [3] * c, [], [], p, f)
    assert post[3] == -two_step and not pre.any() and np.count_nonzero(post) == 1


def test_only_the_last_65535_ids_count():
    from vitron_amd.sampling import logit_adjust
    h = [1] * 10 + [2] * 65535
    _, post = R.bias_rows(4, h, [], [], 0.0, 1.0)
    assert post.tolist() == [0.0, 0.0, -65535.0, 0.0]
    assert np.array_equal(post, logit_adjust(4, h, None, 0.0, 1.0)[1])
    _, post = R.bias_rows(4, h[1:] + [1], [], [], 0.5, 1.0)
    assert post.tolist() == [0.0, -1.5, -65534.5, 0.0]


@pytest.mark.skipif(not HF, reason="transformers is not installed")
def test_pre_is_the_installed_sequence_bias_processor():
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    rng = np.random.default_rng(982)
    for V in (31, 64, 1000):
        ids = rng.choice(V, size=7, replace=False).tolist() + [0, V - 1]
        ids = sorted(set(ids))
        vals = (rng.standard_normal(len(ids)) * 8).astype(F32).tolist()
        raw = (rng.standard_normal((1, V)) * 3).astype(F32)
        proc = SequenceBiasLogitsProcessor({(int(t),): float(v) for t, v in zip(ids, vals)})
        want = proc(torch.tensor([[1, 2, 3]], dtype=torch.long), torch.from_numpy(raw.copy())).numpy()
        pre, post = R.bias_rows(V, [], ids, vals, 0.0, 0.0)
        got = R.adjusted(raw[0], None, pre, post)
        assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32)), V
        assert not np.array_equal(got, raw[0])


def test_adjusted_applies_the_steps_in_order():
    raw = np.array([1.0, 3.0, 4.0, 1.0, -2.0], dtype=F32)
    pre = np.array([3.0, 0, 0, 0, 1.0], dtype=F32)
    post = np.array([0, 0, -1.5, 0, 0], dtype=F32)
    x = R.adjusted(raw, np.array([1, 1, 1, 0, 1], bool), pre, post, 2.0, [0, 2, 4])
    assert x.tolist() == [2.0, 3.0, 0.5, -np.inf, -2.0]                            # (1 + 3) / 2; 4 / 2 - 1.5; (-2 + 1) * 2
    assert R.adjusted(raw, None, pre, post, 1.0, [0, 2]).tolist() == [4.0, 3.0, 2.5, 1.0, -1.0]
    assert R.adjusted(np.array([-np.inf], F32), None, np.array([1e30], F32), np.array([0], F32)).tolist() == [-np.inf]


def test_bias_row_struct_and_the_header_table():
    from vitron_amd.sampling import BIAS_ROW_BYTES, BIAS_ROW_DTYPE, BIAS_ROWS_MAX_V, bias_rows_array
    assert BIAS_ROW_BYTES == 48 == BIAS_ROW_DTYPE.itemsize
    arr = bias_rows_array([(0x1122334455667788, 7, 0x0102030405060708, 0x1112131415161718, 3, 0x2122232425262728, 0.5, -1.25),
                           (0, 0, 0, 0, 0, 0x40, 0.0, 2.0)])
    raw = arr.view(np.uint8).reshape(2, 48)
    u64 = lambda r, o: int(raw[r, o:o + 8].view("<u8")[0])                        # noqa: E731
    i32 = lambda r, o: int(raw[r, o:o + 4].view("<i4")[0])                        # noqa: E731
    f32 = lambda r, o: float(raw[r, o:o + 4].view("<f4")[0])                      # noqa: E731
    assert (u64(0, 0), u64(0, 8), u64(0, 16), u64(0, 24)) == (0x1122334455667788, 0x0102030405060708, 0x1112131415161718, 0x2122232425262728)
    assert (i32(0, 32), i32(0, 36), f32(0, 40), f32(0, 44)) == (7, 3, 0.5, -1.25)
    assert (u64(1, 24), f32(1, 44)) == (0x40, 2.0)
    for bad in ((0, 5, 0, 0, 0, 0x40, 0.0, 0.0), (0, 0, 0x40, 0, 2, 0x40, 0.0, 0.0), (0, 0, 0, 0x40, 2, 0x40, 0.0, 0.0)):
        with pytest.raises(ValueError):
            bias_rows_array([bad])                                                # a length without its buffer
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    doc = hdr[hdr.index("ADDITIVE ADJUSTMENTS"):hdr.index("typedef struct vt_bias_row")]
    table = {m.group(2): int(m.group(1)) for m in re.finditer(r"^ \*\s+@(\d+)\s+(?:const )?(?:int32_t|float)\*?\s+(\w+)", doc, flags=re.M)}
    assert table == {n: BIAS_ROW_DTYPE.fields[n][1] for n in BIAS_ROW_DTYPE.names}, table
    body = re.search(r"typedef struct vt_bias_row \{(.*?)\} vt_bias_row;", hdr, flags=re.S).group(1)
    assert [ln.split()[-1].rstrip(";") for ln in body.strip().splitlines()] == list(BIAS_ROW_DTYPE.names)
    assert re.search(r"#define VT_BIAS_ROWS_MAX_V 65536\b", hdr) and BIAS_ROWS_MAX_V == 65536


def test_the_header_keeps_its_other_parsers():
    """tests/test_sample_ref_host.py runs one regex over the whole header and wants exactly vt_sample_row's fields;
    tests/test_ban_ref_host.py parses the span in front of struct vt_ban_row. The new section is outside both."""
    from vitron_amd.sampling import BAN_ROW_DTYPE, ROW_DTYPE
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    rows = re.findall(r"^ \*\s+(\d+) (float|int32|uint64|uint32|const int\*)\s+(\w+)", hdr, flags=re.M)
    assert {name: int(off) for off, _, name in rows} == {n: ROW_DTYPE.fields[n][1] for n in ROW_DTYPE.names} and len(rows) == len(ROW_DTYPE.names)
    span = hdr[hdr.index("HISTORY-DEPENDENT BANS"):hdr.index("typedef struct vt_ban_row")]
    assert "vt_bias" not in span and "ADDITIVE" not in span
    table = {m.group(2): int(m.group(1)) for m in re.finditer(r"^ \*\s+(\d+) (?:const )?u?int32_t\*?\s+(\w+)", span, flags=re.M)}
    assert table == {n: BAN_ROW_DTYPE.fields[n][1] for n in BAN_ROW_DTYPE.names}
    from tests import test_sample_ref_host as T
    ran = 0
    for name in dir(T):
        fn = getattr(T, name)
        if name.startswith("test_") and callable(fn) and "header" in name:
            fn()
            ran += 1
    assert ran >= 1


def test_header_build_and_binding():
    from vitron_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_bias_rows\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_bias_rows is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["rows", "n_rows", "V", "stream"] and "const vt_bias_row* rows" in args
    m2 = re.search(r"^int\s+vt_sample_rows_adj\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m2, "vt_sample_rows_adj is not declared"
    args2 = re.sub(r"/\*.*?\*/", "", m2.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args2.split(",")] == ["logits", "rows", "V", "ldl", "params", "allow", "adjust", "out_ids",
                                                                       "kept_count", "logprob", "stream"]
    assert "const float* const* adjust" in args2
    doc = hdr[hdr.index("ADDITIVE ADJUSTMENTS"):m2.start()]
    for needle in ("x + pre[t]", "x + post[t]", "rounded separately", "GENERATED", "LAST 65535", "must NOT alias", "total", "VT_BIAS_ROWS_MAX_V",
                   "n_rows == 0", "skipped", "RAW row"):
        assert needle in doc, needle
    assert "vt_bias_rows, struct vt_bias_row and vt_sample_rows_adj WITHOUT a bump" in hdr
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    assert len(_lib.SIGNATURES["vt_bias_rows"][1]) == 4 and len(_lib.SIGNATURES["vt_sample_rows_adj"][1]) == 11
    assert "vt_bias.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "vitron_amd", "csrc", "vt_bias.hip"))
    kh = open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_kernels.h")).read()
    api = open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_api.hip")).read()
    assert "vt_bias_rows_launch" in kh and "vt_bias_rows_launch" in api and "vt_sample_rows_adj" in api


def test_refusals_come_before_any_launch():
    """Through the library itself (it validates first, so this runs without a GPU): the ABI version and vt_bias_rows' /
    vt_sample_rows_adj's argument refusals, each with its message."""
    from vitron_amd import _lib
    lib = _lib.load()
    assert lib.vt_version() == 114
    P = 0x10000                      # an aligned non-null address; never dereferenced because validation fails first
    for n_rows, V, ptr, needle in ((1, 0, P, "V=0"), (1, -5, P, "V=-5"), (1, 65537, P, "V=65537"), (1, 262144, P, "V=262144"),
                                   (-1, 64, P, "n_rows=-1"), (1, 64, None, "NULL"), (1, 64, P + 4, "8-byte")):
        assert lib.vt_bias_rows(ptr, n_rows, V, None) == -1                       # VT_STATUS_ARG
        assert "vt_bias_rows" in _lib.last_error(lib) and needle in _lib.last_error(lib), (needle, _lib.last_error(lib))
    assert lib.vt_bias_rows(None, 0, 64, None) == 0 and lib.vt_bias_rows(P, 0, 65536, None) == 0          # no rows: launches nothing
    for args, needle in (((None, 1, 64, 64, P, None, P, P, None, None, None), "null pointer"),
                         ((P, 0, 64, 64, P, None, P, P, None, None, None), "rows=0"),
                         ((P, 1, 64, 32, P, None, P, P, None, None, None), "ldl=32"),
                         ((P, 1, 64, 64, P, None, P + 4, P, None, None, None), "adjust pointer array"),
                         ((P, 1, 64, 64, P, P + 4, P, P, None, None, None), "allow pointer array"),
                         ((P, 1, 262145, 262148, P, None, P, P, None, None, None), "V=262145")):
        assert lib.vt_sample_rows_adj(*args) == -1
        assert needle in _lib.last_error(lib), (needle, _lib.last_error(lib))


def test_logit_adjust_dataclass():
    from vitron_amd.sampling import LogitAdjust, SamplingParams
    d = LogitAdjust()
    assert [f.name for f in dataclasses.fields(d)] == ["logit_bias", "presence_penalty", "frequency_penalty"]
    assert d.bias == () and not d.active and not d.penalties
    a = LogitAdjust({7: 1.5, 3: -2}, frequency_penalty=0.5)
    assert a.bias == ((3, -2.0), (7, 1.5)) and a.active and a.penalties
    assert LogitAdjust({np.int64(3): np.float32(0.5)}).bias == ((3, 0.5),) and not LogitAdjust({3: 1.0}).penalties
    assert a == LogitAdjust({7: 1.5, 3: -2}, frequency_penalty=0.5) and hash(a) == hash(LogitAdjust({3: -2, 7: 1.5}, 0.0, 0.5))
    assert LogitAdjust(presence_penalty=-3.5).penalties                            # any finite float; [-2, 2] is not enforced
    with pytest.raises(Exception):
        a.presence_penalty = 1.0                                                   # frozen
    for bad in (dict(logit_bias={-1: 1.0}), dict(logit_bias={3: float("nan")}), dict(logit_bias={3: float("inf")}), dict(logit_bias={3: "1"}),
                dict(logit_bias={(3,): 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={True: 1.0}), dict(logit_bias=[(3, 1.0)]),
                dict(presence_penalty=float("nan")), dict(frequency_penalty=float("inf")), dict(presence_penalty=None),
                dict(frequency_penalty=True)):
        with pytest.raises(ValueError):
            LogitAdjust(**bad)
    a.check_vocab(8)
    with pytest.raises(ValueError, match="7"):
        a.check_vocab(7)
    # SamplingParams did not grow: the adjustment travels beside it
    assert not {"logit_bias", "presence_penalty", "frequency_penalty", "adjust"} & {f.name for f in dataclasses.fields(SamplingParams)}


def test_submit_takes_and_refuses_adjust():
    from vitron_amd.sampling import LogitAdjust, SamplingParams
    from vitron_amd.serving import ServingEngine
    stub = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=64), device="cpu")
    eng = ServingEngine(stub)
    ids = torch.tensor([[1, 5, 6]])
    with pytest.raises(ValueError, match="64"):
        eng.submit(ids, adjust=LogitAdjust({64: 1.0}))
    with pytest.raises(TypeError):
        eng.submit(ids, adjust={3: 1.0})
    assert eng.pending() == 0
    rid = eng.submit(ids, adjust=LogitAdjust({63: 1.0}, 0.5, 0.5))
    off = eng.submit(ids, sampling=SamplingParams(), adjust=LogitAdjust())
    held = {r.rid: r for r in eng.waiting}
    assert held[rid].adjust is not None and held[rid].sampling is None and held[off].adjust is None
    assert eng.cancel(rid) and eng.cancel(off) and eng.pending() == 0 and held[rid].adj_buf is None and held[rid].gen is None
    big = ServingEngine(types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=70000), device="cpu"))
    with pytest.raises(ValueError, match="65536"):
        big.submit(ids, adjust=LogitAdjust({3: 1.0}))
    big.submit(ids, adjust=LogitAdjust())                                          # nothing to adjust: nothing to refuse


def _resolve(**kw):
    from vitron_amd.picker import resolve_generate_args
    cfg = types.SimpleNamespace(eos_token_id=2, pad_token_id=0, vocab_size=kw.pop("vocab_size", 64), top_k=50)
    args = dict(do_sample=False, temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=4, max_length=None, stopping_criteria=None,
                eos_token_id=None, pad_token_id=None, num_beams=1, seed=None, return_logits=False, padded_batch=False, repetition_penalty=1.0,
                return_logprobs=False, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None,
                allowed_token_ids=None, num_return_sequences=1, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None)
    args.update(kw)
    return resolve_generate_args(cfg, 5, **args)


def test_generate_arguments_resolve_and_refuse():
    plain = _resolve()
    assert plain.bias == () and plain.presence_penalty == 0.0 and plain.frequency_penalty == 0.0 and not plain.adjusted and not plain.per_row
    assert plain.given == ()
    a = _resolve(sequence_bias={(7,): 2.0, 3: -1, (np.int64(9),): np.float32(0.5)})
    assert a.bias == ((3, -1.0), (7, 2.0), (9, 0.5)) and a.adjusted and a.per_row and not a.count_penalties
    for kw in (dict(presence_penalty=0.5), dict(frequency_penalty=-0.25), dict(presence_penalty=-7.0, frequency_penalty=3.0)):
        b = _resolve(**kw)
        assert b.adjusted and b.per_row and b.count_penalties and b.bias == ()
    assert not _resolve(sequence_bias={}, presence_penalty=0.0).per_row
    with pytest.raises(NotImplementedError, match=r"\(5, 6\)"):
        _resolve(sequence_bias={(5, 6): 1.0})
    for bad in ({(64,): 1.0}, {-1: 1.0}, {3: float("nan")}, {(3,): float("-inf")}, {3: 1.0, (3,): 2.0}, {(): 1.0}, {"3": 1.0}, [(3, 1.0)]):
        with pytest.raises(ValueError, match="sequence_bias"):
            _resolve(sequence_bias=bad)
    with pytest.raises(ValueError, match="presence_penalty"):
        _resolve(presence_penalty=float("nan"))
    with pytest.raises(ValueError, match="frequency_penalty"):
        _resolve(frequency_penalty=float("inf"))
    for kw, name in ((dict(sequence_bias={3: 1.0}), "sequence_bias"), (dict(presence_penalty=0.5), "presence_penalty"),
                     (dict(frequency_penalty=0.5), "frequency_penalty")):
        with pytest.raises(NotImplementedError, match=name):
            _resolve(num_beams=2, **kw)
        with pytest.raises(NotImplementedError, match=name):
            _resolve(padded_batch=True, **kw)
    # the order of the earlier refusals did not move: an earlier name is still refused first
    with pytest.raises(NotImplementedError, match="suppress_tokens"):
        _resolve(num_beams=2, suppress_tokens=[4], sequence_bias={3: 1.0})
    with pytest.raises(NotImplementedError, match="return_logits"):
        _resolve(num_beams=2, return_logits=True, frequency_penalty=1.0)
    with pytest.raises(NotImplementedError, match="65536"):
        _resolve(vocab_size=70000, presence_penalty=0.5)
    assert not _resolve(vocab_size=70000).per_row


def test_generate_names_its_arguments():
    """They are parameters of generate() now, not swallowed by **kwargs."""
    import inspect

    from vitron_amd.model import LlavaLlamaForCausalLM
    p = inspect.signature(LlavaLlamaForCausalLM.generate).parameters
    assert p["sequence_bias"].default is None and p["presence_penalty"].default == 0.0 and p["frequency_penalty"].default == 0.0
