"""The host side of vt_sample_rows_trunc, no GPU: tests/trunc_ref.py's fp64 restatement of the four truncation stages
equals transformers' MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper -- each alone and all chained in
GenerationMixin._get_logits_processor's order -- on rows whose parameters place() has moved to the middle of a gap; the constructed row
where typical sampling removes the arg-max and a later epsilon stage protects the NEW maximum; the ABI of struct vt_trunc_row; the
argument validation of SamplingParams and generate(); the library's argument refusals, which come back without a GPU."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import trunc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 1000


@pytest.fixture(scope="module")
def cases():
    """64 placed cases at V = 1000 (four draws of the 16 stage combinations), built once and never modified"""
    out = []
    for seed in range(4):
        out += R.placed_cases(V, seed=seed)
    return out


def _hf_keep(c, only=None):
    """The ids transformers' fp32 warper chain leaves finite for case c. only: the index of ONE truncation stage to run alone, on the
    scores with -inf outside the survivors of the stages in front of it (which is what that warper sees inside the chain)."""
    from transformers.generation import logits_process as LP
    mp, ty, ep, et = c["trunc"]
    act = R.on(c["trunc"])
    make = (lambda: LP.MinPLogitsWarper(min_p=mp), lambda: LP.TypicalLogitsWarper(mass=ty), lambda: LP.EpsilonLogitsWarper(epsilon=ep),
            lambda: LP.EtaLogitsWarper(epsilon=et, device="cpu"))
    ids = torch.zeros((1, 1), dtype=torch.long)
    if only is not None:
        before = tuple(v if i < only else R.OFF[i] for i, v in enumerate(c["trunc"]))
        A = R.apply(c["s"], c["A0"], before)
        x = torch.from_numpy(np.where(A, c["s"], -np.inf).astype(np.float32))[None]
        return make[only]()(ids, x)[0].isfinite().numpy(), A
    x = torch.from_numpy(np.where(c["allow"], c["row"], -np.inf) if c["allow"] is not None else c["row"].copy())[None]
    chain = [LP.TemperatureLogitsWarper(c["T"])]
    if c["top_k"] > 0:
        chain.append(LP.TopKLogitsWarper(top_k=c["top_k"]))
    if c["top_p"] < 1.0:
        chain.append(LP.TopPLogitsWarper(top_p=c["top_p"]))
    chain += [make[i]() for i in range(4) if act[i]]
    for w in chain:
        x = w(ids, x)
    return x[0].isfinite().numpy(), None


def test_the_chain_order_is_transformers_own():
    """Temperature, TopK, TopP, MinP, Typical, Epsilon, Eta: what GenerationMixin builds from a GenerationConfig with all of them on"""
    from transformers import GenerationConfig
    from transformers.generation.logits_process import LogitsProcessorList
    from transformers.generation.utils import GenerationMixin

    class Bare(GenerationMixin):
        pass
    m = Bare.__new__(Bare)
    m.config = types.SimpleNamespace(is_encoder_decoder=False)
    gc = GenerationConfig(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, min_p=0.1, typical_p=0.8, epsilon_cutoff=1e-3,
                          eta_cutoff=1e-3)
    got = m._get_logits_processor(gc, input_ids_seq_length=1, encoder_input_ids=None, prefix_allowed_tokens_fn=None,
                                  logits_processor=LogitsProcessorList(), device="cpu")
    assert [type(p).__name__ for p in got] == ["TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper", "MinPLogitsWarper",
                                               "TypicalLogitsWarper", "EpsilonLogitsWarper", "EtaLogitsWarper"]


def test_placed_cases_are_complete_and_consistent(cases):
    assert len(cases) == 64 and [c["combo"] for c in cases[:16]] == list(R.COMBOS)
    for c in cases:
        act = R.on(c["trunc"])
        assert tuple(i for i in range(4) if act[i]) == tuple(sorted(set(c["combo"])))
        assert all(float(np.float32(v)) == v for v in c["trunc"])                  # what the kernel receives is what was placed
        assert np.array_equal(R.apply(c["s"], c["A0"], c["trunc"]), c["A"]) and c["A"].any() and not (c["A"] & ~c["A0"]).any()
    assert sum(int(c["A"].sum()) < int(c["A0"].sum()) for c in cases) >= 48        # the stages do remove something


def test_the_restatement_equals_transformers_chain(cases):
    for n, c in enumerate(cases):
        got, _ = _hf_keep(c)
        assert np.array_equal(got, c["A"]), (n, c["combo"], c["trunc"], int(got.sum()), int(c["A"].sum()))


def test_each_stage_alone_equals_its_warper(cases):
    ran = [0, 0, 0, 0]
    for n, c in enumerate(cases):
        for i in range(4):
            if R.on(c["trunc"])[i]:
                got, before = _hf_keep(c, only=i)
                alone = tuple(v if j == i else R.OFF[j] for j, v in enumerate(c["trunc"]))
                assert np.array_equal(got, R.apply(c["s"], before, alone)), (n, i, c["trunc"])
                ran[i] += 1
    assert min(ran) >= 16


def test_protecting_the_original_arg_max_would_be_wrong(cases):
    """The "top token" of epsilon and eta is the maximum of the survivors so far. Among the placed cases some have typical sampling remove
    the row's arg-max; and the constructed row pins the consequence."""
    assert sum(1 for c in cases if R.on(c["trunc"])[1] and not c["A"][int(np.argmax(c["s"]))]) >= 1
    s, A0, trunc = R.argmax_removed_case(V)
    top = int(np.argmax(s))
    after_typical = R.apply(s, A0, (0.0, trunc[1], 0.0, 0.0))
    assert not after_typical[top] and after_typical.sum() > 10                     # typical removed the arg-max ...
    A = R.apply(s, A0, trunc)
    new_top = int(np.argmax(np.where(after_typical, s, -np.inf)))
    assert A.sum() == 1 and A[new_top] and new_top != top                          # ... and epsilon keeps the new maximum alone
    got, _ = _hf_keep(dict(row=s.astype(np.float32), allow=None, T=1.0, top_k=0, top_p=1.0, trunc=trunc))
    assert np.array_equal(got, A)


def test_trunc_row_dtype_matches_the_header():
    from vitron_amd import _lib
    from vitron_amd.sampling import TRUNC_OFF, TRUNC_ROW_BYTES, TRUNC_ROW_DTYPE, pack_trunc_rows, trunc_rows_array
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_sample_rows_trunc\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_sample_rows_trunc is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["logits", "rows", "V", "ldl", "params", "allow", "adjust", "trunc",
                                                                      "out_ids", "kept_count", "logprob", "stream"]
    assert "const vt_trunc_row* trunc" in args
    span = hdr[hdr.index("PER-ROW TRUNCATION"):hdr.index("typedef struct vt_trunc_row")]
    table = {mm.group(2): int(mm.group(1)) for mm in re.finditer(r"^ \*\s+@(\d+)\s+float\s+(\w+)", span, flags=re.M)}
    assert table == {n: TRUNC_ROW_DTYPE.fields[n][1] for n in TRUNC_ROW_DTYPE.names} == dict(min_p=0, typical_p=4, epsilon_cutoff=8, eta_cutoff=12)
    struct = hdr[hdr.index("typedef struct vt_trunc_row"):hdr.index("} vt_trunc_row;")]
    assert re.findall(r"float (\w+);", struct) == list(TRUNC_ROW_DTYPE.names) and TRUNC_ROW_BYTES == 16
    assert "vt_sample_rows_trunc and struct vt_trunc_row WITHOUT a bump" in hdr
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    assert len(_lib.SIGNATURES["vt_sample_rows_trunc"][1]) == 12
    a = trunc_rows_array([(0.1, 0.9, 1e-3, 2e-3), None])
    assert a.tobytes() == np.asarray([0.1, 0.9, 1e-3, 2e-3, *TRUNC_OFF], dtype="<f4").tobytes()
    assert pack_trunc_rows([None, None, None], "cpu").shape == (3, 16)
    for bad in ((0.1, 0.9, 1e-3), (1.5, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, 1.0, 0.0, float("nan"))):
        with pytest.raises(ValueError):
            trunc_rows_array([bad])


def test_sampling_params_fields_and_validation():
    from vitron_amd.sampling import SamplingParams
    d = SamplingParams()
    assert (d.min_p, d.typical_p, d.epsilon_cutoff, d.eta_cutoff) == (0.0, 1.0, 0.0, 0.0) and not d.truncated
    # the four come behind the dataclass fields (whose pinned list did not grow) in the constructor, repr, ==, hash and replace()
    assert not set(R.STAGES) & set(SamplingParams.__dataclass_fields__)
    assert repr(d).endswith("bad_words=None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)")
    a, b = SamplingParams(temperature=0.8, min_p=0.1, seed=3), SamplingParams(temperature=0.8, min_p=0.2, seed=3)
    assert a != b and a == SamplingParams(temperature=0.8, seed=3, min_p=0.1) and hash(a) == hash(b.replace(min_p=0.1)) and a != d
    assert a.replace(seed=4).min_p == 0.1 and a.replace(min_p=0.0) == SamplingParams(temperature=0.8, seed=3)
    for name in R.STAGES + ("seed",):
        with pytest.raises(Exception):
            setattr(a, name, 0.5)                                                  # frozen, the four included
    for kw in (dict(min_p=0.1), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3), dict(min_p=1.0)):
        sp = SamplingParams(temperature=0.8, **kw)
        assert sp.truncated and not sp.constrained and sp.replace(seed=3).truncated
        assert not SamplingParams(**kw).truncated                                  # a greedy request ignores them
    assert SamplingParams(temperature=1.0, min_p=0.25, eta_cutoff=0.5).trunc_row == (0.25, 1.0, 0.0, 0.5)
    assert not SamplingParams(temperature=1.0, min_p=0.0, typical_p=1.0).truncated
    nan, inf = float("nan"), float("inf")
    for bad in (dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=nan), dict(min_p=inf), dict(min_p=None), dict(min_p=True),
                dict(typical_p=0.0), dict(typical_p=-0.5), dict(typical_p=1.5), dict(typical_p=nan), dict(typical_p="0.9"),
                dict(epsilon_cutoff=-1e-3), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=nan), dict(epsilon_cutoff=inf),
                dict(eta_cutoff=-1e-3), dict(eta_cutoff=1.0), dict(eta_cutoff=2.0), dict(eta_cutoff=nan)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            SamplingParams(temperature=1.0, **bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            SamplingParams(**bad)                                                  # validated whether or not the request samples


def _resolve(**kw):
    from vitron_amd.picker import resolve_generate_args
    cfg = types.SimpleNamespace(eos_token_id=2, pad_token_id=0, vocab_size=64, top_k=50)
    args = dict(do_sample=False, temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=4, max_length=None, stopping_criteria=None,
                eos_token_id=None, pad_token_id=None, num_beams=1, seed=None, return_logits=False, padded_batch=False, repetition_penalty=1.0,
                return_logprobs=False, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None,
                allowed_token_ids=None, num_return_sequences=1, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None)
    args.update(kw)
    return resolve_generate_args(cfg, 5, **args)


def test_generate_arguments_resolve_and_refuse():
    from vitron_amd.model import LlavaLlamaForCausalLM
    p = inspect.signature(LlavaLlamaForCausalLM.generate).parameters
    assert all(p[n].default is None for n in R.STAGES)                             # parameters of generate(), not swallowed by **kwargs
    plain = _resolve(do_sample=True, seed=1)
    assert plain.trunc == (0.0, 1.0, 0.0, 0.0) and not plain.truncated and not plain.per_row and plain.given == ()
    for kw, want in ((dict(min_p=0.1), (0.1, 1.0, 0.0, 0.0)), (dict(typical_p=0.9), (0.0, 0.9, 0.0, 0.0)),
                     (dict(epsilon_cutoff=1e-3), (0.0, 1.0, 1e-3, 0.0)), (dict(eta_cutoff=2e-3), (0.0, 1.0, 0.0, 2e-3))):
        a = _resolve(do_sample=True, seed=1, **kw)
        assert a.trunc == want and a.truncated and a.per_row
        g = _resolve(do_sample=False, **kw)                                        # ignored without do_sample
        assert g.trunc == (0.0, 1.0, 0.0, 0.0) and not g.truncated and not g.per_row
        name = next(iter(kw))
        with pytest.raises(NotImplementedError, match=name):
            _resolve(num_beams=2, **kw)                                            # through the `given` list
        with pytest.raises(NotImplementedError, match="min_p / typical_p / epsilon_cutoff / eta_cutoff"):
            _resolve(do_sample=True, seed=1, padded_batch=True, **kw)
    off = _resolve(do_sample=True, seed=1, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    assert not off.truncated and not off.per_row and off.given == ()
    _resolve(num_beams=2, min_p=0.0, typical_p=1.0)                                # the off values are not "given"
    with pytest.raises(NotImplementedError, match="suppress_tokens"):              # an earlier name is still refused first
        _resolve(num_beams=2, suppress_tokens=[4], min_p=0.1)
    nan = float("nan")
    for bad in (dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=nan), dict(typical_p=0.0), dict(typical_p=1.5), dict(typical_p=nan),
                dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-1.0), dict(eta_cutoff=1.0), dict(eta_cutoff=nan), dict(eta_cutoff=float("inf"))):
        for sample in (True, False):
            with pytest.raises(ValueError, match=next(iter(bad))):
                _resolve(do_sample=sample, seed=1, **bad)


def test_both_libraries_export_the_entry_point_and_refuse_bad_arguments():
    """Through the libraries themselves (they validate first, so this runs without a GPU): argument errors come back as status -1."""
    from vitron_amd import _lib
    for operand in ("bf16", "fp16"):
        lib = _lib.load(operand=operand)
        assert lib.vt_version() == 114 and hasattr(lib, "vt_sample_rows_trunc")
        P = 0x10000                  # an aligned non-null address; never dereferenced because validation fails first
        for args, needle in (((None, 1, 64, 64, P, None, None, P, P, None, None, None), "null pointer"),          # logits
                             ((P, 1, 64, 64, None, None, None, P, P, None, None, None), "null pointer"),          # params
                             ((P, 1, 64, 64, P, None, None, P, None, None, None, None), "null pointer"),          # out_ids
                             ((P, 1, 64, 64, P, None, None, P + 2, P, None, None, None), "trunc must be 4-byte aligned"),
                             ((P, 1, 64, 64, P, None, P + 4, P, P, None, None, None), "adjust pointer array"),
                             ((P, 1, 64, 64, P, P + 4, None, P, P, None, None, None), "allow pointer array"),
                             ((P, 0, 64, 64, P, None, None, P, P, None, None, None), "rows=0"),
                             ((P, 1, 64, 32, P, None, None, P, P, None, None, None), "ldl=32"),
                             ((P, 1, 262145, 262148, P, None, None, P, P, None, None, None), "V=262145")):
            assert lib.vt_sample_rows_trunc(*args) == -1                           # VT_STATUS_ARG
            assert needle in _lib.last_error(lib), (operand, needle, _lib.last_error(lib))
