"""tests/allow_ref.py (the host restatement of the allow masks of vt_sample_rows_allow) pinned: sampling.allow_mask's word / bit layout
against an explicit loop; the -inf edit against transformers' SuppressTokens / BeginSuppressTokens / MinNewTokensLength / NoBadWords /
PrefixConstrained logits processors -- the installed classes themselves wherever the `transformers` package is present, and always their
4.31 rules restated in torch;
the choices trie; SamplingParams' validation and submit's refusals; the engine's host mask function over a scripted token history; the
header. No GPU."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import allow_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -float("inf")

# The installed classes themselves. Only a missing `transformers` package switches the comparison off; a class that is missing from an
# installed package is an error of this file, not a reason to compare less. (5.x renamed BeginSuppressTokensLogitsProcessor to
# SuppressTokensAtBeginLogitsProcessor; both take (begin_suppress_tokens, begin_index).)
HF = importlib.util.find_spec("transformers") is not None
if HF:
    import transformers.generation.logits_process as _LP
    SuppressTokensLogitsProcessor = _LP.SuppressTokensLogitsProcessor
    BeginSuppressTokensLogitsProcessor = getattr(_LP, "BeginSuppressTokensLogitsProcessor", None) or _LP.SuppressTokensAtBeginLogitsProcessor
    MinNewTokensLengthLogitsProcessor = _LP.MinNewTokensLengthLogitsProcessor
    NoBadWordsLogitsProcessor = _LP.NoBadWordsLogitsProcessor
    PrefixConstrainedLogitsProcessor = _LP.PrefixConstrainedLogitsProcessor


def _rows(V=257, n=4, seed=5):
    return torch.randn((n, V), generator=torch.Generator().manual_seed(seed)) * 3.0


def _edit(x, allowed=None, banned=None):
    from vitron_amd.sampling import allow_mask
    return A.masked_logits(x, [allow_mask(x.shape[-1], allowed, banned)] * x.shape[0])


def _hf_equal(got, make, input_ids, x):
    """`got` equals what the installed class returns on a copy of x; nothing is compared only where the package is absent. The
    constructors are called with positional arguments that 4.31 and 5.x share (5.x adds a device keyword that defaults to the CPU); a
    signature that drifts raises here instead of dropping the comparison."""
    if not HF:
        return
    want = make()(input_ids, x.clone())
    assert torch.equal(got, want), type(make()).__name__


# ---- layout ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (1, 31, 32, 33, 257, 32000, 32003))
def test_allow_mask_layout_against_an_explicit_loop(V):
    from vitron_amd.sampling import allow_mask, mask_ids
    g = np.random.default_rng(V)
    some = sorted(set(g.integers(0, V, size=min(V, 40)).tolist()) | {0, V - 1, min(31, V - 1), min(32, V - 1)})
    for allowed, banned in ((None, None), (some, None), (None, some), (some, some[::2]), ([V - 1], None), (None, [0])):
        m = allow_mask(V, allowed, banned)
        assert m.dtype == np.uint32 and m.shape == (A.words(V),)
        assert np.array_equal(m, A.mask_loop(V, allowed, banned)), (V, allowed, banned)
        want = sorted((set(range(V)) if allowed is None else set(allowed)) - set(banned or ()))
        assert mask_ids(m, V).tolist() == want and np.flatnonzero(A.mask_bool(m, V)).tolist() == want
        if V % 32:
            assert int(m[-1]) >> (V % 32) == 0                                      # the bits past V stay clear
    m = allow_mask(70, [0, 31, 32, 69])
    assert [int(w) for w in m] == [0x80000001, 0x1, 0x20]
    for bad in (dict(allowed=[V]), dict(allowed=[-1]), dict(banned=[V]), dict(banned=[-1])):
        with pytest.raises(ValueError):
            allow_mask(V, **bad)
    with pytest.raises(ValueError):
        allow_mask(0)


# ---- the -inf edit is what the processors do --------------------------------------------------------------------------------------------
def test_suppress_tokens_is_the_processor():
    """4.31 SuppressTokensLogitsProcessor: scores[:, self.suppress_tokens] = -float("inf")"""
    x = _rows()
    sup = [0, 5, 31, 32, 256]
    rule = x.clone()
    rule[:, sup] = NEG
    got = _edit(x, banned=sup)
    assert torch.equal(got, rule)
    _hf_equal(got, lambda: SuppressTokensLogitsProcessor(sup), torch.zeros((x.shape[0], 3), dtype=torch.long), x)


def test_begin_suppress_tokens_is_the_processor():
    """4.31 BeginSuppressTokensLogitsProcessor: if input_ids.shape[1] == self.begin_index: scores[:, self.begin_suppress_tokens] = -inf
    -- the first generated token only (generate: step 0)."""
    x = _rows()
    sup, L0 = [7, 64, 255], 6
    for cur in (L0, L0 + 1, L0 + 4):
        rule = x.clone()
        if cur == L0:
            rule[:, sup] = NEG
        got = _edit(x, banned=sup if cur - L0 == 0 else None)
        assert torch.equal(got, rule)
        _hf_equal(got, lambda: BeginSuppressTokensLogitsProcessor(sup, L0), torch.zeros((x.shape[0], cur), dtype=torch.long), x)


def test_min_new_tokens_is_the_processor():
    """4.31 MinNewTokensLengthLogitsProcessor: new_tokens_length = input_ids.shape[-1] - prompt_length_to_skip;
    if new_tokens_length < self.min_new_tokens: for i in self.eos_token_id: scores[:, i] = -float("inf")"""
    from vitron_amd.sampling import SamplingParams, step_allow_mask
    x = _rows()
    V, L0, eos, min_new = x.shape[-1], 6, [2, 200], 3
    sp = SamplingParams(min_new_tokens=min_new)
    for n in range(6):
        rule = x.clone()
        if n < min_new:
            rule[:, eos] = NEG
        key, m = step_allow_mask(sp, n, [9] * n, eos, V)
        assert key == ("pre" if n < min_new else None) and (m is None) == (n >= min_new)
        got = A.masked_logits(x, [m] * x.shape[0])
        assert torch.equal(got, rule)
        _hf_equal(got, lambda: MinNewTokensLengthLogitsProcessor(L0, min_new, eos), torch.zeros((x.shape[0], L0 + n), dtype=torch.long), x)


def test_single_token_bad_words_is_the_processor():
    """4.31 NoBadWordsLogitsProcessor with single-token words: a static mask, scores.masked_fill(static_bad_words_mask, -inf), whatever
    the ids so far."""
    x = _rows()
    bad = [[3], [31], [32], [250]]
    rule = x.clone()
    rule[:, [w[0] for w in bad]] = NEG
    got = _edit(x, banned=[w[0] for w in bad])
    assert torch.equal(got, rule)
    _hf_equal(got, lambda: NoBadWordsLogitsProcessor(bad, 2), torch.randint(0, 257, (x.shape[0], 5)), x)


def test_prefix_constrained_is_the_processor():
    """4.31 PrefixConstrainedLogitsProcessor: mask = full(-inf); mask[row, prefix_allowed_tokens_fn(batch_id, sent)] = 0; scores + mask"""
    x = _rows()
    fn = lambda ids: [int(ids[-1]) % 7, 31, 32, 256]                               # noqa: E731
    input_ids = torch.tensor([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]])
    from vitron_amd.sampling import allow_mask
    masks = [allow_mask(x.shape[-1], fn(row.tolist())) for row in input_ids]
    got = A.masked_logits(x, masks)
    rule = torch.full_like(x, NEG)
    for r, row in enumerate(input_ids):
        rule[r, fn(row.tolist())] = 0
    rule = x + rule
    assert torch.equal(got, rule)
    _hf_equal(got, lambda: PrefixConstrainedLogitsProcessor(lambda b, sent: fn(sent.tolist()), 1), input_ids, x)


def test_the_installed_classes_are_the_five_processors():
    """Where the package is installed, the five names above are classes of its logits_process module (so the comparisons ran)."""
    if not HF:
        return                                                                     # package absent: only the restated 4.31 rules were compared
    for c in (SuppressTokensLogitsProcessor, BeginSuppressTokensLogitsProcessor, MinNewTokensLengthLogitsProcessor,
              NoBadWordsLogitsProcessor, PrefixConstrainedLogitsProcessor):
        assert isinstance(c, type) and c.__module__ == "transformers.generation.logits_process", c


# ---- the choices trie ------------------------------------------------------------------------------------------------------------------
def test_trie_walk():
    from vitron_amd.sampling import SamplingParams, TokenTrie, mask_ids, step_allow_mask
    V, eos = 70, [2]
    choices = [[5, 6], [5], [7, 8, 9], [5, 6, 6]]                                  # [5] is a prefix of [5, 6], which is one of [5, 6, 6]
    t = TokenTrie(choices)
    assert t.children([]) == [5, 7] and not t.ends([])
    assert t.children([5]) == [6] and t.ends([5])
    assert t.children([5, 6]) == [6] and t.ends([5, 6])
    assert t.children([7, 8, 9]) == [] and t.ends([7, 8, 9])                       # a leaf
    assert t.children([7]) == [8] and not t.ends([7])
    assert t.children([9]) == [] and not t.ends([9])                               # off every choice
    sp = SamplingParams(choices=choices)
    cache = {}
    for toks in ([], [5], [5, 6], [5, 6, 6], [7], [7, 8], [7, 8, 9]):
        key, m = step_allow_mask(sp, len(toks), toks, eos, V, cache)
        assert key is None and set(mask_ids(m, V).tolist()) == A.choices_next(choices, toks, eos) == A.step_allowed(V, toks, eos, choices=choices)
    assert set(mask_ids(step_allow_mask(sp, 3, [7, 8, 9], eos, V)[1], V).tolist()) == {2}         # a leaf: only EOS
    one = SamplingParams(choices=[[11, 12]])                                       # a single choice: one path
    assert [set(mask_ids(step_allow_mask(one, len(t_), t_, eos, V)[1], V).tolist()) for t_ in ([], [11], [11, 12])] == [{11}, {12}, {2}]
    with pytest.raises(ValueError):
        step_allow_mask(sp, 1, [9], eos, V)                                        # off every choice: nothing to emit
    with pytest.raises(ValueError):
        step_allow_mask(sp, 0, [], [-1], V)                                        # no EOS id inside [0, V)


# ---- SamplingParams ----------------------------------------------------------------------------------------------------------------------
def test_sampling_params_constraint_fields():
    from vitron_amd.sampling import SamplingParams
    d = SamplingParams()
    assert (d.allowed_token_ids, d.banned_token_ids, d.min_new_tokens, d.choices, d.allowed_tokens_fn) == (None, None, 0, None, None)
    assert not d.constrained and not SamplingParams(temperature=0.7, repetition_penalty=1.2, logprobs=True).constrained
    names = list(SamplingParams.__dataclass_fields__)
    assert names[:6] == ["temperature", "top_p", "top_k", "seed", "repetition_penalty", "logprobs"]      # the new fields come after
    assert names[6:] == ["allowed_token_ids", "banned_token_ids", "min_new_tokens", "choices", "allowed_tokens_fn",
                         "no_repeat_ngram_size", "bad_words"]
    sp = SamplingParams(allowed_token_ids=[3, 4], banned_token_ids=np.array([4]), choices=[[1, 2], (3,)], min_new_tokens=2)
    assert sp.allowed_token_ids == (3, 4) and sp.banned_token_ids == (4,) and sp.choices == ((1, 2), (3,)) and sp.constrained
    assert isinstance(hash(sp), int) and sp == SamplingParams(allowed_token_ids=(3, 4), banned_token_ids=(4,), choices=((1, 2), (3,)),
                                                              min_new_tokens=2)
    with pytest.raises(Exception):
        sp.min_new_tokens = 3                                                      # still frozen
    for bad in (dict(allowed_token_ids=[]), dict(allowed_token_ids=[1.5]), dict(allowed_token_ids=5), dict(banned_token_ids="12"),
                dict(banned_token_ids=[True]), dict(min_new_tokens=-1), dict(min_new_tokens=1.0), dict(choices=[]), dict(choices=[[]]),
                dict(choices=[3]), dict(allowed_tokens_fn=3)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_submit_refuses_impossible_constraints():
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    stub = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=64), device="cpu")
    eng = ServingEngine(stub)
    ids = torch.tensor([[1, 5, 6]])
    for bad in (SamplingParams(allowed_token_ids=[64]), SamplingParams(banned_token_ids=[-1]),             # outside [0, V)
                SamplingParams(allowed_token_ids=[3], banned_token_ids=[3]),                              # nothing left
                SamplingParams(allowed_token_ids=[2], min_new_tokens=1),                                  # only EOS, banned at first
                SamplingParams(choices=[[5, 64]]),                                                        # a choice outside [0, V)
                SamplingParams(choices=[[5]], banned_token_ids=[5]),                                      # the first step is empty
                SamplingParams(banned_token_ids=list(range(64)))):
        with pytest.raises(ValueError):
            eng.submit(ids, sampling=bad)
    with pytest.raises(ValueError):
        eng.submit(ids, sampling=SamplingParams(choices=[[5]]), eos_token_id=-1)                          # choices without an EOS id in [0, V)
    with pytest.raises(ValueError):
        eng.submit(ids, sampling=SamplingParams(choices=[[5]]), eos_token_id=64)
    assert eng.pending() == 0
    called = []
    ok = [SamplingParams(choices=[[5], [5, 6]]), SamplingParams(min_new_tokens=4), SamplingParams(allowed_token_ids=[2, 3], min_new_tokens=1),
          SamplingParams(allowed_tokens_fn=lambda t: called.append(t) or [])]                             # the function is not called at submit
    for sp in ok:
        eng.submit(ids, sampling=sp)
    assert eng.pending() == len(ok) and called == []


# ---- the engine's host mask function ---------------------------------------------------------------------------------------------------
def test_step_mask_over_a_scripted_history():
    """step_allow_mask(sampling, n, tokens, eos, V) against the restated sets, step by step; which steps are static (a key the engine
    keeps the device copy under) and which are step-dependent (key None)."""
    from vitron_amd.sampling import SamplingParams, mask_ids, step_allow_mask
    V, eos = 100, frozenset([2, 99])
    script = [5, 6, 7, 8, 9, 10]
    calls = []

    def fn(toks):
        calls.append(list(toks))
        return None if len(toks) % 2 else [2, 5, 6, 7, 8, 9, 10, 50 + len(toks)]

    cases = [
        (dict(allowed_token_ids=list(range(40))), lambda n: "post"),
        (dict(banned_token_ids=[5, 31, 32]), lambda n: "post"),
        (dict(min_new_tokens=3), lambda n: "pre" if n < 3 else None),
        (dict(allowed_token_ids=[2, 5, 6, 7, 99], banned_token_ids=[7], min_new_tokens=2), lambda n: "pre" if n < 2 else "post"),
        (dict(choices=[script[:2], script[:4], [5, 7]], min_new_tokens=1), lambda n: None),
        (dict(allowed_tokens_fn=fn, banned_token_ids=[10]), lambda n: "post" if n % 2 else None),
    ]
    for kw, want_key in cases:
        sp = SamplingParams(**kw)
        cache = {}
        for n in range(len(script) + 1):
            toks = script[:n]
            want = A.step_allowed(V, toks, eos, allowed=kw.get("allowed_token_ids"), banned=kw.get("banned_token_ids", ()),
                                  min_new_tokens=kw.get("min_new_tokens", 0), choices=kw.get("choices"), fn=kw.get("allowed_tokens_fn"))
            if want is not None and not want:
                with pytest.raises(ValueError):
                    step_allow_mask(sp, n, toks, eos, V, cache)
                continue
            key, m = step_allow_mask(sp, n, toks, eos, V, cache)
            assert key == (want_key(n) if want is not None else None), (kw, n, key)
            assert (m is None) == (want is None) and (m is None or set(mask_ids(m, V).tolist()) == want), (kw, n)
            if key is not None and "allowed_tokens_fn" not in kw:
                assert step_allow_mask(sp, n, toks, eos, V, cache)[1] is m       # a static mask is built once per request
    assert calls == [script[:n] for n in range(len(script) + 1) for _ in range(2)]      # (twice per step: the restatement and the function under test)
    assert step_allow_mask(None, 0, [], eos, V) == (None, None) and step_allow_mask(SamplingParams(), 3, [1, 2, 3], eos, V) == (None, None)


# ---- the header -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbol_and_documents_the_layout():
    from vitron_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_sample_rows_allow\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_sample_rows_allow is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["logits", "rows", "V", "ldl", "params", "allow", "out_ids", "kept_count",
                                                                    "logprob", "stream"]
    assert "const uint32_t* const* allow" in args
    doc = hdr[hdr.index("vt_sample_rows with a PER-ROW ALLOW MASK"):m.start()]
    for needle in ("bit (i & 31) of word (i >> 5)", "ceil(V / 32)", "NULL", ">= V", "RAW row", "-inf", "readable"):
        assert needle in doc, needle
    assert len(_lib.SIGNATURES["vt_sample_rows_allow"][1]) == 10 and len(_lib.SIGNATURES["vt_sample_rows"][1]) == 9
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
