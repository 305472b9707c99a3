"""DoLa on the host: tests/dola_ref.py against a literal fp64 torch port of transformers 4.4x' _dola_select_contrast
and _relative_top_filter, the low / high layer ranges, the tie rule, the keep rule at its threshold, a NaN row, the bound and the ladder
builder, struct vt_dola_row and its packing, the header and the binding, the two new vt_llama_model fields, the argument errors of
resolve_generate_args, SamplingParams(dola_layers=) and what the engine refuses at submit()."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dola_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- transformers 4.4x, ported literally (generation/utils.py), fp64, a batch of one -----------------------------------------------------
def _hf_relative_top_filter(scores, baseline_scores, relative_top=0.1, filter_value=-float("Inf"), base_filter_value=-1e-3,
                            min_tokens_to_keep=1):
    scores_normalized = scores.log_softmax(dim=-1)
    baseline_scores_normalized = baseline_scores.log_softmax(dim=-1)
    sorted_logits, sorted_indices = torch.sort(scores_normalized, descending=True)
    min_thresh = sorted_logits[..., min_tokens_to_keep - 1]
    probs_max = torch.max(scores_normalized, dim=-1).values
    probs_thresh = probs_max + np.log(relative_top)
    probs_thresh = torch.min(min_thresh, probs_thresh)
    probs_thresh = probs_thresh.unsqueeze(-1)
    baseline_scores_normalized[scores_normalized < probs_thresh] = base_filter_value
    scores_normalized[scores_normalized < probs_thresh] = filter_value
    return scores_normalized, baseline_scores_normalized


def _hf_dola_select_contrast(candidate_premature_layers, candidate_premature_logits, final_logits, relative_top=0.1):
    if len(candidate_premature_layers) == 1:
        base_logits = candidate_premature_logits[candidate_premature_layers[0]]
        final_logits, base_logits = _hf_relative_top_filter(final_logits, base_logits, relative_top)
        return final_logits - base_logits, candidate_premature_layers[0], None
    stacked_premature_layers = torch.stack([candidate_premature_logits[i] for i in candidate_premature_layers], dim=0)
    softmax_mature_layer = F.softmax(final_logits, dim=-1)
    softmax_premature_layers = F.softmax(stacked_premature_layers, dim=-1)
    avg_dist = 0.5 * (softmax_mature_layer[None, :, :] + softmax_premature_layers)
    log_softmax_mature_layer = F.log_softmax(final_logits, dim=-1)
    log_softmax_premature_layers = F.log_softmax(stacked_premature_layers, dim=-1)
    kl1 = F.kl_div(log_softmax_mature_layer[None, :, :], avg_dist, reduction="none").mean(-1)
    kl2 = F.kl_div(log_softmax_premature_layers, avg_dist, reduction="none").mean(-1)
    js_divs = 0.5 * (kl1 + kl2)
    js_divs = js_divs.mean(-1)
    premature_layer = candidate_premature_layers[int(js_divs.argmax().cpu().item())]
    base_logits = candidate_premature_logits[premature_layer]
    final_logits, base_logits = _hf_relative_top_filter(final_logits, base_logits, relative_top)
    return final_logits - base_logits, premature_layer, js_divs


@pytest.mark.parametrize("V,n_cand,rt", [(33, 1, 0.1), (33, 2, 0.1), (1025, 8, 0.1), (4097, 16, 0.02), (32000, 8, 0.1), (1025, 3, 1.0)])
def test_reference_matches_the_transformers_port(V, n_cand, rt):
    for seed in range(3):
        final, prem, j = R.ladder_case(V, n_cand, seed)
        layers = list(range(10, 10 + 2 * n_cand, 2))
        cand = {l: torch.from_numpy(prem[i]).double()[None] for i, l in enumerate(layers)}
        out, layer, js = _hf_dola_select_contrast(layers, cand, torch.from_numpy(final).double()[None], rt)
        got = R.row64(final, prem, rt)
        assert layers[got["j"]] == layer and got["j"] == j
        if js is not None:       # transformers' mean over V, then over the batch of one
            np.testing.assert_allclose(got["div"], js.numpy() * V, rtol=1e-10, atol=1e-13)
        else:
            assert got["div"].tolist() == [0.0]
        out = out[0].numpy()
        assert np.array_equal(np.isneginf(out), ~got["keep"]) and got["keep"][int(np.argmax(final))]
        np.testing.assert_allclose(got["out"][got["keep"]], out[got["keep"]], rtol=0, atol=1e-11)
        # the fp32 restatement, fed fp64 lse values rounded once: inside three roundings of magnitude max |lp| plus the lse roundings
        lse_f, lse_j = R.lse64(final)[0], R.lse64(prem[got["j"]])[0]
        o32 = R.out32(final, prem[got["j"]], lse_f, lse_j, rt)
        k = got["keep"]
        assert np.array_equal(np.isneginf(o32), ~k)
        scale = np.abs(final).max() + np.abs(prem).max() + abs(lse_f) + abs(lse_j)
        assert np.abs(o32[k] - got["out"][k]).max() <= 6 * R.U * scale


def test_layer_ranges():
    from vitron_amd.sampling import DOLA_MAX_LAYERS, dola_candidate_layers
    want = {(4, False): ([0], [2]), (4, True): ([], [2]), (8, False): ([0, 2], [4, 6]), (8, True): ([2], [4, 6]),
            (32, False): (list(range(0, 16, 2)), list(range(16, 32, 2))), (32, True): (list(range(2, 16, 2)), list(range(16, 32, 2))),
            (40, False): (list(range(0, 20, 2)), list(range(20, 40, 2))), (40, True): (list(range(2, 20, 2)), list(range(20, 40, 2))),
            (48, False): (list(range(0, 20, 2)), list(range(28, 48, 2))), (48, True): (list(range(2, 20, 2)), list(range(28, 48, 2)))}
    for (N, tied), (low, high) in want.items():
        assert R.candidate_layers("low", N, tied) == low and R.candidate_layers("high", N, tied) == high
        for name, layers in (("low", low), ("high", high)):
            if layers:
                assert list(dola_candidate_layers(name, N, tied)) == layers, (N, tied, name)
            else:
                with pytest.raises(ValueError, match="names no layer"):
                    dola_candidate_layers(name, N, tied)
    assert dola_candidate_layers([6, 1, 3], 8) == (6, 1, 3) and dola_candidate_layers((0,), 1) == (0,)     # a list keeps its order
    assert DOLA_MAX_LAYERS == R.MAX_LAYERS == 16 and len(dola_candidate_layers(list(range(16)), 32)) == 16
    for bad in ("mid", "", None, 3, 2.5, [], [8], [-1], [1, 1], [1.0], [True], list(range(17))):
        with pytest.raises(ValueError):
            dola_candidate_layers(bad, 32 if bad == list(range(17)) else 8)


def test_tie_rule_and_nan():
    assert R.choose([1.0, 2.0, 2.0]) == 1 and R.choose([3.0, 3.0]) == 0 and R.choose([0.5]) == 0
    assert R.choose([np.nan, 5.0]) == 0 and R.choose([1.0, np.nan, 2.0]) == 2 and R.choose([1.0, np.nan]) == 0
    final, prem, _ = R.ladder_case(1025, 4, 0, furthest_at=2)
    prem[0] = prem[2]                                    # two bitwise equal rows: the lower index
    got = R.row64(final, prem)
    assert got["div"][0] == got["div"][2] and got["j"] == 0
    prem[1] = final                                      # a candidate equal to the final row: divergence exactly 0, never chosen
    got = R.row64(final, prem)
    assert got["div"][1] == 0.0 and got["j"] == 0
    bad = final.copy()
    bad[7] = np.nan                                      # a NaN row: NaN divergences, j = 0, NaN where kept, -inf elsewhere
    got = R.row64(bad, prem)
    assert np.isnan(got["div"]).all() and got["j"] == 0 and not got["keep"][7] and got["keep"].any()
    assert np.isnan(got["out"][got["keep"]]).all() and np.isneginf(got["out"][~got["keep"]]).all()
    assert np.array_equal(got["keep"], R.keep(final, 0.1) & (np.arange(1025) != 7))      # the maximum skips the NaN
    o32 = R.out32(bad, prem[0], np.nan, 1.0, 0.1)
    assert np.isnan(o32[got["keep"]]).all() and np.isneginf(o32[~got["keep"]]).all()
    inf = final.copy()
    inf[3] = -np.inf                                     # -inf is an ordinary value: p_f = 0 < p_j there makes the divergence +inf
    got = R.row64(inf, prem)
    assert np.isposinf(got["div"]).all() and got["j"] == 0 and not got["keep"][3] and np.isneginf(got["out"][3])
    both = prem.copy()
    both[:, 3] = -np.inf                                 # p_f = p_j = 0: M == 0, the term counts 0
    got = R.row64(inf, both)
    assert np.isfinite(got["div"]).all() and got["div"][0] > 0 and got["div"][1] == 0.0 and np.isneginf(got["out"][3])


def test_keep_rule_at_the_threshold():
    for rt in (0.1, 0.5, 0.013):
        lrt = R.log_rt(rt)
        for m in (F32(3.25), F32(-17.5), F32(1e-3)):
            thr = F32(m + lrt)
            row = np.array([m, thr, np.nextafter(thr, F32(-np.inf)), np.nextafter(thr, F32(np.inf)), F32(-50.0)], dtype=F32)
            assert R.keep(row, rt).tolist() == [True, True, False, True, False]
            words = R.mask(row, rt)
            assert words.tolist() == [0b01011]
            assert R.mask(row, rt, base=np.array([0xfffffff9], dtype=np.uint32)).tolist() == [0xffffffe9]     # tail bits: base's own
    row = np.full((40,), 2.0, dtype=F32)                 # relative_top = 1: only the ties for the maximum
    row[5] = 1.9999999
    assert R.keep(row, 1.0).sum() == 39 and R.mask(row, 1.0).tolist() == [0xffffffdf, 0xff]


def test_bound_and_ladder_builder():
    for V in (33, 1025, 32000):
        final, prem, j = R.ladder_case(V, 8, 1)
        d64 = R.divergences64(final, prem)
        for k in range(8):
            b = R.div_bound(final, prem[k])
            assert 0 < b < 1e-3 and abs(float(R.div32(final, prem[k])) - d64[k]) <= b
        assert R.div_bound(final, prem[0], reg=False) >= R.div_bound(final, prem[0], reg=True) * 0.5
    for pos in range(8):
        assert R.ladder_case(1025, 8, 2, furthest_at=pos)[2] == pos
    assert R.chain(32000, True) == 54 and R.chain(50000, False) == 49 + 22 and R.register_form(32768) and not R.register_form(32769)
    assert not R.register_form(100, (0, 4, 0)) and not R.register_form(100, (0, 0, 0), prem_stride=102)


# ---- struct, header, binding ---------------------------------------------------------------------------------------------------------------
def test_row_struct_against_the_header():
    from vitron_amd.sampling import DOLA_ROW_BYTES, DOLA_ROW_DTYPE, dola_rows_array
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    doc = hdr[hdr.index("DOLA (DESIGN.md 9.14"):hdr.index("typedef struct vt_dola_row")]
    table = {m.group(2): int(m.group(1)) for m in
             re.finditer(r"^ \*\s+(\d+) (?:const )?(?:float|uint32_t|fp32|int64|int)\*?\s+(\w+)", doc, flags=re.M)}
    assert table == {n: DOLA_ROW_DTYPE.fields[n][1] for n in DOLA_ROW_DTYPE.names}, table
    body = re.search(r"typedef struct vt_dola_row \{(.*?)\} vt_dola_row;", hdr, flags=re.S).group(1)
    assert [ln.split()[-1].rstrip(";") for ln in body.strip().splitlines()] == list(DOLA_ROW_DTYPE.names)
    assert "80 bytes each" in doc and DOLA_ROW_BYTES == 80 and re.search(r"#define VT_DOLA_MAX_LAYERS 16\b", hdr)

    class Row(C.Structure):
        _fields_ = [(n, C.c_void_p) for n in DOLA_ROW_DTYPE.names[:8]] + [("prem_stride", C.c_longlong), ("n_cand", C.c_int),
                                                                         ("log_relative_top", C.c_float)]
    assert C.sizeof(Row) == 80 and all(getattr(Row, n).offset == DOLA_ROW_DTYPE.fields[n][1] for n in DOLA_ROW_DTYPE.names)
    arr = dola_rows_array([(16, 32, 1000, 8, 16, 0, 48, 64, 80, 96, np.log(0.1)), (0,) * 10 + (0.0,)])
    assert arr["final"].tolist() == [16, 0] and arr["out"][0] == 16 and arr["prem_stride"][0] == 1000 and arr["n_cand"].tolist() == [8, 0]
    assert arr["log_relative_top"][0] == F32(np.log(0.1)) and arr["layer_out"][0] == 64 and arr["lse_out"][0] == 96
    for bad in ((16, 0, 4, 1, 16, 0, 0, 0, 0, 0, 0.0), (16, 32, 4, 1, 0, 0, 0, 0, 0, 0, 0.0), (-1, 32, 4, 1, 16, 0, 0, 0, 0, 0, 0.0),
                (16, 32, 4, 1, 16, 48, 48, 0, 0, 0, 0.0)):
        with pytest.raises(ValueError):
            dola_rows_array([bad])


def test_header_build_and_binding():
    from vitron_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_dola_rows\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_dola_rows is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["rows", "n_rows", "V", "stream"]
    doc = hdr[hdr.index("DOLA (DESIGN.md 9.14"):m.start()]
    for needle in ("_dola_decoding", "_relative_top_filter", "MAY alias final", "skipped entirely", "BIT FOR BIT", "VT_LOGPROB_MAX_V",
                   "n_rows <= 0", "layer_out = -1", "ties and NaNs go to the lower j", "M == 0 counting 0"):
        assert needle in doc, needle
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    assert len(_lib.SIGNATURES["vt_dola_rows"][1]) == 4
    assert "vt_dola.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "vitron_amd", "csrc", "vt_dola.hip"))
    assert callable(ops.dola_rows)
    src = open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_kernels.h")).read() + open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_api.hip")).read()
    assert src.count("vt_dola_rows_launch") >= 2
    kern = open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_dola.hip")).read()
    for fn, end in (("float dola_term(", "// the contrast"), ("float dola_out(", "__device__ __forceinline__ uint32_t dola_base_word")):
        body = kern[kern.index(fn):kern.index(end)]
        assert "#pragma clang fp contract(off)" in body and "fma" not in body.lower()      # every operation rounds on its own


def test_llama_model_gains_its_two_fields_at_the_end():
    from vitron_amd import _lib
    names = [f[0] for f in _lib.VtLlamaModel._fields_]
    assert names[-3:] == ["hidden_trace", "logit_row_trace", "logit_row_trace_layers"]
    assert _lib.VtLlamaModel.logit_row_trace.offset == _lib.VtLlamaModel.hidden_trace.offset + 8
    assert C.sizeof(_lib.VtLlamaModel) == _lib.VtLlamaModel.logit_row_trace_layers.offset + 8
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    body = re.search(r"typedef struct vt_llama_model \{(.*?)\} vt_llama_model;", hdr, flags=re.S).group(1)
    decl = re.findall(r"^\s*(?:const )?\w+\*? (\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert decl[-3:] == ["hidden_trace", "logit_row_trace", "logit_row_trace_layers"], decl[-4:]
    m = _lib.VtLlamaModel()
    assert m.logit_row_trace is None and m.logit_row_trace_layers is None                  # zero-initialised: off


# ---- generate()'s arguments -----------------------------------------------------------------------------------------------------------------
def _resolve(**kw):
    from vitron_amd.picker import resolve_generate_args
    cfg = types.SimpleNamespace(eos_token_id=2, pad_token_id=0, vocab_size=64, top_k=50, num_hidden_layers=8)
    args = dict(do_sample=False, temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=4, max_length=None, stopping_criteria=None,
                eos_token_id=None, pad_token_id=None, num_beams=1, seed=None, return_logits=False, padded_batch=False, repetition_penalty=1.0,
                return_logprobs=False, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None,
                allowed_token_ids=None, num_return_sequences=1, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None,
                batch_size=2)
    args.update(kw)
    return resolve_generate_args(cfg, 5, **args)


def test_generate_arguments_resolve_and_refuse():
    plain = _resolve()
    assert not plain.dola and plain.dola_layers is None and not plain.per_row and plain.given == ()
    assert not _resolve(dola_layers=None, dola_relative_top=0.5).dola
    a = _resolve(dola_layers="high")
    assert a.dola and a.dola_layers == (4, 6) and a.dola_relative_top == 0.1 and a.per_row and a.given == ("dola_layers=...",)
    assert _resolve(dola_layers="low").dola_layers == (0, 2) and _resolve(dola_layers=[6], dola_relative_top=1).dola_layers == (6,)
    assert _resolve(dola_layers=[5, 1], dola_relative_top=0.25, do_sample=True, seed=3).dola_relative_top == 0.25
    for bad in ("mid", [], [8], [1, 1], 4, [0.5]):
        with pytest.raises(ValueError, match="dola_layers"):
            _resolve(dola_layers=bad)
    for bad in (0, -0.1, 1.5, float("nan"), "x", None, True):
        with pytest.raises(ValueError, match="dola_relative_top"):
            _resolve(dola_layers="low", dola_relative_top=bad)
    with pytest.raises(ValueError, match="dola_relative_top"):
        _resolve(dola_relative_top=2.0)                                                     # checked even when DoLa is off
    with pytest.raises(NotImplementedError, match=r"num_beams > 1, dola_layers"):
        _resolve(dola_layers="low", num_beams=2)
    with pytest.raises(NotImplementedError, match="dola_layers.*padded_batch"):
        _resolve(dola_layers="low", padded_batch=True)
    with pytest.raises(NotImplementedError, match="dola_layers.*guidance_scale"):
        _resolve(dola_layers="low", guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="dola_layers.*penalty_alpha"):
        _resolve(dola_layers="low", penalty_alpha=0.6, top_k=4)
    b = _resolve(dola_layers="low", repetition_penalty=1.2, no_repeat_ngram_size=2, choices=[[3, 4], [5]])
    assert b.dola and b.ngram == 2 and b.automaton is not None


def test_sampling_params_and_submit():
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    sp = SamplingParams(dola_layers=[4, 6], dola_relative_top=0.2)
    assert sp.dola and sp.dola_layers == (4, 6) and "dola_layers=(4, 6)" in repr(sp) and "dola_relative_top=0.2" in repr(sp)
    assert sp == SamplingParams(dola_layers=(4, 6), dola_relative_top=0.2) != SamplingParams(dola_layers=[4, 6])
    assert hash(sp) == hash(sp.replace()) and sp.replace(temperature=0.7).dola_layers == (4, 6)
    assert sp.replace(dola_layers="high").dola_layers == "high" and not sp.replace(dola_layers=None).dola
    plain = SamplingParams()
    assert not plain.dola and "dola" not in repr(plain) and plain == SamplingParams() and plain != sp
    assert not sp.guided and not sp.constrained
    for kw in (dict(dola_layers="mid"), dict(dola_layers=[]), dict(dola_layers=[1, 1]), dict(dola_layers=[-1]), dict(dola_layers=3),
               dict(dola_layers="low", dola_relative_top=0), dict(dola_layers="low", dola_relative_top=1.01), dict(dola_relative_top="x")):
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    with pytest.raises(NotImplementedError, match="dola_layers together with guidance_scale"):
        SamplingParams(dola_layers="low", guidance_scale=2.0)
    with pytest.raises(Exception):
        sp.dola_layers = "low"                                                             # frozen like every field
    eng = ServingEngine(types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=64, num_hidden_layers=8), device="cpu"))
    ids = torch.tensor([[1, 5, 6, 7]])
    h = eng.submit(ids, sampling=SamplingParams(dola_layers="high"))
    l = eng.submit(ids, sampling=sp)
    u = eng.submit(ids, sampling=plain)
    held = {r.rid: r for r in eng.waiting}
    assert held[h].dola == (4, 6) and held[h].rows == 1 and held[l].dola == (4, 6) and held[u].dola is None
    assert eng._dola_layers([held[h], held[u]]) == [4, 6] and eng._dola_layers([held[u]]) is None
    with pytest.raises(ValueError, match="dola_layers"):
        eng.submit(ids, sampling=SamplingParams(dola_layers=[9]))                           # no layer 9 in an 8-layer model
    tied = ServingEngine(types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=64, num_hidden_layers=4,
                                                                            tie_word_embeddings=True), device="cpu"))
    with pytest.raises(ValueError, match="names no layer"):
        tied.submit(ids, sampling=SamplingParams(dola_layers="low"))
    assert eng.pending() == 3 and all(eng.cancel(r) for r in (h, l, u)) and eng.pending() == 0 and tied.pending() == 0
