"""Classifier-free guidance without a GPU: tests/cfg_ref.py against torch in fp64 and against transformers'
UnbatchedClassifierFreeGuidanceLogitsProcessor, the plausibility-mask rule, struct vt_cfg_row and its packing, the header and the
binding, the argument errors of resolve_generate_args, SamplingParams(guidance_scale=) and what the engine refuses at submit()."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cfg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _rows(V, seed):
    g = torch.Generator().manual_seed(seed)
    c = (torch.randn((3, V), generator=g) * 4.0).numpy()
    u = (torch.randn((3, V), generator=g) * 4.0).numpy()
    return c, u


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (1.5, 0.0, -0.5, 7.0, 1.0))
def test_guided64_is_the_textbook_expression(scale):
    c, u = _rows(777, 5)
    cl = torch.log_softmax(torch.from_numpy(c).double(), -1)
    ul = torch.log_softmax(torch.from_numpy(u).double(), -1)
    want = (scale * (cl - ul) + ul).numpy()
    got = R.guided64(c, u, scale)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, abs(scale)) * np.abs(want).max()
    # the fp32 restatement from the fp64 lse values, rounded: within fp32 rounding of the fp64 row (three roundings of |x| <= ~60 values)
    lc, lu = R.lse64(c), R.lse64(u)
    for r in range(3):
        g32 = R.guided32(c[r], u[r], scale, lc[r], lu[r])
        assert g32.dtype == F32
        assert np.abs(g32 - want[r]).max() <= 2.0 ** -23 * (4 + 4 * abs(scale)) * 80.0


def test_guided64_equals_transformers_processor():
    try:
        from transformers import UnbatchedClassifierFreeGuidanceLogitsProcessor as Proc
    except Exception:  # noqa: BLE001
        pytest.skip("the installed transformers has no UnbatchedClassifierFreeGuidanceLogitsProcessor")
    c, u = _rows(300, 9)
    fed = []

    class Out(dict):
        logits = None

    def stub(input_ids, attention_mask=None, use_cache=True, past_key_values=None):
        fed.append((input_ids.clone(), attention_mask.clone()))
        out = Out()
        out.logits = torch.from_numpy(u).double().unsqueeze(1).expand(3, input_ids.shape[1], 300)
        return out

    ids = torch.tensor([[4, 5, 6]] * 3)
    for scale in (1.5, 0.0, -0.5, 7.0):
        proc = Proc(scale, stub, unconditional_ids=None)
        got = proc(ids, torch.from_numpy(c).double()).numpy()
        assert np.abs(got - R.guided64(c, u, scale)).max() <= 1e-11 * max(1.0, abs(scale))
    assert fed[0][0].tolist() == [[6]] * 3                     # its default negative prompt: the last token (negative_prompt's default too)


def test_default_negative_prompt_and_broadcast():
    from vitron_amd.picker import negative_prompt
    ids = torch.tensor([[1, 7, 9, 0], [1, -200, 8, 5]])
    neg, am = negative_prompt(ids, None, None, None)
    assert neg.tolist() == [[0], [5]] and am is None
    neg, _ = negative_prompt(ids, torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1]]), None, None)
    assert neg.tolist() == [[9], [5]]                          # the last token the mask keeps
    with pytest.raises(ValueError, match="sentinel"):
        negative_prompt(torch.tensor([[1, 7, -200]]), None, None, None)
    with pytest.raises(ValueError, match="sentinel"):
        negative_prompt(ids, torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]]), None, None)
    neg, am = negative_prompt(ids, None, torch.tensor([[3, 4, 5]]), torch.tensor([[1, 1, 0]]))
    assert neg.tolist() == [[3, 4, 5]] * 2 and am.tolist() == [[1, 1, 0]] * 2


# ---- the mask ------------------------------------------------------------------------------------------------------------------------------
def _bits(words, V):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:V].astype(bool)


@pytest.mark.parametrize("V", (1, 33, 64, 1025))
def test_mask_rule(V):
    from vitron_amd.sampling import allow_mask
    c, _ = _rows(V, 40 + V)
    c = c[0]
    top = int(np.argmax(c))
    p = torch.softmax(torch.from_numpy(c).double(), -1).numpy()
    full = _bits(R.mask(c, 0.0), V)
    assert full.all()                                                                     # beta = 0: no cut
    one = _bits(R.mask(c, 1.0), V)
    assert one[top] and (one == (c == c[top])).all()                                      # beta = 1: the maxima alone
    tenth = _bits(R.mask(c, 0.1), V)
    assert tenth[top]
    sure = np.abs(p - 0.1 * p.max()) > 1e-5 * p.max()                                     # away from the threshold the fp32 rule is the textbook one
    assert (tenth[sure] == (p >= 0.1 * p.max())[sure]).all()
    # a base: its bits below V are intersected, the tail of its last word is kept as it is; without one the tail is clear
    banned = sorted({top, 0, V - 1})
    base = allow_mask(V, None, banned)
    base[-1] |= np.uint32((0xffffffff << (V & 31)) & 0xffffffff) if V & 31 else np.uint32(0)
    got = R.mask(c, 0.1, base)
    assert (_bits(got, V) == (tenth & ~np.isin(np.arange(V), banned))).all()
    if V & 31:
        assert int(got[-1]) >> (V & 31) == (1 << (32 - (V & 31))) - 1 and int(R.mask(c, 0.1)[-1]) >> (V & 31) == 0
    # a NaN fails the comparison and is skipped by the maximum; a tie exactly at the threshold stays
    if V >= 33:
        d = c.copy()
        d[1] = np.nan
        d[2] = F32(R.row_max(d) + R.log_beta(0.1))
        m = _bits(R.mask(d, 0.1), V)
        assert not m[1] and m[2] and m[int(np.nanargmax(d))]


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------
def test_cfg_row_struct():
    from vitron_amd.sampling import CFG_ROW_BYTES, CFG_ROW_DTYPE, cfg_rows_array, log_beta
    assert CFG_ROW_BYTES == 56 == CFG_ROW_DTYPE.itemsize
    p = [0x1122334455667700 + 16 * i for i in range(6)]
    arr = cfg_rows_array([(p[0], p[1], p[0], p[3], p[4], p[5], 1.5, log_beta(0.1)), (0, 0, 0, 0, 0, 0, 1.0, log_beta(0.0))])
    raw = arr.view(np.uint8).reshape(2, 56)
    u64 = lambda r, o: int(raw[r, o:o + 8].view("<u8")[0])                                # noqa: E731
    f32 = lambda r, o: float(raw[r, o:o + 4].view("<f4")[0])                              # noqa: E731
    assert [u64(0, 8 * i) for i in range(6)] == [p[0], p[1], p[0], p[3], p[4], p[5]]       # cond uncond out (in place) base mask_out lse_out
    assert f32(0, 48) == 1.5 and f32(0, 52) == float(F32(np.log(0.1))) and f32(1, 52) == -np.inf and u64(1, 0) == 0
    for bad in ((p[0], 0, p[2], 0, 0, 0, 1.0, 0.0), (p[0], p[1], 0, 0, 0, 0, 1.0, 0.0), (p[0], p[1], p[1], 0, 0, 0, 1.0, 0.0),
                (p[0], p[1], p[2], p[3], p[3], 0, 1.0, 0.0), (-8, p[1], p[2], 0, 0, 0, 1.0, 0.0)):
        with pytest.raises(ValueError):
            cfg_rows_array([bad])
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    doc = hdr[hdr.index("CLASSIFIER-FREE GUIDANCE"):hdr.index("typedef struct vt_cfg_row")]
    table = {m.group(2): int(m.group(1)) for m in re.finditer(r"^ \*\s+(\d+) (?:const )?(?:float|uint32_t|fp32)\*?\s+(\w+)", doc, flags=re.M)}
    assert table == {n: CFG_ROW_DTYPE.fields[n][1] for n in CFG_ROW_DTYPE.names}, table
    body = re.search(r"typedef struct vt_cfg_row \{(.*?)\} vt_cfg_row;", hdr, flags=re.S).group(1)
    assert [ln.split()[-1].rstrip(";") for ln in body.strip().splitlines()] == list(CFG_ROW_DTYPE.names)
    assert "56 bytes each" in doc


def test_header_build_and_binding():
    from vitron_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_cfg_rows\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_cfg_rows is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["rows", "n_rows", "V", "stream"]
    doc = hdr[hdr.index("CLASSIFIER-FREE GUIDANCE"):m.start()]
    for needle in ("UnbatchedClassifierFreeGuidanceLogitsProcessor", "MAY alias cond", "must NOT alias uncond", "skipped entirely",
                   "BIT FOR BIT", "no fused multiply-add", "VT_LOGPROB_MAX_V", "n_rows <= 0", "A NaN c_i fails", "vt_ban_rows"):
        assert needle in doc, needle
    assert "vt_cfg_rows and struct vt_cfg_row WITHOUT a bump" in hdr
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    assert len(_lib.SIGNATURES["vt_cfg_rows"][1]) == 4
    assert "vt_cfg.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "vitron_amd", "csrc", "vt_cfg.hip"))
    assert callable(ops.cfg_rows)
    src = open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_kernels.h")).read() + open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_api.hip")).read()
    assert src.count("vt_cfg_rows_launch") >= 2
    kern = open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_cfg.hip")).read()
    blend = kern[kern.index("float cfg_blend("):kern.index("// word w of the starting mask")]
    assert "#pragma clang fp contract(off)" in blend and "fma" not in blend.lower()       # the three roundings: no contraction in the blend


# ---- generate()'s arguments -----------------------------------------------------------------------------------------------------------------
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


def test_generate_arguments_resolve_and_refuse():
    neg = torch.tensor([[3, 4, 5]])
    plain = _resolve()
    assert not plain.guided and plain.guidance_scale is None and plain.guidance_plausibility == 0.0 and not plain.per_row and plain.given == ()
    off = _resolve(guidance_scale=1, negative_prompt_ids=neg)                              # a scale of 1 is off, whatever comes with it
    assert not off.guided and not off.per_row and off.given == ()
    a = _resolve(guidance_scale=2.0, negative_prompt_ids=neg)
    assert a.guided and a.guidance_scale == 2.0 and not a.per_row and a.given == ("guidance_scale=...",)
    assert _resolve(guidance_scale=0).guided and _resolve(guidance_scale=-0.5).guidance_scale == -0.5
    b = _resolve(guidance_scale=1.5, guidance_plausibility=0.1, negative_prompt_ids=torch.tensor([[3], [4]]))
    assert b.guided and b.per_row and b.guidance_plausibility == 0.1
    for bad in (float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match="guidance_scale"):
            _resolve(guidance_scale=bad)
    for bad in (-0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="guidance_plausibility"):
            _resolve(guidance_scale=2.0, guidance_plausibility=bad)
    with pytest.raises(ValueError, match="guidance_plausibility needs"):
        _resolve(guidance_plausibility=0.5)
    with pytest.raises(ValueError, match="guidance_plausibility needs"):
        _resolve(guidance_scale=1, guidance_plausibility=0.5)
    for name, value in (("negative_prompt_ids", neg), ("negative_attention_mask", torch.ones((1, 3))), ("negative_images", [torch.zeros(3, 4, 4)]),
                        ("negative_regions", [None])):
        with pytest.raises(ValueError, match=name + " needs guidance_scale"):
            _resolve(**{name: value})
    with pytest.raises(ValueError, match="negative_images needs negative_prompt_ids"):
        _resolve(guidance_scale=2.0, negative_images=[torch.zeros(3, 4, 4)])
    with pytest.raises(ValueError, match="batch size 3"):
        _resolve(guidance_scale=2.0, negative_prompt_ids=torch.zeros((3, 4), dtype=torch.long))
    with pytest.raises(ValueError, match="empty"):
        _resolve(guidance_scale=2.0, negative_prompt_ids=torch.zeros((2, 0), dtype=torch.long))
    with pytest.raises(ValueError, match="empty"):
        _resolve(guidance_scale=2.0, negative_prompt_ids=neg, negative_attention_mask=torch.zeros((1, 3), dtype=torch.long))
    with pytest.raises(ValueError, match="negative_attention_mask has shape"):
        _resolve(guidance_scale=2.0, negative_prompt_ids=neg, negative_attention_mask=torch.ones((1, 2), dtype=torch.long))
    with pytest.raises(ValueError, match=r"\[B, Ln\]"):
        _resolve(guidance_scale=2.0, negative_prompt_ids=torch.tensor([3, 4]))
    with pytest.raises(NotImplementedError, match=r"num_beams > 1, guidance_scale"):
        _resolve(guidance_scale=2.0, num_beams=2)
    with pytest.raises(NotImplementedError, match="padded_batch=True.*guidance_scale"):
        _resolve(guidance_scale=2.0, padded_batch=True)
    _resolve(guidance_scale=1, num_beams=2)                                                # off: a beam call does not see it


def test_sampling_params_and_submit():
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    sp = SamplingParams(guidance_scale=2.0, negative_prompt_ids=torch.tensor([[3, 4]]))
    assert sp.guided and sp.negative_prompt_ids == (3, 4) and "guidance_scale=2.0" in repr(sp) and "negative_prompt_ids=(3, 4)" in repr(sp)
    assert sp == SamplingParams(guidance_scale=2.0, negative_prompt_ids=[3, 4]) != SamplingParams(guidance_scale=2.0, negative_prompt_ids=[3, 5])
    assert hash(sp) == hash(sp.replace()) and sp.replace(guidance_scale=3.0).guidance_scale == 3.0
    assert sp.replace(guidance_scale=3.0).negative_prompt_ids == (3, 4)
    plain = SamplingParams()
    assert not plain.guided and not SamplingParams(guidance_scale=1).guided and "guidance" not in repr(plain) and plain == SamplingParams()
    with pytest.raises(NotImplementedError, match="guidance_plausibility"):
        SamplingParams(guidance_scale=2.0, guidance_plausibility=0.1)
    with pytest.raises(NotImplementedError, match="negative_images"):
        SamplingParams(guidance_scale=2.0, negative_prompt_ids=[3], negative_images=[torch.zeros(3, 4, 4)])
    for kw in (dict(guidance_scale=float("nan")), dict(negative_prompt_ids=[3]), dict(guidance_scale=2.0, negative_prompt_ids=[]),
               dict(guidance_scale=2.0, negative_prompt_ids=[3, -200]), dict(guidance_scale=2.0, negative_prompt_ids=[[1, 2], [3, 4]])):
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    eng = ServingEngine(types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=64), device="cpu"))
    ids = torch.tensor([[1, 5, 6, 7]])
    g = eng.submit(ids, sampling=sp)
    d = eng.submit(ids, sampling=SamplingParams(guidance_scale=2.0))
    u = eng.submit(ids, sampling=SamplingParams(guidance_scale=1))
    held = {r.rid: r for r in eng.waiting}
    assert held[g].rows == 2 and held[g].neg_ids.tolist() == [[3, 4]] and held[g].nseq is not None
    assert held[d].rows == 2 and held[d].neg_ids.tolist() == [[7]]                         # the default: the prompt's last token
    assert held[u].rows == 1 and held[u].nseq is None and held[u].neg_ids is None
    with pytest.raises(ValueError, match="sentinel"):
        eng.submit(torch.tensor([[1, 5, -200]]), sampling=SamplingParams(guidance_scale=2.0))
    assert eng.pending() == 3 and all(eng.cancel(r) for r in (g, d, u)) and eng.pending() == 0
