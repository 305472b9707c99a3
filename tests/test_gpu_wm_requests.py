"""watermarking_config end to end on the tiny synthetic model (tests/allow_cases.py, V = 512): generate(do_sample=True,
top_k=8, watermarking_config=, return_logits=True) teacher-forced from the returned rows through tests/synthid_ref.py -- the sampler's
fp64 keep-set, the fp64 tournament behind the cell's context, the kernel's uniform -- predicts every emitted id (a step whose uniform
lies within 1e-4 of a seam of the fp64 CDF is left out; at most 2 of 48 may be, about 0.1 is expected: 8 seams x 2e-4); the same
request through a ServingEngine beside a plain one; the launches; the refusals. mean_g of the watermarked and of the plain reply is
recorded, not asserted (48 tokens of a synthetic model score too few n-grams for a bound)."""
import inspect

import numpy as np
import pytest
import torch

from tests import sample_ref as S
from tests import synthid_ref as W
from tests import trunc_ref as R
from tests.golden import cases as G
from tests.allow_cases import solo as _solo, submit as _submit, tiny_model

pytestmark = pytest.mark.gpu
TV = G.LLM["vocab_size"]
NEW, TOP_K, SEED, SEAM = 48, 8, 17, 1e-4
CFG = W.Config(5, W.KEYS30[:9], history_size=64)


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return tiny_model(dev)


@pytest.fixture(scope="module")
def reqs():
    g = torch.Generator().manual_seed(131)
    rnd = lambda n: torch.randint(3, TV, (n,), generator=g).tolist()                    # noqa: E731
    return [dict(input_ids=torch.tensor([[1] + rnd(13)]), images=None, regions=None, max_new_tokens=NEW),
            dict(input_ids=torch.tensor([[1] + rnd(21)]), images=None, regions=None, max_new_tokens=9)]


def _predict(rows, emitted, seed, stream=0):
    """(agreeing steps, steps left out, the restatement's flags per step) for one sample: rows fp32 [steps, V] as returned, emitted the
    ids the call returned for them. The context is teacher-forced with the EMITTED id."""
    cell = W.Cell(CFG)
    left_out, flags_seen = 0, []
    for st, tok in enumerate(emitted):
        s = R.scaled(rows[st], 1.0)
        A = R.base_keep(s, TOP_K, 1.0)
        assert A.sum() == TOP_K
        q, flags = cell.call(np.where(A, np.exp(np.where(A, s, 0.0) - s[A].max()), 0.0))
        want, dist, _ = W.pick(q, S.uniform24(seed, st, stream))
        flags_seen.append(flags)
        print(f"step {st}: emitted {tok} fp64 {want} seam {dist:.2e} flags {flags} q {q[want]:.3f}")
        if dist < SEAM:
            left_out += 1
        else:
            assert tok == want, (st, tok, want, dist)
        assert A[tok]
        cell.finish(tok)
    return left_out, flags_seen


@pytest.fixture(scope="module")
def marked(dev, model, reqs):
    """The watermarked reply to reqs[0] with its raw rows, the plain reply from the same seed: computed once"""
    ids = reqs[0]["input_ids"].to(dev)
    kw = dict(max_new_tokens=NEW, eos_token_id=-1, do_sample=True, temperature=1.0, top_k=TOP_K, top_p=1.0, seed=SEED)
    out, rows = model.generate(ids, return_logits=True, watermarking_config=CFG.as_dict(), **kw)
    plain = model.generate(ids, **kw)
    L = ids.shape[1]
    return dict(ids=out[0, L:].cpu().tolist(), rows=torch.stack(rows)[:, 0].float().cpu().numpy(), plain=plain[0, L:].cpu().tolist(), all=out[0].cpu(), L=L,
                plain_all=plain[0].cpu())


def test_generate_follows_the_fp64_restatement(marked, record_property):
    from vitron_amd.watermark import SynthIDWatermark
    assert len(marked["ids"]) == NEW and marked["rows"].shape == (NEW, TV)
    left_out, flags = _predict(marked["rows"], marked["ids"], SEED)
    assert left_out <= 2, left_out
    assert flags.count(W.WATERMARKED) >= NEW - 8, flags                           # (a repeated context is drawn plainly; few are)
    assert marked["ids"] != marked["plain"]                                       # the tournament moved the draws
    wm = SynthIDWatermark(CFG.as_dict())
    for name, seq in (("watermarked", marked["all"]), ("plain", marked["plain_all"])):
        mean, count = wm.mean_g(seq, generated_from=marked["L"], return_count=True)
        print(f"mean g of the {name} reply: {mean:.4f} over {count} g-values (sigma {0.5 / np.sqrt(max(count, 1)):.4f})")
        record_property(f"mean_g_{name}", mean)
        record_property(f"g_values_{name}", count)


def test_a_batch_of_two_rows_owns_two_cells(dev, model, reqs, marked):
    """B = 2 of the same prompt: row 0 draws what the call of one draws (stream 0), row 1 (stream 1) follows the restatement too"""
    ids = reqs[0]["input_ids"].to(dev).repeat(2, 1)
    out, rows = model.generate(ids, return_logits=True, watermarking_config=CFG.as_dict(), max_new_tokens=12, eos_token_id=-1,
                               do_sample=True, temperature=1.0, top_k=TOP_K, top_p=1.0, seed=SEED)
    got = out[:, marked["L"]:].cpu().tolist()
    assert got[0] == marked["ids"][:12]
    left_out, _ = _predict(torch.stack(rows)[:, 1].float().cpu().numpy(), got[1], SEED, stream=1)
    assert left_out <= 1
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_request_beside_a_plain_one(dev, model, reqs, marked):
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    sp = SamplingParams(temperature=1.0, top_k=TOP_K, top_p=1.0, seed=SEED, watermarking_config=CFG.as_dict())
    nb = SamplingParams(temperature=0.9, top_k=TOP_K, seed=7)
    assert _solo(model, dev, reqs[0], sp, watermarking_config=CFG.as_dict()) == marked["ids"]       # (what the restatement predicted)
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    alone = _submit(eng, reqs[1], nb)
    plain_alone = eng.run()[alone].cpu().tolist()[-reqs[1]["max_new_tokens"]:]
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    a, b = _submit(eng, reqs[0], sp), _submit(eng, reqs[1], nb)
    out = eng.run()
    assert not eng.failed
    assert out[a].cpu().tolist()[-NEW:] == marked["ids"]
    assert out[b].cpu().tolist()[-reqs[1]["max_new_tokens"]:] == plain_alone
    assert eng.finished[a].wm_cell is None                                       # dropped at retirement
    assert len(model.kv.free) == model.kv.num_pages
    assert sp == sp.replace() and sp != sp.replace(watermarking_config=None) and "watermarking_config" in repr(sp)


@pytest.fixture
def calls(monkeypatch):
    """Recorders around the pick launches that call through: the names in launch order; a sampler launch is noted as
    ("sample_rows", was watermark given)."""
    from vitron_amd import ops
    seen = []

    def wrap(name):
        real = getattr(ops, name)
        sig = inspect.signature(real)

        def recorder(*a, **kw):
            seen.append((name, sig.bind(*a, **kw).arguments.get("watermark") is not None) if name == "sample_rows" else name)
            return real(*a, **kw)
        return recorder
    for name in ("argmax", "sample_top_p", "sample_rows", "ban_rows", "bias_rows", "beam_step"):
        monkeypatch.setattr(ops, name, wrap(name))
    return seen


def test_launches_and_refusals(dev, model, reqs, calls):
    from transformers import WatermarkingConfig
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    ids = reqs[0]["input_ids"].to(dev)
    n = 3
    gen = lambda **kw: model.generate(ids, max_new_tokens=n, eos_token_id=-1, **kw)[0, ids.shape[1]:].cpu().tolist()     # noqa: E731
    WM, PLAIN = ("sample_rows", True), ("sample_rows", False)
    cfg = CFG.as_dict()
    plain = gen(do_sample=True, seed=3)
    assert calls == ["sample_top_p"] * n, calls                                    # without the argument: the launches it always ran
    del calls[:]
    assert gen(do_sample=True, seed=3, watermarking_config=None) == plain and calls == ["sample_top_p"] * n
    del calls[:]
    gen(do_sample=True, seed=3, watermarking_config=cfg)
    assert calls == [WM] * n, calls                                                # exactly one vt_sample_rows_wm launch per step
    del calls[:]
    gen(do_sample=True, seed=3, watermarking_config=cfg, min_p=0.05, repetition_penalty=1.2, no_repeat_ngram_size=2,
        sequence_bias={(5,): 1.0}, presence_penalty=0.2)
    assert calls == ["ban_rows", "bias_rows", WM] * n, calls                       # behind everything in front of the sampler
    del calls[:]
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    _submit(eng, reqs[1], SamplingParams(temperature=0.9, seed=7))
    eng.run()
    assert calls and all(c == PLAIN for c in calls), calls                         # no watermarked request: what it launched before
    del calls[:]
    _submit(eng, reqs[1], SamplingParams(temperature=0.9, seed=7, watermarking_config=cfg))
    _submit(eng, dict(reqs[1], max_new_tokens=4))
    eng.run()
    assert calls.count(WM) == reqs[1]["max_new_tokens"] and all(c in (WM, "argmax") for c in calls), calls
    # refusals, before any page is taken
    for kw, needle in ((dict(do_sample=False), "do_sample=False"), (dict(num_beams=2), "watermarking_config"),
                       (dict(do_sample=True, padded_batch=True), "padded_batch"), (dict(penalty_alpha=0.5, top_k=4), "watermarking_config")):
        with pytest.raises(NotImplementedError, match=needle):
            gen(watermarking_config=cfg, **kw)
    with pytest.raises(NotImplementedError, match="randperm"):
        gen(do_sample=True, watermarking_config=WatermarkingConfig())
    with pytest.raises(NotImplementedError, match="debug_mode"):
        gen(do_sample=True, watermarking_config=dict(cfg, debug_mode=True))
    with pytest.raises(ValueError, match="ngram_len"):
        gen(do_sample=True, watermarking_config=dict(cfg, ngram_len=1))
    with pytest.raises(NotImplementedError, match="greedy"):
        SamplingParams(watermarking_config=cfg)
    assert len(model.kv.free) == model.kv.num_pages
