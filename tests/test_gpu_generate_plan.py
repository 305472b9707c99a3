"""The launch plan of generate() (its docstring's promises) on the tiny synthetic model (tests/allow_cases.py): which
of ops.argmax / sample_top_p / sample_rows / ban_rows / beam_step a call launches per step, in which order, and whether the sampler got
allow pointers -- for the defaults, sampling, a penalty, log-probabilities, a static constraint, an n-gram ban and beams. The batch is
two text prompts of 5 and 9 ids under an attention mask: the smallest case in which a row / step mix-up in the per-step row arrays, the
pointer arrays or the device histories changes a row's ids, so every mode whose draws are per-row reproducible must also return for each
row the ids of the same call on that row alone."""
import inspect

import pytest
import torch

from tests.allow_cases import tiny_model

pytestmark = pytest.mark.gpu
PICKS = ("argmax", "sample_top_p", "sample_rows", "ban_rows", "beam_step")
NEW = 3


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return tiny_model(dev)


@pytest.fixture(scope="module")
def batch(dev):
    rows = [[1, 40, 41, 42, 40], [1, 7, 300, 7, 300, 7, 150, 9, 7]]
    L = max(len(r) for r in rows)
    ids = torch.tensor([r + [0] * (L - len(r)) for r in rows]).to(dev)
    mask = torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows]).to(dev)
    return ids, mask


@pytest.fixture
def calls(monkeypatch):
    """Recorders around the five pick launches that call through: the names in launch order; a sampler launch is noted as
    ("sample_rows", were allow masks given)."""
    from vitron_amd import ops
    seen = []

    def wrap(name):
        real = getattr(ops, name)
        sig = inspect.signature(real)

        def recorder(*a, **kw):
            if name == "sample_rows":
                given = sig.bind(*a, **kw).arguments
                seen.append((name, given.get("_allow_ptrs") is not None or given.get("allow") is not None))
            else:
                seen.append(name)
            return real(*a, **kw)
        return recorder
    for name in PICKS:
        monkeypatch.setattr(ops, name, wrap(name))
    return seen


def _gen(model, ids, mask, n=NEW, **kw):
    return model.generate(ids, attention_mask=mask, max_new_tokens=n, eos_token_id=-1, pad_token_id=0, **kw)


PLAIN, MASKED = ("sample_rows", False), ("sample_rows", True)
MODES = [
    # (name, arguments, the launches of one step, are the draws per-row reproducible)
    ("defaults", {}, ["argmax"], True),
    ("sampled", dict(do_sample=True, seed=1), ["sample_top_p"], False),
    ("penalty", dict(repetition_penalty=1.3), [PLAIN], True),
    ("logprobs", dict(return_logprobs=True), [PLAIN], False),
    ("suppress", dict(suppress_tokens=[4]), [MASKED], True),
    ("ngram", dict(no_repeat_ngram_size=2), ["ban_rows", MASKED], True),
]


@pytest.mark.parametrize("name,kw,per_step,per_row", MODES, ids=[m[0] for m in MODES])
def test_launches_per_step_and_rows_alone(model, batch, calls, name, kw, per_step, per_row):
    ids, mask = batch
    out = _gen(model, ids, mask, **kw)
    assert calls == per_step * NEW, calls
    if name == "logprobs":
        out, lps = out
        assert lps.shape == (2, NEW) and lps.dtype == torch.float32 and bool((lps <= 0).all())
    assert out.shape == (2, ids.shape[1] + NEW) and torch.equal(out[:, :ids.shape[1]], ids)
    if per_row:
        for b in range(2):
            alone = _gen(model, ids[b:b + 1], mask[b:b + 1], **kw)
            assert torch.equal(alone[0], out[b]), (name, b, alone[0].tolist(), out[b].tolist())
        assert calls == per_step * NEW * 3, calls
    assert len(model.kv.free) == model.kv.num_pages


def test_beams_launch_beam_step_only(model, batch, calls):
    ids, mask = batch
    out = _gen(model, ids, mask, num_beams=2)
    assert calls and set(calls) == {"beam_step"}, calls
    assert len(calls) == model.last_generate_stats["beam_steps"]
    assert out.shape[0] == 2 and torch.equal(out[:, :ids.shape[1]], ids)
    assert len(model.kv.free) == model.kv.num_pages


def test_one_token_and_no_token(model, batch, calls):
    """max_new_tokens=1 is the call without a decode state (one pick, read back at once); max_new_tokens=0 returns the prompt and picks
    nothing."""
    ids, mask = batch
    one = _gen(model, ids, mask, n=1)
    assert calls == ["argmax"] and one.shape == (2, ids.shape[1] + 1)
    assert torch.equal(one, _gen(model, ids, mask)[:, :ids.shape[1] + 1])
    del calls[:]
    assert torch.equal(_gen(model, ids, mask, n=0), ids) and calls == []
    assert torch.equal(_gen(model, ids, mask, n=0, no_repeat_ngram_size=2, repetition_penalty=1.3), ids) and calls == []
    assert len(model.kv.free) == model.kv.num_pages
