"""sequence_bias / presence_penalty / frequency_penalty end to end on the tiny synthetic model (tests/allow_cases.py,
V = 512): generate() replayed on the host from its RETURNED raw logits through tests/bias_ref.py, greedy and sampled, with and without
a repetition penalty; rows of a batch against the same call on the row alone; the launches of a call; ServingEngine requests with a
LogitAdjust against their solo generate() while other requests join and leave, and the release of their device buffers; the refusals."""
import inspect

import numpy as np
import pytest
import torch

from tests import bias_ref as R
from tests.golden import cases as G
from tests.allow_cases import pack as _pack, solo as _solo, tiny_model

pytestmark = pytest.mark.gpu
TV = G.LLM["vocab_size"]
BIAS = {(40,): 1.5, (77,): -2.0, 130: 0.75, (511,): 1.0, (0,): -0.5}
BIAS_IDS = [k if isinstance(k, int) else k[0] for k in BIAS]
BIAS_VALS = list(BIAS.values())
PRES, FREQ = 2.0, 3.0


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
    """Two text prompts of 9 and 5 ids, right-padded, under an attention mask"""
    g = torch.Generator().manual_seed(95)
    rows = [[1] + torch.randint(3, TV, (8,), generator=g).tolist(), [1] + torch.randint(3, TV, (4,), generator=g).tolist()]
    L = max(len(r) for r in rows)
    ids = torch.tensor([r + [0] * (L - len(r)) for r in rows])
    mask = torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows])
    return ids.to(dev), mask.to(dev)


def _gen(model, ids, mask, n, **kw):
    return model.generate(ids, attention_mask=mask, max_new_tokens=n, eos_token_id=-1, pad_token_id=0, **kw)


def _host_rows(logits_st, prompts, gens, penalty, presence=PRES, frequency=FREQ):
    """The rows the sampler works on at one step, from the step's returned raw logits and what every row has generated so far"""
    out = []
    for r, raw in enumerate(logits_st):
        pre, post = R.bias_rows(TV, gens[r], BIAS_IDS, BIAS_VALS, presence, frequency)
        out.append(R.adjusted(raw, None, pre, post, penalty, [t for t in prompts[r] if t >= 0] + gens[r]))
    return np.stack(out)


def test_a_huge_bias_is_emitted_at_every_step(dev, model, batch):
    ids, mask = batch
    t, n = 77, 5
    plain = _gen(model, ids, mask, n)[:, ids.shape[1]:].cpu().tolist()
    assert all(row != [t] * n for row in plain)
    out = _gen(model, ids, mask, n, sequence_bias={(t,): 1e4})
    assert out[:, ids.shape[1]:].cpu().tolist() == [[t] * n] * 2 and torch.equal(out[:, :ids.shape[1]], ids)
    assert _gen(model, ids, mask, n, sequence_bias={t: 1e4})[:, ids.shape[1]:].cpu().tolist() == [[t] * n] * 2      # a bare int key
    assert len(model.kv.free) == model.kv.num_pages


@pytest.mark.parametrize("penalty", (1.0, 1.3))
def test_greedy_generate_replays_from_its_logits(dev, model, batch, penalty):
    """12 steps at B = 2 with ragged prompts: every emitted id is the first arg-max of bias_ref.adjusted on that step's RETURNED raw
    logits (the penalty history: the row's non-negative ids, then what it emitted; the counts: what it emitted). The replay without the
    two penalties picks differently somewhere (asserted: the penalties bite), and so does the plain call."""
    ids, mask = batch
    n = 12
    out, logits = _gen(model, ids, mask, n, sequence_bias=BIAS, presence_penalty=PRES, frequency_penalty=FREQ, repetition_penalty=penalty,
                       return_logits=True)
    new = out[:, ids.shape[1]:].cpu().tolist()
    assert len(logits) == n and all(len(r) == n for r in new)
    prompts = ids.cpu().tolist()
    gens, changed = [[], []], 0
    for st in range(n):
        raw = logits[st].float().cpu().numpy()
        x = _host_rows(raw, prompts, gens, penalty)
        x0 = _host_rows(raw, prompts, gens, penalty, 0.0, 0.0)
        for r in range(2):
            want = int(np.argmax(x[r]))
            assert new[r][st] == want, (penalty, r, st, new[r][st], want)
            changed += want != int(np.argmax(x0[r]))
            gens[r].append(want)
    print(f"penalty {penalty}: presence / frequency changed {changed} of {2 * n} picks")
    assert changed > 0
    plain = _gen(model, ids, mask, n, repetition_penalty=penalty)
    assert not torch.equal(plain, out)
    assert len(model.kv.free) == model.kv.num_pages


def test_sampled_generate_replays_through_the_existing_sampler(dev, model, batch):
    """do_sample with a seed: every step's ids equal ops.sample_rows (no adjust, penalty 1) on the host-adjusted rows with the call's
    seed, counter = step, stream = row."""
    from vitron_amd import ops
    ids, mask = batch
    n, seed, T, k, p = 8, 11, 0.8, 20, 0.9
    out, logits = _gen(model, ids, mask, n, do_sample=True, temperature=T, top_k=k, top_p=p, seed=seed, sequence_bias=BIAS,
                       presence_penalty=PRES, frequency_penalty=FREQ, repetition_penalty=1.2, return_logits=True)
    new = out[:, ids.shape[1]:].cpu().tolist()
    prompts = ids.cpu().tolist()
    gens = [[], []]
    for st in range(n):
        x = _host_rows(logits[st].float().cpu().numpy(), prompts, gens, 1.2)
        want = ops.sample_rows(torch.from_numpy(x).to(dev), _pack([(T, k, p, 1.0, seed, st, b, 0, 0) for b in range(2)], dev)).cpu().tolist()
        assert [new[0][st], new[1][st]] == want, (st, new, want)
        for r in range(2):
            gens[r].append(want[r])
    assert len(model.kv.free) == model.kv.num_pages


@pytest.mark.parametrize("kw", (dict(presence_penalty=PRES, frequency_penalty=FREQ), dict(sequence_bias=BIAS),
                                dict(sequence_bias=BIAS, frequency_penalty=-FREQ, repetition_penalty=1.3, no_repeat_ngram_size=2)),
                         ids=("penalties", "bias", "everything"))
def test_rows_of_a_batch_equal_the_rows_alone(dev, model, batch, kw):
    ids, mask = batch
    out = _gen(model, ids, mask, 6, **kw)
    for b in range(2):
        alone = _gen(model, ids[b:b + 1], mask[b:b + 1], 6, **kw)
        assert torch.equal(alone[0], out[b]), (b, alone[0].tolist(), out[b].tolist())
    assert len(model.kv.free) == model.kv.num_pages


# ---- the launches ---------------------------------------------------------------------------------------------------------------------------
PICKS = ("argmax", "sample_top_p", "sample_rows", "ban_rows", "bias_rows", "beam_step")


@pytest.fixture
def calls(monkeypatch):
    """Recorders around the pick launches that call through: the names in launch order; a sampler launch is noted as
    ("sample_rows", were adjust pointers given)."""
    from vitron_amd import ops
    seen = []

    def wrap(name):
        real = getattr(ops, name)
        sig = inspect.signature(real)

        def recorder(*a, **kw):
            if name == "sample_rows":
                given = sig.bind(*a, **kw).arguments
                seen.append((name, given.get("_adjust_ptrs") is not None or given.get("adjust") is not None))
            else:
                seen.append(name)
            return real(*a, **kw)
        return recorder
    for name in PICKS:
        monkeypatch.setattr(ops, name, wrap(name))
    return seen


def test_launches(model, batch, calls):
    ids, mask = batch
    n = 3
    ADJ, PLAIN = ("sample_rows", True), ("sample_rows", False)
    _gen(model, ids, mask, n, presence_penalty=0.5)
    assert calls == ["bias_rows", ADJ] * n, calls                                 # with a penalty: one bias_rows + one sample_rows per step
    del calls[:]
    _gen(model, ids, mask, n, sequence_bias=BIAS, frequency_penalty=0.5, no_repeat_ngram_size=2)
    assert calls == ["ban_rows", "bias_rows", ADJ] * n, calls
    del calls[:]
    _gen(model, ids, mask, n, sequence_bias=BIAS)
    assert calls == ["bias_rows"] + [ADJ] * n, calls                              # bias only: one bias_rows in total, before step 0
    del calls[:]
    _gen(model, ids, mask, n, sequence_bias={}, presence_penalty=0.0, frequency_penalty=0.0)
    assert calls == ["argmax"] * n, calls                                         # the arguments off: the launches of a plain call
    del calls[:]
    _gen(model, ids, mask, n, repetition_penalty=1.3, sequence_bias=None)
    assert calls == [PLAIN] * n, calls
    del calls[:]
    assert torch.equal(_gen(model, ids, mask, 0, sequence_bias=BIAS, presence_penalty=1.0), ids) and calls == []
    assert len(model.kv.free) == model.kv.num_pages


# ---- ServingEngine --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reqs(dev):
    g = torch.Generator().manual_seed(96)
    rnd = lambda n: torch.randint(3, TV, (n,), generator=g).tolist()                    # noqa: E731
    return [dict(input_ids=torch.tensor([[1] + rnd(11)]), images=None, regions=None, max_new_tokens=10),
            dict(input_ids=torch.tensor([[1] + rnd(19)]), images=None, regions=None, max_new_tokens=8),
            dict(input_ids=torch.tensor([[1] + rnd(30)]), images=None, regions=None, max_new_tokens=6)]


def _submit(eng, r, sp=None, adjust=None):
    return eng.submit(r["input_ids"], r["images"], r["regions"], r["max_new_tokens"], eos_token_id=-1, sampling=sp, adjust=adjust)


def _adjust_kw(adj):
    return dict(sequence_bias={(t,): v for t, v in adj.bias} or None, presence_penalty=adj.presence_penalty, frequency_penalty=adj.frequency_penalty)


def test_engine_requests_equal_their_solo_generate(dev, model, reqs):
    """Four requests with an adjustment -- greedy without SamplingParams (its legacy row parameters), greedy with, sampled with a
    repetition penalty, bias only -- and two neighbours without one (greedy legacy, sampled) join and leave at different steps: every
    one returns the tokens of its own solo generate()."""
    from vitron_amd.sampling import LogitAdjust, SamplingParams
    from vitron_amd.serving import ServingEngine
    full = LogitAdjust({40: 8.0, 300: 8.0, 77: -2.0}, PRES, FREQ)      # two boosted ids that the penalties push down again once emitted
    pen_only = LogitAdjust(None, -30.0, -1.0)                          # negative penalties: whatever was emitted once comes again
    bias_only = LogitAdjust({40: 30.0, 300: 30.0})
    greedy, sampled = SamplingParams(), SamplingParams(temperature=0.8, seed=5, repetition_penalty=1.2)
    nb = SamplingParams(temperature=0.9, seed=7)
    want = {"legacy": _solo(model, dev, reqs[0], greedy, **_adjust_kw(full)),
            "greedy": _solo(model, dev, reqs[1], greedy, **_adjust_kw(pen_only)),
            "sampled": _solo(model, dev, reqs[0], sampled, **_adjust_kw(full)),
            "bias": _solo(model, dev, reqs[2], greedy, **_adjust_kw(bias_only)),
            "plain": _solo(model, dev, reqs[1], greedy), "nb": _solo(model, dev, reqs[2], nb)}
    assert want["legacy"] != _solo(model, dev, reqs[0], greedy) and want["greedy"] != want["plain"]        # the adjustments bite
    assert want["bias"] != _solo(model, dev, reqs[2], greedy) and set(want["bias"]) <= {40, 300}
    assert want["greedy"] == want["plain"][:1] * reqs[1]["max_new_tokens"] and {40, 300} & set(want["legacy"])
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    rid = {"plain": _submit(eng, reqs[1])}
    seen, steps = {}, 0
    while eng.pending():
        if steps == 1:
            rid["legacy"] = _submit(eng, reqs[0], None, full)
            rid["nb"] = _submit(eng, reqs[2], nb)
        if steps == 3:
            rid["sampled"] = _submit(eng, reqs[0], sampled, full)
            rid["greedy"] = _submit(eng, reqs[1], greedy, pen_only)
            rid["bias"] = _submit(eng, reqs[2], greedy, bias_only)
        for i, t in eng.step():
            seen.setdefault(i, []).append(t)
        if steps == 2:
            live = [q for q in eng.active if q.rid == rid["legacy"]][0]
            assert live.adj_buf is not None and live.adj_buf.shape == (TV, 2) and live.gen is not None and live.adj_ids is not None
            assert live.sampling is None and live.hist is None
        steps += 1
        assert steps < 100
    assert not eng.failed
    for name, r in rid.items():
        assert seen[r] == want[name], (name, seen[r], want[name])
        q = eng.finished[r]
        assert q.adj_buf is None and q.adj_ids is None and q.adj_vals is None and q.gen is None and q.hist is None
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_launches_and_releases(dev, model, reqs, calls):
    """One bias_rows launch per pick while a request with penalties is active, one in total for a bias-only request, none without an
    adjustment; the buffers go where `hist` goes: on retirement, when the request fails on its own and on cancel."""
    from vitron_amd.sampling import LogitAdjust, SamplingParams
    from vitron_amd.serving import ServingEngine
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    a = _submit(eng, reqs[2], None, LogitAdjust({40: 6.0}))
    eng.run()
    assert calls.count("bias_rows") == 1 and calls.count(("sample_rows", True)) == reqs[2]["max_new_tokens"], calls
    del calls[:]
    _submit(eng, reqs[2])
    eng.run()
    assert calls == ["argmax"] * reqs[2]["max_new_tokens"], calls                 # no adjustment anywhere: the launches of before
    del calls[:]
    failing = SamplingParams(allowed_tokens_fn=lambda toks: [] if len(toks) == 2 else None)
    adj = LogitAdjust({40: 6.0}, 0.5, 0.5)
    ok = _submit(eng, reqs[0], None, adj)
    bad = _submit(eng, reqs[1], failing, adj)
    waiting = _submit(eng, reqs[2], None, adj)                                    # max_batch 2: it waits
    eng.step()
    live = {q.rid: q for q in eng.active}
    assert all(live[r].adj_buf is not None and live[r].gen is not None for r in (ok, bad))
    eng.step()                                                                    # the second token is out: `bad` fails here, alone
    assert bad in eng.failed and [q.rid for q in eng.active] == [ok]
    held = [q for q in eng.waiting if q.rid == waiting][0]
    assert eng.cancel(waiting) and held.adj_buf is None and held.gen is None
    out = eng.run()
    for q in (eng.failed[bad], eng.finished[ok]):
        assert q.adj_buf is None and q.adj_ids is None and q.adj_vals is None and q.gen is None
    assert isinstance(eng.failed[bad].error, ValueError) and len(eng.failed[bad].tokens) == 2
    n_picks = calls.count(("sample_rows", True))
    assert calls.count("bias_rows") == n_picks and n_picks >= reqs[0]["max_new_tokens"] - 1
    assert out[ok].tolist() == _solo(model, dev, reqs[0], SamplingParams(), **_adjust_kw(adj))
    assert waiting not in out and len(model.kv.free) == model.kv.num_pages


def test_refusals(dev, model, batch):
    ids, mask = batch
    one = ids[:1, :5]
    with pytest.raises(NotImplementedError, match=r"\(40, 41\)"):
        model.generate(one, max_new_tokens=2, sequence_bias={(40, 41): 1.0})
    for kw, name in ((dict(sequence_bias={(40,): 1.0}), "sequence_bias"), (dict(presence_penalty=0.5), "presence_penalty"),
                     (dict(frequency_penalty=0.5), "frequency_penalty")):
        with pytest.raises(NotImplementedError, match=name):
            model.generate(one, max_new_tokens=2, num_beams=2, **kw)
        with pytest.raises(NotImplementedError, match=name):
            model.generate(ids, attention_mask=mask, max_new_tokens=2, padded_batch=True, **kw)
    for bad in ({(TV,): 1.0}, {-1: 1.0}, {(40,): float("nan")}, {40: float("inf")}, {40: 1.0, (40,): 2.0}):
        with pytest.raises(ValueError, match="sequence_bias"):
            model.generate(one, max_new_tokens=2, sequence_bias=bad)
    with pytest.raises(ValueError, match="presence_penalty"):
        model.generate(one, max_new_tokens=2, presence_penalty=float("nan"))
    assert len(model.kv.free) == model.kv.num_pages
