"""min_p / typical_p / epsilon_cutoff / eta_cutoff end to end on the tiny synthetic model (tests/allow_cases.py, V = 512):
generate(do_sample=True, ...) against a ServingEngine request with the same SamplingParams, alone and while other requests join and
leave; every emitted id against the fp64 keep-set of its step, the parameters placed per step on the RETURNED raw logits through
tests/trunc_ref.py (steps that cannot be placed are excluded, and their share is asserted to stay under 10 %); the launches; the
refusals."""
import inspect

import numpy as np
import pytest
import torch

from tests import trunc_ref as R
from tests.golden import cases as G
from tests.allow_cases import solo as _solo, submit as _submit, tiny_model

pytestmark = pytest.mark.gpu
TV = G.LLM["vocab_size"]
# one setting per stage, and all four
KW = dict(min_p=dict(min_p=0.08), typical=dict(typical_p=0.6), epsilon=dict(epsilon_cutoff=4e-3), eta=dict(eta_cutoff=6e-3),
          all=dict(min_p=0.03, typical_p=0.9, epsilon_cutoff=2.5e-3, eta_cutoff=3e-3))


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return tiny_model(dev)


@pytest.fixture(scope="module")
def reqs(dev):
    g = torch.Generator().manual_seed(97)
    rnd = lambda n: torch.randint(3, TV, (n,), generator=g).tolist()                    # noqa: E731
    return [dict(input_ids=torch.tensor([[1] + rnd(11)]), images=None, regions=None, max_new_tokens=10),
            dict(input_ids=torch.tensor([[1] + rnd(19)]), images=None, regions=None, max_new_tokens=8),
            dict(input_ids=torch.tensor([[1] + rnd(30)]), images=None, regions=None, max_new_tokens=6)]


def _sp(name, **kw):
    from vitron_amd.sampling import SamplingParams
    return SamplingParams(temperature=1.4, top_k=0, top_p=0.98, seed=5, **KW[name], **kw)


def test_engine_requests_equal_their_solo_generate(dev, model, reqs):
    """One request per stage and one with all four, each alone in an engine and then all together with a greedy legacy request and a
    sampled request without truncation joining and leaving at different steps: every one returns the tokens of its solo generate()."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    nb = SamplingParams(temperature=0.9, seed=7)
    plan = {name: (reqs[i % 3], _sp(name, repetition_penalty=1.2 if name == "all" else 1.0)) for i, name in enumerate(KW)}
    want = {name: _solo(model, dev, r, sp, **KW[name]) for name, (r, sp) in plan.items()}
    want["plain"] = _solo(model, dev, reqs[1], SamplingParams())
    want["nb"] = _solo(model, dev, reqs[2], nb)
    bare = {name: _solo(model, dev, r, sp) for name, (r, sp) in plan.items()}          # the same calls without the stages
    assert sum(want[name] != bare[name] for name in plan) >= 3, (want, bare)           # the stages bite
    for name, (r, sp) in plan.items():                                                 # alone
        eng = ServingEngine(model, max_batch=2, kv_pages=64)
        rid = _submit(eng, r, sp)
        assert eng.run()[rid].cpu().tolist()[-r["max_new_tokens"]:] == want[name], name
    eng = ServingEngine(model, max_batch=4, kv_pages=64)                               # joining and leaving
    rid = {"plain": _submit(eng, reqs[1])}
    seen, steps = {}, 0
    names = list(plan)
    while eng.pending():
        if steps == 1:
            rid[names[0]] = _submit(eng, *plan[names[0]])
            rid["nb"] = _submit(eng, reqs[2], nb)
        if steps == 3:
            for name in names[1:4]:
                rid[name] = _submit(eng, *plan[name])
        if steps == 6:
            rid[names[4]] = _submit(eng, *plan[names[4]])
        for i, t in eng.step():
            seen.setdefault(i, []).append(t)
        steps += 1
        assert steps < 100
    assert not eng.failed and set(rid) == set(want)
    for name, r in rid.items():
        assert seen[r] == want[name], (name, seen[r], want[name])
    assert len(model.kv.free) == model.kv.num_pages


def _draw(g, combo):
    """Drawn parameters for a row of this model: after top_k = 40 its q are nearly flat (about 1 / 40 each, within a factor 2), so the
    draws cover THAT range of q / q_max (min_p), q (epsilon) and sqrt(eta) * exp(-entropy) (eta) -- each draw then meets another gap."""
    drawn = (float(g.uniform(0.3, 0.95)), float(g.uniform(0.2, 0.9)), float(g.uniform(0.01, 0.04)), float(g.uniform(0.2, 0.95)))
    return tuple(drawn[i] if i in combo else R.OFF[i] for i in range(4))


def test_emitted_ids_lie_in_the_fp64_keep_set_of_their_step(dev, model, reqs):
    """Six steps per stage setting (each stage alone, all four), one generate() call per step so that the parameters can be PLACED for
    that step: the step's raw logits come from a return_logits call on the same ids, tests/trunc_ref.py places drawn parameters in the
    middle of a gap of that row (up to 8 draws; fp64 margin >= 1e-3, the top-p step >= 1e-4 of the mass from another keep-set), and the
    sampled call with the placed parameters must emit a survivor of the fp64 chain. The emitted id extends the prompt of the next step.
    A step that cannot be placed is excluded; at most 10 % of all steps may be."""
    g = np.random.default_rng(5)
    T, k, p, steps = 1.0, 40, 0.95, 6
    total = excluded = shrunk = 0
    for combo in ((0,), (1,), (2,), (3,), (0, 1, 2, 3)):
        ids = reqs[0]["input_ids"].to(dev)
        for st in range(steps):
            total += 1
            _, logits = model.generate(ids, max_new_tokens=1, eos_token_id=-1, return_logits=True)
            s = R.scaled(logits[0][0].float().cpu().numpy(), T)
            A0 = R.base_keep(s, k, p)
            got = None
            if R.top_p_margin(s, k, p) >= 1e-4:
                for _ in range(8):
                    got = R.place(s, A0, _draw(g, combo))
                    if got is not None:
                        break
            trunc, A = got if got is not None else (R.OFF, A0)
            kw = {name: trunc[i] for i, name in enumerate(R.STAGES) if i in combo and got is not None}
            out = model.generate(ids, max_new_tokens=1, eos_token_id=-1, do_sample=True, temperature=T, top_k=k, top_p=p, seed=21 + st, **kw)
            tok = int(out[0, -1])
            print(f"stages {combo} step {st}: trunc {trunc} kept {int(A.sum())} of {int(A0.sum())} emitted {tok} placed {got is not None}")
            if got is None:
                excluded += 1
            else:
                shrunk += int(A.sum() < A0.sum())
                assert A[tok], (combo, st, tok, trunc, int(A.sum()), int(A0.sum()))
            ids = out
    print(f"steps {total}, excluded {excluded} ({excluded / total:.1%}), steps where the stages removed something {shrunk}")
    assert total == 5 * steps and excluded <= 0.10 * total, (excluded, total)
    assert shrunk >= total // 2
    assert len(model.kv.free) == model.kv.num_pages


@pytest.fixture
def calls(monkeypatch):
    """Recorders around the pick launches that call through: the names in launch order; a sampler launch is noted as
    ("sample_rows", was trunc given)."""
    from vitron_amd import ops
    seen = []

    def wrap(name):
        real = getattr(ops, name)
        sig = inspect.signature(real)

        def recorder(*a, **kw):
            seen.append((name, sig.bind(*a, **kw).arguments.get("trunc") is not None) if name == "sample_rows" else name)
            return real(*a, **kw)
        return recorder
    for name in ("argmax", "sample_top_p", "sample_rows", "ban_rows", "bias_rows", "beam_step"):
        monkeypatch.setattr(ops, name, wrap(name))
    return seen


def test_launches_and_refusals(dev, model, reqs, calls):
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    ids = reqs[0]["input_ids"].to(dev)
    n = 3
    gen = lambda **kw: model.generate(ids, max_new_tokens=n, eos_token_id=-1, **kw)[0, ids.shape[1]:].cpu().tolist()     # noqa: E731
    TRUNC, PLAIN = ("sample_rows", True), ("sample_rows", False)
    gen(do_sample=True, seed=3, min_p=0.1)
    assert calls == [TRUNC] * n, calls                                             # one vt_sample_rows_trunc launch per step
    del calls[:]
    gen(do_sample=True, seed=3, typical_p=0.9, eta_cutoff=1e-3, repetition_penalty=1.2, no_repeat_ngram_size=2)
    assert calls == ["ban_rows", TRUNC] * n, calls
    del calls[:]
    off = gen(do_sample=True, seed=3, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    assert calls == ["sample_top_p"] * n and off == gen(do_sample=True, seed=3), calls       # the arguments off: a plain sampling call
    del calls[:]
    greedy = gen(min_p=0.5, typical_p=0.2, epsilon_cutoff=0.1, eta_cutoff=0.1)
    assert calls == ["argmax"] * n and greedy == gen(), calls                      # ignored without do_sample
    del calls[:]
    # the engine: no truncated request -> the launches it always made; one truncated request -> ONE trunc launch for all rows
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    _submit(eng, reqs[1], SamplingParams(temperature=0.9, seed=7))
    _submit(eng, reqs[2], SamplingParams(min_p=0.5))                               # greedy: not truncated
    eng.run()
    assert calls and all(c == PLAIN for c in calls), calls
    del calls[:]
    _submit(eng, reqs[1], SamplingParams(temperature=0.9, seed=7, epsilon_cutoff=1e-3))
    _submit(eng, reqs[2])
    eng.run()
    assert TRUNC in calls and all(c in (TRUNC, "argmax") for c in calls), calls
    assert calls.count(TRUNC) == reqs[1]["max_new_tokens"]
    # refusals
    for kw in KW.values():
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            gen(num_beams=2, **kw)
        with pytest.raises(NotImplementedError, match="padded_batch"):
            gen(do_sample=True, seed=3, padded_batch=True, **kw)
    for bad in (dict(min_p=1.5), dict(typical_p=0.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            gen(do_sample=True, seed=3, **bad)
    assert len(model.kv.free) == model.kv.num_pages
