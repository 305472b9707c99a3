"""mirostat_tau end to end on the tiny synthetic model (tests/allow_cases.py, V = 512): generate(mirostat_tau=,
return_logits=True) against a loop the test drives itself with ops.sample_rows(miro=) over the returned rows, id for id, plain and with
repetition_penalty, min_p and no_repeat_ngram_size in front; last_generate_stats["mirostat"] against that loop's cell; a ServingEngine
request against its solo generate while neighbours (one of them on Mirostat with other parameters) join, leave and are cancelled; the
release of the cell on every exit path; the launches; the refusals through generate and submit."""
import inspect

import numpy as np
import pytest
import torch

from tests.golden import cases as G
from tests.allow_cases import solo as _solo, submit as _submit, tiny_model

pytestmark = pytest.mark.gpu
TV = G.LLM["vocab_size"]
NEW, SEED, TAU, ETA = 32, 23, 3.0, 0.2


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
    g = torch.Generator().manual_seed(137)
    rnd = lambda n: torch.randint(3, TV, (n,), generator=g).tolist()                    # noqa: E731
    return [dict(input_ids=torch.tensor([[1] + rnd(13)]), images=None, regions=None, max_new_tokens=NEW),
            dict(input_ids=torch.tensor([[1] + rnd(21)]), images=None, regions=None, max_new_tokens=5),
            dict(input_ids=torch.tensor([[1] + rnd(9)]), images=None, regions=None, max_new_tokens=11)]


def _drive(dev, prompt, rows, T, top_k, tau, eta, seed, penalty=1.0, min_p=0.0, ngram=0):
    """The test's own loop over the returned rows [steps, V]: one ops.sample_rows(miro=) per step on a cell of its own, with the
    history, the n-gram mask and the truncation entry built here from the ids it has drawn. Returns (ids, the cell as two floats)."""
    from vitron_amd import ops
    from vitron_amd.sampling import allow_mask, history_bans, new_miro_cell, pack_miro_rows, pack_sample_rows, pack_trunc_rows
    cell = new_miro_cell(tau, dev)
    miro = pack_miro_rows([(cell, tau, eta)], dev)
    trunc = pack_trunc_rows([(min_p, 1.0, 0.0, 0.0)], dev) if min_p > 0 else None
    hist, out = list(prompt), []
    for st in range(rows.shape[0]):
        h = torch.tensor(hist, dtype=torch.int32, device=dev)
        params = pack_sample_rows([(T, top_k, 1.0, penalty, seed, st, 0, h.data_ptr() if penalty != 1.0 else 0, len(hist) if penalty != 1.0 else 0)], dev)
        allow = None
        if ngram:
            allow = [torch.from_numpy(allow_mask(TV, None, history_bans(TV, hist, ngram)).view(np.int32)).to(dev)]
        tok = int(ops.sample_rows(rows[st:st + 1].contiguous(), params, allow=allow, trunc=trunc, miro=miro)[0])
        out.append(tok)
        hist.append(tok)
    return out, tuple(float(v) for v in cell.cpu().tolist())


@pytest.mark.parametrize("front", [dict(), dict(repetition_penalty=1.3, min_p=0.05, no_repeat_ngram_size=2)])
def test_generate_equals_a_loop_over_its_own_rows(dev, model, reqs, front):
    ids = reqs[0]["input_ids"].to(dev)
    kw = dict(max_new_tokens=NEW, eos_token_id=-1, do_sample=True, temperature=1.1, top_k=40, top_p=1.0, seed=SEED)
    out, rows = model.generate(ids, return_logits=True, mirostat_tau=TAU, mirostat_eta=ETA, **kw, **front)
    stats = dict(model.last_generate_stats["mirostat"])
    got = out[0, ids.shape[1]:].cpu().tolist()
    rows = torch.stack(rows)[:, 0].float()
    assert len(got) == NEW and rows.shape == (NEW, TV)
    want, cell = _drive(dev, ids[0].cpu().tolist(), rows, 1.1, 40, TAU, ETA, SEED, penalty=front.get("repetition_penalty", 1.0),
                        min_p=front.get("min_p", 0.0), ngram=front.get("no_repeat_ngram_size", 0))
    print(f"front {front}: ids {got}\n mirostat {stats}, the loop's cell {cell}")
    assert got == want
    assert (np.float32(stats["mu"][0]), np.float32(stats["surprise"][0])) == (np.float32(cell[0]), np.float32(cell[1]))
    assert len(stats["mu"]) == 1 and cell[0] != 2 * TAU and cell[1] >= 0.0
    plain = model.generate(ids, **kw, **front)[0, ids.shape[1]:].cpu().tolist()
    assert "mirostat" not in model.last_generate_stats
    assert plain != got                                                                   # the cutoff moved the draws
    assert model.generate(ids, mirostat_tau=0, **kw, **front)[0, ids.shape[1]:].cpu().tolist() == plain
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_request_equals_its_solo_generate(dev, model, reqs):
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    sp = SamplingParams(temperature=1.1, top_k=40, top_p=1.0, seed=SEED, mirostat_tau=TAU, mirostat_eta=ETA)
    other = SamplingParams(temperature=0.8, top_k=20, seed=5, mirostat_tau=4.5, mirostat_eta=0.05)
    plain = SamplingParams(temperature=0.9, top_k=8, seed=7)
    solo_a = _solo(model, dev, reqs[0], sp, mirostat_tau=TAU, mirostat_eta=ETA)
    state_a = model.last_generate_stats["mirostat"]
    solo_c = _solo(model, dev, reqs[2], other, mirostat_tau=4.5, mirostat_eta=0.05)
    state_c = model.last_generate_stats["mirostat"]
    # two neighbours join and leave: max_batch = 2, so c (on Mirostat with other parameters) joins when b (plain, short) has left
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    a, b, c = _submit(eng, reqs[0], sp), _submit(eng, reqs[1], plain), _submit(eng, reqs[2], other)
    assert eng.mirostat_state(a) is None                                                  # not picked yet
    eng.step()
    eng.step()
    mid = eng.mirostat_state(a)
    assert mid is not None and len(mid) == 2 and mid[0] != 2 * TAU and eng.mirostat_state(b) is None
    cell_a = [r for r in eng.active if r.rid == a][0].miro_cell
    assert cell_a is not None and cell_a.numel() == 2
    out = eng.run()
    assert not eng.failed
    assert out[a].cpu().tolist()[-NEW:] == solo_a
    assert out[c].cpu().tolist()[-reqs[2]["max_new_tokens"]:] == solo_c
    for rid, st in ((a, state_a), (c, state_c)):
        got = eng.mirostat_state(rid)
        assert (np.float32(got[0]), np.float32(got[1])) == (np.float32(st["mu"][0]), np.float32(st["surprise"][0])), (rid, got, st)
        assert eng.finished[rid].miro_cell is None                                        # released at retirement
    assert eng.mirostat_state(b) is None and eng.finished[b].miro_cell is None and eng.mirostat_state(12345) is None
    # after the cancel of a neighbour
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    a, b, c = _submit(eng, reqs[0], sp), _submit(eng, reqs[1], plain), _submit(eng, reqs[2], other)
    eng.step()
    assert eng.cancel(c) and eng.mirostat_state(c) is None
    out = eng.run()
    assert out[a].cpu().tolist()[-NEW:] == solo_a and c not in out
    # a request that fails on its own gives its cell back too
    def boom(tokens):
        if len(tokens) >= 2:
            raise RuntimeError("the request's own constraint fails")
        return None
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    a, f = _submit(eng, reqs[0], sp), _submit(eng, reqs[2], other.replace(allowed_tokens_fn=boom))
    out = eng.run()
    assert f in eng.failed and eng.failed[f].miro_cell is None and eng.mirostat_state(f) is None
    assert out[a].cpu().tolist()[-NEW:] == solo_a
    assert len(model.kv.free) == model.kv.num_pages


def test_a_mirostat_request_beside_a_watermarked_one(dev, model, reqs):
    """No kernel carries both arrays: a step in which both kinds are active is two launches, and each request equals its solo generate --
    with a plain neighbour that asks for log-probabilities, and while the kinds join and leave"""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    cfg = dict(ngram_len=5, keys=[654, 400, 836, 123, 340, 443, 597, 160, 57], context_history_size=64)
    miro = SamplingParams(temperature=1.1, top_k=40, top_p=1.0, seed=SEED, mirostat_tau=TAU, mirostat_eta=ETA, logprobs=True)
    mark = SamplingParams(temperature=1.0, top_k=8, top_p=1.0, seed=17, watermarking_config=cfg)
    plain = SamplingParams(temperature=0.9, top_k=8, seed=7, logprobs=True)
    solo_m = _solo(model, dev, reqs[0], miro, mirostat_tau=TAU, mirostat_eta=ETA)
    state_m = model.last_generate_stats["mirostat"]
    solo_w = _solo(model, dev, reqs[2], mark, watermarking_config=cfg)
    solo_p = _solo(model, dev, reqs[1], plain)
    assert solo_w != _solo(model, dev, reqs[2], mark.replace(watermarking_config=None))             # the tournament moves this reply
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    alone = _submit(eng, reqs[0], miro)
    lp_alone = (eng.run(), eng.logprobs(alone).tolist())[1]
    for order in ((0, 2, 1), (2, 1, 0)):
        eng = ServingEngine(model, max_batch=3, kv_pages=64)
        sps = {0: miro, 1: plain, 2: mark}
        rid = {i: _submit(eng, reqs[i], sps[i]) for i in order}
        out = eng.run()
        assert not eng.failed, {k: v.error for k, v in eng.failed.items()}
        assert out[rid[0]].tolist()[-NEW:] == solo_m
        assert out[rid[2]].tolist()[-reqs[2]["max_new_tokens"]:] == solo_w
        assert out[rid[1]].tolist()[-reqs[1]["max_new_tokens"]:] == solo_p
        got = eng.mirostat_state(rid[0])
        assert (np.float32(got[0]), np.float32(got[1])) == (np.float32(state_m["mu"][0]), np.float32(state_m["surprise"][0]))
        # (the ids are exact; a decode row's logits may differ in the last bits with the batch's size, so the log-probabilities are close)
        assert np.allclose(eng.logprobs(rid[0]).numpy(), np.asarray(lp_alone, np.float32), atol=2e-3)
        assert len(eng.logprobs(rid[1])) == reqs[1]["max_new_tokens"]
        assert eng.finished[rid[0]].miro_cell is None and eng.finished[rid[2]].wm_cell is None
    # max_batch = 2: the watermarked request joins the Mirostat one when the plain one has left
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    a, b, c = _submit(eng, reqs[0], miro), _submit(eng, reqs[1], plain), _submit(eng, reqs[2], mark)
    out = eng.run()
    assert not eng.failed and out[a].tolist()[-NEW:] == solo_m and out[c].tolist()[-reqs[2]["max_new_tokens"]:] == solo_w
    assert len(model.kv.free) == model.kv.num_pages


@pytest.fixture
def calls(monkeypatch):
    """Recorders around the pick launches that call through: the names in launch order; a sampler launch is noted as
    ("sample_rows", was miro given)."""
    from vitron_amd import ops
    seen = []

    def wrap(name):
        real = getattr(ops, name)
        sig = inspect.signature(real)

        def recorder(*a, **kw):
            seen.append((name, sig.bind(*a, **kw).arguments.get("miro") is not None) if name == "sample_rows" else name)
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
    MIRO, PLAIN = ("sample_rows", True), ("sample_rows", False)
    plain = gen(do_sample=True, seed=3)
    assert calls == ["sample_top_p"] * n, calls                                    # without the argument: the launches it always ran
    del calls[:]
    assert gen(do_sample=True, seed=3, mirostat_tau=None, mirostat_eta=0.3) == plain and calls == ["sample_top_p"] * n
    del calls[:]
    gen(do_sample=True, seed=3, mirostat_tau=4.0)
    assert calls == [MIRO] * n, calls                                              # exactly one vt_sample_rows_miro launch per step
    del calls[:]
    gen(do_sample=True, seed=3, mirostat_tau=4.0, min_p=0.05, repetition_penalty=1.2, no_repeat_ngram_size=2, sequence_bias={(5,): 1.0},
        presence_penalty=0.2)
    assert calls == ["ban_rows", "bias_rows", MIRO] * n, calls                     # behind everything in front of the sampler
    del calls[:]
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    _submit(eng, reqs[1], SamplingParams(temperature=0.9, seed=7))
    eng.run()
    assert calls and all(c == PLAIN for c in calls), calls                         # no Mirostat request: what it launched before
    del calls[:]
    # refusals, before any page is taken
    wm = dict(ngram_len=5, keys=[1, 2, 3])
    for kw, needle in ((dict(do_sample=False), "do_sample=False"), (dict(do_sample=False, num_beams=2), "do_sample=False"),
                       (dict(do_sample=True, num_beams=2), "num_beams > 1"), (dict(do_sample=True, padded_batch=True), "padded_batch"),
                       (dict(do_sample=False, penalty_alpha=0.5, top_k=4), "mirostat_tau"),
                       (dict(do_sample=True, watermarking_config=wm), "watermarking_config"),
                       (dict(do_sample=True, mirostat_mode=1), "mirostat_mode=1")):
        with pytest.raises(NotImplementedError, match="mirostat_tau") as ei:
            gen(mirostat_tau=4.0, **kw)
        assert needle in str(ei.value), (needle, str(ei.value))
    for kw in (dict(mirostat_tau=-1.0), dict(mirostat_tau=float("nan")), dict(mirostat_tau=4.0, mirostat_eta=1.5), dict(mirostat_tau=4.0, mirostat_mode=7)):
        with pytest.raises(ValueError, match="mirostat_"):
            gen(do_sample=True, **kw)
    assert calls == []                                                             # nothing was launched by a refused call
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    with pytest.raises(NotImplementedError, match="mirostat_tau"):
        _submit(eng, reqs[1], SamplingParams(temperature=0.0, mirostat_tau=4.0))
    with pytest.raises(NotImplementedError, match="watermarking_config"):
        _submit(eng, reqs[1], SamplingParams(temperature=0.9, mirostat_tau=4.0, watermarking_config=wm))
    with pytest.raises(ValueError, match="mirostat_tau"):
        SamplingParams(temperature=0.9, mirostat_tau=100.0)
    assert eng.pending() == 0 and len(model.kv.free) == model.kv.num_pages
