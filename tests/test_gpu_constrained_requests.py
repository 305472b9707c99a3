"""Constrained decoding end to end on the tiny synthetic model of the golden cases (tests/allow_cases.py; 2 layers, V = 512, kv_prefix_reuse off):
generate()'s suppress_tokens / begin_suppress_tokens / min_new_tokens / bad_words_ids / allowed_token_ids and ServingEngine requests whose
SamplingParams carry allowed / banned ids, min_new_tokens, choices or an allowed_tokens_fn. The constrained request equals its solo
generate(), its unconstrained neighbours keep their solo tokens, a request whose constraints run empty fails alone, and a static mask is
uploaded once."""
import numpy as np
import pytest
import torch

from tests import allow_ref as A
from tests.golden import cases
from tests.allow_cases import solo as _solo, submit as _submit, tiny_model

pytestmark = pytest.mark.gpu
V = cases.LLM["vocab_size"]
ALLOWED = sorted(set(range(3, V, 7)) | {31, 32, V - 1})          # 76 ids, the word boundaries among them


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
    g = torch.Generator().manual_seed(44)
    rnd = lambda n: torch.randint(3, V, (n,), generator=g).tolist()                     # noqa: E731
    return [
        dict(input_ids=torch.tensor([[1] + rnd(19)]), images=None, regions=None, max_new_tokens=8),
        dict(input_ids=torch.tensor([[1, -200] + rnd(9)]), images=[torch.randn((3, 56, 56), generator=g).bfloat16().to(dev)], regions=None,
             max_new_tokens=8),
        dict(input_ids=torch.tensor([[1] + rnd(30)]), images=None, regions=None, max_new_tokens=7),
    ]


def _new(out, r):
    return out[0, r["input_ids"].shape[1]:].cpu().tolist()


def test_allowed_ids_generate_equals_the_engine_in_a_mixed_batch(dev, model, reqs):
    """generate(allowed_token_ids=) emits only allowed ids, greedy and sampled; the same requests through ServingEngine beside two
    unconstrained neighbours (one greedy, one sampled, one joining late) return the same tokens, and the neighbours their solo tokens."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    sps = [SamplingParams(allowed_token_ids=ALLOWED),                                                   # greedy, the image request
           SamplingParams(temperature=0.9, top_p=0.95, top_k=20, seed=11, allowed_token_ids=ALLOWED),    # sampled
           SamplingParams(),                                                                             # unconstrained greedy neighbour
           SamplingParams(temperature=0.8, seed=12)]                                                     # unconstrained sampled neighbour
    rs = [reqs[1], reqs[0], reqs[2], reqs[0]]
    solo = [None] * 4
    for i in range(4):
        kw = dict(allowed_token_ids=ALLOWED) if sps[i].constrained else {}
        o = model.generate(rs[i]["input_ids"].to(dev), images=rs[i]["images"], regions=rs[i]["regions"], do_sample=sps[i].temperature > 0,
                           temperature=sps[i].temperature or 1.0, top_p=sps[i].top_p, top_k=sps[i].top_k, seed=sps[i].seed,
                           max_new_tokens=rs[i]["max_new_tokens"], eos_token_id=-1, **kw)
        solo[i] = _new(o, rs[i])
    assert set(solo[0]) <= set(ALLOWED) and set(solo[1]) <= set(ALLOWED)
    free = [_solo(model, dev, rs[i], SamplingParams(temperature=sps[i].temperature, top_p=sps[i].top_p, top_k=sps[i].top_k, seed=sps[i].seed))
            for i in (0, 1)]
    assert not set(free[0]) <= set(ALLOWED) and free[0] != solo[0] and free[1] != solo[1]               # the constraint changed both runs
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    ids = [_submit(eng, rs[0], sps[0]), _submit(eng, rs[2], sps[2])]
    seen = {i: [] for i in range(4)}
    steps = 0
    while eng.pending():
        if steps == 2:
            ids += [_submit(eng, rs[1], sps[1]), _submit(eng, rs[3], sps[3])]
        for rid, t in eng.step():
            seen[rid].append(t)
        steps += 1
        assert steps < 100
    order = [0, 2, 1, 3]                                                         # request id -> index into rs / sps / solo
    for rid, i in enumerate(order):
        assert seen[rid] == solo[i], (rid, seen[rid], solo[i])
    for rid, i in enumerate(order):                                              # a static mask: one upload per request, released at the end
        r = eng.finished[rid]
        assert r.mask_uploads == (1 if sps[i].constrained else 0) and r.allow_dev == {} and r.allow_cur is None
    assert len(model.kv.free) == model.kv.num_pages
    # a batch of two through generate: both rows held to the set
    two = torch.cat([reqs[0]["input_ids"], reqs[2]["input_ids"][:, :20]], 0).to(dev)
    b2 = model.generate(two, do_sample=True, temperature=1.0, top_k=30, seed=4, max_new_tokens=6, eos_token_id=-1, allowed_token_ids=ALLOWED)
    assert set(b2[:, 20:].flatten().tolist()) <= set(ALLOWED)


def test_generate_keywords_equal_the_host_loop(dev, model, reqs):
    """Greedy generate with suppress_tokens, begin_suppress_tokens, bad_words_ids, min_new_tokens and allowed_token_ids together: every
    emitted id is the first maximum of the RETURNED logits with -inf at that step's banned ids (tests/allow_ref.py)."""
    r = reqs[0]
    ids = r["input_ids"].to(dev)
    L0, n = ids.shape[1], 8
    plain, plain_logits = model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, return_logits=True)
    t = _new(plain, r)
    order0 = plain_logits[0][0].argsort(descending=True).cpu().tolist()
    sup, begin, bad, eos = [t[0]], [order0[1]], [[order0[2]], [t[3]]], order0[3]
    allowed = sorted(set(order0[:200]) | set(t) | {eos})
    kw = dict(suppress_tokens=sup, begin_suppress_tokens=begin, bad_words_ids=bad, min_new_tokens=3, allowed_token_ids=allowed)
    out, logits = model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos, return_logits=True, **kw)
    got = _new(out, r)
    assert len(got) >= 3
    for step, tok in enumerate(got):
        banned = set(sup) | {w[0] for w in bad} | (set(begin) if step == 0 else set()) | ({eos} if step < 3 else set())
        want = int(A.masked_logits(logits[step][:1].cpu(), [A.mask_loop(V, allowed, sorted(banned & set(allowed)))])[0].argmax())
        assert tok == want, (step, tok, want)
    assert got[0] == order0[4]                                                   # the four best first tokens are banned, each by another keyword
    # the defaults are the call without the keywords; what cannot be served is refused
    same = model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, suppress_tokens=None, begin_suppress_tokens=None,
                          min_new_tokens=None, bad_words_ids=None, allowed_token_ids=None)
    assert torch.equal(same, plain)
    assert torch.equal(model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, min_new_tokens=3), plain)     # no EOS id to ban: no mask
    with pytest.raises(NotImplementedError, match=r"\[5, 6\]"):
        model.generate(ids, do_sample=False, max_new_tokens=2, bad_words_ids=[[4], [5, 6]])
    with pytest.raises(ValueError):
        model.generate(ids, do_sample=False, max_new_tokens=2, allowed_token_ids=[7], suppress_tokens=[7])
    with pytest.raises(ValueError):
        model.generate(ids, do_sample=False, max_new_tokens=2, allowed_token_ids=[V])
    with pytest.raises(NotImplementedError):
        model.generate(torch.cat([ids, ids], 0), do_sample=False, max_new_tokens=2, padded_batch=True, suppress_tokens=[7])
    assert len(model.kv.free) == model.kv.num_pages


def test_min_new_tokens(dev, model, reqs):
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    r = reqs[2]
    ids = r["input_ids"].to(dev)
    t0 = _new(model.generate(ids, do_sample=False, max_new_tokens=1, eos_token_id=-1), r)[0]
    short = _new(model.generate(ids, do_sample=False, max_new_tokens=7, eos_token_id=t0), r)
    assert short == [t0]                                                         # the first greedy token is EOS: the run ends at once
    held = _new(model.generate(ids, do_sample=False, max_new_tokens=7, eos_token_id=t0, min_new_tokens=3), r)
    assert len(held) >= 3 and held[0] != t0 and t0 not in held[:3]
    eng = ServingEngine(model, max_batch=3, kv_pages=64)
    a = eng.submit(r["input_ids"], None, None, 7, eos_token_id=t0)
    b = eng.submit(r["input_ids"], None, None, 7, eos_token_id=t0, sampling=SamplingParams(min_new_tokens=3))
    c = eng.submit(r["input_ids"], None, None, 7, eos_token_id=t0, sampling=SamplingParams(min_new_tokens=3, allowed_token_ids=range(V)))
    out = eng.run()
    assert out[a].tolist() == short and out[b].tolist() == held and out[c].tolist() == held
    assert eng.finished[b].mask_uploads == 1 and eng.finished[c].mask_uploads == 2        # "pre" only (after it: NULL); "pre" and "post"
    assert len(model.kv.free) == model.kv.num_pages


def test_choices(dev, model, reqs):
    """The reply is one of the choices followed by EOS, where one choice is a prefix of another; greedy and five sampled streams, beside
    an unconstrained neighbour that keeps its solo tokens."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    eos = 2
    choices = [[40, 41], [40], [40, 41, 42], [77, 78, 79], [300]]
    sps = [SamplingParams(choices=choices)] + [SamplingParams(choices=choices, temperature=1.5, seed=s) for s in range(5)]
    nb = SamplingParams(temperature=0.9, seed=3)
    solo_nb = _solo(model, dev, reqs[0], nb)
    eng = ServingEngine(model, max_batch=8, kv_pages=128)
    rids = [eng.submit(reqs[i % 3]["input_ids"], reqs[i % 3]["images"], None, 6, eos_token_id=eos, sampling=sp) for i, sp in enumerate(sps)]
    n = _submit(eng, reqs[0], nb)
    out = eng.run()
    assert not eng.failed
    replies = set()
    for rid in rids:
        toks = out[rid].tolist()
        assert toks[-1] == eos and toks[:-1] in choices, toks
        replies.add(tuple(toks[:-1]))
        assert eng.finished[rid].mask_uploads == len(toks)                       # step-dependent: one small upload per pick
    assert out[n].tolist() == solo_nb
    print("choices taken:", sorted(replies))
    assert len(model.kv.free) == model.kv.num_pages


def test_allowed_tokens_fn_and_a_request_that_runs_empty(dev, model, reqs):
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    calls, calls_bad = [], []

    def fn(toks):
        calls.append(list(toks))
        return None if len(toks) == 1 else [100 + len(toks), 200 + len(toks)]

    def fn_bad(toks):
        calls_bad.append(list(toks))
        return [] if len(toks) == 2 else ALLOWED

    nb = SamplingParams(temperature=0.7, seed=9)
    solo_nb = _solo(model, dev, reqs[2], nb)
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    a = _submit(eng, reqs[0], SamplingParams(allowed_tokens_fn=fn))
    b = _submit(eng, reqs[1], SamplingParams(allowed_tokens_fn=fn_bad, temperature=1.0, seed=1))
    c = _submit(eng, reqs[2], nb)
    out = eng.run()
    ta = out[a].tolist()
    assert len(ta) == reqs[0]["max_new_tokens"]
    assert calls == [ta[:n] for n in range(len(ta))]                             # once per pick, with the tokens so far
    for n, t in enumerate(ta):
        assert t in (100 + n, 200 + n) or n == 1
    assert b in eng.failed and b not in out and isinstance(eng.errors()[b], ValueError)
    fb = eng.failed[b]
    assert len(fb.tokens) == 2 and set(fb.tokens) <= set(ALLOWED) and calls_bad == [fb.tokens[:n] for n in range(3)]
    assert fb.allow_dev == {} and fb.allow_cur is None
    assert out[c].tolist() == solo_nb                                            # the neighbours went on
    assert len(model.kv.free) == model.kv.num_pages


def test_batch_prefill_prepares_the_masks_before_the_shared_forward(dev, model, reqs):
    """batch_prefill=True: a request whose function leaves nothing for the FIRST token fails at admission, alone, with its function called
    once; the others share the packed prefill, and every function is still called once per pick."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    calls, calls_bad = [], []

    def fn(toks):
        calls.append(list(toks))
        return [100 + len(toks), 200 + len(toks)]

    def fn_bad(toks):
        calls_bad.append(list(toks))
        return []

    eng = ServingEngine(model, max_batch=4, kv_pages=64, batch_prefill=True)
    a = _submit(eng, reqs[0], SamplingParams(allowed_tokens_fn=fn))
    b = _submit(eng, reqs[1], SamplingParams(allowed_tokens_fn=fn_bad))
    c = _submit(eng, reqs[2], SamplingParams(temperature=0.7, seed=9))
    out = eng.run()
    ta = out[a].tolist()
    assert calls_bad == [[]] and b in eng.failed and isinstance(eng.errors()[b], ValueError) and eng.failed[b].tokens == []
    assert len(ta) == reqs[0]["max_new_tokens"] and calls == [ta[:n] for n in range(len(ta))]
    assert all(t in (100 + n, 200 + n) for n, t in enumerate(ta))
    assert len(out[c]) == reqs[2]["max_new_tokens"]
    assert len(model.kv.free) == model.kv.num_pages
