"""Per-request sampling end to end on the tiny synthetic model of tests/test_gpu_model.py (kv_prefix_reuse off, no EOS): a request
submitted with SamplingParams gets the tokens of its solo generate() whatever else is in the batch; requests without keep their legacy
draws; generate()'s repetition penalty equals the restated processor on its own returned logits and its log-probabilities stay inside
the fp64 bound of tests/sample_ref.py."""
import numpy as np
import pytest
import torch

from tests import sample_ref as R
from tests.golden import cases
from tests.test_gpu_model import _states

pytestmark = pytest.mark.gpu
V = cases.LLM["vocab_size"]


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from vitron_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    st = _states()
    cfg = LlavaConfig(**cases.LLM, mm_hidden_size=cases.MM_HIDDEN, mm_image_tower="golden/LanguageBind_Image",
                      mm_video_tower="golden/LanguageBind_Video_merge", kv_prefix_reuse=False)
    m = LlavaLlamaForCausalLM(cfg)
    m.get_image_tower().load_state(cases.VIT_IMAGE, st["image_tower"])
    m.get_video_tower().load_state(cases.VIT_VIDEO, st["video_tower"])
    sd = dict(st["llama"])
    sd.update({"model.mm_projector." + k: v for k, v in st["projector"].items()})
    sd.update({"model.region_extractor." + k: v for k, v in st["region"].items()})
    m.load_state_dict(sd)
    m = m.to(dev)
    m.config.kv_prefix_reuse = False
    return m


@pytest.fixture(scope="module")
def reqs(dev):
    g = torch.Generator().manual_seed(33)
    img = lambda: torch.randn((3, 56, 56), generator=g).bfloat16().to(dev)            # noqa: E731
    rnd = lambda n: torch.randint(3, V, (n,), generator=g).tolist()                     # noqa: E731
    return [
        dict(input_ids=torch.tensor([[1] + rnd(23)]), images=None, regions=None, max_new_tokens=9),
        dict(input_ids=torch.tensor([[1, -200] + rnd(11)]), images=[img()], regions=None, max_new_tokens=12),
        dict(input_ids=torch.tensor([[1, -200] + rnd(5) + [-300, 1] + rnd(7)]), images=[img()], regions=[[20.0, 30.0, 150.0, 200.0]], max_new_tokens=10),
        dict(input_ids=torch.tensor([[1] + rnd(40)]), images=None, regions=None, max_new_tokens=8),
    ]


def _params():
    from vitron_amd.sampling import SamplingParams
    return [SamplingParams(),                                                                       # greedy
            SamplingParams(temperature=0.7, top_p=0.9, seed=101),
            SamplingParams(temperature=1.0, top_k=5, seed=202, repetition_penalty=1.3),
            SamplingParams(repetition_penalty=1.2, logprobs=True)]                                   # greedy + penalty + logprobs


def _solo(model, dev, r, sp, **kw):
    o = model.generate(r["input_ids"].to(dev), images=r["images"], regions=r["regions"], do_sample=sp.temperature > 0,
                       temperature=sp.temperature if sp.temperature > 0 else 1.0, top_p=sp.top_p, top_k=sp.top_k, seed=sp.seed,
                       repetition_penalty=sp.repetition_penalty, max_new_tokens=r["max_new_tokens"], eos_token_id=-1, **kw)
    if kw:
        return (o[0][0, r["input_ids"].shape[1]:].cpu().tolist(),) + tuple(o[1:])
    return o[0, r["input_ids"].shape[1]:].cpu().tolist()


def _submit(eng, r, sp=None):
    return eng.submit(r["input_ids"], r["images"], r["regions"], r["max_new_tokens"], eos_token_id=-1, sampling=sp)


def test_solo_equality_under_mixed_sampling(dev, model, reqs):
    """text / image / image + region / text with four different SamplingParams, joining at different steps with max_batch = 3: every
    request's tokens are those of its solo generate() with the same arguments; the logprobs accessor returns the solo run's."""
    from vitron_amd.serving import ServingEngine
    sps = _params()
    solo = [_solo(model, dev, r, sp) for r, sp in zip(reqs, sps)]
    solo3, solo3_lp = _solo(model, dev, reqs[3], sps[3], return_logprobs=True)
    assert solo3 == solo[3] and tuple(solo3_lp.shape) == (1, reqs[3]["max_new_tokens"])
    eng = ServingEngine(model, max_batch=3, kv_pages=64)
    ids = [_submit(eng, reqs[0], sps[0]), _submit(eng, reqs[1], sps[1])]
    seen = {i: [] for i in range(4)}
    steps = 0
    while eng.pending():
        if steps == 2:      # two more arrive while the first two decode; max_batch = 3 makes the fourth wait for a free slot
            ids += [_submit(eng, reqs[2], sps[2]), _submit(eng, reqs[3], sps[3])]
        for rid, t in eng.step():
            seen[rid].append(t)
        steps += 1
        assert len(eng.active) <= 3 and steps < 200
    assert ids == [0, 1, 2, 3]
    for i in range(4):
        assert seen[i] == solo[i], (i, seen[i], solo[i])
    assert torch.equal(eng.logprobs(3), solo3_lp[0].cpu())
    with pytest.raises(ValueError):
        eng.logprobs(0)
    assert len(model.kv.free) == model.kv.num_pages


def test_neighbour_independence(dev, model, reqs):
    """The same sampled request alone, beside a neighbour, and beside the same neighbour joining two steps late: one token list."""
    from vitron_amd.serving import ServingEngine
    from vitron_amd.sampling import SamplingParams
    sp = SamplingParams(temperature=0.9, top_p=0.95, seed=7)
    nb = SamplingParams(temperature=1.1, seed=8)
    outs = []
    for mode in ("alone", "together", "late"):
        eng = ServingEngine(model, max_batch=3, kv_pages=64)
        a = _submit(eng, reqs[0], sp)
        if mode == "together":
            _submit(eng, reqs[3], nb)
        got, steps = [], 0
        while eng.pending():
            if mode == "late" and steps == 2:
                _submit(eng, reqs[3], nb)
            got += [t for rid, t in eng.step() if rid == a]
            steps += 1
        outs.append(got)
        assert len(model.kv.free) == model.kv.num_pages
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) == reqs[0]["max_new_tokens"]
    assert outs[0] == _solo(model, dev, reqs[0], sp)


def test_legacy_requests_are_unchanged(dev, model, reqs):
    """do_sample=True, seed=7 engine: two requests without `sampling` give the same tokens whether or not a request WITH sampling is served
    by the same engine afterwards, and -- through sample_rows, in a mixed step -- when it decodes beside them."""
    from vitron_amd.serving import ServingEngine
    from vitron_amd.sampling import SamplingParams

    def run(third, late):
        eng = ServingEngine(model, max_batch=3, kv_pages=64, do_sample=True, temperature=0.8, top_p=0.9, seed=7)
        a, b = _submit(eng, reqs[0]), _submit(eng, reqs[3])
        if third and not late:
            _submit(eng, reqs[1], SamplingParams(temperature=0.7, seed=5))
        out = eng.run()
        if third and late:                      # submitted after the first two have finished
            c = _submit(eng, reqs[1], SamplingParams(temperature=0.7, seed=5))
            out.update(eng.run())
            assert len(out[c]) == reqs[1]["max_new_tokens"]
        assert len(model.kv.free) == model.kv.num_pages
        return out[a].tolist(), out[b].tolist()

    base = run(False, False)
    assert run(True, True) == base
    assert run(True, False) == base             # mixed steps: the legacy rows' (engine seed, engine step, batch row) draw through sample_rows


def test_generate_penalty_logprobs_and_defaults(dev, model, reqs):
    r = reqs[0]
    ids = r["input_ids"].to(dev)
    L0, n = ids.shape[1], 12
    # greedy + penalty: the ids are the host loop over the RETURNED logits (restated processor, first argmax)
    out, logits, lps = model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, repetition_penalty=1.3, return_logits=True,
                                      return_logprobs=True)
    hist = [t for t in r["input_ids"][0].tolist() if t >= 0]
    worst = 0.0
    for step in range(n):
        raw = logits[step][0].cpu().numpy()
        want = int(np.argmax(R.repetition_penalty(raw, hist, 1.3)))
        assert int(out[0, L0 + step]) == want, (step, int(out[0, L0 + step]), want)
        err = abs(float(lps[0, step]) - R.logprob_ref(raw)[want])
        bound = R.logprob_bound(raw, [want])[0]
        assert err <= bound, (step, err, bound)
        worst = max(worst, err / bound)
        hist.append(want)
    print(f"generate logprob err/bound max {worst:.3f}")
    plain = model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1)
    assert not torch.equal(plain, out)                                                             # the penalty changes the greedy run
    # the image + region prompt: negative sentinels stay out of the history
    r2 = reqs[2]
    out2, logits2 = model.generate(r2["input_ids"].to(dev), images=r2["images"], regions=r2["regions"], do_sample=False, max_new_tokens=6,
                                   eos_token_id=-1, repetition_penalty=1.3, return_logits=True)
    hist = [t for t in r2["input_ids"][0].tolist() if t >= 0]
    for step in range(6):
        want = int(np.argmax(R.repetition_penalty(logits2[step][0].cpu().numpy(), hist, 1.3)))
        assert int(out2[0, r2["input_ids"].shape[1] + step]) == want
        hist.append(want)
    # sampled: seed 3 is one for which the penalty changes at least one token; logprobs alone change nothing
    kw = dict(do_sample=True, temperature=1.0, top_p=0.95, top_k=20, seed=3, max_new_tokens=n, eos_token_id=-1)
    base = model.generate(ids, **kw)
    pen = model.generate(ids, repetition_penalty=1.3, **kw)
    assert base.shape == pen.shape and not torch.equal(base, pen)
    same, lp = model.generate(ids, return_logprobs=True, **kw)
    assert torch.equal(same, base) and tuple(lp.shape) == (1, n) and bool((lp <= 0).all())
    # defaults: the new arguments at their defaults are the call without them; a batch of two keeps its rows
    assert torch.equal(model.generate(ids, repetition_penalty=1.0, return_logprobs=False, **kw), base)
    assert torch.equal(model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=-1, repetition_penalty=1.0, return_logprobs=False), plain)
    two = torch.cat([ids, reqs[3]["input_ids"][:, :L0].to(dev)], 0)
    b2 = model.generate(two, **kw)
    b2p, lp2 = model.generate(two, return_logprobs=True, **kw)
    assert torch.equal(b2, b2p) and tuple(lp2.shape) == (2, n)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0)):
        with pytest.raises(ValueError):
            model.generate(ids, do_sample=False, max_new_tokens=2, **bad)
    assert len(model.kv.free) == model.kv.num_pages
