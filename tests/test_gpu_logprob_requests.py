"""Top-N log-probabilities, prompt scoring and option ranking end to end on the tiny synthetic model and the request set
of tests/test_gpu_sampling_requests.py: generate(top_logprobs=) against tests/logprob_ref.py on its own returned logits and bit-equal
ids / logprobs with and without it; ServingEngine requests with SamplingParams(top_logprobs=) against their solo generate(); score()
against the fp64 log_softmax of the rows it returns, against forward()'s logits and with the pool and the kept prefix untouched;
rank_options() against the options scored alone."""
import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests.test_gpu_sampling_requests import V, _solo, _submit, dev, model, reqs  # noqa: F401  (module-scoped fixtures, built here again)
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


def _chain(logits):
    """The bound's chain length for rows as the kernel saw them (the tiny vocabulary: the register form)."""
    reg = LR.register_form(logits.shape[1], logits.stride(0), logits.data_ptr() % 16)
    assert reg
    return LR.lse_chain(logits.shape[1], reg)


def test_generate_top_logprobs(dev, model, reqs):
    r = reqs[2]                                             # image + region prompt, sampled with a penalty
    ids = r["input_ids"].to(dev)
    L0, n, N = ids.shape[1], 8, 5
    kw = dict(images=r["images"], regions=r["regions"], do_sample=True, temperature=1.0, top_p=0.95, top_k=20, seed=3, repetition_penalty=1.2,
              max_new_tokens=n, eos_token_id=-1, return_logits=True, return_logprobs=True)
    out, logits, lps, top = model.generate(ids, top_logprobs=N, **kw)
    out_b, logits_b, lps_b = model.generate(ids, **kw)
    assert torch.equal(out, out_b) and torch.equal(lps.view(torch.int32), lps_b.view(torch.int32))      # bit-equal without it
    assert all(torch.equal(a, b) for a, b in zip(logits, logits_b))
    assert set(top) == {"top_ids", "top_logprobs", "rank"}
    assert tuple(top["top_ids"].shape) == (1, n, N) and top["top_ids"].dtype == torch.int32
    assert tuple(top["top_logprobs"].shape) == (1, n, N) and top["top_logprobs"].dtype == torch.float32
    assert tuple(top["rank"].shape) == (1, n) and top["rank"].dtype == torch.int32
    worst = 0.0
    for step in range(n):
        raw = logits[step].cpu().numpy()
        want_ids, want_lp = LR.top(raw, N)
        assert np.array_equal(top["top_ids"][:, step].cpu().numpy(), want_ids), step
        assert np.array_equal(top["rank"][:, step].cpu().numpy(), LR.rank(raw, out[:, L0 + step].cpu().numpy())), step
        worst = max(worst, LR.worst_ratio(top["top_logprobs"][:, step].cpu().numpy(), want_lp, LR.logprob_bound(raw, want_lp, _chain(logits[step]))))
    print(f"generate top_logprobs err/bound max {worst:.3f}")
    assert worst <= 1.0
    # a greedy batch of two, without return_logprobs: the pick stays vt_argmax; the emitted id is the head of its own list with rank 1
    two = torch.cat([reqs[0]["input_ids"][:, :20], reqs[3]["input_ids"][:, :20]], 0).to(dev)
    plain = model.generate(two, do_sample=False, max_new_tokens=6, eos_token_id=-1)
    got, top2 = model.generate(two, do_sample=False, max_new_tokens=6, eos_token_id=-1, top_logprobs=3)
    assert torch.equal(got, plain) and tuple(top2["top_ids"].shape) == (2, 6, 3)
    assert torch.equal(top2["top_ids"][:, :, 0].long(), got[:, 20:]) and bool((top2["rank"] == 1).all())
    assert bool((top2["top_logprobs"][:, :, :-1] >= top2["top_logprobs"][:, :, 1:]).all())
    for bad, exc in ((dict(top_logprobs=21), ValueError), (dict(top_logprobs=-1), ValueError), (dict(top_logprobs=2, num_beams=2), NotImplementedError),
                     (dict(top_logprobs=2, padded_batch=True), NotImplementedError)):
        with pytest.raises(exc):
            model.generate(two, do_sample=False, max_new_tokens=2, **bad)
    assert len(model.kv.free) == model.kv.num_pages


def _count_ops(monkeypatch, counts):
    from vitron_amd import ops
    for name in ("argmax", "sample_top_p", "sample_rows", "ban_rows", "bias_rows", "logprob_rows"):
        def wrap(*a, _f=getattr(ops, name), _n=name, **k):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrap)


def test_serving_top_logprobs_equal_solo(dev, model, reqs, monkeypatch):
    """Four mixed requests, two of which ask for top lists (5 and 3), joining at different steps with max_batch = 3: everybody's tokens are
    those of the solo generate(); the askers' lists are the solo run's -- ids exact, values bit-equal (the same rows, the same kernel)."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    sps = [SamplingParams(top_logprobs=5),                                                           # greedy
           SamplingParams(temperature=0.7, top_p=0.9, seed=101),
           SamplingParams(temperature=1.0, top_k=5, seed=202, repetition_penalty=1.3, top_logprobs=3),
           SamplingParams(repetition_penalty=1.2, logprobs=True)]
    solo = {}
    for i, (r, sp) in enumerate(zip(reqs, sps)):
        if sp.top_logprobs:
            solo[i] = _solo(model, dev, r, sp, return_logprobs=True, top_logprobs=sp.top_logprobs)
        else:
            solo[i] = (_solo(model, dev, r, sp),)

    def run(params):
        eng = ServingEngine(model, max_batch=3, kv_pages=64)
        ids = [_submit(eng, reqs[0], params[0]), _submit(eng, reqs[1], params[1])]
        seen, steps = {i: [] for i in range(4)}, 0
        while eng.pending():
            if steps == 2:
                ids += [_submit(eng, reqs[2], params[2]), _submit(eng, reqs[3], params[3])]
            for rid, t in eng.step():
                seen[rid].append(t)
            steps += 1
            assert steps < 200
        assert ids == [0, 1, 2, 3] and len(model.kv.free) == model.kv.num_pages
        return eng, seen

    counts = {}
    _count_ops(monkeypatch, counts)
    eng, seen = run(sps)
    asked = dict(counts)
    for i in range(4):
        assert seen[i] == solo[i][0], (i, seen[i], solo[i][0])
    for i in (0, 2):
        toks, lps, top = solo[i]
        N = sps[i].top_logprobs
        got = eng.top_logprobs(i)
        assert len(got) == len(toks) == reqs[i]["max_new_tokens"]
        for s, (tok, lp, rank, ids, vals) in enumerate(got):
            assert tok == toks[s] and rank == int(top["rank"][0, s]) and isinstance(ids, tuple) and isinstance(vals, tuple)
            assert lp == float(lps[0, s])                                                             # bit-equal: fp32 -> float is exact
            assert list(ids) == top["top_ids"][0, s].tolist() and len(ids) == N
            assert list(vals) == top["top_logprobs"][0, s].tolist()
        assert torch.equal(eng.logprobs(i), lps[0].cpu())                                              # implied by top_logprobs
    assert all(rank == 1 and ids[0] == tok for tok, _, rank, ids, _ in eng.top_logprobs(0))           # the greedy request
    with pytest.raises(ValueError):
        eng.top_logprobs(1)
    with pytest.raises(ValueError):
        eng.top_logprobs(3)
    assert all(r.last_top is None for r in eng.finished.values())
    # nobody asks: no vt_logprob_rows launch, and every other launch count is what it is with the askers
    counts.clear()
    _, seen_plain = run([sp.replace(top_logprobs=0, logprobs=bool(sp.top_logprobs) or sp.logprobs) for sp in sps])
    assert seen_plain == seen
    assert counts.get("logprob_rows", 0) == 0 and asked["logprob_rows"] > 0
    assert {k: v for k, v in counts.items() if k != "logprob_rows"} == {k: v for k, v in asked.items() if k != "logprob_rows"}
    counts.clear()
    eng = ServingEngine(model, max_batch=3, kv_pages=64)                                               # requests without SamplingParams: the legacy launches
    _submit(eng, reqs[0]), _submit(eng, reqs[3])
    eng.run()
    assert set(counts) == {"argmax"}


def _score_checks(out, ids_rows, with_target):
    """score()'s dict against the fp64 log_softmax of the rows it returned; `with_target`: per sample the positions that must be scored."""
    logits, index = out["logits"], out["logit_index"]
    raw = logits.cpu().numpy()
    B, L = out["logprobs"].shape
    lp, rank = out["logprobs"].cpu().numpy(), out["rank"].cpu().numpy()
    assert [sorted(int(j) for b2, j, _ in index.tolist() if b2 == b) for b in range(B)] == with_target
    targets = np.array([ids_rows[b][j] for b, j, _ in index.tolist()])
    want = LR.target_lp(raw, targets)
    chain = _chain(logits)
    got = np.array([lp[b, j] for b, j, _ in index.tolist()])
    worst = LR.worst_ratio(got, want, LR.logprob_bound(raw, want, chain))
    assert [int(rank[b, j]) for b, j, _ in index.tolist()] == LR.rank(raw, targets).tolist()
    scored = np.zeros((B, L), dtype=bool)
    for b, j, _ in index.tolist():
        scored[b, j] = True
    assert np.isnan(lp[~scored]).all() and (rank[~scored] == 0).all() and np.isfinite(lp[scored]).all() and (rank[scored] >= 1).all()
    if "top_ids" in out:
        N = out["top_ids"].shape[-1]
        want_ids, want_lp = LR.top(raw, N)
        ti, tl = out["top_ids"].cpu().numpy(), out["top_logprobs"].cpu().numpy()
        assert np.array_equal(np.stack([ti[b, j] for b, j, _ in index.tolist()]), want_ids)
        worst = max(worst, LR.worst_ratio(np.stack([tl[b, j] for b, j, _ in index.tolist()]), want_lp, LR.logprob_bound(raw, want_lp, chain)))
        assert (ti[~scored] == -1).all() and np.isnan(tl[~scored]).all()
    assert worst <= 1.0, worst
    return worst


def test_score(dev, model, reqs):
    r = reqs[2]                                             # [1, <image>, 5 tokens, <objs>, 1, 7 tokens]
    ids = r["input_ids"].to(dev)
    row = r["input_ids"][0].tolist()
    L = len(row)
    free0 = None if model.kv is None else len(model.kv.free)
    out = model.score(ids, images=r["images"], regions=r["regions"], top_logprobs=5, return_logits=True)
    assert free0 is None or len(model.kv.free) == free0
    text = [j for j in range(1, L) if row[j] >= 0]
    assert row[1] == -200 and row[7] == -300 and 0 not in text and 1 not in text and 7 not in text and 2 in text and 8 in text
    worst = _score_checks(out, [row], [text])
    # the rows score() read are forward()'s logits at the same spliced rows (both arms run the last layer on all rows)
    llama = model.get_model().llama
    llama.set_last_layer_full(True)
    try:
        full = model.score(ids, images=r["images"], regions=r["regions"], return_logits=True)
        fw = model.forward(input_ids=ids, images=r["images"], regions=r["regions"]).logits          # [1, S, V]
    finally:
        llama.set_last_layer_full(False)
    rows_read = full["logit_index"][:, 2].tolist()
    assert rows_read == sorted(rows_read) and len(rows_read) == len(text)
    want = fw[0, rows_read]
    d = rel_l2(full["logits"], want)
    print(f"score rows vs forward(): rel_l2 {d:.3e}, bit-equal {torch.equal(full['logits'], want)}; err/bound max {worst:.3f}")
    assert torch.equal(full["logits"], want)
    # a ragged text batch as a list: every sequence's numbers are those of the same sequence alone, bit for bit
    a, b = reqs[0]["input_ids"][0], reqs[3]["input_ids"][0]
    both = model.score([a, b], return_logits=True)
    assert tuple(both["logprobs"].shape) == (2, b.numel())
    _score_checks(both, [a.tolist(), b.tolist()], [list(range(1, a.numel())), list(range(1, b.numel()))])
    for i, t in enumerate((a, b)):
        alone = model.score(t.unsqueeze(0).to(dev))
        n = t.numel()
        assert torch.equal(both["logprobs"][i, :n].view(torch.int32), alone["logprobs"][0].view(torch.int32))
        assert torch.equal(both["rank"][i, :n], alone["rank"][0]) and bool(both["logprobs"][i, n:].isnan().all())
    packed = model.score([a, b], packed_prefill=True)
    assert torch.equal(packed["rank"] > 0, both["rank"] > 0)
    print(f"score packed vs per-sequence prefill: max |d logprob| {float((packed['logprobs'] - both['logprobs']).nan_to_num().abs().max()):.3e}")
    with pytest.raises(ValueError):
        model.score(ids, images=r["images"], regions=r["regions"], top_logprobs=21)
    assert free0 is None or len(model.kv.free) == free0


def test_score_leaves_the_pool_and_the_kept_prefix_alone(dev, model, reqs):
    g = torch.Generator().manual_seed(12)
    ids = torch.tensor([[1] + torch.randint(3, V, (69,), generator=g).tolist()]).to(dev)            # more than one page: a prefix worth keeping
    model.config.kv_prefix_reuse = True
    try:
        first = model.generate(ids, do_sample=False, max_new_tokens=4, eos_token_id=-1)             # leaves its pages as the next call's prefix
        kept = model._prefix
        assert kept is not None and len(kept.pages) > 0
        state = (list(kept.pages), kept.sig.copy(), len(model.kv.free), model.kv.num_pages, model.kv)
        model.score(reqs[3]["input_ids"].to(dev), top_logprobs=3)
        many = len(model.kv.free) // 2 + 1                                                            # more pages than the pool has free:
        model.score([reqs[3]["input_ids"][0]] * many, packed_prefill=True)                            # the call brings a pool of its own
        assert model._prefix is kept and list(kept.pages) == state[0] and np.array_equal(kept.sig, state[1])
        assert len(model.kv.free) == state[2] and model.kv.num_pages == state[3] and model.kv is state[4]
        again = model.generate(ids, do_sample=False, max_new_tokens=4, eos_token_id=-1)
        assert torch.equal(again, first) and model.last_generate_stats["reused_tokens"] > 0         # the prefix was still usable
    finally:
        model.reset_prefix_cache()
        model.config.kv_prefix_reuse = False
    assert len(model.kv.free) == model.kv.num_pages


def test_rank_options(dev, model, reqs):
    r = reqs[1]                                             # [1, <image>, 11 tokens]
    prompt = r["input_ids"][0]
    P = prompt.numel()
    g = torch.Generator().manual_seed(5)
    options = [torch.randint(3, V, (n,), generator=g) for n in (1, 4, 2, 6, 4)]
    solo_lp, solo_bound = [], []
    for o in options:
        s = model.score(torch.cat([prompt, o]).unsqueeze(0).to(dev), images=r["images"], return_logits=True)
        lp = s["logprobs"][0, P:].double().cpu().numpy()
        assert np.isfinite(lp).all() and lp.size == o.numel()
        raw = s["logits"].cpu().numpy()[-o.numel():]                                                 # the rows that score the option's tokens
        assert s["logit_index"][-o.numel():, 1].tolist() == list(range(P, P + o.numel()))
        solo_lp.append(lp)
        solo_bound.append(LR.logprob_bound(raw, LR.target_lp(raw, o.numpy()), _chain(s["logits"])))
    for normalize in ("sum", "mean"):
        order, scores = model.rank_options(prompt, options, images=r["images"], normalize=normalize)
        assert scores.dtype == torch.float64 and tuple(scores.shape) == (len(options),) and sorted(order) == list(range(len(options)))
        div = [o.numel() if normalize == "mean" else 1 for o in options]
        want = np.array([lp.sum() / d for lp, d in zip(solo_lp, div)])
        tol = np.array([2.0 * b.sum() / d for b, d in zip(solo_bound, div)])                          # both sides are inside their bounds
        diff = np.abs(scores.numpy() - want)
        print(f"rank_options({normalize}): max |batch - solo| {diff.max():.3e}, summed bounds {tol.min():.3e} .. {tol.max():.3e}")
        assert (diff <= tol).all(), (diff.tolist(), tol.tolist())
        # the order is exact on the options whose gaps exceed the bounds: keep those, in option order
        keep = [i for i in range(len(options)) if all(j == i or abs(want[i] - want[j]) > tol[i] + tol[j] for j in range(len(options)))]
        assert len(keep) >= 3
        assert [i for i in order if i in keep] == sorted(keep, key=lambda i: -want[i])
        order_k, scores_k = model.rank_options(prompt, [options[i] for i in keep], images=r["images"], normalize=normalize)
        assert [keep[i] for i in order_k] == sorted(keep, key=lambda i: -want[i])
        assert torch.equal(scores_k, scores[keep])                                                   # an option's score does not depend on its neighbours
    assert model.last_tower_items == 0                                                               # the image came out of the cache
    order, scores = model.rank_options(prompt, [options[1], options[1], options[4]], images=r["images"])
    assert float(scores[0]) == float(scores[1]) and order.index(0) < order.index(1)                  # ties keep option order
    with pytest.raises(ValueError):
        model.rank_options(prompt, options, images=r["images"], normalize="median")
    with pytest.raises(ValueError):
        model.rank_options(prompt, [], images=r["images"])
    assert len(model.kv.free) == model.kv.num_pages
