"""Classifier-free guidance end to end on the tiny synthetic model (tests/allow_cases.py): generate(guidance_scale=)
against a loop this file drives itself over the same 2B sequences (llama_forward, DecodeState, ops.cfg_rows, the picker's own launch),
the identities that need no reference (guidance against itself, scale 0, scale None / 1), what return_logits / return_logprobs /
top_logprobs show, the plausibility cut, the compositions with no_repeat_ngram_size and choices, ServingEngine requests with
SamplingParams(guidance_scale=) beside other requests and the return of their pages, the refusals."""
import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import sample_ref as SR
from tests.golden import cases as G
from tests.allow_cases import tiny_model

pytestmark = pytest.mark.gpu
TV = G.LLM["vocab_size"]
NINF = -float("inf")


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return tiny_model(dev)


def _ids(seed, n, image=False):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([[1] + ([-200] if image else []) + torch.randint(3, TV, (n,), generator=g).tolist()])


def _image(dev, seed):
    return torch.randn((3, 56, 56), generator=torch.Generator().manual_seed(seed)).bfloat16().to(dev)


def _new(out, L0, b=0):
    return out[b, L0:].cpu().tolist()


@pytest.fixture(scope="module")
def one(dev):
    """B = 1: a prompt with an image, a text-only negative prompt"""
    return dict(ids=_ids(501, 10, image=True).to(dev), images=[_image(dev, 502)], neg=_ids(503, 6).to(dev))


@pytest.fixture(scope="module")
def two(dev):
    """B = 2: text prompts of one length, negative prompts of another"""
    return dict(ids=torch.cat([_ids(511, 12), _ids(512, 12)]).to(dev), images=None, neg=torch.cat([_ids(513, 5), _ids(514, 5)]).to(dev))


def drive(model, dev, ids, images, neg, neg_images, scale, n_new, pick=None):
    """The loop generate(guidance_scale=) is held to, driven from here: both prompts embedded and prefilled as generate() does it (the
    conditional batch in one pass, the negative batch in a pass of its own), one DecodeState over the 2B sequences fed the picked ids
    twice, per step ONE ops.cfg_rows launch in place over the conditional rows and then `pick(step, guided rows)` (ops.argmax by
    default). Returns (the picked ids per sample, every step's guided rows as host arrays)."""
    from vitron_amd import ops
    from vitron_amd.engine import DecodeState, SequenceState, llama_forward
    from vitron_amd.sampling import pack_cfg_rows
    B = ids.shape[0]
    llama = model.model.llama
    emb, mh, _ = model._embed_prompt(ids, None, images, None, use_vis_cache=False)
    flat, flat_lo, lens, _ = model._pack_rows(emb, mh)
    nemb, nmh, _ = model._embed_prompt(neg, None, neg_images, None, use_vis_cache=False)
    nflat, nflat_lo, nlens, _ = model._pack_rows(nemb, nmh)
    model._ensure_kv(sum((n + n_new + 63) // 64 + 1 for n in lens + nlens))
    seqs, nseqs = [SequenceState() for _ in range(B)], [SequenceState() for _ in range(B)]
    toks, guided, state = [], [], None
    try:
        c = llama_forward(llama, model.kv, seqs, flat, lens, embeds_lo=flat_lo)
        u = llama_forward(llama, model.kv, nseqs, nflat, nlens, embeds_lo=nflat_lo)
        V = c.shape[1]
        for st in range(n_new):
            rows = pack_cfg_rows([(c[b].data_ptr(), u[b].data_ptr(), c[b].data_ptr(), 0, 0, 0, scale, NINF) for b in range(B)], dev)
            ops.cfg_rows(rows, B, V)
            guided.append(c.float().cpu().numpy().copy())
            nxt = ops.argmax(c) if pick is None else pick(st, c)
            toks.append(nxt.cpu().tolist())
            if st + 1 < n_new:
                if state is None:
                    state = DecodeState(llama, model.kv, seqs + nseqs, n_new, [], 0)
                state.feed(torch.cat((nxt, nxt)))
                full = state.forward()
                c, u = full[:B], full[B:]
    finally:
        for s in seqs + nseqs:
            model.kv.release(s.pages)
    return [[t[b] for t in toks] for b in range(B)], guided


def test_off_is_todays_call(dev, model, one):
    """guidance_scale=None and =1 (with or without a negative prompt): the ids and the returned logits of the call without the argument,
    bit for bit; no second sequence is run."""
    kw = dict(images=one["images"], do_sample=False, max_new_tokens=5, eos_token_id=-1, return_logits=True)
    out0, lg0 = model.generate(one["ids"], **kw)
    for extra in (dict(guidance_scale=None), dict(guidance_scale=1), dict(guidance_scale=1.0, negative_prompt_ids=one["neg"])):
        out, lg = model.generate(one["ids"], **kw, **extra)
        assert torch.equal(out, out0) and len(lg) == len(lg0) and all(torch.equal(a, b) for a, b in zip(lg, lg0))
        assert "negative_rows" not in model.last_generate_stats
    assert len(model.kv.free) == model.kv.num_pages


@pytest.mark.parametrize("case", ("one", "two"))
def test_greedy_ids_equal_the_driven_loop(dev, model, one, two, case):
    """Plumbing: the greedy guided ids are those of the loop above -- the same launches over the same sequences -- at B = 1 with an image
    against a text-only negative prompt and at B = 2; guidance changes the reply (the premise); a [1, Ln] negative prompt is every
    sample's."""
    d = one if case == "one" else two
    L0, n_new, scale = d["ids"].shape[1], 6, 2.5
    want, _ = drive(model, dev, d["ids"], d["images"], d["neg"], None, scale, n_new)
    out = model.generate(d["ids"], images=d["images"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, guidance_scale=scale,
                         negative_prompt_ids=d["neg"])
    got = [_new(out, L0, b) for b in range(d["ids"].shape[0])]
    assert got == want, (got, want)
    assert model.last_generate_stats["negative_rows"] == d["neg"].numel()
    plain = model.generate(d["ids"], images=d["images"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1)
    assert [_new(plain, L0, b) for b in range(d["ids"].shape[0])] != got
    if case == "two":
        shared = d["neg"][:1]
        want1, _ = drive(model, dev, d["ids"], None, shared.expand(2, -1).contiguous(), None, scale, n_new)
        out1 = model.generate(d["ids"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, guidance_scale=scale, negative_prompt_ids=shared)
        assert [_new(out1, L0, b) for b in range(2)] == want1
        # the default negative prompt: every sample's last token
        wantd, _ = drive(model, dev, d["ids"], None, d["ids"][:, -1:].contiguous(), None, scale, n_new)
        outd = model.generate(d["ids"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, guidance_scale=scale)
        assert [_new(outd, L0, b) for b in range(2)] == wantd
    assert len(model.kv.free) == model.kv.num_pages


def test_guidance_against_itself_is_a_no_op(dev, model, one):
    """The negative prompt and its image ARE the positive ones (B = 1, no prefix reuse: both prefills are the same solo pass, both
    decode rows hold the same values): cl - ul is exactly 0, so the ids for any scale are the unguided greedy ids."""
    L0 = one["ids"].shape[1]
    kw = dict(images=one["images"], do_sample=False, max_new_tokens=8, eos_token_id=-1)
    plain = _new(model.generate(one["ids"], **kw), L0)
    for scale in (3.0, 0.0, -2.0, 7.5):
        got = _new(model.generate(one["ids"], **kw, guidance_scale=scale, negative_prompt_ids=one["ids"], negative_images=one["images"]), L0)
        assert got == plain, (scale, got, plain)
    assert len(model.kv.free) == model.kv.num_pages


def test_scale_zero_follows_the_negative_prompt(dev, model, one):
    """scale = 0: the guided row is log_softmax(uncond), so the ids are the unguided greedy ids of generate(negative_prompt_ids)."""
    n_new = 8
    want = _new(model.generate(one["neg"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1), one["neg"].shape[1])
    got = _new(model.generate(one["ids"], images=one["images"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, guidance_scale=0.0,
                              negative_prompt_ids=one["neg"]), one["ids"].shape[1])
    assert got == want, (got, want)
    assert len(model.kv.free) == model.kv.num_pages


def test_return_logits_stay_conditional_and_sampling_is_reproducible(dev, model, one):
    """return_logits are the conditional model rows, cloned before the combine: step 0 is bit for bit the unguided call's; they are not
    the guided rows. Sampling with a seed is reproducible, and another seed gives another reply."""
    kw = dict(images=one["images"], max_new_tokens=6, eos_token_id=-1, return_logits=True)
    _, lg0 = model.generate(one["ids"], do_sample=False, **kw)
    out, lg = model.generate(one["ids"], do_sample=False, guidance_scale=2.5, negative_prompt_ids=one["neg"], **kw)
    assert torch.equal(lg[0], lg0[0]) and len(lg) == 6
    _, guided = drive(model, dev, one["ids"], one["images"], one["neg"], None, 2.5, 1)
    assert not np.array_equal(lg[0].float().cpu().numpy(), guided[0])                      # (log_softmax blends are not the raw row)
    assert float(torch.logsumexp(lg[3].double(), -1).abs().max()) > 1e-3                   # a later step's row is raw too, not normalised
    skw = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=40, guidance_scale=2.0, negative_prompt_ids=one["neg"], **kw)
    a, la = model.generate(one["ids"], seed=7, **skw)
    b, lb = model.generate(one["ids"], seed=7, **skw)
    c, _ = model.generate(one["ids"], seed=8, **skw)
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(la, lb)) and not torch.equal(a, c)
    assert len(model.kv.free) == model.kv.num_pages


def test_logprobs_are_those_of_the_guided_row(dev, model, two):
    """return_logprobs and top_logprobs describe the guided row, which is what every stage behind the combine sees: checked against
    ops.logprob_rows over the driven loop's guided rows (top ids, top log-probabilities and ranks bit for bit -- the same kernel --
    and the sampler's own log-probability within the two kernels' bounds)."""
    from vitron_amd import ops
    L0, n_new, scale = two["ids"].shape[1], 5, 2.0
    want, guided = drive(model, dev, two["ids"], None, two["neg"], None, scale, n_new)
    out, lp, top = model.generate(two["ids"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, guidance_scale=scale,
                                  negative_prompt_ids=two["neg"], return_logprobs=True, top_logprobs=4)
    assert [_new(out, L0, b) for b in range(2)] == want
    lp = lp.cpu().numpy()
    for st in range(n_new):
        rows = torch.from_numpy(guided[st]).to(dev)
        tgt = torch.tensor([want[b][st] for b in range(2)], dtype=torch.int32, device=dev)
        ref = ops.logprob_rows(rows, tgt, 4, return_rank=True)
        assert torch.equal(top["top_ids"][:, st], ref["top_ids"]) and torch.equal(top["rank"][:, st], ref["rank"])
        assert torch.equal(top["top_logprobs"][:, st].view(torch.int32), ref["top_logprobs"].view(torch.int32))
        assert top["rank"][:, st].cpu().tolist() == [1, 1]                                 # greedy: the pick is the guided row's best
        lp64 = LR.target_lp(guided[st], tgt.cpu().numpy())
        bound = SR.logprob_bound(guided[st], tgt.cpu().numpy()) + LR.logprob_bound(guided[st], lp64, LR.lse_chain(TV, True))
        assert (np.abs(lp[:, st] - ref["logprob"].cpu().numpy()) <= bound).all(), (st, lp[:, st], ref["logprob"], bound)
    assert len(model.kv.free) == model.kv.num_pages


def test_plausibility_one_leaves_the_conditional_argmax(dev, model, one):
    """beta = 1: only the conditional row's maximum survives the cut, so sampling with any seed returns the conditional arg-max of every
    step (read from return_logits, which stay conditional), whatever the scale prefers. beta = 0 is the call without the argument."""
    kw = dict(images=one["images"], max_new_tokens=6, eos_token_id=-1, negative_prompt_ids=one["neg"], guidance_scale=3.0)
    L0 = one["ids"].shape[1]
    for seed in (1, 2):
        out, lg = model.generate(one["ids"], do_sample=True, temperature=1.3, top_k=0, seed=seed, guidance_plausibility=1.0, return_logits=True, **kw)
        assert _new(out, L0) == [int(torch.argmax(x[0])) for x in lg]
    base = model.generate(one["ids"], do_sample=True, temperature=1.3, top_k=0, seed=1, **kw)
    assert torch.equal(model.generate(one["ids"], do_sample=True, temperature=1.3, top_k=0, seed=1, guidance_plausibility=0.0, **kw), base)
    # a static mask is the base of the cut's mask: with beta = 1 and the conditional arg-max allowed alone, it is the pick; suppressed
    # under a weak cut, it is not
    _, lg0 = model.generate(one["ids"], do_sample=False, return_logits=True, **kw)
    top0 = int(torch.argmax(lg0[0][0]))
    out = model.generate(one["ids"], do_sample=False, guidance_plausibility=1e-4, suppress_tokens=[top0], **kw)
    assert _new(out, L0)[0] != top0
    out = model.generate(one["ids"], do_sample=True, seed=3, guidance_plausibility=1.0, begin_suppress_tokens=[(top0 + 1) % TV], **kw)
    assert _new(out, L0)[0] == top0
    assert len(model.kv.free) == model.kv.num_pages


def test_composition_with_ngram_ban_and_choices(dev, model, one):
    """The guided row is what the later stages see: with no_repeat_ngram_size and with choices the ids equal the driven loop whose pick
    is the same chain (vt_ban_rows / the choices' masks in front of vt_sample_rows_allow over the guided rows)."""
    from vitron_amd import ops
    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.picker import device_history
    from vitron_amd.sampling import mask_words, pack_ban_rows, pack_fsm_rows, pack_sample_rows
    L0, n_new, scale = one["ids"].shape[1], 8, 2.5
    kw = dict(images=one["images"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, guidance_scale=scale, negative_prompt_ids=one["neg"])
    greedy = pack_sample_rows([(0.0, 0, 1.0, 1.0, 0, 0, 0, 0, 0)], dev)
    # -- no_repeat_ngram_size = 1: no id twice, the prompt's ids (sentinel included) count
    hist, lens = device_history(one["ids"], n_new)
    work = torch.empty((1, mask_words(TV)), dtype=torch.int32, device=dev)

    def pick_ban(st, c):
        ops.ban_rows(pack_ban_rows([(hist.data_ptr(), lens[0] + st, 0, work.data_ptr(), 1, 0, 0, 0)], dev), 1, TV)
        nxt = ops.sample_rows(c, greedy, allow=[work[0]])
        hist[0, lens[0] + st:lens[0] + st + 1] = nxt
        return nxt
    want, _ = drive(model, dev, one["ids"], one["images"], one["neg"], None, scale, n_new, pick=pick_ban)
    got = _new(model.generate(one["ids"], no_repeat_ngram_size=1, **kw), L0)
    assert got == want[0] and len(set(got)) == n_new, (got, want)
    # -- choices: the reply is one of them, then EOS
    choices = [[40, 41, 42], [40, 77], [300], [301, 5, 6, 7]]
    A = TokenAutomaton.from_choices(choices)
    cell = torch.tensor([A.start, 0], dtype=torch.int32).to(dev)
    gen = torch.zeros((n_new,), dtype=torch.int32, device=dev)
    fwork = torch.empty((mask_words(TV),), dtype=torch.int32, device=dev)

    def pick_fsm(st, c):
        ops.fsm_rows(pack_fsm_rows([(gen.data_ptr() if st else 0, st, cell.data_ptr(), 0, fwork.data_ptr(), *A.row_fields(dev), [2])], dev), 1, TV)
        nxt = ops.sample_rows(c, greedy, allow=[fwork])
        gen[st:st + 1] = nxt
        return nxt
    want, _ = drive(model, dev, one["ids"], one["images"], one["neg"], None, scale, 6, pick=pick_fsm)
    kw["eos_token_id"], kw["max_new_tokens"] = 2, 6
    got = _new(model.generate(one["ids"], choices=choices, **kw), L0)
    assert got[-1] == 2 and got[:-1] in choices and got == want[0][:len(got)], (got, want)
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_request_equals_solo_generate(dev, model, one, two):
    """A guided engine request returns its solo generate(guidance_scale=, negative_prompt_ids=) while an unguided request joins and
    leaves; that neighbour returns its own solo ids; a guided request takes two of max_batch's rows; every page is back in the pool
    after the requests retire, after a cancel and after a request fails on its own. An engine without a guided request emits what it
    emitted before."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    ids, neg = two["ids"][:1], two["neg"][:1]
    nb = _ids(531, 18).to(dev)
    L0 = ids.shape[1]
    solo = _new(model.generate(ids, do_sample=False, max_new_tokens=8, eos_token_id=-1, guidance_scale=2.5, negative_prompt_ids=neg), L0)
    solo_d = _new(model.generate(ids, do_sample=False, max_new_tokens=6, eos_token_id=-1, guidance_scale=1.5), L0)
    solo_s = _new(model.generate(ids, do_sample=True, temperature=0.8, top_p=0.9, top_k=30, seed=5, max_new_tokens=7, eos_token_id=-1,
                                 guidance_scale=2.0, negative_prompt_ids=neg), L0)
    solo_nb = _new(model.generate(nb, do_sample=False, max_new_tokens=4, eos_token_id=-1), nb.shape[1])
    plain = _new(model.generate(ids, do_sample=False, max_new_tokens=8, eos_token_id=-1), L0)
    assert solo != plain
    eng = ServingEngine(model, max_batch=7, kv_pages=64)
    g = eng.submit(ids, None, None, 8, eos_token_id=-1, sampling=SamplingParams(guidance_scale=2.5, negative_prompt_ids=neg))
    seen, steps = {}, 0
    while eng.pending():
        if steps == 2:                                                                     # they join a running guided request
            n = eng.submit(nb, None, None, 4, eos_token_id=-1)
            d = eng.submit(ids, None, None, 6, eos_token_id=-1, sampling=SamplingParams(guidance_scale=1.5))
            s = eng.submit(ids, None, None, 7, eos_token_id=-1,
                           sampling=SamplingParams(temperature=0.8, top_p=0.9, top_k=30, seed=5, guidance_scale=2.0, negative_prompt_ids=neg))
            w = eng.submit(ids, None, None, 8, eos_token_id=-1, sampling=SamplingParams(guidance_scale=2.5, negative_prompt_ids=neg))
        for rid, t in eng.step():
            seen.setdefault(rid, []).append(t)
        if steps == 2:
            assert sum(q.rows for q in eng.active) == 7                                    # g 2 + n 1 + d 2 + s 2: max_batch counts rows,
            assert [q.rid for q in eng.waiting] == [w]                                     # so w's two more do not fit
            held = eng.waiting[0]
            assert eng.cancel(w) and held.neg_flat is None and not held.nseq.pages
        steps += 1
        assert steps < 50
    assert not eng.failed and w not in seen
    assert seen[g] == solo and seen[d] == solo_d and seen[s] == solo_s and seen[n] == solo_nb
    assert len(model.kv.free) == model.kv.num_pages
    # a forced failure of the request's own: its negative prompt runs past the rotary table -- both sequences' pages come back
    llama = model.model.llama
    long_neg = torch.randint(3, TV, (llama.rope_len + 1,), generator=torch.Generator().manual_seed(3)).tolist()
    eng = ServingEngine(model, max_batch=4, kv_pages=llama.rope_len // 64 + 16)
    bad = eng.submit(ids, None, None, 4, eos_token_id=-1, sampling=SamplingParams(guidance_scale=2.0, negative_prompt_ids=long_neg))
    ok = eng.submit(ids, None, None, 4, eos_token_id=-1)
    res = eng.run()
    assert bad in eng.failed and not eng.failed[bad].seq.pages and not eng.failed[bad].nseq.pages
    assert res[ok].tolist() == plain[:4]                                                   # no guided request is live: today's ids
    assert len(model.kv.free) == model.kv.num_pages


def test_refusals(dev, model, one):
    from vitron_amd.sampling import SamplingParams
    ids = one["ids"]
    kw = dict(images=one["images"], do_sample=False, max_new_tokens=2, eos_token_id=-1)
    free = len(model.kv.free) if model.kv is not None else None
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        model.generate(ids, num_beams=2, guidance_scale=2.0, negative_prompt_ids=one["neg"], **kw)
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        model.generate(torch.cat([ids, ids]), padded_batch=True, guidance_scale=2.0, **{**kw, "images": one["images"] * 2})
    with pytest.raises(ValueError, match="sentinel"):
        model.generate(torch.tensor([[1, 5, 6, -200]]).to(dev), guidance_scale=2.0, **kw)  # the default negative prompt would be the image
    with pytest.raises(ValueError, match="guidance_scale"):
        model.generate(ids, guidance_scale=float("nan"), **kw)
    with pytest.raises(ValueError, match="guidance_plausibility"):
        model.generate(ids, guidance_scale=2.0, guidance_plausibility=1.5, **kw)
    with pytest.raises(ValueError, match="needs guidance_scale"):
        model.generate(ids, negative_prompt_ids=one["neg"], **kw)
    with pytest.raises(ValueError, match="batch size 2"):
        model.generate(ids, guidance_scale=2.0, negative_prompt_ids=torch.cat([one["neg"], one["neg"]]), **kw)
    with pytest.raises(ValueError, match="empty"):
        model.generate(ids, guidance_scale=2.0, negative_prompt_ids=one["neg"][:, :0], **kw)
    with pytest.raises(NotImplementedError, match="guidance_plausibility"):
        SamplingParams(guidance_scale=2.0, guidance_plausibility=0.5)
    with pytest.raises(NotImplementedError, match="negative_images"):
        SamplingParams(guidance_scale=2.0, negative_prompt_ids=[3, 4], negative_images=one["images"])
    if free is not None:
        assert len(model.kv.free) == free
