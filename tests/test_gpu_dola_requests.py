"""DoLa end to end on the tiny synthetic model with eight decoder layers (tests/dola_cases.py): generate(dola_layers=)
against a loop this file drives itself (llama_forward with the logit-row trace, ops.gemm, ops.dola_rows, ops.argmax), dola_layers=None
against the call without the argument, every row of a batch against the same call on that row alone, last_dola_layers, a single
candidate, seeded sampling, the compositions with repetition_penalty, no_repeat_ngram_size and choices, return_logits, ServingEngine
requests with SamplingParams(dola_layers=) beside other requests and the return of their pages, the refusals."""
import numpy as np
import pytest
import torch

from tests.dola_cases import LAYERS, drive, tiny_model8
from tests.golden import cases as G

pytestmark = pytest.mark.gpu
TV = G.LLM["vocab_size"]


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return tiny_model8(dev)


def _ids(seed, n, image=False):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([[1] + ([-200] if image else []) + torch.randint(3, TV, (n,), generator=g).tolist()])


def _new(out, L0, b=0):
    return out[b, L0:].cpu().tolist()


@pytest.fixture(scope="module")
def one(dev):
    """B = 1: a prompt with an image"""
    img = torch.randn((3, 56, 56), generator=torch.Generator().manual_seed(602)).bfloat16().to(dev)
    return dict(ids=_ids(601, 10, image=True).to(dev), images=[img], mask=None)


@pytest.fixture(scope="module")
def two(dev):
    """B = 2: ragged text prompts, right-padded under an attention mask"""
    a, b = _ids(611, 14), _ids(612, 9)
    ids = torch.zeros((2, 15), dtype=torch.long)
    mask = torch.zeros((2, 15), dtype=torch.long)
    ids[0, :15], mask[0, :15] = a[0], 1
    ids[1, :10], mask[1, :10] = b[0], 1
    return dict(ids=ids.to(dev), images=None, mask=mask.to(dev), solo=[a.to(dev), b.to(dev)])


def _layers(model, spec):
    from vitron_amd.sampling import dola_candidate_layers
    return list(dola_candidate_layers(spec, LAYERS))


def test_off_is_todays_call(dev, model, one):
    """dola_layers=None: the ids and the returned logits of the call without the argument, bit for bit."""
    kw = dict(images=one["images"], do_sample=False, max_new_tokens=5, eos_token_id=-1, return_logits=True)
    out0, lg0 = model.generate(one["ids"], **kw)
    for extra in (dict(dola_layers=None), dict(dola_layers=None, dola_relative_top=0.3)):
        out, lg = model.generate(one["ids"], **kw, **extra)
        assert torch.equal(out, out0) and len(lg) == len(lg0) and all(torch.equal(a, b) for a, b in zip(lg, lg0))
        assert model.last_dola_layers is None
    assert len(model.kv.free) == model.kv.num_pages


@pytest.mark.parametrize("spec", ("low", "high", [6]), ids=("low", "high", "one"))
@pytest.mark.parametrize("case", ("one", "two"))
def test_greedy_ids_equal_the_driven_loop(dev, model, one, two, case, spec):
    """The greedy ids and the chosen layers are those of the driven loop -- the same launches over the same sequences -- at B = 1 with an
    image and at B = 2 with ragged prompts; each row of B = 2 gets the ids and layers of the same call on that row alone; a list
    naming one layer skips the divergence and still contrasts."""
    d = one if case == "one" else two
    B, L0, n_new = d["ids"].shape[0], d["ids"].shape[1], 6
    layers = _layers(model, spec)
    want, chosen, rows, finals = drive(model, dev, d["ids"], d["images"], d["mask"], layers, n_new)
    out = model.generate(d["ids"], images=d["images"], attention_mask=d["mask"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1,
                         dola_layers=spec)
    got = [_new(out, L0, b) for b in range(B)]
    assert got == want, (got, want)
    assert model.last_dola_layers.shape == (B, n_new) and model.last_dola_layers.cpu().tolist() == chosen
    assert {l for c in chosen for l in c} <= set(layers)
    assert not np.array_equal(rows[0], finals[0]) and np.isneginf(rows[0]).any()           # the contrast ran, and it filtered
    if case == "two":
        for b in range(2):
            solo = model.generate(d["solo"][b], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, dola_layers=spec)
            assert _new(solo, d["solo"][b].shape[1]) == got[b], (b, spec)
            assert model.last_dola_layers.cpu().tolist() == [chosen[b]]
    assert len(model.kv.free) == model.kv.num_pages


def test_return_logits_stay_final_and_sampling_is_reproducible(dev, model, one):
    """return_logits are the model's final rows, cloned before the contrast: step 0 is bit for bit the plain call's, and no row holds
    the -inf the contrast writes. Sampling with a seed is reproducible; another seed gives another reply."""
    kw = dict(images=one["images"], max_new_tokens=6, eos_token_id=-1, return_logits=True)
    _, lg0 = model.generate(one["ids"], do_sample=False, **kw)
    out, lg = model.generate(one["ids"], do_sample=False, dola_layers="high", **kw)
    assert torch.equal(lg[0], lg0[0]) and len(lg) == 6 and all(bool(torch.isfinite(x).all()) for x in lg)
    skw = dict(do_sample=True, temperature=1.2, top_p=0.98, top_k=0, dola_layers="low", dola_relative_top=0.01, **kw)
    a, la = model.generate(one["ids"], seed=7, **skw)
    b, lb = model.generate(one["ids"], seed=7, **skw)
    c, _ = model.generate(one["ids"], seed=8, **skw)
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(la, lb)) and not torch.equal(a, c)
    # relative_top = 1 keeps only the final row's maximum: sampling with any seed returns the final arg-max of every step
    out, lg = model.generate(one["ids"], do_sample=True, temperature=1.3, top_k=0, seed=3, dola_layers="high", dola_relative_top=1.0, **kw)
    assert _new(out, one["ids"].shape[1]) == [int(torch.argmax(x[0])) for x in lg]
    assert len(model.kv.free) == model.kv.num_pages


def test_composition_with_penalty_ngram_ban_and_choices(dev, model, one):
    """The contrasted row and its mask are what the later stages see: with repetition_penalty, with no_repeat_ngram_size and with choices
    the ids equal the driven loop whose pick is the same chain over the contrasted rows, the kept-token mask as the `base`."""
    from vitron_amd import ops
    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.picker import device_history
    from vitron_amd.sampling import mask_words, pack_ban_rows, pack_fsm_rows, pack_sample_rows
    L0, n_new = one["ids"].shape[1], 8
    layers = _layers(model, "high")
    kw = dict(images=one["images"], do_sample=False, max_new_tokens=n_new, eos_token_id=-1, dola_layers="high")
    plain = _new(model.generate(one["ids"], **kw), L0)
    # -- repetition_penalty: the penalty history is the non-negative prompt ids, then the picks
    hist, lens = device_history(one["ids"], n_new, nonneg=True)

    def pick_pen(st, f, masks):
        row = pack_sample_rows([(0.0, 0, 1.0, 1.7, 0, st, 0, hist.data_ptr(), lens[0] + st)], dev)
        nxt = ops.sample_rows(f, row, allow=[masks[0]])
        hist[0, lens[0] + st:lens[0] + st + 1] = nxt
        return nxt
    want, _, _, _ = drive(model, dev, one["ids"], one["images"], None, layers, n_new, pick=pick_pen)
    got = _new(model.generate(one["ids"], repetition_penalty=1.7, **kw), L0)
    assert got == want[0], (got, want)
    # -- no_repeat_ngram_size = 1: no id twice, the prompt's ids (sentinel included) count; the ban starts from the kept-token mask
    greedy = pack_sample_rows([(0.0, 0, 1.0, 1.0, 0, 0, 0, 0, 0)], dev)
    bhist, blens = device_history(one["ids"], n_new)
    work = torch.empty((1, mask_words(TV)), dtype=torch.int32, device=dev)

    def pick_ban(st, f, masks):
        ops.ban_rows(pack_ban_rows([(bhist.data_ptr(), blens[0] + st, masks[0].data_ptr(), work.data_ptr(), 1, 0, 0, 0)], dev), 1, TV)
        nxt = ops.sample_rows(f, greedy, allow=[work[0]])
        bhist[0, blens[0] + st:blens[0] + st + 1] = nxt
        return nxt
    want, _, _, _ = drive(model, dev, one["ids"], one["images"], None, layers, n_new, pick=pick_ban)
    got = _new(model.generate(one["ids"], no_repeat_ngram_size=1, **kw), L0)
    assert got == want[0] and len(set(got)) == n_new, (got, want)
    # -- choices: the reply is one of them, then EOS. relative_top is tiny so that the choices' ids stay among the kept tokens
    choices = [[40, 41, 42], [40, 77], [300], [301, 5, 6, 7]]
    A = TokenAutomaton.from_choices(choices)
    cell = torch.tensor([A.start, 0], dtype=torch.int32).to(dev)
    gen = torch.zeros((n_new,), dtype=torch.int32, device=dev)
    fwork = torch.empty((mask_words(TV),), dtype=torch.int32, device=dev)

    def pick_fsm(st, f, masks):
        ops.fsm_rows(pack_fsm_rows([(gen.data_ptr() if st else 0, st, cell.data_ptr(), masks[0].data_ptr(), fwork.data_ptr(),
                                     *A.row_fields(dev), [2])], dev), 1, TV)
        nxt = ops.sample_rows(f, greedy, allow=[fwork])
        gen[st:st + 1] = nxt
        return nxt
    rt = 1e-30
    want, _, _, _ = drive(model, dev, one["ids"], one["images"], None, layers, 6, relative_top=rt, pick=pick_fsm)
    kw.update(eos_token_id=2, max_new_tokens=6, dola_relative_top=rt)
    got = _new(model.generate(one["ids"], choices=choices, **kw), L0)
    assert got[-1] == 2 and got[:-1] in choices and got == want[0][:len(got)], (got, want)
    assert plain is not None and len(model.kv.free) == model.kv.num_pages


def test_engine_request_equals_solo_generate(dev, model, two):
    """A DoLa engine request returns its solo generate(dola_layers=) while a plain request and other DoLa requests (another layer set, a
    sampled one) join and leave; the neighbour returns its own solo ids; a DoLa request takes one of max_batch's rows; every page is
    back in the pool after the requests retire, after a cancel and after a request fails on its own; an engine without a DoLa request
    emits what it emitted before."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    ids, nb = two["solo"]
    L0 = ids.shape[1]
    g_kw = dict(do_sample=False, eos_token_id=-1)
    solo = _new(model.generate(ids, max_new_tokens=8, dola_layers="high", **g_kw), L0)
    solo_l = _new(model.generate(ids, max_new_tokens=6, dola_layers=[1, 6, 3], dola_relative_top=0.3, **g_kw), L0)
    solo_s = _new(model.generate(ids, do_sample=True, temperature=0.8, top_p=0.9, top_k=30, seed=5, max_new_tokens=7, eos_token_id=-1,
                                 dola_layers="low"), L0)
    solo_nb = _new(model.generate(nb, max_new_tokens=4, **g_kw), nb.shape[1])
    plain = _new(model.generate(ids, max_new_tokens=8, **g_kw), L0)
    assert solo != plain
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    g = eng.submit(ids, None, None, 8, eos_token_id=-1, sampling=SamplingParams(dola_layers="high"))
    seen, steps = {}, 0
    while eng.pending():
        if steps == 2:                                                                     # they join a running DoLa request
            n = eng.submit(nb, None, None, 4, eos_token_id=-1)
            l = eng.submit(ids, None, None, 6, eos_token_id=-1, sampling=SamplingParams(dola_layers=[1, 6, 3], dola_relative_top=0.3))
            s = eng.submit(ids, None, None, 7, eos_token_id=-1,
                           sampling=SamplingParams(temperature=0.8, top_p=0.9, top_k=30, seed=5, dola_layers="low"))
            w = eng.submit(ids, None, None, 8, eos_token_id=-1, sampling=SamplingParams(dola_layers="high"))
        for rid, t in eng.step():
            seen.setdefault(rid, []).append(t)
        if steps == 2:
            assert sum(q.rows for q in eng.active) == 4 and [q.rid for q in eng.waiting] == [w]     # one row each: w does not fit
            assert eng._dola_layers(eng.active) == [0, 1, 2, 3, 4, 6]                       # the union of the live requests' layers
            assert eng.cancel(w)
        steps += 1
        assert steps < 50
    assert not eng.failed and w not in seen
    assert seen[g] == solo and seen[l] == solo_l and seen[s] == solo_s and seen[n] == solo_nb
    assert len(model.kv.free) == model.kv.num_pages
    # a forced failure of the request's own: its prompt runs past the rotary table -- its pages come back, the neighbour is served
    llama = model.model.llama
    long_ids = torch.randint(3, TV, (1, llama.rope_len + 1), generator=torch.Generator().manual_seed(3)).to(dev)
    eng = ServingEngine(model, max_batch=4, kv_pages=llama.rope_len // 64 + 16)
    bad = eng.submit(long_ids, None, None, 4, eos_token_id=-1, sampling=SamplingParams(dola_layers="high"))
    ok = eng.submit(ids, None, None, 4, eos_token_id=-1)
    res = eng.run()
    assert bad in eng.failed and not eng.failed[bad].seq.pages
    assert res[ok].tolist() == plain[:4]                                                   # no DoLa request is live: today's ids
    assert len(model.kv.free) == model.kv.num_pages


def test_refusals(dev, model, one):
    from vitron_amd.sampling import SamplingParams
    ids = one["ids"]
    kw = dict(images=one["images"], do_sample=False, max_new_tokens=2, eos_token_id=-1)
    free = len(model.kv.free) if model.kv is not None else None
    with pytest.raises(NotImplementedError, match="dola_layers"):
        model.generate(ids, num_beams=2, dola_layers="low", **kw)
    with pytest.raises(NotImplementedError, match="dola_layers.*padded_batch"):
        model.generate(torch.cat([ids, ids]), padded_batch=True, dola_layers="low", **{**kw, "images": one["images"] * 2})
    with pytest.raises(NotImplementedError, match="dola_layers.*guidance_scale"):
        model.generate(ids, guidance_scale=2.0, negative_prompt_ids=_ids(9, 4).to(dev), dola_layers="low", **kw)
    with pytest.raises(NotImplementedError, match="dola_layers.*penalty_alpha"):
        model.generate(ids, penalty_alpha=0.6, top_k=4, dola_layers="low", **kw)
    for bad in ("mid", [LAYERS], [], [2, 2]):
        with pytest.raises(ValueError, match="dola_layers"):
            model.generate(ids, dola_layers=bad, **kw)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="dola_relative_top"):
            model.generate(ids, dola_layers="low", dola_relative_top=bad, **kw)
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        SamplingParams(dola_layers="low", guidance_scale=2.0)
    if free is not None:
        assert len(model.kv.free) == free
