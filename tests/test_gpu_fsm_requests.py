"""Guided decoding end to end on the tiny synthetic model (tests/allow_cases.py): generate(automaton=) replayed from its
returned logits through vt_sample_rows_allow under tests/fsm_ref.py's masks, generate(choices=) against the engine's existing host
path, ServingEngine requests with SamplingParams(automaton=) beside other requests, their accounting and the release of their device
buffers, the compositions with no_repeat_ngram_size and min_new_tokens, the refusals."""
import numpy as np
import pytest
import torch

from tests import fsm_ref as R
from tests.golden import cases as G
from tests.allow_cases import tiny_model

pytestmark = pytest.mark.gpu
TV = G.LLM["vocab_size"]
EOS = 2
S8 = [33, 64, 95, 160, 223, 320, 415, 511]


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return tiny_model(dev)


def _prompt(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [1] + [t for t in torch.randint(3, TV, (n,), generator=g).tolist() if t not in S8]


def _ref(A, eos):
    return R.table(A.offsets.tolist(), A.edge_tok.tolist(), A.edge_next.tolist(), A.state_info().tolist(), eos=eos)


def _new(out, L0, b=0):
    return out[b, L0:].cpu().tolist()


@pytest.fixture(scope="module")
def free(dev, model):
    """An unconstrained greedy run of two prompts with its logits: what the automata below are chosen from"""
    pa, pb = _prompt(301, 14), _prompt(302, 14)
    n = min(len(pa), len(pb))
    ids = torch.tensor([pa[:n], pb[:n]]).to(dev)
    out, logits = model.generate(ids, do_sample=False, max_new_tokens=4, eos_token_id=-1, return_logits=True)
    return ids, out[:, n:].cpu().tolist(), [lg.float().cpu().numpy() for lg in logits]


def _biting_automaton(free):
    """s0 --(eight ids, none of them a row's unconstrained first pick)--> s1 --(anything but ten ids)--> s2 --(anything)--> s3, accepting, where
    only EOS may follow: a reply is three tokens and EOS."""
    from vitron_amd.automaton import TokenAutomaton
    _, toks, logits = free
    first = {int(np.argmax(logits[0][b])) for b in range(2)}
    assert first == {toks[0][0], toks[1][0]}
    s0 = [t for t in range(100, 400, 7) if t not in first and t != EOS][:8]
    order = np.argsort(-logits[0][0])
    banned1 = sorted(int(t) for t in order[:10] if t != EOS)                               # s1 forbids ids the model likes
    return TokenAutomaton.from_states([{t: 1 for t in s0}, {t: -1 for t in banned1}, {}, {}], [-1, 2, 3, -1], [0, 0, 0, 1]), first


@pytest.mark.parametrize("sampled", (False, True))
def test_generate_replays_from_its_logits_under_the_reference_masks(dev, model, free, sampled):
    """generate(automaton=A) at B = 2: replayed from the returned logits, every token is what vt_sample_rows_allow picks under fsm_ref's
    mask for the state the row's earlier tokens lead to; the mask bites (the unconstrained arg-max of step 0 is forbidden); the reply
    ends with EOS in an accepting state."""
    from vitron_amd import ops
    from vitron_amd.sampling import pack_sample_rows
    ids, _, _ = free
    A, first = _biting_automaton(free)
    a = _ref(A, [EOS])
    kw = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=20, seed=11) if sampled else dict(do_sample=False)
    out, logits = model.generate(ids, automaton=A, max_new_tokens=8, eos_token_id=EOS, return_logits=True, **kw)
    L0 = ids.shape[1]
    new = [_new(out, L0, b) for b in range(2)]
    assert len(logits) == 4 and all(len(r) == 4 for r in new), new                         # three tokens and EOS, then the call stops
    state = [A.start, A.start]
    bites = 0
    for st in range(4):
        masks = [R.mask(a, state[b], TV) for b in range(2)]
        for b in range(2):
            top = int(np.argmax(logits[st][b].float().cpu().numpy()))
            bites += int((masks[b][top >> 5] >> (top & 31)) & 1) == 0                     # the unconstrained pick is forbidden here
        T, k, p, seed = (0.9, 20, 0.95, 11) if sampled else (0.0, 0, 1.0, 0)
        rows = pack_sample_rows([(T, k, p, 1.0, seed, st, b, 0, 0) for b in range(2)], dev)
        want = ops.sample_rows(logits[st].contiguous(), rows, allow=[torch.from_numpy(m.view(np.int32)).to(dev) for m in masks]).cpu().tolist()
        for b in range(2):
            assert new[b][st] == want[b], (st, b, new[b], want)
            assert (masks[b][want[b] >> 5] >> (want[b] & 31)) & 1                          # (the replayed pick is an allowed id)
            state[b] = R.step(a, state[b], new[b][st])
            assert state[b] >= 0
    assert bites >= 2 and all(r[0] not in first for r in new)
    assert all(r[3] == EOS and A.accept[A.walk(r[:3], [EOS])] for r in new)
    assert len(model.kv.free) == model.kv.num_pages


def test_generate_choices_equals_the_engines_host_path(dev, model):
    """generate(choices=c) (the trie as an automaton, on the device) returns what a ServingEngine request with the existing
    SamplingParams(choices=c) returns (the host trie, one mask upload per step), token for token, under greedy decoding."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    choices = [[40, 41, 42], [40, 77], [300], [301, 5, 6, 7]]
    for seed in (311, 312):
        ids = torch.tensor([_prompt(seed, 12)]).to(dev)
        got = _new(model.generate(ids, do_sample=False, choices=choices, max_new_tokens=6, eos_token_id=EOS), ids.shape[1])
        eng = ServingEngine(model, max_batch=2, kv_pages=32)
        rid = eng.submit(ids, None, None, 6, eos_token_id=EOS, sampling=SamplingParams(choices=choices))
        want = eng.run()[rid].tolist()
        assert got == want and got[-1] == EOS and got[:-1] in choices, (got, want)
        assert eng.finished[rid].mask_uploads == len(want)                                 # the host path keeps its accounting
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_request_equals_solo_generate_beside_a_neighbour(dev, model, free):
    """An engine request with SamplingParams(automaton=A) returns its solo generate(automaton=A), greedy and sampled, next to an
    unconstrained neighbour whose tokens equal its own solo run; the request costs no mask upload and its cell, working mask and
    generated ids are released when it retires. A waiting request that is cancelled holds nothing."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    A, _ = _biting_automaton(free)
    ids = free[0][:1]
    nb_ids = torch.tensor([_prompt(321, 20)]).to(dev)
    L0 = ids.shape[1]
    solo = _new(model.generate(ids, do_sample=False, automaton=A, max_new_tokens=8, eos_token_id=EOS), L0)
    sp_s = SamplingParams(automaton=A, temperature=0.8, top_p=0.9, top_k=30, seed=5)
    solo_s = _new(model.generate(ids, do_sample=True, temperature=0.8, top_p=0.9, top_k=30, seed=5, automaton=A, max_new_tokens=8,
                                 eos_token_id=EOS), L0)
    solo_nb = _new(model.generate(nb_ids, do_sample=False, max_new_tokens=7, eos_token_id=-1), nb_ids.shape[1])
    assert len(solo) == 4 and solo[-1] == EOS and len(solo_s) == 4 and solo_s[-1] == EOS
    eng = ServingEngine(model, max_batch=3, kv_pages=64)
    n = eng.submit(nb_ids, None, None, 7, eos_token_id=-1)
    seen, steps = {}, 0
    while eng.pending():
        if steps == 1:
            g = eng.submit(ids, None, None, 8, eos_token_id=EOS, sampling=SamplingParams(automaton=A))
            s = eng.submit(ids, None, None, 8, eos_token_id=EOS, sampling=sp_s)
            w = eng.submit(ids, None, None, 8, eos_token_id=EOS, sampling=SamplingParams(automaton=A))    # max_batch 3: it waits
        for rid, t in eng.step():
            seen.setdefault(rid, []).append(t)
        if steps == 2:
            live = [q for q in eng.active if q.rid == g][0]
            assert live.fsm_cell is not None and live.fsm_mask is not None and live.gen is not None and live.hist is None
            assert live.fsm_cell.cpu().tolist() == [A.walk(live.tokens[:live.gen_len], [EOS]), live.gen_len]
            held = [q for q in eng.waiting if q.rid == w][0]
            assert eng.cancel(w) and held.fsm_cell is None and held.fsm_mask is None and held.gen is None
        steps += 1
        assert steps < 50
    assert not eng.failed and w not in seen
    assert seen[g] == solo and seen[s] == solo_s and seen[n] == solo_nb
    for rid in (g, s):
        q = eng.finished[rid]
        assert q.mask_uploads == 0 and q.fsm_cell is None and q.fsm_mask is None and q.gen is None and q.allow_cur is None
    assert len(A._device) == 1                                                            # one set of tables serves every request
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_failure_releases_the_buffers(dev, model, free):
    """A request with an automaton that fails on its own (its allowed_tokens_fn leaves nothing after one token) gives its cell and mask
    back like its other buffers."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    A, _ = _biting_automaton(free)
    eng = ServingEngine(model, max_batch=2, kv_pages=32)
    bad = eng.submit(free[0][:1], None, None, 8, eos_token_id=EOS,
                     sampling=SamplingParams(automaton=A, allowed_tokens_fn=lambda toks: [] if len(toks) == 1 else None))
    eng.run()
    q = eng.failed[bad]
    assert isinstance(q.error, ValueError) and len(q.tokens) == 1 and q.fsm_cell is None and q.fsm_mask is None and q.gen is None
    assert len(model.kv.free) == model.kv.num_pages


def test_automaton_with_no_repeat_ngram_size(dev, model):
    """An automaton that holds the reply to eight ids for ever is generate(allowed_token_ids=those eight): with no_repeat_ngram_size=2 on
    top, vt_ban_rows takes the automaton's working mask as its base and the run equals generate(allowed_token_ids=, no_repeat_ngram_size=2)
    token for token -- and differs from the run without the ban (its premise: the free run closes a bigram twice). The engine agrees."""
    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    A = TokenAutomaton.from_states([{t: 0 for t in S8}], [-1], [0])
    g = torch.Generator().manual_seed(94)
    prompt = [1] + [t for t in torch.randint(3, TV, (14,), generator=g).tolist() if t not in S8]
    ids = torch.tensor([prompt]).to(dev)
    L0, n_new = len(prompt), 12
    kw = dict(do_sample=False, max_new_tokens=n_new, eos_token_id=-1)
    held = _new(model.generate(ids, allowed_token_ids=S8, **kw), L0)
    want = _new(model.generate(ids, allowed_token_ids=S8, no_repeat_ngram_size=2, **kw), L0)
    assert want != held
    assert _new(model.generate(ids, automaton=A, **kw), L0) == held
    assert _new(model.generate(ids, automaton=A, no_repeat_ngram_size=2, **kw), L0) == want
    # a static mask under both: suppress one of the eight ids -- base of the automaton's mask, which is the base of the ban's
    want7 = _new(model.generate(ids, allowed_token_ids=[t for t in S8 if t != want[0]], no_repeat_ngram_size=2, **kw), L0)
    assert _new(model.generate(ids, automaton=A, suppress_tokens=[want[0]], no_repeat_ngram_size=2, **kw), L0) == want7 != want
    eng = ServingEngine(model, max_batch=2, kv_pages=32)
    rid = eng.submit(ids, None, None, n_new, eos_token_id=-1, sampling=SamplingParams(automaton=A, no_repeat_ngram_size=2))
    rid7 = eng.submit(ids, None, None, n_new, eos_token_id=-1,
                      sampling=SamplingParams(automaton=A, no_repeat_ngram_size=2, banned_token_ids=[want[0]]))
    out = eng.run()
    assert out[rid].tolist() == want and out[rid7].tolist() == want7
    assert eng.finished[rid].mask_uploads == 0 and eng.finished[rid7].mask_uploads == 1   # the static mask: uploaded once
    assert len(model.kv.free) == model.kv.num_pages


def test_automaton_with_min_new_tokens(dev, model, free):
    """The EOS id is the model's own first pick and the automaton's only state accepts: without min_new_tokens the reply is EOS at once;
    with min_new_tokens=3 EOS is withheld in the accepting state for three tokens (they come from the four listed ids) and allowed
    from the fourth on; replayed from the logits."""
    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    ids, toks, _ = free
    ids = ids[:1]
    L0 = ids.shape[1]
    e = toks[0][0]                                                                        # the unconstrained first pick serves as the EOS id
    S4 = [t for t in (120, 121, 250, 251, 252) if t != e][:4]
    A = TokenAutomaton.from_states([{t: 0 for t in S4}], [-1], [1])
    assert _new(model.generate(ids, do_sample=False, automaton=A, max_new_tokens=6, eos_token_id=e), L0) == [e]
    out, logits = model.generate(ids, do_sample=False, automaton=A, min_new_tokens=3, max_new_tokens=6, eos_token_id=e, return_logits=True)
    new = _new(out, L0)
    assert len(new) >= 4 and all(t in S4 for t in new[:3])
    for st, t in enumerate(new):
        x = logits[st][0].float().cpu().numpy()
        allowed = S4 + ([e] if st >= 3 else [])
        assert t == min(i for i in allowed if x[i] == x[allowed].max()), (st, t)          # the first arg-max over the allowed ids
    eng = ServingEngine(model, max_batch=2, kv_pages=32)
    rid = eng.submit(ids, None, None, 6, eos_token_id=e, sampling=SamplingParams(automaton=A, min_new_tokens=3))
    assert eng.run()[rid].tolist() == new
    assert len(model.kv.free) == model.kv.num_pages


def test_refusals(dev, model):
    from vitron_amd.automaton import TokenAutomaton
    A = TokenAutomaton.from_choices([[40, 41], [77]])
    ids = torch.tensor([[1, 9, 8, 7, 9]]).to(dev)
    with pytest.raises(NotImplementedError, match="automaton"):
        model.generate(ids, do_sample=False, max_new_tokens=2, num_beams=2, automaton=A, eos_token_id=EOS)
    with pytest.raises(NotImplementedError, match="automaton"):
        model.generate(torch.cat([ids, ids], 0), do_sample=False, max_new_tokens=2, padded_batch=True, automaton=A, eos_token_id=EOS)
    with pytest.raises(ValueError, match="at most 4"):
        model.generate(ids, do_sample=False, max_new_tokens=2, automaton=A, eos_token_id=[2, 3, 4, 5, 6])
    with pytest.raises(ValueError, match="start state allows no token"):
        model.generate(ids, do_sample=False, max_new_tokens=2, choices=[[TV + 1]], eos_token_id=EOS)
    with pytest.raises(ValueError, match="EOS id inside"):
        model.generate(ids, do_sample=False, max_new_tokens=2, automaton=A, eos_token_id=-1)
    plain = model.generate(ids, do_sample=False, max_new_tokens=4, eos_token_id=-1)
    assert torch.equal(model.generate(ids, do_sample=False, max_new_tokens=4, eos_token_id=-1, automaton=None, choices=None), plain)
    assert len(model.kv.free) == model.kv.num_pages
