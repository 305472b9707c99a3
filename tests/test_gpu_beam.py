"""Beam search on the device. vt_beam_step against fp64 (the selected (beam, token) lists exactly, every score inside
the derived bound of tests/sample_ref.py plus one rounding), its tie rule and its refusals; vt_kv_copy_pages bit for bit on both pool
formats; BeamGroup keeps every beam's cache bit-equal to a fresh private-page sequence through 70 scripted reorders; generate(num_beams=3)
equals tests/beam_ref.py fed from ops.beam_step on fresh private-page sequences, to the id and the score bit; the refused combinations and
the error path leave the pool as it was."""
import numpy as np
import pytest
import torch

from tests import beam_ref
from tests import sample_ref as R
from tests.golden import cases

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
LEVEL = 0.25                 # spacing of the logit grid
BEAM_STEP = LEVEL / 16       # spacing of the beams' offsets: any two distinct candidate scores are >= 0.015625 apart


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- vt_beam_step ------------------------------------------------------------------------------------------------------------------------------
def _grid_rows(rows, V, seed):
    """fp32 [rows][V] on a grid of LEVEL: a bulk of low levels with many repeats, up to 40 planted peaks per row on levels of their own, two of
    them repeated (in-row ties among the best)"""
    g = np.random.default_rng(seed)
    x = g.integers(0, 40, (rows, V)).astype(np.float64)
    n_peaks = min(40, V - 8)
    for r in range(rows):
        pos = g.permutation(V)[:n_peaks + 2]
        x[r, pos[:n_peaks]] = 41 + g.permutation(n_peaks)
        x[r, pos[n_peaks]] = x[r, pos[0]]
        x[r, pos[n_peaks + 1]] = x[r, pos[3]]
    return (x * LEVEL).astype(np.float32)


def _beam_scores(x, beams_in):
    """beam scores that put beam b's candidates at (logit - 3 - b * BEAM_STEP) up to fp32's rounding of the score itself: the offsets of
    two beams differ by a multiple of BEAM_STEP that is no multiple of LEVEL, so no two candidates of different beams come closer"""
    lse = torch.logsumexp(torch.from_numpy(x).double(), -1).numpy()
    b = np.arange(x.shape[0]) % beams_in
    return (lse - 3.0 - b * BEAM_STEP).astype(np.float32)


def _reference(x, bs, groups, beams_in, n_out):
    """fp64: per group (scores, beams, tokens, rows) of the n_out best, descending, exact ties by the lower flat index"""
    V = x.shape[1]
    lp = R.logprob_ref(x)
    out = []
    for g in range(groups):
        s = (lp[g * beams_in:(g + 1) * beams_in] + bs[g * beams_in:(g + 1) * beams_in].astype(np.float64)[:, None]).reshape(-1)
        order = np.argsort(-s, kind="stable")[:n_out]
        d = np.diff(np.unique(s[np.argsort(-s, kind="stable")[:n_out + 1]]))
        assert d.size == 0 or d.min() >= 1e-2, "the inputs must keep distinct candidates 1e-2 apart"
        out.append((s[order], order // V, order % V))
    return out


SHAPES = [(64, 64), (97, 97), (1000, 1000), (32000, 32000), (32003, 32064), (50000, 50000), (33001, 33001)]


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("beams_in", [1, 2, 4, 16])
@pytest.mark.parametrize("V,ldl", SHAPES, ids=[f"V{v}" for v, _ in SHAPES])
def test_beam_step_against_fp64(dev, V, ldl, beams_in, groups):
    from vitron_amd import ops
    n_out = min(2 * beams_in, 32)
    rows = groups * beams_in
    x = _grid_rows(rows, V, 100 * beams_in + groups + V)
    bs = _beam_scores(x, beams_in)
    buf = torch.full((rows, ldl), 1e30, dtype=torch.float32)          # what lies between V and the row stride must never be read as a logit
    buf[:, :V] = torch.from_numpy(x)
    buf = buf.to(dev)
    ld = buf[:, :V]
    before = buf.clone()
    s, t, b = ops.beam_step(ld, torch.from_numpy(bs).to(dev), groups, beams_in, n_out)
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "logits were modified"
    s, t, b = s.cpu().numpy().astype(np.float64), t.cpu().numpy(), b.cpu().numpy()
    worst = 0.0
    for g, (rs, rb, rt) in enumerate(_reference(x, bs, groups, beams_in, n_out)):
        assert b[g].tolist() == rb.tolist() and t[g].tolist() == rt.tolist(), (g, b[g], rb, t[g], rt)
        r = g * beams_in + rb
        bound = R.logprob_bound(x[r], rt) + R.U * (np.abs(bs[r].astype(np.float64)) + np.abs(rs))
        err = np.abs(s[g] - rs)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (g, err, bound)
    print(f"beam_step V={V} beams_in={beams_in} groups={groups}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("V", [97, 32000, 50000])
def test_beam_step_tie_rule(dev, V):
    """identical rows with identical beam scores and repeated values: the lowest flat indices b * V + t, in index order -- also where the
    tie straddles rank n_out"""
    from vitron_amd import ops
    beams_in, n_out = 4, 8
    g = np.random.default_rng(V)
    row = g.integers(0, 30, V).astype(np.float32)
    top = g.permutation(V)[:5]
    row[top[:3]] = 50.0                  # 3 per row x 4 rows = 12 candidates tie for the best 8: the tie straddles rank n_out
    row[top[3:]] = 45.0
    x = np.stack([row] * beams_in)
    ld = torch.from_numpy(x).to(dev)
    s, t, b = ops.beam_step(ld, torch.full((beams_in,), -1.5, device=dev), 1, beams_in, n_out)
    flat = sorted(int(bb) * V + int(tt) for bb in range(beams_in) for tt in top[:3])[:n_out]
    assert (b[0].cpu().numpy() * V + t[0].cpu().numpy()).tolist() == flat
    assert len(set(s[0].cpu().tolist())) == 1
    # distinct beam scores: beam 2 first (its three ties in index order), then beam 0's, then two of beam 1's
    bs = torch.tensor([-1.0, -2.0, -0.5, -3.0], device=dev)
    s, t, b = ops.beam_step(ld, bs, 1, beams_in, n_out)
    want = [(2, i) for i in sorted(top[:3])] + [(0, i) for i in sorted(top[:3])] + [(1, i) for i in sorted(top[:3])][:2]
    assert list(zip(b[0].cpu().tolist(), t[0].cpu().tolist())) == [(bb, int(i)) for bb, i in want]
    # n_out = 1 with the tie inside one row: the first index
    s, t, b = ops.beam_step(ld[:1], bs[:1], 1, 1, 1)
    assert (int(b[0, 0]), int(t[0, 0])) == (0, int(min(top[:3])))


def test_beam_step_refusals(dev):
    from vitron_amd import _lib, ops
    lib = _lib.load_any()
    V = 64
    ld = torch.zeros((17, V), device=dev)
    bs = torch.zeros((17,), device=dev)
    outs = [torch.full((40,), -7, dtype=dt, device=dev) for dt in (torch.float32, torch.int32, torch.int32)]
    scratch = torch.zeros((1 << 16,), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(V_, beams_in, n_out):
        return lib.vt_beam_step(ld.data_ptr(), V, V_, 1, beams_in, bs.data_ptr(), n_out, outs[0].data_ptr(), outs[1].data_ptr(),
                                outs[2].data_ptr(), scratch.data_ptr(), scratch.numel() * 4, stream)
    assert call(V, 17, 2) == -1 and "beams_in" in _lib.last_error(lib)
    assert call(V, 2, 33) == -1 and "n_out" in _lib.last_error(lib)
    assert call(8, 4, 9) == -1 and "exceeds V" in _lib.last_error(lib)
    assert call(V, 0, 1) == -1 and call(V, 1, 0) == -1
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs), "a refused call wrote its outputs"
    with pytest.raises(_lib.VitronHipError):
        ops.beam_step(ld, bs, 1, 17, 2)
    with pytest.raises(_lib.VitronHipError):
        ops.beam_step(ld[:4], bs[:4], 1, 2, 4)          # rows != groups * beams_in
    assert call(V, 16, 32) == 0                         # the limits themselves are served
    assert lib.vt_beam_step_scratch_bytes(3, 16, 32) == 3 * 16 * 32 * 8


# ---- vt_kv_copy_pages ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_llama(dev):
    from vitron_amd import synth
    from vitron_amd.engine import PackedLlama
    made = {}

    def get(dt):
        if dt not in made:
            made[dt] = PackedLlama(synth.llama_state(cases.LLM, synth.make_generator(cases.SEED_LLM), **cases.LLM_INIT), cases.LLM, dev, dtype=dt)
        return made[dt]
    return get


@pytest.mark.parametrize("fmt", ["16bit", "fp8"])
def test_kv_copy_pages(dev, tiny_llama, fmt):
    from vitron_amd import _lib, ops
    from vitron_amd.engine import PagedKVCache
    llama = tiny_llama(torch.bfloat16)
    kv = PagedKVCache(llama, 8, kv_dtype=fmt)
    L, P = llama.L, 8
    assert (llama.L, llama.heads, llama.hd) == (2, 2, 128) and kv.k.element_size() == (1 if fmt == "fp8" else 2)
    page_bytes = llama.heads * 64 * llama.hd * kv.k.element_size()
    views = [p.view(torch.uint8).view(L, P, page_bytes) for p in (kv.k, kv.vt)]
    for i, v in enumerate(views):        # every byte of every page differs from its neighbours and from the same byte of every other page
        n = torch.arange(v.numel(), dtype=torch.int64, device=dev)
        v.view(-1).copy_((((n * 2654435761 + 97 * i) >> 7) & 0xFF).to(torch.uint8))
    # n = 0; n = 1; n = 5 with source 2 (and 0) used twice and the last page of the pool a destination; the last page alone
    for src, dst in [([], []), ([3], [5]), ([0, 2, 2, 6, 0], [1, 3, 5, 7, 4]), ([1], [7])]:
        before = [v.clone() for v in views]
        ops.kv_copy_pages(kv, src, dst)
        torch.cuda.synchronize()
        for v, b in zip(views, before):
            want = b.clone()
            for a, d in zip(src, dst):
                want[:, d] = b[:, a]
            assert torch.equal(v, want), (fmt, src, dst)
    lib = _lib.load_any()
    assert lib.vt_kv_copy_pages(kv.k.data_ptr(), kv.vt.data_ptr(), L, P, page_bytes, None, None, 0, torch.cuda.current_stream().cuda_stream) == 0
    for bad in (([8], [1]), ([1], [-1]), ([1, 2], [2, 3]), ([1, 2], [3, 3]), ([1], [2, 3])):     # the host wrapper raises first
        with pytest.raises(_lib.VitronHipError):
            ops.kv_copy_pages(kv, *bad)


# ---- BeamGroup ---------------------------------------------------------------------------------------------------------------------------------
K = 4
STEPS = 70
CHECK = {1, 2, 3, 62, 63, 64, 65, 66, 70}
PARENTS = [[0, 1, 2, 3], [2, 2, 2, 2], [1, 2, 3, 0], [0, 0, 3, 3]]


def _embed(llama, toks, dev):
    from vitron_amd import ops
    plan = torch.tensor([[0, int(t)] for t in toks], dtype=torch.int32).to(dev)
    return ops.embed_splice(llama.embed, None, None, plan)


@pytest.mark.parametrize("prompt_len", [63, 64, 65, 130])
@pytest.mark.parametrize("fmt", ["16bit", "fp8"])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_beam_group_keeps_every_cache_exact(dev, tiny_llama, dt, fmt, prompt_len):
    from vitron_amd.beam import BeamGroup
    from vitron_amd.engine import PagedKVCache, SequenceState, llama_forward
    llama = tiny_llama(dt)
    kv = PagedKVCache(llama, 40, kv_dtype=fmt)
    free0 = len(kv.free)
    g = torch.Generator().manual_seed(prompt_len)
    prompt = _embed(llama, torch.randint(3, cases.LLM["vocab_size"], (prompt_len,), generator=g).tolist(), dev)

    def prefilled():
        s = SequenceState()
        llama_forward(llama, kv, [s], prompt, [prompt_len])
        return s

    group = BeamGroup(llama, kv, prefilled(), K, STEPS)
    try:
        whole = prompt_len // 64
        assert all(s.pages[:whole] == group.shared and s.length == prompt_len for s in group.seqs)
        assert len({p for s in group.seqs for p in s.pages[whole:]}) == K * len(group.tails[0])       # every tail page has one owner
        hist = [[] for _ in range(K)]
        for t in range(1, STEPS + 1):
            toks = [(7 * t + 3 * s) % 90 + 5 for s in range(K)]
            got = llama_forward(llama, kv, group.seqs, _embed(llama, toks, dev), [1] * K)
            for s in range(K):
                hist[s].append(toks[s])
            if t in CHECK:
                fresh = [prefilled() for _ in range(K)]
                try:
                    for j in range(t):
                        want = llama_forward(llama, kv, fresh, _embed(llama, [hist[s][j] for s in range(K)], dev), [1] * K)
                finally:
                    for s in fresh:
                        kv.release(s.pages)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"step {t}: the group's logits differ from fresh sequences"
            parents = PARENTS[t % len(PARENTS)]
            slot_of_child = group.reorder(parents)
            new = [None] * K
            for c, s in enumerate(slot_of_child):
                new[s] = list(hist[parents[c]])
            hist = new
    finally:
        group.release()
    assert len(kv.free) == free0 and sorted(kv.free) == list(range(40))


# ---- generate(num_beams=...) ----------------------------------------------------------------------------------------------------------------
EOS = [7, 19, 33, 101]
NB, MAX_NEW = 3, 12


@pytest.fixture(scope="module")
def model(dev):
    from tests.allow_cases import tiny_model
    return tiny_model(dev)


def _prompt_rows(model, input_ids, attention_mask, images):
    """the packed prompt rows and lengths generate() prefills (its own steps, restated)"""
    dev = model.device
    input_ids = input_ids.to(dev)
    B = input_ids.shape[0]
    (_, _, _, _, embeds, _) = model.prepare_inputs_labels_for_multimodal(input_ids, None, attention_mask, None, None, images, None)
    if embeds is None:
        embeds = model.model.embed_tokens(input_ids)
        mask = attention_mask.to(torch.int32).tolist() if attention_mask is not None else [[1] * input_ids.shape[1]] * B
    else:
        mask = model._last_splice[0]
    S, H = embeds.shape[1], embeds.shape[2]
    idx = [b * S + j for b in range(B) for j in range(S) if mask[b][j]]
    flat = embeds.reshape(B * S, H).to(model.model.llama.dtype)[torch.tensor(idx, device=dev)].contiguous()
    return flat, [sum(r) for r in mask]


def _reference_generate(model, input_ids, attention_mask, images, nrs, lp, es):
    """tests/beam_ref.py with candidates from ops.beam_step on the logits of FRESH private-page sequences: every call prefills the prompts
    once per beam and replays every hypothesis token by token, in passes shaped like generate's (the groups live at that step, k rows each).
    Only the scorer and the page management differ from generate()."""
    from vitron_amd import ops
    from vitron_amd.engine import SequenceState, llama_forward
    dev = model.device
    llama, kv = model.model.llama, model.kv
    flat, lens = _prompt_rows(model, input_ids, attention_mask, images)
    B = len(lens)
    n = beam_ref.num_candidates(NB, len(EOS))
    live_at = []                 # the groups live at call 0, 1, ...

    def topk(live):
        groups = [g for g, _, _ in live]
        live_at.append(groups)
        hyps = {g: h for g, h, _ in live}
        scores = {g: s for g, _, s in live}
        t = len(live_at) - 1
        if t == 0:
            seqs = [SequenceState() for _ in range(B)]
            try:
                logits = llama_forward(llama, kv, seqs, flat, lens)
                s, tok, b = ops.beam_step(logits, torch.zeros((B,), device=dev), B, 1, n)
            finally:
                for q in seqs:
                    kv.release(q.pages)
            return [(s[g].cpu().tolist(), b[g].cpu().tolist(), tok[g].cpu().tolist()) for g in groups]
        fresh = [[SequenceState() for _ in range(B)] for _ in range(NB)]
        try:
            for beam in range(NB):
                llama_forward(llama, kv, fresh[beam], flat, lens)
            for j in range(1, t + 1):
                rows = live_at[j]
                toks = [hyps[g][beam][j - 1] if g in hyps else 5 for g in rows for beam in range(NB)]
                x = ops.embed_splice(llama.embed, None, None, torch.tensor([[0, tk] for tk in toks], dtype=torch.int32).to(dev))
                logits = llama_forward(llama, kv, [fresh[beam][g] for g in rows for beam in range(NB)], x, [1] * len(toks))
            assert live_at[t] == groups
            bs = torch.tensor([v for g in groups for v in scores[g]], dtype=torch.float32).to(dev)
            s, tok, b = ops.beam_step(logits, bs, len(groups), NB, n)
        finally:
            for col in fresh:
                for q in col:
                    kv.release(q.pages)
        return [(s[i].cpu().tolist(), b[i].cpu().tolist(), tok[i].cpu().tolist()) for i in range(len(groups))]

    return beam_ref.beam_search(topk, B, NB, MAX_NEW, EOS, lp, es, nrs)


def _e2e_inputs(which, dev):
    g = torch.Generator().manual_seed(77)
    V = cases.LLM["vocab_size"]
    rnd = lambda n: torch.randint(3, V, (n,), generator=g).tolist()                     # noqa: E731
    if which == "image":
        return torch.tensor([[1, -200] + rnd(9)]), None, [torch.randn((3, 56, 56), generator=g).bfloat16().to(dev)]
    a, b = [1] + rnd(69), [1] + rnd(19)                       # 70 rows (a shared whole page and a partial one) beside 20, right-padded
    ids = torch.tensor([a, b + [0] * 50])
    mask = torch.tensor([[1] * 70, [1] * 20 + [0] * 50])
    return ids, mask.to(dev), None


@pytest.mark.parametrize("fmt", ["16bit", "fp8"])
@pytest.mark.parametrize("which", ["image", "text2"])
def test_generate_beams_equals_the_restatement(dev, model, which, fmt):
    model.set_kv_cache_dtype(fmt)
    try:
        ids, mask, images = _e2e_inputs(which, dev)
        B, L0 = ids.shape
        model._ensure_kv(64)
        free0 = len(model.kv.free)
        out = model.generate(ids.to(dev), images=images, attention_mask=mask, num_beams=NB, num_return_sequences=NB, max_new_tokens=MAX_NEW,
                             eos_token_id=EOS, pad_token_id=0)
        scores = model.last_beam_scores.cpu().numpy()
        assert len(model.kv.free) == free0
        assert out.shape[0] == B * NB and out.dtype == torch.long and scores.dtype == np.float32 and scores.shape == (B * NB,)
        assert torch.equal(out[:, :L0].cpu(), ids.repeat_interleave(NB, 0))
        ref = _reference_generate(model, ids, mask, images, NB, 1.0, False)
        assert len(model.kv.free) == free0
        longest = max(len(h) for grp in ref for _, h in grp)
        assert out.shape[1] == L0 + longest
        row = 0
        for grp in ref:
            assert len({tuple(h) for _, h in grp}) == NB                      # three different hypotheses
            for sc, h in grp:
                assert out[row, L0:].cpu().tolist() == h + [0] * (longest - len(h)), (which, row)
                assert np.float32(sc).tobytes() == scores[row].tobytes(), (which, row, sc, scores[row])
                row += 1
        # another length penalty and early stopping: one more pair, returning the best hypothesis only
        out1 = model.generate(ids.to(dev), images=images, attention_mask=mask, num_beams=NB, max_new_tokens=MAX_NEW, eos_token_id=EOS,
                              pad_token_id=0, length_penalty=2.0, early_stopping=True)
        ref1 = _reference_generate(model, ids, mask, images, 1, 2.0, True)
        longest = max(len(h) for grp in ref1 for _, h in grp)
        assert [r[L0:] for r in out1.cpu().tolist()] == [h + [0] * (longest - len(h)) for grp in ref1 for _, h in grp]
        assert [np.float32(sc) for grp in ref1 for sc, _ in grp] == model.last_beam_scores.cpu().numpy().tolist()
    finally:
        model.set_kv_cache_dtype("16bit")


def test_num_beams_1_is_the_plain_greedy_call(dev, model):
    ids, mask, images = _e2e_inputs("image", dev)
    kw = dict(images=images, max_new_tokens=8, eos_token_id=EOS, pad_token_id=0)
    assert torch.equal(model.generate(ids.to(dev), num_beams=1, **kw), model.generate(ids.to(dev), **kw))
    ids, mask, _ = _e2e_inputs("text2", dev)
    kw = dict(attention_mask=mask, max_new_tokens=8, eos_token_id=EOS, pad_token_id=0)
    assert torch.equal(model.generate(ids.to(dev), num_beams=1, **kw), model.generate(ids.to(dev), **kw))


REFUSED = [dict(do_sample=True), dict(padded_batch=True), dict(repetition_penalty=1.1), dict(suppress_tokens=[5]),
           dict(begin_suppress_tokens=[5]), dict(min_new_tokens=2), dict(bad_words_ids=[[5]]), dict(allowed_token_ids=[5, 6, 7, 8, 9, 10, 11]),
           dict(num_beams=17), dict(num_beams=9, eos_token_id=[7, 19, 33])]


@pytest.mark.parametrize("kw", REFUSED, ids=[next(iter(k)) + str(i) for i, k in enumerate(REFUSED)])
def test_refused_combinations_take_no_page(dev, model, kw):
    ids, mask, _ = _e2e_inputs("text2", dev)
    model._ensure_kv(64)
    free0 = len(model.kv.free)
    args = dict(attention_mask=mask, num_beams=2, max_new_tokens=4, eos_token_id=EOS, pad_token_id=0)
    args.update(kw)
    with pytest.raises(NotImplementedError) as e:
        model.generate(ids.to(dev), **args)
    name = next(iter(kw))
    assert name in str(e.value)
    assert len(model.kv.free) == free0


def test_more_candidates_than_the_vocabulary_is_refused(dev, model):
    ids, mask, _ = _e2e_inputs("text2", dev)
    model._ensure_kv(64)
    free0 = len(model.kv.free)
    V = model.config.vocab_size
    model.config.vocab_size = 6           # 2 * num_beams = 8 candidates > 6
    try:
        with pytest.raises(NotImplementedError) as e:
            model.generate(ids.to(dev), attention_mask=mask, num_beams=4, max_new_tokens=4, eos_token_id=7, pad_token_id=0)
    finally:
        model.config.vocab_size = V
    assert "num_beams" in str(e.value) and len(model.kv.free) == free0


def test_a_failure_in_the_middle_gives_every_page_back(dev, model, monkeypatch):
    from vitron_amd import ops
    ids, mask, _ = _e2e_inputs("text2", dev)
    model._ensure_kv(64)
    free0 = sorted(model.kv.free)
    real = ops.beam_step
    calls = []

    def failing(*a, **k):
        calls.append(1)
        if len(calls) == 3:
            raise ValueError("injected at step 3")
        return real(*a, **k)
    monkeypatch.setattr(ops, "beam_step", failing)
    with pytest.raises(ValueError, match="injected"):
        model.generate(ids.to(dev), attention_mask=mask, num_beams=NB, max_new_tokens=MAX_NEW, eos_token_id=EOS, pad_token_id=0)
    assert len(calls) == 3 and sorted(model.kv.free) == free0
    monkeypatch.setattr(ops, "beam_step", real)
    out = model.generate(ids.to(dev), attention_mask=mask, num_beams=NB, max_new_tokens=4, eos_token_id=EOS, pad_token_id=0)     # and works again
    assert out.shape[0] == 2 and sorted(model.kv.free) == free0
