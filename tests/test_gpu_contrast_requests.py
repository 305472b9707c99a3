"""Contrastive search end to end on the tiny synthetic model, both builds and both pool formats: contrastive.CandidateGroup
against k private-page sequences kept in step by whole-sequence page copies (bit-equal logits, at most k - 1 pages copied per step), and
generate(penalty_alpha=, top_k=) against a loop this file drives itself on private-page sequences through ops.logprob_rows,
ops.unit_rows and ops.contrast_rows (tests/contrast_ref.contrastive_loop): B = 1 and ragged B = 2, a multimodal prompt with a region, EOS,
stopping_criteria, the return of every page, the off switches."""
import pytest
import torch

from tests import contrast_cases as CC
from tests import contrast_ref as R
from tests.golden import cases

pytestmark = pytest.mark.gpu
TV = cases.LLM["vocab_size"]
DT = pytest.mark.parametrize("dt", CC.DTYPES, ids=["bf16", "fp16"])
FMT = pytest.mark.parametrize("fmt", ["16bit", "fp8"])
ALPHA = 0.6


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    made = {}

    def get(dt):
        if dt not in made:
            made[dt] = CC.tiny_model(dev, dt)
        return made[dt]
    return get


def _embed(llama, toks, dev):
    from vitron_amd import ops
    return ops.embed_splice(llama.embed, None, None, torch.tensor([[0, int(t)] for t in toks], dtype=torch.int32).to(dev))


def _copy_whole(kv, copy, src, others):
    """private pages: the whole sequence `src` onto every sequence of `others`"""
    for o in others:
        assert len(o.pages) == len(src.pages)
        copy(kv, src.pages, o.pages)


# ---- CandidateGroup against private pages -------------------------------------------------------------------------------------------------
K = 3
STEPS = 68                     # from 63 / 64 / 65 / 130 rows: across the boundaries at 64, 128 and 192


@pytest.mark.parametrize("prompt_len", [63, 64, 65, 130])
@FMT
@DT
def test_candidate_group_equals_private_pages(dev, models, dt, fmt, prompt_len, monkeypatch):
    from vitron_amd import ops
    from vitron_amd.contrastive import CandidateGroup
    from vitron_amd.engine import PagedKVCache, SequenceState, llama_forward
    llama = models(dt).model.llama
    kv = PagedKVCache(llama, 40, kv_dtype=fmt)
    copied = []
    real_copy = ops.kv_copy_pages

    def counting(kv_, src, dst):
        copied.append(len(list(src)))
        return real_copy(kv_, src, dst)
    monkeypatch.setattr(ops, "kv_copy_pages", counting)
    g = torch.Generator().manual_seed(prompt_len)
    prompt = _embed(llama, torch.randint(3, TV, (prompt_len,), generator=g).tolist(), dev)

    def prefilled():
        s = SequenceState()
        llama_forward(llama, kv, [s], prompt, [prompt_len])
        return s

    private = [prefilled()]
    for _ in range(K - 1):
        s = SequenceState()
        s.pages, s.length = kv.alloc(len(private[0].pages)), prompt_len
        private.append(s)
    _copy_whole(kv, real_copy, private[0], private[1:])
    group = CandidateGroup(llama, kv, prefilled(), K, STEPS)
    try:
        assert sum(copied) == (K - 1 if prompt_len % 64 else 0)
        for t in range(STEPS):
            toks = [(7 * t + 3 * s) % 90 + 5 for s in range(K)]
            x = _embed(llama, toks, dev)
            got = llama_forward(llama, kv, group.seqs, x, [1] * K)
            want = llama_forward(llama, kv, private, x, [1] * K)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"step {t}: the group's logits differ from private pages"
            sel = (5 * t + 1) % K
            before = sum(copied)
            n = group.select(sel)
            assert sum(copied) - before == n <= K - 1
            if len(private[0].pages) * 64 == private[0].length:               # (the private model: the next step's page, then the whole copy)
                for s in private:
                    s.pages += kv.alloc(1)
            _copy_whole(kv, real_copy, private[sel], [s for i, s in enumerate(private) if i != sel])
        assert len(group.shared) == (prompt_len + STEPS) // 64
    finally:
        group.release()
        for s in private:
            kv.release(s.pages)
    assert sorted(kv.free) == list(range(40))


# ---- generate against a driven loop ------------------------------------------------------------------------------------------------------
def _rnd(seed, n):
    return torch.randint(3, TV, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _image(dev, dt, seed):
    return torch.randn((3, 56, 56), generator=torch.Generator().manual_seed(seed)).to(dt).to(dev)


def fixture(which, dev, dt):
    """(input_ids, attention_mask, images, regions)"""
    if which == "image":
        return torch.tensor([[1, -200] + _rnd(601, 9)]).to(dev), None, [_image(dev, dt, 602)], None
    if which == "region":
        return (torch.tensor([[1, -200] + _rnd(603, 5) + [-300, 1] + _rnd(604, 7)]).to(dev), None, [_image(dev, dt, 605)],
                [[20.0, 30.0, 150.0, 200.0]])
    if which == "text":
        return torch.tensor([[1] + _rnd(606, 66)]).to(dev), None, None, None
    a, b = [1] + _rnd(607, 69), [1] + _rnd(608, 19)              # 70 rows (a whole page and a partial one) beside 20, right-padded
    ids = torch.tensor([a, b + [0] * 50]).to(dev)
    mask = torch.tensor([[1] * 70, [1] * 20 + [0] * 50]).to(dev)
    return ids, mask, None, None


def drive(model, ids, mask, images, regions, k, alpha, n_new, eos=(), pad=0, stop=None):
    """The loop generate(penalty_alpha=, top_k=) is held to, driven from here on PRIVATE pages: the prompts embedded and prefilled as
    generate() does it (one packed pass, the hidden stream of every row), every prompt's cache copied whole into k private sequences, and
    per step ops.logprob_rows (top k), one pass over the live prompts' k private sequences, ops.unit_rows, ops.contrast_rows, the
    selections read back, the chosen sequence copied whole onto its k - 1 siblings. Returns ([B][n] ids, the banks' lengths after the
    prefill)."""
    from vitron_amd import ops
    from vitron_amd.engine import SequenceState, llama_forward
    dev = model.device
    llama = model.model.llama
    emb, mh, _ = model._embed_prompt(ids, mask, images, regions, use_vis_cache=False)
    flat, flat_lo, lens, _ = model._pack_rows(emb, mh)
    B = len(lens)
    model._ensure_kv(sum(k * ((n + n_new + 63) // 64 + 1) for n in lens))
    kv = model.kv
    first = [SequenceState() for _ in range(B)]
    private, banks, blen, cur, lps = [], [], list(lens), {}, {}
    try:
        logits, hidden = llama_forward(llama, kv, first, flat, lens, embeds_lo=flat_lo, return_hidden=True)
        at = 0
        for b in range(B):
            bank = torch.zeros((lens[b] + n_new, llama.H), dtype=llama.dtype, device=dev)
            ops.unit_rows(hidden[at:at + lens[b]], llama.final_norm, out=bank[:lens[b]])
            banks.append(bank)
            at += lens[b]
            cur[b] = logits[b].clone()
            sib = []
            for _ in range(k - 1):
                s = SequenceState()
                s.pages, s.length = kv.alloc(len(first[b].pages)), first[b].length
                sib.append(s)
            private.append([first[b]] + sib)
            _copy_whole(kv, ops.kv_copy_pages, first[b], sib)

        def candidates(live):
            top = ops.logprob_rows(torch.stack([cur[b] for b in live]), None, k)
            for j, b in enumerate(live):
                lps[b] = top["top_logprobs"][j].clone()
            return top["top_ids"].cpu().tolist()

        def step(live, cands):
            x = _embed(llama, [t for row in cands for t in row], dev)
            lg, hid = llama_forward(llama, kv, [s for b in live for s in private[b]], x, [1] * (len(live) * k), return_hidden=True)
            cand = ops.unit_rows(hid, llama.final_norm, dtype=llama.dtype)
            d = torch.empty((len(live), k), dtype=torch.float32, device=dev)
            sc = torch.empty((len(live), k), dtype=torch.float32, device=dev)
            sel = torch.empty((len(live),), dtype=torch.int32, device=dev)
            ops.contrast_rows([dict(bank=banks[b], bank_len=blen[b], k=k, first=j * k, alpha=alpha, lp=lps[b], d=d[j], score=sc[j],
                                    sel=sel[j:j + 1]) for j, b in enumerate(live)], cand)
            sels = sel.cpu().tolist()
            for j, b in enumerate(live):
                blen[b] += 1
                cur[b] = lg[j * k + sels[j]].clone()
                for s in private[b]:
                    if len(s.pages) * 64 == s.length:
                        s.pages += kv.alloc(1)
                _copy_whole(kv, ops.kv_copy_pages, private[b][sels[j]], [s for i, s in enumerate(private[b]) if i != sels[j]])
            return sels
        out = R.contrastive_loop(B, k, n_new, eos, pad, candidates, step, stop)
    finally:
        for s in first:
            kv.release(s.pages)
            s.pages = []
        for grp in private:
            for s in grp[1:]:
                kv.release(s.pages)
    return out, list(lens)


def _new(out, L0):
    return [row[L0:] for row in out.cpu().tolist()]


@FMT
@DT
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("which", ["image", "text"])
def test_generate_equals_the_driven_loop(dev, models, dt, fmt, which, k):
    """The ids of generate(penalty_alpha=0.6, top_k=k) are those of the driven loop on private pages; every page is back afterwards; a
    prompt of 67 rows generates across the page boundary at 128."""
    model = models(dt)
    model.set_kv_cache_dtype(fmt)
    try:
        ids, mask, images, regions = fixture(which, dev, dt)
        n_new = 8 if which == "image" else 64
        want, _ = drive(model, ids, mask, images, regions, k, ALPHA, n_new)
        free0 = len(model.kv.free)
        out = model.generate(ids, images=images, attention_mask=mask, penalty_alpha=ALPHA, top_k=k, max_new_tokens=n_new, eos_token_id=-1)
        assert _new(out, ids.shape[1]) == want
        st = model.last_generate_stats
        assert st["contrastive_steps"] == n_new and st["top_k"] == k and st["pages_copied"] <= (k - 1) * n_new
        assert len(model.kv.free) == free0 == model.kv.num_pages
    finally:
        model.set_kv_cache_dtype("16bit")


@DT
def test_reply_differs_from_greedy_and_off_switches(dev, models, dt, monkeypatch):
    """The penalty changes the reply on at least one fixture; penalty_alpha None / 0 and top_k = 1 are the plain greedy call: the same
    ids and none of the mode's launches."""
    from vitron_amd import ops
    model = models(dt)
    differs = []
    for which in ("image", "region", "text"):
        ids, mask, images, regions = fixture(which, dev, dt)
        kw = dict(images=images, regions=regions, max_new_tokens=8, eos_token_id=-1)
        plain = model.generate(ids, **kw)
        differs.append(not torch.equal(model.generate(ids, penalty_alpha=ALPHA, top_k=4, **kw), plain))
        calls = []
        for name in ("contrast_rows", "unit_rows", "logprob_rows", "kv_copy_pages"):
            real = getattr(ops, name)
            monkeypatch.setattr(ops, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
        for off in (dict(penalty_alpha=None), dict(penalty_alpha=0), dict(penalty_alpha=0.0, top_k=4), dict(penalty_alpha=ALPHA, top_k=1)):
            assert torch.equal(model.generate(ids, **kw, **off), plain), off
            assert "contrastive_steps" not in model.last_generate_stats
        assert calls == []
        monkeypatch.undo()
    assert any(differs), "contrastive search returned the greedy reply on all three fixtures"
    assert len(model.kv.free) == model.kv.num_pages


@DT
def test_ragged_batch_rows_equal_their_solo_calls(dev, models, dt):
    """B = 2 ragged prompts (70 and 20 rows), k = 4 (B k <= 16): the batch equals the driven loop, and each row equals the same call on
    that prompt alone."""
    model = models(dt)
    ids, mask, _, _ = fixture("text2", dev, dt)
    n_new, k = 7, 4
    out = model.generate(ids, attention_mask=mask, penalty_alpha=ALPHA, top_k=k, max_new_tokens=n_new, eos_token_id=-1)
    got = _new(out, ids.shape[1])
    want, lens = drive(model, ids, mask, None, None, k, ALPHA, n_new)
    assert got == want and lens == [70, 20] and model.last_generate_stats["bank_len"] == [70, 20]
    for b, n in enumerate((70, 20)):
        solo = model.generate(ids[b:b + 1, :n], penalty_alpha=ALPHA, top_k=k, max_new_tokens=n_new, eos_token_id=-1)
        assert _new(solo, n)[0] == got[b], b
    assert len(model.kv.free) == model.kv.num_pages


@DT
def test_multimodal_bank_holds_the_visual_rows(dev, models, dt):
    """An image and a region: the bank's length after the prefill is the SPLICED row count (text ids - 2 sentinels + the image's rows + the
    region's row), and the ids equal the driven loop's."""
    model = models(dt)
    ids, mask, images, regions = fixture("region", dev, dt)
    want, lens = drive(model, ids, mask, images, regions, 3, ALPHA, 6)
    out = model.generate(ids, images=images, regions=regions, penalty_alpha=ALPHA, top_k=3, max_new_tokens=6, eos_token_id=-1)
    assert _new(out, ids.shape[1]) == want
    emb, _, spliced = model._embed_prompt(ids, None, images, regions, use_vis_cache=False)
    assert spliced and model.last_generate_stats["bank_len"] == [emb.shape[1]] == lens and emb.shape[1] > ids.shape[1]
    assert len(model.kv.free) == model.kv.num_pages


@DT
def test_eos_and_stopping_criteria(dev, models, dt):
    """EOS mid-way pads the finished row while the other goes on; a stopping criterion that fires on the third token stops there."""
    model = models(dt)
    ids, mask, _, _ = fixture("text2", dev, dt)
    L0, n_new, k = ids.shape[1], 7, 4
    kw = dict(attention_mask=mask, penalty_alpha=ALPHA, top_k=k, max_new_tokens=n_new)
    full = _new(model.generate(ids, eos_token_id=-1, **kw), L0)
    eos = full[0][2]
    first = full[0].index(eos)
    out = _new(model.generate(ids, eos_token_id=eos, pad_token_id=0, **kw), L0)
    want, _ = drive(model, ids, mask, None, None, k, ALPHA, n_new, eos=[eos], pad=0)
    assert out == want
    assert out[0][:first + 1] == full[0][:first + 1] and set(out[0][first + 1:]) <= {0}
    if eos not in full[1]:
        assert out[1] == full[1] and len(out[1]) == n_new                                    # the other row goes on, unchanged
    seen = []

    def third(input_ids, scores):
        seen.append(input_ids.shape[1] - L0)
        return input_ids.shape[1] - L0 >= 3
    stopped = _new(model.generate(ids, eos_token_id=-1, stopping_criteria=[third], **kw), L0)
    assert stopped == [r[:3] for r in full] and seen == [1, 2, 3]
    assert len(model.kv.free) == model.kv.num_pages


@DT
def test_pages_return_after_a_refusal_and_after_a_failure(dev, models, dt, monkeypatch):
    from vitron_amd import ops
    model = models(dt)
    ids, mask, images, regions = fixture("image", dev, dt)
    model.generate(ids, images=images, max_new_tokens=2, eos_token_id=-1)
    assert len(model.kv.free) == model.kv.num_pages
    with pytest.raises(NotImplementedError, match="top_k"):
        model.generate(ids, images=images, penalty_alpha=ALPHA, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match="return_logits"):
        model.generate(ids, images=images, penalty_alpha=ALPHA, top_k=4, max_new_tokens=4, return_logits=True)
    with pytest.raises(ValueError, match="penalty_alpha"):
        model.generate(ids, images=images, penalty_alpha=1.5, top_k=4, max_new_tokens=4)
    assert len(model.kv.free) == model.kv.num_pages
    real, calls = ops.contrast_rows, []

    def failing(*a, **k):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("injected")
        return real(*a, **k)
    monkeypatch.setattr(ops, "contrast_rows", failing)
    with pytest.raises(RuntimeError, match="injected"):
        model.generate(ids, images=images, penalty_alpha=ALPHA, top_k=4, max_new_tokens=6, eos_token_id=-1)
    monkeypatch.undo()
    assert len(model.kv.free) == model.kv.num_pages
    out = model.generate(ids, images=images, penalty_alpha=ALPHA, top_k=4, max_new_tokens=6, eos_token_id=-1)       # and the next call is whole
    assert out.shape[1] == ids.shape[1] + 6 and len(model.kv.free) == model.kv.num_pages
