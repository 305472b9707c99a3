"""vt_ban_rows on the GPU, both operand builds: the whole mask bit for bit against tests/ban_ref.py over the vocabulary
sizes, history lengths and n-gram sizes at which the kernel's paths change, given and missing base masks, matching / missing / too long /
malformed sequences and sentinels -- every row of one launch with its own parameters and a guard word behind its mask; then the
feature end to end on the tiny synthetic model (tests/allow_cases.py): generate(no_repeat_ngram_size=) replayed from its returned
logits, ServingEngine requests with no_repeat_ngram_size / bad_words beside other requests, and the release of their device buffers."""
import numpy as np
import pytest
import torch

from tests import ban_ref as R
from tests import sample_ref as S
from tests.golden import cases as G
from tests.allow_cases import solo as _solo, submit as _submit, tiny_model

pytestmark = pytest.mark.gpu
VS = (31, 32, 33, 64, 1000, 32000, 50257)
GUARD = 0x5A5A5A5A
TV = G.LLM["vocab_size"]


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return tiny_model(dev)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def _case(h=(), g=0, seqs=None, flat=None, n_seqs=None, seqs_len=None, base=None, hist_len=None, hist_null=False, out_null=False,
          must_ban=False):
    """One row. seqs: well-formed sequences (flattened here); flat / n_seqs / seqs_len: the raw fields instead."""
    if flat is None and seqs is not None:
        flat = [x for s in seqs for x in [len(s)] + list(s)]
        n_seqs = len(seqs)
    flat = None if flat is None else [int(x) for x in flat]
    return dict(h=[int(t) for t in h], g=int(g), flat=flat, n_seqs=int(n_seqs or 0), seqs_len=len(flat or ()) if seqs_len is None else int(seqs_len),
                base=base, hist_len=len(h) if hist_len is None else int(hist_len), hist_null=hist_null, out_null=out_null, must_ban=must_ban)


def _expected(V, c):
    h = [] if (c["hist_null"] or c["hist_len"] <= 0) else c["h"][:c["hist_len"]]
    seqs = [] if c["flat"] is None else R.parse_seqs(c["flat"], c["n_seqs"], c["seqs_len"])
    return R.ban_mask(V, h, c["g"], seqs, c["base"])


_built = {}


def _cases(V):
    """The rows of one launch at vocabulary V and their reference masks, built once and shared by both builds"""
    if V in _built:
        return _built[V]
    rng = np.random.default_rng(7000 + V)
    W = R.words(V)

    def base(kind):
        if kind == 0:
            return None
        b = rng.integers(0, 2 ** 32, size=W, dtype=np.uint64).astype(np.uint32)
        if V % 32:
            if kind == 1:
                b[-1] &= np.uint32((1 << (V % 32)) - 1)
            else:
                b[-1] |= np.uint32(0xFFFFFFFF ^ ((1 << (V % 32)) - 1))          # bits at positions >= V: they come back as they were
        return b

    rows, k = [], 0
    for g in (0, 1, 2, 3, 5):
        for n in sorted({x for x in (0, 1, g - 2, g - 1, g, 255, 256, 257, 1500) if x >= 0}):
            alphabet = rng.choice(V, size=2 + k % 3, replace=False)
            h = rng.choice(alphabet, size=n).tolist()
            seqs = [rng.choice(alphabet, size=int(rng.integers(1, 5))).tolist() for _ in range(2)] if k % 2 else None
            rows.append(_case(h, g, seqs, base=base(k % 3)))
            k += 1
    for p, n, g in R.MUST_BAN:                                                   # periodic histories: the rule bans something (CPU test)
        rows.append(_case(R.periodic(n, p), g, must_ban=True))
    # sequences of length 1, 2 and 4 that match, that miss at each position, that are longer than the history allows
    h4 = [10, 11, 12, 13]
    for seqs in ([[20]], [[13, 21]], [[12, 21]], [[11, 12, 13, 22]], [[9, 12, 13, 23]], [[11, 9, 13, 24]], [[11, 12, 9, 25]],
                 [[20], [13, 21], [12, 26], [11, 12, 13, 22], [9, 12, 13, 23], [11, 9, 13, 24], [11, 12, 9, 25], [13, 21]]):
        rows.append(_case(h4, 0, seqs, base=base(k % 2)))
        k += 1
    rows += [_case([12, 13], 0, [[11, 12, 13, 26]]), _case([11, 12, 13], 0, [[11, 12, 13, 22]]), _case([], 0, [[13, 21], [20]]),
             _case([13], 0, [[13, 21]]), _case([13], 0, [[12, 13, 21]]), _case(h4, 3, [[13, 21]], base=base(1))]
    rows.append(_case(h4, 0, [[(3 * i) % V] if i % 2 else [13, (5 * i) % V] for i in range(1100)]))       # more sequences than threads
    rows.append(_case(R.periodic(64, 2), 2, [[7, 9]], out_null=True))            # out NULL between live rows: skipped entirely
    # malformed buffers: the parsing ends there, the entries before count; nothing outside seqs[0 .. seqs_len) is read
    rows += [_case(h4, 0, flat=[1, 20, 0, 21, 22], n_seqs=3), _case(h4, 0, flat=[2, 13, 21, 4, 11, 12], n_seqs=2),
             _case(h4, 0, flat=[1, 20], n_seqs=10), _case(h4, 0, flat=[1, 20, 1, 21], n_seqs=2, seqs_len=2),
             _case(h4, 0, flat=[-1, 20], n_seqs=1), _case(h4, 0, flat=[1, 20], n_seqs=1, seqs_len=0),
             _case(h4, 0, flat=[1, 20], n_seqs=0), _case(h4, 0, flat=[1, 20], n_seqs=-3), _case(h4, 0, flat=[1, 20], n_seqs=1, seqs_len=-2),
             _case(h4, 0, flat=[2 ** 31 - 1, 20, 21], n_seqs=1), _case(h4, 0, flat=[1, 20, 2 ** 31 - 1], n_seqs=2),
             _case(h4, 0, flat=None, n_seqs=4, seqs_len=9)]                                               # seqs NULL with counts set
    # degenerate history fields
    rows += [_case([5, 6, 5], 2, hist_len=-4), _case([5, 6, 5], 2, hist_null=True), _case([5, 6, 5, 6, 5], 2, hist_len=3),
             _case(R.periodic(300, 3), -2), _case(R.periodic(300, 3), 2 ** 31 - 1), _case(R.periodic(300, 3), 301), _case(R.periodic(300, 3), 300)]
    # sentinels and ids >= V: inside the window they compare like any id, as the id to clear they are skipped
    rows += [_case([5, -200, 6, 9, 5, -200], 3), _case([5, -200, 6, 9, 5, -300], 3), _case([5, V + 7, 6, 9, 5, V + 7], 3),
             _case([5, -200, 9, 5], 2), _case([5, V, 9, 5], 2), _case([5, V - 1, 9, 5], 2), _case([3, -200, V, 2 ** 31 - 1, -2 ** 31, 3], 1),
             _case([V - 1] * 3, 1, base=base(2)), _case([1, 2], 0, [[-200, 4], [2, V], [2, -1], [2, V - 1], [-5], [V]]),
             _case([-200], 0, [[-200, 4]])]
    want = [None if c["out_null"] else _expected(V, c) for c in rows]
    for c, m in zip(rows, want):
        if c["must_ban"]:
            assert not np.array_equal(m, R.ban_mask(V, [], 0)), c["g"]           # non-vacuity: the expected mask has bits cleared
    _built[V] = (rows, want)
    return _built[V]


def _layout(V, rows, want):
    """All buffers of the launch in ONE int32 image: per row history, seqs, base and out (W words + a guard), separated by guard words;
    every other row's base and out on a 16-byte boundary, the rest off it. Returns (image before, image expected after, struct fields)."""
    from vitron_amd.sampling import BAN_ROW_DTYPE
    W = R.words(V)
    chunks, pos = [], 0
    fields = np.zeros((len(rows),), dtype=BAN_ROW_DTYPE)

    def put(words_, i, vec):
        nonlocal pos
        pos += 1                                                                 # at least one guard word between any two buffers
        pos += (-pos) % 4
        if not vec or i % 2:
            pos += 1 + i % 3                                                     # 4-byte aligned only
        off = pos
        chunks.append((off, np.asarray(words_, dtype=np.int64)))
        pos += len(words_)
        return off

    outs = []
    for i, c in enumerate(rows):
        ho = put(c["h"], i, False) if c["h"] else put([GUARD], i, False)
        so = None if c["flat"] is None else put(c["flat"] or [GUARD], i, False)
        bo = None if c["base"] is None else put(c["base"].astype(np.int64), i, True)
        oo = put([GUARD] * W, i, True)
        outs.append(oo)
        fields[i] = (0 if c["hist_null"] else ho, 0 if bo is None else bo, 0 if c["out_null"] else oo, 0 if so is None else so,
                     c["hist_len"], c["g"], c["n_seqs"], c["seqs_len"])
    img = np.full((pos + 8,), GUARD, dtype=np.int64)
    for off, w in chunks:
        img[off:off + len(w)] = w
    before = (img & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    after = before.copy()
    for c, oo, m in zip(rows, outs, want):
        if m is not None:
            after[oo:oo + W] = m.view(np.int32)
    return before, after, fields


def _launch(lib, dev, V, before, fields):
    buf = torch.from_numpy(before.copy()).to(dev)
    f = fields.copy()
    for name in ("history", "base", "out", "seqs"):                              # word offsets -> device addresses (0 stays NULL)
        f[name] = np.where(fields[name] != 0, buf.data_ptr() + 4 * fields[name].astype(np.uint64), 0).astype(np.uint64)
    rows_dev = torch.from_numpy(f.view(np.uint8).reshape(len(f), 48).copy()).to(dev)
    st = lib.vt_ban_rows(rows_dev.data_ptr(), len(f), V, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, buf.cpu().numpy()


@pytest.mark.parametrize("operand", ("bf16", "fp16"))
@pytest.mark.parametrize("V", VS)
def test_ban_rows_equals_the_reference_bit_for_bit(dev, V, operand):
    """Every row's whole mask equals ban_ref; everything else in the image -- histories, sequences, bases, the guard word behind every
    mask, the words between the buffers -- is what it was. One launch of 105 rows, each with its own parameters."""
    from vitron_amd import _lib
    rows, want = _cases(V)
    before, after, fields = _layout(V, rows, want)
    st, got = _launch(_lib.load(operand=operand), dev, V, before, fields)
    assert st == 0, _lib.last_error()
    if not np.array_equal(got, after):
        W = R.words(V)
        for i, (c, m) in enumerate(zip(rows, want)):
            if m is None:
                continue
            oo = int(fields["out"][i])
            assert np.array_equal(got[oo:oo + W], m.view(np.int32)), (V, i, {k: c[k] for k in ("g", "hist_len", "n_seqs", "seqs_len")}, c["h"][:8])
        assert False, ("a word outside the masks changed", np.flatnonzero(got != after)[:8].tolist())


def test_mixed_rows_through_ops_skip_and_repeat(dev):
    """ops.ban_rows + sampling.pack_ban_rows: three rows with their own parameters, the middle one with out NULL (skipped entirely: the
    buffer prepared for it and every guard word stay as they were); three launches give equal masks."""
    from vitron_amd import ops
    from vitron_amd.sampling import allow_mask, flatten_ban_seqs, history_bans, pack_ban_rows
    V = 1000
    W = R.words(V)
    h0, h2 = R.periodic(257, 3), [5, -200, 6, 9, 5, -200, 6, 9]
    seqs = [[6, 9, 40], [41]]
    base2 = allow_mask(V, range(0, V, 2))
    t = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)                  # noqa: E731
    hist = [t(h0), t([1, 2, 3, 1]), t(h2)]
    flat = torch.from_numpy(flatten_ban_seqs(seqs)).to(dev)
    base = torch.from_numpy(base2.view(np.int32)).to(dev)
    outs = [torch.full((W + 1,), GUARD, dtype=torch.int32, device=dev) for _ in range(3)]
    rows = [(hist[0].data_ptr(), len(h0), 0, outs[0].data_ptr(), 3, 0, 0, 0),
            (hist[1].data_ptr(), 4, 0, 0, 1, 0, 0, 0),                           # out NULL: skipped
            (hist[2].data_ptr(), len(h2), base.data_ptr(), outs[2].data_ptr(), 4, flat.data_ptr(), len(seqs), int(flat.numel()))]
    packed = pack_ban_rows(rows, dev)
    assert packed.shape == (3, 48) and packed.dtype == torch.uint8
    runs = []
    for _ in range(3):
        ops.ban_rows(packed, 3, V)
        torch.cuda.synchronize()
        runs.append([o.cpu().numpy().copy() for o in outs])
    want0, want2 = R.ban_mask(V, h0, 3), R.ban_mask(V, h2, 4, seqs, base2)
    assert R.banned(V, h0, 3) == history_bans(V, h0, 3) != [] and R.banned(V, h2, 4, seqs) == history_bans(V, h2, 4, seqs) == [5, 40, 41]
    for got in runs:
        assert np.array_equal(got[0][:W], want0.view(np.int32)) and np.array_equal(got[2][:W], want2.view(np.int32))
        assert (got[1] == GUARD).all() and got[0][W] == GUARD and got[2][W] == GUARD
    assert np.array_equal(base.cpu().numpy(), base2.view(np.int32))


def test_refusals_and_no_rows(dev):
    from vitron_amd import _lib, ops
    from vitron_amd.sampling import pack_ban_rows
    lib = _lib.load()
    out = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
    packed = pack_ban_rows([(0, 0, 0, out.data_ptr(), 0, 0, 0, 0)], dev)
    stream = torch.cuda.current_stream().cuda_stream
    for n_rows, V, ptr, needle in ((1, 0, packed.data_ptr(), "V=0"), (1, -5, packed.data_ptr(), "V=-5"), (1, 262145, packed.data_ptr(), "V=262145"),
                                   (-1, 64, packed.data_ptr(), "n_rows=-1"), (1, 64, None, "NULL")):
        assert lib.vt_ban_rows(ptr, n_rows, V, stream) == -1                      # VT_STATUS_ARG, with a message
        assert needle in _lib.last_error(lib), (needle, _lib.last_error(lib))
    assert lib.vt_ban_rows(None, 0, 64, stream) == 0 and lib.vt_ban_rows(packed.data_ptr(), 0, 64, stream) == 0
    ops.ban_rows(packed, 0, 64)                                                   # n_rows == 0: a success that launches nothing
    with pytest.raises(_lib.VitronHipError, match="V=0"):
        ops.ban_rows(packed, 1, 0)
    with pytest.raises(_lib.VitronHipError):
        ops.ban_rows(packed, 2, 64)                                               # 48 bytes are one row, not two
    with pytest.raises(_lib.VitronHipError):
        ops.ban_rows(packed.cpu(), 1, 64)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()                                     # nothing was launched
    ops.ban_rows(packed, 1, 64)                                                   # the largest legal V runs too (the LDS mask at its full size)
    big = torch.full((262144 // 32 + 1,), GUARD, dtype=torch.int32, device=dev)
    ops.ban_rows(pack_ban_rows([(0, 0, 0, big.data_ptr(), 1, 0, 0, 0)], dev), 1, 262144)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert (got[:-1] == -1).all() and got[-1] == GUARD and out.cpu().numpy().tolist() == [-1, -1, GUARD, GUARD]


# ---- generate ------------------------------------------------------------------------------------------------------------------------------
def _new(out, L0):
    return out[0, L0:].cpu().tolist()


def test_generate_unigram_ban_forces_the_worst_allowed_token(dev, model):
    """The prompt ends with the ids of a set A. Held to A the model emits t0 in A; y is the LEAST likely id outside the prompt. Held to
    A + {y} with no_repeat_ngram_size=1 every id of A is banned (each occurs in the prompt), so the call must return y -- without the
    device-built mask it returns the arg-max over A + {y}, which is not y."""
    g = torch.Generator().manual_seed(91)
    A = [40, 77, 130, 255, 300]
    prompt = [1] + torch.randint(3, TV, (12,), generator=g).tolist() + A
    ids = torch.tensor([prompt]).to(dev)
    out, logits = model.generate(ids, do_sample=False, allowed_token_ids=A, max_new_tokens=1, eos_token_id=-1, return_logits=True)
    t0 = _new(out, len(prompt))[0]
    assert t0 in A
    row = logits[0][0].float().cpu().numpy().copy()
    row[sorted(set(prompt))] = np.inf
    y = int(row.argmin())
    assert y not in prompt and y != t0
    got = model.generate(ids, do_sample=False, allowed_token_ids=A + [y], no_repeat_ngram_size=1, max_new_tokens=1, eos_token_id=-1)
    assert _new(got, len(prompt)) == [y]
    assert _new(model.generate(ids, do_sample=False, allowed_token_ids=A + [y], max_new_tokens=1, eos_token_id=-1), len(prompt)) == [t0]
    assert len(model.kv.free) == model.kv.num_pages


@pytest.mark.parametrize("penalty", (1.0, 1.3))
def test_generate_bigram_ban_replays_from_its_logits(dev, model, penalty):
    """generate(no_repeat_ngram_size=2) for 12 steps at B = 2 with unequal prompt lengths (right padding, packed): every emitted id is the
    first arg-max of that step's returned logits -- penalised through tests/sample_ref.py when a repetition penalty is set -- with
    ban_ref's ids at -inf, where the history is the sample's ids under its attention mask followed by the ids it has emitted."""
    g = torch.Generator().manual_seed(92)
    a = [1] + torch.randint(3, TV, (9,), generator=g).tolist()
    a = a + [a[3], a[4]] + torch.randint(3, TV, (4,), generator=g).tolist() + [a[3]]      # ... x y ... x y ... x: the bigram (x, y) is closed
    b = [1] + torch.randint(3, TV, (5,), generator=g).tolist()
    b = b + [b[2]]
    pad, n_new = 0, 12
    ids = torch.full((2, len(a)), pad, dtype=torch.long)
    ids[0, :len(a)] = torch.tensor(a)
    ids[1, :len(b)] = torch.tensor(b)
    am = torch.zeros_like(ids)
    am[0, :len(a)] = 1
    am[1, :len(b)] = 1
    out, logits = model.generate(ids.to(dev), attention_mask=am.to(dev), do_sample=False, no_repeat_ngram_size=2, max_new_tokens=n_new,
                                 eos_token_id=-1, pad_token_id=pad, return_logits=True, repetition_penalty=penalty)
    new = out[:, ids.shape[1]:].cpu().tolist()
    assert len(logits) == n_new and all(len(r) == n_new for r in new)
    changed = 0
    for r, prompt in enumerate((a, b)):
        hist = list(prompt)
        pen_hist = [t for t in ids[r].tolist() if t >= 0]                         # the penalty's history: the row's non-negative ids (generate's docstring)
        for st in range(n_new):
            raw = logits[st][r].float().cpu().numpy()
            x = S.repetition_penalty(raw, pen_hist, penalty) if penalty != 1.0 else raw.copy()
            free = int(np.argmax(x))
            banned = R.banned(TV, hist, 2)
            if st == 0:
                assert banned == ([a[4]] if r == 0 else [b[3]])                    # what followed the earlier occurrence of the last id
            x[banned] = -np.inf
            want = int(np.argmax(x))
            assert new[r][st] == want, (r, st, new[r][st], want, banned)
            changed += want != free
            hist.append(want)
            pen_hist.append(want)
        assert len({(hist[i], hist[i + 1]) for i in range(len(hist) - 1)}) == len(hist) - 1 or r == 0        # b: no bigram occurs twice
    print(f"penalty {penalty}: the ban changed {changed} of {2 * n_new} picks")
    assert len(model.kv.free) == model.kv.num_pages


def test_generate_bigram_ban_on_top_of_an_allowed_set(dev, model):
    """Held to eight ids the greedy run repeats a bigram within 12 steps (asserted: the premise of this test); with
    no_repeat_ngram_size=2 on top the run equals it up to that step and differs there, and replays from its logits with the allowed set
    and ban_ref's ids at -inf: the static mask is the base of the device-built one. Eight ids cannot all be banned after one id within
    12 steps (that takes nine occurrences of it), so no row runs empty."""
    g = torch.Generator().manual_seed(94)
    S8 = [33, 64, 95, 160, 223, 320, 415, 511]
    prompt = [1] + [t for t in torch.randint(3, TV, (14,), generator=g).tolist() if t not in S8]
    ids = torch.tensor([prompt]).to(dev)
    L0, n_new = len(prompt), 12
    free = _new(model.generate(ids, do_sample=False, allowed_token_ids=S8, max_new_tokens=n_new, eos_token_id=-1), L0)
    hist, first = list(prompt), None
    for st, t in enumerate(free):
        if first is None and t in R.banned(TV, hist, 2):
            first = st
        hist.append(t)
    assert first is not None, free                                                # the free run closes a bigram twice
    out, logits = model.generate(ids, do_sample=False, allowed_token_ids=S8, no_repeat_ngram_size=2, max_new_tokens=n_new, eos_token_id=-1,
                                 return_logits=True)
    got = _new(out, L0)
    assert got[:first] == free[:first] and got[first] != free[first], (first, free, got)
    hist = list(prompt)
    off = np.ones((TV,), dtype=bool)
    off[S8] = False
    for st, t in enumerate(got):
        x = logits[st][0].float().cpu().numpy().copy()
        x[off] = -np.inf
        x[R.banned(TV, hist, 2)] = -np.inf
        assert np.isfinite(x).any() and t == int(np.argmax(x)), (st, t)
        hist.append(t)
    assert len({(hist[i], hist[i + 1]) for i in range(len(hist) - 1)}) == len(hist) - 1       # no bigram occurs twice
    assert len(model.kv.free) == model.kv.num_pages


def test_generate_refusals_and_defaults(dev, model):
    ids = torch.tensor([[1, 9, 8, 7, 9]]).to(dev)
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        model.generate(ids, do_sample=False, max_new_tokens=2, num_beams=2, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        model.generate(torch.cat([ids, ids], 0), do_sample=False, max_new_tokens=2, padded_batch=True, no_repeat_ngram_size=2)
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            model.generate(ids, do_sample=False, max_new_tokens=2, no_repeat_ngram_size=bad)
    plain = model.generate(ids, do_sample=False, max_new_tokens=4, eos_token_id=-1)
    for off in (None, 0):
        assert torch.equal(model.generate(ids, do_sample=False, max_new_tokens=4, eos_token_id=-1, no_repeat_ngram_size=off), plain)
    assert len(model.kv.free) == model.kv.num_pages


# ---- ServingEngine --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reqs(dev):
    g = torch.Generator().manual_seed(93)
    rnd = lambda n: torch.randint(3, TV, (n,), generator=g).tolist()                    # noqa: E731
    x = rnd(6)
    return [
        dict(input_ids=torch.tensor([[1, -200] + x + rnd(3) + x[:3]]), images=[torch.randn((3, 56, 56), generator=g).bfloat16().to(dev)],
             regions=None, max_new_tokens=10),                                          # an image sentinel in the history, a repeated trigram
        dict(input_ids=torch.tensor([[1] + rnd(19)]), images=None, regions=None, max_new_tokens=8),
        dict(input_ids=torch.tensor([[1] + rnd(30)]), images=None, regions=None, max_new_tokens=6),
    ]


def test_engine_request_equals_solo_generate(dev, model, reqs):
    """A request with SamplingParams(no_repeat_ngram_size=2) returns the tokens of solo generate(no_repeat_ngram_size=2) -- the image
    sentinel is part of both histories -- while an unconstrained request and a `choices` request join and leave around it and keep
    their own tokens; with a repetition penalty on top (one history buffer serves both) it equals its solo run too."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    r = reqs[0]
    S8 = [33, 64, 95, 160, 223, 320, 415, 511]                                    # held to eight ids the free run repeats a bigram: the ban bites
    sp = SamplingParams(no_repeat_ngram_size=2, allowed_token_ids=S8)
    sp_pen = SamplingParams(no_repeat_ngram_size=2, repetition_penalty=1.3)
    solo = _solo(model, dev, r, sp, no_repeat_ngram_size=2, allowed_token_ids=S8)
    solo_pen = _solo(model, dev, r, sp_pen, no_repeat_ngram_size=2)
    free = _solo(model, dev, r, SamplingParams(), allowed_token_ids=S8)
    hist = r["input_ids"][0].tolist()
    for t in solo:                                                                # the solo run itself obeys the rule, sentinel and all
        assert t in S8 and t not in R.banned(TV, hist, 2)
        hist.append(t)
    print("held to eight ids:", free, "with no_repeat_ngram_size=2:", solo)
    assert solo != free                                                           # (the premise: the free run closes a bigram twice)
    nb = SamplingParams(temperature=0.8, seed=5)
    solo_nb = _solo(model, dev, reqs[1], nb)
    choices = [[40, 41], [77]]
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    n = _submit(eng, reqs[1], nb)
    seen = {}
    steps = 0
    while eng.pending():
        if steps == 1:
            a = _submit(eng, r, sp)
            c = eng.submit(reqs[2]["input_ids"], None, None, 6, eos_token_id=2, sampling=SamplingParams(choices=choices))
        if steps == 3:
            p = _submit(eng, r, sp_pen)
        for rid, t in eng.step():
            seen.setdefault(rid, []).append(t)
        if steps == 2:
            live = [q for q in eng.active if q.rid == a][0]
            assert live.hist is not None and live.ban_mask is not None and live.hist[:2].tolist() == [1, -200]
        steps += 1
        assert steps < 100
    assert not eng.failed
    assert seen[a] == solo and seen[p] == solo_pen and seen[n] == solo_nb
    assert seen[c][-1] == 2 and seen[c][:-1] in choices
    for rid, uploads in ((a, 1), (p, 0)):                                          # the static mask is the base: uploaded once; no mask per step
        q = eng.finished[rid]
        assert q.hist is None and q.ban_mask is None and q.ban_seqs is None and q.mask_uploads == uploads
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_bad_words(dev, model, reqs):
    """A request that emits u = (u0, u1, ...) unconstrained emits u0 and then something other than u1 under bad_words=[[u0, u1]]; a
    single-token entry is banned at every step."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    r = reqs[1]
    eng = ServingEngine(model, max_batch=4, kv_pages=64)
    rid = _submit(eng, r, SamplingParams())
    u = eng.run()[rid].tolist()
    assert len(u) >= 2
    b = _submit(eng, r, SamplingParams(bad_words=[[u[0], u[1]]]))
    s = _submit(eng, r, SamplingParams(bad_words=[[u[0]], [u[1], 5, 6]]))
    out = eng.run()
    got, single = out[b].tolist(), out[s].tolist()
    assert got[0] == u[0] and got[1] != u[1], (u, got)
    assert all(not (x == u[0] and y == u[1]) for x, y in zip(got, got[1:]))
    assert u[0] not in single
    assert not eng.failed and eng.finished[b].ban_seqs is None and eng.finished[b].ban_mask is None
    assert len(model.kv.free) == model.kv.num_pages


def test_engine_releases_the_device_buffers(dev, model, reqs):
    """The history and the working mask go where `hist` goes: on retirement, when the request fails on its own (here: its
    allowed_tokens_fn leaves nothing after two tokens) and on cancel; a neighbour with a ban keeps its solo tokens through it."""
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    sp = SamplingParams(no_repeat_ngram_size=3, bad_words=[[7, 8]])
    solo = _solo(model, dev, reqs[0], SamplingParams(), no_repeat_ngram_size=3)
    failing = SamplingParams(no_repeat_ngram_size=2, allowed_tokens_fn=lambda toks: [] if len(toks) == 2 else None)
    eng = ServingEngine(model, max_batch=2, kv_pages=64)
    ok = _submit(eng, reqs[0], sp)
    bad = _submit(eng, reqs[1], failing)
    waiting = _submit(eng, reqs[2], sp)                                              # max_batch 2: it waits
    eng.step()
    live = {q.rid: q for q in eng.active}
    assert live[ok].hist is not None and live[ok].ban_mask is not None and live[ok].ban_seqs is not None
    assert live[bad].hist is not None and live[bad].ban_mask is not None and live[bad].ban_seqs is None
    eng.step()                                                                       # the second token is out: `bad` fails here, alone
    assert bad in eng.failed and [q.rid for q in eng.active] == [ok]
    held = [q for q in eng.waiting if q.rid == waiting][0]
    assert eng.cancel(waiting) and held.hist is None and held.ban_mask is None and held.ban_seqs is None
    out = eng.run()
    fb = eng.failed[bad]
    assert isinstance(fb.error, ValueError) and len(fb.tokens) == 2 and fb.hist is None and fb.ban_mask is None and fb.ban_seqs is None
    done = eng.finished[ok]
    assert done.hist is None and done.ban_mask is None and done.ban_seqs is None
    assert 7 not in solo and int(reqs[0]["input_ids"][0, -1]) != 7                   # ([7, 8] never applied)
    assert out[ok].tolist() == solo
    assert waiting not in out and len(model.kv.free) == model.kv.num_pages
