"""vt_fsm_rows on the GPU, both operand builds: every row's whole mask and its {state, consumed} cell bit for bit
against tests/fsm_ref.py over the vocabulary sizes at which the kernel's paths change -- about 100 rows per launch, each with its own
automaton, state, generated ids, base mask and EOS ids. All buffers of a launch live in ONE image, so every word outside the masks and
the cells is checked too; the same launch repeated changes nothing; a sequence of launches with a growing gen_len equals the reference
walk. Every pointer handed to the kernel stays inside its buffer."""
import numpy as np
import pytest
import torch

from tests import fsm_ref as R

pytestmark = pytest.mark.gpu
VS = (31, 32, 33, 1000, 32000, 32003, 50257)
GUARD = 0x5A5A5A5A
BIG = 2 ** 31 - 1


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _hand_table(V, eos):
    """Six states, one of each kind the contract names. e0, e1: two EOS ids of the row."""
    e0, e1 = eos[0], eos[1]
    ex = sorted({1, 5, V // 2, V - 1} - {e0, e1})
    edges = [
        ({}, -1, 1),                                                                       # 0: no edge, no default, accepting: only EOS
        ({t: (t % 3 if t % 2 else -1) for t in range(V)}, -1, 0),                          # 1: V listed edges, every second one forbidden
        ({**{t: -1 for t in ex[:2]}, **{t: 4 for t in ex[2:]}, 0: 9, 2: 1}, 3, 0),          # 2: default edge, exceptions; 0 -> a next out of range
        ({e0: -1, e1: 0, 3: -1}, 3, 1),                                                    # 3: default edge, accepting, both EOS ids listed
        ({e0: 2, 7: 5, 9: -1, V - 1: 0}, -1, 0),                                           # 4: a few edges, an EOS id listed, not accepting
        ({}, 5, 0),                                                                        # 5: everything but EOS, for ever
    ]
    offsets, tok, nxt, info = [0], [], [], []
    for d, dflt, acc in edges:
        for t in sorted(d):
            tok.append(t)
            nxt.append(d[t])
        offsets.append(len(tok))
        info.append([dflt, acc])
    return offsets, tok, nxt, info


def _row(ai, cell, gen=(), gen_len=None, base=0, eos=None, n_eos=None, out_null=False, cell_null=False, gen_null=False, fields=None):
    return dict(ai=ai, cell=[int(cell[0]), int(cell[1])], gen=[int(t) for t in gen], gen_len=len(gen) if gen_len is None else int(gen_len),
                base=base, eos=eos, n_eos=n_eos, out_null=out_null, cell_null=cell_null, gen_null=gen_null, fields=fields or {})


_built = {}


def _cases(V):
    """(automata, rows, expected masks, expected cells) of one launch at vocabulary V, built once and shared by both builds"""
    if V in _built:
        return _built[V]
    rng = np.random.default_rng(8000 + V)
    W = R.words(V)
    e0, e1 = 2, V - 2
    autos = [R.table(*_hand_table(V, (e0, e1)), eos=[e0, e1])]
    for _ in range(3):
        autos.append(R.random_table(rng, V))
    autos.append(R.table([0, 1, 1], [4], [1], [[-1, 0], [1, 1]], eos=[e0]))                 # a two-state automaton, for the degenerate fields

    def tokens(a, s, n):
        """n ids to generate from state s: listed ids of the state reached, EOS ids, random ids, a negative one, one >= V"""
        out = []
        for _ in range(n):
            lo, hi = (a["offsets"][s], a["offsets"][s + 1]) if 0 <= s < a["n_states"] else (0, 0)
            k = int(rng.integers(0, 10))
            if k < 5 and hi > lo:
                t = a["edge_tok"][int(rng.integers(lo, hi))]
            elif k == 5 and a["n_eos"]:
                t = a["eos"][int(rng.integers(0, a["n_eos"]))]
            elif k == 6:
                t = -int(rng.integers(1, 300))
            elif k == 7:
                t = V + int(rng.integers(0, 5))
            else:
                t = int(rng.integers(0, V))
            out.append(t)
            s = R.step(a, s, t)
        return out

    rows = []
    for s in range(6):                                                                     # every kind of state, every kind of base
        for base in (0, 1, 2):
            rows.append(_row(0, (s, 0), base=base))
    for s in (0, 3, 4):                                                                    # n_eos 0, 1, 4 (with a duplicate and an id >= V), and clamped
        for eos, n_eos in (([e0, e1], 0), ([e0, e1], 1), ([e1, e0, e1, V + 1], 4), ([e0, e1, 7, 9], 9), ([e0, e1], -3)):
            rows.append(_row(0, (s, 0), eos=eos, n_eos=n_eos, base=len(rows) % 3))
    for st in (-1, 6, BIG, -BIG - 1):                                                      # dead cells and cells out of range
        rows.append(_row(0, (st, 0), base=len(rows) % 3))
        rows.append(_row(0, (st, 0), gen=[5, 7], base=len(rows) % 3))
    for ai in (0, 1, 2, 3):                                                                # consumed behind by 0, 1 and 5, ahead, negative
        a = autos[ai]
        for behind in (0, 1, 5, 1, 5):
            n = int(rng.integers(behind, behind + 4))
            s0 = int(rng.integers(0, a["n_states"]))
            gen = tokens(a, s0, n)
            mid = R.advance(a, [s0, 0], gen, n - behind)                                   # where the cell stands, `behind` ids back
            rows.append(_row(ai, mid, gen=gen, base=len(rows) % 3))
        gen = tokens(a, 0, 4)
        rows.append(_row(ai, (0, 6), gen=gen, base=1))                                     # consumed ahead of gen_len: nothing moves, consumed stays
        rows.append(_row(ai, (0, -7), gen=gen, gen_len=2))                                 # a negative consumed counts as 0
        rows.append(_row(ai, (0, 0), gen=gen, gen_len=0))                                  # gen_len 0 with a buffer
        rows.append(_row(ai, (0, 0), gen=gen, gen_len=-5))
        rows.append(_row(ai, (0, 1), gen=gen, gen_null=True, gen_len=3, base=2))           # gen NULL advances nothing
        rows.append(_row(ai, (0, 0), gen=[-1, V, V + 100, -BIG - 1, BIG]))                 # ids outside [0, V) step like any other id
    rows.append(_row(0, (2, 0), gen=[8], out_null=True))                                   # skipped entirely: the cell stays what it was
    rows.append(_row(0, (2, 0), gen=[8], cell_null=True, base=1))
    rows.append(_row(1, (0, 0), out_null=True, cell_null=True))
    # degenerate table fields: counts beyond, at and below the tables' lengths are clamped or dead; nothing outside the tables is read
    for f in (dict(n_edges=0), dict(n_edges=-4), dict(n_states=0), dict(n_states=-1), dict(n_states=1), dict(offsets=None), dict(edge_tok=None),
              dict(edge_next=None), dict(info=None)):
        rows.append(_row(4, (0, 0), gen=[4], fields=f))
        rows.append(_row(4, (0, 0), fields=f, base=1))
    while len(rows) < 124:                                                                 # random rows over the random automata
        ai = int(rng.integers(1, 4))
        a = autos[ai]
        s0 = int(rng.integers(-1, a["n_states"] + 1))
        gen = tokens(a, s0, int(rng.integers(0, 4)))
        rows.append(_row(ai, (s0, 0), gen=gen, base=len(rows) % 3))

    def base_words(kind):
        if kind == 0:
            return None
        b = rng.integers(0, 2 ** 32, size=W, dtype=np.uint64).astype(np.uint32)
        if V % 32:
            if kind == 1:
                b[-1] &= np.uint32((1 << (V % 32)) - 1)
            else:
                b[-1] |= np.uint32(0xFFFFFFFF ^ ((1 << (V % 32)) - 1))                      # bits at positions >= V set: out has them CLEAR
        return b

    want_mask, want_cell = [], []
    memo = {}
    for c in rows:
        a = dict(autos[c["ai"]])
        if c["eos"] is not None:
            a["eos"], a["n_eos"] = (list(c["eos"]) + [0, 0, 0, 0])[:4], len(c["eos"])
        if c["n_eos"] is not None:
            a["n_eos"] = c["n_eos"]
        a.update(c["fields"])
        c["auto"] = a
        c["base_words"] = base_words(c["base"])
        if c["out_null"] or c["cell_null"]:
            want_mask.append(None)
            want_cell.append(None)
            continue
        cell = R.advance(a, c["cell"], None if c["gen_null"] else c["gen"], c["gen_len"])
        key = (c["ai"], cell[0], tuple(a["eos"]), a["n_eos"], tuple(sorted((k, v is None, v if isinstance(v, int) else 0) for k, v in c["fields"].items())))
        if key not in memo:
            memo[key] = R.allowed_fast(a, cell[0], V)
        bits = np.zeros((W * 32,), dtype=bool)
        bits[:V] = memo[key]
        m = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
        if c["base_words"] is not None:
            m = m & c["base_words"]
        want_mask.append(m)
        want_cell.append(cell)
    kinds = {(c["auto"]["n_eos"], c["cell"][0] < 0, c["gen_len"] > c["cell"][1]) for c in rows}
    assert len(rows) >= 100 and len(kinds) > 8
    pop = [int(np.unpackbits(m.view(np.uint8)).sum()) for m in want_mask if m is not None]
    assert sum(0 < p < V for p in pop) >= 20 and 0 in pop                                  # non-vacuity: masks with structure, and dead rows
    _built[V] = (autos, rows, want_mask, want_cell)
    return _built[V]


def _layout(V, autos, rows, want_mask, want_cell):
    """All buffers of the launch in ONE int32 image, at least one guard word between any two: every automaton's four tables once, then
    per row gen, cell, base and out. out / base sit on a 16-byte boundary or off it in every combination. Returns (image before, image
    expected after, struct fields with word offsets in the pointer slots)."""
    from vitron_amd.sampling import FSM_ROW_DTYPE
    W = R.words(V)
    chunks, pos = [], 4

    def put(vals, aligned):
        nonlocal pos
        pos += 1
        pos += (-pos) % 4
        if not aligned:
            pos += 1 + len(chunks) % 3
        off = pos
        chunks.append((off, np.asarray(vals, dtype=np.int64)))
        pos += len(vals)
        return off

    tabs = []
    for a in autos:
        tabs.append(dict(offsets=put(a["offsets"], True), edge_tok=put(a["edge_tok"] or [GUARD], True), edge_next=put(a["edge_next"] or [GUARD], True),
                         info=put([x for p in a["info"] for x in p], True)))
    fields = np.zeros((len(rows),), dtype=FSM_ROW_DTYPE)
    at = []
    for i, c in enumerate(rows):
        a, t = c["auto"], tabs[c["ai"]]
        n_gen = max(c["gen_len"], len(c["gen"]), 1)
        go = put((c["gen"] + [GUARD] * n_gen)[:n_gen], False)
        co = put(c["cell"], i % 2 == 0)
        bo = None if c["base_words"] is None else put(c["base_words"].astype(np.int64), i % 4 in (0, 1))
        oo = put([GUARD] * W, i % 4 in (0, 2))
        at.append((co, oo))
        assert c["gen_len"] <= len(c["gen"]) or c["gen_null"]                              # every pointer stays inside its buffer
        assert a["n_states"] <= len(autos[c["ai"]]["info"]) and a["n_edges"] <= max(len(autos[c["ai"]]["edge_tok"]), 0)
        fields[i] = (0 if c["gen_null"] else go, 0 if c["cell_null"] else co, 0 if bo is None else bo, 0 if c["out_null"] else oo,
                     0 if a["offsets"] is None else t["offsets"], 0 if a["edge_tok"] is None else t["edge_tok"],
                     0 if a["edge_next"] is None else t["edge_next"], 0 if a["info"] is None else t["info"],
                     c["gen_len"], a["n_states"], a["n_edges"], a["n_eos"], a["eos"])
    img = np.full((pos + 8,), GUARD, dtype=np.int64)
    for off, w in chunks:
        img[off:off + len(w)] = w
    before = (img & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    after = before.copy()
    for (co, oo), m, cell in zip(at, want_mask, want_cell):
        if m is not None:
            after[oo:oo + W] = m.view(np.int32)
            after[co:co + 2] = np.asarray(cell, dtype=np.int64).astype(np.int32)
    return before, after, fields, at


PTRS = ("gen", "cell", "base", "out", "offsets", "edge_tok", "edge_next", "state_info")


def _rows_dev(buf, fields, dev):
    f = fields.copy()
    for name in PTRS:                                                                      # word offsets -> device addresses (0 stays NULL)
        f[name] = np.where(fields[name] != 0, buf.data_ptr() + 4 * fields[name].astype(np.uint64), 0).astype(np.uint64)
    return torch.from_numpy(f.view(np.uint8).reshape(len(f), 96).copy()).to(dev)


@pytest.mark.parametrize("operand", ("bf16", "fp16"))
@pytest.mark.parametrize("V", VS)
def test_fsm_rows_equals_the_reference_bit_for_bit(dev, V, operand):
    """Every row's mask and cell equal fsm_ref; everything else in the image -- tables, generated ids, bases, skipped rows' cells and
    masks, the guard words -- is what it was. The same launch once more leaves the image as it is: the advance is idempotent."""
    from vitron_amd import _lib
    autos, rows, want_mask, want_cell = _cases(V)
    before, after, fields, at = _layout(V, autos, rows, want_mask, want_cell)
    lib = _lib.load(operand=operand)
    buf = torch.from_numpy(before.copy()).to(dev)
    rows_dev = _rows_dev(buf, fields, dev)
    stream = torch.cuda.current_stream().cuda_stream
    W = R.words(V)
    for launch in (1, 2):
        st = lib.vt_fsm_rows(rows_dev.data_ptr(), len(rows), V, stream)
        torch.cuda.synchronize()
        assert st == 0, _lib.last_error(lib)
        got = buf.cpu().numpy()
        if not np.array_equal(got, after):
            for i, (c, m, cell) in enumerate(zip(rows, want_mask, want_cell)):
                if m is None:
                    continue
                co, oo = at[i]
                what = (V, launch, i, c["ai"], c["cell"], c["gen"][:6], c["gen_len"], c["base"], c["auto"]["n_eos"], c["fields"])
                assert got[co:co + 2].tolist() == np.asarray(cell, dtype=np.int64).astype(np.int32).tolist(), what
                assert np.array_equal(got[oo:oo + W], m.view(np.int32)), what
            assert False, ("a word outside the masks and cells changed", launch, np.flatnonzero(got != after)[:8].tolist())


def test_growing_gen_len_equals_the_reference_walk(dev):
    """ops.fsm_rows + sampling.pack_fsm_rows + TokenAutomaton.device_tables: three rows share one automaton's tables. Row 0 is launched at
    every step, row 1 at every third step (it catches up), row 2 runs another automaton; after every launch the cells and masks are the
    reference's for the ids generated so far."""
    from vitron_amd import ops
    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.sampling import pack_fsm_rows
    V, eos = 1000, [2]
    W = R.words(V)
    A = TokenAutomaton.from_choices([[5, 6, 7, 8, 9, 10], [5, 6, 40], [5, 6, 7, 8, 9, 11, 12]])
    vocab = [None, None, None] + [chr(97 + i % 26) * (1 + i % 3) for i in range(V - 3)]
    B = TokenAutomaton.from_regex(r"a+(bb|c)*d?", vocab, eos=eos)
    assert A.device_tables(dev) is A.device_tables(dev) and A.device_tables(dev)["offsets"].device.type == "cuda"
    gens = [[5, 6, 7, 8, 9, 11, 12, 2, 2], [5, 6, 40, 2, 7, 7, 7, 7, 7], [3, 29, 4, 5, 5, 6, 2, 3, 3]]
    autos = [A, A, B]
    ref = [R.table(X.offsets.tolist(), X.edge_tok.tolist(), X.edge_next.tolist(), X.state_info().tolist(), eos=eos) for X in autos]
    gen_dev = [torch.tensor(g, dtype=torch.int32, device=dev) for g in gens]
    cells = torch.tensor([[X.start, 0] for X in autos], dtype=torch.int32, device=dev)
    outs = torch.full((3, W + 1), GUARD, dtype=torch.int32, device=dev)
    want = [[X.start, 0] for X in autos]
    seen_dead = seen_accept = False
    for step in range(len(gens[0]) + 1):
        live = [b for b in range(3) if b != 1 or step % 3 == 0]
        rows = [(gen_dev[b].data_ptr() if step else 0, step, cells[b].data_ptr(), 0, outs[b].data_ptr(), *autos[b].row_fields(dev), eos) for b in live]
        packed = pack_fsm_rows(rows, dev)
        assert packed.shape == (len(live), 96) and packed.dtype == torch.uint8
        ops.fsm_rows(packed, len(live), V)
        torch.cuda.synchronize()
        got_cells, got = cells.cpu().tolist(), outs.cpu().numpy()
        for b in live:
            want[b] = R.advance(ref[b], want[b], gens[b], step)
            assert want[b] == [autos[b].walk(gens[b][:step], eos), step]                   # (the product's host walk agrees)
        for b in range(3):
            assert got_cells[b] == want[b], (step, b)
            if b in live:
                assert np.array_equal(got[b][:W], R.mask(ref[b], want[b][0], V).view(np.int32)), (step, b)
                assert sorted(np.flatnonzero(np.unpackbits(got[b][:W].view(np.uint8), bitorder="little")).tolist()) \
                    == autos[b].allowed(want[b][0], V, eos).tolist()
            assert got[b][W] == GUARD
        seen_dead |= any(w[0] < 0 for w in want)
        seen_accept |= any(w[0] >= 0 and autos[b].accept[w[0]] for b, w in enumerate(want))
    assert seen_dead and seen_accept


def test_refusals_and_no_rows(dev):
    from vitron_amd import _lib, ops
    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.sampling import pack_fsm_rows
    lib = _lib.load()
    A = TokenAutomaton.from_choices([[1], [40]])
    out = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
    cell = torch.tensor([0, 0], dtype=torch.int32, device=dev)
    packed = pack_fsm_rows([(0, 0, cell.data_ptr(), 0, out.data_ptr(), *A.row_fields(dev), [2])], dev)
    stream = torch.cuda.current_stream().cuda_stream
    for n_rows, V, ptr, needle in ((1, 0, packed.data_ptr(), "V=0"), (1, -5, packed.data_ptr(), "V=-5"), (1, 262145, packed.data_ptr(), "V=262145"),
                                   (-1, 64, packed.data_ptr(), "n_rows=-1"), (1, 64, None, "NULL")):
        assert lib.vt_fsm_rows(ptr, n_rows, V, stream) == -1                      # VT_STATUS_ARG, with a message
        assert needle in _lib.last_error(lib), (needle, _lib.last_error(lib))
    assert lib.vt_fsm_rows(None, 0, 64, stream) == 0 and lib.vt_fsm_rows(packed.data_ptr(), 0, 64, stream) == 0
    ops.fsm_rows(packed, 0, 64)                                                   # n_rows == 0: a success that launches nothing
    with pytest.raises(_lib.VitronHipError, match="V=0"):
        ops.fsm_rows(packed, 1, 0)
    with pytest.raises(_lib.VitronHipError):
        ops.fsm_rows(packed, 2, 64)                                               # 96 bytes are one row, not two
    with pytest.raises(_lib.VitronHipError):
        ops.fsm_rows(packed.cpu(), 1, 64)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all() and cell.cpu().tolist() == [0, 0]   # nothing was launched
    ops.fsm_rows(packed, 1, 64)
    big = torch.full((262144 // 32 + 1,), GUARD, dtype=torch.int32, device=dev)   # the largest legal V runs too (the LDS mask at its full size)
    ops.fsm_rows(pack_fsm_rows([(0, 0, cell.data_ptr(), 0, big.data_ptr(), *A.row_fields(dev), [2])], dev), 1, 262144)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert got[0] == 2 and got[1] == 1 << 8 and (got[2:-1] == 0).all() and got[-1] == GUARD
    assert out.cpu().numpy().tolist() == [2, 1 << 8, GUARD, GUARD]
