"""tests/fsm_ref.py (the host restatement of vt_fsm_rows' contract) and vitron_amd.automaton.TokenAutomaton (the product's own) pinned
against each other on seeded random automata; from_choices against sampling.TokenTrie; from_regex against Python's `re` over a
vocabulary whose pieces straddle the DFA's states; the project's own reply format through output_parser; struct vt_fsm_row's packing,
the header, the binding, SamplingParams(automaton=). No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import fsm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS = (31, 32, 33, 100, 1000)


def _automaton(a):
    from vitron_amd.automaton import TokenAutomaton
    return TokenAutomaton(a["offsets"], a["edge_tok"], a["edge_next"], [d for d, _ in a["info"]], [c for _, c in a["info"]])


# ---- the two statements of the contract ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
def test_reference_equals_the_product_on_random_automata(V):
    """100 automata per V (500 in all): step on every state (and two outside the range) for the listed ids, the EOS ids, ids around the
    ends of [0, V) and random ones; the allowed set of every state -- fsm_ref's V explicit calls of step where that is affordable, its
    shortcut everywhere -- against TokenAutomaton.allowed."""
    rng = np.random.default_rng(4100 + V)
    kinds = set()
    for k in range(100):
        a = R.random_table(rng, V)
        A = _automaton(a)
        eos = a["eos"][:a["n_eos"]]
        n = a["n_states"]
        for s in list(range(n)) + [-1, n]:
            lo, hi = (a["offsets"][s], a["offsets"][s + 1]) if 0 <= s < n else (0, 0)
            listed = a["edge_tok"][lo:hi]
            probe = set(listed[:6] + listed[-6:]) | set(eos) | {-3, -1, 0, 1, V - 1, V, V + 3} | {int(t) for t in rng.integers(0, V, size=6)}
            for t in probe:
                assert R.step(a, s, t) == A.step(s, t, eos), (V, k, s, t)
            fast = np.nonzero(R.allowed_fast(a, s, V))[0].tolist()
            assert fast == A.allowed(s, V, eos).tolist(), (V, k, s)
            if (hi - lo + 1) * V <= 40000:
                assert R.allowed(a, s, V) == fast, (V, k, s)
            if 0 <= s < n:
                kinds.add((hi - lo == 0, hi - lo == V, a["info"][s][0] >= 0, -1 in a["edge_next"][lo:hi], bool(set(eos) & set(listed))))
    # what the issue asks the random set to contain: empty states, states with V edges, default edges, -1 edges, EOS ids that are listed
    for i in range(5):
        assert any(kd[i] for kd in kinds) and any(not kd[i] for kd in kinds), i


def test_step_by_hand():
    """One automaton read off the contract line by line: listed edge first, then EOS by accept, then default; clamped edge ranges."""
    #            state 0: 5 -> 1, 7 -> -1 | default 2, not accepting;  state 1: 2 -> 0 (an EOS id listed) | no default, accepting;  state 2: nothing, accepting
    a = R.table([0, 2, 3, 3], [5, 7, 2], [1, -1, 0], [[2, 0], [-1, 1], [-1, 1]], eos=[2, 9])
    assert [R.step(a, 0, t) for t in (5, 7, 2, 9, 4, -6)] == [1, -1, -1, -1, 2, 2]       # 2 and 9 are EOS: the default never covers them
    assert [R.step(a, 1, t) for t in (2, 9, 4)] == [0, 1, -1]                             # listed beats EOS; EOS stays; no default
    assert [R.step(a, 2, t) for t in (2, 9, 4)] == [2, 2, -1]
    assert R.step(a, 3, 5) == -1 and R.step(a, -1, 5) == -1
    assert R.allowed(a, 0, 12) == [0, 1, 3, 4, 5, 6, 8, 10, 11] and R.allowed(a, 1, 12) == [2, 9] and R.allowed(a, -1, 12) == []
    assert [int(w) for w in R.mask(a, 0, 12)] == [0b110101111011] and [int(w) for w in R.mask(a, 0, 12, np.array([0xFFFFFFF0], np.uint32))] == [0b110101110000]
    b = dict(a, n_eos=1)                                                                   # 9 is no EOS id any more
    assert R.step(b, 0, 9) == 2 and R.step(b, 1, 9) == -1
    assert R.step(dict(a, n_eos=7), 2, 9) == 2 and R.step(dict(a, n_eos=-2), 2, 9) == -1   # n_eos clamped into [0, 4]
    c = dict(a, n_edges=1)                                                                 # ranges clamped into [0, n_edges]: 7 and state 1's edge are gone
    assert R.step(c, 0, 5) == 1 and R.step(c, 0, 7) == 2 and R.step(c, 1, 2) == 1
    d = R.table([0, 1], [5], [3], [[4, 1]])                                               # next / default outside [0, n_states): dead
    assert R.step(d, 0, 5) == -1 and R.step(d, 0, 6) == -1
    assert R.step(dict(a, offsets=None), 0, 5) == -1 and R.step(dict(a, edge_next=None), 0, 5) == 2
    # the advance: catches up, is idempotent, never goes back, ignores a NULL gen
    gen = [5, 2, 4, 4]
    assert R.advance(a, [0, 0], gen, 1) == [1, 1] and R.advance(a, [0, 0], gen, 3) == [2, 3] and R.advance(a, [1, 1], gen, 3) == [2, 3]
    assert R.advance(a, [2, 3], gen, 3) == [2, 3] and R.advance(a, [2, 3], gen, 1) == [2, 3] and R.advance(a, [0, -4], gen, 2) == [0, 2]
    assert R.advance(a, [0, 0], gen, 4) == [-1, 4] and R.advance(a, [0, 0], None, 3) == [0, 0] and R.advance(a, [77, -2], gen, 0) == [77, 0]


def test_constructor_validation_and_check():
    from vitron_amd.automaton import TokenAutomaton
    ok = dict(offsets=[0, 2, 2], edge_tok=[3, 5], edge_next=[1, -1], default_next=[-1, 0], accept=[0, 1])
    A = TokenAutomaton(**ok)
    assert A.n_states == 2 and A.n_edges == 2 and A.offsets.dtype == np.int32 and A.state_info().tolist() == [[-1, 0], [0, 1]]
    for bad in (dict(offsets=[0, 2]), dict(offsets=[1, 2, 2]), dict(offsets=[0, 3, 2]), dict(offsets=[0, 1, 1]), dict(edge_tok=[5, 3]),
                dict(edge_tok=[3, 3]), dict(edge_next=[2, -1]), dict(edge_next=[1, -2]), dict(default_next=[-1, 2]), dict(accept=[0]),
                dict(start=2), dict(start=-1), dict(edge_next=[1]), dict(edge_tok=[1.5, 3])):
        with pytest.raises(ValueError):
            TokenAutomaton(**dict(ok, **bad))
    A.check(8, [2])
    with pytest.raises(ValueError, match="at most 4"):
        A.check(8, [1, 2, 4, 6, 7])
    with pytest.raises(ValueError, match="EOS id inside"):
        A.check(8, [8])
    with pytest.raises(ValueError, match="EOS id inside"):
        A.check(8, [])
    with pytest.raises(ValueError, match="start state allows no token"):
        TokenAutomaton([0, 1], [3], [-1], [-1], [0]).check(8, [2])
    with pytest.raises(ValueError, match="start state allows no token"):
        A.check(3, [2])                                                                # the only allowed id lies outside [0, V)
    with pytest.raises(ValueError, match="forbidden edge"):
        TokenAutomaton([0, 1], [2], [-1], [0], [1]).check(8, [2])
    TokenAutomaton([0, 0], [], [], [0], [0]).check(8, [])                              # nothing accepts: no EOS id is needed


# ---- from_choices against TokenTrie -------------------------------------------------------------------------------------------------------
def test_from_choices_is_the_trie():
    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.sampling import TokenTrie
    rng = np.random.default_rng(4200)
    V, eos = 40, [2, 39]
    for _ in range(40):
        choices = [rng.integers(3, 12, size=int(rng.integers(1, 5))).tolist() for _ in range(int(rng.integers(1, 7)))]
        A, trie = TokenAutomaton.from_choices(choices), TokenTrie(choices)
        prefixes = {tuple(c[:k]) for c in choices for k in range(len(c) + 1)}
        for p in prefixes:
            s = A.walk(p, eos)
            assert s >= 0
            want = sorted(trie.children(p) + (eos if trie.ends(p) else []))
            assert A.allowed(s, V, eos).tolist() == want, (choices, p)
            for t in range(3, 12):                                                         # an unknown prefix is dead
                if p + (t,) not in prefixes:
                    assert A.walk(p + (t,), eos) == -1 and A.allowed(-1, V, eos).size == 0
        A.check(V, eos)
    with pytest.raises(ValueError):
        TokenAutomaton.from_choices([])
    with pytest.raises(ValueError):
        TokenAutomaton.from_choices([[3], []])


# ---- from_regex against re ------------------------------------------------------------------------------------------------------------------
SINGLE = list("abcdexymoulrginstAH<>/: .{}]-_0123CBG")
PIECES = ["<module>", "</module>", "</", "mod", "ule>", ": ", "<instruction>", "</instruction>", "<region>", "</region>", "ab", "abb", "cd",
          "ins", "truction>", "<mo", "dule>", "A</", "12", ".5", "aa", "bb", "x: ", "::", "<<", "H</module><instruction>", "reg", "ion>",
          "a: b", "> <", "e>", "<r", "1.", "{x}", "a-", "]]", "cde", "dab", "ba", "xy", "yx", "0.0", "__", "a1", "_a", "<inst", "ruction>x",
          "B", "D", "E", "F", "</instruction><instruction>", "</instruction><region>", "F</", "module>", "/module", "<module>C</module>",
          "k", "v", "k: v", ":", " ", "  "]
VOCAB = [None, "", None] + SINGLE + [""] + PIECES + [None]
EOS = 2                                                                                   # an id without text
PATTERNS = [
    r"abc", r"a.c", r"[a-c]+x", r"[^<]*<module>[A-H]</module>", r"(ab|cd)*e?", r"a{2,3}b{2}c{1,}d{,2}", r"\d+\.\d*", r"(?:mod|ule>)+",
    r"\w+: [^<:]*", r"(<module>|<region>)[A-H]?(</module>|</region>)", r"[\]a\-]+\{x\}", r"(a|b)*abb", r"a{x|\S\s\W\D",
]
FORMAT = r"[^<]*<module>[A-H]</module>(<instruction>[^<:]*: [^<]*</instruction>)+(<region>[^<]*</region>)?"

_compiled = {}


def _compile(pattern):
    from vitron_amd.automaton import TokenAutomaton
    if pattern not in _compiled:
        _compiled[pattern] = TokenAutomaton.from_regex(pattern, VOCAB, eos=[EOS])
    return _compiled[pattern]


def _dense(A):
    """next state [n_states + 1][V] through TokenAutomaton.step, the last row (and -1 as an index) being the dead state"""
    V = len(VOCAB)
    T = np.full((A.n_states + 1, V), -1, dtype=np.int64)
    for s in range(A.n_states):
        for t in range(V):
            T[s, t] = A.step(s, t, [EOS]) if t != EOS else -1
    return T


def _completion(A, T, s):
    """A shortest list of tokens from state s to an accepting state (breadth first over T), or None"""
    seen, todo = {s: []}, [s]
    while todo:
        u = todo.pop(0)
        if A.accept[u]:
            return seen[u]
        for t in np.nonzero(T[u] >= 0)[0]:
            v = int(T[u, t])
            if v not in seen:
                seen[v] = seen[u] + [int(t)]
                todo.append(v)
    return None


def _check_liveness(A, T):
    """Check 3: every state reachable from the start accepts or allows a token, and every allowed edge leads to a state from which an
    accepting state is reachable -- by graph search over the automaton's own tables."""
    reach, todo = {A.start}, [A.start]
    while todo:
        u = todo.pop()
        for v in {int(x) for x in T[u] if x >= 0}:
            if v not in reach:
                reach.add(v)
                todo.append(v)
    for u in reach:
        assert A.accept[u] or (T[u] >= 0).any(), u
        for v in {int(x) for x in T[u] if x >= 0}:
            assert _completion(A, T, v) is not None, (u, v)
    return reach


@pytest.fixture(scope="module")
def texts3():
    """The strings of all token sequences of length <= 3 over the vocabulary's ids that carry text, as one object array per length"""
    ids = [i for i, v in enumerate(VOCAB) if v]
    s1 = np.array([VOCAB[i] for i in ids], dtype=object)
    s2 = (s1[:, None] + s1[None, :])
    s3 = (s2[:, :, None] + s1[None, None, :])
    return ids, s1, s2, s3


@pytest.mark.parametrize("pattern", PATTERNS + [FORMAT])
def test_from_regex_equals_re(pattern, texts3):
    """Checks 1-3 of the issue. Every token sequence of length <= 3 and 2000 seeded random ones of length <= 8: the walk ends in an
    accepting state iff re.fullmatch; a dead sequence has no matching extension among the enumerated ones, a live one has a completion
    (found in the automaton) that re.fullmatch accepts."""
    A = _compile(pattern)
    rx = re.compile(pattern)
    T = _dense(A)
    ids, s1, s2, s3 = texts3
    n = len(ids)
    assert len(VOCAB) >= 100 and n >= 95
    col = np.array(ids)
    st1 = T[A.start, col]                                                                   # [n]
    st2 = T[st1][:, col]                                                                    # [n, n]  (index -1 is the dead last row)
    st3 = T[st2.reshape(-1)][:, col].reshape(n, n, n)
    acc = np.append(A.accept.astype(bool), False)                                           # (index -1: dead)
    match = np.frompyfunc(lambda s: rx.fullmatch(s) is not None, 1, 1)
    m1, m2, m3 = (match(x).astype(bool) for x in (s1, s2, s3))
    assert bool(acc[A.start]) == (rx.fullmatch("") is not None)
    assert np.array_equal(acc[st1], m1) and np.array_equal(acc[st2], m2) and np.array_equal(acc[st3], m3)
    # dead => no enumerated extension matches
    any3 = m3.any(axis=2)
    any2 = (m2 | any3).any(axis=1)
    assert not (any3 & (st2 < 0)).any() and not (m2 & (st2 < 0)).any()
    assert not ((m1 | any2) & (st1 < 0)).any()
    assert not (m3 & (st3 < 0)).any()
    # live => a completion exists and matches
    _check_liveness(A, T)
    done = {}
    for s in {int(x) for x in np.unique(st3) if x >= 0} | {A.start}:
        done[s] = _completion(A, T, s)
        assert done[s] is not None
    for a, b in itertools.islice(zip(*np.nonzero(st2 >= 0)), 300):
        text = s2[a, b] + "".join(VOCAB[t] for t in done.setdefault(int(st2[a, b]), _completion(A, T, int(st2[a, b]))))
        assert rx.fullmatch(text), (pattern, text)
    # random longer sequences, biased towards allowed tokens so that many stay alive
    rng = np.random.default_rng(4300 + len(pattern))
    alive = matched = 0
    for _ in range(2000):
        seq, s = [], A.start
        for _ in range(int(rng.integers(1, 9))):
            ok = np.nonzero(T[s] >= 0)[0] if s >= 0 else []
            u = rng.random()
            near = done.setdefault(s, _completion(A, T, s)) if s >= 0 else None
            t = near[0] if (u < 0.4 and near) else (int(rng.choice(ok)) if (len(ok) and u < 0.85) else int(rng.choice(col)))
            seq.append(t)
            s = int(T[s, t]) if s >= 0 else -1
        assert s == A.walk(seq, [EOS])
        text = "".join(VOCAB[t] for t in seq)
        hit = rx.fullmatch(text) is not None
        assert bool(acc[s]) == hit, (pattern, seq, text)
        if s >= 0:
            alive += 1
            assert rx.fullmatch(text + "".join(VOCAB[t] for t in _completion(A, T, s)))
        matched += hit
    assert alive > 200 and matched > 20, (alive, matched)
    # EOS: allowed exactly in the accepting states, and it leaves the state where it is; ids without text are never allowed
    for s in range(A.n_states):
        assert A.step(s, EOS, [EOS]) == (s if A.accept[s] else -1)
        assert all(A.step(s, t, [EOS]) == -1 for t, v in enumerate(VOCAB) if not v and t != EOS)
    A.check(len(VOCAB), [EOS])


def test_from_regex_details():
    from vitron_amd.automaton import TokenAutomaton
    # '.' does not match a newline, as in re without DOTALL
    A = TokenAutomaton.from_regex(r"a.b", ["a", "b", "\n", "a\nb", "axb"])
    assert A.accept[A.walk([4])] and A.walk([3]) == -1 and A.walk([0, 2]) == -1 and A.accept[A.walk([0, 1, 1])]
    # a free-text state is a default edge with a few exceptions, not V edges
    V = 2000
    vocab = [f"w{i}" for i in range(V - 3)] + ["<", "<end>", None]
    B = TokenAutomaton.from_regex(r"[^<]*<end>", vocab, eos=[V - 1])
    assert B.default_next[B.start] >= 0 and B.n_edges <= 3 * B.n_states
    assert B.allowed(B.start, V, [V - 1]).tolist() == list(range(V - 3)) + [V - 2]          # "<" alone can never be completed: forbidden
    assert B.accept[B.walk([5, 6, V - 2])] and B.walk([5, V - 3]) == -1
    # a pattern the vocabulary cannot satisfy
    with pytest.raises(ValueError, match="no sequence of vocabulary tokens|matches nothing"):
        TokenAutomaton.from_regex(r"abc", ["a", "b", "x"])
    with pytest.raises(ValueError):
        TokenAutomaton.from_regex(r"a", [])


@pytest.mark.parametrize("pattern,needle", [(r"^abc", "anchor"), (r"abc$", "anchor"), (r"\bab", r"escape '\\b'"), (r"(?=a)b", r"group extension"),
                                            (r"(?P<n>a)", "group extension"), (r"a*?b", "lazy"), (r"a++", "possessive"), (r"(a)\1", "back-reference"),
                                            (r"(?i)a", "group extension"), (r"[[:alpha:]]", "POSIX"), (r"*a", "nothing to repeat"),
                                            (r"(ab", "unbalanced"), (r"ab)", "unbalanced"), (r"[ab", "unterminated"), (r"a{3,2}", "min > max"),
                                            (r"\Aab", "escape"), (r"a{1000}", "beyond")])
def test_unsupported_constructs_raise_and_name_themselves(pattern, needle):
    from vitron_amd.automaton import TokenAutomaton
    with pytest.raises(ValueError, match=needle):
        TokenAutomaton.from_regex(pattern, VOCAB)


def test_the_projects_reply_format_parses():
    """200 seeded random walks over the compiled format that take only allowed tokens and stop with EOS in an accepting state: each
    gives a reply output_parser routes -- a module in A-H and a non-empty instruction list."""
    from vitron_amd.output_parser import parse_model_output
    A = _compile(FORMAT)
    V = len(VOCAB)
    T = _dense(A)
    rng = np.random.default_rng(4400)
    rx = re.compile(FORMAT)
    with_region = 0
    for _ in range(200):
        s, seq = A.start, []
        while True:
            ok = A.allowed(s, V, [EOS]).tolist()
            assert ok, (seq, s)
            if len(seq) >= 40:                                                              # long enough: head for the nearest accepting state
                path = _completion(A, T, s)
                t = path[0] if path else EOS
            else:
                t = int(rng.choice(ok))
            if t == EOS:
                assert A.accept[s] and A.step(s, t, [EOS]) == s
                break
            seq.append(t)
            s = A.step(s, t, [EOS])
            assert s >= 0
        text = "".join(VOCAB[t] for t in seq)
        assert rx.fullmatch(text), text
        got = parse_model_output(text)
        assert got.module in list("ABCDEFGH") and got.instruction and len(got.instruction) >= 1, text
        with_region += got.region is not None
    assert 0 < with_region < 200


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------
def test_fsm_row_struct():
    from vitron_amd.sampling import FSM_ROW_BYTES, FSM_ROW_DTYPE, fsm_rows_array
    assert FSM_ROW_BYTES == 96 == FSM_ROW_DTYPE.itemsize
    p = [0x1122334455667788 + i for i in range(8)]
    arr = fsm_rows_array([(p[0], 7, p[1], p[2], p[3], p[4], p[5], p[6], p[7], 5, 9, [2, -1, 31999]), (0, 0, 0x40, 0, 0x80, 0, 0, 0, 0, 0, 0, [])])
    raw = arr.view(np.uint8).reshape(2, 96)
    u64 = lambda r, o: int(raw[r, o:o + 8].view("<u8")[0])                                # noqa: E731
    i32 = lambda r, o: int(raw[r, o:o + 4].view("<i4")[0])                                # noqa: E731
    assert [u64(0, 8 * i) for i in range(8)] == p                                          # gen cell base out offsets edge_tok edge_next state_info
    assert [i32(0, o) for o in range(64, 96, 4)] == [7, 5, 9, 3, 2, -1, 31999, 0]
    assert (u64(1, 8), u64(1, 24), i32(1, 76)) == (0x40, 0x80, 0)
    for bad in ((0, 5, 0x40, 0, 0x80, 0, 0, 0, 0, 0, 0, []), (0, 0, 0x40, 0, 0x80, 0, 0, 0, 0, 2, 0, []), (0, 0, 0x40, 0, 0x80, 0x10, 0, 0, 0x10, 1, 3, []),
                (0, 0, 0x40, 0, 0x80, 0, 0, 0, 0, 0, 0, [1, 2, 3, 4, 5]), (0, 0, -8, 0, 0x80, 0, 0, 0, 0, 0, 0, [])):
        with pytest.raises(ValueError):
            fsm_rows_array([bad])
    # the header's table names the same offsets, the struct the same order
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    doc = hdr[hdr.index("TOKEN AUTOMATA"):hdr.index("typedef struct vt_fsm_row")]
    table = {m.group(2): int(m.group(1)) for m in re.finditer(r"^ \*\s+(\d+) (?:const )?u?int32_t\*?\s+(\w+)", doc, flags=re.M)}
    assert table == {n: FSM_ROW_DTYPE.fields[n][1] for n in FSM_ROW_DTYPE.names}, table
    body = re.search(r"typedef struct vt_fsm_row \{(.*?)\} vt_fsm_row;", hdr, flags=re.S).group(1)
    assert [ln.split()[-1].rstrip(";").split("[")[0] for ln in body.strip().splitlines()] == list(FSM_ROW_DTYPE.names)
    assert "int32_t eos[4];" in body and "96 bytes each" in doc


def test_header_build_and_binding():
    from vitron_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_fsm_rows\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_fsm_rows is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["rows", "n_rows", "V", "stream"]
    assert "const vt_fsm_row* rows" in args
    doc = hdr[hdr.index("TOKEN AUTOMATA"):m.start()]
    for needle in ("bit (i & 31) of word (i >> 5)", "ceil(V / 32)", "NULL", "must NOT alias", "total", "VT_SAMPLE_ROWS_MAX_V", "n_rows == 0",
                   "A default edge never covers an EOS id", "max(consumed, gen_len)", "idempotent", "skipped entirely", "CLEAR", "clamped"):
        assert needle in doc, needle
    assert "vt_fsm_rows and struct vt_fsm_row WITHOUT a bump" in hdr
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    assert len(_lib.SIGNATURES["vt_fsm_rows"][1]) == 4
    assert "vt_fsm.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "vitron_amd", "csrc", "vt_fsm.hip"))
    assert callable(ops.fsm_rows)
    src = open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_kernels.h")).read() + open(os.path.join(ROOT, "vitron_amd", "csrc", "vt_api.hip")).read()
    assert src.count("vt_fsm_rows_launch") >= 2


def test_sampling_params_automaton_is_keyword_only():
    import dataclasses

    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.sampling import SamplingParams, check_constraints, step_allow_mask
    A, B = TokenAutomaton.from_choices([[5, 6], [7]]), TokenAutomaton.from_choices([[5, 6], [7]])
    d = SamplingParams()
    assert d.automaton is None and not d.constrained
    sp = SamplingParams(automaton=A, temperature=0.5)
    assert sp.automaton is A and sp.constrained and not sp.device_bans
    assert "automaton" not in [f.name for f in dataclasses.fields(SamplingParams)]        # the pinned positional field list does not move
    assert SamplingParams(0.5, 1.0, None, 0, 1.0, False, None, None, 0, None, None, 0, None).automaton is None
    with pytest.raises(TypeError):
        SamplingParams(0.5, 1.0, None, 0, 1.0, False, None, None, 0, None, None, 0, None, A)    # no positional slot
    c = sp.replace(seed=3)
    assert c.automaton is A and c.seed == 3 and sp.replace(automaton=None).automaton is None and not sp.replace(automaton=None).constrained
    assert sp == SamplingParams(automaton=A, temperature=0.5) and hash(sp) == hash(SamplingParams(automaton=A, temperature=0.5))
    assert sp != SamplingParams(temperature=0.5) and sp != SamplingParams(automaton=B, temperature=0.5)     # by identity
    assert "automaton=" in repr(sp) and "automaton" not in repr(d)
    with pytest.raises(Exception):
        sp.automaton = B                                                                   # frozen like the rest
    for bad in ("a+", 5, [[5, 6]]):
        with pytest.raises(ValueError, match="automaton"):
            SamplingParams(automaton=bad)
    # the automaton costs no host mask: the step's mask is what the other constraints give
    assert step_allow_mask(sp, 0, [], [2], 64, {}) == (None, None)
    key, mask = step_allow_mask(SamplingParams(automaton=A, banned_token_ids=[9]), 0, [], [2], 64, {})
    assert key == "post" and mask is not None
    check_constraints(sp, [2], 64)


def test_submit_checks_the_automaton_before_queueing():
    import types

    import torch

    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.sampling import SamplingParams
    from vitron_amd.serving import ServingEngine
    stub = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2, vocab_size=64), device="cpu")
    eng = ServingEngine(stub)
    ids = torch.tensor([[1, 5, 6]])
    A = TokenAutomaton.from_choices([[5, 6], [7]])
    with pytest.raises(ValueError, match="at most 4"):
        eng.submit(ids, sampling=SamplingParams(automaton=A), eos_token_id=[2, 3, 4, 5, 6])
    with pytest.raises(ValueError, match="EOS id inside"):
        eng.submit(ids, sampling=SamplingParams(automaton=A), eos_token_id=-1)
    with pytest.raises(ValueError, match="start state allows no token"):
        eng.submit(ids, sampling=SamplingParams(automaton=TokenAutomaton.from_choices([[70]])))
    assert eng.pending() == 0
    rid = eng.submit(ids, sampling=SamplingParams(automaton=A))
    assert eng.pending() == 1 and eng.cancel(rid) and eng.pending() == 0


def test_generate_arguments_resolve_and_refuse():
    import types

    from vitron_amd.automaton import TokenAutomaton
    from vitron_amd.picker import resolve_generate_args
    cfg = types.SimpleNamespace(eos_token_id=2, pad_token_id=0, vocab_size=64, top_k=50)
    base = dict(do_sample=False, temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=4, max_length=None, stopping_criteria=None,
                eos_token_id=None, pad_token_id=None, num_beams=1, seed=None, return_logits=False, padded_batch=False, repetition_penalty=1.0,
                return_logprobs=False, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None,
                allowed_token_ids=None, num_return_sequences=1, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None)
    A = TokenAutomaton.from_choices([[5, 6], [7]])
    a = resolve_generate_args(cfg, 3, **base, automaton=A)
    assert a.automaton is A and a.per_row and not a.constrained
    c = resolve_generate_args(cfg, 3, **base, choices=[[5, 6], [7]])
    assert c.automaton.edge_tok.tolist() == A.edge_tok.tolist() and c.automaton.accept.tolist() == A.accept.tolist()
    assert resolve_generate_args(cfg, 3, **base).automaton is None and not resolve_generate_args(cfg, 3, **base).per_row
    with pytest.raises(NotImplementedError, match="automaton"):
        resolve_generate_args(cfg, 3, **dict(base, num_beams=2), automaton=A)
    with pytest.raises(NotImplementedError, match="automaton"):
        resolve_generate_args(cfg, 3, **dict(base, padded_batch=True), automaton=A)
    with pytest.raises(NotImplementedError, match="automaton"):
        resolve_generate_args(cfg, 3, **dict(base, padded_batch=True), choices=[[5]])
    with pytest.raises(ValueError, match="at most 4"):
        resolve_generate_args(cfg, 3, **dict(base, eos_token_id=[2, 3, 4, 5, 6]), automaton=A)
    with pytest.raises(ValueError, match="EOS id inside"):
        resolve_generate_args(cfg, 3, **dict(base, eos_token_id=-1), automaton=A)
    with pytest.raises(ValueError, match="start state allows no token"):
        resolve_generate_args(cfg, 3, **base, choices=[[64]])
    with pytest.raises(ValueError, match="not both"):
        resolve_generate_args(cfg, 3, **base, automaton=A, choices=[[5]])
    with pytest.raises(ValueError, match="TokenAutomaton"):
        resolve_generate_args(cfg, 3, **base, automaton="a+")
