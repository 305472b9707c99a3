"""Token automata for guided decoding: the host side of vt_fsm_rows.

A `TokenAutomaton` is a finite automaton over token ids in the CSR form struct vt_fsm_row names (include/vitron_hip.h): state s lists
the edges [offsets[s], offsets[s + 1]) as (edge_tok, edge_next) with the ids ascending, next -1 meaning "forbidden here"; every other
id follows default_next[s] (-1: forbidden), except the request's EOS ids, which a default edge never covers: they are allowed exactly
in the accepting states and leave the state where it is. `step` / `allowed` are the product's own host statement of that contract;
the device never asks the host: the tables are uploaded once per device (`device_tables`) and shared by every request that runs the
automaton, each with its own two-int cell.

`from_choices` turns the choices of SamplingParams.choices (sampling.TokenTrie) into an automaton, `from_regex` compiles a regular
expression over the STRINGS of a vocabulary: Thompson NFA -> subset construction -> character DFA -> token edges.
"""
from __future__ import annotations

import re as _re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAX_EOS = 4                       # the eos[4] of struct vt_fsm_row
_INF = -1                         # an open upper bound of a repeat


def _i32(x, what: str) -> np.ndarray:
    a = np.asarray(x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"TokenAutomaton: {what} must hold integers")
    a = a.astype(np.int64).reshape(-1)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f"TokenAutomaton: {what} holds a value outside int32")
    return np.ascontiguousarray(a, dtype=np.int32)


class TokenAutomaton:
    """offsets int32 [n_states + 1], edge_tok / edge_next int32 [n_edges], default_next / accept int32 [n_states], start state.
    Validated here: offsets start at 0, do not decrease and end at n_edges; the ids of a state ascend strictly; every next state and
    every default is -1 or inside [0, n_states); the start state exists. Immutable after construction."""

    def __init__(self, offsets, edge_tok, edge_next, default_next, accept, start: int = 0):
        self.offsets = _i32(offsets, "offsets")
        self.edge_tok = _i32(edge_tok, "edge_tok")
        self.edge_next = _i32(edge_next, "edge_next")
        self.default_next = _i32(default_next, "default_next")
        self.accept = (_i32(accept, "accept") != 0).astype(np.int32)
        self.n_states = int(self.default_next.size)
        self.n_edges = int(self.edge_tok.size)
        self.start = int(start)
        n, e = self.n_states, self.n_edges
        if n < 1:
            raise ValueError("TokenAutomaton: at least one state is needed")
        if self.accept.size != n or self.offsets.size != n + 1 or self.edge_next.size != e:
            raise ValueError("TokenAutomaton: offsets must hold n_states + 1 entries, accept n_states, edge_next one entry per edge")
        if self.offsets[0] != 0 or self.offsets[-1] != e or (np.diff(self.offsets) < 0).any():
            raise ValueError("TokenAutomaton: offsets must start at 0, never decrease and end at the number of edges")
        if e > 1:
            inner = np.ones((e,), dtype=bool)                      # inner[j]: edge j belongs to the state of edge j - 1
            starts = self.offsets[:-1]
            inner[starts[starts < e]] = False
            if (inner[1:] & (np.diff(self.edge_tok.astype(np.int64)) <= 0)).any():
                raise ValueError("TokenAutomaton: the token ids of a state's edges must ascend and be unique")
        for name, a in (("edge_next", self.edge_next), ("default_next", self.default_next)):
            if a.size and (a.min() < -1 or a.max() >= n):
                raise ValueError(f"TokenAutomaton: {name} must hold -1 or a state in [0, {n})")
        if not 0 <= self.start < n:
            raise ValueError(f"TokenAutomaton: start={start!r} is no state of [0, {n})")
        for a in (self.offsets, self.edge_tok, self.edge_next, self.default_next, self.accept):
            a.setflags(write=False)
        self._device: Dict[str, dict] = {}

    # ---- the contract on the host -------------------------------------------------------------------------------------------------
    def step(self, s: int, t: int, eos: Iterable[int] = ()) -> int:
        """The state after token t in state s, -1 when dead (vt_fsm_rows' step, include/vitron_hip.h)."""
        s, t = int(s), int(t)
        if not 0 <= s < self.n_states:
            return -1
        lo, hi = int(self.offsets[s]), int(self.offsets[s + 1])
        j = lo + int(np.searchsorted(self.edge_tok[lo:hi], t))
        if j < hi and int(self.edge_tok[j]) == t:
            nx = int(self.edge_next[j])
        elif t in [int(e) for e in list(eos)[:MAX_EOS]]:
            nx = s if self.accept[s] else -1
        else:
            nx = int(self.default_next[s])
        return nx if 0 <= nx < self.n_states else -1

    def walk(self, tokens: Iterable[int], eos: Iterable[int] = (), s: Optional[int] = None) -> int:
        s = self.start if s is None else int(s)
        eos = list(eos)
        for t in tokens:
            s = self.step(s, t, eos)
        return s

    def allowed(self, s: int, V: int, eos: Iterable[int] = ()) -> np.ndarray:
        """Sorted ids of [0, V) that state s allows: step(s, t) >= 0."""
        s, V = int(s), int(V)
        if not 0 <= s < self.n_states:
            return np.zeros((0,), dtype=np.int64)
        ok = np.full((V,), 0 <= int(self.default_next[s]) < self.n_states, dtype=bool)
        for e in list(eos)[:MAX_EOS]:
            if 0 <= int(e) < V:
                ok[int(e)] = bool(self.accept[s])
        lo, hi = int(self.offsets[s]), int(self.offsets[s + 1])
        tok, nxt = self.edge_tok[lo:hi].astype(np.int64), self.edge_next[lo:hi]
        inside = (tok >= 0) & (tok < V)
        ok[tok[inside]] = nxt[inside] >= 0
        return np.nonzero(ok)[0]

    def check(self, V: int, eos: Iterable[int]) -> None:
        """What generate() and submit() refuse before any device work: more than 4 EOS ids; an accepting state without an EOS id in
        [0, V) to end the reply with; an accepting state in which a listed edge forbids every EOS id; a start state that allows nothing."""
        eos = [int(e) for e in eos]
        if len(eos) > MAX_EOS:
            raise ValueError(f"automaton: at most {MAX_EOS} EOS ids (struct vt_fsm_row), got {len(eos)}")
        eos_in = [e for e in eos if 0 <= e < int(V)]
        if self.accept.any() and not eos_in:
            raise ValueError(f"automaton: an accepting state needs an EOS id inside [0, {int(V)}) to end the reply")
        for s in np.nonzero(self.accept)[0]:
            if all(self.step(int(s), e, eos) < 0 for e in eos_in):
                raise ValueError(f"automaton: the accepting state {int(s)} lists every EOS id as a forbidden edge")
        if self.allowed(self.start, V, eos).size == 0:
            raise ValueError("automaton: the start state allows no token")

    # ---- the device form ----------------------------------------------------------------------------------------------------------
    def state_info(self) -> np.ndarray:
        """int32 [n_states][2] = {default_next, accept}: the state_info table of vt_fsm_row"""
        return np.ascontiguousarray(np.stack([self.default_next, self.accept], axis=1), dtype=np.int32)

    def device_tables(self, device) -> dict:
        """The four tables on `device`, uploaded on first use and kept on the object: {"offsets", "edge_tok", "edge_next",
        "state_info"} int32 tensors. Requests that share the automaton share them."""
        import torch
        key = str(torch.device(device))
        got = self._device.get(key)
        if got is None:
            def up(a):
                return torch.from_numpy(np.array(a if a.size else np.zeros((1,), np.int32), dtype=np.int32)).to(device)
            got = self._device[key] = {"offsets": up(self.offsets), "edge_tok": up(self.edge_tok), "edge_next": up(self.edge_next),
                                       "state_info": up(self.state_info().reshape(-1))}
        return got

    def row_fields(self, device) -> tuple:
        """(offsets_ptr, edge_tok_ptr, edge_next_ptr, state_info_ptr, n_states, n_edges) for sampling.fsm_rows_array"""
        t = self.device_tables(device)
        return (t["offsets"].data_ptr(), t["edge_tok"].data_ptr(), t["edge_next"].data_ptr(), t["state_info"].data_ptr(),
                self.n_states, self.n_edges)

    # ---- builders -----------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_states(cls, edges: Sequence[Dict[int, int]], default_next: Sequence[int], accept: Sequence[int], start: int = 0):
        """From one {token id: next state or -1} dict per state."""
        offsets, tok, nxt = [0], [], []
        for d in edges:
            for t in sorted(d):
                tok.append(int(t))
                nxt.append(int(d[t]))
            offsets.append(len(tok))
        return cls(offsets, tok, nxt, default_next, accept, start)

    @classmethod
    def from_choices(cls, choices: Sequence[Sequence[int]]):
        """The trie of sampling.TokenTrie as an automaton: one state per trie node, an edge per child, no default edge; a state
        accepts where a choice ends (so EOS may follow there, and only there)."""
        choices = [[int(t) for t in c] for c in choices]
        if not choices or any(len(c) == 0 for c in choices):
            raise ValueError("TokenAutomaton.from_choices: at least one choice and no empty one")
        edges: List[Dict[int, int]] = [{}]
        accept = [0]
        for c in choices:
            s = 0
            for t in c:
                if t not in edges[s]:
                    edges[s][t] = len(edges)
                    edges.append({})
                    accept.append(0)
                s = edges[s][t]
            accept[s] = 1
        return cls.from_states(edges, [-1] * len(edges), accept, 0)

    @classmethod
    def from_regex(cls, pattern: str, vocab: Sequence[Optional[str]], eos: Iterable[int] = ()):
        """The automaton of the token sequences whose concatenated strings FULLY match `pattern`. vocab: V strings, vocab[t] the text
        of token t (None or "": never allowed). eos: ids that will serve as EOS ids; they get no edge in any state, so the contract's
        EOS rule decides them (allowed in the accepting states). Supported: literals and escapes (\\n \\t \\r \\f \\v \\0, an escaped
        punctuation character, \\d \\w \\s \\D \\W \\S), '.', classes [...] / [^...] with ranges, groups (...) and (?:...), '|', '*',
        '+', '?', '{m}', '{m,}', '{,n}', '{m,n}'. Anything else raises ValueError naming the construct. A state where one next state
        takes more than half of the vocabulary stores it as the default edge and lists the exceptions."""
        vocab = list(vocab)
        V = len(vocab)
        if V == 0:
            raise ValueError("TokenAutomaton.from_regex: an empty vocabulary")
        skip = {int(e) for e in eos}
        texts = [v if (isinstance(v, str) and v and i not in skip) else None for i, v in enumerate(vocab)]
        for i, v in enumerate(vocab):
            if v is not None and not isinstance(v, str):
                raise ValueError(f"TokenAutomaton.from_regex: vocab[{i}] must be a string or None, got {v!r}")
        ast, preds = _parse(pattern)
        chars = sorted({c for v in texts if v for c in v})
        # characters with the same answers to every predicate are one class
        sig_of: Dict[tuple, int] = {}
        cls_of: Dict[str, int] = {}
        for c in chars:
            sig = tuple(p(c) for p in preds)
            cls_of[c] = sig_of.setdefault(sig, len(sig_of))
        sigs = sorted(sig_of, key=sig_of.get)
        trans, acc = _char_dfa(ast, sigs)                                   # trans [S + 1][C], row S is the dead state; acc [S]
        S = len(acc)
        if S == 0:
            raise ValueError(f"TokenAutomaton.from_regex: {pattern!r} matches nothing over this vocabulary")
        # every vocabulary string from every DFA state, one character position at a time
        live = [i for i, v in enumerate(texts) if v]
        target = np.full((S, V), -1, dtype=np.int64)
        if live:
            lens = np.array([len(texts[i]) for i in live])
            C = max(len(sigs), 1)
            codes = np.zeros((len(live), int(lens.max())), dtype=np.int64)
            for k, i in enumerate(live):
                codes[k, :lens[k]] = [cls_of[c] for c in texts[i]]
            cur = np.repeat(np.arange(S, dtype=np.int64)[:, None], len(live), axis=1)
            flat = trans.reshape(-1)
            for pos in range(codes.shape[1]):
                on = lens > pos
                cur[:, on] = flat[cur[:, on] * C + codes[on, pos][None, :]]
            cur[cur == S] = -1
            target[:, np.array(live)] = cur
        # token-level liveness: keep the states reachable from the start over token edges from which an accepting state is reachable
        reach = _reach(target, [0], forward=True)
        good = _reach(target, [s for s in reach if acc[s]], forward=False, within=reach)
        if 0 not in good:
            raise ValueError(f"TokenAutomaton.from_regex: no sequence of vocabulary tokens matches {pattern!r}")
        order = sorted(good)
        new_id = np.full((S + 1,), -1, dtype=np.int64)
        new_id[order] = np.arange(len(order))
        edges, dflt = [], []
        candidates = np.array([i for i in range(V) if i not in skip], dtype=np.int64)
        for s in order:
            row = new_id[target[s]]                                         # [V]: the renumbered next state, -1 forbidden
            vals, counts = np.unique(row[candidates], return_counts=True) if candidates.size else (np.array([-1]), np.array([0]))
            k = int(np.argmax(counts))
            d = int(vals[k]) if (vals[k] >= 0 and counts[k] * 2 > V) else -1
            listed = candidates[row[candidates] != d]
            edges.append({int(t): int(row[t]) for t in listed})
            dflt.append(d)
        a = cls.from_states(edges, dflt, [int(acc[s]) for s in order], 0)
        for s in range(a.n_states):                                         # the property the build guarantees (a cheap self-check)
            if not a.accept[s] and a.allowed(s, V).size == 0:
                raise ValueError(f"TokenAutomaton.from_regex: {pattern!r} has a state that neither accepts nor allows a token")
        return a


def _reach(target: np.ndarray, seeds, forward: bool, within=None) -> set:
    """States reachable from `seeds` over token edges (forward), or from which a seed is reachable (backward), inside `within`."""
    S = target.shape[0]
    succ = [set(int(x) for x in np.unique(target[s]) if x >= 0) for s in range(S)]
    if within is not None:
        succ = [succ[s] & within if s in within else set() for s in range(S)]
    if not forward:
        pred: List[set] = [set() for _ in range(S)]
        for s in range(S):
            for d in succ[s]:
                pred[d].add(s)
        succ = pred
    seen, todo = set(seeds), list(seeds)
    while todo:
        s = todo.pop()
        for d in succ[s]:
            if d not in seen:
                seen.add(d)
                todo.append(d)
    return seen


# ---- the regular expression: parser -> AST ---------------------------------------------------------------------------------------------
_CLASS_ESCAPES = "dwsDWS"
_CHAR_ESCAPES = {"n": "\n", "t": "\t", "r": "\r", "f": "\f", "v": "\v", "0": "\0", "a": "\a"}
_MAX_REPEAT = 256


def _class_pred(letter: str):
    rx = _re.compile("\\" + letter)
    return lambda c: rx.fullmatch(c) is not None


class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError(f"TokenAutomaton.from_regex: the pattern must be a string, got {pattern!r}")
        self.p, self.i, self.preds = pattern, 0, []

    def fail(self, what: str):
        raise ValueError(f"TokenAutomaton.from_regex: unsupported construct {what} at position {self.i} of {self.p!r}")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def atom_pred(self, fn):
        self.preds.append(fn)
        return ("char", len(self.preds) - 1)

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() not in ("", "|", ")"):
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                lo, hi = 0, _INF
            elif c == "+":
                lo, hi = 1, _INF
            elif c == "?":
                lo, hi = 0, 1
            elif c == "{":
                m = _re.compile(r"\{(\d*)(?:(,)(\d*))?\}").match(self.p, self.i)
                if not m or self.p[self.i + 1:self.i + 2] == "}":
                    return node                                              # a literal '{' (as in Python's re): the next atom
                lo = int(m.group(1)) if m.group(1) else 0
                hi = (int(m.group(3)) if m.group(3) else _INF) if m.group(2) else lo
                if hi != _INF and hi < lo:
                    self.fail(f"repeat {m.group(0)!r} with min > max")
                if max(lo, hi) > _MAX_REPEAT:
                    self.fail(f"repeat {m.group(0)!r} beyond {_MAX_REPEAT}")
                self.i = m.end() - 1
            else:
                return node
            self.i += 1
            if self.peek() in ("?", "+"):
                self.fail(f"lazy or possessive quantifier '{c}{self.peek()}'")
            node = ("rep", node, lo, hi)

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] != "?:":
                    self.fail(f"group extension '({self.p[self.i:self.i + 2]}'")
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            return self.atom_pred(lambda ch: ch != "\n")
        if c in "^$":
            self.fail(f"anchor '{c}'")
        if c in "*+?":
            self.fail(f"quantifier '{c}' with nothing to repeat")
        if c == "\\":
            kind, v = self.escape()
            return self.atom_pred(v if kind == "class" else (lambda ch, v=v: ch == v))
        return self.atom_pred(lambda ch, c=c: ch == c)

    def escape(self):
        """after a backslash: ("char", c) or ("class", predicate)"""
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash")
        self.i += 1
        if c in _CLASS_ESCAPES:
            return "class", _class_pred(c)
        if c in _CHAR_ESCAPES:
            return "char", _CHAR_ESCAPES[c]
        if c.isalnum():
            self.i -= 1
            self.fail(f"escape '\\{c}'" + (" (back-reference)" if c.isdigit() else ""))
        return "char", c

    def char_class(self):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        singles, ranges, fns = set(), [], []
        first = True
        while True:
            c = self.peek()
            if c == "":
                self.fail("unterminated '['")
            self.i += 1
            if c == "]" and not first:
                break
            first = False
            if c == "[" and self.peek() == ":":
                self.fail("POSIX class '[:'")
            if c == "\\":
                kind, v = self.escape()
                if kind == "class":
                    fns.append(v)
                    continue
                c = v
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.peek()
                self.i += 1
                if hi == "\\":
                    kind, hi = self.escape()
                    if kind == "class":
                        self.fail("a class escape as the end of a range")
                if ord(hi) < ord(c):
                    self.fail(f"reversed range '{c}-{hi}'")
                ranges.append((c, hi))
            else:
                singles.add(c)

        def pred(ch, singles=frozenset(singles), ranges=tuple(ranges), fns=tuple(fns), negate=negate):
            hit = ch in singles or any(a <= ch <= b for a, b in ranges) or any(f(ch) for f in fns)
            return hit != negate
        return self.atom_pred(pred)


def _parse(pattern: str):
    ps = _Parser(pattern)
    return ps.parse(), ps.preds


# ---- AST -> Thompson NFA -> character DFA over the vocabulary's character classes ---------------------------------------------------------
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.chr: List[List[Tuple[int, int]]] = []      # (predicate, target)

    def new(self) -> int:
        self.eps.append([])
        self.chr.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        if kind == "char":
            a, b = self.new(), self.new()
            self.chr[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                x, y = self.build(item)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for br in node[1]:
                x, y = self.build(br)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):                              # the mandatory copies
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if hi == _INF:                                   # then a star
            x, y = self.build(sub)
            end = self.new()
            self.eps[b] += [x, end]
            self.eps[y] += [x, end]
            return a, end
        end = self.new()
        for _ in range(hi - lo):                         # then optional copies, each of which may leave to the end
            self.eps[b].append(end)
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        self.eps[b].append(end)
        return a, end


def _char_dfa(ast, sigs: Sequence[tuple]):
    """Subset construction over the character classes `sigs` (sig[p]: does a character of the class satisfy predicate p), then the
    states from which no accepting state is reachable are removed. Returns (trans int64 [S + 1][max(C, 1)] with S the dead state,
    accept bool [S]); state 0 is the start. S == 0: the pattern matches nothing at all."""
    nfa = _NFA()
    start, final = nfa.build(ast)

    def closure(states) -> frozenset:
        seen, todo = set(states), list(states)
        while todo:
            for d in nfa.eps[todo.pop()]:
                if d not in seen:
                    seen.add(d)
                    todo.append(d)
        return frozenset(seen)

    C = len(sigs)
    ids = {closure([start]): 0}
    sets = [closure([start])]
    rows: List[List[int]] = []
    k = 0
    while k < len(sets):
        row = []
        for sig in sigs:
            nxt = closure({d for s in sets[k] for p, d in nfa.chr[s] if sig[p]})
            if not nxt:
                row.append(-1)
                continue
            if nxt not in ids:
                ids[nxt] = len(sets)
                sets.append(nxt)
            row.append(ids[nxt])
        rows.append(row)
        k += 1
    n = len(sets)
    acc = [final in st for st in sets]
    pred: List[set] = [set() for _ in range(n)]
    for s, row in enumerate(rows):
        for d in row:
            if d >= 0:
                pred[d].add(s)
    good, todo = {s for s in range(n) if acc[s]}, [s for s in range(n) if acc[s]]
    while todo:
        for s in pred[todo.pop()]:
            if s not in good:
                good.add(s)
                todo.append(s)
    if 0 not in good:
        return np.zeros((1, max(C, 1)), dtype=np.int64), np.zeros((0,), dtype=bool)
    order = [0] + sorted(good - {0})
    S = len(order)
    new = {s: i for i, s in enumerate(order)}
    trans = np.full((S + 1, max(C, 1)), S, dtype=np.int64)
    for s in order:
        for c, d in enumerate(rows[s]):
            if d in new:
                trans[new[s], c] = new[d]
    return trans, np.array([acc[s] for s in order], dtype=bool)
