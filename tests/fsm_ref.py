"""Host restatement of vt_fsm_rows' contract (include/vitron_hip.h) in explicit loops, written from the contract's
text; it does not import vitron_amd. An automaton here is a plain dict of Python lists: offsets [n_states + 1], edge_tok / edge_next
[n_edges], info [n_states][2] = {default_next, accept}, plus the row's fields n_states, n_edges, n_eos and eos (four ints). `step` is the
contract's step, `advance` the cell update, `mask` the whole uint32 mask the kernel must write."""
import numpy as np


def words(V: int) -> int:
    return (int(V) + 31) // 32


def table(offsets, edge_tok, edge_next, info, n_states=None, n_edges=None, eos=(), n_eos=None):
    """The fields of one row. n_states / n_edges / n_eos default to what the lists hold; eos is padded to four ints."""
    eos = [int(e) for e in eos]
    return dict(offsets=None if offsets is None else [int(x) for x in offsets],
                edge_tok=None if edge_tok is None else [int(x) for x in edge_tok],
                edge_next=None if edge_next is None else [int(x) for x in edge_next],
                info=None if info is None else [[int(d), int(a)] for d, a in info],
                n_states=(len(info) if info is not None else 0) if n_states is None else int(n_states),
                n_edges=(len(edge_tok) if edge_tok is not None else 0) if n_edges is None else int(n_edges),
                n_eos=len(eos) if n_eos is None else int(n_eos), eos=(eos + [0, 0, 0, 0])[:4])


def _sizes(a):
    """n_states counts as 0 when offsets or state_info is NULL, n_edges as 0 when edge_tok or edge_next is NULL; n_eos into [0, 4]"""
    ns = a["n_states"] if (a["offsets"] is not None and a["info"] is not None and a["n_states"] > 0) else 0
    ne = a["n_edges"] if (a["edge_tok"] is not None and a["edge_next"] is not None and a["n_edges"] > 0) else 0
    return ns, ne, min(max(a["n_eos"], 0), 4)


def step(a, s: int, t: int) -> int:
    ns, ne, n_eos = _sizes(a)
    s, t = int(s), int(t)
    if s < 0 or s >= ns:
        return -1
    lo = min(max(a["offsets"][s], 0), ne)
    hi = min(max(a["offsets"][s + 1], lo), ne)
    nxt = None
    for j in range(lo, hi):                       # (the ids ascend and are unique: a linear search finds what the binary one finds)
        if a["edge_tok"][j] == t:
            nxt = a["edge_next"][j]
            break
    if nxt is None:
        is_eos = False
        for k in range(n_eos):
            if a["eos"][k] == t:
                is_eos = True
        if is_eos:
            nxt = s if a["info"][s][1] != 0 else -1
        else:
            nxt = a["info"][s][0]
    return nxt if 0 <= nxt < ns else -1


def advance(a, cell, gen, gen_len: int):
    """cell {state, consumed} after the launch: gen None counts as gen_len 0; a state that consumed nothing stays as it was"""
    state, consumed = int(cell[0]), max(int(cell[1]), 0)
    n = int(gen_len) if gen is not None else 0
    i = consumed
    while i < n:
        state = step(a, state, gen[i])
        i += 1
    return [state, max(consumed, n)]


def allowed(a, s: int, V: int) -> list:
    return [t for t in range(int(V)) if step(a, s, t) >= 0]


def allowed_fast(a, s: int, V: int) -> np.ndarray:
    """bool [V]: the same set as `allowed` without V searches, in the contract's order of precedence: every id starts with what the
    default edge gives it, the EOS ids get what accept gives them, and a listed edge decides its own id last (the ids of a state are
    unique, so each is decided once). test_fsm_ref_host.py pins it against `allowed`."""
    ns, ne, n_eos = _sizes(a)
    ok = np.zeros((int(V),), dtype=bool)
    if s < 0 or s >= ns:
        return ok
    ok[:] = 0 <= a["info"][s][0] < ns
    for k in range(n_eos):
        e = a["eos"][k]
        if 0 <= e < V:
            ok[e] = a["info"][s][1] != 0
    lo = min(max(a["offsets"][s], 0), ne)
    hi = min(max(a["offsets"][s + 1], lo), ne)
    for j in range(lo, hi):
        t = a["edge_tok"][j]
        if 0 <= t < V:
            ok[t] = 0 <= a["edge_next"][j] < ns
    return ok


def mask(a, s: int, V: int, base=None) -> np.ndarray:
    """uint32 [ceil(V / 32)]: (base, or the bits [0, V)) AND allowed; the bits at positions >= V are clear"""
    W = words(V)
    bits = np.zeros((W * 32,), dtype=bool)
    bits[:V] = allowed_fast(a, s, V)
    m = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
    if base is not None:
        m &= np.asarray(base).view(np.uint32)[:W]
    return m


# ---- seeded random automata, shared by the CPU and the GPU tests ------------------------------------------------------------------------
def random_table(rng, V: int, n_states=None):
    """A valid automaton over [0, V) with 1-12 states: per state 0, 1, a few, about V / 2 or all V ids listed (ascending, unique), next
    states inside the range or -1, a default edge on about half of the states, and 0-4 EOS ids of which some are listed edges, some lie
    outside [0, V)."""
    n = int(rng.integers(1, 13)) if n_states is None else int(n_states)
    offsets, tok, nxt, info = [0], [], [], []
    for _ in range(n):
        kind = int(rng.integers(0, 5))
        k = (0, 1, min(V, int(rng.integers(2, 9))), V // 2, V)[kind]
        ids = np.sort(rng.choice(V, size=k, replace=False)).tolist() if k else []
        tok += ids
        nxt += [int(x) for x in rng.integers(-1, n, size=k)]
        offsets.append(len(tok))
        info.append([int(rng.integers(0, n)) if rng.integers(0, 2) else -1, int(rng.integers(0, 2))])
    n_eos = int(rng.integers(0, 5))
    eos = []
    for _ in range(n_eos):
        r = int(rng.integers(0, 4))
        eos.append(int(tok[int(rng.integers(0, len(tok)))]) if (r == 0 and tok) else (V + 3 if r == 1 else int(rng.integers(0, V))))
    return table(offsets, tok, nxt, info, eos=eos)
