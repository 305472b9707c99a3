"""Host restatement of vt_ban_rows' contract (include/vitron_hip.h) in numpy and explicit loops, written from the
contract's text; it does not import vitron_amd. `banned` is the set of ids a row's rules clear, `ban_mask` the whole uint32 mask the
kernel must write (base copied word for word, then bits cleared), `parse_seqs` the reading of the flattened {L, ids...} buffer."""
import numpy as np


def words(V: int) -> int:
    return (int(V) + 31) // 32


def parse_seqs(flat, n_seqs: int, seqs_len: int):
    """The sequences a row's buffer holds: at most n_seqs entries {L, id_0 .. id_{L-1}} read from flat[0 .. seqs_len); an L <= 0 or an
    entry that runs past seqs_len ends the parsing (the entries before it count)."""
    flat = [] if flat is None else [int(t) for t in np.asarray(flat).reshape(-1)]
    end = min(int(seqs_len), len(flat))
    out, pos = [], 0
    for _ in range(max(int(n_seqs), 0)):
        if pos >= end:
            break
        L = flat[pos]
        if L <= 0 or pos + 1 + L > end:
            break
        out.append(flat[pos + 1:pos + 1 + L])
        pos += 1 + L
    return out


def ngram_banned(history, g: int) -> set:
    """NoRepeatNGram: with the last g - 1 ids as the open n-gram, every id that completed the same g - 1 ids earlier in the history."""
    h = [int(t) for t in history]
    n = len(h)
    out = set()
    if g < 1 or n < g - 1:
        return out
    i = 0
    while i + g - 1 < n:                      # i in [0, n - g + 1): position i + g - 1 exists
        same = True
        for k in range(g - 1):
            if h[i + k] != h[n - g + 1 + k]:
                same = False
                break
        if same:
            out.add(h[i + g - 1])
        i += 1
    return out


def seq_banned(history, seqs) -> set:
    h = [int(t) for t in history]
    n = len(h)
    out = set()
    for s in seqs:
        s = [int(t) for t in s]
        L = len(s)
        if L == 1:
            out.add(s[0])
        elif L >= 2 and n >= L - 1 and all(h[n - L + 1 + k] == s[k] for k in range(L - 1)):
            out.add(s[L - 1])
    return out


def banned(V: int, history, g: int = 0, seqs=()) -> list:
    """Sorted ids of [0, V) that the rules clear (an id outside [0, V) is skipped)."""
    return sorted(t for t in ngram_banned(history, g) | seq_banned(history, seqs) if 0 <= t < V)


def ban_mask(V: int, history, g: int = 0, seqs=(), base=None) -> np.ndarray:
    """uint32 [ceil(V / 32)]: base's words as they are (bits >= V included), or the bits [0, V) when base is None; then the banned bits cleared."""
    W = words(V)
    if base is None:
        m = np.full((W,), 0xFFFFFFFF, dtype=np.uint32)
        if V % 32:
            m[W - 1] = np.uint32((1 << (V % 32)) - 1)
    else:
        m = np.array(np.asarray(base).view(np.uint32)[:W], dtype=np.uint32, copy=True)
    for t in banned(V, history, g, seqs):
        m[t >> 5] &= np.uint32(~(1 << (t & 31)) & 0xFFFFFFFF)
    return m


def periodic(n: int, p: int) -> list:
    """h[i] = 7 + i % p: a history in which every rule with g <= n bans something."""
    return [7 + i % p for i in range(n)]


MUST_BAN = [(p, n, g) for p in (2, 3, 5) for n in (64, 257) for g in (1, 2, 3, 4)]
