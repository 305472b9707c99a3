"""Contrastive search restated on the host in fp64 (Su et al. 2022): vt_unit_rows, the d / score / sel of
vt_contrast_rows with their error bounds, and the whole decoding loop given callbacks. transformers no longer ships contrastive_search /
_ranking_fast, so this file is the statement the kernels and generate() are held to, not a copy of an installed arbiter.

Per sequence and step, k = top_k, alpha = penalty_alpha: the candidates are the k most probable ids of the current logit row with their
probabilities p_c (softmax over the full vocabulary); each is run as a decode row behind the same context and gives a final-normed hidden
state h_c; d_c = max_j cos(h_c, bank_j) over ALL earlier positions j; score_c = (1 - alpha) p_c - alpha d_c; the arg-max is emitted (ties
to the lower rank), its h joins the bank and its logit row is the next current row."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                                             # fp32 unit roundoff


def unit_rows(x, w=None):
    """fp64 [rows, H]: (w * x) / |w * x| row by row; a row of zero norm gives zeros. x, w: the fp32 values the kernel reads."""
    y = np.asarray(x, np.float64) * (1.0 if w is None else np.asarray(w, np.float64)[None, :])
    n = np.sqrt((y * y).sum(-1, keepdims=True))
    return np.divide(y, n, out=np.zeros_like(y), where=n > 0)


def dots(bank, cand):
    """fp64 [T, k]: the dot product of every bank row with every candidate (the 16-bit values, widened)"""
    return np.asarray(bank, np.float64) @ np.asarray(cand, np.float64).T


def dot_bound(bank, cand):
    """fp64 [T, k]: tests/gemm_ref.sum_bound for these operands: H 2^-23 sum_i |b_i c_i| (exact products, fp32 additions in any order)"""
    bank, cand = np.asarray(bank, np.float64), np.asarray(cand, np.float64)
    return bank.shape[1] * 2.0 ** -23 * (np.abs(bank) @ np.abs(cand).T)


def d_of(bank, cand):
    """(d fp64 [k], its bound [k]): |max_j a_j - max_j b_j| <= max_j |a_j - b_j|"""
    return dots(bank, cand).max(0), dot_bound(bank, cand).max(0)


def score(alpha, lp, d):
    """fp64 [k]: (1 - alpha) exp(lp) - alpha d with the kernel's constants: alpha as fp32 and 1 - alpha as the fp32 difference"""
    a = F32(alpha)
    om = F32(1.0) - a
    return np.float64(om) * np.exp(np.asarray(lp, F32).astype(np.float64)) - np.float64(a) * np.asarray(d, np.float64)


def score_bound(alpha, lp, d, d_bound):
    """What |kernel score - score()| may be, [k]: alpha times d's bound; (1 - alpha) p times __expf's allowance -- the argument's product
    with the rounded log2 e (2 |lp| u on the exponential) and the 1-ulp hardware exp2 (2 u), as tests/gemm_ref.e_silu states it for the
    same intrinsic; and two roundings: the product (1 - alpha) p and the final fused multiply-add."""
    a = np.float64(F32(alpha))
    om = np.float64(F32(1.0) - F32(alpha))
    lp = np.asarray(lp, F32).astype(np.float64)
    t = om * np.exp(lp)
    s = score(alpha, lp, d)
    return a * np.asarray(d_bound, np.float64) + t * (2.0 * np.abs(lp) + 2.0) * U + U * (np.abs(t) + np.abs(s)) + 2.0 ** -126


def select(scores) -> int:
    """The arg-max, exact ties to the lower index; always inside [0, k) (a NaN never wins)"""
    sel, best = 0, scores[0]
    for c in range(1, len(scores)):
        if scores[c] > best:
            sel, best = c, scores[c]
    return sel


def top_k(logit_row, k):
    """(ids [k], log-probabilities fp64 [k]) of the k most probable tokens: larger logit first, ties by the lower id (vt_logprob_rows' order)"""
    x = np.asarray(logit_row, np.float64)
    order = np.lexsort((np.arange(x.size), -x))[:k]
    m = x.max()
    lse = m + np.log(np.exp(x - m).sum())
    return order.astype(np.int64), x[order] - lse


def contrastive_loop(B, k, max_new_tokens, eos, pad, candidates, step, stop=None):
    """The decoding loop for B sequences. candidates(live) -> for every live sequence (in `live`'s order) its k candidate ids;
    step(live, cands) -> the selection of every live sequence: the callback runs the k candidates of every live sequence, scores them,
    selects, extends the banks and keeps the chosen candidate's cache and logit row. stop(rows) -> bool: the caller's stopping criteria
    over the B rows generated so far (finished rows padded). Returns [B][n]: the generated ids, `pad` behind a row's EOS."""
    eos = set(int(e) for e in eos)
    out = [[] for _ in range(B)]
    live = list(range(B))
    for _ in range(int(max_new_tokens)):
        cands = candidates(live)
        sels = step(live, cands)
        nxt = []
        for j, b in enumerate(live):
            sel = int(sels[j])
            assert 0 <= sel < k
            tok = int(cands[j][sel])
            out[b].append(tok)
            if tok not in eos:
                nxt.append(b)
        for b in range(B):
            if b not in live:
                out[b].append(int(pad))
        live = nxt
        if not live or (stop is not None and stop(out)):
            break
    return out
