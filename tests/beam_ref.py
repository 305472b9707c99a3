"""Host restatement of beam search for tests/test_beam_ref_host.py and tests/test_gpu_beam.py: the loop of transformers'
GenerationMixin._beam_search, written per group with whole hypotheses -- no slots, no pages, no scorer object -- and with that loop's own
device of masking by adding -1e9 instead of vitron_amd.beam.BeamScorer's lists, so the two agree only if both follow the algorithm.
Nothing here calls the library: the candidates come from `logprob_topk_fn`."""
import numpy as np

NEG = -1.0e9


def num_candidates(num_beams, n_eos):
    return max(2, 1 + n_eos) * num_beams


def _top(scores, n):
    """indices of the n largest, descending; stable (the earlier index wins a tie)"""
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")[:n]


def beam_search(logprob_topk_fn, groups, num_beams, max_new_tokens, eos_ids, length_penalty=1.0, early_stopping=False,
                num_return_sequences=1):
    """logprob_topk_fn(live) -> for every entry of `live`, the sorted best num_candidates continuations of that group as three lists
    (scores, beams, tokens). `live` is a list of (group, hypotheses, scores): the group's running beams in rank order, each hypothesis
    the list of ids generated so far (one empty hypothesis with score 0 at the first step).
    Returns per group [(score, generated ids)] * num_return_sequences, best first."""
    k = num_beams
    eos = set(int(e) for e in eos_ids)
    n_cand = num_candidates(k, len(eos))
    top_mask = np.arange(n_cand) < k
    run_hyp = [[[]] for _ in range(groups)]
    run_score = [np.zeros(1) for _ in range(groups)]
    fin_hyp = [[None] * k for _ in range(groups)]
    fin_score = [np.full(k, NEG) for _ in range(groups)]
    fin_flag = [np.zeros(k, dtype=bool) for _ in range(groups)]
    unsatisfied = [True] * groups
    alive = [True] * groups
    for step in range(max_new_tokens):
        live = [g for g in range(groups) if alive[g]]
        if not live:
            break
        cands = logprob_topk_fn([(g, run_hyp[g], [float(s) for s in run_score[g]]) for g in live])
        for g, (cs, cb, ct) in zip(live, cands):
            cs = np.asarray(cs, dtype=np.float32)
            assert len(cs) == n_cand and np.all(cs[:-1] >= cs[1:])
            hyps = [run_hyp[g][int(b)] + [int(t)] for b, t in zip(cb, ct)]
            hits = np.array([(int(t) in eos) or (step + 1 >= max_new_tokens) for t in ct])
            # e. the running beams of the next step
            masked = cs.astype(np.float64) + hits * NEG
            nxt = _top(masked, k)
            # f. the finished hypotheses
            fs = (cs / np.float32(float(step + 1) ** length_penalty)).astype(np.float64)
            fs = fs + (NEG if (fin_flag[g].all() and early_stopping is True) else 0.0)
            fs = fs + (0.0 if unsatisfied[g] else NEG)
            just = hits & top_mask
            fs = fs + (~just) * NEG
            m_scores = np.concatenate([fin_score[g], fs])
            m_hyp = fin_hyp[g] + hyps
            m_flag = np.concatenate([fin_flag[g], just])
            keep = _top(m_scores, k)
            fin_score[g], fin_hyp[g], fin_flag[g] = m_scores[keep], [m_hyp[i] for i in keep], m_flag[keep]
            run_hyp[g], run_score[g] = [hyps[i] for i in nxt], masked[nxt]
            # g. can the running beams still improve on the finished ones?
            best_len = max_new_tokens if (early_stopping == "never" and length_penalty > 0.0) else step + 1
            best_possible = float(np.float32(run_score[g][0]) / np.float32(float(best_len) ** length_penalty))
            worst = np.where(fin_flag[g], fin_score[g].min(), NEG)
            unsatisfied[g] = unsatisfied[g] and bool((best_possible > worst).any())
            alive[g] = unsatisfied[g] and not (fin_flag[g].all() and early_stopping is True) and not hits.all()
    return [[(float(fin_score[g][r]), fin_hyp[g][r]) for r in range(num_return_sequences)] for g in range(groups)]
