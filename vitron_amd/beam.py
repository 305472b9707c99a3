"""Beam search on the host side: the scorer, the slot plan of a KV reorder, and the beam group that owns the pages.

`BeamScorer` is the bookkeeping of transformers' beam search (GenerationMixin._beam_search of the transformers release this project is
tested against) for `groups` prompts and `num_beams` beams in plain Python / numpy. It never sees logits: per group and step it gets the
`num_candidates` best continuations (score, parent beam, token) in rank order -- what ops.beam_step returns -- and answers with the next
beams. `plan_beam_reorder` turns the parents of the next beams into slots and page copies; `BeamGroup` owns the KV pages of one prompt's
beams: the prompt's whole pages are shared and only ever read, every slot owns its tail pages, and the pool's allocator is untouched."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

NEG = -1.0e9          # transformers' "never" score: what an empty finished slot holds


def num_candidates(num_beams: int, n_eos: int) -> int:
    """How many continuations a step keeps per group: max(2, 1 + number of EOS ids) * num_beams, so that num_beams of them are no
    EOS whatever the ranking (transformers' beams_to_keep)."""
    return max(2, 1 + int(n_eos)) * int(num_beams)


class BeamScorer:
    """State of `groups` independent beam searches. Per step, for every group that is not done:

        tokens, parents, scores = scorer.process(g, cand_scores, cand_parents, cand_tokens)

    walks the candidates in rank order. One that hits a stopping criterion -- an EOS id, or the last of max_new_tokens -- inside the
    first num_beams ranks closes a hypothesis (score / generated length ** length_penalty, the EOS included in both); one outside them
    is dropped. The first num_beams candidates that hit none become the next beams. A group is done when its finished hypotheses cannot
    be improved on (early_stopping False / "never": transformers' two heuristics), as soon as num_beams hypotheses are finished
    (early_stopping True), or after max_new_tokens steps, where the best num_beams candidates close. `parents` are the caller's beam
    indices (the cand_parents it passed in); hypotheses are kept whole here, so the caller may place beams where it likes."""

    def __init__(self, groups: int, num_beams: int, max_new_tokens: int, eos_token_ids: Sequence[int] = (), length_penalty: float = 1.0,
                 early_stopping=False):
        if early_stopping not in (False, True, "never"):
            raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
        if num_beams < 1 or max_new_tokens < 1:
            raise ValueError(f"BeamScorer: num_beams={num_beams}, max_new_tokens={max_new_tokens}")
        self.groups, self.k, self.max_new = int(groups), int(num_beams), int(max_new_tokens)
        self.eos = frozenset(int(e) for e in eos_token_ids)
        self.length_penalty = float(length_penalty)
        self.early_stopping = early_stopping
        self.num_candidates = num_candidates(self.k, len(self.eos))
        self.step = [0] * self.groups                               # tokens generated so far
        self.running: List[List[Tuple[float, List[int]]]] = [[(0.0, [])] for _ in range(self.groups)]   # (score, generated ids), by beam
        self.finished: List[List[Tuple[float, Optional[List[int]]]]] = [[(NEG, None)] * self.k for _ in range(self.groups)]
        self.improvable = [True] * self.groups                      # transformers' is_early_stop_heuristic_unsatisfied
        self.exhausted = [False] * self.groups                      # every candidate of the last step hit a stopping criterion

    def _full(self, g: int) -> bool:
        return all(h is not None for _, h in self.finished[g])

    def is_done(self, g: int) -> bool:
        return (not self.improvable[g]) or (self.early_stopping is True and self._full(g)) or self.exhausted[g]

    def beam_scores(self, g: int) -> List[float]:
        return [s for s, _ in self.running[g]]

    def process(self, g: int, cand_scores, cand_parents, cand_tokens):
        """One step of group g. The candidates come in rank order (descending score); cand_parents index the beams of the previous
        step as the caller ordered them (all 0 at the first step). Returns (tokens, parents, scores) of the next beams, num_beams of
        each, in rank order -- empty lists when the step was the last one."""
        if self.is_done(g):
            raise RuntimeError(f"BeamScorer.process: group {g} is done")
        k, n = self.k, len(cand_scores)
        length = self.step[g] + 1                                   # generated length of every candidate, its new token included
        last = length >= self.max_new
        hits = [last or int(t) in self.eos for t in cand_tokens]
        hyp = [self.running[g][int(p)][1] + [int(t)] for p, t in zip(cand_parents, cand_tokens)]
        # the next beams: the best num_beams candidates that hit nothing
        nxt = [i for i in range(n) if not hits[i]][:k]
        if not last and len(nxt) < k:
            raise RuntimeError(f"BeamScorer.process: {n} candidates hold only {len(nxt)} continuations for {k} beams")
        # finished hypotheses: the new ones among the first num_beams ranks join, the best num_beams stay
        if not (self.early_stopping is True and self._full(g)):
            new = [(float(np.float32(cand_scores[i]) / np.float32(float(length) ** self.length_penalty)), hyp[i])
                   for i in range(min(k, n)) if hits[i]]
            merged = self.finished[g] + new
            order = sorted(range(len(merged)), key=lambda i: -merged[i][0])        # stable: an earlier entry wins a tie
            self.finished[g] = [merged[i] for i in order[:k]]
        self.running[g] = [(float(cand_scores[i]), hyp[i]) for i in nxt]
        self.step[g] = length
        self.exhausted[g] = all(hits)
        # can a running beam still beat the worst finished hypothesis? (transformers' _check_early_stop_heuristic)
        if self._full(g) and self.running[g]:
            best_len = self.max_new if (self.early_stopping == "never" and self.length_penalty > 0.0) else length
            best_possible = float(np.float32(self.running[g][0][0]) / np.float32(float(best_len) ** self.length_penalty))
            self.improvable[g] = self.improvable[g] and best_possible > min(s for s, _ in self.finished[g])
        return ([hyp[i][-1] for i in nxt], [int(cand_parents[i]) for i in nxt], [float(cand_scores[i]) for i in nxt])

    def finalize(self, num_return_sequences: int = 1):
        """Per group the best `num_return_sequences` hypotheses: [(score, generated ids)], best first. A hypothesis that closed on an
        EOS carries it. A group that was stopped from outside before it was done contributes its running beams, scored at their
        present length."""
        out = []
        for g in range(self.groups):
            fin = [(s, h) for s, h in self.finished[g] if h is not None]
            if not self.is_done(g) and self.step[g] > 0:
                fin += [(float(np.float32(s) / np.float32(float(self.step[g]) ** self.length_penalty)), h) for s, h in self.running[g]]
                fin.sort(key=lambda e: -e[0])
            if len(fin) < num_return_sequences:
                raise RuntimeError(f"BeamScorer.finalize: group {g} holds {len(fin)} hypotheses, {num_return_sequences} asked for")
            out.append(fin[:num_return_sequences])
        return out


def plan_beam_reorder(parents: Sequence[int]):
    """Where the children of a step live. parents[c]: the slot of child c's parent beam. Returns (slot_of_child, copies): a child whose
    parent's slot has not been kept by an earlier child stays in that slot (no copy); every other child gets a slot whose beam has no
    child this step and one copy (parent's slot -> that slot). Sources are exactly the kept slots and destinations exactly the childless
    ones, so no destination is a source and no spare slot is needed."""
    k = len(parents)
    parents = [int(p) for p in parents]
    if any(not 0 <= p < k for p in parents):
        raise ValueError(f"plan_beam_reorder: parents {parents} outside [0, {k})")
    slot_of_child: List[Optional[int]] = [None] * k
    kept = set()
    for c, p in enumerate(parents):
        if p not in kept:
            kept.add(p)
            slot_of_child[c] = p
    childless = [s for s in range(k) if s not in kept]
    copies = []
    for c, p in enumerate(parents):
        if slot_of_child[c] is None:
            slot_of_child[c] = childless.pop(0)
            copies.append((p, slot_of_child[c]))
    return slot_of_child, copies


class BeamGroup:
    """The KV pages of one prompt's num_beams beams. Takes over the pages of an already prefilled SequenceState: its whole pages
    become the shared prompt, which every slot's page table names and nothing writes again; every slot owns tail pages for the rest of
    the prompt and max_new_tokens more tokens, and the prompt's partial last page is copied into each slot's first tail page. A decode
    step writes position kv_len - 1, which lies in a tail page by construction. `seqs[slot]` is an ordinary SequenceState for
    llama_forward. release() gives every page back exactly once."""

    def __init__(self, llama, kv, prompt_seq, num_beams: int, max_new_tokens: int):
        from . import ops
        from .engine import SequenceState
        self.llama, self.kv, self.k = llama, kv, int(num_beams)
        self.prompt_len = int(prompt_seq.length)
        whole = self.prompt_len // 64
        prompt_pages = list(prompt_seq.pages)
        prompt_seq.pages, prompt_seq.length = [], 0            # the group owns them from here on
        self.shared = prompt_pages[:whole]
        self._owned = list(prompt_pages)                       # every page this group gives back: the prompt's, then the tails
        self.tails: List[List[int]] = []
        self.seqs = []
        try:
            n_tail = (self.prompt_len + int(max_new_tokens) + 63) // 64 - whole
            for _ in range(self.k):
                pages = kv.alloc(n_tail)
                self._owned += pages
                self.tails.append(pages)
            if self.prompt_len % 64:
                ops.kv_copy_pages(kv, [prompt_pages[whole]] * self.k, [t[0] for t in self.tails])
            for t in self.tails:
                s = SequenceState()
                s.pages, s.length = self.shared + t, self.prompt_len
                self.seqs.append(s)
        except BaseException:
            self.release()
            raise

    def reorder(self, parents: Sequence[int]) -> List[int]:
        """Make slot s hold the cache of the child the plan puts there; returns slot_of_child. Copies only the tail pages in use."""
        slot_of_child, copies = plan_beam_reorder(parents)
        length = self.seqs[0].length
        used = (length + 63) // 64 - len(self.shared)
        if copies and used > 0:
            from . import ops
            ops.kv_copy_pages(self.kv, [self.tails[a][j] for a, b in copies for j in range(used)],
                              [self.tails[b][j] for a, b in copies for j in range(used)])
        return slot_of_child

    def release(self) -> None:
        pages, self._owned = self._owned, []
        for s in self.seqs:
            s.pages, s.length = [], 0
        self.kv.release(pages)
