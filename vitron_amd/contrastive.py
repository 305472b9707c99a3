"""Contrastive search on the host side: the candidate group that owns the KV pages of one sequence's k candidates.

A step of contrastive search runs a sequence's k most probable next tokens as k single-query decode rows behind the SAME context and keeps
one of them. `CandidateGroup` gives the k rows their page tables with static ownership and no reference counts, beside beam.BeamGroup:
every completed 64-token page of the context is named by all k tables and never written again; each slot owns only its CURRENT page, the
one position `length` falls into. After the selection the chosen slot's current page is copied onto the other k - 1 -- or, when the step
has just filled it, it becomes shared in every table without a copy and the slots move on to fresh current pages. A step therefore copies
at most k - 1 pages, whatever the generated length (BeamGroup.reorder would copy every tail page in use)."""
from __future__ import annotations

from typing import Callable, List, Optional

PAGE = 64


class CandidateGroup:
    """The KV pages of one sequence's k candidates. Takes over the pages of an already prefilled SequenceState: its whole pages become the
    shared context; slot 0 keeps the prompt's partial last page as its current page and the other slots get a copy of it. Everything the
    group will ever need is taken from the pool here: k current pages and one spare per page the generation can fill. `seqs[slot]` is an
    ordinary SequenceState for llama_forward (pages = the shared ones + the slot's current page): a decode step over them writes position
    `length` into every slot's current page, then select(sel) makes every slot hold the chosen candidate's cache. release() gives every
    page back exactly once. copy_pages(kv, src, dst): ops.kv_copy_pages unless given (both pool formats: it counts bytes)."""

    def __init__(self, llama, kv, prompt_seq, k: int, max_new_tokens: int, copy_pages: Optional[Callable] = None):
        from .engine import SequenceState
        if copy_pages is None:
            from . import ops
            copy_pages = ops.kv_copy_pages
        self.llama, self.kv, self.k, self._copy = llama, kv, int(k), copy_pages
        if self.k < 1 or int(max_new_tokens) < 1:
            raise ValueError(f"CandidateGroup: k={k}, max_new_tokens={max_new_tokens}")
        self.length = int(prompt_seq.length)
        if self.length < 1:
            raise ValueError("CandidateGroup: the prompt sequence is empty")
        whole = self.length // PAGE
        prompt_pages = list(prompt_seq.pages)
        prompt_seq.pages, prompt_seq.length = [], 0            # the group owns them from here on
        self._owned = list(prompt_pages)                       # every page this group gives back
        self.shared: List[int] = prompt_pages[:whole]
        self.current: List[int] = []
        self.spare: List[int] = []
        self.seqs = []
        self.copied = 0                                        # pages copied so far (construction included)
        try:
            partial = self.length % PAGE != 0
            fills = (self.length + int(max_new_tokens)) // PAGE - whole      # pages the steps can fill
            fresh = kv.alloc(self.k - (1 if partial else 0) + fills)
            self._owned += fresh
            if partial:
                self.current = [prompt_pages[whole]] + fresh[:self.k - 1]
                self.spare = fresh[self.k - 1:]
                if self.k > 1:
                    self._copy(kv, [self.current[0]] * (self.k - 1), self.current[1:])
                    self.copied += self.k - 1
            else:
                self.current, self.spare = fresh[:self.k], fresh[self.k:]
            for _ in range(self.k):
                self.seqs.append(SequenceState())
            self._publish()
        except BaseException:
            self.release()
            raise

    def _publish(self) -> None:
        for s, cur in zip(self.seqs, self.current):
            s.pages, s.length = self.shared + [cur], self.length

    def select(self, sel: int) -> int:
        """After a decode step over `seqs` (every slot has written position `length` into its current page): keep slot `sel`'s candidate
        in every slot. Returns the number of pages copied, at most k - 1."""
        sel = int(sel)
        if not 0 <= sel < self.k:
            raise ValueError(f"CandidateGroup.select: sel={sel} outside [0, {self.k})")
        if any(s.length != self.length + 1 for s in self.seqs):
            raise RuntimeError("CandidateGroup.select: the slots have not all taken exactly one step")
        self.length += 1
        n = 0
        if self.length % PAGE == 0:                            # the step filled the page: shared from here on, nobody copies it
            if not self.spare:
                raise RuntimeError("CandidateGroup.select: generated past max_new_tokens")
            self.shared = self.shared + [self.current[sel]]
            self.current[sel] = self.spare.pop(0)              # the other slots start over in the pages they hold
        elif self.k > 1:
            others = [c for i, c in enumerate(self.current) if i != sel]
            self._copy(self.kv, [self.current[sel]] * len(others), others)
            n = len(others)
        self.copied += n
        self._publish()
        return n

    def release(self) -> None:
        pages, self._owned = self._owned, []
        for s in self.seqs:
            s.pages, s.length = [], 0
        self.shared, self.current, self.spare = [], [], []
        self.kv.release(pages)
