"""Beam search on the host, pinned: tests/beam_ref.py (the loop-shaped restatement) AND vitron_amd.beam.BeamScorer return
the sequences (exactly) and scores (to 1e-5) of the installed transformers' generate(num_beams=...) on a tiny random CPU Llama -- that
library's own fp32 arithmetic is the reference -- both driven by the model's logits through an fp64 log-softmax and numpy selection;
plan_beam_reorder over every parents vector for k <= 4 and random ones for k = 8, 16; the header and the ctypes signatures. No GPU."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import beam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 97
PAD = 96
EOS = [2, 10, 20, 30, 40, 50, 60, 70, 80, 90]
MAX_NEW = 8
PROMPTS = [[1, 5, 9, 11, 3], [1, 7, 8, 21, 33]]
GRID = [(k, nrs, lp, es) for k in (2, 3, 5) for nrs in sorted({1, k}) for lp in (0.0, 1.0, 2.0) for es in (False, True, "never")]


class _Model:
    """The tiny CPU Llama and a memo of its next-token log-probabilities (fp64 log-softmax of its fp32 logits), shared by every case."""

    def __init__(self):
        from transformers import LlamaConfig, LlamaForCausalLM
        torch.manual_seed(1234)
        cfg = LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                          num_key_value_heads=2, max_position_embeddings=64, pad_token_id=PAD, bos_token_id=1, eos_token_id=2)
        self.m = LlamaForCausalLM(cfg).eval()
        with torch.no_grad():     # a peaked next-token distribution: candidates a long way apart compared with fp32's rounding
            self.m.lm_head.weight.mul_(40.0)
        self.memo = {}

    def logprobs(self, g, hyp):
        key = (g, tuple(hyp))
        if key not in self.memo:
            with torch.no_grad():
                lg = self.m(torch.tensor([PROMPTS[g] + list(hyp)])).logits[0, -1].float()
            self.memo[key] = torch.log_softmax(lg.double(), -1).numpy()
        return self.memo[key]

    def topk(self, g, hyps, scores, n):
        """the n best (score, beam, token) over the beams of one group, descending, ties by the lower flat index"""
        acc = np.concatenate([self.logprobs(g, h) + s for h, s in zip(hyps, scores)])
        order = np.argsort(-acc, kind="stable")[:n]
        return [float(np.float32(acc[i])) for i in order], [int(i) // V for i in order], [int(i) % V for i in order]

    def hf(self, k, nrs, lp, es):
        out = self.m.generate(torch.tensor(PROMPTS), num_beams=k, num_return_sequences=nrs, max_new_tokens=MAX_NEW, eos_token_id=EOS,
                              pad_token_id=PAD, do_sample=False, length_penalty=lp, early_stopping=es, return_dict_in_generate=True,
                              output_scores=True)
        return out.sequences.tolist(), out.sequences_scores.tolist()


@pytest.fixture(scope="module")
def model():
    pytest.importorskip("transformers")
    return _Model()


def _padded(results, longest):
    """[(score, ids)] per group -> rows like generate's: prompt + ids, padded"""
    rows, scores = [], []
    for g, grp in enumerate(results):
        for sc, h in grp:
            rows.append(PROMPTS[g] + list(h) + [PAD] * (longest - len(PROMPTS[g]) - len(h)))
            scores.append(sc)
    return rows, scores


def _run_ref(model, k, nrs, lp, es):
    n = beam_ref.num_candidates(k, len(EOS))
    return beam_ref.beam_search(lambda live: [model.topk(g, hyps, scores, n) for g, hyps, scores in live], len(PROMPTS), k, MAX_NEW, EOS,
                                lp, es, nrs)


def _run_scorer(model, k, nrs, lp, es, stats=None):
    from vitron_amd.beam import BeamScorer
    sc = BeamScorer(len(PROMPTS), k, MAX_NEW, EOS, lp, es)
    assert sc.num_candidates == beam_ref.num_candidates(k, len(EOS))
    beams = {g: ([[]], [0.0]) for g in range(len(PROMPTS))}
    while True:
        live = [g for g in range(len(PROMPTS)) if not sc.is_done(g)]
        if not live:
            break
        for g in live:
            hyps, scores = beams[g]
            cs, cb, ct = model.topk(g, hyps, scores, sc.num_candidates)
            toks, parents, nscores = sc.process(g, cs, cb, ct)
            beams[g] = ([hyps[p] + [t] for p, t in zip(parents, toks)], nscores)
    if stats is not None:
        stats["steps"] = list(sc.step)          # how many steps every group ran
    return sc.finalize(nrs)


@pytest.mark.parametrize("k,nrs,lp,es", GRID)
def test_restatement_and_scorer_equal_transformers(model, k, nrs, lp, es):
    seqs, scores = model.hf(k, nrs, lp, es)
    for name, res in (("beam_ref", _run_ref(model, k, nrs, lp, es)), ("BeamScorer", _run_scorer(model, k, nrs, lp, es))):
        rows, got = _padded(res, len(seqs[0]))
        assert rows == seqs, name
        assert np.abs(np.array(got) - np.array(scores)).max() <= 1e-5, name


def test_hypotheses_close_early_and_groups_finish_early(model):
    """the grid exercises what it is there for: an EOS closes a hypothesis before max_new_tokens, and a group is done before the last step"""
    closed = finished = False
    for k, nrs, lp, es in GRID:
        stats = {}
        res = _run_scorer(model, k, k, lp, es, stats)
        closed = closed or any(len(h) < MAX_NEW and h[-1] in EOS for grp in res for _, h in grp)
        finished = finished or min(stats["steps"]) < MAX_NEW
    assert closed and finished


def _check_plan(parents):
    from vitron_amd.beam import plan_beam_reorder
    k = len(parents)
    slot_of_child, copies = plan_beam_reorder(parents)
    assert sorted(slot_of_child) == list(range(k))
    srcs, dsts = [a for a, _ in copies], [b for _, b in copies]
    assert not set(srcs) & set(dsts) and len(set(dsts)) == len(dsts)
    assert set(dsts) == set(range(k)) - set(parents)                   # exactly the childless slots
    assert set(srcs) <= set(parents)
    labels = [f"beam{s}" for s in range(k)]
    after = list(labels)
    for a, b in copies:
        after[b] = after[a]
    assert [after[slot_of_child[c]] for c in range(k)] == [labels[parents[c]] for c in range(k)]
    return copies


def test_plan_beam_reorder_exhaustive_and_random():
    for k in (1, 2, 3, 4):
        for parents in itertools.product(range(k), repeat=k):
            _check_plan(list(parents))
        assert _check_plan(list(range(k))) == []
    rng = np.random.default_rng(7)
    for k in (8, 16):
        assert _check_plan(list(range(k))) == []
        assert _check_plan(list(rng.permutation(k))) == []            # a permutation moves nothing either
        for _ in range(300):
            _check_plan([int(p) for p in rng.integers(0, k, k)])
            _check_plan([int(p) for p in rng.integers(0, 2, k)])


def test_header_and_signatures():
    from vitron_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    want = {"vt_beam_step": ["logits", "ldl", "V", "groups", "beams_in", "beam_scores", "n_out", "out_scores", "out_tokens", "out_beams",
                             "scratch", "scratch_bytes", "stream"],
            "vt_kv_copy_pages": ["k", "vt", "num_layers", "num_pages", "page_bytes", "src_pages", "dst_pages", "n", "stream"],
            "vt_beam_step_scratch_bytes": ["groups", "beams_in", "n_out"]}
    for sym, names in want.items():
        m = re.search(r"^(?:int|size_t)\s+" + sym + r"\s*\(([^;]*)\);", hdr, flags=re.M)
        assert m, f"{sym} is not declared"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
        assert len(_lib.SIGNATURES[sym][1]) == len(names)
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    src = open(os.path.join(ROOT, "vitron_amd", "build.py")).read()
    assert '"vt_beam.hip"' in src
