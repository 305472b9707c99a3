"""Host side of model.score / model.rank_options: which spliced rows are read, and which token each of them scores.

A causal decoder's logits at spliced row r are the distribution of whatever stands at row r + 1. `score_targets` decides from ONE
sample's input ids and the kinds of its spliced rows (the splice plan of prepare_inputs_labels_for_multimodal) which positions of
input_ids have a log-probability at all:
  * a TEXT token at input position j that lands on spliced row r >= 1 is scored by row r - 1, whatever that row is -- a text token, the
    last row of an image / video block, or a region row: every spliced row is a readable row;
  * the first spliced row has no row before it: a text token that lands there has no target (the first token of the sequence, or a
    token behind a leading <image> whose block holds no rows);
  * an <image> or <objs> sentinel is no token of the vocabulary: its position has no target, and the rows it expands to score nothing
    themselves unless the row behind them is a text token;
  * a token the plan dropped (tokenizer_model_max_length truncation) has no row and no target.
Positions without a target hold NaN / rank 0 in score()'s output. Plain Python; nothing here touches the device."""
from __future__ import annotations

from typing import List, Sequence, Tuple

KIND_TOKEN = 0          # model/llava_arch.py's splice kinds; 1: visual row, 2: region row


def score_targets(ids: Sequence[int], kinds: Sequence[int]) -> Tuple[List[int], List[int], List[int]]:
    """ids: one sample's valid input ids in order (sentinels negative). kinds: the kinds of its spliced rows in order.
    Returns (rows, targets, positions), equally long: spliced row rows[i] is read, it scores token targets[i], which stands at
    position positions[i] of `ids`. rows are strictly increasing."""
    tok_rows = [r for r, k in enumerate(kinds) if int(k) == KIND_TOKEN]
    tok_pos = [j for j, t in enumerate(ids) if int(t) >= 0]
    if len(tok_rows) > len(tok_pos):
        raise ValueError(f"score_targets: the plan holds {len(tok_rows)} token rows, the sample {len(tok_pos)} text tokens")
    rows, targets, positions = [], [], []
    for r, j in zip(tok_rows, tok_pos):          # (zip stops at the shorter: tokens the plan truncated away have no row)
        if r >= 1:
            rows.append(r - 1)
            targets.append(int(ids[j]))
            positions.append(j)
    return rows, targets, positions


def option_score(logprobs: Sequence[float], normalize: str) -> float:
    """The score of one answer option from its tokens' log-probabilities: their sum, or their mean. Added in order, in Python floats."""
    if normalize not in ("sum", "mean"):
        raise ValueError(f"rank_options: normalize must be 'sum' or 'mean', got {normalize!r}")
    total = 0.0
    for v in logprobs:
        total += float(v)
    return total / len(logprobs) if normalize == "mean" else total


def rank_order(scores: Sequence[float]) -> List[int]:
    """Option indices by descending score; ties keep option order (a stable sort). A NaN score goes last."""
    return sorted(range(len(scores)), key=lambda i: (scores[i] != scores[i], -scores[i] if scores[i] == scores[i] else 0.0))
