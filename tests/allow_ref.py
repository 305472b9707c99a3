"""Host restatement of the allow masks of vt_sample_rows_allow (vitron_amd/csrc/vt_sample.hip) for
tests/test_allow_ref_host.py, tests/test_gpu_sample_allow.py and tests/test_gpu_constrained_requests.py: the word / bit layout as an
explicit loop, the -inf edit that DEFINES the kernel's answer (out_ids and kept_count equal vt_sample_rows on the edited logits), the
allowed set of a constrained request as plain Python sets (static ids, min_new_tokens, the choices walk, allowed_tokens_fn; all
intersected). Plain numpy / torch on the CPU; nothing here calls the library or vitron_amd.sampling."""
import numpy as np
import torch


def words(V: int) -> int:
    return (V + 31) // 32


def mask_loop(V: int, allowed=None, banned=None) -> np.ndarray:
    """uint32 [ceil(V / 32)]: bit (i & 31) of word (i >> 5) is set iff token i may be chosen -- one id at a time"""
    m = [0] * words(V)
    for i in (range(V) if allowed is None else allowed):
        m[i >> 5] |= 1 << (i & 31)
    for i in (banned or ()):
        m[i >> 5] &= ~(1 << (i & 31))
    return np.array(m, dtype=np.uint64).astype(np.uint32)


def mask_bool(mask, V: int) -> np.ndarray:
    """bool [V] of a mask; bits at positions >= V are ignored"""
    mask = np.asarray(mask, dtype=np.uint32)
    i = np.arange(V)
    return ((mask[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def masked_logits(x: torch.Tensor, masks) -> torch.Tensor:
    """A copy of fp32 logits [rows][V] with -inf written where row r's mask (None: nothing banned) has a clear bit"""
    out = x.clone()
    V = x.shape[-1]
    for r, m in enumerate(masks):
        if m is not None:
            out[r, torch.from_numpy(~mask_bool(m, V))] = -float("inf")
    return out


def choices_next(choices, tokens, eos_ids):
    """The ids that may follow `tokens` when the reply must be one of `choices` followed by EOS: the next id of every choice that starts
    with `tokens`; the EOS ids as well where `tokens` IS a choice. (A leaf: only EOS. Off every choice: nothing.)"""
    tokens = list(tokens)
    n = len(tokens)
    out = set()
    for c in choices:
        c = list(c)
        if c[:n] == tokens:
            out |= {c[n]} if len(c) > n else set(eos_ids)
    return out


def step_allowed(V, tokens, eos_ids, allowed=None, banned=(), min_new_tokens=0, choices=None, fn=None):
    """The set of ids a request may emit next, or None when nothing constrains the step: allowed minus banned, minus the EOS ids while
    fewer than min_new_tokens have been generated, intersected with the choices walk and with fn(tokens) (None from fn: no constraint)."""
    s = set(range(V)) if allowed is None else set(allowed)
    s -= set(banned)
    constrained = allowed is not None or bool(banned)
    if len(tokens) < min_new_tokens and any(0 <= e < V for e in eos_ids):
        s -= set(eos_ids)
        constrained = True
    if choices is not None:
        s &= choices_next(choices, tokens, [e for e in eos_ids if 0 <= e < V])
        constrained = True
    if fn is not None:
        got = fn(list(tokens))
        if got is not None:
            s &= set(got)
            constrained = True
    return s if constrained else None
