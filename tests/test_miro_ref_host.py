"""CPU tests of Mirostat v2: the two restatements of tests/miro_ref.py against each other, the property the algorithm
exists for (the observed surprise converges to tau), the ABI of struct vt_miro_row, and every refusal of the Python layers."""
import os
import re
import types

import numpy as np
import pytest

from tests import miro_ref as M
from tests import trunc_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the two restatements -----------------------------------------------------------------------------------------------------------------
def _rows(V, n, seed):
    g = np.random.default_rng(seed * 7919 + V)
    for i in range(n):
        row, temp, k, p = T.draw_row(g, V)
        s = T.scaled(row, temp)
        A = T.base_keep(s, k, p)
        yield s, A, g


@pytest.mark.parametrize("V", [64, 1000, 32000])
def test_restatements_agree_on_random_rows(V):
    """Keep-sets and drawn ids exactly, mu to 1e-12, at cutoffs from below every surprise to above every surprise"""
    for s, A, g in _rows(V, 12 if V < 32000 else 4, 1):
        _, sv = M.surprises(s, A)
        fin = sv[A]
        v = np.unique(fin)                         # (a cutoff AT a surprise is decided by the last bit of q: between two, never at one)
        mid = 0.5 * (v[v.size // 2 - 1] + v[v.size // 2])
        for mu in (fin.min() - 1.0, fin.min() + 1e-9, float(mid), float(g.uniform(fin.min(), fin.max())), fin.max() + 1.0):
            for tau, eta in ((3.0, 0.1), (5.0, 0.25)):
                u = float(g.uniform(0.001, 0.999))
                a, b = M.step(s, A, mu, tau, eta, u), M.llama_step(s, A, mu, tau, eta, u)
                assert np.array_equal(a["K"], b["K"]) and a["count"] == b["count"] and a["id"] == b["id"], (V, mu)
                assert abs(a["mu"] - b["mu"]) <= 1e-12 and abs(a["e"] - b["e"]) <= 1e-12
                assert a["K"][a["id"]] and a["count"] >= 1


@pytest.mark.parametrize("V", [64, 1000, 32000])
def test_restatements_agree_over_trajectories(V):
    """256 steps with the cutoff carried along: counts and ids exactly, mu to 1e-12 at every step"""
    for s, A, g in _rows(V, 2 if V < 32000 else 1, 2):
        u = g.uniform(0.001, 0.999, size=256)
        a = M.trajectory(M.step, s, A, 4.0, 0.1, u)
        b = M.trajectory(M.llama_step, s, A, 4.0, 0.1, u)
        for (ca, ia, ea, ma), (cb, ib, eb, mb) in zip(a, b):
            assert ca == cb and ia == ib and abs(ma - mb) <= 1e-12 and abs(ea - eb) <= 1e-12


def test_the_maximum_always_survives_first_index_on_a_tie():
    s = np.zeros(64)
    s[[9, 40]] = 3.0                              # two equal maxima
    A = np.ones(64, dtype=bool)
    K = M.keep(s, A, -1.0)                        # below every surprise
    assert K.sum() == 1 and K[9]
    assert np.array_equal(K, M.llama_step(s, A, -1.0, 3.0, 0.1, 0.5)["K"])
    K = M.keep(s, A, float("nan"))
    assert K.sum() == 1 and K[9]
    _, sv = M.surprises(s, A)
    K = M.keep(s, A, sv[9])                       # at the maxima's own surprise: both or neither, here both
    assert K.sum() == 2 and K[9] and K[40]
    assert M.keep(s, A, 1e9).sum() == 64
    s2 = np.where(np.arange(64) % 2 == 0, 0.0, -np.inf)
    A2 = np.isfinite(s2)
    assert not (M.keep(s2, A2, 100.0) & ~A2).any()


# the margin of the convergence test: the algorithm's own residual on this row with these seeds (see the test)
CONVERGENCE_MARGIN = 0.1


@pytest.mark.parametrize("tau", [3.0, 5.0])
def test_observed_surprise_converges_to_tau(tau):
    """A fixed Zipf(1.1) row of V = 32000, eta = 0.1: the mean observed surprise over steps 200..2000 lies within 0.1 bit of tau"""
    s = M.zipf_row(32000, 1.1)
    A = np.ones(s.shape, dtype=bool)
    u = np.random.default_rng(int(tau) * 101).uniform(0.0, 1.0, size=2000)
    tr = M.trajectory(M.step, s, A, tau, 0.1, u)
    mean = float(np.mean([e for _, _, e, _ in tr[200:]]))
    print(f"tau={tau}: mean observed surprise over steps 200..2000 = {mean:.4f}")
    assert abs(mean - tau) <= CONVERGENCE_MARGIN, mean


def test_bounds_are_what_the_formats_give():
    b = M.surprise_bound(30.0, 10.0)
    assert 1e-6 < b < 1e-4 and M.surprise_bound(30.0, 10.0, observed_e=True) > b
    assert M.mu_bound(64, 0.1, b, 10.0, 20.0) < 1e-3
    assert np.array_equal(M.fresh_cell(5.0), np.array([10.0, 0.0], np.float32))
    s, A, _ = next(_rows(1000, 1, 3))
    mu, K = M.place_mu(s, A, 20)
    _, sv = M.surprises(s, A)
    assert np.float32(mu) == mu and np.abs(sv[A] - mu).min() > 2 * M.surprise_bound(np.abs(s[A]).max(), mu)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_miro_row_dtype_matches_the_header():
    from vitron_amd import _lib
    from vitron_amd import sampling as S
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_sample_rows_miro\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_sample_rows_miro is not declared in include/vitron_hip.h"
    args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    assert len(args) == 13 == len(_lib.SIGNATURES["vt_sample_rows_miro"][1])
    assert "const vt_miro_row* miro" in args[8] and "const vt_trunc_row* trunc" in args[7]
    doc = hdr[hdr.index("vt_sample_rows_trunc with PER-ROW MIROSTAT"):m.start()]
    table = dict((name, int(off)) for off, name in re.findall(r"^ \*\s+@(\d+)\s+\w+\*? (\w+) ", doc, flags=re.M))
    assert table == {"cell": 0, "tau": 8, "eta": 12} == {n: S.MIRO_ROW_DTYPE.fields[n][1] for n in S.MIRO_ROW_DTYPE.names}, table
    struct = hdr[hdr.index("typedef struct vt_miro_row"):hdr.index("} vt_miro_row;")]
    assert re.findall(r"(\w+);", struct) == list(S.MIRO_ROW_DTYPE.names) and S.MIRO_ROW_BYTES == 16 and S.MIRO_ROW_DTYPE.alignment <= 8
    assert "vt_sample_rows_miro and struct vt_miro_row WITHOUT a bump" in hdr and "Basu" in doc and "llama.cpp" in doc and "tree sums" in doc
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    a = S.miro_rows_array([None, (0x1008, 5.0, 0.1), (0x2000, 0, 0.3)])
    assert a[0].tobytes() == bytes(16)
    assert a[1].tobytes() == np.asarray([0x1008], "<u8").tobytes() + np.asarray([5.0, 0.1], "<f4").tobytes()
    assert a[2]["tau"] == 0
    for bad in ((0x1004, 5.0, 0.1), (0x1008, float("nan"), 0.1), (0x1008, 5.0, -0.1), (0x1008, 5.0, float("inf")), (0x1008, 5.0)):
        with pytest.raises(ValueError):
            S.miro_rows_array([bad])
    import torch
    cell = S.new_miro_cell(5.0, "cpu")
    assert cell.dtype == torch.float32 and cell.tolist() == [10.0, 0.0]
    assert S.pack_miro_rows([None, (cell, 5.0, 0.1)], "cpu").shape == (2, 16)
    with pytest.raises(ValueError, match="cell"):
        S.pack_miro_rows([(torch.zeros(3), 5.0, 0.1)], "cpu")


def test_the_library_refuses_without_a_gpu():
    """The argument checks in front of the launch come back without a device"""
    from vitron_amd import _lib
    for operand in ("bf16", "fp16"):
        lib = _lib.load(operand=operand)
        assert lib.vt_version() == 114 and hasattr(lib, "vt_sample_rows_miro")
        P = 0x10000                  # an aligned non-null address; never dereferenced because validation fails first
        for args, needle in (((None, 1, 64, 64, P, None, None, None, P, P, None, None, None), "null pointer"),
                             ((P, 1, 64, 64, P, None, None, None, P + 4, P, None, None, None), "miro must be 8-byte aligned"),
                             ((P, 1, 64, 64, P, None, None, P + 2, P, P, None, None, None), "trunc must be 4-byte aligned"),
                             ((P, 1, 33000, 33000, P, None, None, None, P, P, None, None, None), "Mirostat runs in the register form only"),
                             ((P, 1, 63, 63, P, None, None, None, P, P, None, None, None), "Mirostat runs in the register form only"),
                             ((P + 4, 1, 64, 64, P, None, None, None, P, P, None, None, None), "Mirostat runs in the register form only"),
                             ((P, 0, 64, 64, P, None, None, None, P, P, None, None, None), "rows=0")):
            assert lib.vt_sample_rows_miro(*args) == -1                            # VT_STATUS_ARG
            assert needle in _lib.last_error(lib), (operand, needle, _lib.last_error(lib))


# ---- the Python layers' refusals ------------------------------------------------------------------------------------------------------------
def _resolve(vocab_size=64, **kw):
    from vitron_amd.picker import resolve_generate_args
    cfg = types.SimpleNamespace(eos_token_id=2, pad_token_id=0, vocab_size=vocab_size, top_k=50, num_hidden_layers=4)
    args = dict(do_sample=True, temperature=1.0, top_p=1.0, top_k=None, max_new_tokens=4, max_length=None, stopping_criteria=None,
                eos_token_id=None, pad_token_id=None, num_beams=1, seed=7, return_logits=False, padded_batch=False, repetition_penalty=1.0,
                return_logprobs=False, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, bad_words_ids=None,
                allowed_token_ids=None, num_return_sequences=1, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=None,
                batch_size=2)
    args.update(kw)
    return resolve_generate_args(cfg, 5, **args)


def test_off_values_are_not_given():
    for off in (dict(), dict(mirostat_tau=None), dict(mirostat_tau=0), dict(mirostat_tau=0.0, mirostat_eta=0.3), dict(mirostat_mode=2),
                dict(mirostat_tau=None, mirostat_mode=0), dict(mirostat_tau=0, mirostat_mode=1),
                dict(mirostat_eta=None), dict(mirostat_tau=0, mirostat_eta=7.0, mirostat_mode=3)):      # off: eta and mode are not looked at
        a = _resolve(**off)
        assert a.mirostat_tau == 0.0 and not a.per_row and a.given == (), off
        assert not _resolve(do_sample=False, num_beams=2, **off).given       # a beam call is not refused for an argument that is off
    a = _resolve(mirostat_tau=5, mirostat_eta=0.2)
    assert a.mirostat_tau == 5.0 and a.mirostat_eta == 0.2 and a.per_row and a.given == ("mirostat_tau=...",)
    # the stages in front compose: none of them is refused with it
    a = _resolve(mirostat_tau=3.0, repetition_penalty=1.2, min_p=0.05, no_repeat_ngram_size=3, top_logprobs=2, sequence_bias={(3,): 1.0},
                 suppress_tokens=[5], guidance_scale=1.5, return_logprobs=True)
    assert a.mirostat_tau == 3.0 and a.truncated and a.ngram == 3
    assert _resolve(mirostat_tau=3.0, dola_layers=[1, 2]).dola


def test_generate_refusals_name_mirostat_tau():
    for bad in (dict(mirostat_tau=-1.0), dict(mirostat_tau=float("nan")), dict(mirostat_tau=float("inf")), dict(mirostat_tau=65.0),
                dict(mirostat_tau="5"), dict(mirostat_tau=True), dict(mirostat_tau=5.0, mirostat_eta=-0.1),
                dict(mirostat_tau=5.0, mirostat_eta=1.5), dict(mirostat_tau=5.0, mirostat_eta=float("nan")),
                dict(mirostat_tau=5.0, mirostat_eta=None), dict(mirostat_tau=5.0, mirostat_mode=3), dict(mirostat_tau=5.0, mirostat_mode="2"),
                dict(mirostat_tau=5.0, mirostat_mode=0)):
        with pytest.raises(ValueError, match="mirostat_"):
            _resolve(**bad)
    from vitron_amd.watermark import SynthIDWatermark
    wm = SynthIDWatermark(dict(ngram_len=5, keys=[1, 2, 3]))
    for bad, name in ((dict(mirostat_mode=1), "mirostat_mode=1"), (dict(do_sample=False), "do_sample=False"),
                      (dict(do_sample=False, num_beams=2), "do_sample=False"), (dict(num_beams=2), "num_beams > 1"),
                      (dict(padded_batch=True), "padded_batch"), (dict(watermarking_config=wm), "watermarking_config"),
                      (dict(vocab_size=32769), "32768")):
        with pytest.raises(NotImplementedError, match="mirostat_tau") as ei:
            _resolve(mirostat_tau=5.0, **bad)
        assert name in str(ei.value), (name, str(ei.value))
    # penalty_alpha > 0 comes with do_sample=False (with do_sample=True its own ValueError stands in front): named by the first of the two
    with pytest.raises(NotImplementedError, match="mirostat_tau"):
        _resolve(mirostat_tau=5.0, do_sample=False, penalty_alpha=0.6, top_k=4)
    from vitron_amd.sampling import check_mirostat_request
    with pytest.raises(NotImplementedError, match=r"mirostat_tau with penalty_alpha > 0"):
        check_mirostat_request(False, 1, 0.6, False, False, 64, "generate(mirostat_tau=...)")


def test_sampling_params_and_check_constraints():
    from vitron_amd.sampling import SamplingParams, check_constraints
    sp = SamplingParams(temperature=0.8, mirostat_tau=5.0)
    assert sp.mirostat and sp.mirostat_eta == 0.1 and "mirostat_tau=5.0" in repr(sp) and "mirostat_eta=0.1" in repr(sp)
    assert sp.replace(seed=3).mirostat_tau == 5.0 and sp.replace(mirostat_tau=None) == SamplingParams(temperature=0.8)
    assert sp != SamplingParams(temperature=0.8) and sp != sp.replace(mirostat_eta=0.2) and hash(sp) == hash(sp.replace())
    for off in (SamplingParams(), SamplingParams(mirostat_tau=None), SamplingParams(mirostat_tau=0), SamplingParams(mirostat_tau=0.0, mirostat_eta=0.5)):
        assert not off.mirostat and "mirostat" not in repr(off)
        check_constraints(off, (2,), 64)
    assert SamplingParams(mirostat_tau=0) == SamplingParams()
    for bad in (dict(mirostat_tau=-1), dict(mirostat_tau=float("nan")), dict(mirostat_tau=65), dict(mirostat_tau=5.0, mirostat_eta=2.0),
                dict(mirostat_tau=5.0, mirostat_eta=-1e-3), dict(mirostat_tau="x")):
        with pytest.raises(ValueError, match="mirostat_"):
            SamplingParams(temperature=0.8, **bad)
    check_constraints(sp, (2,), 64)
    check_constraints(sp.replace(min_p=0.1, repetition_penalty=1.2, no_repeat_ngram_size=2, banned_token_ids=(3,), top_logprobs=2), (2,), 64)
    with pytest.raises(NotImplementedError, match="mirostat_tau") as ei:
        check_constraints(SamplingParams(temperature=0.0, mirostat_tau=5.0), (2,), 64)
    assert "temperature=0" in str(ei.value)
    with pytest.raises(NotImplementedError, match="mirostat_tau") as ei:
        check_constraints(sp.replace(watermarking_config=dict(ngram_len=5, keys=[1, 2, 3])), (2,), 64)
    assert "watermarking_config" in str(ei.value)
    with pytest.raises(NotImplementedError, match="mirostat_tau") as ei:
        check_constraints(sp, (2,), 32769)
    assert "32768" in str(ei.value)
