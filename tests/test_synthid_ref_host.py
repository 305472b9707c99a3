"""The host side of vt_sample_rows_wm, no GPU: tests/synthid_ref.py's restatement (uint64 hashes, fp64 tournament, the
cell's state machine) against the installed SynthIDTextWatermarkLogitsProcessor itself -- g-values and repeat decisions exactly,
probabilities and their prefix sums within 1e-6 (the processor's fp32 against fp64; measured 2.9e-7; logarithms are not compared:
the tournament is ill-conditioned there); vitron_amd.watermark's detector helpers against the processor's compute_* methods; the ABI
of struct vt_wm_row; the argument errors; and the detection score on synthetic rows."""
import os
import re

import numpy as np
import pytest
import torch

from tests import synthid_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, CALLS, TOP = 3, 16, 40
PROB_TOL = 1e-6


def _processor(cfg):
    from transformers.generation.logits_process import SynthIDTextWatermarkLogitsProcessor
    return SynthIDTextWatermarkLogitsProcessor(ngram_len=cfg.ngram_len, keys=list(cfg.keys), sampling_table_size=cfg.table_size,
                                               sampling_table_seed=cfg.table_seed, context_history_size=cfg.history_size, device="cpu",
                                               skip_first_ngram_calls=cfg.skip_first)


def _tokens(V, ngram_len):
    """[B, CALLS] tokens fed back as the 'chosen' ones: row 0 cycles with period 3 (from call ngram_len + 2 on its contexts come back
    behind two others: found again by a history of 1024, evicted from one of 2), row 1 is constant (an immediate repeat), row 2 never
    repeats."""
    period = 3
    return np.stack([np.asarray([(7 * (n % period) + 3) % V for n in range(CALLS)]), np.full((CALLS,), V - 1),
                     np.asarray([(11 * n + 5) % V for n in range(CALLS)])]).astype(np.int64)


def _scores(V, seed):
    """fp32 [CALLS, B, V] log-space scores with TOP finite entries per row, the rest -inf (what the warpers leave)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((CALLS, B, V), generator=g) * 2.0
    kth = x.topk(TOP, dim=-1).values[..., -1:]
    return torch.where(x >= kth, x, torch.full_like(x, float("-inf")))


@pytest.mark.parametrize("skip_first", (False, True))
@pytest.mark.parametrize("history_size", (2, 1024))
@pytest.mark.parametrize("depth", (1, 9, 30))
@pytest.mark.parametrize("ngram_len", (2, 3, 5))
@pytest.mark.parametrize("V", (257, 1000))
def test_restatement_equals_the_installed_processor(V, ngram_len, depth, history_size, skip_first):
    cfg = W.Config(ngram_len, W.KEYS30[:depth], history_size=history_size, skip_first=skip_first)
    proc = _processor(cfg)
    assert np.array_equal(proc.sampling_table.numpy(), cfg.table)
    cells = [W.Cell(cfg) for _ in range(B)]
    toks, scores = _tokens(V, ngram_len), _scores(V, 1000 * V + 10 * ngram_len + depth)
    prompt = torch.tensor([[1, 2, 3]] * B)
    past_hashes = [[] for _ in range(B)]
    worst = 0.0
    _seen = {"repeated": 0, "evicted": 0, "skipped": 0, "watermarked": 0}
    for n in range(CALLS):
        ids = torch.cat([prompt, torch.from_numpy(toks[:, :n])], dim=1)
        hist_before = None if proc.state is None else proc.state.context_history.clone()
        out = proc(ids, scores[n].clone())
        keys, ctx_hash = proc._compute_keys(proc.state.context, torch.arange(V)[None].expand(B, -1))
        g_hf = proc.sample_g_values(keys).numpy()
        skipped = skip_first and n + 1 < ngram_len
        rep_hf = np.zeros((B,), bool) if hist_before is None else (hist_before == ctx_hash[:, None]).any(dim=1).numpy()
        if hist_before is None and not skipped:       # the first call compares against the fresh, all-zero history
            rep_hf = (torch.zeros((B, history_size), dtype=torch.long) == ctx_hash[:, None]).any(dim=1).numpy()
        for b in range(B):
            p = torch.softmax(scores[n, b].double(), dim=-1).numpy()
            q, flags = cells[b].call(p)
            H = int(cells[b].w[2])
            assert H == int(ctx_hash[b].item()) & ((1 << 64) - 1)
            assert np.array_equal(cfg.g_next(H, V), g_hf[b]), (n, b)
            if skipped:
                assert flags == W.SKIPPED and torch.equal(out[b], scores[n, b])
                _seen["skipped"] += 1
            else:
                assert (flags == W.REPEATED) == bool(rep_hf[b]), (n, b, flags, rep_hf[b])
                if flags == W.REPEATED:
                    assert torch.equal(out[b], scores[n, b])
                    _seen["repeated"] += 1
                else:
                    got = torch.exp(out[b].double()).numpy()          # (finfo.min entries are exactly 0)
                    err = max(float(np.abs(got - q).max()), float(np.abs(np.cumsum(got) - np.cumsum(q)).max()))
                    worst = max(worst, err)
                    assert err <= PROB_TOL, (n, b, err)
                    _seen["watermarked"] += 1
                    if H in past_hashes[b]:
                        _seen["evicted"] += 1                         # seen before, no longer in the history
                past_hashes[b].append(H)
            cells[b].finish(int(toks[b, n]))
        # the cell's context is the processor's (it appends at the NEXT call; compare what it used at this one)
        for b in range(B):
            used = proc.state.context[b].numpy()
            want = np.concatenate([np.zeros(ngram_len - 1, np.int64), toks[b, :n]])[-(ngram_len - 1):]
            assert np.array_equal(used, want)
            assert np.array_equal(cells[b].w[4:4 + ngram_len - 1].astype(np.int64), np.concatenate([want, toks[b, n:n + 1]])[1:])
    print(f"V={V} ngram={ngram_len} depth={depth} history={history_size} skip={skip_first}: worst probability / prefix error {worst:.2e} "
          f"{_seen}")
    # the sequences repeat on purpose: repeated contexts in every case, contexts evicted from the history of two and found again
    # (none evicted from the history of 1024), skipped calls exactly where they are asked for
    assert _seen["repeated"] > 0 and _seen["watermarked"] > 0 and (_seen["evicted"] > 0) == (history_size == 2), _seen
    assert _seen["skipped"] == (B * (ngram_len - 1) if skip_first else 0), _seen


@pytest.mark.parametrize("ngram_len,depth,history_size", ((2, 1, 2), (5, 30, 1024), (3, 9, 4)))
def test_detector_helpers_equal_the_processors(ngram_len, depth, history_size):
    from vitron_amd.watermark import SynthIDWatermark
    cfg = W.Config(ngram_len, W.KEYS30[:depth], history_size=history_size)
    proc, wm = _processor(cfg), SynthIDWatermark(cfg.as_dict())
    g = torch.Generator().manual_seed(ngram_len)
    ids = torch.randint(0, 50, (4, 40), generator=g)
    ids[1, 10:] = ids[1, :30].clone()                         # repeated stretches
    ids[2] = 7
    ids[3, 17] = 2
    assert np.array_equal(wm.g_values(ids), proc.compute_g_values(ids).numpy())
    assert np.array_equal(wm.context_repetition_mask(ids), proc.compute_context_repetition_mask(ids).numpy())
    for eos in (2, 7, 49, 1000):
        assert np.array_equal(wm.eos_token_mask(ids, eos), proc.compute_eos_token_mask(ids, eos).numpy().astype(bool))
    assert np.array_equal(wm.table, cfg.table)
    # the restatement's next-token g-values are the n-gram g-values of the sequence it extends
    row = ids[0].numpy()
    t = 20
    H = cfg.context_hash(row[t - (ngram_len - 1):t])
    assert np.array_equal(cfg.g_next(H, 50)[row[t]], wm.g_values(row)[0, t - (ngram_len - 1)])
    assert np.array_equal(wm.g_next(H, 50), cfg.g_next(H, 50))
    # the kernel's decomposition: key = A_v + B_i with B_i = layer_add[i]
    with np.errstate(over="ignore"):
        A = ((np.uint64(H) + np.arange(50, dtype=np.uint64)) * W.M + W.ONE) * W.M
        assert np.array_equal(cfg.table[((A[:, None] + wm.layer_add[None]) & np.uint64(cfg.table_size - 1)).astype(np.int64)],
                              cfg.g_next(H, 50))
        assert np.array_equal(np.diff(A), np.full(49, W.M * W.M))
    bits = np.unpackbits(wm.table_bits.view(np.uint8), bitorder="little")
    assert np.array_equal(bits, cfg.table)


def test_wm_row_dtype_matches_the_header():
    from vitron_amd import _lib
    from vitron_amd import watermark as WM
    hdr = open(os.path.join(ROOT, "include", "vitron_hip.h")).read()
    m = re.search(r"^int\s+vt_sample_rows_wm\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m, "vt_sample_rows_wm is not declared in include/vitron_hip.h"
    args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    assert len(args) == 13 == len(_lib.SIGNATURES["vt_sample_rows_wm"][1])
    assert "const vt_wm_row* wm" in args[8] and "const vt_trunc_row* trunc" in args[7]
    assert re.search(r"^size_t\s+vt_wm_cell_words\s*\(int history_size\);", hdr, flags=re.M) and "vt_wm_cell_words" in _lib.SIGNATURES
    table = dict((name, int(off)) for off, name in re.findall(r"^ \*\s+@(\d+)\s+(?:const )?\w+\*? (\w+) ", hdr[:m.start()], flags=re.M)
                 if name in WM.WM_ROW_DTYPE.names)
    assert table == {n: WM.WM_ROW_DTYPE.fields[n][1] for n in WM.WM_ROW_DTYPE.names}, table
    struct = hdr[hdr.index("typedef struct vt_wm_row"):hdr.index("} vt_wm_row;")]
    assert re.findall(r"(\w+);", struct) == list(WM.WM_ROW_DTYPE.names) and WM.WM_ROW_BYTES == 48
    assert "vt_sample_rows_wm and struct vt_wm_row WITHOUT a bump" in hdr and "SynthIDTextWatermarkLogitsProcessor" in hdr
    assert re.search(r"#define VT_ABI_VERSION 114\b", hdr) and _lib.ABI_VERSION == 114
    for name, value in (("DEPTH", WM.WM_MAX_DEPTH), ("TABLE", WM.WM_MAX_TABLE), ("NGRAM", WM.WM_MAX_NGRAM), ("HISTORY", WM.WM_MAX_HISTORY)):
        assert re.search(rf"#define VT_WM_MAX_{name} {value}\b", hdr)
    wm = WM.SynthIDWatermark(dict(ngram_len=5, keys=[1, 2, 3], context_history_size=7, skip_first_ngram_calls=True))
    cell = wm.new_cell("cpu")
    assert cell.shape == (WM.WM_CELL_HEADER + 7,) and cell.dtype == torch.int64 and not cell.any()
    a = WM.wm_rows_array([None, wm.row_fields(cell)])
    add, tab = wm.device_tables("cpu")
    assert a[0].tobytes() == bytes(48)
    assert a[1].tobytes() == np.asarray([cell.data_ptr(), add.data_ptr(), tab.data_ptr()], "<u8").tobytes() \
        + np.asarray([3, 65536, 5, 7, 1, 0], "<i4").tobytes()
    assert WM.pack_wm_rows([None, (wm, cell), None], "cpu").shape == (3, 48)
    assert wm.device_tables("cpu")[0] is add                       # uploaded once per device
    assert [int(x) & ((1 << 64) - 1) for x in add.tolist()] == [(k * 6364136223846793005 + 1) % (1 << 64) for k in (1, 2, 3)]


def test_argument_errors():
    from vitron_amd.watermark import SynthIDWatermark
    ok = dict(ngram_len=5, keys=[1, 2, 3])
    SynthIDWatermark(ok)
    SynthIDWatermark(dict(ok, keys=[-(1 << 63), (1 << 63) - 1]))
    for bad in (dict(ok, keys=[]), dict(ok, keys=list(range(33))), dict(ok, keys=[1 << 63]), dict(ok, keys=[1.5]), dict(ok, ngram_len=1),
                dict(ok, ngram_len=9), dict(ok, context_history_size=0), dict(ok, context_history_size=4097), dict(keys=[1]),
                dict(ok, colour="green")):
        with pytest.raises(ValueError):
            SynthIDWatermark(bad)
    for bad, name in ((dict(ok, sampling_table_size=1000), "sampling_table_size"), (dict(ok, sampling_table_size=16), "sampling_table_size"),
                      (dict(ok, sampling_table_size=1 << 17), "sampling_table_size"), (dict(ok, debug_mode=True), "debug_mode")):
        with pytest.raises(NotImplementedError, match=name):
            SynthIDWatermark(bad)
    from transformers import SynthIDTextWatermarkingConfig, WatermarkingConfig
    with pytest.raises(NotImplementedError, match="randperm"):
        SynthIDWatermark(WatermarkingConfig())
    with pytest.raises(NotImplementedError, match="randperm"):
        SynthIDWatermark(dict(greenlist_ratio=0.25, bias=2.0))
    wm = SynthIDWatermark(SynthIDTextWatermarkingConfig(ngram_len=5, keys=list(W.KEYS30)))
    assert wm.depth == 30 and wm.sampling_table_size == 65536 and wm.context_history_size == 1024 and not wm.skip_first_ngram_calls
    wm.check_vocab(32768)
    with pytest.raises(NotImplementedError, match="32768"):
        wm.check_vocab(32769)


def test_the_library_refuses_without_a_gpu():
    """The argument checks in front of the launch come back without a device"""
    from vitron_amd import _lib
    for operand in ("bf16", "fp16"):
        lib = _lib.load(operand=operand)
        assert lib.vt_version() == 114 and hasattr(lib, "vt_sample_rows_wm")
        P = 0x10000                  # an aligned non-null address; never dereferenced because validation fails first
        for args, needle in (((None, 1, 64, 64, P, None, None, None, P, P, None, None, None), "null pointer"),
                             ((P, 1, 64, 64, P, None, None, None, P + 4, P, None, None, None), "wm must be 8-byte aligned"),
                             ((P, 1, 64, 64, P, None, None, P + 2, P, P, None, None, None), "trunc must be 4-byte aligned"),
                             ((P, 1, 33000, 33000, P, None, None, None, P, P, None, None, None), "register form"),     # by size
                             ((P, 1, 63, 63, P, None, None, None, P, P, None, None, None), "register form"),           # by stride
                             ((P + 4, 1, 64, 64, P, None, None, None, P, P, None, None, None), "register form"),       # by alignment
                             ((P, 0, 64, 64, P, None, None, None, P, P, None, None, None), "rows=0")):
            assert lib.vt_sample_rows_wm(*args) == -1                              # VT_STATUS_ARG
            assert needle in _lib.last_error(lib), (operand, needle, _lib.last_error(lib))
        assert lib.vt_wm_cell_words(1024) == 12 + 1024 and lib.vt_wm_cell_words(1) == 13


def test_detection_on_synthetic_rows():
    """64 seeded sequences of 24 steps, 8 equal survivors per step, depth 4, drawn through the restatement with and without the
    tournament from the same uniforms: mean_g of the watermarked ids exceeds 0.5 by 5 sigma, that of the plain ids stays within 4 sigma,
    sigma = 0.5 / sqrt(scored g-values)."""
    from vitron_amd.watermark import SynthIDWatermark
    V, steps, rows = 257, 24, 64
    cfg = W.Config(3, W.KEYS30[:4], history_size=64)
    wm = SynthIDWatermark(cfg.as_dict())
    g = np.random.default_rng(20241021)
    marked, plain = np.zeros((rows, steps), np.int64), np.zeros((rows, steps), np.int64)
    for r in range(rows):
        cell = W.Cell(cfg)
        for st in range(steps):
            p = np.zeros((V,))
            p[g.choice(V, 8, replace=False)] = 1.0
            u = float(g.uniform(0.0, 1.0))
            q, _ = cell.call(p)
            marked[r, st] = W.pick(q, u)[0]
            plain[r, st] = W.pick(p, u)[0]
            cell.finish(int(marked[r, st]))
    m_w, n_w = wm.mean_g(marked, return_count=True)
    m_p, n_p = wm.mean_g(plain, return_count=True)
    print(f"mean g: watermarked {m_w:.4f} over {n_w} g-values, plain {m_p:.4f} over {n_p}")
    assert n_w > 4000 and n_p > 4000
    assert m_w - 0.5 > 5 * 0.5 / np.sqrt(n_w), (m_w, n_w)
    assert abs(m_p - 0.5) < 4 * 0.5 / np.sqrt(n_p), (m_p, n_p)
    # generated_from and eos_token_id narrow the scored n-grams
    with_prompt = np.concatenate([np.full((rows, 5), 9), marked], axis=1)
    assert wm.mean_g(with_prompt, generated_from=5, return_count=True) == (m_w, n_w)
    eos = int(marked[0, 10])
    assert wm.mean_g(marked, eos_token_id=eos, return_count=True)[1] < n_w
    assert np.isnan(wm.mean_g(marked[:, :2]))
