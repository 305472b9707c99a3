"""vt_llama_model.logit_row_trace / logit_row_trace_layers through engine.llama_forward(trace_rows_layers=) on 8-layer models (DESIGN.md
9.14): entry [l][i] of the trace is, bit for bit, the operand-format rounding of row logit_rows[i] of layer l's entry in
return_all_hidden's fp32 trace -- for a prefill of more than 32 rows with the pruned last layer and with last_layer_full = 1, for
several logit rows per sequence, for decode steps of 1, 4 and 16 rows (with and without the folded norms), on the fp8 pool and on NF4
weights; layers that are not flagged keep the caller's sentinel; logits and KV pages are bitwise those of the same call without the
trace."""
import pytest
import torch

from vitron_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = {"h256": (256, 512, 2), "h1024": (1024, 1408, 8)}       # h1024: a decode step folds its norms into the GEMMs
L = 8
SENTINEL = 1234.0


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_models = {}


def _model(dev, shape, wfmt):
    from vitron_amd.engine import PackedLlama
    if (shape, wfmt) not in _models:
        H, I, heads = SHAPES[shape]
        cfg = dict(synth.VICUNA_7B, hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=heads, vocab_size=640)
        sd = synth.llama_state(cfg, synth.make_generator(41), w_std=0.05)
        _models[(shape, wfmt)] = PackedLlama(sd, cfg, dev, **({"weight_format": "nf4"} if wfmt == "nf4" else {}))
    return _models[(shape, wfmt)]


def _arm(dev, llama, kvd, passes, rows, **kw):
    """All passes on a fresh pool; the keyword arguments go to the LAST pass. Returns (what it returned, K pool, V^T pool)."""
    from vitron_amd.engine import PagedKVCache, SequenceState, llama_forward
    kv = PagedKVCache(llama, 24, kv_dtype=kvd)
    seqs = [SequenceState() for _ in passes[0]]
    g = torch.Generator().manual_seed(42)
    out = None
    for pi, q_lens in enumerate(passes):
        x = (torch.randn((sum(q_lens), llama.H), generator=g) * 0.5).to(dev).to(llama.dtype)
        last = pi == len(passes) - 1
        out = llama_forward(llama, kv, seqs, x, q_lens, logit_rows=rows if last else None, **(kw if last else {}))
    torch.cuda.synchronize()
    return out, kv.k.clone(), kv.vt.clone()


def _check(dev, llama, kvd, passes, rows, layers, full=False):
    """The three arms of one pass shape: plain, with the row trace (into a sentinel-filled buffer), with return_all_hidden."""
    q = passes[-1]
    logit_rows = rows if rows is not None else [sum(q[:i + 1]) - 1 for i in range(len(q))]
    llama.set_last_layer_full(full)
    try:
        plain, k0, v0 = _arm(dev, llama, kvd, passes, rows)
        buf = torch.full((L, len(logit_rows), llama.H), SENTINEL, dtype=llama.dtype, device=dev)
        (traced, got), k1, v1 = _arm(dev, llama, kvd, passes, rows, trace_rows_layers=layers, trace_rows_out=buf)
        (_, _, full_trace), _, _ = _arm(dev, llama, kvd, passes, rows, return_all_hidden=True)
    finally:
        llama.set_last_layer_full(False)
    assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (L, len(logit_rows), llama.H) and got.dtype == llama.dtype
    assert torch.equal(traced, plain) and torch.equal(k1, k0) and torch.equal(v1, v0)      # no logit and no page bit moves
    want = full_trace[:, torch.tensor(logit_rows, device=dev)].to(llama.dtype)             # fp32 -> operand format, round to nearest even
    for l in range(L):
        if l in layers:
            assert torch.equal(got[l].view(torch.int16), want[l].view(torch.int16)), (l, kvd, passes, rows)
        else:
            assert bool((got[l] == SENTINEL).all()), (l, kvd, passes, rows)
    assert len({tuple(want[l].view(torch.int16).flatten().tolist()[:64]) for l in layers}) == len(layers)      # the layers do differ
    # a fresh buffer of the call's own when none is given
    (_, own), _, _ = _arm(dev, llama, kvd, passes, rows, trace_rows_layers=layers)
    assert own.data_ptr() != buf.data_ptr() and all(torch.equal(own[l].view(torch.int16), got[l].view(torch.int16)) for l in layers)


@pytest.mark.parametrize("full", (False, True), ids=("pruned", "last_layer_full"))
@pytest.mark.parametrize("kvd", ("16bit", "fp8"))
def test_prefill(dev, kvd, full):
    """More than 32 rows, the last layer pruned (the default) or run on all rows: one sequence read at its last row; two ragged
    sequences read at three rows, two of them in one sequence; a chunk behind a past."""
    llama = _model(dev, "h256", "16bit")
    _check(dev, llama, kvd, [[40]], None, [0, 3, 6, 7], full)
    _check(dev, llama, kvd, [[37, 45]], [3, 36, 81], list(range(L)), full)
    _check(dev, llama, kvd, [[70], [35]], None, [7], full)


@pytest.mark.parametrize("shape", ("h256", "h1024"))
@pytest.mark.parametrize("n", (1, 4, 16))
def test_decode_step(dev, shape, n):
    """A decode step of 1, 4 and 16 rows behind short prompts, on both pools."""
    llama = _model(dev, shape, "16bit")
    for kvd in ("16bit", "fp8"):
        _check(dev, llama, kvd, [[5 + (i % 3) for i in range(n)], [1] * n], None, [0, 2, 4, 6] if n != 4 else [1, 7])


@pytest.mark.parametrize("shape", ("h256", "h1024"))
def test_nf4_weights(dev, shape):
    llama = _model(dev, shape, "nf4")
    _check(dev, llama, "16bit", [[40]], None, [0, 4, 6])
    _check(dev, llama, "16bit", [[6, 9], [1, 1]], None, [2, 7])


def test_argument_errors(dev):
    from vitron_amd import _lib
    from vitron_amd.engine import PagedKVCache, SequenceState, llama_forward
    llama = _model(dev, "h256", "16bit")
    kv, s = PagedKVCache(llama, 4), SequenceState()
    x = torch.zeros((3, llama.H), dtype=llama.dtype, device=dev)
    for kw in (dict(trace_rows_layers=[8]), dict(trace_rows_layers=[-1]), dict(trace_rows_layers=[]),
               dict(trace_rows_out=torch.empty((L, 1, llama.H), dtype=llama.dtype, device=dev)),
               dict(trace_rows_layers=[1], trace_rows_out=torch.empty((L, 2, llama.H), dtype=llama.dtype, device=dev)),
               dict(trace_rows_layers=[1], trace_rows_out=torch.empty((L, 1, llama.H), dtype=torch.float32, device=dev)),
               dict(trace_rows_layers=[1], logit_rows=[])):
        with pytest.raises(_lib.VitronHipError, match="trace_rows"):
            llama_forward(llama, kv, [s], x, [3], **kw)
    assert not s.pages and s.length == 0 and len(kv.free) == kv.num_pages                   # refused before a page was taken
