"""vt_bias_rows on the GPU, both operand builds: every row's whole [V][2] adjustment bit for bit against tests/bias_ref.py
at the vocabulary sizes where the packed 16-bit counters and the dynamic LDS change (31: one ragged word; 32000 / 32003 / 40000: the
sampler's three forms; 65536: the limit, 136 KiB of LDS), over the history lengths around the block stride, a heavily repeated id, ids at
both ends of the vocabulary and outside it, no / one / 300 biased ids, both signs of the penalties -- every row of one launch with its own
parameters, all buffers in one image with a guard word behind every adjustment."""
import numpy as np
import pytest
import torch

from tests import bias_ref as R

pytestmark = pytest.mark.gpu
VS = (31, 32000, 32003, 40000, 65536)
GUARD = 0x5A5A5A5A
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    from vitron_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _case(h=(), ids=(), vals=(), presence=0.0, frequency=0.0, hist_len=None, n_bias=None, hist_null=False, ids_null=False, vals_null=False,
          out_null=False):
    return dict(h=[int(t) for t in h], ids=[int(t) for t in ids], vals=[float(F32(v)) for v in vals], presence=float(F32(presence)),
                frequency=float(F32(frequency)), hist_len=len(h) if hist_len is None else int(hist_len),
                n_bias=len(ids) if n_bias is None else int(n_bias), hist_null=hist_null, ids_null=ids_null, vals_null=vals_null,
                out_null=out_null)


def _expected(V, c):
    h = [] if (c["hist_null"] or c["hist_len"] <= 0) else c["h"][:c["hist_len"]]
    nb = 0 if (c["ids_null"] or c["vals_null"] or c["n_bias"] <= 0) else c["n_bias"]
    pre, post = R.bias_rows(V, h, c["ids"][:nb], c["vals"][:nb], c["presence"], c["frequency"])
    return np.stack([pre, post], 1).reshape(-1)                                  # [V][2]


_built = {}


def _cases(V):
    """The rows of one launch at vocabulary V and their reference adjustments, built once and shared by both builds"""
    if V in _built:
        return _built[V]
    rng = np.random.default_rng(8100 + V)
    small = lambda k: rng.choice(V, size=min(k, V), replace=False)               # noqa: E731
    inside = np.unique(np.concatenate([[0, V - 1], rng.choice(V, size=min(V, 280), replace=False)]))[:290]
    outside = [-1, V, V + 5, -2 ** 31, 2 ** 31 - 1]
    ids300 = rng.permutation(np.concatenate([inside, outside, V + 10 + np.arange(300 - len(inside) - len(outside))]))
    assert len(ids300) == 300
    vals300 = rng.standard_normal(300) * 6
    rows = [
        _case(h=[3, 3, 4], presence=0.5, frequency=0.25, hist_null=True),                                 # history NULL with a length set
        _case(h=[], ids=[0], vals=[2.5], presence=1.0, frequency=1.0),                                    # length 0, one biased id
        _case(h=[V - 1], ids=ids300, vals=vals300, presence=0.75, frequency=0.1),                         # length 1, 300 biased ids
        _case(h=rng.choice(small(3), size=1023), presence=-0.5, frequency=-0.3),                          # the block stride - 1, negative
        _case(h=rng.choice(small(2), size=1024), ids=[V - 1], vals=[-7.0], presence=0.3, frequency=0.7),  # the block stride
        _case(h=rng.choice(small(4), size=1025), ids=ids300, vals=vals300, presence=-1.25, frequency=0.01),
        _case(h=[V // 2] * 4096, presence=0.1, frequency=0.3),                                            # contention and a large count
        _case(h=[V - 1] * 4097, presence=-4097.0, frequency=1.0 + 2.0 ** -12),                            # a fused multiply-add differs here
        _case(h=[0, V - 1, 0, V - 1, V - 1, -1, V, V + 7, -200, 2 ** 31 - 1, -2 ** 31, 1 % V], ids=[-1, V], vals=[9.0, 9.0],
              presence=1.5, frequency=0.5),                                                               # both ends; ids outside the vocabulary
        _case(h=rng.choice(small(5), size=300), ids=[0], vals=[1.0], presence=2.0, frequency=2.0, out_null=True),     # skipped entirely
        _case(h=[5 % V, 5 % V], presence=1.0, frequency=1.0, hist_len=-4),
        _case(h=[5 % V, 6 % V, 5 % V, 5 % V], presence=1.0, frequency=1.0, hist_len=2),                   # only the first two count
        _case(h=[1 % V], ids=[0, 1 % V], vals=[3.0, 4.0], presence=0.5, n_bias=-2),
        _case(h=[1 % V], ids=[0, 2 % V], vals=[3.0, 4.0], frequency=0.5, ids_null=True),
        _case(h=[1 % V], ids=[0, 2 % V], vals=[3.0, 4.0], frequency=0.5, vals_null=True),
        _case(h=[1 % V], ids=[0, 2 % V, 3 % V], vals=[3.0, 4.0, 5.0], frequency=0.5, n_bias=1),           # only the first pair counts
        _case(h=rng.integers(0, V, size=3000), ids=inside[:17], vals=vals300[:17], presence=0.2, frequency=0.4),
        _case(),                                                                                          # nothing at all: zeros
    ]
    want = [None if c["out_null"] else _expected(V, c) for c in rows]
    two_step = F32(F32(F32(1.0 + 2.0 ** -12) * F32(4097)) + F32(-4097.0))
    assert want[7][2 * (V - 1) + 1] == -two_step and two_step != F32((1.0 + 2.0 ** -12) * 4097 - 4097.0)
    assert want[6][2 * (V // 2) + 1] == -F32(F32(F32(0.3) * F32(4096)) + F32(0.1))
    _built[V] = (rows, want)
    return _built[V]


def _layout(V, rows, want):
    """All buffers of the launch in ONE int32 image: per row history, bias ids, bias values and out (2 V words + a guard), separated by
    guard words; every other out on an 8-byte boundary (the 8-byte stores), the rest off it. Returns (image before, image expected
    after, struct fields with word offsets for pointers)."""
    from vitron_amd.sampling import BIAS_ROW_DTYPE
    chunks, pos = [], 0
    fields = np.zeros((len(rows),), dtype=BIAS_ROW_DTYPE)

    def put(words_, odd):
        nonlocal pos
        pos += 1                                                                 # at least one guard word between any two buffers
        pos += (-pos) % 2
        if odd:
            pos += 1                                                             # 4-byte aligned only
        off = pos
        chunks.append((off, np.asarray(words_, dtype=np.int64)))
        pos += len(words_)
        return off

    outs = []
    for i, c in enumerate(rows):
        ho = put(c["h"] or [GUARD], i % 3 == 0)
        io = put(c["ids"] or [GUARD], i % 3 == 1)
        vo = put(np.asarray(c["vals"] or [0.0], dtype=F32).view(np.int32).astype(np.int64), i % 3 == 2)
        oo = put([GUARD] * (2 * V), i % 2 == 1)
        outs.append(oo)
        fields[i] = (0 if c["hist_null"] else ho, 0 if c["ids_null"] else io, 0 if c["vals_null"] else vo, 0 if c["out_null"] else oo,
                     c["hist_len"], c["n_bias"], c["presence"], c["frequency"])
    img = np.full((pos + 8,), GUARD, dtype=np.int64)
    for off, w in chunks:
        img[off:off + len(w)] = w
    before = (img & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    after = before.copy()
    for oo, m in zip(outs, want):
        if m is not None:
            after[oo:oo + 2 * V] = m.view(np.int32)
    return before, after, fields


def _launch(lib, dev, V, before, fields, times=1):
    buf = torch.from_numpy(before.copy()).to(dev)
    f = fields.copy()
    for name in ("history", "bias_ids", "bias_vals", "out"):                     # word offsets -> device addresses (0 stays NULL)
        f[name] = np.where(fields[name] != 0, buf.data_ptr() + 4 * fields[name].astype(np.uint64), 0).astype(np.uint64)
    rows_dev = torch.from_numpy(f.view(np.uint8).reshape(len(f), 48).copy()).to(dev)
    got = []
    for _ in range(times):
        st = lib.vt_bias_rows(rows_dev.data_ptr(), len(f), V, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got.append((st, buf.cpu().numpy()))
    return got


@pytest.mark.parametrize("operand", ("bf16", "fp16"))
@pytest.mark.parametrize("V", VS)
def test_bias_rows_equals_the_reference_bit_for_bit(dev, V, operand):
    """Every row's whole adjustment equals bias_ref; everything else in the image -- histories, bias ids and values, the guard word
    behind every adjustment, the words between the buffers, the buffer of the skipped row -- is what it was; a second launch over the
    first one's result gives the same bytes."""
    from vitron_amd import _lib
    rows, want = _cases(V)
    before, after, fields = _layout(V, rows, want)
    (st, got), (st2, again) = _launch(_lib.load(operand=operand), dev, V, before, fields, times=2)
    assert st == 0 and st2 == 0, _lib.last_error()
    if not np.array_equal(got, after):
        for i, (c, m) in enumerate(zip(rows, want)):
            if m is None:
                continue
            oo = int(fields["out"][i])
            bad = np.flatnonzero(got[oo:oo + 2 * V] != m.view(np.int32))
            assert bad.size == 0, (V, i, {k: c[k] for k in ("hist_len", "n_bias", "presence", "frequency")}, bad[:6].tolist(),
                                   got[oo:oo + 2 * V].view(F32)[bad[:6]].tolist(), m[bad[:6]].tolist())
        assert False, ("a word outside the adjustments changed", np.flatnonzero(got != after)[:8].tolist())
    assert np.array_equal(again, got)


def test_through_ops_matches_the_products_own_statement(dev):
    """ops.bias_rows + sampling.pack_bias_rows against sampling.logit_adjust: three rows, the middle one with out NULL."""
    from vitron_amd import ops
    from vitron_amd.sampling import logit_adjust, pack_bias_rows
    V = 1000
    t = lambda a, dt=torch.int32: torch.tensor(a, dtype=dt, device=dev)           # noqa: E731
    h0, h2 = [7, 8, 7, 7, -200, 999], [0] * 70 + [5]
    bias = {3: 1.5, 999: -2.0, 0: 0.25}
    ids, vals = t(list(bias)), t(list(bias.values()), torch.float32)
    hist = [t(h0), t([1, 2]), t(h2)]
    outs = [torch.full((2 * V + 2,), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    packed = pack_bias_rows([(hist[0].data_ptr(), len(h0), ids.data_ptr(), vals.data_ptr(), 3, outs[0].data_ptr(), 0.5, 0.25),
                             (hist[1].data_ptr(), 2, ids.data_ptr(), vals.data_ptr(), 3, 0, 0.5, 0.25),
                             (hist[2].data_ptr(), len(h2), 0, 0, 0, outs[2].data_ptr(), -1.0, 0.1)], dev)
    assert packed.shape == (3, 48) and packed.dtype == torch.uint8
    ops.bias_rows(packed, 3, V)
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    for g, (h, b, p, f) in ((got[0], (h0, bias, 0.5, 0.25)), (got[2], (h2, None, -1.0, 0.1))):
        pre, post = logit_adjust(V, h, b, p, f)
        assert np.array_equal(g[:2 * V].reshape(V, 2)[:, 0].view(np.uint32), pre.view(np.uint32))
        assert np.array_equal(g[:2 * V].reshape(V, 2)[:, 1].view(np.uint32), post.view(np.uint32))
        assert np.isnan(g[2 * V:]).all()
    assert np.isnan(got[1]).all()
    assert got[0][2 * 7 + 1] == -F32(F32(F32(0.25) * F32(3)) + F32(0.5)) and got[0][2 * 3] == 1.5


def test_refusals_and_no_rows(dev):
    from vitron_amd import _lib, ops
    from vitron_amd.sampling import pack_bias_rows
    lib = _lib.load()
    out = torch.full((2 * 64 + 2,), float("nan"), dtype=torch.float32, device=dev)
    packed = pack_bias_rows([(0, 0, 0, 0, 0, out.data_ptr(), 1.0, 1.0)], dev)
    stream = torch.cuda.current_stream().cuda_stream
    for n_rows, V, ptr, needle in ((1, 0, packed.data_ptr(), "V=0"), (1, -5, packed.data_ptr(), "V=-5"), (1, 65537, packed.data_ptr(), "V=65537"),
                                   (-1, 64, packed.data_ptr(), "n_rows=-1"), (1, 64, None, "NULL")):
        assert lib.vt_bias_rows(ptr, n_rows, V, stream) == -1                     # VT_STATUS_ARG, with a message
        assert needle in _lib.last_error(lib), (needle, _lib.last_error(lib))
    assert lib.vt_bias_rows(None, 0, 64, stream) == 0 and lib.vt_bias_rows(packed.data_ptr(), 0, 64, stream) == 0
    ops.bias_rows(packed, 0, 64)                                                  # n_rows == 0: a success that launches nothing
    with pytest.raises(_lib.VitronHipError, match="V=65537"):
        ops.bias_rows(packed, 1, 65537)
    with pytest.raises(_lib.VitronHipError):
        ops.bias_rows(packed, 2, 64)                                              # 48 bytes are one row, not two
    with pytest.raises(_lib.VitronHipError):
        ops.bias_rows(packed.cpu(), 1, 64)
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()                                      # nothing was launched
    ops.bias_rows(packed, 1, 64)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:128] == 0).all() and np.isnan(got[128:]).all()
