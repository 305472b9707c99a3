"""The host restatement of the decode attention kernels (tests/attn_ref.py) on its own: the page layout round-trips, V saturates into the
fp16 pages, the fp32 fused multiply-add emulation of the rotary embedding is exact, an fp32 attention stays inside decode_bound, and the
bound is tight enough that one wrong key breaks it; the same for the prefill kernels' restatement (prefill_ref / prefill_bound) against a
plain fp32 emulation of their scheme. No GPU needed."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import attn_ref as R

DTYPES = [torch.bfloat16, torch.float16]


def _frac_to_f32(x: Fraction) -> float:
    """round-to-nearest-even of an exact rational to fp32 (normal range)"""
    if x == 0:
        return 0.0
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    m = x / Fraction(2) ** (e - 23)              # in [2^23, 2^24)
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * float(Fraction(n) * Fraction(2) ** (e - 23))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_pack_unpack_round_trip_and_layout(dtype, hd):
    heads, npages = 3, 11
    g = torch.Generator().manual_seed(hd)
    for L in (1, 63, 64, 65, 200):
        nt = (L + 63) // 64
        table = torch.randperm(npages, generator=g)[:nt]
        k = torch.randn((L, heads, hd), generator=g).to(dtype)
        v = torch.randn((L, heads, hd), generator=g).to(dtype)
        kp, vp = R.pack_pages(k, v, table, heads, hd, dtype, npages=npages, fill=float("nan"))
        k2, v2 = R.unpack_pages(kp, vp, table, L, heads, hd)
        assert torch.equal(k2, k) and torch.equal(v2, R.to_f16_page(v))
        big = v.float().abs() >= 2.0 ** -14                 # exact in fp16's normal range
        assert torch.equal(v2.float()[big], v.float()[big])
        # the documented addressing: tile i of head h at (table[i] * heads + h) * 64 * hd; K [64][hd], V^T [hd][64]
        j, h, d = L - 1, heads - 1, hd - 1
        base = (int(table[j // 64]) * heads + h) * 64 * hd
        assert kp[base + (j % 64) * hd + d] == k[j, h, d] and vp[base + d * 64 + j % 64].float() == v[j, h, d].float()
        used = torch.zeros(npages, dtype=torch.bool)
        used[table] = True
        assert torch.isnan(kp.view(npages, -1)[~used].float()).all() and torch.isnan(vp.view(npages, -1)[~used].float()).all()
        last = int(table[-1])
        kl = kp.view(npages, heads, 64, hd)[last]
        vl = vp.view(npages, heads, hd, 64)[last]
        r = L - (nt - 1) * 64
        assert (kl[:, r:] == 0).all() and (vl[:, :, r:] == 0).all()


def test_v_pages_saturate_at_fp16_max():
    v = torch.tensor([1e5, -3e5, 65504.0, 70000.0, -65520.0, 1.0, 2.0 ** -20], dtype=torch.bfloat16)
    got = R.to_f16_page(v).float().tolist()
    want = [65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 1.0, 2.0 ** -20]
    assert got == [float(np.float16(x)) for x in want] and got[:2] == [65504.0, -65504.0]
    k = torch.zeros((3, 1, 64), dtype=torch.bfloat16)
    vv = torch.zeros((3, 1, 64), dtype=torch.bfloat16)
    vv[:, 0, 0] = torch.tensor([1e5, -1e5, 3.0])
    _, vp = R.pack_pages(k, vv, [0], 1, 64, torch.bfloat16)
    assert vp[:3].float().tolist() == [65504.0, -65504.0, 3.0] and torch.isfinite(vp.float()).all()


def test_fma_emulation_is_exact():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(np.float32) * np.exp2(rng.integers(-30, 30, 4000)).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * np.exp2(rng.integers(-40, 20, 4000))).astype(np.float32)
    # and a sum that lies just below an fp32 midpoint whose fp64 rounding lands on it: naive a * b + c in fp64, then fp32, rounds to even
    a = np.append(a, np.float32(2.0 ** -24 * (1 + 2.0 ** -23)))
    b = np.append(b, np.float32(1 - 2.0 ** -23))
    c = np.append(c, np.float32(1 + 2.0 ** -23))
    got = R.fma32(a, b, c)
    want = np.array([_frac_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got, want)
    assert got[-1] == np.float32(1 + 2.0 ** -23) and (a[-1:].astype(np.float64) * b[-1] + c[-1]).astype(np.float32)[0] != got[-1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_ref_matches_exact_arithmetic(dtype):
    from oracle import vitron_oracle as O
    hd = 128
    cos, sin = O.rope_tables(hd, 8192)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((40, 2, hd), generator=g) * 3).to(dtype)
    pos = torch.randint(0, 8192, (40,), generator=g).numpy()
    got = R.rope_ref(x, cos, sin, pos, dtype).float().numpy()
    xf, cf, sf = x.float().numpy(), cos.numpy(), sin.numpy()
    h = hd // 2
    for i in range(0, 40, 3):
        for hh in range(2):
            for d in range(0, h, 5):
                a, b = Fraction(float(xf[i, hh, d])), Fraction(float(xf[i, hh, d + h]))
                c, s = Fraction(float(cf[pos[i], d])), Fraction(float(sf[pos[i], d]))
                lo = _frac_to_f32(a * c - Fraction(float(np.float32(xf[i, hh, d + h]) * np.float32(sf[pos[i], d]))))
                hi = _frac_to_f32(b * c + Fraction(float(np.float32(xf[i, hh, d]) * np.float32(sf[pos[i], d]))))
                want = R.to_op(torch.tensor([lo, hi], dtype=torch.float64), dtype).float().tolist()
                assert [got[i, hh, d], got[i, hh, d + h]] == want, (i, hh, d)
    # against the oracle's fp32 rotary: the same values to within one operand rounding
    ref = O._rope(x.float().permute(1, 0, 2), cos[pos], sin[pos]).permute(1, 0, 2)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    assert torch.allclose(torch.from_numpy(got), ref, rtol=tol, atol=1e-6)


def _attn_f32(q, k, v, scale, dtype):
    """plain fp32 single-query attention (exp2 of scores scaled by an fp32 scale * log2 e), rounded to the operand"""
    q, k, v = (torch.as_tensor(x).float() for x in (q, k, v))
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(R.LOG2E, dtype=torch.float32)
    t = torch.einsum("hd,lhd->hl", q, k) * sl2
    p = torch.exp2(t - t.max(dim=-1, keepdim=True).values)
    o = torch.einsum("hl,lhd->hd", p, v) / p.sum(dim=-1, keepdim=True)
    return R.to_op(o, dtype).double()


def _problem(L, hd, dtype, seed, heads=4):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((heads, hd), generator=g).to(dtype)
    k = torch.randn((L, heads, hd), generator=g).to(dtype)
    v = R.to_f16_page((torch.randn((L, heads, hd), generator=g) + 2).to(dtype))     # a mean: |v_j - o| and |o| both O(1)
    return q, k, v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_fp32_attention_stays_inside_the_bound(dtype, hd):
    store, worst = R.FMT[dtype], 0.0
    for L in (1, 2, 65, 100, 577):
        q, k, v = _problem(L, hd, dtype, L + hd)
        scale = 1.0 / math.sqrt(hd)
        err = (_attn_f32(q, k, v, scale, dtype) - R.decode_ref(q, k, v, scale)).abs()
        bound = R.decode_bound(q, k, v, scale, store)
        assert (err <= bound).all(), (L, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    assert worst > 0.25          # and the bound is not vacuous: the store's rounding alone takes up to half of it


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_the_bound_breaks_under_one_wrong_key(dtype, hd):
    store, L, scale = R.FMT[dtype], 100, 1.0 / math.sqrt(hd)
    q, k, v = _problem(L, hd, dtype, 11 * hd)
    k[5] = (q.float() * 0.35).to(dtype)                  # key 5 carries a large weight (its tile-1 twin, key 69, does not)
    ref = R.decode_ref(q, k, v, scale)
    bound = R.decode_bound(q, k, v, scale, store)
    assert (_attn_f32(q, k, v, scale, dtype) - ref).abs().le(bound).all()

    def broken(q2, k2, v2):
        got = _attn_f32(q2, k2, v2, scale, dtype)
        return float(((got - ref).abs() > bound).double().mean())     # share of the elements out of bounds

    # dropping the last key
    assert broken(q, k[:-1], v[:-1]) > 0.1
    # admitting one padding key (zero K row, zero V column)
    z = torch.zeros((1,) + k.shape[1:], dtype=k.dtype)
    assert broken(q, torch.cat([k, z]), torch.cat([v, z.to(v.dtype)])) > 0.1
    # key 5 read from the wrong tile (key 69's row and column)
    k2, v2 = k.clone(), v.clone()
    k2[5], v2[5] = k[69], v[69]
    assert broken(q, k2, v2) > 0.1


# ---- prefill: an fp32 emulation of the kernels' scheme against prefill_bound ----------------------------------------------------------
def _prefill_f32(q, k, v, scale, past, dtype, causal=True, lim_shift=0, l_bug_tile=None):
    """flash_attn_kernel's scheme in plain fp32 torch: 64-key tiles in order, the deferred rescale decided per group of 32 rows (a wave),
    weights exp2(s * sl2 + (7 - m_run)), fp16 weights into P.V, the row sum from the unrounded ones, o * (1 / l), one rounding to the
    operand. q [Lq][heads][hd], k / v [past + Lq][heads][hd]. Wrong on purpose: lim_shift moves the causal limit (-1 drops the diagonal
    key, +1 admits the key behind it); l_bug_tile: on that tile l adds the fp16 weights of one half-wave's keys (16 of every 32) only."""
    q, k, v = (torch.as_tensor(x).float().permute(1, 0, 2) for x in (q, k, v))        # [heads][L][hd]
    heads, Lq, hd = q.shape
    Lk = k.shape[1]
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(R.LOG2E, dtype=torch.float32)
    m = torch.full((heads, Lq), -math.inf)
    l = torch.zeros((heads, Lq))
    o = torch.zeros((heads, Lq, hd))
    lim = (past + torch.arange(Lq) + lim_shift) if causal else torch.full((Lq,), Lk - 1)
    grp = torch.arange(Lq) // 32
    for ti, t0 in enumerate(range(0, Lk, 64)):
        keys = t0 + torch.arange(min(64, Lk - t0))
        s = (q @ k[:, t0:t0 + 64].transpose(1, 2)).masked_fill((keys[None, :] > lim[:, None])[None], -math.inf)
        mt = s.amax(dim=-1) * sl2
        over = torch.nn.functional.pad(mt > m + R.RESCALE_THR, (0, -Lq % 32))
        trig = over.view(heads, -1, 32).any(dim=-1)[:, grp]
        mn = torch.where(trig, torch.maximum(m, mt), m)
        a = torch.where(mn == -math.inf, torch.ones(()), torch.exp2(m - mn))
        a = torch.where(trig, a, torch.ones(()))
        m, l, o = mn, l * a, o * a[..., None]
        ms = torch.where(m == -math.inf, torch.zeros(()), m)
        e = torch.exp2(s * sl2 + (R.P_BIAS - ms)[..., None])
        p16 = e.half().float()
        if l_bug_tile == ti:
            l = l + (p16 * ((keys % 32) < 16)[None, None, :]).sum(-1)
        else:
            l = l + e.sum(-1)
        o = o + p16 @ v[:, t0:t0 + 64]
    out = o * torch.where(l > 0, 1.0 / l, torch.zeros(()))[..., None]
    return R.to_op(out, dtype).double().permute(1, 0, 2)


def _prefill_problem(Lq, past, hd, dtype, seed, amp=1.0, heads=2):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((Lq, heads, hd), generator=g) * amp).to(dtype)
    k = (torch.randn((past + Lq, heads, hd), generator=g) * amp).to(dtype)
    v = R.to_f16_page((torch.randn((past + Lq, heads, hd), generator=g) + 2).to(dtype))
    return q, k, v


def test_half_ulp_in_torch_equals_the_numpy_one():
    from tests.nf4_ref import half_ulp
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-40, 17, (4000,), generator=g).double())
    x = torch.cat([x, torch.tensor([0.0, 1.0, 2.0 ** -14, 2.0 ** -15, 65504.0, 3.0])])
    for fmt in ("bf16", "fp16"):
        assert np.array_equal(R.half_ulp_t(x, fmt).numpy(), half_ulp(x.numpy(), fmt))


def test_prefill_ref_is_plain_attention_and_takes_row_subsets():
    q, k, v = _prefill_problem(70, 30, 64, torch.float16, 5)
    scale = 0.125
    ref = R.prefill_ref(q, k, v, scale, 30, True)
    for i in (0, 1, 33, 69):                             # row i = single-query attention over keys 0 .. past + i
        assert torch.allclose(ref[i], R.decode_ref(q[i], k[:31 + i], v[:31 + i], scale), rtol=1e-13, atol=1e-15)
    full = R.prefill_ref(q, k, v, scale, 30, False)
    assert torch.allclose(full[7], R.decode_ref(q[7], k, v, scale), rtol=1e-13, atol=1e-15)
    rows = [3, 64, 69]
    r2, b2 = R.prefill_ref_and_bound(q[rows], k, v, scale, 30, True, "fp16", rows=rows)
    assert torch.equal(r2, ref[rows]) and torch.equal(b2, R.prefill_bound(q, k, v, scale, 30, True, "fp16")[rows])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_emulation_stays_inside_the_bound_which_is_not_vacuous(dtype, hd):
    """Mild scores, wide scores (q, k scaled by 3: the rows' score spans exceed 60 in log2 units, the deferred rescale and the fp16
    weights' subnormal tail act) and a chunk behind a past, causal and not. Non-vacuity: the emulation reaches more than a quarter of
    the bound somewhere, and on the mild cases the median of bound / (half an ulp of the store) is at most 4 -- a condition on the
    derivation (the fp16-weight term 2^-11 sum p |v| is one to two half-ulps of an fp16 store by itself when |v| is about |o|), not a
    measurement of any kernel."""
    store, scale, worst, med = R.FMT[dtype], 1.0 / math.sqrt(hd), 0.0, {}
    for name, Lq, past, amp, causal in (("mild", 300, 0, 1.0, True), ("past", 130, 1000, 1.0, True), ("full", 257, 0, 1.0, False),
                                        ("wide", 300, 0, 3.0, True)):
        q, k, v = _prefill_problem(Lq, past, hd, dtype, hd + Lq, amp)
        ref, bound = R.prefill_ref_and_bound(q, k, v, scale, past, causal, store)
        if name == "wide":
            t = torch.einsum("qhd,khd->hqk", q.double(), k.double()) * scale * R.LOG2E
            assert float(t.amax(-1).amax() - t.amin(-1).amin()) > 60.0 and float((t.amax(-1) - t.amin(-1)).max()) > 60.0
        err = (_prefill_f32(q, k, v, scale, past, dtype, causal) - ref).abs()
        ratio = float((err / bound).max())
        assert (err <= bound).all(), (name, ratio)
        worst = max(worst, ratio)
        if name != "wide":
            med[name] = float((bound / R.half_ulp_t(ref, store)).median())
    assert worst > 0.25, worst
    assert max(med.values()) <= 4.0, f"median bound / half-ulp of the {store} store: {med}"
    print(f"\n[prefill bound, host] {store} hd {hd}: emulation error / bound up to {worst:.2f}, median bound / half-ulp {med}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_the_prefill_bound_breaks_under_one_wrong_key(dtype, hd):
    """96 rows without a past (a row has at most 96 visible keys: one key's weight is >= 1 / 96 of the row on average, several
    half-ulps of either store at |v_j - o| about 1): the share of elements outside the bound when the diagonal key is dropped, when the
    key behind the diagonal is admitted, when a heavy key is read from the neighbouring tile, and when l is the fp16 weights' sum
    without one half-wave's share on one tile."""
    store, Lq, scale = R.FMT[dtype], 96, 1.0 / math.sqrt(hd)
    q, k, v = _prefill_problem(Lq, 0, hd, dtype, 13 * hd)
    k[5] = (q[40:].float().mean(0) * 2.0).to(dtype)              # key 5 is heavy for the later rows (its tile-1 twin, key 69, is not)
    ref, bound = R.prefill_ref_and_bound(q, k, v, scale, 0, True, store)
    assert (_prefill_f32(q, k, v, scale, 0, dtype) - ref).abs().le(bound).all()

    def broken(k2=k, v2=v, rows=slice(None), **kw):
        got = _prefill_f32(q, k2, v2, scale, 0, dtype, **kw)
        return float(((got - ref).abs() > bound)[rows].double().mean())

    assert broken(lim_shift=-1) > 0.1
    assert broken(lim_shift=1, rows=slice(0, Lq - 1)) > 0.1       # (the last row has no key behind its diagonal)
    k2, v2 = k.clone(), v.clone()
    k2[5], v2[5] = k[69], v[69]
    assert broken(k2, v2, rows=slice(40, None)) > 0.1
    # (tile 1 = keys 64 .. 95: rows 80 .. 95 see keys of its dropped half-wave, keys 80 .. 95)
    assert broken(l_bug_tile=0) > 0.5 and broken(l_bug_tile=1, rows=slice(80, None)) > 0.5
