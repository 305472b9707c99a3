"""The host restatement of the decode attention kernels (tests/attn_ref.py) on its own: the page layout round-trips, V saturates into the
fp16 pages, the fp32 fused multiply-add emulation of the rotary embedding is exact, an fp32 attention stays inside decode_bound, and the
bound is tight enough that one wrong key breaks it. No GPU needed."""
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
