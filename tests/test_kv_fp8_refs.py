"""The fp8 KV cache format on the CPU: ``ops.decode.kv_quantize_reference`` (the definition) against the properties
the format promises and against the independent float64 path of ``tests/kv_fp8_refs.py``; ``kv_append_fp8_reference``
against ``decode_refs.kv_append`` + that path.

Bounds, all derived: with ``s`` the row's scale, ``|x / s| <= 448`` and e4m3 has 3 mantissa bits, so a normal result
is off by at most half an ulp, ``2^-4 |x|``, and a subnormal one (``|x / s| < 2^-6``, spacing ``2^-9``) by at most
``2^-10 s``: ``|deq - x| <= max(2^-4 |x|, 2^-10 s)`` per element.
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.ops import decode as OD
from bpe_transformer.ops import reference as R

from . import decode_refs as DR
from . import kv_fp8_refs as KR
from .decode_refs import BF16, f64


def _rows(D=64, n=4096, seed=0):
    g = torch.Generator().manual_seed(seed)
    mag = 10 ** (torch.rand(n, 1, generator=g) * 10 - 6)  # 1e-6 .. 1e4
    return (torch.randn(n, D, generator=g) * mag).to(BF16)


@pytest.mark.parametrize("D", [64, 128])
def test_quantiser_properties_on_random_rows(D):
    x = _rows(D)
    q, s = OD.kv_quantize_reference(x)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and s.shape == x.shape[:-1]
    m, _ = torch.frexp(s)
    assert torch.equal(m, torch.full_like(m, 0.5)), "scales are powers of two"
    r = (f64(x) / f64(s)[:, None]).abs().amax(-1)
    assert float(r.max()) <= 448.0 and float(r.min()) > 224.0, (float(r.min()), float(r.max()))
    deq = OD.kv_dequantize_reference(q, s)
    assert deq.dtype == BF16
    assert torch.equal(f64(deq), f64(q.float()) * f64(s)[:, None]), "dequantised values are bf16 values"
    assert torch.equal(deq.float().to(BF16), deq)
    err = (f64(deq) - f64(x)).abs()
    assert bool((err <= torch.maximum(2.0 ** -4 * f64(x).abs(), 2.0 ** -10 * f64(s)[:, None])).all())
    assert float((err.amax(-1) / f64(x).abs().amax(-1)).max()) <= 2.0 ** -4


@pytest.mark.parametrize("D", [64, 128])
def test_quantiser_equals_the_independent_float64_path(D):
    x = torch.cat([_rows(D, 1024, seed=1), KR.planted(D)])
    q, s = OD.kv_quantize_reference(x)
    c64, s64 = KR.quantize64(x)
    assert torch.equal(f64(s), s64)
    assert torch.equal(KR.codes(q), c64)
    assert torch.equal(f64(OD.kv_dequantize_reference(q, s)), KR.dequantize64(c64, s64))


def test_quantiser_scale_boundaries():
    rows = KR.special_rows(64)
    scale = lambda name: float(OD.kv_quantize_reference(rows[name][None])[1])
    for k in (-3, 0, 5):
        assert scale(f"448*2^{k}") == 2.0 ** k and scale(f"450*2^{k}") == 2.0 ** (k + 1)
        # 450 * 2^k is the next bf16 above 448 * 2^k
        a = rows[f"448*2^{k}"][0]
        assert float(rows[f"450*2^{k}"][0]) == float((a.view(torch.int16) + 1).view(BF16))
    assert scale("m=0.875") == 2.0 ** -6 and scale("m>0.875") == 2.0 ** -5
    assert float(rows["m>0.875"][0]) == float((rows["m=0.875"][0].abs().view(torch.int16) + 1).view(BF16))
    q, s = OD.kv_quantize_reference(rows["m=0.875"][None])
    assert float(q.float()[0, 0]) == -448.0
    assert scale("zero") == 1.0 and scale("clamped") == 2.0 ** -64 and scale("clamp edge") == 2.0 ** -64
    assert scale("below edge") == 2.0 ** -64 and scale("huge") == 2.0 ** 120
    q, _ = OD.kv_quantize_reference(rows["clamped"][None])
    assert not KR.codes(q).bitwise_and(0x7F).any(), "a row below the clamp quantises to zeros"
    q, _ = OD.kv_quantize_reference(rows["below edge"][None])
    assert float(q.float()[0, 0]) == 128.0
    q, _ = OD.kv_quantize_reference(rows["zero"][None])
    assert not KR.codes(q).any()


def test_quantiser_reaches_the_subnormals_and_ties():
    """The planted fillers land on e4m3 subnormals and on exact ties (which go to the even code)."""
    q, s = OD.kv_quantize_reference(KR.special_rows(64)["448*2^0"][None])
    got = q.float()[0, 1:9].tolist()
    # 1, -0.75, 0.3125 exact; 2^-7 and -2^-8 subnormal; 3 * 2^-10 is the tie between 2^-9 and 2^-8 -> 2^-8 (code 2);
    # 2^-10 the tie between 0 and 2^-9 -> 0 (code 0); 5 * 2^-10 the tie between 2^-8 and 3 * 2^-9 -> 2^-8 (code 2)
    assert got == [1.0, -0.75, 0.3125, 2.0 ** -7, -(2.0 ** -8), 2.0 ** -8, 0.0, 2.0 ** -8], got


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_quantiser_non_finite_row(bad):
    x = _rows(64, 4)
    x[2, 17] = bad
    q, s = OD.kv_quantize_reference(x)
    assert torch.isnan(s[2]) and torch.isfinite(s[[0, 1, 3]]).all()
    assert torch.isnan(OD.kv_dequantize_reference(q, s)[2]).all()
    assert torch.isnan(KR.quantize64(x)[1][2])


# ------------------------------------------------------------------ kv_append_fp8_reference
def _append_case(B, T, H, Hkv, D, Lmax, pos, rope=True, plant=False):
    W = (H + 2 * Hkv) * D
    qkv = DR.randn(B * T, W, seed=(sum(pos), T, D))
    if plant:  # special rows into V of head 0, one per token row
        sp = KR.planted(D)
        for i in range(B * T):
            qkv.view(B * T, H + 2 * Hkv, D)[i, H + Hkv] = sp[i % sp.shape[0]]
    cos, sin = R.rope_tables(D, Lmax + 8, 10000.0) if rope else (None, None)
    old = KR.fp8_caches(B, Hkv, Lmax, D, 0, seed=5)  # poison everywhere: untouched rows stay poison
    k8, v8, ks, vs = old["k8"].clone(), old["v8"].clone(), old["ks"].clone(), old["vs"].clone()
    p = torch.tensor(pos, dtype=torch.int32)
    q = OD.kv_append_fp8(qkv, k8, v8, ks, vs, cos, sin, p, B, T, H)
    plist = pos if len(pos) > 1 else pos * B
    for b, p0 in enumerate(plist):
        ref = DR.kv_append(f64(qkv.view(B, T, -1)[b]), None if cos is None else cos.double(),
                           None if sin is None else sin.double(), p0, 1, T, H, Hkv, D, Lmax)
        n = ref["n"]
        assert n == max(0, min(T, Lmax - p0))
        # q: the bf16 kv_append oracle's, which decode_refs bounds; here bit for bit the same function
        kc, vc = torch.zeros(1, Hkv, Lmax, D, dtype=BF16), torch.zeros(1, Hkv, Lmax, D, dtype=BF16)
        q_bf = OD.kv_append_reference(qkv.view(B, T, -1)[b], kc, vc, cos, sin, p[b:b + 1] if len(pos) > 1 else p, 1, T, H)
        assert torch.equal(q.view(B, T, -1)[b], q_bf)
        err = (f64(q_bf).view(1, T, H, D)[:, :n] - ref["q"][:, :n]).abs()
        assert bool((err <= DR.bound(ref["q"][:, :n], ref["aq"][:, :n], 1e-5)).all())
        # K / V rows: quantise64 of the bf16 rows the bf16 cache would hold
        for t8, ts, cache in ((k8, ks, kc), (v8, vs, vc)):
            c64, s64 = KR.quantize64(cache[0, :, p0:p0 + n])
            assert torch.equal(KR.codes(t8)[b, :, p0:p0 + n], c64) and torch.equal(f64(ts[b, :, p0:p0 + n]), s64)
        assert torch.equal(f64(vc[0, :, p0:p0 + n]), ref["v"][0])
        # every other row of the slab is untouched (still poison)
        for t8, ts in ((k8, ks), (v8, vs)):
            rest = torch.ones(Lmax, dtype=torch.bool)
            rest[p0:p0 + n] = False
            assert bool((KR.codes(t8)[b][:, rest] == KR.NAN_BYTE).all()) and bool(torch.isnan(ts[b][:, rest]).all())
    return q


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rope", [True, False])
def test_append_reference_slab_isolation(rope, D):
    _append_case(2, 3, 4, 2, D, 16, [5], rope=rope)


def test_append_reference_nearly_full_cache_drops_the_tail():
    _append_case(2, 3, 4, 2, 64, 16, [14])


def test_append_reference_ragged_positions():
    _append_case(3, 2, 4, 2, 64, 16, [0, 15, 7])


def test_append_reference_special_rows_in_v():
    _append_case(4, 4, 2, 1, 64, 32, [3], plant=True)


def test_decode_attention_fp8_reference_is_the_bf16_oracle_on_dequantised_caches():
    c = KR.fp8_caches(2, 2, 300, 64, [1, 300], spread=True)
    q = DR.queries(2, 1, 4, 64)
    pos = torch.tensor([0, 299], dtype=torch.int32)
    a = OD.decode_attention_fp8(q, c["k8"], c["v8"], c["ks"], c["vs"], pos, 4)
    b = OD.decode_attention_reference(q, c["k"], c["v"], pos, 4)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    ko, vo = torch.full_like(c["k"], 7.0), torch.full_like(c["v"], 7.0)
    OD.kv_dequant(c["k8"], c["v8"], c["ks"], c["vs"], pos, 1, ko, vo)
    assert torch.equal(ko[0, :, :1], c["k"][0, :, :1]) and torch.equal(vo[1], c["v"][1])
    assert bool((ko[0, :, 1:] == 7.0).all()) and bool((vo[0, :, 1:] == 7.0).all())
