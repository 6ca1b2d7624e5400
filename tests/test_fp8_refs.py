"""CPU tests of ``tests/fp8_refs.py``: the decode tables and the rounding search against torch's own CPU float8
conversion, the scale-update reference's defining inequalities, and the invariants of the input builders that
``tests/test_fp8_edges_gpu.py`` relies on (accept sets almost always a single code, saturating and subnormal
elements really present, exactness budgets of the GEMM operands)."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from . import fp8_refs as FR
from .rowwise_refs import f64

DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
DTYPES = [torch.float32, torch.bfloat16]


def torch_codes(x32: torch.Tensor, fmt: str) -> torch.Tensor:
    """torch's CPU conversion made saturating (its e4m3fn conversion alone is not: 1e9 -> NaN); NaN passes."""
    m = FR.FMAX[fmt]
    return x32.clamp(-m, m).to(DT[fmt]).view(torch.uint8)


# ------------------------------------------------------------------ decode / quantize
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_decode_equals_torch_float8(fmt):
    ref = torch.arange(256, dtype=torch.uint8).view(DT[fmt]).to(torch.float64)
    tab = FR.decode(fmt)
    assert torch.equal(torch.isnan(tab), torch.isnan(ref))
    assert torch.equal(tab.nan_to_num(nan=0.0), ref.nan_to_num(nan=0.0))
    assert torch.equal(torch.signbit(tab)[~torch.isnan(tab)], torch.signbit(ref)[~torch.isnan(ref)])
    assert torch.equal(FR.is_nan_code(torch.arange(256, dtype=torch.uint8), fmt), torch.isnan(ref))
    pos = FR.positive_codes(fmt)
    assert float(pos[-1]) == FR.FMAX[fmt] and bool((pos[1:] > pos[:-1]).all()) and bool(torch.isfinite(pos).all())


@pytest.mark.parametrize("fmt", FR.FMTS)
def test_quantize_equals_torch_on_random_fp32(fmt):
    """1e5 fp32 values with random sign, exponent (the full range, subnormals included) and mantissa."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2 ** 31, 2 ** 31, (100_000,), generator=g).to(torch.int32).view(torch.float32)
    x = torch.cat((x, 500 * torch.randn(20_000, generator=g), 1e-2 * torch.randn(20_000, generator=g)))
    got, ref = FR.quantize(x.double(), fmt), torch_codes(x, fmt)
    assert bool(torch.isnan(x).any()) and bool((x.abs() < 2.0 ** -126).any())
    assert bool(FR.same_codes(got, ref, fmt).all()), int((~FR.same_codes(got, ref, fmt)).sum())


@pytest.mark.parametrize("scale", FR.cast_scales())
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_cast_equals_torch_on_boundary_inputs(fmt, dtype, scale):
    x = FR.boundary_inputs(fmt, dtype, scale)
    prod = x.float() * torch.tensor(scale, dtype=torch.float32)  # torch's fp32 multiply: one rounding
    got, ref = FR.cast(x, scale, fmt), torch_codes(prod, fmt)
    assert bool(FR.same_codes(got, ref, fmt).all())
    # NaN, +-inf and -0 where the contract puts them
    xs = f64(x)
    assert torch.equal(FR.is_nan_code(got, fmt), torch.isnan(xs)) and bool(torch.isnan(xs).any())
    top = FR.positive_codes(fmt).numel() - 1
    assert bool((got[xs == math.inf] == top).all()) and bool((got[xs == -math.inf] == (0x80 | top)).all())
    assert bool((got[(xs == 0) & torch.signbit(xs)] == 0x80).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_boundary_inputs_layout_and_ties(fmt, dtype):
    """Odd length, a scalar tail of V - 1 special values, a special value at index 0; every tie is present in both
    signs and lands on the even mantissa; the tie neighbours land on either side."""
    V = FR.RR.vec_elems(dtype)
    x = FR.boundary_inputs(fmt, dtype, 2.0 ** -3)
    n = x.numel()
    assert n % 2 == 1 and n % V == V - 1
    assert math.isnan(float(x[0])) and math.isnan(float(x[n - V + 1])) and float(x[n - V + 2]) == -math.inf
    v = f64(x) * 2.0 ** -3  # the exact products
    pos = FR.positive_codes(fmt)
    mids = (pos[:-1] + pos[1:]) / 2
    codes = FR.cast(x, 2.0 ** -3, fmt)
    for sign in (1.0, -1.0):
        for k, m in enumerate(mids.tolist()):
            hit = v == sign * m
            assert bool(hit.any()), (sign, m)
            even = k if k % 2 == 0 else k + 1
            assert bool((codes[hit] == (even | (0x80 if sign < 0 else 0))).all()), (sign, m)
    below, above = FR._step(FR._to_dtype(mids, dtype), -1), FR._step(FR._to_dtype(mids, dtype), 1)
    k = torch.arange(mids.numel())
    assert torch.equal(FR.quantize(f64(below), fmt).long(), k) and torch.equal(FR.quantize(f64(above), fmt).long(), k + 1)
    half_sub = float(pos[1]) / 2
    assert bool((codes[v == half_sub] == 0).all()) and bool((codes[v == -half_sub] == 0x80).all())
    assert bool((v == half_sub).any()) and bool((v == -half_sub).any())
    # the saturating values are there
    assert bool((v.abs()[torch.isfinite(v)] > FR.FMAX[fmt]).any()) and bool((v == FR.FMAX[fmt]).any())
    # the finite variant has no NaN / inf and the same layout
    xf = FR.boundary_inputs(fmt, dtype, 2.0 ** -3, nonfinite=False)
    assert bool(torch.isfinite(xf.float()).all()) and xf.numel() % V == V - 1
    for (N, K), T in (((64, 64), 64), ((192, 128), 64), ((128, 128), 128), ((128, 384), 128)):
        w = f64(FR.tiled_boundary_matrix(fmt, N, K, 2.0 ** 7)).abs() * 2.0 ** 7
        tie = torch.isin(w, mids)
        sub = (w < float(pos[2 ** FR._BITS[fmt][1]])) & (w != 0)
        for m in (tie, sub, tie & sub):  # folded onto one T x T tile: every row and column position is met
            t = m.reshape(N // T, T, K // T, T).any(0).any(1)
            assert bool(t.any(0).all() and t.any(1).all()), (N, K)


def test_round_bf16_single_rounding():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(50_000, generator=g, dtype=torch.float64) * torch.exp(40 * torch.randn(50_000, generator=g)).double()
    x32 = x.float()
    assert torch.equal(FR.round_bf16(x32.double()), x32.to(torch.bfloat16).double())  # fp32 inputs: torch is exact
    # a float64 just above a bf16 midpoint rounds up here, down through fp32
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 3.0e38 * 1.2, -1e-45, math.inf, math.nan], dtype=torch.float64)
    r = FR.round_bf16(v)
    assert r[0] == 1.0 + 2.0 ** -7 and r[1] == math.inf and r[2] == 0 and r[3] == math.inf and math.isnan(r[4])


# ------------------------------------------------------------------ update_scales
@pytest.mark.parametrize("margin", [1.0, 1.5])
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_update_scales_reference_inequalities(fmt, margin):
    am = FR.scale_cases(fmt)
    n = am.numel()
    scale, inv, hist, zero = FR.update_scales(am, torch.zeros(n, 4), 0, margin, fmt)
    assert torch.equal(hist[:, 0], am) and not bool(zero.any())
    fmax = FR.FMAX[fmt]
    ulp = 2.0 ** -23  # one fp32 ulp of allowance on the quotient
    for a, s, i in zip(am.tolist(), scale.tolist(), inv.tolist()):
        assert math.isfinite(s) and s > 0 and math.frexp(s)[0] == 0.5, (a, s)  # a power of two
        assert np.float32(s) * np.float32(i) == 1 and i >= 2.0 ** -126, (a, s, i)
        if a == 0 or not math.isfinite(a):
            assert s == 1.0
            continue
        if 2.0 ** -126 < s < 2.0 ** 126:
            assert s * a * margin <= fmax * (1 + ulp) and fmax * (1 - ulp) < 2 * s * a * margin, (a, s)
        elif s == 2.0 ** 126:
            assert s * a * margin <= fmax * (1 + ulp)
        else:  # fl32(m margin) overflowed: pinned at the smallest normal scale instead of 0
            assert np.isinf(np.float32(a) * np.float32(margin))
    # exact powers of two at margin 1: the scale is the quotient itself
    if margin == 1.0:
        assert scale[:41].tolist() == [2.0 ** k for k in range(-20, 21)]
    tiny = (am > 0) & (am < 2.0 ** -126)
    assert int(tiny.sum()) == 2 and bool((scale[tiny] == 2.0 ** 126).all())


@pytest.mark.parametrize("fmt", FR.FMTS)
def test_update_scales_reference_ring_wrap(fmt):
    H = 4
    hist = torch.zeros(1, H)
    seq = [8.0, 1.0, 1.0, 1.0, 1.0, 0.5]  # pos = H overwrites the 8, pos = H + 1 the first 1
    scales = []
    for t, a in enumerate(seq):
        s, _, hist, _ = FR.update_scales(torch.tensor([a]), hist, t, 1.0, fmt)
        scales.append(float(s))
    f = 2.0 ** math.floor(math.log2(FR.FMAX[fmt]))
    assert scales == [f / 8, f / 8, f / 8, f / 8, f, f]
    assert hist.tolist() == [[1.0, 0.5, 1.0, 1.0]]


# ------------------------------------------------------------------ fused-cast builders and accept sets
def _fused_cases():
    for M, F in FR.SWIGLU_SHAPES:
        gu, da = FR.swiglu_inputs(M, F)
        yield f"swiglu fwd {M}x{F}", "e4m3", FR.swiglu_fwd(gu, FR.SWIGLU_FWD_SCALE), gu, None, FR.SWIGLU_FWD_SCALE
        yield f"swiglu bwd {M}x{F}", "e5m2", FR.swiglu_bwd(gu, da, FR.SWIGLU_BWD_SCALE), gu, da, FR.SWIGLU_BWD_SCALE
    gu, da = FR.swiglu_edge_inputs()
    yield "swiglu fwd edge", "e4m3", FR.swiglu_fwd(gu, FR.EDGE_SCALE), gu, None, FR.EDGE_SCALE
    yield "swiglu bwd edge", "e5m2", FR.swiglu_bwd(gu, da, FR.EDGE_BWD_SCALE), gu, da, FR.EDGE_BWD_SCALE
    for M, N in FR.NORM_SHAPES:
        x, d, w = FR.norm_inputs(M, N)
        for add in (True, False):
            yield f"norm {M}x{N} add={add}", "e4m3", FR.add_rmsnorm(x, d if add else None, w, 1e-5, FR.NORM_SCALE)[2], \
                None, None, FR.NORM_SCALE


def test_accept_sets_are_almost_always_one_code(capsys):
    """A condition on the GPU tests' inputs: at least 99.5 % of the elements admit exactly one byte."""
    with capsys.disabled():
        for what, fmt, acc, *_ in _fused_cases():
            share = float((acc.lo != acc.hi).double().mean())
            print(f"\n{what}: {share:.2e} of the accept sets hold more than one code", end="")
            assert share <= 0.005, (what, share)
            # one bf16 place, except the backward edge rows: at g = 1e4 the bound on g (1 - sg) is 2 % of dg
            assert acc.amax_lo <= acc.amax_hi <= acc.amax_lo * (1 + (2.0 ** -5 if "bwd edge" in what else 2.0 ** -7))


def test_fused_inputs_reach_saturation_and_subnormals():
    for what, fmt, acc, gu, da, scale in _fused_cases():
        if "edge" in what:
            continue
        top = FR.positive_codes(fmt).numel() - 1
        first_normal = 1 << FR._BITS[fmt][1]
        mag = acc.lo & 0x7F
        assert int((mag == top).sum()) >= 4, what
        assert int(((mag > 0) & (mag < first_normal)).sum()) >= 4, what
        assert int(((mag >= first_normal) & (mag < top)).sum()) > acc.lo.numel() // 2, what


def test_gate_inputs_below_g_min_give_the_zero_code():
    """DELTA_* hold for g >= G_MIN.  Where an input has g < G_MIN the output must not depend on the bound: even
    with a 50 % error both ends give the same (zero) code."""
    seen = 0
    for what, fmt, acc, gu, da, scale in _fused_cases():
        if gu is None:
            continue
        F = gu.shape[1] // 2
        low = f64(gu[:, :F]) < FR.G_MIN
        wide = FR.swiglu_fwd(gu, scale, fmt, delta=0.5) if da is None else FR.swiglu_bwd(gu, da, scale, fmt, delta=0.5)
        low = low if da is None else torch.cat((low, low), dim=1)
        seen += int(low.sum())
        assert bool(((wide.lo[low] & 0x7F) == 0).all() and ((wide.hi[low] & 0x7F) == 0).all()), what
    assert seen > 0  # the edge rows have g = -20, -88, -1e4


def test_in_accept():
    acc = FR.Accept(torch.tensor([0x38, 0x38, 0x80, 0x7F, 0x05], dtype=torch.uint8),
                    torch.tensor([0x38, 0x39, 0x01, 0x7F, 0x05], dtype=torch.uint8),
                    torch.tensor([False, False, False, False, True]), 0.0, 0.0)
    yes = torch.tensor([0x38, 0x39, 0x00, 0xFF, 0x80], dtype=torch.uint8)
    no = torch.tensor([0x39, 0x3A, 0x02, 0x7E, 0x06], dtype=torch.uint8)
    assert FR.in_accept(yes, acc, "e4m3").tolist() == [True] * 5
    assert FR.in_accept(no, acc, "e4m3").tolist() == [False] * 5


# ------------------------------------------------------------------ GEMM operands
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_all_codes_matrix_and_diagonal(fmt):
    for K in (256, 384):
        a = FR.all_codes_matrix(fmt, 256, K)
        finite = torch.isfinite(FR.decode(fmt))
        want = set(torch.arange(256)[finite].tolist())
        for k in (0, 1, 127, K - 1):  # every finite code in a k position
            assert set(a[:, k].tolist()) == want
        assert bool(finite[a.long()].all())
        b, d = FR.diag_matrix("e4m3", 256, K)
        prod = FR.decode(fmt)[a.long()] @ FR.decode("e4m3")[b.long()].t()
        assert torch.equal(prod, FR.decode(fmt)[a[:, :256].long()] * d)
        assert torch.equal(FR.round_bf16(prod * 2.0), prod * 2.0)  # gemm_fp8's output is exact in bf16
        c = prod + 4.0                                            # gemm_fp8_acc onto integers in [-4, 4]
        assert torch.equal(c.float().double(), c) and torch.equal((prod - 4.0).float().double(), prod - 4.0)


@pytest.mark.parametrize("fmt", FR.FMTS)
def test_window_codes_bit_budget(fmt):
    a, b = FR.window_codes(fmt, 256, 384, 41), FR.window_codes("e4m3", 256, 384, 43)
    va, vb = FR.decode(fmt)[a.long()], FR.decode("e4m3")[b.long()]
    assert bool((va.abs() >= 1).all() and (va.abs() < 8).all() and (vb.abs() >= 1).all() and (vb.abs() < 8).all())
    assert len(set(a.flatten().tolist())) == 2 * 3 * (1 << FR._BITS[fmt][1])  # every mantissa, sign and exponent
    exact = va @ vb.t()
    absum = va.abs() @ vb.abs().t()
    assert float(absum.max()) < 2.0 ** 15           # no partial sum in any order reaches 2^15 ...
    assert torch.equal(torch.round(exact * 64), exact * 64)  # ... and every product is a multiple of 2^-6: 21 bits
    assert torch.equal(exact.float().double(), exact)
