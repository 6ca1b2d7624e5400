"""CPU tests of ``tests/gemm_refs.py``: the invariants that ``tests/test_gemm_edges_gpu.py`` relies on, asserted on
the very inputs it uses -- exactness budgets, how much of the exact-accumulation outputs exercise the fp32 -> bf16
rounding, that the accept sets are almost always a single bf16 value, and that the planted edge values are there."""

from __future__ import annotations

import math

import pytest
import torch

from . import fp8_refs as FR
from . import gemm_refs as GR
from .rowwise_refs import f64

ALL_CASES = sorted({(GR.PP_SHAPE, R) for R, _ in GR.PP_CASES} | {(GR.G128_SHAPE, R) for R, _ in GR.G128_CASES}
                   | {(GR.G256_SHAPE, R) for R, _ in GR.G256_CASES})


def test_round_bf16_is_one_rounding_where_torch_rounds_twice():
    """257 + 2^-20 lies above the midpoint of 256 and 258: one rounding gives 258; through fp32 (257, a tie) 256."""
    v = torch.tensor([257.0 + 2.0 ** -20, 257.0, 259.0, -257.0, 3.3961775292304601e38, 2.0 ** -134],
                     dtype=torch.float64)
    assert FR.round_bf16(v).tolist() == [258.0, 256.0, 260.0, -256.0, math.inf, 0.0]
    assert float(v[:1].to(torch.float32).to(torch.bfloat16)) == 256.0


@pytest.mark.parametrize("shape,R", ALL_CASES)
def test_exact_accumulation_inputs(shape, R):
    """Operands and C are bf16 values; every partial sum plus beta * C stays below 2^24 (2^23 for the half-integers
    of beta = -0.5); the outputs exercise the rounding: >= 30 % need it, >= 10 % are exact ties, truncation would
    change >= 10 %, and with beta = 1 rounding the product before adding C would change >= 5 %."""
    M, N = shape
    A, B = GR.int_operands(M, N, R)
    C = GR.int_c(M, N)
    for t in (A, B, C):
        assert torch.equal(f64(GR.to_bf16(t)), t)
    a = GR.int_amax(R)
    assert float(A.abs().max()) == a and float(B.abs().max()) == a and float(C.abs().max()) == GR.C_MAX
    assert GR.exact_bound(R) < 2 ** 24 and R * a * a < 2 ** 24
    # the bound really bounds: sum of |products| is what any partial sum, in any order, cannot exceed
    assert float((A.abs() @ B.abs().t()).max()) + 2 * GR.C_MAX <= GR.exact_bound(R) / 2
    P = GR.int_product(M, N, R)
    for beta in GR.BETAS:
        v = GR.gemm_exact(P, C, beta)
        sh = GR.rounding_shares(v, P if beta == 1.0 else None, C)
        print(f"{M}x{N} R={R} a={a} beta={beta}: {sh}")
        assert sh["rounded"] >= 0.30, sh
        assert sh["ties"] >= 0.10, sh
        assert sh["trunc"] >= 0.10, sh
        if beta == 1.0:
            assert sh["double"] >= 0.05, sh
        assert torch.equal(GR.gemm_ref(M, N, R, beta, True), v)
        assert torch.equal(GR.gemm_ref(M, N, R, beta, False), FR.round_bf16(v))


def test_issue_example_double_rounding():
    """acc = 257, C = 1: one rounding gives 258, rounding the product first 256."""
    P, C = torch.tensor([257.0], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64)
    assert float(FR.round_bf16(P + C)) == 258.0 and float(FR.round_bf16(FR.round_bf16(P) + C)) == 256.0
    assert GR.rounding_shares(P + C, P, C)["double"] == 1.0


def test_case_tables_cover_the_k_tile_counts():
    per = lambda R, s, bk: sorted({(i + 1) * (R // bk) // s - i * (R // bk) // s for i in range(s)})  # noqa: E731
    pp = [per(R, s, 64) for R, s in GR.PP_CASES]
    assert [1] in pp and [2] in pp and [3] in pp and [2, 3] in pp and [7] in pp
    assert any(s == R // 64 and s > 1 for R, s in GR.PP_CASES)  # splits = the K-tile count
    g = [per(R, s, 64) for R, s in GR.G128_CASES]
    assert [1] in g and [2] in g and [3] in g and [2, 3] in g
    for R, s in GR.G256_CASES:  # gemm_shape_ok of the 256-tile kernel
        assert R % 32 == 0 and R // 32 // s >= 3
    assert min(R for R, s in GR.G256_CASES if s == 1) == 96 and min(R for R, s in GR.G256_CASES if s == 3) == 288
    for R, _ in GR.PP_CASES + GR.G128_CASES + GR.G256_CASES:
        assert 64 <= R <= 448


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_poison_is_all_nonfinite(dtype):
    p = GR.poison(64, 40, dtype)
    assert not torch.isfinite(p).any()
    assert torch.isnan(p).any() and (p == math.inf).any() and (p == -math.inf).any()


def test_widen_keeps_the_values_and_the_sentinel():
    t = GR.to_bf16(GR.int_c(16, 24))
    parent, view = GR.widen(t, 8, 24, GR.SENTINEL16)
    assert torch.equal(view, t) and view.stride() == (48, 1) and view.data_ptr() == parent.data_ptr() + 16
    outside = torch.ones(16, 48, dtype=torch.bool)
    outside[:, 8:32] = False
    assert bool((parent.view(torch.int16)[outside] == GR.SENTINEL16).all())
    assert torch.isnan(GR.widen(t, 8, 24)[0][:, 0]).all()


@pytest.mark.parametrize("R", [64, 96, 192, 288])
def test_overflow_operands(R):
    """bf16 operands; monotone exact partial sums below fp32 overflow; the results hit the last finite bf16, the tie
    that goes to inf, inf of both signs, and a finite rounded value."""
    A, B, S = GR.overflow_operands(20, 8, R)
    assert torch.equal(f64(GR.to_bf16(A)), A) and torch.equal(f64(GR.to_bf16(B)), B)
    v = A @ B.t()
    assert torch.equal(v, (S * 2.0 ** 114).unsqueeze(1).expand(20, 8))
    assert float(v.abs().max()) < 3.4028234663852886e38
    assert bool(((A >= 0).all(1) | (A <= 0).all(1)).all())  # one sign per row: monotone partial sums
    r = FR.round_bf16(v)[:, 0].tolist()
    assert r[0] == GR.BF16_MAX and r[1] == -GR.BF16_MAX  # 16351: rounds down
    assert r[2] == math.inf and r[3] == -math.inf        # 16352: the tie goes to the even code, inf
    assert r[4] == math.inf and r[6] == math.inf and math.isfinite(r[8])


def test_subnormal_operands():
    A, B = GR.subnormal_operands(32, 16, 64, "out")
    assert torch.equal(f64(GR.to_bf16(A)), A) and float(A.abs()[A != 0].min()) >= 2.0 ** -126  # normal inputs
    v = A @ B.t()
    assert 0 < float(v.abs().max()) < 2.0 ** -126  # results below the fp32 normal range
    assert torch.equal(v.float().double(), v)      # ... but fp32 values (multiples of 2^-140 >= 2^-149)
    assert bool((FR.round_bf16(v) != 0).any())     # some survive as bf16 subnormals
    A, B = GR.subnormal_operands(32, 16, 64, "in")
    assert torch.equal(f64(GR.to_bf16(A)), A) and float(A.abs().max()) < 2.0 ** -126  # bf16-subnormal inputs
    v = A @ B.t()
    assert float(v.abs()[v != 0].min()) >= 2.0 ** -126 and torch.equal(v.float().double(), v)


# ------------------------------------------------------------------ accept sets
def test_in_accept16():
    v = torch.tensor([1.0, 257.0, math.nan, math.inf, 1e-40, -0.0], dtype=torch.float64)
    acc = GR.accept16(v, torch.tensor([0.0, 0.5, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64))
    assert acc.lo.tolist()[:2] == [1.0, 256.0] and acc.hi.tolist()[:2] == [1.0, 258.0]
    ok = GR.in_accept16(torch.tensor([1.0, 258.0, math.nan, math.inf, 0.0, 0.0], dtype=torch.float64), acc)
    assert bool(ok.all())
    bad = GR.in_accept16(torch.tensor([1.0078125, 260.0, 0.0, math.nan, 1.0, 1.0], dtype=torch.float64), acc)
    assert not bool(bad.any())
    assert math.copysign(1.0, float(acc.lo[5])) == -1.0  # a -0 reference stays -0


@pytest.mark.parametrize("D", sorted(GR.ROPE_HEADS))
@pytest.mark.parametrize("S,M", GR.ROPE_SM)
def test_rope_accept_sets_are_single_codes(S, M, D):
    """At most 1 % of the elements accept more than one bf16 value (expected ~2^-13 of the rotated ones); the
    geometry is what the cases claim."""
    H, Hkv = GR.ROPE_HEADS[D]
    N, rot_cols = (H + 2 * Hkv) * D, (H + Hkv) * D
    assert N == 768 and M % S == 0 and rot_cols % D == 0
    if D == 96:
        assert rot_cols == 576 and rot_cols % 256 != 0 and 256 % D != 0
    A, B = GR.int_operands(M, N, GR.ROPE_R, seed=2)
    P = FR.round_bf16(A @ B.t())
    cos, sin = GR.rope_tables(S, D)
    assert cos.shape == (S + GR.ROPE_EXTRA_ROWS, D // 2) and cos.dtype == torch.float32
    rot, acc = GR.rope_epilogue(P, cos, sin, S, D, rot_cols)
    share = 1.0 - GR.single_code_share(acc)
    print(f"S={S} D={D}: {share:.2e} of the elements accept two codes")
    assert share <= 0.01
    assert torch.equal(acc.lo[~rot], P[~rot]) and torch.equal(acc.hi[~rot], P[~rot])
    # position 0 (rows m % S == 0) rotates by nothing; a row past the first sequence uses the table row m % S
    assert torch.equal(acc.lo[0], P[0]) and torch.equal(acc.lo[S], P[S])
    m, c = S + 3, 2 * D + 4  # an even column of head 2
    a, b = float(P[m, c]), float(P[m, c + 1])
    want = a * float(cos[3, 2]) - b * float(sin[3, 2])
    assert float(acc.lo[m, c]) <= float(FR.round_bf16(torch.tensor([want], dtype=torch.float64))) <= float(acc.hi[m, c])


def test_swiglu_forward_inputs():
    """x is one-hot with a power of two, w13 finite; the expected gu holds +-inf (from overflow only), the largest
    finite value, subnormals, zeros (all +0) and every edge magnitude; the accept sets of the finite elements are
    single codes for all but a few."""
    x, w13, gu = GR.swiglu_fwd_inputs()
    M, F, R = GR.SWF_SHAPE
    assert x.shape == (M, R) and w13.shape == (2 * F, R) and gu.shape == (M, 2 * F)
    assert torch.isfinite(w13).all() and torch.isfinite(x).all()
    xs = f64(x)
    assert bool(((xs != 0).sum(1) == 1).all())
    nz = xs[xs != 0]
    assert torch.equal(torch.frexp(nz)[0], torch.full_like(nz, 0.5))  # powers of two
    assert torch.equal(FR.round_bf16(xs @ f64(w13).t()).nan_to_num(nan=7.0), gu.nan_to_num(nan=7.0))
    assert (gu == math.inf).any() and (gu == -math.inf).any() and not torch.isnan(gu).any()
    assert (gu.abs() == GR.BF16_MAX).any() and ((gu != 0) & (gu.abs() < 2.0 ** -126)).any()
    exact = xs @ f64(w13).t()
    assert not torch.signbit(gu[exact == 0]).any()         # an exactly zero sum is +0
    under = (gu == 0) & (exact < 0)                        # an fp32 value that rounds to zero in bf16: -0
    assert torch.signbit(gu[under]).all() and under.any()
    inrange = exact.abs() < 3.4028235677973366e38          # every product that does not overflow is an fp32 value
    assert torch.equal(exact[inrange].float().double(), exact[inrange]) and float(exact[exact != 0].abs().min()) == 2.0 ** -149
    for v in (1e-30, 1.0, 20.0, 88.0, 1e4):
        b = float(torch.tensor(v).to(torch.bfloat16))
        assert (gu[:, :F] == b).any() and (gu[:, :F] == -b).any()  # (u is +-1.5 in the 1e-30 row)
    fin = torch.isfinite(gu[:, :F]) & torch.isfinite(gu[:, F:])
    acc = GR.swiglu_fwd_accept(gu)
    two = ((acc.lo != acc.hi) & fin).double().sum() / fin.double().sum()
    print(f"swiglu fwd: {float(two):.2e} of the finite elements accept two codes")
    assert float(two) <= 0.01


def test_swiglu_backward_inputs():
    dy, w2, gu, da = GR.swiglu_bwd_inputs()
    M, F, R = GR.SWB_SHAPE
    assert dy.shape == (M, R) and w2.shape == (R, F) and gu.shape == (M, 2 * F) and da.shape == (M, F)
    assert torch.isfinite(gu).all() and F % 256 == 0
    assert float((f64(dy).abs() @ f64(w2).abs()).max()) < 2 ** 24
    g = f64(gu)
    for v in (1e-30, 1.0, 20.0, 88.0, 1e4):
        b = float(torch.tensor(v).to(torch.bfloat16))
        assert (g[:, :F] == b).any() and (g[:, :F] == -b).any()
    assert ((g != 0) & (g.abs() < 2.0 ** -126)).any() and torch.signbit(g[g == 0]).any()
    acc = GR.swiglu_bwd_accept(g, da)
    # Edge values make wide sets by construction: the bound's scale A carries |g| sg 37 U for the error of (1 - sg),
    # percents of dg at |g| >= 20; and where sg is exactly 1/2 or 1 the exact result is a product of two 8-bit
    # numbers (da u / 2 with u = +-1.5 in the 1e-30 row), which is an exact bf16 tie for a third of the elements.
    # There the comparison with the unfused kernel is what binds.  At the generic magnitude |g| = 1 the sets are
    # single values for all but 1 %; overall at most a quarter are wide.
    wide = (acc.lo != acc.hi) & ~(torch.isnan(acc.lo) & torch.isnan(acc.hi))
    one = (g[:, :F].abs() == 1.0).repeat(1, 2)
    two = float((wide & one).double().sum() / one.double().sum())
    print(f"swiglu bwd: {two:.2e} of the |g| = 1 elements accept two codes, {float(wide.double().mean()):.2e} of all")
    assert two <= 0.01 and float(wide.double().mean()) <= 0.25
