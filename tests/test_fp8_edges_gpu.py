"""The fp8 training path's kernels (``csrc/fp8.hip`` casts and ``update_scales``, ``pack4_fp8`` in ``csrc/common.h``,
the F8 forms of ``csrc/gemm_pp.hip``) against the plain references of ``tests/fp8_refs.py``, at the values where a
cast can go wrong: every rounding tie, the fp8 subnormal range, the last finite code, saturation, +-0, NaN / inf,
and every operand code through the MFMA decode.

Inputs are built on the CPU (fixed seed, already rounded to the input dtype) and copied to the GPU.  Bounds:

* the plain casts, the scale update and the GEMMs are exact: every byte / bit equals the reference (NaN codes
  compare as a class -- which NaN code is written is not part of the contract);
* the fused casts compute their value in fp32 before rounding it to bf16, so each output byte must lie in the
  reference's accept interval (``fp8_refs.Accept``; a single code for all but ~0.1 % of the elements, asserted
  on these very inputs in ``tests/test_fp8_refs.py``).  There is no mismatch budget.
"""

from __future__ import annotations

import math

import pytest
import torch

from . import fp8_refs as FR
from .rowwise_refs import f64, vec_elems

pytestmark = pytest.mark.gpu

DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
DTYPES = [torch.float32, torch.bfloat16]
MAXC = {"e4m3": 0x7E, "e5m2": 0x7B}


def _f32(dev, v: float) -> torch.Tensor:
    return torch.tensor([v], dtype=torch.float32, device=dev)


def _slot(dev, v: float = 0.0) -> torch.Tensor:
    return torch.tensor([v], dtype=torch.float32).view(torch.int32).to(dev)


def _slot_value(slot: torch.Tensor) -> float:
    return slot.view(torch.float32).item()


def _u8(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8).cpu()


def _cast(dev, x, scale, fmt, slot=None):
    out = torch.empty(x.shape, dtype=DT[fmt], device=dev)
    slot = _slot(dev) if slot is None else slot
    torch.ops.bpe_hip.cast_fp8(x.to(dev), _f32(dev, scale), out, slot)
    return _u8(out), _slot_value(slot)


def _cast_t(dev, w, scale, fmt):
    N, K = w.shape
    w8 = torch.empty(N, K, dtype=DT[fmt], device=dev)
    w8t = torch.empty(K, N, dtype=DT[fmt], device=dev)
    slot = _slot(dev)
    torch.ops.bpe_hip.cast_fp8_t(w.to(dev), _f32(dev, scale), w8, w8t, slot)
    return _u8(w8), _u8(w8t), _slot_value(slot)


def assert_codes(got, ref, fmt, x=None, what=""):
    bad = ~FR.same_codes(got, ref, fmt)
    n = int(bad.sum())
    print(f"{what}: {n} of {bad.numel()} bytes differ")
    if n:
        i = bad.flatten().nonzero().flatten()[:8]
        show = [(int(j), hex(int(got.flatten()[j])), hex(int(ref.flatten()[j])),
                 None if x is None else float(x.flatten()[j])) for j in i]
        raise AssertionError((what, n, "index, got, ref, input", show))


# ------------------------------------------------------------------ a. cast_fp8
@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "naninf"])
@pytest.mark.parametrize("scale", FR.cast_scales())
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_cast_fp8_boundaries(gpu_device, fmt, dtype, scale, nonfinite):
    """Every code, every tie between two codes and its two input-dtype neighbours, +-0, the tie with zero, the
    last finite code and values past it (with ``naninf`` also +-inf and NaN), in the vector body, the scalar tail
    and at index 0: bytes and amax equal the reference exactly."""
    x = FR.boundary_inputs(fmt, dtype, scale, nonfinite)
    got, am = _cast(gpu_device, x, scale, fmt)
    assert_codes(got, FR.cast(x, scale, fmt), fmt, x, f"{fmt} {dtype} x{scale}")
    assert am == FR.amax(x), (am, FR.amax(x))


@pytest.mark.parametrize("n", [1, 7, "V-1"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_cast_fp8_tail_only(gpu_device, fmt, dtype, n):
    """Fewer elements than one vector: the scalar tail alone (n = 7 for fp32: one vector and a tail of three)."""
    n = vec_elems(dtype) - 1 if n == "V-1" else n
    full = FR.boundary_inputs(fmt, dtype, 2.0 ** -3, nonfinite=False)
    x = torch.cat((full[-3:], full[:8]))[:n].contiguous()  # ties to zero and the saturating half step first
    got, am = _cast(gpu_device, x, 2.0 ** -3, fmt)
    assert_codes(got, FR.cast(x, 2.0 ** -3, fmt), fmt, x, f"{fmt} {dtype} n={n}")
    assert am == FR.amax(x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_cast_fp8_amax_slot(gpu_device, fmt, dtype):
    """The amax slot is a running maximum: a larger recorded value is kept, a smaller one replaced; an all-negative
    tensor records max |x|; a tensor of only +-0 records 0 and keeps the signs of its zeros."""
    dev = gpu_device
    x = FR.boundary_inputs(fmt, dtype, 1.0, nonfinite=False)
    x = x[f64(x).abs() <= FR.FMAX[fmt]].contiguous()
    ref = FR.amax(x)
    assert ref == FR.FMAX[fmt]
    assert _cast(dev, x, 1.0, fmt, _slot(dev, 2 * ref))[1] == 2 * ref
    assert _cast(dev, x, 1.0, fmt, _slot(dev, ref / 2))[1] == ref
    neg = -x.abs()
    got, am = _cast(dev, neg, 1.0, fmt)
    assert am == ref
    assert_codes(got, FR.cast(neg, 1.0, fmt), fmt, neg, "all negative")
    z = torch.zeros(2 * vec_elems(dtype) + 3, dtype=dtype)
    z[1::2] = -0.0
    got, am = _cast(dev, z, 4.0, fmt)
    assert am == 0.0
    assert got.tolist() == [0x80 if i % 2 else 0 for i in range(z.numel())]


# ------------------------------------------------------------------ b. cast_fp8_t
# (64, 64), (192, 128): the 64 x 64 kernel; (128, 128), (128, 384): the 128 x 128 one
@pytest.mark.parametrize("scale", [2.0 ** 7, 0.37])
@pytest.mark.parametrize("N,K", [(64, 64), (192, 128), (128, 128), (128, 384)])
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_cast_fp8_t_boundaries(gpu_device, fmt, N, K, scale):
    """The two-layout cast on the boundary set tiled over the matrix: the row-major bytes equal the reference,
    the transposed output is their transpose, amax is exact."""
    w = FR.tiled_boundary_matrix(fmt, N, K, scale)
    w8, w8t, am = _cast_t(gpu_device, w, scale, fmt)
    assert_codes(w8, FR.cast(w, scale, fmt), fmt, w, f"{fmt} {N}x{K} x{scale}")
    assert torch.equal(w8t, w8.t())
    assert am == FR.amax(w)


# ------------------------------------------------------------------ c. fused casts
def _state(dev, fmt, scale):
    from bpe_transformer.ops.fp8 import Fp8State

    st = Fp8State(1, dev, fmt=fmt)
    st.scale.fill_(scale)
    return st


def check_fused(o8, o8t, acc: FR.Accept, st, fmt, what):
    got = _u8(o8)
    single = acc.lo == acc.hi
    ok = FR.in_accept(got, acc, fmt)
    ok &= ~single | acc.tiny | FR.same_codes(got, acc.lo, fmt)  # a single candidate: that very byte, sign included
    n = int((~ok).sum())
    print(f"{what}: {n} of {ok.numel()} bytes outside their accept set; "
          f"{float((~single).double().mean()):.2e} of the sets are not a single code")
    if n:
        i = (~ok).flatten().nonzero().flatten()[:8]
        raise AssertionError((what, n, "index, got, lo, hi", [
            (int(j), hex(int(got.flatten()[j])), hex(int(acc.lo.flatten()[j])), hex(int(acc.hi.flatten()[j])))
            for j in i]))
    assert torch.equal(_u8(o8t), got.t()), what
    am = _slot_value(st.amax)
    print(f"{what}: amax {am!r} in [{acc.amax_lo!r}, {acc.amax_hi!r}]")
    assert acc.amax_lo <= am <= acc.amax_hi, (what, am, acc.amax_lo, acc.amax_hi)


@pytest.mark.parametrize("M,F", FR.SWIGLU_SHAPES)
def test_swiglu_fwd_cast_t_accept(gpu_device, M, F):
    from bpe_transformer.ops.fp8 import swiglu_fwd_cast_t

    gu, _ = FR.swiglu_inputs(M, F)
    st = _state(gpu_device, "e4m3", FR.SWIGLU_FWD_SCALE)
    a8, a8t = swiglu_fwd_cast_t(st, gu.to(gpu_device), 0)
    check_fused(a8, a8t, FR.swiglu_fwd(gu, FR.SWIGLU_FWD_SCALE), st, "e4m3", f"swiglu fwd {M}x{F}")


@pytest.mark.parametrize("M,F", FR.SWIGLU_SHAPES)
def test_swiglu_bwd_cast_t_accept(gpu_device, M, F):
    from bpe_transformer.ops.fp8 import swiglu_bwd_cast_t

    gu, da = FR.swiglu_inputs(M, F)
    st = _state(gpu_device, "e5m2", FR.SWIGLU_BWD_SCALE)
    g8, g8t = swiglu_bwd_cast_t(st, da.to(gpu_device), gu.to(gpu_device), 0)
    check_fused(g8, g8t, FR.swiglu_bwd(gu, da, FR.SWIGLU_BWD_SCALE), st, "e5m2", f"swiglu bwd {M}x{F}")


def test_swiglu_cast_t_edge_rows(gpu_device):
    """g and u from the activation edge rows (+-0, 1e-30, 1, 20, 88, 1e4): saturation of the sigmoid both ways,
    products that underflow fp32, zeros of both signs."""
    from bpe_transformer.ops.fp8 import swiglu_bwd_cast_t, swiglu_fwd_cast_t

    gu, da = FR.swiglu_edge_inputs()
    st = _state(gpu_device, "e4m3", FR.EDGE_SCALE)
    a8, a8t = swiglu_fwd_cast_t(st, gu.to(gpu_device), 0)
    check_fused(a8, a8t, FR.swiglu_fwd(gu, FR.EDGE_SCALE), st, "e4m3", "swiglu fwd edge rows")
    st = _state(gpu_device, "e5m2", FR.EDGE_BWD_SCALE)
    g8, g8t = swiglu_bwd_cast_t(st, da.to(gpu_device), gu.to(gpu_device), 0)
    check_fused(g8, g8t, FR.swiglu_bwd(gu, da, FR.EDGE_BWD_SCALE), st, "e5m2", "swiglu bwd edge rows")


def _norm_case(dev, x, d, w, what):
    from bpe_transformer.ops.fp8 import add_rmsnorm_cast_t

    st = _state(dev, "e4m3", FR.NORM_SCALE)
    xd = x.to(dev)
    s, (y8, y8t), rstd = add_rmsnorm_cast_t(st, xd, None if d is None else d.to(dev), w.to(dev), 1e-5, 0)
    s_ref, rstd_ref, acc = FR.add_rmsnorm(x, d, w, 1e-5, FR.NORM_SCALE)
    if d is None:
        assert s is xd
    else:
        assert s.dtype == torch.bfloat16 and torch.equal(f64(s).nan_to_num(nan=-7.0), s_ref.nan_to_num(nan=-7.0))
    fin = torch.isfinite(rstd_ref)
    err = float(((f64(rstd) - rstd_ref)[fin]).abs().max() / rstd_ref[fin].abs().max())
    print(f"{what}: rstd rel {err:.3e}")
    assert err < 1e-5  # test_rowwise_kernels_gpu.py's bound for add_rmsnorm_fwd's rstd
    check_fused(y8, y8t, acc, st, "e4m3", what)
    return rstd, rstd_ref


@pytest.mark.parametrize("add", [True, False], ids=["add", "noadd"])
@pytest.mark.parametrize("M,N", FR.NORM_SHAPES)
def test_add_rmsnorm_cast_t_accept(gpu_device, M, N, add):
    x, d, w = FR.norm_inputs(M, N)
    _norm_case(gpu_device, x, d if add else None, w, f"add_rmsnorm {M}x{N} add={add}")


# ------------------------------------------------------------------ d. fp8 GEMM operand decode
@pytest.fixture(params=[0, 1, 3], ids=["tile", "persist", "persist3"])
def gpp_mode(request, gpu_device):
    """gemm_pp kernel form, as in test_kernels_gpu.py: one tile per workgroup, persistent, persistent with 3
    workgroups."""
    h = torch.ops.bpe_hip
    prev = h.gpp_persist_config(request.param)
    yield request.param
    h.gpp_persist_config(prev)


def _all_codes_case(fmt_a: str, side: str, K: int):
    """(a codes, b codes, float64 a @ b^T) with every finite code of one operand against the diagonal pattern."""
    if side == "a":
        a = FR.all_codes_matrix(fmt_a, 256, K)
        b, _ = FR.diag_matrix("e4m3", 256, K)
    else:
        a, _ = FR.diag_matrix(fmt_a, 256, K)
        b = FR.all_codes_matrix("e4m3", 256, K)
    va, vb = FR.decode(fmt_a)[a.long()], FR.decode("e4m3")[b.long()]
    return a, b, va @ vb.t()


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("fmt_a", FR.FMTS)
def test_gemm_fp8_decodes_every_code(gpu_device, gpp_mode, fmt_a, side):
    """Every finite code (subnormals, +-max, -0) at every k position of one operand times a signed power-of-two
    diagonal: each output is one decoded code times a power of two, exact in bf16."""
    dev = gpu_device
    a, b, prod = _all_codes_case(fmt_a, side, 256)
    y = torch.ops.bpe_hip.gemm_fp8(a.view(DT[fmt_a]).to(dev), b.view(DT["e4m3"]).to(dev), _f32(dev, 0.25),
                                   _f32(dev, 8.0))
    ref = prod * 2.0
    assert torch.equal(FR.round_bf16(ref), ref)
    assert y.dtype == torch.bfloat16 and torch.equal(f64(y), ref)


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("splits", [1, 3])
def test_gemm_fp8_acc_decodes_every_code(gpu_device, splits, side):
    """The split-K accumulating form (e5m2 x e4m3, fp32 C, beta = 1 onto small integers); K = 384 for three
    splits (the binding wants one 128-wide K-tile per split), the diagonal partner's last 128 columns zero."""
    dev = gpu_device
    K = 128 * max(2, splits)
    a, b, prod = _all_codes_case("e5m2", side, K)
    c0 = torch.randint(-4, 5, (256, 256), generator=torch.Generator().manual_seed(splits)).double()
    ref = c0 + prod
    assert torch.equal(ref.float().double(), ref)
    c = c0.float().to(dev)
    torch.ops.bpe_hip.gemm_fp8_acc(a.view(DT["e5m2"]).to(dev), b.view(DT["e4m3"]).to(dev), _f32(dev, 0.5),
                                   _f32(dev, 2.0), c, 1.0, splits)
    assert torch.equal(f64(c), ref)


@pytest.mark.parametrize("fmt_a", FR.FMTS)
def test_gemm_fp8_dense_window_exact(gpu_device, gpp_mode, fmt_a):
    """Dense random codes from a three-exponent window per operand, every mantissa, both signs, K = 384.  Bit
    budget (``fp8_refs.window_codes``): 8-bit products whose magnitudes span 2^4, summed over fewer than 2^9 terms:
    8 + 4 + 9 = 21 bits < 24, so any order of fp32 accumulation is exact and the output is the one bf16 rounding of the exact
    value (fp32 C: the exact value)."""
    dev = gpu_device
    a = FR.window_codes(fmt_a, 256, 384, 41)
    b = FR.window_codes("e4m3", 256, 384, 43)
    exact = FR.decode(fmt_a)[a.long()] @ FR.decode("e4m3")[b.long()].t()
    a8, b8 = a.view(DT[fmt_a]).to(dev), b.view(DT["e4m3"]).to(dev)
    y = torch.ops.bpe_hip.gemm_fp8(a8, b8, _f32(dev, 0.25), _f32(dev, 2.0))
    assert torch.equal(f64(y), FR.round_bf16(exact * 0.5))
    if fmt_a == "e5m2":
        for splits in (1, 3):
            c = torch.zeros(256, 256, device=dev)
            torch.ops.bpe_hip.gemm_fp8_acc(a8, b8, _f32(dev, 0.25), _f32(dev, 2.0), c, 1.0, splits)
            assert torch.equal(f64(c), exact * 0.5), splits


# ------------------------------------------------------------------ e. update_scales
@pytest.mark.parametrize("margin", [1.0, 1.5])
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_update_scales_power_of_two_edges(gpu_device, fmt, margin):
    dev = gpu_device
    am = FR.scale_cases(fmt)
    n, H = am.numel(), 4
    hist0 = torch.zeros(n, H)
    slot = am.view(torch.int32).clone().to(dev)
    hist, scale, inv = hist0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    torch.ops.bpe_hip.update_scales(slot, hist, scale, inv, 0, margin, 0 if fmt == "e4m3" else 1)
    s_ref, i_ref, h_ref, _ = FR.update_scales(am, hist0, 0, margin, fmt)
    bad = (scale.cpu() != s_ref) | (inv.cpu() != i_ref)
    print(f"{fmt} margin {margin}: {int(bad.sum())} of {n} scales differ")
    assert not bad.any(), [(float(am[j]), float(scale[j]), float(s_ref[j]), float(inv[j]), float(i_ref[j]))
                           for j in bad.nonzero().flatten()[:8]]
    assert torch.equal(hist.cpu(), h_ref)
    assert slot.cpu().tolist() == [0] * n
    assert bool(torch.isfinite(scale).all()) and bool(((scale * inv) == 1).all())


@pytest.mark.parametrize("fmt", FR.FMTS)
def test_fp8_state_ring(gpu_device, fmt):
    """history = 4 driven six steps through Fp8State.update(): an old maximum governs the scale until the step
    that overwrites its ring slot, and not one step longer."""
    from bpe_transformer.ops.fp8 import Fp8State

    steps = torch.tensor([[8.0, 1.0, 1.0, 1.0, 1.0, 0.5],      # the 8 leaves at step 4 (slot 0 again)
                          [0.25, 64.0, 0.25, 0.25, 0.25, 0.25]])  # the 64 leaves at step 5
    st = Fp8State(2, gpu_device, history=4, fmt=fmt)
    hist = torch.zeros(2, 4)
    seen = []
    for t in range(6):
        st.amax.copy_(steps[:, t].contiguous().view(torch.int32))
        st.update()
        s_ref, i_ref, hist, _ = FR.update_scales(steps[:, t], hist, t, 1.0, fmt)
        assert torch.equal(st.scale.cpu(), s_ref) and torch.equal(st.inv_scale.cpu(), i_ref), t
        assert torch.equal(st.hist.cpu(), hist) and st.amax.cpu().tolist() == [0, 0]
        seen.append(s_ref.tolist())
    assert seen[3][0] == seen[0][0] and seen[4][0] == 8 * seen[3][0]
    assert seen[4][1] == seen[1][1] and seen[5][1] == 256 * seen[4][1]


# ------------------------------------------------------------------ f. NaN / inf policy
def _nan_positions(codes, fmt):
    return set(map(tuple, FR.is_nan_code(codes, fmt).nonzero().tolist()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_cast_fp8_nan_inf_policy(gpu_device, fmt, dtype):
    """NaN -> a NaN code there and nowhere else (index 0, vector body, scalar tail); +-inf -> +-max; amax ignores
    NaN and reports inf, and without an inf it is the largest finite |x|."""
    V = vec_elems(dtype)
    n = 40 * V + V - 1
    x = torch.randn(n, generator=torch.Generator().manual_seed(47)).to(dtype)
    nans = [0, 5 * V + 3, n - 1]
    x[nans] = math.nan
    ref_amax = FR.amax(x)
    got, am = _cast(gpu_device, x, 4.0, fmt)
    assert _nan_positions(got, fmt) == {(i,) for i in nans}
    assert am == ref_amax and math.isfinite(am)
    x[7], x[n - 2] = math.inf, -math.inf
    got, am = _cast(gpu_device, x, 4.0, fmt)
    assert _nan_positions(got, fmt) == {(i,) for i in nans}
    assert got[7] == MAXC[fmt] and got[n - 2] == (0x80 | MAXC[fmt])
    assert am == math.inf
    assert_codes(got, FR.cast(x, 4.0, fmt), fmt, x, "nan / inf")


@pytest.mark.parametrize("N,K", [(64, 128), (128, 128)])  # the 64 x 64 and the 128 x 128 kernel
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_cast_fp8_t_nan_inf_policy(gpu_device, fmt, N, K):
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(53)).to(torch.bfloat16)
    nans = {(0, 0), (3, 70), (N - 1, K - 1)}
    for i, j in nans:
        w[i, j] = math.nan
    w[5, 9], w[N - 2, 1] = math.inf, -math.inf
    w8, w8t, am = _cast_t(gpu_device, w, 4.0, fmt)
    assert _nan_positions(w8, fmt) == nans
    assert _nan_positions(w8t, fmt) == {(j, i) for i, j in nans}
    assert w8[5, 9] == MAXC[fmt] and w8[N - 2, 1] == (0x80 | MAXC[fmt])
    assert_codes(w8, FR.cast(w, 4.0, fmt), fmt, w, "cast_t nan / inf")
    assert torch.equal(w8t, w8.t())
    assert am == math.inf


@pytest.mark.parametrize("M,F", [(64, 64), (128, 128)])
def test_swiglu_cast_t_nan_inf_policy(gpu_device, M, F):
    """A NaN gate poisons its own output only (forward: a; backward: dg and du), a NaN dout both halves of its
    column; an infinite u saturates; amax ignores the NaN and reports the inf."""
    from bpe_transformer.ops.fp8 import swiglu_bwd_cast_t, swiglu_fwd_cast_t

    dev = gpu_device
    gu, da = FR.swiglu_inputs(M, F)
    gu[2, 3] = math.nan           # g
    gu[M - 1, 2 * F - 1] = math.nan  # u
    st = _state(dev, "e4m3", FR.SWIGLU_FWD_SCALE)
    a8, a8t = swiglu_fwd_cast_t(st, gu.to(dev), 0)
    assert _nan_positions(_u8(a8), "e4m3") == {(2, 3), (M - 1, F - 1)}
    assert _nan_positions(_u8(a8t), "e4m3") == {(3, 2), (F - 1, M - 1)}
    check_fused(a8, a8t, FR.swiglu_fwd(gu, FR.SWIGLU_FWD_SCALE), st, "e4m3", "swiglu fwd nan")
    assert math.isfinite(_slot_value(st.amax))

    gu[4, F + 6] = math.inf if float(gu[4, 6]) > 0 else -math.inf  # u = +-inf with silu(g) u = +inf
    st = _state(dev, "e4m3", FR.SWIGLU_FWD_SCALE)
    a8, a8t = swiglu_fwd_cast_t(st, gu.to(dev), 0)
    assert _u8(a8)[4, 6] == MAXC["e4m3"] and _slot_value(st.amax) == math.inf
    check_fused(a8, a8t, FR.swiglu_fwd(gu, FR.SWIGLU_FWD_SCALE), st, "e4m3", "swiglu fwd inf")

    gu, da = FR.swiglu_inputs(M, F)
    gu[2, 3] = math.nan
    da[7, 5] = math.nan
    st = _state(dev, "e5m2", FR.SWIGLU_BWD_SCALE)
    g8, g8t = swiglu_bwd_cast_t(st, da.to(dev), gu.to(dev), 0)
    want = {(2, 3), (2, F + 3), (7, 5), (7, F + 5)}
    assert _nan_positions(_u8(g8), "e5m2") == want
    assert _nan_positions(_u8(g8t), "e5m2") == {(j, i) for i, j in want}
    check_fused(g8, g8t, FR.swiglu_bwd(gu, da, FR.SWIGLU_BWD_SCALE), st, "e5m2", "swiglu bwd nan")
    assert math.isfinite(_slot_value(st.amax))


def test_add_rmsnorm_cast_t_nan_inf_policy(gpu_device):
    """A NaN in a row makes that row's statistics NaN: the whole row is NaN codes in both layouts, every other row
    is untouched; an inf gives rstd = 0, so its own element is inf * 0 = NaN and the rest of its row zero; a NaN
    weight poisons its column."""
    M, N = 128, 256
    x, d, w = FR.norm_inputs(M, N)
    x[3, 17] = math.nan
    x[100, 255] = math.inf
    w[9] = math.nan
    what = "add_rmsnorm nan"
    rstd, rstd_ref = _norm_case(gpu_device, x, d, w, what)
    assert torch.equal(torch.isnan(rstd.cpu()), torch.isnan(rstd_ref))
    assert torch.isnan(rstd_ref).nonzero().flatten().tolist() == [3]
    assert float(rstd[100]) == 0.0


@pytest.mark.parametrize("fmt", FR.FMTS)
def test_fp8_state_subnormal_amax_end_to_end(gpu_device, fmt):
    """A tensor whose largest magnitude is 1e-40 (a bf16 subnormal): after update() the scale is finite (2^126),
    and the next cast keeps zeros zero and saturates nothing."""
    from bpe_transformer.ops.fp8 import Fp8State

    st = Fp8State(1, gpu_device, history=4, fmt=fmt)
    x = torch.zeros(2 * 8 + 5, dtype=torch.bfloat16)
    x[1::3] = 1e-40
    x[2::6] = -1e-40
    x[3::6] = -0.0
    xd = x.to(gpu_device)
    st.cast(xd, 0)
    assert _slot_value(st.amax) == FR.amax(x) > 0
    st.update()
    assert st.scale.item() == 2.0 ** 126 and st.inv_scale.item() == 2.0 ** -126
    got = _u8(st.cast(xd, 0))
    assert_codes(got, FR.cast(x, 2.0 ** 126, fmt), fmt, x, "after a subnormal amax")
    zero = f64(x) == 0
    assert bool(((got[zero] & 0x7F) == 0).all())
    assert not bool(((got & 0x7F) == MAXC[fmt]).any()) and not bool(FR.is_nan_code(got, fmt).any())
