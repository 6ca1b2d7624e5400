"""RMSNorm forward and backward (``csrc/rmsnorm.hip``) against the float64 references of ``tests/optim_refs.py``,
at every ``(kernel, C)`` instance ``rms_bwd_dispatch`` can launch, in fp32 and bf16, at row counts below and
beyond one round of the grid.

Inputs are built on the CPU with a fixed seed, rounded to the test dtype and copied to the GPU; the reference sees
the same rounded values in float64, and the backward reference is given the forward's stored fp32 ``rstd`` (the
kernel's input).  Every test that checks ``dx`` or ``dw`` first asserts which kernel its shape takes
(``rms_bwd_kernel_for``), so a change to the dispatch fails here instead of silently moving the coverage.

Bounds (``FWD`` = 1e-5, ``BWD`` = 1e-4, ``BF16_ULP`` = 2^-7, as in ``tests/test_rowwise_kernels_gpu.py``):

* ``y``, ``dx``: ``check()``'s bound applied ROW BY ROW -- bf16 per element with the row's floor, fp32 as the
  row's max-abs error over the row's max-abs reference -- so a wrong row of small magnitude is not hidden by a
  large one.  This implies ``check()`` over the whole tensor.
* ``rstd`` (fp32): ``rel < FWD``; per row where rows differ in scale.
* ``dw[c]``: ``|got - ref| <= BWD * dw_abs[c]`` (fp32), plus ``BF16_ULP * |ref|`` for the one rounding of a bf16
  result.  ``dw_abs[c] = sum_rows |dy x_hat|`` is the scale of the fp32 summation error of column c: a row's
  term is added once per thread, threads and blocks combine in trees, so the error is a few dozen fp32 roundings
  of partial sums that never exceed ``dw_abs[c]``.  It is at most ``BWD * max(dw_abs)``.
* exact results (an all-zero ``dy`` row, ``dw`` with and without ``dres``, ``dx`` with and without ``dw_acc``,
  the autograd path against the raw ops, determinism) with ``torch.equal``.
"""

from __future__ import annotations

import pytest
import torch

from bpe_transformer import ops

from . import optim_refs as OR
from .optim_refs import f64
from .test_rowwise_kernels_gpu import BF16_ULP, BWD, FWD, check, rel

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EPS = OR.RMS_EPS
ALL_CASES = OR.RMS_FAMILY_CASES + OR.RMS_ROUND_CASES


def hip():
    return torch.ops.bpe_hip


def check_rows(got: torch.Tensor, ref: torch.Tensor, dtype: torch.dtype, tol32: float, what: str):
    """``check`` with every row judged on its own (see the module docstring)."""
    if dtype != torch.float32:
        check(got, ref, dtype, tol32, what=what)  # per element, floor from the element's row
        return
    g = f64(got)
    assert g.shape == ref.shape and got.dtype == dtype, (what, g.shape, got.dtype)
    r = (g - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-12)
    worst = float(r.nan_to_num(nan=float("inf")).max())
    print(f"{what}: worst row rel {worst:.3e} (< {tol32:g})")
    assert worst < tol32, (what, worst, int(r.argmax()))


def check_dw(got: torch.Tensor, ref: torch.Tensor, dw_abs: torch.Tensor, out_dtype: torch.dtype, what: str):
    g = f64(got)
    assert g.shape == ref.shape and got.dtype == out_dtype, (what, g.shape, got.dtype)
    bound = BWD * dw_abs + (BF16_ULP * ref.abs() if out_dtype == torch.bfloat16 else 0.0)
    err = (g - ref).abs()
    bad = ~(err <= bound)
    print(f"{what}: worst err / bound {float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max()):.3e}")
    assert not bad.any(), (what, int(bad.sum()), int(bad.nonzero()[0]))


def _fwd_bwd(dev, x, w, dy, dres=None, dw_acc=None):
    """The raw ops on CPU inputs -> (y, rstd, dx, dw) on the CPU."""
    xg, wg = x.to(dev), w.to(dev)
    y, rstd = hip().rmsnorm_fwd(xg, wg, EPS)
    dx, dw = hip().rmsnorm_bwd(dy.to(dev), xg, wg, rstd, None if dres is None else dres.to(dev), dw_acc)
    return y.cpu(), rstd.cpu(), dx.cpu(), dw.cpu()


def _case(dev, M, N, dtype, expect, x=None, w=None, dy=None, autograd=True, per_row_rstd=False):
    """Forward and backward at [M, N] against the reference; ``expect`` is the (kernel, C) the shape must take.
    -> (y, rstd, dx, dw, refs)."""
    assert OR.rms_bwd_kernel_for(M, N, dtype) == expect, (M, N, dtype, OR.rms_bwd_kernel_for(M, N, dtype))
    if x is None:
        x, w, dy, _ = OR.rms_input(M, N, dtype)
    y, rstd, dx, dw = _fwd_bwd(dev, x, w, dy)
    xf, wf, dyf = f64(x), f64(w), f64(dy)
    y_ref, rstd_ref = OR.rmsnorm(xf, wf, EPS)
    what = f"{expect} M={M} N={N}"
    assert rstd.dtype == torch.float32 and rstd.shape == (M,)
    if per_row_rstd:
        assert float(((f64(rstd) - rstd_ref).abs() / rstd_ref).max()) < FWD, what
    else:
        assert rel(rstd, rstd_ref) < FWD, what
    check_rows(y, y_ref, dtype, FWD, what + " y")
    dx_ref, dw_ref, dw_abs = OR.rmsnorm_bwd(dyf, xf, wf, f64(rstd))
    check_rows(dx, dx_ref, dtype, BWD, what + " dx")
    check_dw(dw, dw_ref, dw_abs, dtype, what + " dw")
    if autograd:  # ops.rmsnorm runs the same two kernels: bitwise the same results
        xa, wa = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
        ya = ops.rmsnorm(xa, wa, EPS)
        ya.backward(dy.to(dev))
        assert torch.equal(ya.detach().cpu(), y) and torch.equal(xa.grad.cpu(), dx) and torch.equal(wa.grad.cpu(), dw)
    return y, rstd, dx, dw, (dx_ref, dw_ref, dw_abs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nv", OR.RMS_NVS)
def test_rmsnorm_widths(gpu_device, nv, dtype):
    """M = 1, 2, 3, 7, 8 at every width: one vector, partial waves (33), whole waves +- 1 vector, every chunk
    count of the narrow kernel (C = 8 at nv 257 / 320 / 511), the half-wave kernel at even M and the narrow one
    at odd M of the same widths, every wide instance (C2 = 3 at nv 768)."""
    N = nv * OR.vec_elems(dtype)
    for M in OR.RMS_MS:
        if nv in OR.RMS_WIDE_NVS:
            expect = ("wide", nv // 256)
        elif nv in OR.RMS_HW_NVS and M % 2 == 0:
            expect = ("half_wave", nv // 32)
        else:
            expect = ("narrow", next(c for c in (1, 2, 4, 8) if (nv + 63) // 64 <= c))
        _case(gpu_device, M, N, dtype, expect)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,nv,M", OR.RMS_ROUND_CASES)
def test_rmsnorm_beyond_one_round(gpu_device, family, nv, M, dtype):
    """One full round of the full-size grid plus a ragged remainder: the prefetched second iteration of the
    narrow and half-wave kernels, the wide kernels' row-group loop with a partial last group."""
    N = nv * OR.vec_elems(dtype)
    assert OR.rms_family(M, N, dtype) == family and M > OR.rms_bwd_rows_per_round(M, N, dtype)
    _case(gpu_device, M, N, dtype, OR.rms_bwd_kernel_for(M, N, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,nv,M", ALL_CASES)
def test_rmsnorm_bwd_dres(gpu_device, family, nv, M, dtype):
    """The fused residual-branch gradient: dx = reference + dres in float64, rounded once; dw bitwise as without."""
    N = nv * OR.vec_elems(dtype)
    assert OR.rms_family(M, N, dtype) == family
    x, w, dy, dres = OR.rms_input(M, N, dtype)
    _, rstd, dx0, dw0 = _fwd_bwd(gpu_device, x, w, dy)
    _, _, dx1, dw1 = _fwd_bwd(gpu_device, x, w, dy, dres)
    assert torch.equal(dw1, dw0)
    dx_ref, _, _ = OR.rmsnorm_bwd(f64(dy), f64(x), f64(w), f64(rstd), f64(dres))
    check_rows(dx1, dx_ref, dtype, BWD, f"{family} dx + dres")
    assert not torch.equal(dx1, dx0)


@pytest.mark.parametrize("slot_dtype", DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,nv,M", ALL_CASES)
def test_rmsnorm_bwd_dw_acc(gpu_device, family, nv, M, dtype, slot_dtype):
    """dw added into a gradient slot: slot_before + dw in float64 under the slot dtype's bound (the fp32 slot
    gets the unrounded column sums, for a bf16 activation too); nothing returned; dx bitwise unchanged."""
    dev = gpu_device
    N = nv * OR.vec_elems(dtype)
    assert OR.rms_family(M, N, dtype) == family
    x, w, dy, dres = OR.rms_input(M, N, dtype)
    _, rstd, dx0, _ = _fwd_bwd(dev, x, w, dy, dres)
    before = torch.randn(N, generator=torch.Generator().manual_seed(41)).to(slot_dtype)
    slot = before.to(dev)
    _, _, dx1, dw1 = _fwd_bwd(dev, x, w, dy, dres, slot)
    assert dw1.numel() == 0 and torch.equal(dx1, dx0)
    _, dw_ref, dw_abs = OR.rmsnorm_bwd(f64(dy), f64(x), f64(w), f64(rstd))
    check_dw(slot.cpu(), f64(before) + dw_ref, dw_abs, slot_dtype, f"{family} slot")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", OR.RMS_SPECIAL_ROWS)
@pytest.mark.parametrize("family,nv,M", OR.RMS_FAMILY_CASES)
def test_rmsnorm_special_rows(gpu_device, family, nv, M, kind, dtype):
    """Rows scaled by 2^-10 ... 2^10 in one tensor (each row judged on its own), an all-zero x row
    (rstd = eps^-1/2, dx = rstd dy w), an all-zero dy row (dx exactly 0, nothing added to dw), w with zeros and
    negative entries.  |x| < 2^13, so a row's fp32 sum of squares stays finite (below N * 2^26)."""
    N = nv * OR.vec_elems(dtype)
    assert OR.rms_family(M, N, dtype) == family
    x, w, dy, row = OR.rms_special_input(kind, M, N, dtype)
    assert float(x.float().abs().max()) < 2.0 ** 13
    expect = OR.rms_bwd_kernel_for(M, N, dtype)
    y, rstd, dx, dw, (dx_ref, dw_ref, dw_abs) = _case(gpu_device, M, N, dtype, expect, x, w, dy, autograd=False,
                                                     per_row_rstd=True)
    if kind == "zero_x_row":
        assert abs(float(rstd[row]) - EPS ** -0.5) < FWD * EPS ** -0.5
        assert torch.equal(y[row], torch.zeros(N, dtype=dtype))
        check_rows(dx[row:row + 1], (f64(rstd)[row] * f64(dy)[row] * f64(w)).unsqueeze(0), dtype, BWD, "zero x row")
    elif kind == "zero_dy_row":
        assert torch.equal(dx[row], torch.zeros(N, dtype=dtype))
        keep = torch.arange(M) != row
        # the row adds exact zeros: dw equals the reference without the row under the same bound
        _, dw_wo, dw_abs_wo = OR.rmsnorm_bwd(f64(dy)[keep], f64(x)[keep], f64(w), f64(rstd)[keep])
        check_dw(dw, dw_wo, dw_abs_wo, dtype, "dw without the zero row")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,nv,M", ALL_CASES)
def test_rmsnorm_bwd_deterministic(gpu_device, family, nv, M, dtype):
    N = nv * OR.vec_elems(dtype)
    assert OR.rms_family(M, N, dtype) == family
    x, w, dy, dres = OR.rms_input(M, N, dtype)
    a = _fwd_bwd(gpu_device, x, w, dy, dres)
    b = _fwd_bwd(gpu_device, x, w, dy, dres)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


# ------------------------------------------------------------------ the binding's checks (host side, no launch)
def _valid(dev, dtype, M=4, nv=64):
    N = nv * OR.vec_elems(dtype)
    x, w, dy, _ = OR.rms_input(M, N, dtype)
    return dy.to(dev), x.to(dev), w.to(dev), torch.ones(M, device=dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nv", OR.RMS_REJECTED_NVS)
def test_rmsnorm_bwd_rejects_unsupported_widths(gpu_device, nv, dtype):
    """nv = 513 (more than 8 chunks, no multiple of 256) and nv = 1280 (beyond the wide kernel): the binding
    raises before any launch."""
    assert OR.rms_bwd_kernel_for(4, nv * OR.vec_elems(dtype), dtype) == OR.REJECTED
    dy, x, w, rstd = _valid(gpu_device, dtype, nv=nv)
    with pytest.raises(RuntimeError, match="hidden size too large"):
        hip().rmsnorm_bwd(dy, x, w, rstd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_bwd_argument_checks(gpu_device, dtype):
    dev = gpu_device
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    dy, x, w, rstd = _valid(dev, dtype)
    M, N = x.shape
    hip().rmsnorm_bwd(dy, x, w, rstd)  # the valid call
    with pytest.raises(RuntimeError, match="multiple of 8"):  # N % vec_elems
        hip().rmsnorm_bwd(dy[:, :N - 1].contiguous(), x[:, :N - 1].contiguous(), w[:N - 1].contiguous(), rstd)
    with pytest.raises(RuntimeError, match="contiguous"):  # x strided
        hip().rmsnorm_bwd(dy, torch.cat((x, x), 1)[:, :N], w, rstd)
    with pytest.raises(RuntimeError, match="dy and x sizes differ"):
        hip().rmsnorm_bwd(dy[:M - 1], x, w, rstd)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        hip().rmsnorm_bwd(dy.to(other), x, w, rstd)
    with pytest.raises(RuntimeError, match="weight must be"):  # w.numel() != N
        hip().rmsnorm_bwd(dy, x, torch.cat((w, w)), rstd)
    with pytest.raises(RuntimeError, match="weight must be"):  # w.dtype != x.dtype
        hip().rmsnorm_bwd(dy, x, w.to(other), rstd)
    with pytest.raises(RuntimeError, match="rstd must be"):  # rstd.numel() != M
        hip().rmsnorm_bwd(dy, x, w, rstd[:M - 1])
    with pytest.raises(RuntimeError, match="rstd must be"):  # rstd not fp32
        hip().rmsnorm_bwd(dy, x, w, rstd.to(torch.bfloat16))
