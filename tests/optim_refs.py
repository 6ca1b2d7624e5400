"""Plain float64 references, dispatch mirrors and shape tables for the end of the training step: RMSNorm
forward / backward (``csrc/rmsnorm.hip``) and the AdamW, gradient-norm and clip kernels (``csrc/optim.hip``).

Same conventions as ``tests/rowwise_refs.py``: every function takes inputs that are already rounded to the test
dtype, upcast to float64 (``f64``), and is the textbook formula.  ``tests/test_optim_refs.py`` checks each
against torch's float64 autograd / ``torch.optim.AdamW`` (CPU) and asserts that the shape tables reach every
backward kernel instance; ``tests/test_rmsnorm_bwd_gpu.py`` and ``tests/test_optim_kernels_gpu.py`` check the
kernels against them.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from .rowwise_refs import f64, vec_elems  # noqa: F401  (re-exported for the tests)


# ------------------------------------------------------------------ RMSNorm
def rmsnorm(x: Tensor, w: Tensor, eps: float) -> tuple[Tensor, Tensor]:
    """-> (y, rstd): ``rstd = (mean(x^2) + eps)^-1/2`` per row, ``y = x rstd w``."""
    rstd = torch.rsqrt((x * x).mean(dim=-1) + eps)
    return x * rstd.unsqueeze(-1) * w, rstd


def rmsnorm_bwd(dy: Tensor, x: Tensor, w: Tensor, rstd: Tensor, dres: Tensor | None = None):
    """-> (dx, dw, dw_abs) for 2-D ``x``.  ``rstd`` is an input (the backward kernel reads the forward's stored
    fp32 value).  With x_hat = x rstd and g = dy w: ``dx = rstd (g - x_hat mean(g x_hat)) [+ dres]``,
    ``dw = sum_rows dy x_hat``; ``dw_abs[c] = sum_rows |dy x_hat|`` is the scale of dw[c]'s summation error."""
    xh = x * rstd.unsqueeze(-1)
    g = dy * w
    dx = rstd.unsqueeze(-1) * (g - xh * (g * xh).mean(dim=-1, keepdim=True))
    if dres is not None:
        dx = dx + dres
    t = dy * xh
    return dx, t.sum(dim=0), t.abs().sum(dim=0)


RMS_BWD_GRID = 768      # rmsnorm_bwd_grid: min(ceil(M / 4), 768) blocks
RMS_BWD_HW_GRID = 512   # the half-wave kernel's own cap
REJECTED = ("rejected", 0)


def rms_bwd_kernel_for(M: int, N: int, dtype: torch.dtype) -> tuple[str, int]:
    """(kernel, C) that ``rms_bwd_dispatch`` launches for an [M, N] backward: ("wide", C2), ("half_wave", C),
    ("narrow", C), or ``REJECTED`` where the binding raises before any launch."""
    V = vec_elems(dtype)
    if N < V or N % V:
        return REJECTED
    nv = N // V
    if not (nv <= 512 or (nv % 256 == 0 and nv <= 1024)):
        return REJECTED
    if nv >= 256 and nv % 256 == 0:
        return "wide", nv // 256
    if M % 2 == 0 and nv % 32 == 0 and 64 <= nv <= 128:
        return "half_wave", nv // 32
    chunks = (nv + 63) // 64
    return "narrow", next(c for c in (1, 2, 4, 8) if chunks <= c)


def rms_bwd_wide_rpi(C2: int) -> int:
    """Rows a block of the wide kernel holds per iteration."""
    return 2 if C2 == 1 else 1


def rms_bwd_rows_per_round(M: int, N: int, dtype: torch.dtype) -> int:
    """Rows one pass of the launched grid covers; a block's loop runs again for the rows beyond it.  The grid
    depends on M (a quarter of the rows, capped), so the wide kernel, whose blocks hold RPI rows and not 4, loops
    at every M > RPI."""
    kernel, C = rms_bwd_kernel_for(M, N, dtype)
    grid = min((M + 3) // 4, RMS_BWD_GRID)
    if kernel == "wide":
        return grid * rms_bwd_wide_rpi(C)
    if kernel == "half_wave":
        return min(grid, RMS_BWD_HW_GRID) * 8
    assert kernel == "narrow", (kernel, M, N)
    return grid * 4


# every (kernel, C) instance of rms_bwd_dispatch
RMS_BWD_INSTANCES = frozenset(
    [("narrow", c) for c in (1, 2, 4, 8)] + [("half_wave", c) for c in (2, 3, 4)] + [("wide", c) for c in (1, 2, 3, 4)])

# widths as nv = N / V
RMS_NARROW_NVS = (1, 33, 65, 192, 255, 257, 320, 511)   # narrow at any M
RMS_HW_NVS = (64, 96, 128)                              # half-wave at even M, narrow at odd M
RMS_WIDE_NVS = (256, 512, 768, 1024)
RMS_NVS = RMS_NARROW_NVS + RMS_HW_NVS + RMS_WIDE_NVS
RMS_MS = (1, 2, 3, 7, 8)
# (family, nv, M): the smallest M with one full round of the full-size grid plus a ragged remainder
RMS_ROUND_CASES = (("narrow", 65, 3077), ("half_wave", 96, 4098), ("wide_rpi2", 256, 1537), ("wide_rpi1", 512, 769))
# small shapes, one or two per kernel family, for the dres / dw_acc / determinism / special-row tests (the dres and
# dw_acc tests run at RMS_ROUND_CASES too: the prefetched second iteration carries dres as well)
RMS_FAMILY_CASES = (("narrow", 65, 38), ("narrow", 320, 7), ("half_wave", 96, 38), ("wide_rpi2", 256, 38),
                    ("wide_rpi1", 768, 7))
RMS_REJECTED_NVS = (513, 1280)
RMS_EPS = 1e-5


def rms_family(M: int, N: int, dtype: torch.dtype) -> str:
    kernel, C = rms_bwd_kernel_for(M, N, dtype)
    if kernel == "wide":
        return "wide_rpi2" if rms_bwd_wide_rpi(C) == 2 else "wide_rpi1"
    return kernel


def rms_shapes(dtype: torch.dtype) -> list[tuple[int, int]]:
    """Every (M, N) the GPU tests run the backward at."""
    V = vec_elems(dtype)
    out = [(M, nv * V) for nv in RMS_NVS for M in RMS_MS]
    out += [(M, nv * V) for _, nv, M in RMS_ROUND_CASES]
    out += [(M, nv * V) for _, nv, M in RMS_FAMILY_CASES]
    return out


def rms_input(M: int, N: int, dtype: torch.dtype, seed: int = 0):
    """-> (x, w, dy, dres) rounded to ``dtype``."""
    g = torch.Generator().manual_seed(29 + 1000 * seed + 7 * M + N)
    x = torch.randn(M, N, generator=g).to(dtype)
    w = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype)
    dy = torch.randn(M, N, generator=g).to(dtype)
    dres = torch.randn(M, N, generator=g).to(dtype)
    return x, w, dy, dres


RMS_SPECIAL_ROWS = ("scaled", "zero_x_row", "zero_dy_row", "w_zeros_negative")


def rms_special_input(kind: str, M: int, N: int, dtype: torch.dtype):
    """-> (x, w, dy, row): the inputs of ``rms_input`` with one property changed; ``row`` is the affected row
    (None where every row is).  Row scales are powers of two (exact in bf16), |x| stays below 2^10 * 6, so a row's
    fp32 sum of squares stays below N * 2^26: finite."""
    x, w, dy, _ = rms_input(M, N, dtype, seed=1)
    row = None
    if kind == "scaled":
        e = torch.linspace(-10, 10, M).round()
        x = (x.float() * torch.exp2(e).unsqueeze(-1)).to(dtype)
        dy = (dy.float() * torch.exp2(-e.flip(0)).unsqueeze(-1)).to(dtype)
    elif kind == "zero_x_row":
        row = M // 2
        x[row] = 0
    elif kind == "zero_dy_row":
        row = M // 2
        dy[row] = 0
    elif kind == "w_zeros_negative":
        w = w.clone()
        w[::3] = 0
        w[1::3] = -w[1::3]
    else:
        raise KeyError(kind)
    return x, w, dy, row


# ------------------------------------------------------------------ AdamW
def adamw(p: Tensor, m: Tensor, v: Tensor, g: Tensor, lr: float, b1: float, b2: float, eps: float, wd: float,
          step: int, scale: float | None = None, wd_mask: Tensor | None = None):
    """One decoupled-weight-decay Adam step in float64 -> ((p, m, v), (p_abs, m_abs, v_abs)).

    ``wd_mask``: per ELEMENT 0 / 1 (decay applies where 1).  ``*_abs``: the sum of the absolute values of the
    terms each output is formed from -- m: |b1 m| + |(1 - b1) g|; v likewise; p: |p| + |lr wd p| + the update
    with m's two terms taken in absolute value -- the scale an fp32 evaluation's error is relative to."""
    if scale is not None:
        g = g * scale
    wdv = wd if wd_mask is None else wd * wd_mask.to(p.dtype)
    m1 = b1 * m + (1 - b1) * g
    m_abs = (b1 * m).abs() + ((1 - b1) * g).abs()
    v1 = b2 * v + (1 - b2) * g * g
    v_abs = (b2 * v).abs() + (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2_sqrt = math.sqrt(1 - b2 ** step)
    denom = v1.sqrt() / bc2_sqrt + eps
    p1 = p * (1 - lr * wdv) - (lr / bc1) * m1 / denom
    p_abs = p.abs() + (lr * wdv * p).abs() + (lr / bc1) * m_abs / denom
    return (p1, m1, v1), (p_abs, m_abs, v_abs)


ADAMW_SWEEP = 2048 * 256 * 4    # launch_adamw: at most 2048 blocks of 256 threads, 4 elements each
ADAMW_NS = (1, 3, 4, 5, 63, 64, 65, 1027, ADAMW_SWEEP + 4 * 256 + 3)
ADAMW_HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)


def adamw_input(n: int, gdtype: torch.dtype, seed: int = 0):
    """-> fp32 (p, m, v) and the gradient in ``gdtype``."""
    gen = torch.Generator().manual_seed(31 + seed + n)
    p = torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen)
    g = torch.randn(n, generator=gen).to(gdtype)
    return p, m, v, g


FP32_TINY = 2.0 ** -149   # fp32's smallest spacing: an exact result below it (v from |g| = 1e-30) cannot be stored


def adamw_err_ratio(got: Tensor, ref: Tensor, abs_sum: Tensor, tol: float) -> float:
    """max |got - ref| / (tol * abs_sum + FP32_TINY); at most 1 inside the bound, inf for a NaN."""
    r = (f64(got) - ref).abs() / (tol * abs_sum + FP32_TINY)
    return float(r.nan_to_num(nan=float("inf")).max())


ADAMW_EDGE_KINDS = ("zero_grad", "tiny_huge", "first_step")
ADAMW_EDGE_N = 67   # 16 vectors and a 3-element scalar tail


def adamw_edge_input(kind: str, gdtype: torch.dtype):
    """-> (p, m, v, g, step).  ``zero_grad``: g = m = v = 0, p only decays.  ``tiny_huge``: |g| cycles through
    1e-30, 1e15, 1 with both signs (g^2 <= 1e30 stays finite in fp32; (1e-30)^2 underflows to 0, see
    ``FP32_TINY``).  ``first_step``: zero moments, step 1, where m / sqrt(v) = sign(g) and |dp| = lr up to
    eps / |g| and the decay."""
    n = ADAMW_EDGE_N
    p, m, v, g = adamw_input(n, gdtype, seed=5)
    if kind == "zero_grad":
        return p, torch.zeros(n), torch.zeros(n), torch.zeros(n).to(gdtype), 3
    if kind == "tiny_huge":
        mag = torch.tensor([1e-30, 1e15, 1.0, 1e15, 1e-30, 1.0, 1e-30])
        sign = torch.tensor([1.0, -1.0])
        g = (mag.repeat(n // 7 + 1)[:n] * sign.repeat(n // 2 + 1)[:n]).to(gdtype)
        return p, m, v, g, 3
    if kind == "first_step":
        return p, torch.zeros(n), torch.zeros(n), g, 1
    raise KeyError(kind)


def block_mask(n: int, first: int) -> Tensor:
    """One byte per 64 elements, alternating, the first block ``first``."""
    nb = (n + 63) // 64
    return ((torch.arange(nb) + first) % 2).to(torch.uint8)


def expand_mask(mask: Tensor, n: int) -> Tensor:
    return torch.repeat_interleave(mask, 64)[:n]


# ------------------------------------------------------------------ gradient norm / clip
def grad_norm(tensors: list[Tensor], max_norm: float) -> tuple[float, float]:
    """-> (global L2 norm, clip coefficient ``min(1, max / (norm + 1e-6))``); the coefficient is -1, the skip
    sentinel, where the norm is not finite."""
    norm = float(torch.stack([(t * t).sum() for t in tensors]).sum().sqrt())  # inf / NaN propagate
    if not math.isfinite(norm):
        return norm, -1.0
    return norm, min(1.0, max_norm / (norm + 1e-6))


NORM_SWEEP_VECS = 2048 * 256    # S: vectors one sweep of sumsq_partial_kernel's 2048 blocks covers
NORM_NVS = (0, 1, 255, NORM_SWEEP_VECS, NORM_SWEEP_VECS + 1, 2 * NORM_SWEEP_VECS, 2 * NORM_SWEEP_VECS + 1)


def norm_sizes(dtype: torch.dtype) -> list[int]:
    V = vec_elems(dtype)
    return [nv * V + tail for nv in NORM_NVS for tail in (0, V - 1) if nv * V + tail > 0]


_NORM_BASE: dict[torch.dtype, Tensor] = {}


def norm_input(n: int, dtype: torch.dtype) -> Tensor:
    """The first ``n`` elements of one fixed random vector per dtype (built once, never modified)."""
    if dtype not in _NORM_BASE:
        top = max(norm_sizes(dtype))
        _NORM_BASE[dtype] = torch.randn(top, generator=torch.Generator().manual_seed(37)).to(dtype)
    return _NORM_BASE[dtype][:n]
