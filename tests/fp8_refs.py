"""Plain references and input builders for the fp8 training path: the casts of ``csrc/fp8.hip`` (``pack4_fp8`` in
``csrc/common.h``), ``update_scales`` and the operand decode of the fp8 GEMMs (``csrc/gemm_pp.hip``, F8).

Nothing here touches a GPU, a kernel or a torch float8 dtype: the code values come from the OCP bit fields, the
rounding is a search over the sorted code values in float64, and the fused casts reuse the float64 formulas of
``tests/rowwise_refs.py``.  ``tests/test_fp8_refs.py`` checks all of it against torch's CPU float8 conversion and
guards the builders' invariants; ``tests/test_fp8_edges_gpu.py`` checks the kernels against it.

The contract the references state (and the kernels are held to):

* ``cast``: ``quantize(fl32(x * scale))`` -- the product rounded to fp32 once, then ONE saturating
  round-to-nearest-even onto the finite codes.  +-inf and everything out of range give +-max, NaN gives a NaN
  code, -0.0 keeps its sign.  ``amax`` is max |x| over the non-NaN inputs (+inf counts).
* ``update_scales``: ``scale = 2^floor(log2(fl32(fmax / fl32(m margin))))`` clamped to [2^-126, 2^126], so that
  scale and 1 / scale are normal fp32 numbers for every positive finite window maximum ``m`` (subnormals
  included); ``scale = 1`` when ``m`` is 0 or not finite.
* the fused casts (SwiGLU forward / backward, add + RMSNorm) round their fp32 result to bf16, multiply by the
  scale in fp32 and convert.  Their fp32 arithmetic can move a value across a bf16 rounding midpoint, so the
  reference is an interval: the codes of the value moved down and up by the kernel's error bound (``DELTA_*``
  below, each derived from that kernel's operation count, never from kernel output).  For almost every element
  both ends give the same code.
"""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import rowwise_refs as RR
from .rowwise_refs import f64

FMTS = ("e4m3", "e5m2")
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
_BITS = {"e4m3": (4, 3, 7), "e5m2": (5, 2, 15)}  # exponent bits, mantissa bits, bias
NAN_CODE = 0x7F  # e4m3fn: S.1111.111; e5m2: S.11111.11 -- a NaN in both formats
U = 2.0 ** -24  # relative error bound of one fp32 rounding (half an ulp)


# ------------------------------------------------------------------ decode tables
def decode(fmt: str) -> Tensor:
    """float64 [256]: the value of every code, from the bit fields.  e4m3fn has no infinities and one NaN mantissa
    (S.1111.111); e5m2 is IEEE-like (exponent 31: inf for mantissa 0, else NaN)."""
    eb, mb, bias = _BITS[fmt]
    out = []
    for code in range(256):
        sign = -1.0 if code & 0x80 else 1.0
        e = (code >> mb) & ((1 << eb) - 1)
        m = code & ((1 << mb) - 1)
        if fmt == "e4m3" and e == 15 and m == 7:
            v = math.nan
        elif fmt == "e5m2" and e == 31:
            v = math.inf if m == 0 else math.nan
        elif e == 0:
            v = m / (1 << mb) * 2.0 ** (1 - bias)
        else:
            v = (1.0 + m / (1 << mb)) * 2.0 ** (e - bias)
        out.append(sign * v)
    return torch.tensor(out, dtype=torch.float64)


def positive_codes(fmt: str) -> Tensor:
    """float64: the finite non-negative code values in code order 0 .. max (ascending in value)."""
    return decode(fmt)[: (0x7F if fmt == "e4m3" else 0x7C)]


def is_nan_code(codes: Tensor, fmt: str) -> Tensor:
    c = codes.to(torch.int32)
    if fmt == "e4m3":
        return (c & 0x7F) == 0x7F
    return ((c & 0x7C) == 0x7C) & ((c & 0x03) != 0)


def same_codes(got: Tensor, ref: Tensor, fmt: str) -> Tensor:
    """Elementwise: equal bytes, or both a NaN code (the formats have several; which one is not part of the
    contract)."""
    return (got == ref) | (is_nan_code(got, fmt) & is_nan_code(ref, fmt))


# ------------------------------------------------------------------ quantize / cast
def quantize(x64: Tensor, fmt: str) -> Tensor:
    """uint8 codes: saturating round-to-nearest-even of float64 values onto the finite codes, as a search over the
    decode table.  The two distances are exact in float64 whenever ``x64`` holds fp32 values and the neighbours
    are within 2^29 of each other; next to zero the larger distance is rounded, which cannot create a false tie
    (a tie there needs |x| = half the smallest subnormal exactly, and then both distances are exact)."""
    pos = positive_codes(fmt)
    a = x64.abs().clamp(max=FMAX[fmt])  # inf and out of range -> max
    nan = torch.isnan(x64)
    a = torch.where(nan, torch.zeros_like(a), a)
    hi = torch.bucketize(a, pos).clamp(max=pos.numel() - 1)  # first code value >= a
    lo = (hi - 1).clamp(min=0)
    d_lo, d_hi = a - pos[lo], pos[hi] - a
    even = torch.where(lo % 2 == 0, lo, hi)  # the mantissa's last bit is the code's last bit
    code = torch.where(d_lo < d_hi, lo, torch.where(d_hi < d_lo, hi, even))
    code = code | torch.where(torch.signbit(x64), 0x80, 0)
    return torch.where(nan, torch.full_like(code, NAN_CODE), code).to(torch.uint8)


def fl32(x64: Tensor) -> Tensor:
    """float64 -> nearest fp32 (one rounding, subnormals kept), back in float64."""
    return x64.to(torch.float32).to(torch.float64)


def scale32(scale: float) -> float:
    """The fp32 value a kernel reads for ``scale``."""
    return float(np.float32(scale))


def cast(x: Tensor, scale: float, fmt: str) -> Tensor:
    """The cast kernels' contract on inputs already rounded to their dtype: uint8 codes of
    ``quantize(fl32(x * scale))``.  x and scale are fp32 values, so the float64 product is exact and ``fl32`` is the
    single rounding of the kernel's fp32 multiply."""
    return quantize(fl32(f64(x) * scale32(scale)), fmt)


def amax(x: Tensor) -> float:
    """max |x| over the non-NaN elements (+inf counts); 0 for none."""
    a = f64(x).abs().flatten()
    a = a[~torch.isnan(a)]
    return float(a.max()) if a.numel() else 0.0


# ------------------------------------------------------------------ update_scales
MAX_SCALE_EXP = 126  # scale and 1 / scale both normal fp32


def update_scales(amax_cur: Tensor, hist: Tensor, pos: int, margin: float, fmt: str):
    """One ``update_scales`` step.  amax_cur fp32 [n], hist fp32 [n, H] -> (scale, inv_scale, hist, amax) as fp32
    tensors, ``amax`` zeroed.  Ring write at ``pos % H``, window max m, ``q = fl32(fmax / fl32(m margin))`` in
    numpy fp32 arithmetic, ``scale = 2^floor(log2 q)`` from ``math.frexp`` (exact), clamped to
    [2^-126, 2^126]: q = inf (subnormal m) gives 2^126, q = 0 (m margin overflows) 2^-126."""
    n, H = hist.shape
    hist = hist.clone()
    hist[:, pos % H] = amax_cur
    scale = torch.ones(n, dtype=torch.float32)
    inv = torch.ones(n, dtype=torch.float32)
    fm, mg = np.float32(FMAX[fmt]), np.float32(margin)
    for i in range(n):
        row = hist[i].numpy()
        m = np.float32(0.0)
        for v in row:  # fmaxf: a NaN entry is ignored
            if v > m:
                m = v
        if not (m > 0 and np.isfinite(m)):
            continue
        with np.errstate(over="ignore", divide="ignore"):
            q = float(fm / np.float32(m * mg))
        if math.isinf(q):
            e = MAX_SCALE_EXP
        elif q == 0.0:
            e = -MAX_SCALE_EXP
        else:
            e = min(max(math.frexp(q)[1] - 1, -MAX_SCALE_EXP), MAX_SCALE_EXP)  # q = f 2^k, f in [0.5, 1)
        scale[i] = 2.0 ** e
        inv[i] = 2.0 ** -e
    return scale, inv, hist, torch.zeros(n, dtype=torch.float32)


def scale_cases(fmt: str) -> torch.Tensor:
    """fp32 amax values: fmax 2^-k for k = -20 .. 20 (the quotient is exactly a power of two at margin 1) with the
    fp32 neighbour on either side of each; inf; 1e-40 and the smallest fp32 subnormal; 0; the largest fp32."""
    base = torch.tensor([FMAX[fmt] * 2.0 ** -k for k in range(-20, 21)], dtype=torch.float32)
    below = (base.view(torch.int32) - 1).view(torch.float32)
    above = (base.view(torch.int32) + 1).view(torch.float32)
    extra = torch.tensor([math.inf, 1e-40, 2.0 ** -149, 0.0, 3.4028234663852886e38], dtype=torch.float32)
    return torch.cat((base, below, above, extra))


# ------------------------------------------------------------------ fused casts (float64, accept intervals)
def round_bf16(v64: Tensor) -> Tensor:
    """float64 -> nearest bf16 in ONE round-to-nearest-even (torch's own float64 -> bfloat16 goes through fp32,
    two roundings), returned in float64.  8 significant bits, quantum 2^-133 below the normal range, overflow to
    inf past the last finite value's rounding boundary."""
    finite = torch.isfinite(v64)
    v = torch.where(finite, v64, torch.zeros_like(v64))
    _, e = torch.frexp(v)  # v = f 2^e, 0.5 <= |f| < 1
    quantum = torch.ldexp(torch.ones_like(v), e.clamp(min=-125) - 8)
    r = torch.round(v / quantum) * quantum  # exact scaling, half-to-even
    r = torch.where(r.abs() > 3.3895313892515355e38, torch.copysign(torch.full_like(r, math.inf), r), r)
    return torch.where(finite, r, v64)


G_MIN = -16.0
"""The DELTA_* bounds below hold for gate inputs g >= G_MIN: the sigmoid's exponent argument t = -g log2(e) is
formed in fp32 with two half-ulp errors (the rounded constant and the product), so 2^t inherits a relative error
of ln2 * 2U * |t|, which for the sigmoid matters when 2^t dominates 1 + 2^t (g < 0) and grows with |g|.  For
g < G_MIN |silu(g)| < 2e-6; ``tests/test_fp8_refs.py`` asserts that on the GPU tests' inputs those elements give
the zero code even with a 50 % error, so no bound is needed there."""

_SIG = math.log(2.0) * 2 * 16 * math.log2(math.e) + 2 + 1 + 2  # = 32 + 5 -> 37
DELTA_SIGMOID = 37 * U
"""fast_sigmoid(g) = rcp(1 + exp2(g * -log2 e)) for g >= G_MIN, relative: the argument error through exp2,
ln2 * 2U * |t| <= ln2 * 2U * 16 log2(e) = 32 U; v_exp_f32 1 ulp = 2U; the add U; v_rcp_f32 1 ulp = 2U."""
assert abs(_SIG - 37) < 1e-9

DELTA_SWIGLU_FWD = 39 * U
"""a = (g * sg) * u: DELTA_SIGMOID + two multiplies (U each) = 39 U = 2^-18.7, relative to |a|."""

DELTA_SWIGLU_BWD = 42 * U
"""du = d * (g * sg): 37 U + 2 U = 39 U relative to |du|.
dg = ((d * u) * sg) * Q, Q = 1 + g * (1 - sg).  P = (d u) sg carries 2U + 37U = 39 U.  Q's absolute error is at
most |g| sg 37U (sg's error through the subtraction) + |g (1 - sg)| 2U (the subtraction and the product) + |Q| U
(the add, or nothing when the compiler fuses it).  With the last multiply (U):
|error(dg)| <= |P| (|Q| 41U + |g| sg 37U + |g (1 - sg)| 2U) <= 41U * A, A = |P| (|Q| + |g| sg + |g (1 - sg)|);
one more U covers the second-order terms.  A equals |dg| up to a small factor except next to the zero of silu'
(g = -1.278), where 1 and g (1 - sg) cancel and only the absolute bound is meaningful.  The reference applies
42 U * A to both halves (A = |du| for du)."""

DELTA_ADD_RMSNORM = 25 * U
"""y = (s * rstd) * w at the kernel's widest row, N = 2048.  The sum of squares has only positive terms, so its
relative error is at most (adds on the longest path + 1 product rounding) U: a lane adds its N / 64 = 32 squares
in turn, the wave reduction adds 6 levels -> 39 U.  ss / N and + eps: U each -> 41 U; through the inverse square
root half of that, 20.5 U, plus v_rsq_f32's 1 ulp = 2U -> 22.5 U; two multiplies -> 24.5 U, rounded up."""


class Accept(NamedTuple):
    """What a fused cast may write: per element the codes of the two ends of its error interval and whether the
    zero code is accepted as well; for the recorded amax (max |bf16 value|) the maxima over the ends nearer to
    and farther from zero."""
    lo: Tensor
    hi: Tensor
    tiny: Tensor
    amax_lo: float
    amax_hi: float


def _candidates(v: Tensor, err: Tensor, scale: float, fmt: str) -> Accept:
    """The fused cast whose fp32 value lies in [v - err, v + err]: each end rounded to bf16, then ``cast``.
    ``tiny``: |v| is below the fp32 normal range, where the kernel's fp32 value may be flushed or lose bits."""
    moved = (err > 0) & torch.isfinite(v)  # v + 0 would turn a -0 into +0, inf - inf an infinite v into NaN
    err = torch.where(moved, err, torch.zeros_like(v))
    lo, hi = round_bf16(torch.where(moved, v - err, v)), round_bf16(torch.where(moved, v + err, v))
    near = round_bf16((v.abs() - err).clamp(min=0.0))
    far = round_bf16(v.abs() + err)
    return Accept(cast(lo, scale, fmt), cast(hi, scale, fmt), v.abs() < 2.0 ** -126, amax(near), amax(far))


def in_accept(got: Tensor, acc: Accept, fmt: str) -> Tensor:
    """Elementwise: ``got`` (uint8 codes) decodes to a value between the two candidates' (the cast is monotone, so
    every value in the error interval lands there; the candidates are equal or adjacent except where a bound is
    absolute and spans zero), either zero counting as zero; a NaN candidate needs a NaN code."""
    lo, hi, tiny = acc.lo, acc.hi, acc.tiny
    tab = decode(fmt)
    g, a, b = tab[got.long()], tab[lo.long()], tab[hi.long()]
    nan_ref = is_nan_code(lo, fmt) | is_nan_code(hi, fmt)
    ok = (g >= torch.minimum(a, b)) & (g <= torch.maximum(a, b))
    ok = ok | (tiny & ((got & 0x7F) == 0))
    return torch.where(nan_ref, is_nan_code(got, fmt), ok & ~is_nan_code(got, fmt))


def swiglu_fwd(gu: Tensor, scale: float, fmt: str = "e4m3", delta: float = DELTA_SWIGLU_FWD):
    """Accept interval of ``swiglu_fwd_cast_t``: a = silu(g) u."""
    v = RR.swiglu(f64(gu))
    return _candidates(v, delta * v.abs(), scale, fmt)


def swiglu_bwd(gu: Tensor, dout: Tensor, scale: float, fmt: str = "e5m2", delta: float = DELTA_SWIGLU_BWD):
    """Accept interval of ``swiglu_bwd_cast_t``: [dg | du]; the error scale A of DELTA_SWIGLU_BWD."""
    gu64, d = f64(gu), f64(dout)
    F = gu64.shape[-1] // 2
    g, u = gu64[..., :F], gu64[..., F:]
    v = RR.swiglu_bwd(gu64, d)
    sg = 1.0 / (1.0 + torch.exp(-g))
    q_parts = (1.0 + g * (1.0 - sg)).abs() + g.abs() * sg + (g * (1.0 - sg)).abs()
    a_dg = (d * u * sg).abs() * q_parts
    scale_a = torch.cat((a_dg, v[..., F:].abs()), dim=-1)
    scale_a = torch.where(torch.isnan(v), v, scale_a.nan_to_num(nan=0.0, posinf=math.inf))
    return _candidates(v, delta * scale_a, scale, fmt)


def add_rmsnorm(x: Tensor, d: Tensor | None, w: Tensor, eps: float, scale: float, fmt: str = "e4m3",
                delta: float = DELTA_ADD_RMSNORM):
    """``add_rmsnorm_cast_t``: -> (sum float64 (exact bf16 values), rstd float64, Accept)."""
    x64 = f64(x)
    d64 = torch.zeros_like(x64) if d is None else f64(d)
    s, y, rstd = RR.add_rmsnorm(x64, d64, f64(w), eps, torch.bfloat16)
    return s, rstd, _candidates(y, delta * y.abs(), scale, fmt)


# ------------------------------------------------------------------ input builders
def _to_dtype(v64: Tensor, dtype: torch.dtype) -> Tensor:
    """float64 -> dtype with one rounding."""
    if dtype == torch.bfloat16:
        return round_bf16(v64).to(torch.float32).to(torch.bfloat16)
    return v64.to(dtype)


def _step(x: Tensor, k: int) -> Tensor:
    """The value ``k`` places up (k > 0) or down the positive tensor ``x``'s own dtype."""
    it = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
    return (x.view(it) + k).view(x.dtype)


def boundary_values(fmt: str, dtype: torch.dtype, nonfinite: bool = True) -> Tensor:
    """The post-scale values (``dtype``) every cast must get right: for each pair of adjacent finite codes the two
    values, their midpoint (a tie) and the midpoint's two ``dtype`` neighbours, in both signs; +-0; +-half the
    smallest subnormal (a tie with zero, to zero); +-max, max plus half and one last-place step (saturate), 1e30;
    with ``nonfinite`` +-inf and NaN."""
    pos = positive_codes(fmt)
    mid = _to_dtype((pos[:-1] + pos[1:]) / 2, dtype)
    assert torch.equal(f64(mid), (pos[:-1] + pos[1:]) / 2), "a midpoint is not representable"
    step = float(pos[-1] - pos[-2])
    top = torch.tensor([FMAX[fmt] + step / 2, FMAX[fmt] + step, 1e30], dtype=torch.float64)
    mag = torch.cat((_to_dtype(pos, dtype), mid, _step(mid, -1), _step(mid, 1), _to_dtype(top, dtype)))
    vals = torch.cat((mag, -mag))
    if nonfinite:
        vals = torch.cat((vals, torch.tensor([math.inf, -math.inf, math.nan]).to(dtype)))
    return vals


def boundary_inputs(fmt: str, dtype: torch.dtype, scale: float = 1.0, nonfinite: bool = True) -> Tensor:
    """1-D CPU tensor of ``dtype``: ``boundary_values`` divided by ``scale`` (exact for a power of two, so the kernel's
    product is the boundary value itself; rounded to ``dtype`` otherwise), in a fixed shuffled order.  Laid out
    for ``cast_fp8``'s three paths: index 0 holds a special value, the body the whole set, and the length is
    ``k V + V - 1`` (odd; V = elements per 16-byte vector) with the scalar tail holding special values again: NaN /
    inf where ``nonfinite``, ties to zero, the saturating half step, -0."""
    V = RR.vec_elems(dtype)
    vals = boundary_values(fmt, dtype, nonfinite)
    vals = vals[torch.randperm(vals.numel(), generator=torch.Generator().manual_seed(29))]
    half_sub = float(positive_codes(fmt)[1]) / 2
    step = float(positive_codes(fmt)[-1] - positive_codes(fmt)[-2])
    sp = [math.nan, -math.inf, -half_sub, math.inf, FMAX[fmt] + step / 2, -0.0, half_sub]
    if not nonfinite:
        sp = [-FMAX[fmt], -1e30, -half_sub, 1e30, FMAX[fmt] + step / 2, -0.0, half_sub]
    special = torch.tensor(sp, dtype=torch.float64).to(dtype)
    pad = (-(1 + vals.numel())) % V
    x = torch.cat((special[:1], vals, torch.ones(pad, dtype=dtype), special[: V - 1]))
    assert x.numel() % 2 == 1 and x.numel() % V == V - 1
    return _to_dtype(f64(x) / scale32(scale), dtype)


def tiled_boundary_matrix(fmt: str, rows: int, cols: int, scale: float, nonfinite: bool = False) -> Tensor:
    """bf16 [rows, cols]: ``boundary_inputs`` repeated along the flattened matrix.  Its length is odd, so the copies
    drift against the 64- and 128-wide tiles and every tile row and column position meets ties.  Subnormals are
    only ~5 % of the set, so row r also gets a tie between two subnormal codes (or with zero) at column 5 r mod
    cols, alternating in sign: every tile row and, 5 being odd, every tile column position holds one."""
    v = boundary_inputs(fmt, torch.bfloat16, scale, nonfinite)
    n = rows * cols
    w = v.repeat(-(-n // v.numel()))[:n].reshape(rows, cols).clone()
    pos = positive_codes(fmt)
    r = torch.arange(rows)
    tie = (pos[r % 3] + pos[r % 3 + 1]) / 2 * torch.where(r % 2 == 0, 1.0, -1.0)
    w[r, (5 * r) % cols] = _to_dtype(tie / scale32(scale), torch.bfloat16)
    return w.contiguous()


def cast_scales() -> tuple[float, ...]:
    return (1.0, 2.0 ** -3, 2.0 ** 7, 0.37)


# fused-cast cases: name -> (shapes, scale, fmt)
SWIGLU_SHAPES = ((64, 64), (128, 128), (192, 128))  # (M, F): 64 x 64 kernel, 128 x 128 kernel, 64 x 64 kernel
NORM_SHAPES = ((128, 128), (128, 2048), (256, 384))
SWIGLU_FWD_SCALE = 32.0
SWIGLU_BWD_SCALE = 2.0 ** 21
NORM_SCALE = 128.0
EDGE_SCALE = 8.0       # swiglu_edge_inputs, forward
EDGE_BWD_SCALE = 1.0   # ... backward: the g = -20 row stays below half the smallest e5m2 subnormal (G_MIN)


def swiglu_inputs(M: int, F: int) -> tuple[Tensor, Tensor]:
    """(gu [M, 2F], dout [M, F]) bf16: random, with column 0 of u (and of dout) enlarged so that outputs
    saturate at the test scales and column 1 shrunk so that outputs fall in the fp8 subnormal range."""
    g = torch.Generator().manual_seed(31 + M + F)
    gu = 2.0 * torch.randn(M, 2 * F, generator=g)
    dout = 0.01 * torch.randn(M, F, generator=g)
    gu[:, F] *= 8.0             # u only: g stays above G_MIN
    dout[:, 0] *= 4.0
    gu[:, F + 1] *= 2.0 ** -9   # a = silu(g) u small
    dout[:, 1] *= 2.0 ** -31    # dg, du small
    return gu.to(torch.bfloat16), dout.to(torch.bfloat16)


def swiglu_edge_inputs() -> tuple[Tensor, Tensor]:
    """The activation edge rows (0 / -0, 1e-30, 1, 20, 88, 1e4, alternating signs) as g and as u, repeated to a
    (64, 64) tile: row i of the tile holds edge row i % 6, u mirrored in odd tile rows so that both sign pairings
    occur; dout = +-1 and +-2^-10."""
    e = RR.act_edge_input(torch.bfloat16)  # [6, 16]
    g = e.repeat(11, 4)[:64]
    u = g.clone()
    u[1::2] = u[1::2].flip(1)
    dout = torch.ones(64, 64)
    dout[:, 1::2] = -(2.0 ** -10)
    return torch.cat((g, u), dim=1).contiguous(), dout.to(torch.bfloat16)


def norm_inputs(M: int, N: int) -> tuple[Tensor, Tensor, Tensor]:
    """(x, d, w) bf16 as ``rowwise_refs.add_rmsnorm_input``, with w[0] enlarged (column 0 saturates at NORM_SCALE)
    and w[1] shrunk (column 1 falls in the e4m3 subnormal range)."""
    x, d, w = RR.add_rmsnorm_input(M, N, torch.bfloat16)
    w = w.clone()
    w[0] = 16.0
    w[1] = 2.0 ** -12
    return x, d, w


# ------------------------------------------------------------------ fp8 GEMM operands
def all_codes_matrix(fmt: str, rows: int, K: int) -> Tensor:
    """uint8 [rows, K]: row i holds code (i + k) % 256 at column k, NaN / inf codes replaced by 0 -- every finite
    code, subnormals and +-max included, in every k position."""
    c = (torch.arange(rows).unsqueeze(1) + torch.arange(K).unsqueeze(0)) % 256
    finite = torch.isfinite(decode(fmt))
    return torch.where(finite[c], c, torch.zeros_like(c)).to(torch.uint8)


def diag_matrix(fmt: str, rows: int, K: int) -> tuple[Tensor, Tensor]:
    """(uint8 codes [rows, K], float64 diagonal [rows]): the identity pattern with entry (-1)^n 2^(n % 3 - 1) at
    (n, n), zeros elsewhere (columns past ``rows`` all zero)."""
    tab = decode(fmt)
    d = torch.tensor([(-1.0) ** n * 2.0 ** (n % 3 - 1) for n in range(rows)], dtype=torch.float64)
    codes = quantize(d, fmt)
    assert torch.equal(tab[codes.long()], d)
    m = torch.zeros(rows, K, dtype=torch.uint8)
    m[torch.arange(rows), torch.arange(rows)] = codes
    return m, d


def window_codes(fmt: str, rows: int, K: int, seed: int) -> Tensor:
    """uint8 [rows, K]: random codes of both signs from three adjacent exponents (values in [1, 8)), every
    mantissa.  Bit budget of a dot product of two such operands: a value has at most 4 significant bits, a product
    8; the products' leading bits span 2^0 .. 2^5, their last bits lie at 2^-6 or above; a sum of K < 2^9 of them
    stays below 2^15 -- 21 bits in all, under fp32's 24, so every partial sum in any order is exact."""
    eb, mb, bias = _BITS[fmt]
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(bias, bias + 3, (rows, K), generator=g)
    m = torch.randint(0, 1 << mb, (rows, K), generator=g)
    s = torch.randint(0, 2, (rows, K), generator=g)
    return ((s << 7) | (e << mb) | m).to(torch.uint8)
