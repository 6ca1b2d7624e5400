"""Plain float64 references and input builders for the bf16 GEMMs (``csrc/gemm.hip``, ``csrc/gemm_pp.hip``) and the
fused epilogues of the ping-pong kernel (QKV + RoPE, SwiGLU forward / backward).  CPU only: nothing here touches a
GPU or a kernel.  ``tests/test_gemm_refs.py`` guards the builders' invariants, ``tests/test_gemm_edges_gpu.py`` holds
the kernels to the references.

The contract the references state:

* plain GEMM: ``C = round_bf16(beta * C + A B^T)`` -- fp32 accumulation, ``beta * C`` added in fp32, ONE rounding to
  bf16 (an fp32 C gets the fp32 sum).  The exact-accumulation operands below are integers small enough that every
  partial sum, in any order, tile schedule or K split, is an integer below 2^24 and therefore exact in fp32; the
  float64 value is then what every correct kernel must produce, bit for bit.
* QKV + RoPE: the product rounded to bf16, then the interleaved-pair rotation evaluated in fp32 and rounded once
  more.  The fp32 evaluation may move a value across a bf16 rounding midpoint, so the reference is an accept set
  (``Accept16``, the bf16 analogue of ``fp8_refs.Accept``: the two ends of the error interval, rounded).
* SwiGLU epilogues: the unfused kernels' contract (``rowwise_refs.swiglu`` / ``swiglu_bwd``) on the bf16-rounded GEMM
  result, with ``fp8_refs``' error bounds.
"""

from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch
from torch import Tensor

from . import fp8_refs as FR
from . import rowwise_refs as RR
from .fp8_refs import U, round_bf16
from .rowwise_refs import f64

LAYOUTS = ((True, True), (True, False), (False, True), (False, False))  # (a_kmajor, b_kmajor)
BETAS = (0.0, 1.0, -0.5, 2.0)
C_MAX = 64
BF16_MAX = 3.3895313892515355e38  # (2 - 2^-7) 2^127
SENTINEL16 = 0x5A5A                 # bf16 bit pattern of the bytes around a view (a finite value)
SENTINEL32 = 0x5A5A5A5A


def to_bf16(v64: Tensor) -> Tensor:
    """float64 -> bf16 tensor with one rounding."""
    return round_bf16(v64).to(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------ A. exact accumulation
def int_amax(R: int) -> int:
    """Largest operand magnitude at reduction length R.  A sum of R products of integers uniform in [-a, a] has a
    standard deviation of sqrt(R) a (a + 1) / 3; a is chosen so that this is about 512 for every R -- most outputs
    then lie in 256 .. 2048, where the bf16 quantum is 2, 4 or 8 and an integer needs rounding (and is an exact tie)
    often.  R = 448 gives 8."""
    return max(2, round(math.sqrt(3 * 508 / math.sqrt(R))))


def exact_bound(R: int) -> int:
    """An upper bound of |beta * C + any partial sum| (times 2, for the half-integers of beta = -0.5)."""
    return 2 * (R * int_amax(R) ** 2 + 2 * C_MAX)


@functools.lru_cache(maxsize=None)
def int_operands(M: int, N: int, R: int, seed: int = 0) -> tuple[Tensor, Tensor]:
    """(A [M, R], B [N, R]) float64 integers in [-a, a], a = int_amax(R): exact in bf16 (|v| <= 256)."""
    a = int_amax(R)
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + M + N)
    A = torch.randint(-a, a + 1, (M, R), generator=g).double()
    B = torch.randint(-a, a + 1, (N, R), generator=g).double()
    return A, B


@functools.lru_cache(maxsize=None)
def int_c(M: int, N: int, seed: int = 0) -> Tensor:
    """C [M, N] float64 integers in [-64, 64]."""
    g = torch.Generator().manual_seed(77 + seed + M + N)
    return torch.randint(-C_MAX, C_MAX + 1, (M, N), generator=g).double()


@functools.lru_cache(maxsize=None)
def int_product(M: int, N: int, R: int, seed: int = 0) -> Tensor:
    A, B = int_operands(M, N, R, seed)
    return A @ B.t()  # integers below 2^24: exact in float64 in any order


def gemm_exact(P: Tensor, C: Tensor | None, beta: float) -> Tensor:
    """beta * C + P in float64 (exact for the inputs above); beta = 0 never reads C."""
    return P if beta == 0.0 or C is None else beta * C + P


@functools.lru_cache(maxsize=None)
def gemm_ref(M: int, N: int, R: int, beta: float, c32: bool, seed: int = 0) -> Tensor:
    """The expected output of the exact-accumulation case, float64: one rounding to bf16, or none (fp32 C)."""
    v = gemm_exact(int_product(M, N, R, seed), int_c(M, N, seed), beta)
    return v if c32 else round_bf16(v)


def store(A: Tensor, kmajor: bool) -> Tensor:
    """The logical [rows, R] float64 operand as the bf16 tensor a kernel reads: [rows, R], or [R, rows] (MN-major)."""
    t = A if kmajor else A.t()
    return to_bf16(t).contiguous()


def rounding_shares(v: Tensor, P: Tensor | None = None, C: Tensor | None = None) -> dict[str, float]:
    """Of the exact results ``v``: the share that is not a bf16 value, that lies exactly between two, that
    truncation would round differently; with P, C (v = P + C) the share where rounding P first differs."""
    r = round_bf16(v)
    _, e = torch.frexp(v)
    q = torch.ldexp(torch.ones_like(v), e - 8)
    trunc = torch.trunc(v / q) * q
    out = {"rounded": float((r != v).double().mean()),
           "ties": float((((v / q) % 1.0).abs() == 0.5).double().mean()),
           "trunc": float((trunc != r).double().mean())}
    if P is not None:
        out["double"] = float((round_bf16(round_bf16(P) + C) != r).double().mean())
    return out


# (R, splits) of the exact-accumulation cases.  K-tile counts per split: 1, 2, 3, 7 and the uneven 2 / 2 / 3.
PP_CASES = ((64, 1), (192, 1), (192, 3), (384, 3), (448, 1), (448, 3), (448, 7))   # 64-wide K-tiles
G128_CASES = ((64, 1), (192, 1), (192, 3), (384, 3), (448, 1), (448, 3))           # 64-wide K-steps
# the 256-tile kernel: 32-wide K-steps and at least NSTAGE - 1 = 3 of them per split, so R = 96 is the smallest
# one-pass size and R = 288 the smallest at three splits; R = 448 splits 14 steps into 4 / 5 / 5
G256_CASES = ((96, 1), (288, 3), (448, 1), (448, 3))
PP_SHAPE = (512, 768)
G128_SHAPE = (256, 384)
G256_SHAPE = (512, 768)


def poison(M: int, N: int, dtype: torch.dtype) -> Tensor:
    """[M, N] of NaN (both signs, quiet and with a payload), +inf and -inf bit patterns."""
    if dtype == torch.bfloat16:
        pats, it = torch.tensor([0x7FC0, 0x7F80, -128, -1, 0x7FA5], dtype=torch.int16), torch.int16  # ff80, ffff
    else:
        pats, it = torch.tensor([0x7FC00000, 0x7F800000, -8388608, -1, 0x7FA55555], dtype=torch.int32), torch.int32
    idx = (torch.arange(M).unsqueeze(1) * 3 + torch.arange(N).unsqueeze(0)) % pats.numel()
    return pats[idx].to(it).view(dtype)


def widen(t: Tensor, off: int, pad: int, fill_bits: int | None = None) -> tuple[Tensor, Tensor]:
    """(parent, view): ``t`` as columns [off, off + width) of a parent ``pad`` columns wider; the rest of the parent
    holds the sentinel bit pattern (or, for an operand, a NaN: reading outside the view would show)."""
    rows, w = t.shape
    it = torch.int16 if t.dtype == torch.bfloat16 else torch.int32
    if fill_bits is None:
        fill_bits = 0x7FC0 if t.dtype == torch.bfloat16 else 0x7FC00000
    parent = torch.full((rows, w + pad), fill_bits, dtype=it).view(t.dtype)
    parent[:, off:off + w] = t
    return parent, parent[:, off:off + w]


# ------------------------------------------------------------------ D. non-finite values and range
def overflow_operands(M: int, N: int, R: int) -> tuple[Tensor, Tensor, Tensor]:
    """(A [M, R], B [N, R], S [M]) float64.  B is 2^57 everywhere, row i of A holds non-negative integers times
    2^57 that sum to S[i] (negated in odd rows), so output (i, j) is +-S[i] 2^114 for every j and every partial sum,
    in any order, is an integer below 2^14 times 2^114: exact and monotone.  The bf16 rounding boundary
    (255.5 2^120) is 16352 2^114: S cycles through 16351 (the largest sum of this grid that rounds down, to the
    last finite bf16), 16352 (the tie: to even, which is inf), 16353, 16383 (the largest below fp32 overflow at
    16384) and 9000 (finite, rounded).  The surplus over R * (S // R) sits at a position that moves with the row."""
    targets = (16351, 16352, 16353, 16383, 9000)
    S = torch.tensor([targets[(i // 2) % len(targets)] for i in range(M)], dtype=torch.float64)
    A = torch.zeros(M, R, dtype=torch.float64)
    for i in range(M):
        base, extra = divmod(int(S[i]), R)
        assert base + 1 <= 256
        row = torch.full((R,), float(base), dtype=torch.float64)
        row[(torch.arange(extra) + 5 * i) % R] += 1.0
        A[i] = row if i % 2 == 0 else -row
    sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).double()
    return A * 2.0 ** 57, torch.full((N, R), 2.0 ** 57, dtype=torch.float64), sign * S


def subnormal_operands(M: int, N: int, R: int, kind: str) -> tuple[Tensor, Tensor]:
    """Integer operands scaled so that the exact result S 2^e is
    ``out``: below the fp32 normal range (A 2^-70, B 2^-70: products of normal bf16 inputs, multiples of 2^-140),
    ``in``:  normal, from bf16-subnormal A entries (A 2^-133 with integers 1 .. 8, B 2^100)."""
    g = torch.Generator().manual_seed(5 + R)
    if kind == "out":
        A = torch.randint(-8, 9, (M, R), generator=g).double() * 2.0 ** -70
        B = torch.randint(-8, 9, (N, R), generator=g).double() * 2.0 ** -70
    else:
        A = torch.randint(-8, 9, (M, R), generator=g).double() * 2.0 ** -133
        B = torch.randint(-8, 9, (N, R), generator=g).double() * 2.0 ** 100
    return A, B


# ------------------------------------------------------------------ accept sets (bf16 outputs)
class Accept16(NamedTuple):
    """What a fused epilogue may write, as bf16 values in float64: the two ends of its error interval, rounded, and
    whether a zero of either sign is accepted as well (``fp8_refs.Accept`` for a bf16 output)."""
    lo: Tensor
    hi: Tensor
    tiny: Tensor


def accept16(v: Tensor, err: Tensor, tiny: Tensor | None = None) -> Accept16:
    moved = (err > 0) & torch.isfinite(v)  # v + 0 would turn -0 into +0, inf - inf an infinite v into NaN
    err = torch.where(moved, err, torch.zeros_like(v))
    lo = round_bf16(torch.where(moved, v - err, v))
    hi = round_bf16(torch.where(moved, v + err, v))
    t = v.abs() < 2.0 ** -126  # below the fp32 normal range the kernel's fp32 value may be flushed or lose bits
    return Accept16(lo, hi, t if tiny is None else (t | tiny))


def in_accept16(got: Tensor, acc: Accept16) -> Tensor:
    """Elementwise: the bf16 output (any dtype, compared in float64) lies between the two candidates; a NaN
    candidate needs a NaN."""
    g = f64(got)
    nan_ref = torch.isnan(acc.lo) | torch.isnan(acc.hi)
    ok = (g >= torch.minimum(acc.lo, acc.hi)) & (g <= torch.maximum(acc.lo, acc.hi))
    ok = ok | (acc.tiny & (g == 0))
    return torch.where(nan_ref, torch.isnan(g), ok & ~torch.isnan(g))


def single_code_share(acc: Accept16) -> float:
    same = (acc.lo == acc.hi) | (torch.isnan(acc.lo) & torch.isnan(acc.hi))
    return float(same.double().mean())


# ------------------------------------------------------------------ E. RoPE epilogue
# (S, M): S = 64 puts four sequences into one 256-row tile, S = 192 with M = 768 sequence boundaries inside tiles
ROPE_SM = ((64, 512), (192, 768), (256, 512))
# D -> (H, Hkv): N = (H + 2 Hkv) D = 768 and rot_cols = (H + Hkv) D; D = 96 rotates 576 columns, so heads straddle
# the 256-column tiles and the rotation ends inside the third
ROPE_HEADS = {32: (16, 4), 64: (8, 2), 96: (4, 2), 128: (4, 1)}
ROPE_R = 64
ROPE_EXTRA_ROWS = 5  # table rows past S
DELTA_ROPE = 2.0 ** -22
"""a c - b s (or a s + b c) in fp32: two products and a sum, or one product and an FMA.  Each product errs by at
most U |product|, the sum by U |result| <= U (|a c| + |b s|) (1 + U): in all at most 2^-23 (|a c| + |b s|) up to
second-order terms.  The bound used is twice that."""


def rope_tables(S: int, D: int) -> tuple[Tensor, Tensor]:
    """fp32 cos / sin [S + ROPE_EXTRA_ROWS, D / 2], theta = 10000."""
    pos = torch.arange(S + ROPE_EXTRA_ROWS, dtype=torch.float64).unsqueeze(1)
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = pos * inv
    return torch.cos(ang).float(), torch.sin(ang).float()


def rope_epilogue(P: Tensor, cos: Tensor, sin: Tensor, S: int, D: int, rot_cols: int) -> tuple[Tensor, Accept16]:
    """(rotated mask [M, N], accept set) of the QKV + RoPE epilogue on the bf16-rounded product P (float64):
    columns below rot_cols are rotated as interleaved pairs with the table row ``m % S`` and pair index
    ``(col % D) / 2``; the others (V) must equal P."""
    M, N = P.shape
    pos = torch.arange(M) % S
    col = torch.arange(N)
    pair = (col % D) // 2
    c = f64(cos)[pos][:, pair]  # [M, N]
    s = f64(sin)[pos][:, pair]
    even = (col % 2 == 0)
    partner = torch.where(even, col + 1, col - 1)
    a, b = P, P[:, partner]  # even column: a c - b s; odd column (a = x2, b = x1): a c + b s
    sgn = torch.where(even, -1.0, 1.0).double()
    v = a * c + sgn * b * s
    err = DELTA_ROPE * ((a * c).abs() + (b * s).abs())
    rot = (col < rot_cols).unsqueeze(0).expand(M, N)
    v = torch.where(rot, v, P)
    err = torch.where(rot, err, torch.zeros_like(err))
    return rot, accept16(v, err)


# ------------------------------------------------------------------ F. SwiGLU epilogues
def delta_swiglu(g: Tensor, base: float) -> Tensor:
    """``fp8_refs``' relative bounds (DELTA_SWIGLU_FWD / _BWD), which hold for g >= G_MIN = -16, extended by their
    own derivation below that: the exponent argument's error through exp2 is ln2 * 2U * |t|, t = -g log2(e),
    that is 2 |g| U, instead of the 32 U at g = -16."""
    return base + 2.0 * U * (-g - 16.0).clamp(min=0.0)


def sigmoid_tiny(g: Tensor) -> Tensor:
    """sigmoid(g) is below the fp32 normal range (g < -87.3): the kernel's fp32 intermediate may be flushed to
    zero, whatever the other factors are."""
    return (1.0 / (1.0 + torch.exp(-g))) < 2.0 ** -126


def swiglu_fwd_accept(gu: Tensor) -> Accept16:
    """a = silu(g) u on bf16 values gu (float64)."""
    F = gu.shape[-1] // 2
    g = gu[..., :F]
    v = RR.swiglu(gu)
    return accept16(v, delta_swiglu(g, FR.DELTA_SWIGLU_FWD) * v.abs(), sigmoid_tiny(g))


def swiglu_bwd_accept(gu: Tensor, d: Tensor) -> Accept16:
    """[dg | du] with the error scale A of ``fp8_refs.DELTA_SWIGLU_BWD``."""
    F = gu.shape[-1] // 2
    g, u = gu[..., :F], gu[..., F:]
    v = RR.swiglu_bwd(gu, d)
    sg = 1.0 / (1.0 + torch.exp(-g))
    q_parts = (1.0 + g * (1.0 - sg)).abs() + g.abs() * sg + (g * (1.0 - sg)).abs()
    a_dg = (d * u * sg).abs() * q_parts
    scale_a = torch.cat((a_dg, v[..., F:].abs()), dim=-1)
    scale_a = torch.where(torch.isnan(v), v, scale_a.nan_to_num(nan=0.0, posinf=math.inf))
    delta = delta_swiglu(g, FR.DELTA_SWIGLU_BWD)
    t = sigmoid_tiny(g)
    return accept16(v, torch.cat((delta, delta), dim=-1) * scale_a, torch.cat((t, t), dim=-1))


SWF_SHAPE = (512, 384, 64)  # M, F, R: gu is 512 x 768
SWF_SCALE_EXP = (0, 1, -1, 2, -2, 4, -16, 0)  # power of two of x's entry, per block of R rows


def swiglu_pairs() -> Tensor:
    """bf16 [K, 2]: the (g, u) pairs planted in gu -- ``rowwise_refs.swiglu_edge_input`` in both flips (0 / -0,
    +-1e-30, +-1, +-20, +-88, +-1e4 against themselves and mirrored) and pairs with the largest finite value and
    with subnormals."""
    e = torch.cat((RR.swiglu_edge_input(torch.bfloat16, False), RR.swiglu_edge_input(torch.bfloat16, True)))
    w = e.shape[1] // 2
    pairs = torch.stack((e[:, :w].reshape(-1), e[:, w:].reshape(-1)), dim=1)
    big, sub, sub2 = BF16_MAX, 2.0 ** -133, 1.5 * 2.0 ** -127
    extra = torch.tensor([[big, 1.0], [-big, 1.0], [1.0, big], [-1.0, -big], [big, big], [big, -big], [2.0, big],
                          [sub, 1.0], [-sub, 1.0], [1.0, sub], [1.0, -sub2], [sub2, sub], [20.0, sub], [-20.0, sub2],
                          [0.0, -0.0], [-0.0, big], [big, 0.0], [sub2, big]], dtype=torch.float64)
    return torch.cat((pairs, to_bf16(extra)))


def swiglu_fwd_inputs() -> tuple[Tensor, Tensor, Tensor]:
    """(x [M, R], w13 [2F, R] bf16, gu float64 [M, 2F] as it must come out).  Row m of x is zero but for
    2^p at column m % R, so gu[m, n] = 2^p w13[n, m % R]: one exact product plus zeros.  Column j of w13 holds pair
    (f + 7 j) % K as (w13[f, j], w13[F + f, j]).  p runs over SWF_SCALE_EXP: the largest finite value overflows to
    +-inf for p > 0 (through the scale, no operand is infinite: 0 * inf would poison the row), p = -16 moves the
    subnormals to the bottom of the fp32 range.  An exactly zero result is +0: the other 63 products are zeros and the accumulator
    starts at +0, and (+0) + (-0) = +0."""
    M, F, R = SWF_SHAPE
    pairs = swiglu_pairs()
    K = pairs.shape[0]
    idx = (torch.arange(F).unsqueeze(1) + 7 * torch.arange(R).unsqueeze(0)) % K  # [F, R]
    w13 = torch.cat((pairs[idx, 0], pairs[idx, 1]), dim=0).contiguous()  # [2F, R]
    x = torch.zeros(M, R, dtype=torch.float64)
    m = torch.arange(M)
    p = torch.tensor(SWF_SCALE_EXP, dtype=torch.float64)[(m // R) % len(SWF_SCALE_EXP)]
    x[m, m % R] = 2.0 ** p
    exact = f64(w13).t()[m % R] * (2.0 ** p).unsqueeze(1)  # [M, 2F], exact in float64
    gu = round_bf16(exact)
    # An exactly zero sum is +0 (above).  A nonzero fp32 value that rounds to zero in the bf16 conversion keeps its
    # sign (-2^-134 -> -0), as IEEE rounding does.  The smallest scale, 2^-16, keeps every product an fp32 value
    # (2^-133 2^-16 = 2^-149): with 2^-24 the product -2^-157 lies below the fp32 range, IEEE rounds it to -0 and
    # the MI355X's MFMA returned +0 -- the sign of a zero no fp32 accumulator can hold is not part of the contract.
    gu = torch.where(exact == 0, torch.zeros_like(gu), gu)
    return to_bf16(x), w13, gu


SWB_SHAPE = (512, 768, 64)  # M, F, R (dy [M, R], w2 [R, F]): da is 512 x 768


def swiglu_bwd_inputs() -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dy [M, R], w2 [R, F], gu [M, 2F] bf16, da float64 [M, F] bf16-rounded).  dy and w2 are the exact-accumulation
    integers, so da = round_bf16(dy w2) holds for every correct kernel; gu tiles ``swiglu_pairs`` (finite: it is an
    input here) over the matrix with a stride that is odd against the tile sizes.  Pairs whose u is the largest
    finite value are left out: dg = ((da u) sg) Q forms da u first, which overflows in fp32 for |da| >= 2 where
    the whole product (sg Q ~ 0.5) would not -- the unfused kernel's order of operations, not an error."""
    M, F, R = SWB_SHAPE
    A, B = int_operands(M, F, R, seed=3)
    da = round_bf16(A @ B.t())
    pairs = swiglu_pairs()
    pairs = pairs[f64(pairs[:, 1]).abs() < 1e38]
    K = pairs.shape[0]
    idx = (torch.arange(M).unsqueeze(1) * 5 + torch.arange(F).unsqueeze(0)) % K
    gu = torch.cat((pairs[idx, 0], pairs[idx, 1]), dim=1).contiguous()
    return to_bf16(A), to_bf16(B.t()).contiguous(), gu, da
