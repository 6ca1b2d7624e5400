"""fp64 oracle and case table of the sampling controls (``ops/sampling.py``, "Sampling controls";
``ops/csrc/logit_process.hip``): shared by ``test_logit_refs.py`` (CPU: the torch references, the fixture itself) and
``test_logit_process_gpu.py`` (the kernels).

The oracle takes the inputs as the kernel receives them -- logits rounded to their dtype, ``rp`` / ``pp`` / ``fp``
rounded to fp32 -- and computes the function in fp64 with an exact ``1 / rp``.

Bounds (derived, not tuned):

* processed logit, fp32: ``8 * 2^-24 * (m * (|x| + |bias|) + |fp| * c + |pp|)``, ``m = max(rp, 1 / rp)``: at most five
  roundings (the add, the multiply, the product ``fp * c``, two subtractions) plus the rounding of ``1 / rp``, with a
  margin of 8 so that either FMA contraction passes;
* processed logit, bf16: that plus ``2^-8 * |ref|`` for the final rounding;
* an element with ``hist == 0`` and ``bias == 0``: its input's bits; a ``-inf`` reference: ``-inf``;
* ``lse`` / log-probs: :data:`lse_bound` (its docstring has the measurements it rests on).

bf16 rows are built so that no processed value lies within the fp32 bound of a bf16 rounding boundary (the midpoint of
two neighbouring bf16 values): ``test_logit_refs.py`` checks that on the CPU.
"""

from __future__ import annotations

import dataclasses
import math

import torch

VOCAB = 50257
SIZES = (1, 7, 8, 63, 1025, VOCAB)

# Worst |torch fp32 logsumexp - fp64| over every row of the case table, on the CPU (measured: 1.122e-06; rows of
# N(0, 4^2) logits, lse up to about 19).  The kernel's own worst |lse - lse64| over the same rows is recorded in
# test_logit_process_gpu.py; the bound below uses the first, never the second.
LSE_CPU_ERR = 1.122e-6


def lse_bound(xmax: torch.Tensor) -> torch.Tensor:
    """The bound on ``|lse - lse64|`` (and on a log-prob, which adds one exact-ish subtraction of the same size) for
    rows whose largest logit is ``xmax``: 4x the larger of the CPU reference's own measured error and ``2^-22 *
    max(1, |max x|)`` -- the floor covers rows where ``x - max`` is exact and the fp32 result is one rounding off."""
    floor = 2.0**-22 * xmax.double().abs().clamp(min=1.0)
    return 4.0 * torch.maximum(torch.full_like(floor, LSE_CPU_ERR), floor)


def f32(v: float) -> float:
    return float(torch.tensor(float(v), dtype=torch.float32))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    V: int
    B: int
    dtype: torch.dtype
    rp: float = 1.3
    pp: float = 0.25
    fp: float = 0.1
    shift: int = 0        # element offset of the input rows in their buffer
    out_shift: int = -1   # of the output rows in theirs; -1: in place
    hist: bool = True
    bias: bool = True
    lse: bool = True
    out: bool = True
    seed: int = 0


def all_cases() -> list[Case]:
    cs: list[Case] = []
    rps = (1.3, 0.7, 1.0)
    for i, V in enumerate(SIZES):
        for j, dt in enumerate((torch.float32, torch.bfloat16)):
            k = 2 * i + j
            cs.append(Case(f"V{V}-{'f32' if j == 0 else 'bf16'}", V, (1, 3)[(i + j) % 2], dt, rp=rps[k % 3],
                           out_shift=-1 if k % 2 else 0, seed=k))
    for j, dt in enumerate((torch.float32, torch.bfloat16)):
        tag = "f32" if j == 0 else "bf16"
        for s in (1, 3, 5):  # no row, the first included, is 16-byte aligned
            cs.append(Case(f"shift{s}-inplace-{tag}", 1025, 3, dt, shift=s, seed=20 + s))
            cs.append(Case(f"shift{s}-out-same-{tag}", 1025, 3, dt, rp=0.7, shift=s, out_shift=s, seed=30 + s))
            cs.append(Case(f"shift{s}-out-other-{tag}", 1025, 3, dt, shift=s, out_shift=(s + 2) % 8, seed=40 + s))
        cs.append(Case(f"no-hist-{tag}", 1025, 3, dt, hist=False, out_shift=0, seed=50))
        cs.append(Case(f"no-bias-{tag}", 1025, 3, dt, bias=False, seed=51))
        cs.append(Case(f"no-lse-{tag}", 1025, 3, dt, lse=False, out_shift=0, seed=52))
        cs.append(Case(f"lse-only-{tag}", 1025, 3, dt, out=False, hist=False, bias=False, seed=53))
        cs.append(Case(f"rp1-no-pen-{tag}", 63, 3, dt, rp=1.0, pp=0.0, fp=0.0, seed=54))
    return cs


def bf16_boundary_distance(y: torch.Tensor) -> torch.Tensor:
    """Distance of each fp64 ``y`` to the nearest bf16 rounding boundary (midpoint of two neighbouring bf16 values);
    ``inf`` for 0 and non-finite ``y``."""
    a = y.abs()
    ok = torch.isfinite(a) & (a > 0)
    e = torch.floor(torch.log2(torch.where(ok, a, torch.ones_like(a))))
    ulp = torch.exp2(e - 7)
    frac = a / ulp - torch.floor(a / ulp)
    return torch.where(ok, (frac - 0.5).abs() * ulp, torch.full_like(a, math.inf))


def process64(x, hist, bias, rp, pp, fp) -> torch.Tensor:
    """The processed logits in fp64 for the rounded inputs (module docstring)."""
    y = x.double()
    if bias is not None:
        y = y + bias.double()[None, :]
    if hist is not None:
        r = f32(rp)
        c = (hist >> 1).double()
        y = torch.where(hist != 0, torch.where(y > 0, y / r, y * r), y)
        y = y - f32(fp) * c - f32(pp) * (c > 0)
    return y


def process_bound(x, hist, bias, rp, pp, fp) -> torch.Tensor:
    """The fp32 bound of the module docstring, per element (fp64)."""
    r = f32(rp)
    mag = x.double().abs()
    if bias is not None:
        b = bias.double().abs()[None, :]
        mag = mag + torch.where(torch.isfinite(b), b, torch.zeros_like(b))
    mag = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag)) * max(r, 1.0 / r)
    if hist is not None:
        mag = mag + abs(f32(fp)) * (hist >> 1).double() + abs(f32(pp))
    return 8.0 * 2.0**-24 * mag


def touched(case_hist, case_bias, shape) -> torch.Tensor:
    t = torch.zeros(shape, dtype=torch.bool)
    if case_hist is not None:
        t |= case_hist != 0
    if case_bias is not None:
        t |= (case_bias != 0)[None, :]
    return t


def lse64(x) -> torch.Tensor:
    return torch.logsumexp(x.double(), -1)


def make(case: Case) -> dict:
    """The inputs of ``case`` on the CPU: ``x [B, V]`` of its dtype (N(0, 4^2), with a ``-0.0``, a ``+0.0`` and a
    ``-inf`` where the row has room), ``hist`` with counts 0, 1 and 1000 on and off the prompt, ``bias`` mostly 0 with a
    few values and one ``-inf``.  bf16 rows: elements whose processed value would lie within the fp32 bound of a
    rounding boundary are redrawn (a few rounds always suffice; asserted)."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    B, V = case.B, case.V
    x = (torch.randn(B, V, generator=g) * 4.0).to(case.dtype)
    hist = bias = None
    if case.hist:
        hist = torch.zeros(B, V, dtype=torch.int32)
        pick = torch.rand(B, V, generator=g)
        for lo, val in ((0.50, 1), (0.60, 2), (0.70, 3), (0.80, 2000), (0.90, 2001)):
            hist[pick >= lo] = val
    if case.bias:
        bias = torch.zeros(V, dtype=torch.float32)
        pick = torch.rand(V, generator=g)
        vals = torch.randn(V, generator=g) * 3.0
        bias[pick >= 0.8] = vals[pick >= 0.8]
        if V >= 7:
            bias[V // 2] = -math.inf
    if V >= 8:  # zeros of both signs and a -inf logit, on elements that nothing touches where there are any
        free = (~touched(hist, bias, (B, V))).nonzero()
        for n, val in enumerate((-0.0, 0.0, -math.inf)):
            if n < len(free):
                x[free[n][0], free[n][1]] = val
        x[0, 3] = -0.0  # (touched or not: -0.0 through the arithmetic)
    if case.dtype == torch.bfloat16 and case.out:
        for _ in range(16):
            ref = process64(x, hist, bias, case.rp, case.pp, case.fp)
            near = touched(hist, bias, (B, V)) & (bf16_boundary_distance(ref)
                                                  <= process_bound(x, hist, bias, case.rp, case.pp, case.fp))
            if not near.any():
                break
            x[near] = (torch.randn(int(near.sum()), generator=g) * 4.0).to(case.dtype)
        else:
            raise AssertionError("fixture: could not clear the bf16 rounding boundaries")
    return {"x": x, "hist": hist, "bias": bias}


def check_processed(case: Case, inp: dict, got: torch.Tensor) -> None:
    """``got [B, V]`` (the case's dtype, on the CPU) against the oracle, under the module docstring's bounds."""
    x, hist, bias = inp["x"], inp["hist"], inp["bias"]
    ref = process64(x, hist, bias, case.rp, case.pp, case.fp)
    t = touched(hist, bias, x.shape)
    bits = torch.int16 if case.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(got.view(bits)[~t], x.view(bits)[~t]), "an untouched element changed its bits"
    inf = torch.isinf(ref)
    assert torch.equal(got.double()[inf], ref[inf]), "an infinite reference must come out as itself"
    bound = process_bound(x, hist, bias, case.rp, case.pp, case.fp)
    if case.dtype == torch.bfloat16:
        bound = bound + 2.0**-8 * ref.abs()
    fin = t & ~inf
    err = (got.double() - ref).abs()[fin]
    assert bool((err <= bound[fin]).all()), f"{case.name}: worst excess {float((err - bound[fin]).max()):.3e}"
