"""The AdamW, gradient-norm and clip kernels (``csrc/optim.hip``) against the float64 references of
``tests/optim_refs.py``.

Inputs are built on the CPU with a fixed seed and rounded to their dtype; the reference sees the rounded values.

AdamW bound, per element of ``p``, ``m`` and ``v``: ``|got - ref| <= FWD * (sum of the absolute values of the
terms the output is formed from)`` (``OR.adamw``), plus 2^-149 for an exact result below fp32's range.  A plain
fp32 evaluation of the update (the CPU path of ``fused_adamw_step``) stays within 1.5e-2 of that bound on the same
inputs (``tests/test_optim_refs.py`` prints and asserts it), so ``FWD`` is used as it stands.

Gradient norm: ``rel(norm) < FWD``.  The sum of squares is a sum of non-negative fp32 terms, so its relative
error is at most (number of roundings on the longest path) * 2^-24.  At the largest size here, 2 S + 1 vectors
(S = 2048 * 256), a thread squares and adds at most 3 vectors of V <= 8 elements (24 adds, one rounding per
square), the two accumulators are added (1), a block combines in a 6-level shuffle tree and 4 sequential adds
(10), and the final kernel adds 8 partials per tensor per thread (<= 16 for two tensors) and combines again
(10): about 62 roundings, 62 * 2^-24 = 3.7e-6.  The square root halves that and adds one rounding: 1.9e-6 < FWD.

The clip coefficient is compared with ``min(1, max / (norm + 1e-6))`` evaluated from the kernel's OWN norm, to
one fp32 ulp; ``scale_`` and the skip sentinel are exact (``torch.equal``).
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from bpe_transformer import ops
from bpe_transformer.ops.optim import count_adam_step, fused_adamw_step

from . import optim_refs as OR
from .optim_refs import f64
from .test_rowwise_kernels_gpu import FWD, check

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
HP = OR.ADAMW_HP
NAN = float("nan")


def _hp_args():
    return HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"]


def _run_adamw(dev, p, m, v, g, step, gscale=None, nstep=None, mask=None, pout=True):
    """One launch on copies of the CPU state -> (p, m, v, pout or None) on the CPU."""
    gp, gm, gv = (t.clone().to(dev) for t in (p, m, v))
    out = torch.full((p.numel(),), 7.0, dtype=torch.bfloat16, device=dev) if pout else None
    gs = None if gscale is None else torch.tensor(gscale, dtype=torch.float32, device=dev)
    ns = None if nstep is None else torch.tensor([nstep], dtype=torch.int32, device=dev)
    fused_adamw_step(gp, gm, gv, g.to(dev), out, *_hp_args(), step, gs, ns, None if mask is None else mask.to(dev))
    if ns is not None:
        assert int(ns.item()) == nstep  # read, never written
    return gp.cpu(), gm.cpu(), gv.cpu(), None if out is None else out.cpu()


def _check_adamw(got, p, m, v, g, step, scale=None, mask=None, what=""):
    n = p.numel()
    refs, sums = OR.adamw(f64(p), f64(m), f64(v), f64(g), step=step, scale=scale,
                          wd_mask=None if mask is None else OR.expand_mask(mask, n), **HP)
    for name, a, r, s in zip("pmv", got, refs, sums):
        assert a.dtype == torch.float32 and a.shape == (n,)
        ratio = OR.adamw_err_ratio(a, r, s, FWD)
        print(f"{what} {name}: worst error / bound {ratio:.3e}")
        assert ratio <= 1.0, (what, name, ratio)
    if got[3] is not None:
        assert torch.equal(got[3], got[0].to(torch.bfloat16))


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("n", OR.ADAMW_NS)
def test_adamw_sizes(gpu_device, n, gdtype):
    """Scalar tail only (1, 3), one vector, vector + tail, around one wave of vectors, and one sweep of the capped
    grid plus a block of vectors plus a 3-element tail: a second grid-stride iteration.  ``pout`` is the bf16
    rounding of the returned p; without it the other outputs are identical."""
    p, m, v, g = OR.adamw_input(n, gdtype)
    got = _run_adamw(gpu_device, p, m, v, g, 3, gscale=0.5)
    _check_adamw(got, p, m, v, g, 3, scale=0.5, what=f"n={n}")
    bare = _run_adamw(gpu_device, p, m, v, g, 3, gscale=0.5, pout=False)
    for a, b in zip(got[:3], bare[:3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("gscale", [None, 1.0, 0.5, -1.0, NAN])
def test_adamw_gscale_and_skip_sentinel(gpu_device, gscale, gdtype):
    """None, 1 and 0.5 scale the gradient; -1 (the non-finite-norm sentinel) and NaN leave p, m, v and pout
    bitwise untouched, and ``adam_count_step`` leaves the step count alone for them."""
    dev = gpu_device
    n = 1027
    p, m, v, g = OR.adamw_input(n, gdtype, seed=1)
    got = _run_adamw(dev, p, m, v, g, 3, gscale=gscale)
    skipped = gscale is not None and not gscale >= 0
    if skipped:
        assert torch.equal(got[0], p) and torch.equal(got[1], m) and torch.equal(got[2], v)
        assert torch.equal(got[3], torch.full((n,), 7.0, dtype=torch.bfloat16))
    else:
        _check_adamw(got, p, m, v, g, 3, scale=gscale, what=f"gscale={gscale}")
        assert not torch.equal(got[0], p)
    ns = torch.tensor([5], dtype=torch.int32, device=dev)
    count_adam_step(ns, None if gscale is None else torch.tensor(gscale, dtype=torch.float32, device=dev))
    assert int(ns.item()) == (5 if skipped else 6)


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("count", [1, 3, 1000])
def test_adamw_bias_correction_from_device_count(gpu_device, count, gdtype):
    """With ``nstep`` the bias correction comes from the device count; the ``step`` argument (77 here) is ignored."""
    p, m, v, g = OR.adamw_input(1027, gdtype, seed=2)
    got = _run_adamw(gpu_device, p, m, v, g, 77, nstep=count)
    _check_adamw(got, p, m, v, g, count, what=f"nstep={count}")
    if count != 1000:  # it does matter: the update with the step argument's correction is another one
        wrong = _run_adamw(gpu_device, p, m, v, g, 77)
        assert not torch.equal(wrong[0], got[0])


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("first", [1, 0], ids=["tail_undecayed", "tail_decayed"])
def test_adamw_wd_mask_with_tail(gpu_device, first, gdtype):
    """One byte per 64 elements, alternating, n = 64 * 5 + 3: the scalar tail lies in block 5, undecayed in one
    run and decayed in the other.  Against the reference's per-element decay, and bitwise equal to one launch per
    64-element segment."""
    dev = gpu_device
    n = 64 * 5 + 3
    mask = OR.block_mask(n, first)
    assert int(mask[5]) == 1 - first
    p, m, v, g = OR.adamw_input(n, gdtype, seed=3)
    got = _run_adamw(dev, p, m, v, g, 3, mask=mask)
    _check_adamw(got, p, m, v, g, 3, mask=mask, what=f"mask first={first}")
    plain = _run_adamw(dev, p, m, v, g, 3)
    assert not torch.equal(plain[0], got[0])
    gp, gm, gv = (t.clone().to(dev) for t in (p, m, v))
    out = torch.empty(n, dtype=torch.bfloat16, device=dev)
    gg = g.to(dev)
    lr, b1, b2, eps, wd = _hp_args()
    for b in range(len(mask)):
        s, e = 64 * b, min(64 * b + 64, n)
        fused_adamw_step(gp[s:e], gm[s:e], gv[s:e], gg[s:e], out[s:e], lr, b1, b2, eps, wd if int(mask[b]) else 0.0, 3)
    for a, b in zip(got, (gp, gm, gv, out)):
        assert torch.equal(a, b.cpu())


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("kind", OR.ADAMW_EDGE_KINDS)
def test_adamw_edge_values(gpu_device, kind, gdtype):
    """g = 0 with zero moments (p only decays); |g| = 1e-30 and 1e15 (g^2 finite in fp32); a first step from zero
    moments, where |dp| is lr."""
    p, m, v, g, step = OR.adamw_edge_input(kind, gdtype)
    got = _run_adamw(gpu_device, p, m, v, g, step)
    for t in got[:3]:
        assert torch.isfinite(t).all()
    _check_adamw(got, p, m, v, g, step, what=kind)
    if kind == "zero_grad":
        assert torch.equal(got[1], m) and torch.equal(got[2], v)
    if kind == "first_step":
        big = g.float().abs() > 1e-3
        dp = (f64(got[0]) - f64(p) * (1 - HP["lr"] * HP["wd"])).abs()
        assert float((dp[big] / HP["lr"] - 1).abs().max()) < 1e-3


# ------------------------------------------------------------------ gradient norm
def _coef_from(norm32: float, max_norm: float) -> float:
    """The kernel's expression in numpy fp32 from its own norm."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return float(min(c, np.float32(1.0)))


def _ulp_close(a: float, b: float) -> bool:
    return abs(a - b) <= float(np.spacing(np.float32(abs(b))))


def _norm_case(dev, tensors, max_norm):
    gts = [t.to(dev) for t in tensors]
    norm, coef = ops.grad_norm(gts, max_norm)
    assert norm.dtype == torch.float32 and coef.dtype == torch.float32 and norm.dim() == 0 and coef.dim() == 0
    n2, c2 = ops.grad_norm(gts, max_norm)
    assert torch.equal(norm.cpu().view(torch.int32), n2.cpu().view(torch.int32))  # bitwise, NaN included
    assert torch.equal(coef, c2)
    return float(norm), float(coef)


@pytest.mark.parametrize("max_norm", [0.0, 1e-2, float("inf")])
@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_norm_sizes(gpu_device, dtype, max_norm):
    """n = nv V + tail with nv = 0, 1, 255, S, S + 1, 2 S, 2 S + 1 vectors (S = one sweep of the 2048 blocks) and
    tail 0 or V - 1: the pair loop alone, the remainder vector alone, both, with and without the scalar tail."""
    for n in OR.norm_sizes(dtype):
        x = OR.norm_input(n, dtype)
        norm, coef = _norm_case(gpu_device, [x], max_norm)
        ref, cref = OR.grad_norm([f64(x)], max_norm)
        assert abs(norm - ref) < FWD * ref, (n, norm, ref)
        assert _ulp_close(coef, _coef_from(norm, max_norm)), (n, coef, norm)
        assert abs(coef - cref) <= 2 * FWD * max(cref, 1e-30), (n, coef, cref)
        if max_norm == 0 or math.isinf(max_norm):
            assert coef == (0.0 if max_norm == 0 else 1.0)


@pytest.mark.parametrize("max_norm", [0.0, 1e-2, float("inf")])
def test_grad_norm_mixed_dtypes(gpu_device, max_norm):
    ts = [OR.norm_input(8 * 300 + 7, torch.bfloat16), OR.norm_input(4 * 513 + 3, torch.float32)]
    norm, coef = _norm_case(gpu_device, ts, max_norm)
    ref, cref = OR.grad_norm([f64(t) for t in ts], max_norm)
    assert abs(norm - ref) < FWD * ref
    assert _ulp_close(coef, _coef_from(norm, max_norm)) and abs(coef - cref) <= 2 * FWD * max(cref, 1e-30)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_norm_all_zero(gpu_device, dtype):
    ts = [torch.zeros(1027, dtype=dtype), torch.zeros(5, dtype=dtype)]
    for max_norm in (1e-2, 1.0, 1e9):
        assert _norm_case(gpu_device, ts, max_norm) == (0.0, 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["body", "tail", "second"])
@pytest.mark.parametrize("bad", [float("inf"), NAN])
def test_grad_norm_non_finite(gpu_device, bad, where, dtype):
    """One inf or NaN in the vector body, in the scalar tail or in the second tensor: coef -1, norm not finite."""
    V = OR.vec_elems(dtype)
    a, b = OR.norm_input(300 * V + V - 1, dtype).clone(), OR.norm_input(77, dtype).clone()
    if where == "body":
        a[131 * V + 1] = bad
    elif where == "tail":
        a[-1] = bad
    else:
        b[40] = bad
    norm, coef = _norm_case(gpu_device, [a, b], 1.0)
    assert not math.isfinite(norm) and coef == -1.0
    assert OR.grad_norm([f64(a), f64(b)], 1.0)[1] == -1.0


# ------------------------------------------------------------------ scale_ and clip_grad_norm_
SCALE_SWEEP_VECS = 2048 * 256  # launch_scale: at most 2048 blocks of 256 threads, one vector each


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [1.0, -1.0, 0.25, 0.3])
def test_scale_exact(gpu_device, coef, dtype):
    """coef 1 and -1 (the skip sentinel) leave the tensor bitwise untouched; otherwise the result is the fp32
    product rounded once.  Sizes: tail only, vector + tail, one vector past a sweep plus a tail.  |x| >= 2^-20:
    no denormal inputs or results."""
    dev = gpu_device
    V = OR.vec_elems(dtype)
    c = torch.tensor(coef, dtype=torch.float32, device=dev)
    for n in (V - 1, 5 * V + V - 1, (SCALE_SWEEP_VECS + 1) * V + V - 1):
        x = OR.norm_input(n, dtype)
        x = torch.where(x.float().abs() < 2.0 ** -20, torch.ones_like(x), x)
        g = x.to(dev)
        torch.ops.bpe_hip.scale_(g, c)
        exp = x if coef in (1.0, -1.0) else (x.float() * coef).to(dtype)
        assert torch.equal(g.cpu(), exp), (n, coef)


def _clip_params(dev, poison=None):
    """-> (parameters, the CPU gradients they were given): fp32, fp32 transposed (non-contiguous), bf16, and a
    fourth parameter whose grad is None.  ``poison = (index, value)`` puts a non-finite value into one gradient."""
    gen = torch.Generator().manual_seed(43)
    grads = [torch.randn(1027, generator=gen), torch.randn(4, 6, generator=gen).t(),
             torch.randn(300, 8, generator=gen).to(torch.bfloat16)]
    if poison is not None:
        g = grads[poison[0]]
        g[(1,) * g.dim()] = poison[1]
    params = []
    for g in grads:
        q = torch.nn.Parameter(torch.zeros(g.shape, dtype=g.dtype, device=dev))
        q.grad = g.to(dev)
        assert q.grad.is_contiguous() == g.is_contiguous()
        params.append(q)
    assert not params[1].grad.is_contiguous()
    params.append(torch.nn.Parameter(torch.zeros(9, device=dev)))
    return params, [g.clone() for g in grads]


@pytest.mark.parametrize("max_norm", [1e-2, 1e9])
def test_clip_grad_norm(gpu_device, max_norm):
    """A parameter list with a ``None`` grad, a non-contiguous grad and a bf16 grad, against the float64
    reference: the fp32 product rounded once to each gradient's dtype."""
    params, grads = _clip_params(gpu_device)
    norm = ops.clip_grad_norm_(params, max_norm)
    ref, cref = OR.grad_norm([f64(g) for g in grads], max_norm)
    assert abs(float(norm) - ref) < FWD * ref
    assert (cref < 1.0) == (max_norm < ref)
    assert params[3].grad is None
    for q, g in zip(params[:3], grads):
        if cref == 1.0:
            assert torch.equal(q.grad.cpu(), g)
        else:
            check(q.grad.cpu().reshape(1, -1), (f64(g) * cref).reshape(1, -1), g.dtype, FWD, what="clipped grad")
    assert not params[1].grad.is_contiguous()


@pytest.mark.parametrize("which", [0, 1, 2], ids=["fp32", "noncontiguous", "bf16"])
@pytest.mark.parametrize("bad", [float("inf"), NAN])
def test_clip_grad_norm_non_finite_leaves_grads(gpu_device, bad, which):
    params, grads = _clip_params(gpu_device, poison=(which, bad))
    norm = ops.clip_grad_norm_(params, 1e-2)
    assert not math.isfinite(float(norm))
    for q, g in zip(params[:3], grads):
        a, b = q.grad.cpu().contiguous(), g.contiguous()
        it = torch.int32 if g.dtype == torch.float32 else torch.int16
        assert torch.equal(a.view(it), b.view(it))  # bitwise: NaN compares equal to itself
