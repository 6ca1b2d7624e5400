"""The float64 references of ``tests/optim_refs.py`` against torch's own float64 autograd, ``torch.optim.AdamW``
and ``clip_grad_norm_``; the coverage of the RMSNorm-backward shape tables over ``rms_bwd_dispatch``'s kernel
instances; and the fp32 CPU path of ``fused_adamw_step`` under the bound the GPU tests use (CPU only)."""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.ops.optim import fused_adamw_step

from . import optim_refs as OR

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16]
FWD = 1e-5


def close(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=1e-12)


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("M,N", [(1, 8), (5, 24), (7, 260)])
def test_rmsnorm_ref_vs_autograd(M, N):
    x, w, dy, dres = _rand(M, N), 1 + 0.1 * _rand(N, seed=1), _rand(M, N, seed=2), _rand(M, N, seed=3)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + OR.RMS_EPS) * wr
    y.backward(dy)
    y_ref, rstd = OR.rmsnorm(x, w, OR.RMS_EPS)
    assert close(y_ref, y.detach()) and rstd.shape == (M,)
    dx, dw, dw_abs = OR.rmsnorm_bwd(dy, x, w, rstd)
    assert close(dx, xr.grad) and close(dw, wr.grad)
    assert dw_abs.shape == (N,) and bool((dw_abs >= dw.abs() - 1e-12).all())
    dx2, dw2, _ = OR.rmsnorm_bwd(dy, x, w, rstd, dres)
    assert close(dx2, xr.grad + dres) and torch.equal(dw2, dw)
    # dy x_hat >= 0 everywhere: no cancellation, the absolute sum is the sum
    dyp = dy.abs() * torch.sign(x)
    _, dwp, dwp_abs = OR.rmsnorm_bwd(dyp, x, w, rstd)
    assert close(dwp, dwp_abs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", OR.RMS_SPECIAL_ROWS)
def test_rms_special_inputs(kind, dtype):
    M, N = 38, 65 * OR.vec_elems(dtype)
    x, w, dy, row = OR.rms_special_input(kind, M, N, dtype)
    assert x.dtype == dtype and torch.isfinite(x.float().pow(2).sum(-1)).all()
    xf, wf, dyf = OR.f64(x), OR.f64(w), OR.f64(dy)
    _, rstd = OR.rmsnorm(xf, wf, OR.RMS_EPS)
    dx, dw, _ = OR.rmsnorm_bwd(dyf, xf, wf, rstd)
    if kind == "scaled":
        amax = xf.abs().amax(-1)
        assert float(amax.max() / amax.min()) > 2.0 ** 18
    elif kind == "zero_x_row":
        assert float(rstd[row]) == pytest.approx(OR.RMS_EPS ** -0.5, rel=1e-12)
        assert close(dx[row], rstd[row] * dyf[row] * wf)
    elif kind == "zero_dy_row":
        assert torch.equal(dx[row], torch.zeros(N, dtype=F64))
        keep = torch.arange(M) != row
        assert close(dw, OR.rmsnorm_bwd(dyf[keep], xf[keep], wf, rstd[keep])[1])
    else:
        assert bool((w == 0).any()) and bool((w < 0).any()) and bool((w > 0).any())


# ------------------------------------------------------------------ dispatch mirror and shape tables
@pytest.mark.parametrize("dtype", DTYPES)
def test_rms_tables_reach_every_instance(dtype):
    shapes = OR.rms_shapes(dtype)
    reached = {OR.rms_bwd_kernel_for(M, N, dtype) for M, N in shapes}
    assert OR.REJECTED not in reached
    assert reached == OR.RMS_BWD_INSTANCES, sorted(OR.RMS_BWD_INSTANCES - reached)
    assert max(M * N for M, N in shapes) * torch.empty((), dtype=dtype).element_size() < 40e6


@pytest.mark.parametrize("dtype", DTYPES)
def test_rms_tables_take_the_kernels_they_name(dtype):
    V = OR.vec_elems(dtype)
    for M in OR.RMS_MS:
        for nv in OR.RMS_NARROW_NVS:
            assert OR.rms_bwd_kernel_for(M, nv * V, dtype)[0] == "narrow"
        for nv in OR.RMS_HW_NVS:
            assert OR.rms_bwd_kernel_for(M, nv * V, dtype)[0] == ("narrow" if M % 2 else "half_wave")
        for nv in OR.RMS_WIDE_NVS:
            assert OR.rms_bwd_kernel_for(M, nv * V, dtype) == ("wide", nv // 256)
    # the instances the issue names: narrow C = 8, wide C2 = 3, partial waves
    assert OR.rms_bwd_kernel_for(3, 257 * V, dtype) == ("narrow", 8) == OR.rms_bwd_kernel_for(3, 511 * V, dtype)
    assert OR.rms_bwd_kernel_for(3, 768 * V, dtype) == ("wide", 3)
    assert OR.rms_bwd_kernel_for(3, 33 * V, dtype) == ("narrow", 1) == OR.rms_bwd_kernel_for(3, 64 * V, dtype)
    assert OR.rms_bwd_kernel_for(3, 65 * V, dtype) == ("narrow", 2)
    assert OR.rms_bwd_kernel_for(3, 255 * V, dtype) == ("narrow", 4)
    for nv in OR.RMS_REJECTED_NVS:
        assert OR.rms_bwd_kernel_for(4, nv * V, dtype) == OR.REJECTED
    assert OR.rms_bwd_kernel_for(4, 64 * V + 1, dtype) == OR.REJECTED  # no whole number of 16-byte vectors
    for fam, nv, M in OR.RMS_FAMILY_CASES:
        assert OR.rms_family(M, nv * V, dtype) == fam


@pytest.mark.parametrize("dtype", DTYPES)
def test_rms_round_cases_go_beyond_one_round(dtype):
    """Each family's round case is one row group more than a whole round of its full-size grid (narrow and
    half-wave: the capped grid itself), with a ragged remainder."""
    V = OR.vec_elems(dtype)
    full = {"narrow": OR.RMS_BWD_GRID * 4, "half_wave": OR.RMS_BWD_HW_GRID * 8, "wide_rpi2": OR.RMS_BWD_GRID * 2,
            "wide_rpi1": OR.RMS_BWD_GRID}
    assert {f for f, _, _ in OR.RMS_ROUND_CASES} == set(full)
    for fam, nv, M in OR.RMS_ROUND_CASES:
        N = nv * V
        assert OR.rms_family(M, N, dtype) == fam
        per = OR.rms_bwd_rows_per_round(M, N, dtype)
        assert M > per and M % per != 0, (fam, M, per)
        assert full[fam] < M < full[fam] + 8
        if fam in ("narrow", "half_wave"):
            assert per == full[fam]
    # the existing (4096, 768) bf16 case is exactly one half-wave round
    assert OR.rms_bwd_rows_per_round(4096, 768, torch.bfloat16) == 4096


# ------------------------------------------------------------------ AdamW
def _torch_adamw(p, grads, hp, wd):
    """``len(grads)`` steps of torch.optim.AdamW in float64 from zero moments -> (p, exp_avg, exp_avg_sq)."""
    q = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
    for g in grads:
        q.grad = g.clone()
        opt.step()
    st = opt.state[q]
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("scale", [None, 0.5])
def test_adamw_ref_vs_torch(scale):
    hp = OR.ADAMW_HP
    n = 131
    p = _rand(n)
    grads = [_rand(n, seed=10 + i) for i in range(6)]
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    q = p.clone()
    for i, g in enumerate(grads):
        (q, m, v), (pa, ma, va) = OR.adamw(q, m, v, g, step=i + 1, scale=scale, **hp)
        assert bool((pa >= q.abs() - 1e-12).all()) and bool((ma >= m.abs()).all()) and close(va, v)
    tp, tm, tv = _torch_adamw(p, [g if scale is None else g * scale for g in grads], hp, hp["wd"])
    assert close(q, tp) and close(m, tm) and close(v, tv)


def test_adamw_ref_mask_is_per_element_decay():
    hp = OR.ADAMW_HP
    n = 64 * 5 + 3
    mask = OR.expand_mask(OR.block_mask(n, 1), n)
    assert mask.shape == (n,) and int(mask[0]) == 1 and int(mask[64]) == 0 and int(mask[-1]) == 0
    assert int(OR.expand_mask(OR.block_mask(n, 0), n)[-1]) == 1
    p, g = _rand(n), _rand(n, seed=1)
    z = torch.zeros(n, dtype=F64)
    (q, m, v), _ = OR.adamw(p, z, z, g, step=1, wd_mask=mask, **hp)
    on = mask.bool()
    for sel, wd in ((on, hp["wd"]), (~on, 0.0)):
        tp, tm, tv = _torch_adamw(p[sel], [g[sel]], hp, wd)
        assert close(q[sel], tp) and close(m[sel], tm) and close(v[sel], tv)


def _cpu_fp32_ratios(p, m, v, g, step, scale=None, mask=None):
    hp = OR.ADAMW_HP
    n = p.numel()
    (rp, rm, rv), sums = OR.adamw(OR.f64(p), OR.f64(m), OR.f64(v), OR.f64(g), step=step, scale=scale,
                                  wd_mask=None if mask is None else OR.expand_mask(mask, n), **hp)
    cp, cm, cv = p.clone(), m.clone(), v.clone()
    fused_adamw_step(cp, cm, cv, g, None, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step,
                     None if scale is None else torch.tensor(scale), None, mask)
    return [OR.adamw_err_ratio(a, b, s, FWD) for a, b, s in zip((cp, cm, cv), (rp, rm, rv), sums)]


@pytest.mark.parametrize("gdtype", DTYPES)
def test_adamw_cpu_fp32_path_is_inside_the_fwd_bound(gdtype):
    """The bound of the GPU tests, ``|got - ref| <= FWD * (sum of absolute terms)``, holds for a plain fp32
    evaluation of the same update: it is not the bound that is too tight if the kernel misses it."""
    worst = 0.0
    for n in OR.ADAMW_NS[:-1]:
        worst = max(worst, *_cpu_fp32_ratios(*OR.adamw_input(n, gdtype), step=3, scale=0.5))
    n = 64 * 5 + 3
    worst = max(worst, *_cpu_fp32_ratios(*OR.adamw_input(n, gdtype), step=3, mask=OR.block_mask(n, 1)))
    for kind in OR.ADAMW_EDGE_KINDS:
        p, m, v, g, step = OR.adamw_edge_input(kind, gdtype)
        assert torch.isfinite(g.float() ** 2).all()
        worst = max(worst, *_cpu_fp32_ratios(p, m, v, g, step))
    print(f"fp32 CPU AdamW: worst error / bound {worst:.3e}")
    assert worst <= 1.0


def test_adamw_first_step_moves_by_lr():
    hp = OR.ADAMW_HP
    p, m, v, g, step = OR.adamw_edge_input("first_step", torch.float32)
    (q, _, _), _ = OR.adamw(OR.f64(p), OR.f64(m), OR.f64(v), OR.f64(g), step=step, **dict(hp, wd=0.0))
    big = g.abs() > 1e-3
    assert bool(big.any()) and float(((q - OR.f64(p)).abs()[big] / hp["lr"] - 1).abs().max()) < 1e-4


def test_adamw_sizes_cross_the_sweep():
    assert OR.ADAMW_NS[-1] == 2_097_152 + 4 * 256 + 3 and OR.ADAMW_NS[-1] % 4 == 3
    assert OR.ADAMW_NS[-1] // 4 > 2048 * 256  # a second grid-stride iteration


# ------------------------------------------------------------------ gradient norm / clip
@pytest.mark.parametrize("max_norm", [0.0, 1e-2, 7.0, 1e9, float("inf")])
def test_grad_norm_ref_vs_torch(max_norm):
    ts = [_rand(5), _rand(33, seed=1), _rand(4, 6, seed=2)]
    norm, coef = OR.grad_norm(ts, max_norm)
    params = [torch.nn.Parameter(t.clone()) for t in ts]
    for q in params:
        q.grad = q.detach().clone()
    tn = torch.nn.utils.clip_grad_norm_(params, max_norm)
    assert abs(norm - float(tn)) <= 1e-12 * norm
    assert 0.0 <= coef <= 1.0
    for q, t in zip(params, ts):
        assert close(q.grad, t * coef)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_grad_norm_ref_sentinel(bad):
    ts = [_rand(5), _rand(9, seed=1)]
    ts[1][3] = bad
    norm, coef = OR.grad_norm(ts, 1.0)
    assert not math.isfinite(norm) and coef == -1.0
    assert OR.grad_norm([torch.zeros(7, dtype=F64)], 1e-2) == (0.0, 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_sizes_isolate_pair_loop_and_remainder(dtype):
    """sumsq_partial_kernel: thread i takes vectors i, i + S in its pair loop while i + S < nv, then one
    remainder vector if i < nv.  nv = S: remainder only, every thread; S + 1: one pair, the rest remainders;
    2 S: pairs only; 2 S + 1: pairs, then one remainder after a loop iteration."""
    V, S = OR.vec_elems(dtype), OR.NORM_SWEEP_VECS
    sizes = OR.norm_sizes(dtype)
    assert 0 not in sizes and len(sizes) == 13 and V - 1 in sizes

    def split(nv):  # (threads that run a pair iteration, threads that run the remainder)
        pairs = max(0, min(S, nv - S))
        rem = sum(1 for i in (0, S - 1) if (i if i + S >= nv else i + 2 * S) < nv)
        return pairs, rem

    assert split(S) == (0, 2) and split(S + 1) == (1, 1) and split(2 * S) == (S, 0) and split(2 * S + 1) == (S, 1)
    x = OR.norm_input(sizes[-1], dtype)
    assert x.dtype == dtype and x.numel() == (2 * S + 1) * V + V - 1
    assert OR.norm_input(5, dtype).data_ptr() == x.data_ptr()
