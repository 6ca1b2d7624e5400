"""The row-wise gfx950 kernels (softmax, cross-entropy, RoPE, embedding, add + RMSNorm, activations) against the
float64 references of ``tests/rowwise_refs.py``, at the widths, dtypes and ``-inf`` patterns where each kernel
takes another path.

Inputs are built on the CPU with a fixed seed, rounded to the test dtype and copied to the GPU; the reference
sees the same rounded values in float64.  Tolerances:

* fp32 outputs: ``rel()`` (max-abs error over max-abs reference) below 1e-5 forward / 1e-4 backward, the
  thresholds ``tests/test_kernels_gpu.py`` uses for the same ops.
* bf16 outputs, per element: ``|got - ref| <= 2^-7 |ref| + a``.  The kernels compute in fp32 and round once;
  2^-7 |ref| is one bf16 ulp (a correctly rounded result may cross a rounding boundary through the fp32 error).
  ``a`` covers results formed by cancellation: the fp32 value is within the fp32 threshold of the row's largest
  magnitude, so ``a = tol32 * max|ref row|`` unless a test derives another floor and says why.
* exact results (zeros at ``-inf`` columns, untouched pads and table rows, ``sum``, RoPE at position 0, the
  embedding gather, determinism) with ``torch.equal``.
"""

from __future__ import annotations

import pytest
import torch

from bpe_transformer import ops
from bpe_transformer.ops import reference as R

from . import rowwise_refs as RR
from .rowwise_refs import f64

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
FWD, BWD = 1e-5, 1e-4
BF16_ULP = 2.0 ** -7


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = f64(a), f64(b)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def check(got: torch.Tensor, ref: torch.Tensor, dtype: torch.dtype, tol32: float, floor=None, what: str = ""):
    """The module docstring's bound for ``dtype``; ``floor`` replaces the default absolute floor ``a``."""
    g = f64(got)
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    assert got.dtype == dtype, (what, got.dtype)
    if dtype == torch.float32:
        r = rel(g, ref)
        print(f"{what}: rel {r:.3e} (< {tol32:g})")
        assert r < tol32, (what, r)
        return
    if floor is None:
        floor = tol32 * ref.abs().amax(dim=-1, keepdim=True)
    bound = BF16_ULP * ref.abs() + floor
    err = (g - ref).abs()
    bad = ~(err <= bound)  # NaN counts as bad
    excess = float((err - bound).nan_to_num(nan=float("inf")).max())
    print(f"{what}: worst err - bound {excess:.3e}, {int(bad.sum())} of {bad.numel()} outside")
    assert not bad.any(), (what, int(bad.sum()), excess)


def _dy(shape, dtype, seed=99):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


# ------------------------------------------------------------------ softmax
def _softmax_case(dev, x, dtype, dim=-1, nan_rows=()):
    """Forward and backward of ``ops.softmax`` on the CPU tensor ``x`` (last-dim rows ``nan_rows`` fully -inf)."""
    xg = x.to(dev).requires_grad_(True)
    y = ops.softmax(xg, dim)
    dy = _dy(x.shape, dtype)
    y.backward(dy.to(dev))
    yc, gc = y.detach().cpu().movedim(dim, -1), xg.grad.cpu().movedim(dim, -1)
    xm, dym = x.movedim(dim, -1), dy.movedim(dim, -1)
    ref = RR.softmax(f64(xm))
    # the backward kernel reads the forward's stored (rounded) output: that is its input
    gref = RR.softmax_bwd(f64(yc), f64(dym))
    keep = torch.ones(xm.shape[:-1], dtype=torch.bool)
    for r in nan_rows:
        keep[r] = False
        assert torch.isnan(yc[r]).all() and torch.isnan(gc[r]).all()
    assert not torch.isnan(yc[keep]).any() and not torch.isnan(gc[keep]).any()
    check(yc[keep], ref[keep], dtype, FWD, what="softmax fwd")
    check(gc[keep], gref[keep], dtype, BWD, what="softmax bwd")
    # rows sum to 1: N roundings of at most 2^-9 y_i each sum to at most 2^-9 (bf16); fp32 within the fwd threshold
    assert float((f64(yc[keep]).sum(-1) - 1).abs().max()) < (FWD if dtype == torch.float32 else 2.0 ** -8)
    minf = torch.isinf(xm) & keep.unsqueeze(-1)
    assert torch.equal(yc[minf], torch.zeros_like(yc[minf])) and torch.equal(gc[minf], torch.zeros_like(gc[minf]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", RR.SOFTMAX_MS)
@pytest.mark.parametrize("N", RR.SOFTMAX_NS)
def test_softmax_widths(gpu_device, N, M, dtype):
    """One element, partial waves, 64 / 256 +- 1 (one wave, all four waves, the strided thread loop), odd widths."""
    _softmax_case(gpu_device, RR.softmax_input(M, N, dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [0, 1])
def test_softmax_other_dim_noncontiguous(gpu_device, dim, dtype):
    base = RR.softmax_input(65 * 37, 6, dtype, seed=2).view(65, 37, 6)
    leaf = base.to(gpu_device).requires_grad_(True)
    z = leaf[:, :, ::2]
    assert not z.is_contiguous()
    y = ops.softmax(z, dim)
    dy = _dy(z.shape, dtype)
    y.backward(dy.to(gpu_device))
    xc = base[:, :, ::2]
    yc = y.detach().cpu()
    check(yc.movedim(dim, -1), RR.softmax(f64(xc), dim).movedim(dim, -1), dtype, FWD, what="fwd")
    gref = RR.softmax_bwd(f64(yc), f64(dy), dim)
    g = leaf.grad.cpu()
    check(g[:, :, ::2].movedim(dim, -1), gref.movedim(dim, -1), dtype, BWD, what="bwd")
    assert torch.equal(g[:, :, 1::2], torch.zeros_like(g[:, :, 1::2]))


def test_softmax_shift_invariance_fp32(gpu_device):
    x = RR.softmax_input(3, 600, torch.float32, seed=6)
    shifted = x + 1e4  # re-rounded to fp32: the reference sees these values
    _softmax_case(gpu_device, shifted, torch.float32)
    # the same logits with the shift taken off again (exact in fp32: multiples of 2^-10 below 2^14) give the
    # same result from the kernel as from the reference
    back = shifted - 1e4
    assert torch.equal(f64(back), f64(shifted) - 1e4)
    y, yb = ops.softmax(shifted.to(gpu_device)), ops.softmax(back.to(gpu_device))
    assert rel(y, RR.softmax(f64(back))) < FWD and rel(y, yb) < FWD


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_spread_200_exact_zeros(gpu_device, dtype):
    x = RR.softmax_spread_input(600, dtype)
    _softmax_case(gpu_device, x, dtype)
    y = ops.softmax(x.to(gpu_device))
    assert (y == 0).any() and torch.isfinite(y).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern,N", [(p, n) for p, ns in RR.SOFTMAX_INF_PATTERNS.items() for n in ns])
def test_softmax_inf_patterns(gpu_device, pattern, N, dtype):
    """-inf entries: exact zeros there (forward and gradient), the float64 reference elsewhere, no NaN."""
    _softmax_case(gpu_device, RR.softmax_inf_input(pattern, N, dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [600, 5])
def test_softmax_fully_masked_row_is_nan(gpu_device, N, dtype):
    """The project's convention (test_masked_sdpa_all_masked_row_is_nan_and_grad): a row of only -inf is NaN;
    its neighbours are untouched."""
    x, r = RR.softmax_masked_row_input(N, dtype)
    _softmax_case(gpu_device, x, dtype, nan_rows=(r,))


# ------------------------------------------------------------------ cross-entropy
def _check_ce(dtype, t, refs, loss, rows, lse, grad, mask=None, what=""):
    loss_ref, rows_ref, lse_ref, grad_ref = refs
    valid = t != RR.IGNORE
    n = max(int(valid.sum()), 1)
    if loss is not None:
        assert abs(float(loss) - float(loss_ref)) <= FWD * abs(float(loss_ref)), (what, float(loss), float(loss_ref))
    if rows is not None:  # fp32 outputs for both logit dtypes
        assert rel(rows, rows_ref) < FWD and rel(lse, lse_ref) < FWD, what
        assert torch.equal(rows.cpu()[~valid], torch.zeros(int((~valid).sum())))
    g = grad.cpu()
    assert not torch.isnan(g).any(), what
    # (p - onehot) / n: cancellation only at the target, where the fp32 error is that of p; p's own fp32 error is
    # relative to p.  So the floor is tied to the row's largest probability, not to the (much larger) target entry.
    onehot = torch.zeros_like(grad_ref)
    onehot[valid, t[valid]] = 1.0 / n
    p_ref = grad_ref + onehot
    check(g, grad_ref, dtype, BWD, floor=BWD * p_ref.amax(dim=-1, keepdim=True), what=what + " grad")
    # max-abs over the row is set by the target entry (~1/n); the other V - 1 entries get the same threshold alone
    off = onehot == 0
    assert rel(f64(g) * off, p_ref * off) < (BWD if dtype == torch.float32 else BF16_ULP), what
    assert torch.equal(g[~valid], torch.zeros_like(g[~valid]))
    if mask is not None:
        assert torch.equal(g[mask], torch.zeros_like(g[mask]))


def _ce_case(dev, x, t, dtype, mask=None, pad=0):
    refs = RR.cross_entropy(f64(x), t)
    M, V = x.shape
    tg = t.to(dev)
    xg = x.to(dev).requires_grad_(True)
    loss = ops.cross_entropy(xg, tg)
    loss.backward()
    assert loss.dtype == torch.float32
    _check_ce(dtype, t, refs, loss, None, None, xg.grad, mask, "ops.cross_entropy")
    # the kernel itself, in place on a (possibly strided) view
    buf = _dy((M, V + pad), dtype, seed=5)
    buf[:, :V] = x
    bg = buf.to(dev)
    rows, lse = torch.ops.bpe_hip.ce_fwd_bwd(bg[:, :V], tg, RR.IGNORE, True)
    out = bg.cpu()
    _check_ce(dtype, t, refs, rows.sum() / max(int((t != RR.IGNORE).sum()), 1), rows, lse, out[:, :V], mask,
              "ce_fwd_bwd")
    assert torch.equal(out[:, V:], buf[:, V:])  # pad columns bitwise untouched
    # loss only: the logits stay as they were
    bg2 = buf.to(dev)
    rows2, lse2 = torch.ops.bpe_hip.ce_fwd_bwd(bg2[:, :V], tg, RR.IGNORE, False)
    assert torch.equal(rows2, rows) and torch.equal(lse2, lse) and torch.equal(bg2.cpu(), buf)


@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("side", ["register", "two_pass"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_kernel_switch_boundary(gpu_device, dtype, side, pad):
    """The odd vocabularies on either side of launch_ce_fwd_bwd's ``(V + vn) / vn <= 8192``: targets in the
    unaligned head, the vector body, the scalar tail and at V - 1, one ignored row; ``pad = 7``: the strided
    ``buf[:, :V]`` call of the LM head."""
    V = RR.ce_boundary_vocabs(dtype)[0 if side == "register" else 1]
    assert RR.ce_uses_register_kernel(V, dtype) == (side == "register")
    t, _ = RR.ce_position_targets(V, dtype)
    _ce_case(gpu_device, RR.ce_logits(V, dtype), t, dtype, pad=pad)


@pytest.mark.parametrize("pattern", RR.CE_INF_PATTERNS)
@pytest.mark.parametrize("side", ["register", "two_pass"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_inf_logits(gpu_device, dtype, side, pattern):
    V = RR.ce_boundary_vocabs(dtype)[0 if side == "register" else 1]
    x, t, mask = RR.ce_inf_case(pattern, V, dtype)
    _ce_case(gpu_device, x, t, dtype, mask=mask)


@pytest.mark.parametrize("side", ["register", "two_pass"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_all_rows_ignored(gpu_device, dtype, side):
    V = RR.ce_boundary_vocabs(dtype)[0 if side == "register" else 1]
    x = RR.ce_logits(V, dtype)
    t = torch.full((RR.CE_M,), RR.IGNORE)
    xg = x.to(gpu_device).requires_grad_(True)
    loss = ops.cross_entropy(xg, t.to(gpu_device))
    loss.backward()
    assert float(loss) == 0.0 and torch.equal(xg.grad.cpu(), torch.zeros_like(x))
    _ce_case(gpu_device, x, t, dtype)


# ------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["none", "s", "b1s"])
@pytest.mark.parametrize("D", RR.ROPE_DS)
def test_apply_rope(gpu_device, D, kind, dtype):
    dev = gpu_device
    B, H, S = RR.ROPE_SHAPE
    cos, sin = R.rope_tables(D, RR.ROPE_MAX_SEQ, 10000.0)
    cg, sg = cos.to(dev), sin.to(dev)
    x = RR.act_input((B, H, S, D), dtype, seed=D, scale=1.0)
    pos = RR.rope_positions(kind)
    p = torch.arange(S) if pos is None else pos
    assert int(p.min()) >= 0 and int(p.max()) < RR.ROPE_MAX_SEQ
    xg = x.to(dev).requires_grad_(True)
    y = ops.apply_rope(xg, cg, sg, None if pos is None else pos.to(dev))
    dy = _dy(x.shape, dtype)
    y.backward(dy.to(dev))
    c64, s64 = cos.double(), sin.double()
    check(y.detach(), RR.rope(f64(x), c64, s64, p), dtype, FWD, what="rope fwd")
    # the backward is the inverse rotation of the incoming gradient
    check(xg.grad, RR.rope(f64(dy), c64, s64, p, inverse=True), dtype, BWD, what="rope bwd")
    at0 = torch.broadcast_to(p == 0, (B, H, S))
    assert at0.any() and torch.equal(y.detach().cpu()[at0], x[at0])  # cos 1, sin 0: bitwise identity
    # rope(rope(x), inverse) = x.  bf16: the forward's rounding (2^-9 |y1|, 2^-9 |y2|) rotates back into each
    # element, at most 2^-9 (|y1| + |y2|) <= 2^-8 max|x row|, on top of the inverse's own single rounding
    flat = torch.broadcast_to(p, (B, H, S)).reshape(-1).to(dev)
    back = torch.ops.bpe_hip.rope(y.detach().reshape(-1, 1, D), flat, cg, sg, True).view(x.shape)
    xr = f64(x)
    floor = None if dtype == torch.float32 else (2.0 ** -8 + FWD) * xr.abs().amax(-1, keepdim=True)
    check(back, xr, dtype, FWD, floor=floor, what="rope round trip")


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (5, 2), (6, 2)])
def test_rope_qk_head_size_96(gpu_device, H, Hkv, pad):
    """D = 96: 12 chunk columns per head, 21 rows per block with 252 of 256 threads active; 50 rows leave a
    partial last block; H + Hkv = 5, 7, 8 cover the 4-head steps and the remainder loop."""
    dev = gpu_device
    D, B, S = 96, 2, 25
    W, nrot = (H + 2 * Hkv) * D, (H + Hkv) * D
    buf = _dy((B * S, W + pad), torch.bfloat16, seed=H)
    cos, sin = R.rope_tables(D, S + 3, 10000.0)
    g = buf.to(dev)
    torch.ops.bpe_hip.rope_qk_(g[:, :W], cos.to(dev), sin.to(dev), B, S, H, Hkv, D)
    out = g.cpu()
    assert torch.equal(out[:, nrot:], buf[:, nrot:])  # V columns and the stride padding
    pos = torch.arange(S).view(1, S, 1)
    ref = RR.rope(f64(buf[:, :nrot]).reshape(B, S, H + Hkv, D), cos.double(), sin.double(), pos)
    check(out[:, :nrot].reshape(B, S, H + Hkv, D), ref, torch.bfloat16, FWD, what="rope_qk_")


# ------------------------------------------------------------------ embedding
@pytest.mark.parametrize("case", RR.EMBED_ID_CASES)
@pytest.mark.parametrize("dtype,D", [(dt, d) for dt, ds in RR.EMBED_DS.items() for d in ds])
def test_embedding_widths_and_runs(gpu_device, dtype, D, case):
    dev = gpu_device
    vocab = RR.EMBED_VOCAB
    ids = RR.embedding_ids(case)
    W = RR.act_input((vocab, D), dtype, seed=D, scale=1.0)
    Wg = W.to(dev).requires_grad_(True)
    y = ops.embedding(Wg, ids.to(dev))
    assert torch.equal(y.detach().cpu(), RR.embedding(W, ids))
    dy = _dy((ids.numel(), D), dtype)
    y.backward(dy.to(dev))
    g1 = Wg.grad.clone()
    # fp32 sums in sorted order, rounded once
    check(g1, RR.embedding_bwd(f64(dy), ids, vocab), dtype, BWD, what="embedding bwd")
    untouched = torch.ones(vocab, dtype=torch.bool)
    untouched[ids] = False
    assert untouched.any() and torch.equal(g1.cpu()[untouched], torch.zeros(int(untouched.sum()), D, dtype=dtype))
    Wg.grad = None
    ops.embedding(Wg, ids.to(dev)).backward(dy.to(dev))
    assert torch.equal(Wg.grad, g1)


# ------------------------------------------------------------------ add + RMSNorm
@pytest.mark.parametrize("M", RR.ADD_RMS_MS)
@pytest.mark.parametrize("dtype,N", [(dt, n) for dt, ns in RR.ADD_RMS_NS.items() for n in ns])
def test_add_rmsnorm_fwd(gpu_device, dtype, N, M):
    dev = gpu_device
    x, d, w = RR.add_rmsnorm_input(M, N, dtype)
    s, y, rstd = torch.ops.bpe_hip.add_rmsnorm_fwd(x.to(dev), d.to(dev), w.to(dev), 1e-5)
    assert torch.equal(s.cpu(), (x.float() + d.float()).to(dtype))  # one rounding
    s_ref, y_ref, rstd_ref = RR.add_rmsnorm(f64(x), f64(d), f64(w), 1e-5, dtype)
    assert torch.equal(f64(s), s_ref)
    assert rstd.dtype == torch.float32 and rstd.shape == (M,) and rel(rstd, rstd_ref) < FWD
    check(y, y_ref, dtype, FWD, what="add_rmsnorm y")


# ------------------------------------------------------------------ activations
ACTS = {"silu": (ops.silu, RR.silu, RR.silu_bwd, R.silu), "gelu": (ops.gelu, RR.gelu, RR.gelu_bwd, R.gelu_tanh)}
GRID_STRIDE_VECS = 4096 * 256 + 1  # stream_grid caps the grid at 4096 blocks of 256 threads


def _act_case(dev, name, x, dtype):
    f, fref, bref, _ = ACTS[name]
    xg = x.to(dev).requires_grad_(True)
    y = f(xg)
    dy = _dy(x.shape, dtype)
    y.backward(dy.to(dev))
    assert torch.isfinite(y).all() and torch.isfinite(xg.grad).all()
    check(y.detach(), fref(f64(x)), dtype, FWD, what=name + " fwd")
    check(xg.grad, bref(f64(x), f64(dy)), dtype, BWD, what=name + " bwd")


def _swiglu_case(dev, gu, dtype):
    gg = gu.to(dev).requires_grad_(True)
    a = ops.swiglu_gate(gg)
    d = _dy(a.shape, dtype)
    a.backward(d.to(dev))
    assert torch.isfinite(a).all() and torch.isfinite(gg.grad).all()
    check(a.detach(), RR.swiglu(f64(gu)), dtype, FWD, what="swiglu fwd")
    check(gg.grad, RR.swiglu_bwd(f64(gu), f64(d)), dtype, BWD, what="swiglu bwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", ["silu", "gelu", "swiglu"])
def test_activation_shapes(gpu_device, name, wide, M, dtype):
    F = 264 if wide else RR.vec_elems(dtype)
    if name == "swiglu":
        _swiglu_case(gpu_device, RR.act_input((M, 2 * F), dtype, seed=M), dtype)
    else:
        _act_case(gpu_device, name, RR.act_input((M, F), dtype, seed=M), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["silu", "gelu", "swiglu"])
def test_activation_edge_values(gpu_device, name, dtype):
    """0, -0, +-1e-30, +-1, +-20, +-88, +-1e4, one magnitude per row (the bound's floor is per row): finite
    forward and backward, equal to the reference."""
    if name == "swiglu":
        _swiglu_case(gpu_device, RR.swiglu_edge_input(dtype, flip=True), dtype)  # g = +-v against u = -+v
        _swiglu_case(gpu_device, RR.swiglu_edge_input(dtype, flip=False), dtype)
    else:
        _act_case(gpu_device, name, RR.act_edge_input(dtype), dtype)


@pytest.mark.parametrize("name,dtype", [("silu", torch.float32), ("gelu", torch.bfloat16),
                                        ("swiglu", torch.bfloat16)])
def test_activation_grid_stride(gpu_device, name, dtype):
    """One vector more than the capped grid covers in one sweep: the last vector is a second loop iteration."""
    v = RR.vec_elems(dtype)
    if name == "swiglu":
        M, fv = 17, GRID_STRIDE_VECS // 17
        assert M * fv == GRID_STRIDE_VECS
        _swiglu_case(gpu_device, RR.act_input((M, 2 * fv * v), dtype, seed=1), dtype)
    else:
        _act_case(gpu_device, name, RR.act_input((GRID_STRIDE_VECS * v,), dtype, seed=1), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["silu", "gelu"])
def test_activation_fallback_off_vector_width(gpu_device, name, dtype):
    """A size that is no multiple of the vector width takes the reference composition (on the GPU)."""
    f, fref, bref, fallback = ACTS[name]
    x = RR.act_input((13,), dtype)
    xg = x.to(gpu_device).requires_grad_(True)
    y = f(xg)
    assert torch.equal(y.detach(), fallback(xg.detach()))
    dy = _dy(x.shape, dtype)
    y.backward(dy.to(gpu_device))
    xr = x.to(gpu_device).requires_grad_(True)
    fallback(xr).backward(dy.to(gpu_device))
    assert torch.equal(xg.grad, xr.grad)
    if dtype == torch.float32:
        check(y.detach(), fref(f64(x)), dtype, FWD, what="fwd")
        check(xg.grad, bref(f64(x), f64(dy)), dtype, BWD, what="bwd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_gate_fallback_off_vector_width(gpu_device, dtype):
    """``ops.swiglu_gate`` with F = 6 (no multiple of 4 or 8): the reference composition, as silu / gelu do,
    where the binding used to raise."""
    gu = RR.act_input((5, 12), dtype)
    gg = gu.to(gpu_device).requires_grad_(True)
    a = ops.swiglu_gate(gg)
    assert a.shape == (5, 6) and a.dtype == dtype
    d = _dy(a.shape, dtype)
    a.backward(d.to(gpu_device))
    gr = gu.to(gpu_device).requires_grad_(True)
    ar = R.silu(gr[..., :6]) * gr[..., 6:]
    ar.backward(d.to(gpu_device))
    assert torch.equal(a.detach(), ar.detach()) and torch.equal(gg.grad, gr.grad)
    if dtype == torch.float32:
        check(a.detach(), RR.swiglu(f64(gu)), dtype, FWD, what="fwd")
        check(gg.grad, RR.swiglu_bwd(f64(gu), f64(d)), dtype, BWD, what="bwd")
