"""Float64 reference, rounding emulation, bounds and the case table for the fused transformer block
(``bpe_transformer/models/fused_block.py``: ``FusedBlockFn`` forward and backward, ``AddRMSNormFn``).

Plain torch on the CPU; nothing here imports the fused block.  ``tests/test_block_refs.py`` checks this module on the
CPU, ``tests/test_fused_block_gpu.py`` checks the kernels' composition against it.

:func:`block_ref64` -- the block as a function, in float64, gradients by float64 autograd::

    x  = xr + xd                (x = xr when xd is None)
    h1 = rmsnorm(x; ln1)        x * rsqrt(mean(x^2) + eps) * w
    qkv = h1 @ [Wq;Wk;Wv]^T     interleaved-pair RoPE on Q and K at positions 0..S-1 (skipped without RoPE)
    o  = causal softmax attention, scale 1/sqrt(D), query head h reads KV head h // (H / Hkv), an optional document
         mask keeps keys doc_start[b, i] <= j <= i
    xm = x + o @ Wo^T
    h2 = rmsnorm(xm; ln2)
    g2 = (silu(h2 W1^T) * (h2 W3^T)) @ W2^T

Outputs ``xm``, ``g2``, ``dxr``, ``dxd`` and the nine parameter gradients (``dln1 dwq dwk dwv dwo dln2 dw1 dw3 dw2``)
from the upstream gradients ``dxm_out``, ``dg2``.  :func:`stack_ref64`: two blocks and the final ``rmsnorm(xr + xd)``.

Inputs (:func:`inputs`): CPU, fixed seed, rounded to bf16 -- the reference sees exactly those values.
``xr, xd ~ N(0, 1)``, weights ``~ N(0, 1 / fan_in)``, norm weights ``1 + 0.1 N(0, 1)``, upstream gradients
``~ N(0, 1)``.  Gradient buffers of the ``main_grad`` modes start from :func:`g0`, a bf16-representable pattern of
non-zero integers in [-4, 4]; the reference there is ``G0 + dW``.

:func:`emulate` -- the same function with one bf16 rounding (through fp32) at every tensor the fused block materialises in
bf16: ``x2, h1, qkv`` (and the rotated Q / K), ``o, g1, xm, h2, gu, a, g2, dgu, dh2, dxm, do, dqkv, dh1, dx2`` and the
bf16 weight gradients; inside attention the rounding points of ``tests/flash_refs.emulate`` (scaled Q, P, dS).
``rstd`` and ``lse`` stay unrounded, as does everything between two rounding points: those values are carried in
float64, not fp32, so that the emulation gives the same bits on every CPU (an fp32 sum depends on the BLAS and the
thread count, and 1e-7 can flip a bf16 rounding); fp32's own error is far below the bf16 steps.  With bf16 ``main_grad`` the slot is ``bf16(G0 + dW)`` (the kernels add in fp32 and
round once); with fp32 ``main_grad`` it is ``G0 + dW`` in fp32, no rounding.  Not modelled (the factor 2 in ``C``):
fp32 accumulation order, split-K partial sums, ``fast_exp2``, the tile-wise online softmax.

Bound, per element (NaN fails)::

    |got - ref| <= 2^-7 |ref| + C[name] * A[name]        bf16 outputs
    |got - ref| <=              C[name] * A[name]        fp32 main_grad slots (names ending in "32")

``A[name]``, from the float64 reference alone:

* ``xm, g2, dxr, dxd`` (``[tokens, d_model]``): the RMS of the element's **row** (one token);
* ``dwq dwk dwv dwo dw1 dw3 dw2`` and their ``...32`` forms (``[out, in]``): the RMS of the element's **row** of dW
  (one output feature: the rows scale with that feature's upstream gradient; G0 is not part of A);
* ``dln1, dln2`` (+ ``32``) (``[d_model]``): the RMS of the whole vector (its one row);
* the stack: ``s_y``, ``s_dx`` rows as above; ``s_dw`` the row RMS of each layer's weight gradient; ``s_dln`` the
  vector RMS of each norm gradient.

``NEED[name]``: the worst ``(err - 2^-7 |ref|) / A`` (fp32 names: ``err / A``) of :func:`emulate` over **all** specs
of :func:`matrix` in every gradient mode; ``C = 2 * NEED``.  Both were computed on the CPU by
``tests/test_block_refs.py::test_emulation_within_need`` (``-s`` prints the table) and are not fitted to a GPU.
"""

from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch
from torch import Tensor

from bpe_transformer.ops import reference as R

from .decode_refs import BF16, BF16_ULP, f64, randn
from .flash_refs import LOG2E, _rot, _rows, visible

EPS = 1e-5
THETA = 10000.0
WEIGHTS = ("ln1", "wq", "wk", "wv", "wo", "ln2", "w1", "w3", "w2")
GRADS = tuple("d" + n for n in WEIGHTS)
ACTS = ("xm", "g2", "dxr", "dxd")
NAMES = ACTS + GRADS
MODES = ("autograd", "bf16", "fp32")  # where dW goes: returned / added into bf16 main_grad / into fp32 main_grad
DEFECTS = ("gqa-mod", "no-resid-grad-1", "no-resid-grad-2", "dw-overwrite", "rope-k-missing", "dxd-missing",
           "norm-dw-twice")

# ------------------------------------------------------------------ the case table (shared by the CPU and GPU tests)
# routes: the predicate values the GPU test asserts before it runs the case (qkv = _fuse_qkv_rope, fwd =
# _fuse_swiglu_fwd, bwd = _fuse_swiglu_bwd, tn = _dx_tn of [Wq;Wk;Wv], Wo, [W1;W3], W2)
Case = namedtuple("Case", "name B S d H Hkv D F qkv fwd bwd tn")
CASES = (
    Case("fused64", 2, 128, 256, 4, 4, 64, 512, True, True, True, (True, True, True, True)),
    Case("fallback", 3, 100, 192, 3, 1, 64, 168, False, False, False, (True, True, False, False)),
    Case("short", 5, 40, 128, 2, 2, 64, 256, False, False, False, (True, True, True, True)),
    Case("d128", 2, 256, 512, 4, 2, 128, 768, True, True, True, (True, True, True, True)),
    Case("d128odd", 2, 192, 512, 4, 2, 128, 768, False, False, False, (True, True, True, True)),
    Case("qkvoff", 2, 128, 256, 4, 1, 64, 512, False, True, True, (True, True, True, True)),
    Case("bwdoff", 2, 128, 256, 4, 4, 64, 384, True, True, False, (True, True, True, True)),
)
BY_NAME = {c.name: c for c in CASES}

# document lengths per batch row: a length-1 document, boundaries at 32, 64 and mid-tile (100 / 84), all inside S
DOCS = {
    "fused64": ((1, 31, 32, 36, 28), (33, 31, 64)),
    "fallback": ((1, 31, 32, 20, 16), (33, 31, 36), (64, 1, 35)),
}

# xd: the residual delta is given; rope: the block rotates Q / K; doc: document mask
Spec = namedtuple("Spec", "case xd rope doc", defaults=(True, True, False))


def matrix() -> list[Spec]:
    """Every (case, variant) whose outputs the GPU tests compare with :func:`block_ref64`.  The kernel selectors
    (pre-rotated / in-kernel RoPE, attention backward form, dW route, gradient storage) change no reference."""
    out = [Spec(c.name) for c in CASES]
    for n in ("fused64", "fallback"):
        out += [Spec(n, xd=False), Spec(n, rope=False), Spec(n, doc=True)]
    return out


def dw_shapes(case: Case) -> list[tuple[int, int, int]]:
    """(n, k, t) of the block's four weight-gradient GEMMs with adjacent gradient slots: [Wq;Wk;Wv], Wo, [W1;W3], W2."""
    t = case.B * case.S
    return [((case.H + 2 * case.Hkv) * case.D, case.d, t), (case.d, case.H * case.D, t), (2 * case.F, case.d, t),
            (case.d, case.F, t)]


# measured on the CPU (tests/test_block_refs.py::test_emulation_within_need -s); C = 2 * NEED
NEED = {
    "xm": 0.0107, "g2": 0.0298, "dxr": 0.0226, "dxd": 0.0226, "dln1": 0.0232, "dwq": 0.048, "dwk": 0.0433,
    "dwv": 0.0372, "dwo": 0.0349, "dln2": 0.0172, "dw1": 0.0297, "dw3": 0.0311, "dw2": 0.0309, "dln132": 0.0262,
    "dwq32": 0.0503, "dwk32": 0.0438, "dwv32": 0.0401, "dwo32": 0.035, "dln232": 0.0218, "dw132": 0.0338,
    "dw332": 0.0328, "dw232": 0.0322, "s_y": 0.0267, "s_dx": 0.0305, "s_dw": 0.0604, "s_dln": 0.0244,
}
C = {
    "xm": 0.0214, "g2": 0.0596, "dxr": 0.0452, "dxd": 0.0452, "dln1": 0.0464, "dwq": 0.096, "dwk": 0.0866,
    "dwv": 0.0744, "dwo": 0.0698, "dln2": 0.0344, "dw1": 0.0594, "dw3": 0.0622, "dw2": 0.0618, "dln132": 0.0524,
    "dwq32": 0.1006, "dwk32": 0.0876, "dwv32": 0.0802, "dwo32": 0.07, "dln232": 0.0436, "dw132": 0.0676,
    "dw332": 0.0656, "dw232": 0.0644, "s_y": 0.0534, "s_dx": 0.061, "s_dw": 0.1208, "s_dln": 0.0488,
}


# ------------------------------------------------------------------ inputs (cached: treat as read-only)
def g0(*shape: int) -> Tensor:
    """The known non-zero start of a gradient buffer: integers in [-4, 4], never 0 (fp32; exact in bf16).  An
    overwritten slot is off by 1 to 4, against 2^-7 |ref| <= 0.04 that G0 adds to the bound."""
    n = math.prod(shape)
    i = torch.arange(n, dtype=torch.int64)
    v = (i * 7 + i // 13) % 8  # 0..7
    v = torch.where(v < 4, v - 4, v - 3)  # -4..-1, 1..4
    return v.float().view(*shape)


def _weights(c: Case, layer: int) -> dict[str, Tensor]:
    kv = c.Hkv * c.D
    sd, sf = c.d ** -0.5, c.F ** -0.5
    L = 100 * layer
    return {
        "ln1": (1 + 0.1 * randn(c.d, seed=(L + 1,)).float()).to(BF16),
        "wq": randn(c.H * c.D, c.d, seed=(L + 2,), scale=sd), "wk": randn(kv, c.d, seed=(L + 3,), scale=sd),
        "wv": randn(kv, c.d, seed=(L + 4,), scale=sd), "wo": randn(c.d, c.H * c.D, seed=(L + 5,), scale=(c.H * c.D) ** -0.5),
        "ln2": (1 + 0.1 * randn(c.d, seed=(L + 6,)).float()).to(BF16),
        "w1": randn(c.F, c.d, seed=(L + 7,), scale=sd), "w3": randn(c.F, c.d, seed=(L + 8,), scale=sd),
        "w2": randn(c.d, c.F, seed=(L + 9,), scale=sf),
    }


@functools.lru_cache(maxsize=None)
def inputs(spec: Spec) -> dict:
    """bf16 CPU tensors of ``spec``: ``xr``, ``xd`` (or None), the nine weights, ``dxm_out``, ``dg2``; fp32 ``cos`` /
    ``sin`` (or None); int32 ``doc_start`` / ``doc_end`` and ``doc_rows`` (or None)."""
    c = BY_NAME[spec.case]
    T = c.B * c.S
    p = _weights(c, 0)
    p["xr"] = randn(T, c.d, seed=(11,))
    p["xd"] = randn(T, c.d, seed=(12,)) if spec.xd else None
    p["dxm_out"] = randn(T, c.d, seed=(13,))
    p["dg2"] = randn(T, c.d, seed=(14,))
    p["cos"], p["sin"] = R.rope_tables(c.D, c.S, THETA) if spec.rope else (None, None)
    p["doc_rows"] = p["doc_start"] = p["doc_end"] = None
    if spec.doc:
        from .test_doc_mask_gpu import bounds_from_lengths

        p["doc_rows"] = DOCS[spec.case]
        p["doc_start"], p["doc_end"] = bounds_from_lengths([list(r) for r in p["doc_rows"]], "cpu")
    return p


STACK = Spec("fused64", xd=False)


@functools.lru_cache(maxsize=None)
def stack_inputs() -> dict:
    """Two layers of ``fused64`` weights, the final norm weight ``lnf``, the block-0 input ``xr`` (the embedding rows
    of tokens ``0..T-1``) and the upstream gradient ``dy`` of the final hidden states."""
    c = BY_NAME[STACK.case]
    T = c.B * c.S
    cos, sin = R.rope_tables(c.D, c.S, THETA)
    return {"layers": (_weights(c, 0), _weights(c, 1)), "lnf": (1 + 0.1 * randn(c.d, seed=(301,)).float()).to(BF16),
            "xr": randn(T, c.d, seed=(11,)), "dy": randn(T, c.d, seed=(302,)), "cos": cos, "sin": sin}


# ------------------------------------------------------------------ float64 reference
def _rms(x: Tensor, w: Tensor) -> Tensor:
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w


def _heads(t: Tensor, B: int, S: int, h: int, D: int) -> Tensor:
    return t.reshape(B, S, h, D).transpose(1, 2)


def _block64(c: Case, w: dict, xr: Tensor, xd: Tensor | None, cos, sin, doc_start) -> tuple[Tensor, Tensor]:
    x = xr if xd is None else xr + xd
    h1 = _rms(x, w["ln1"])
    q = _heads(h1 @ w["wq"].t(), c.B, c.S, c.H, c.D)
    k = _heads(h1 @ w["wk"].t(), c.B, c.S, c.Hkv, c.D)
    v = _heads(h1 @ w["wv"].t(), c.B, c.S, c.Hkv, c.D)
    if cos is not None:
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
    G = c.H // c.Hkv
    k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)  # query head h reads KV head h // G
    s = q @ k.transpose(-1, -2) / math.sqrt(c.D)
    s = s.masked_fill(~visible(c.B, c.S, True, doc_start)[:, None], float("-inf"))
    o = _rows(torch.softmax(s, -1) @ v)
    xm = x + o @ w["wo"].t()
    h2 = _rms(xm, w["ln2"])
    a = torch.nn.functional.silu(h2 @ w["w1"].t()) * (h2 @ w["w3"].t())
    return xm, a @ w["w2"].t()


def _leaf(t: Tensor | None) -> Tensor | None:
    return None if t is None else f64(t).requires_grad_(True)


def _row_rms(t: Tensor) -> Tensor:
    """RMS of each row, broadcastable against ``t`` (a vector is one row)."""
    return t.pow(2).mean(-1, keepdim=True).sqrt()


@functools.lru_cache(maxsize=None)
def block_ref64(spec: Spec) -> dict[str, Tensor]:
    """float64 ``xm g2 dxr dxd`` (``dxd`` None without xd) and ``d<weight>``, with ``A_<name>`` for each."""
    c, p = BY_NAME[spec.case], inputs(spec)
    w = {n: _leaf(p[n]) for n in WEIGHTS}
    xr, xd = _leaf(p["xr"]), _leaf(p["xd"])
    cos = None if p["cos"] is None else f64(p["cos"])
    sin = None if p["sin"] is None else f64(p["sin"])
    xm, g2 = _block64(c, w, xr, xd, cos, sin, p["doc_start"])
    torch.autograd.backward([xm, g2], [f64(p["dxm_out"]), f64(p["dg2"])])
    out = {"xm": xm.detach(), "g2": g2.detach(), "dxr": xr.grad, "dxd": None if xd is None else xd.grad}
    out.update({"d" + n: w[n].grad for n in WEIGHTS})
    for n in NAMES:
        if out[n] is not None:
            out["A_" + n] = _row_rms(out[n])
    return out


@functools.lru_cache(maxsize=None)
def stack_ref64() -> dict:
    """Two blocks and ``y = rmsnorm(xr + xd; lnf)`` in float64: ``y``, ``dx`` (of the block-0 input), ``dlnf`` and
    ``layers``: per layer the nine ``d<weight>``."""
    c, p = BY_NAME[STACK.case], stack_inputs()
    ws = [{n: _leaf(L[n]) for n in WEIGHTS} for L in p["layers"]]
    lnf, x0 = _leaf(p["lnf"]), _leaf(p["xr"])
    cos, sin = f64(p["cos"]), f64(p["sin"])
    xr, xd = x0, None
    for w in ws:
        xr, xd = _block64(c, w, xr, xd, cos, sin, None)
    y = _rms(xr + xd, lnf)
    y.backward(f64(p["dy"]))
    return {"y": y.detach(), "dx": x0.grad, "dlnf": lnf.grad,
            "layers": [{"d" + n: w[n].grad for n in WEIGHTS} for w in ws]}


# ------------------------------------------------------------------ the fused block's rounding points
def _bf(t: Tensor) -> Tensor:
    """One bf16 rounding (through fp32, as the kernels round).  The emulation carries its values in float64 between
    the rounding points, so that it gives the same bits on every CPU: fp32 sums depend on the BLAS and the thread
    count, and a sum that moves by 1e-7 can flip a bf16 rounding and with it the worst element."""
    return t.float().to(BF16).double()


def _rms_fwd(x: Tensor, w: Tensor) -> tuple[Tensor, Tensor]:
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
    return _bf(x * r * w), r


def _rms_bwd(dy: Tensor, x: Tensor, w: Tensor, r: Tensor, dres: Tensor | None) -> tuple[Tensor, Tensor]:
    """-> (bf16 dx [+ dres], fp32 dw)."""
    xh = x * r
    dyw = dy * w
    dx = r * (dyw - xh * (dyw * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres
    return _bf(dx), (dy * xh).sum(0)


def _emu_fwd(c: Case, w: dict, xr: Tensor, xd: Tensor | None, cos, sin, doc_start, defect) -> dict:
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    G = H // Hkv
    x2 = xr if xd is None else _bf(xr + xd)
    h1, r1 = _rms_fwd(x2, w["ln1"])
    wqkv = torch.cat([w["wq"], w["wk"], w["wv"]], 0)
    qkv = _bf(h1 @ wqkv.t())
    q = _heads(qkv[:, :H * D], B, S, H, D)
    k = _heads(qkv[:, H * D:(H + Hkv) * D], B, S, Hkv, D)
    v = _heads(qkv[:, (H + Hkv) * D:], B, S, Hkv, D)
    if cos is not None:
        q = _bf(_rot(q, cos, sin))
        if defect != "rope-k-missing":
            k = _bf(_rot(k, cos, sin))
    if defect == "gqa-mod":
        idx = torch.arange(H) % Hkv
    else:
        idx = torch.arange(H) // G
    kg, vg = k[:, idx], v[:, idx]
    sc = float(torch.tensor(float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32)) * LOG2E, dtype=torch.float32))
    vis = visible(B, S, True, doc_start)[:, None]
    s = (_bf(q * sc) @ kg.transpose(-1, -2)).masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    pexp = torch.exp2(s - m)
    l = pexp.sum(-1, keepdim=True)
    o = _bf(_rows(_bf(pexp) @ vg / l))
    lse = m + torch.log2(l)
    g1 = _bf(o @ w["wo"].t())
    xm = _bf(x2 + g1)
    h2, r2 = _rms_fwd(xm, w["ln2"])
    w13 = torch.cat([w["w1"], w["w3"]], 0)
    gu = _bf(h2 @ w13.t())
    g, u = gu[:, :c.F], gu[:, c.F:]
    a = _bf(torch.nn.functional.silu(g) * u)
    g2 = _bf(a @ w["w2"].t())
    return dict(c=c, w=w, x2=x2, r1=r1, h1=h1, q=q, k=k, v=v, kg=kg, vg=vg, idx=idx, s=s, lse=lse, o=o, xm=xm, r2=r2,
                h2=h2, gu=gu, a=a, g2=g2, has_xd=xd is not None, cos=cos, sin=sin, wqkv=wqkv, w13=w13, defect=defect)


def _emu_bwd(f: dict, dxm_out: Tensor, dg2: Tensor) -> dict:
    """-> bf16-valued ``dxr``, ``dxd`` and **unrounded** ``d<weight>`` (the caller stores them)."""
    c, w, defect = f["c"], f["w"], f["defect"]
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    scale = 1.0 / math.sqrt(D)
    g, u = f["gu"][:, :c.F], f["gu"][:, c.F:]
    da = dg2 @ w["w2"]
    sg = torch.sigmoid(g)
    dgu = _bf(torch.cat([da * u * sg * (1 + g * (1 - sg)), da * g * sg], 1))
    out = {"dw2": dg2.t() @ f["a"]}
    dw13 = dgu.t() @ f["h2"]
    out["dw1"], out["dw3"] = dw13[:c.F], dw13[c.F:]
    dh2 = _bf(dgu @ f["w13"])
    dxm, out["dln2"] = _rms_bwd(dh2, f["xm"], w["ln2"], f["r2"], None if defect == "no-resid-grad-2" else dxm_out)
    do = _bf(dxm @ w["wo"])
    out["dwo"] = dxm.t() @ f["o"]
    # attention backward (tests/flash_refs.emulate, split form)
    doh = _heads(do, B, S, H, D)
    oh = _heads(f["o"], B, S, H, D)
    delta = (doh * oh).sum(-1, keepdim=True)
    dp = doh @ f["vg"].transpose(-1, -2) - delta
    P = torch.exp2(f["s"] - f["lse"])
    ds = _bf(P * dp)
    dq = scale * (ds @ f["kg"])
    dkg = scale * (ds.transpose(-1, -2) @ f["q"])
    dvg = _bf(P).transpose(-1, -2) @ doh
    dk = torch.zeros(B, Hkv, S, D, dtype=torch.float64).index_add_(1, f["idx"], dkg)
    dv = torch.zeros(B, Hkv, S, D, dtype=torch.float64).index_add_(1, f["idx"], dvg)
    if f["cos"] is not None:
        dq = _rot(dq, f["cos"], f["sin"], inverse=True)
        if defect != "rope-k-missing":
            dk = _rot(dk, f["cos"], f["sin"], inverse=True)
    dqkv = _bf(torch.cat([_rows(dq), _rows(dk), _rows(dv)], 1))
    dwqkv = dqkv.t() @ f["h1"]
    q_, kv_ = H * D, Hkv * D
    out["dwq"], out["dwk"], out["dwv"] = dwqkv[:q_], dwqkv[q_:q_ + kv_], dwqkv[q_ + kv_:]
    dh1 = _bf(dqkv @ f["wqkv"])
    dx2, out["dln1"] = _rms_bwd(dh1, f["x2"], w["ln1"], f["r1"], None if defect == "no-resid-grad-1" else dxm)
    out["dxr"] = dx2
    out["dxd"] = None if not f["has_xd"] else torch.zeros_like(dx2) if defect == "dxd-missing" else dx2
    return out


def _store(dw: Tensor, mode: str, defect: str | None, norm: bool) -> Tensor:
    """Where a formed fp32 weight gradient goes: returned in bf16, or added to the ``G0`` of its main_grad slot."""
    if mode == "autograd":
        return dw.float().to(BF16)
    if defect == "norm-dw-twice" and norm:  # added by the kernel, then once more by the caller
        dw = dw + dw
    tot = dw if defect == "dw-overwrite" and not norm else g0(*dw.shape) + dw
    return tot.float().to(BF16) if mode == "bf16" else tot.float()


def emulate(spec: Spec, mode: str = "autograd", defect: str | None = None) -> dict[str, Tensor]:
    """The outputs of the fused block on ``inputs(spec)`` with its rounding points (module docstring): bf16 ``xm g2 dxr
    dxd``; the nine ``d<weight>`` as gradient ``mode`` stores them (bf16; bf16 ``G0 + dW``; fp32 ``G0 + dW``).
    ``defect``: one of :data:`DEFECTS`, each one line of the emulation broken the way the block could be."""
    assert mode in MODES and (defect is None or defect in DEFECTS)
    c, p = BY_NAME[spec.case], inputs(spec)
    fl = lambda t: None if t is None else t.double()  # noqa: E731
    w = {n: p[n].double() for n in WEIGHTS}
    f = _emu_fwd(c, w, p["xr"].double(), fl(p["xd"]), fl(p["cos"]), fl(p["sin"]), p["doc_start"], defect)
    b = _emu_bwd(f, p["dxm_out"].double(), p["dg2"].double())
    out = {"xm": f["xm"].to(BF16), "g2": f["g2"].to(BF16), "dxr": b["dxr"].to(BF16),
           "dxd": None if b["dxd"] is None else b["dxd"].to(BF16)}
    for n in GRADS:
        out[n] = _store(b[n], mode, defect, n in ("dln1", "dln2"))
    return out


def emulate_stack() -> dict:
    """:func:`stack_ref64`'s outputs with the rounding points of the fused stack (``AddRMSNormFn`` tail), autograd
    gradient storage."""
    c, p = BY_NAME[STACK.case], stack_inputs()
    ws = [{n: L[n].double() for n in WEIGHTS} for L in p["layers"]]
    xr, xd, fs = p["xr"].double(), None, []
    for w in ws:
        f = _emu_fwd(c, w, xr, xd, p["cos"].double(), p["sin"].double(), None, None)
        fs.append(f)
        xr, xd = f["xm"], f["g2"]
    lnf = p["lnf"].double()
    s_ = _bf(xr + xd)
    y, r = _rms_fwd(s_, lnf)
    dx, dlnf = _rms_bwd(p["dy"].double(), s_, lnf, r, None)
    da, db, layers = dx, dx, []  # AddRMSNormFn: its dx reaches xr and xd
    for f in reversed(fs):
        b = _emu_bwd(f, da, db)
        layers.insert(0, {n: b[n].float().to(BF16) for n in GRADS})
        da, db = b["dxr"], b["dxd"]
    return {"y": y.to(BF16), "dx": da.to(BF16), "dlnf": dlnf.float().to(BF16), "layers": layers}


# ------------------------------------------------------------------ error measures and the bound
def need_of(got: Tensor, ref: Tensor, A: Tensor, ulp: bool = True) -> float:
    """Worst element ``(|got - ref| - 2^-7 |ref|) / A`` (``ulp=False``: ``|got - ref| / A``); NaN -> inf."""
    err = (f64(got).reshape(ref.shape) - ref).abs().nan_to_num(nan=math.inf)
    if ulp:
        err = err - BF16_ULP * ref.abs()
    return float((err / A.clamp_min(1e-300)).max())


def measures(got: dict, spec: Spec, mode: str = "autograd") -> dict[str, float]:
    """name -> need for every output of ``got`` (``xm g2 dxr dxd`` and the ``d<weight>`` of gradient ``mode``;
    fp32 slots are reported under ``<name>32``)."""
    ref = block_ref64(spec)
    out = {}
    for n in ACTS:
        if ref[n] is None:
            assert got.get(n) is None, f"{n} must be None without xd"
            continue
        assert got[n] is not None, f"{n} is missing"
        out[n] = need_of(got[n], ref[n], ref["A_" + n])
    for n in GRADS:
        if n not in got:
            continue
        r = ref[n] if mode == "autograd" else ref[n] + g0(*ref[n].shape).double()
        if mode == "fp32":
            assert got[n].dtype == torch.float32, (n, got[n].dtype)
            out[n + "32"] = need_of(got[n], r, ref["A_" + n], ulp=False)
        else:
            out[n] = need_of(got[n], r, ref["A_" + n])
    return out


def stack_measures(got: dict) -> dict[str, float]:
    ref = stack_ref64()
    out = {"s_y": need_of(got["y"], ref["y"], _row_rms(ref["y"])),
           "s_dx": need_of(got["dx"], ref["dx"], _row_rms(ref["dx"])), "s_dw": -math.inf,
           "s_dln": need_of(got["dlnf"], ref["dlnf"], _row_rms(ref["dlnf"]))}
    for g, r in zip(got["layers"], ref["layers"]):
        for n in GRADS:
            key = "s_dln" if n in ("dln1", "dln2") else "s_dw"
            out[key] = max(out[key], need_of(g[n], r[n], _row_rms(r[n])))
    return out


def check(ms: dict[str, float], what: str = "") -> None:
    for n, need in ms.items():
        assert need <= C[n], (what, n, "per element need", need, "C", C[n])
