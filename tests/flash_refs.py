"""Float64 reference, rounding emulation and input builders for the training flash-attention kernels
(``csrc/flash_attn_fwd.hip``, ``flash_attn_fwd_v4.hip``, ``flash_attn_bwd_split.hip``, ``flash_attn_bwd_dq16.hip``,
``flash_attn_bwd.hip`` and the DOC variants behind ``fa_fwd_doc`` / ``fa_bwd_doc``).

:func:`reference` works on the fused layout ``qkv [B*S, (H + 2 Hkv) D]`` from the bf16-rounded inputs upcast to
float64 and returns ``o``, ``lse`` (``[B, H, S]``, ``m + log2 l`` with scores in log2 units, as the kernels write
it), ``dq``, ``dk``, ``dv`` (the three column slices of the fused gradient) in closed form -- ``dV = P^T dO``,
``delta = rowsum(dO * O)``, ``dS = P * (dP - delta)``, ``dQ = scale dS K``, ``dK = scale dS^T Q``, inverse rotation,
GQA groups summed -- together with the per-element sums of absolute terms the bounds are scaled by:
``A_o = sum_j p_j |v_j|``, ``A_dv = sum_i p_ij |dO_i|``, ``A_dq = scale sum_j p_ij (|dP_ij| + |delta_i|) |k_j|``,
``A_dk`` likewise with ``|q_i|`` (each pushed through ``|cos|``, ``|sin|`` where the gradient is rotated back).

Bounds (asserted per element by ``tests/test_flash_edges_gpu.py``, shown satisfiable by ``tests/test_flash_refs.py``):

    |got - ref| <= BF16_ULP * |ref| + C[name] * A[name] + FLOOR  name in o, dq, dk, dv
    |lse - ref| <= C["lse"] * A_lse

``A_lse``: rounding ``q * scale * log2(e)`` to bf16 moves score ``j`` by at most
``d_j = 2^-8 sum_d |q_d k_jd| scale log2(e)`` (``cache_prefill_refs``' derivation), so ``m + log2 sum_j 2^(s_j - m)``
moves by at most ``max_j d_j`` over the row's visible keys; rounding ``P`` to bf16 before the row sum (v8) scales the
sum by at most ``1 + 2^-8``: ``A_lse = max_j d_j + log2(1 + 2^-8)``.  A fully masked row would be ``+inf`` in the
kernels (``lsum > 0 ? ... : INFINITY``); none occurs under causal (key 0 .. i includes i) or document masking
(``doc_start <= i``), and :func:`reference` asserts that no row is empty.

:func:`emulate` -- the kernels' rounding points in fp32 arithmetic on the CPU (one-pass maximum):

* Q times ``scale * log2(e)`` rounded to bf16: forward ``flash_attn_fwd.hip:95-99``, ``flash_attn_fwd_v4.hip:92``;
  dQ kernels ``flash_attn_bwd_split.hip:195-199``, ``flash_attn_bwd_dq16.hip:150``.  K times the same, rounded, in
  the split dK/dV kernel: ``flash_attn_bwd_split.hip:528-532``.  The fused backward scales the fp32 score instead
  (``flash_attn_bwd.hip:106``, row constant ``-lse / c`` at ``:226``): ``bwd="fused"``.
* rotated Q / K rounded to bf16 by ``rope_qk_`` (``rope="pre"``), or inside the kernels (``rope="fused"``:
  ``flash_attn_fwd.hip:95`` rotates and scales Q before its one rounding, ``:141-145`` K;
  ``flash_attn_bwd_split.hip:153, 494`` the operands staged to LDS).
* P rounded to bf16 before ``P.V`` (``flash_attn_fwd.hip:242``, ``flash_attn_fwd_v4.hip:135``) and ``P^T.dO``
  (``flash_attn_bwd_split.hip:627``, ``flash_attn_bwd.hip:283``).  The row sum adds the unrounded P in the general
  forward (``flash_attn_fwd.hip:226``, ``fwd="v2"``) and the rounded P in v8 (``flash_attn_fwd_v4.hip:139-141``,
  an MFMA over the bf16 fragments, ``fwd="v8"``).
* dS = P (dP - delta) rounded to bf16 before its MFMAs, from the unrounded P (``flash_attn_bwd_split.hip:334, 628``,
  ``flash_attn_bwd_dq16.hip:237``, ``flash_attn_bwd.hip:284``).
* O rounded to bf16 (``flash_attn_fwd.hip:266``, ``flash_attn_fwd_v4.hip:196``); ``delta`` from the bf16 O
  (``flash_attn_bwd_split.hip:203``); gradients scaled, rotated back and rounded once
  (``flash_attn_bwd_split.hip:366-378, 659-673``, ``flash_attn_bwd.hip:377-391, 419-433, 453-464``).

Not modelled (the factor 2 in ``C``): fp32 accumulation order, ``fast_exp2``, the tile-wise online softmax with the
deferred rescale (P relative to a running max up to 2^8 stale) against the one-pass maximum here.
:func:`forward_tiled` walks 64-key tiles with v8's rule (no tile max unless the tile's P sum exceeds 2^8) for the
staircase inputs and the negative tests.

MEASURED ``need[name] = max (|emulate - ref| - BF16_ULP |ref|) / A`` over every (input, form) pair of the GPU tests
(``tests/test_flash_refs.py`` recomputes it and asserts ``need <= C / 2``): see ``NEED`` below; ``C = 2 * need``
rounded up to one significant digit.
"""

from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch
from torch import Tensor

from bpe_transformer.ops import reference as R

from .decode_refs import BF16, BF16_ULP, f64, randn, rt  # noqa: F401  (rt: re-exported for the tests)

LOG2E = 1.4426950408889634
TOL_O, TOL_G = 2e-2, 3e-2  # the old global bounds (tests/test_kernels_gpu.py): max|got - ref| / max|ref|
NAMES = ("o", "dq", "dk", "dv")
# what lies below the normal range of fp32 / bf16 (2^-126) may be flushed to zero: the descending staircase takes P
# down to 2^-160, where the reference (float64) still has a value and A is as small as the value itself
FLOOR = 2.0 ** -120

# measured on the CPU (tests/test_flash_refs.py::test_need_within_half_c prints them); C = 2 * NEED, one digit, up
# o, dk, dv, lse: the look-ahead inputs (scores of +-1 vectors spread over +-8 sigma) with rotated operands; dq: a
# tiny sequence (S 17, D 128), where delta = rowsum(dO * bf16 O) cancels to far less than sum_d |dO_d O_d| and the
# rounding of O shows against an A_dq that holds |delta| only.  Random inputs alone: 0.007, 0.034, 0.013, 0.006, 0.28.
NEED = {"o": 0.0309, "dq": 0.398, "dk": 0.0584, "dv": 0.0487, "lse": 0.281}
C = {"o": 0.07, "dq": 0.8, "dk": 0.2, "dv": 0.1, "lse": 0.6}

# ------------------------------------------------------------------ shapes shared by the CPU and the GPU tests
EDGE_S = (64, 65, 127, 128, 129, 136, 200, 257)
TINY_S = (1, 2, 15, 17, 31, 33, 63)
STAIR_S = 320
STEPS = (7, 9, -7, -40, 100)
HEADS = ((2, 2), (4, 2), (8, 1))
# document lengths per batch row: edges at and one off 32 / 64 / 128, documents of length 1
DOCS = {
    "d257": ((1, 31, 31, 1, 65, 128), (31, 2, 32, 62, 1, 129)),   # starts 1 32 63 64 129 / 31 33 65 127 128
    "d200": ((64, 1, 63, 72), (33, 95, 72)),                      # starts 64 65 128 / 33 128
    "d129": ((129,), (128, 1)),
}

# kernel forms: name -> (fa_fwd_config, fa_bwd_config, fa_dq_config, emulate fwd, emulate bwd)
FORMS = {
    "v8+split32": (8, 0, 0, "v8", "split"),
    "v8+dq16nw8": (8, 0, 1, "v8", "split"),
    "v8+dq16nw4": (8, 0, 2, "v8", "split"),
    "v2+split32": (2, 0, 0, "v2", "split"),
    "v2rope+splitrope": (8, 0, 0, "v2", "split"),   # D 64, rope == 1: both rotate inside the kernels
    "d128+split": (8, 0, 0, "v2", "split"),         # D 128 (rope == 1: fa_bwd rotates a copy)
    "v8+fused": (8, 1, 0, "v8", "split"),           # D 64 fused atomics (fwd v2 under rope == 1)
    "d128+fused": (8, 1, 0, "v2", "fused"),         # D 128, rope == 1
    "doc": (8, 0, 0, "v2", "split"),
    "public": (8, 0, 3, "v8", "split"),             # ops.flash_attention_qkv with autograd, default selectors
}


def forms_for(case, public: bool = False) -> list[str]:
    """The forms that accept ``case``."""
    if case.doc is not None:
        return ["doc"] + (["public"] if public else [])
    if case.D == 128:
        out = ["d128+split"] + (["d128+fused"] if case.rope == "fused" else [])
    elif case.rope == "fused":
        out = ["v2rope+splitrope", "v8+fused"]
    else:
        out = ["v8+split32", "v8+dq16nw8", "v8+dq16nw4", "v2+split32", "v8+fused"]
    return out + (["public"] if public and case.rope != "fused" else [])


def emu_form(case, form: str) -> tuple[str, str]:
    fwd, bwd = FORMS[form][3:]
    if form in ("v8+fused", "public") and (case.rope == "fused" or case.D == 128 or case.doc is not None):
        fwd = "v2"
    if form == "v8+fused":
        bwd = "fused"
    return fwd, bwd


# ------------------------------------------------------------------ helpers
def _rot(x: Tensor, cos: Tensor, sin: Tensor, inverse: bool = False) -> Tensor:
    """Interleaved pairs of ``x [..., S, D]`` rotated by the table angle at positions 0..S-1 (``apply_rope``)."""
    S = x.shape[-2]
    c, s = cos[:S].to(x.dtype), sin[:S].to(x.dtype)
    if inverse:
        s = -s
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).flatten(-2)


def _rot_abs(a: Tensor, cos: Tensor, sin: Tensor) -> Tensor:
    S = a.shape[-2]
    c, s = cos[:S].to(a.dtype).abs(), sin[:S].to(a.dtype).abs()
    a1, a2 = a[..., 0::2], a[..., 1::2]
    return torch.stack((a1 * c + a2 * s, a1 * s + a2 * c), dim=-1).flatten(-2)


def doc_start_of(rows) -> Tensor:
    """int32 ``[B, S]`` doc_start of ``tests/test_doc_mask_gpu.bounds_from_lengths``."""
    from .test_doc_mask_gpu import bounds_from_lengths
    return bounds_from_lengths([list(r) for r in rows], "cpu")[0]


def visible(B: int, S: int, causal: bool, doc_start: Tensor | None, extra: int = 0) -> Tensor:
    """bool ``[B, S, S]``: query i sees key j.  ``extra = 1`` (negative tests): a causal limit one too far on the
    last row of a diagonal tile from row 127 on (``i % 64 == 63``: key ``i + 1`` opens the next tile), where the
    stray weight is one among 128 or more."""
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    edge = (i % 64 == 63) & (i >= 127)
    vis = (j <= i + extra * edge) if causal else torch.ones(S, S, dtype=torch.bool)
    vis = vis[None].expand(B, S, S).clone()
    if doc_start is not None:
        vis &= j[None] >= doc_start.long()[:, :, None]
    return vis


def _split(x: Tensor, B, S, H, Hkv, D):
    x = x.reshape(B, S, H + 2 * Hkv, D)
    return x[:, :, :H].transpose(1, 2), x[:, :, H:H + Hkv].transpose(1, 2), x[:, :, H + Hkv:].transpose(1, 2)


def _rows(t: Tensor) -> Tensor:
    """``[B, heads, S, D]`` -> ``[B*S, heads*D]``."""
    B, h, S, D = t.shape
    return t.transpose(1, 2).reshape(B * S, h * D)


# ------------------------------------------------------------------ float64 reference
def reference(qkv: Tensor, dout: Tensor, B: int, S: int, H: int, Hkv: int, D: int, cos: Tensor | None = None,
              sin: Tensor | None = None, causal: bool = True, doc_start: Tensor | None = None,
              scale: float | None = None) -> dict[str, Tensor]:
    G = H // Hkv
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    q, k, v = _split(f64(qkv), B, S, H, Hkv, D)
    if cos is not None:
        cos, sin = f64(cos), f64(sin)
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
    kg, vg = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    vis = visible(B, S, causal, doc_start)[:, None]
    assert bool(vis.any(-1).all()), "a query row sees no key"
    s = (q @ kg.transpose(-1, -2) * (scale * LOG2E)).masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    out = {"lse": (m + torch.log2(l)).squeeze(-1), "P": P}
    d = (2.0 ** -8 * scale * LOG2E) * (q.abs() @ kg.abs().transpose(-1, -2)).masked_fill(~vis, 0.0)
    out["A_lse"] = d.amax(-1) + math.log2(1 + 2.0 ** -8)
    o = P @ vg
    out["o"], out["A_o"] = _rows(o), _rows(P @ vg.abs())
    do = f64(dout).view(B, S, H, D).transpose(1, 2)
    dP = do @ vg.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    aS = P * (dP.abs() + delta.abs())
    dq, a_dq = scale * dS @ kg, scale * aS @ kg.abs()
    dk, a_dk = scale * dS.transpose(-1, -2) @ q, scale * aS.transpose(-1, -2) @ q.abs()
    dv, a_dv = P.transpose(-1, -2) @ do, P.transpose(-1, -2) @ do.abs()
    if cos is not None:
        dq, dk = _rot(dq, cos, sin, inverse=True), _rot(dk, cos, sin, inverse=True)
        a_dq, a_dk = _rot_abs(a_dq, cos, sin), _rot_abs(a_dk, cos, sin)
    grp = lambda t: t.view(B, Hkv, G, S, D).sum(2)  # noqa: E731
    out["dq"], out["A_dq"] = _rows(dq), _rows(a_dq)
    out["dk"], out["A_dk"] = _rows(grp(dk)), _rows(grp(a_dk))
    out["dv"], out["A_dv"] = _rows(grp(dv)), _rows(grp(a_dv))
    return out


# ------------------------------------------------------------------ the kernels' rounding points
def _bf(t: Tensor) -> Tensor:
    return t.to(BF16).float()


def _emu_operands(case):
    """-> q (bf16 values the dK/dV kernel reads), qs (the scaled, rounded Q), k, v; fp32 ``[B, heads, S, D]``."""
    B, S, H, Hkv, D = case.B, case.S, case.H, case.Hkv, case.D
    q, k, v = _split(case.qkv.float(), B, S, H, Hkv, D)
    sc = torch.tensor(float(torch.tensor(case.scale, dtype=torch.float32)) * LOG2E, dtype=torch.float32)
    if case.rope == "pre":
        q, k = _bf(_rot(q, case.cos, case.sin)), _bf(_rot(k, case.cos, case.sin))
        qs = _bf(q * sc)
    elif case.rope == "fused":
        qr = _rot(q, case.cos, case.sin)
        q, qs, k = _bf(qr), _bf(qr * sc), _bf(_rot(k, case.cos, case.sin))
    else:
        qs = _bf(q * sc)
    return q, qs, k, v, sc


def emulate(case, fwd: str = "v8", bwd: str = "split", defect: str | None = None) -> dict[str, Tensor]:
    """bf16 ``o``, ``dq``, ``dk``, ``dv`` and fp32 ``lse`` with the rounding points of the module docstring.
    ``defect`` (negative tests): ``"causal+1"`` a causal limit one too far (:func:`visible`), ``"doc-1"`` a document limit one too far
    down, ``"lse"`` an LSE 0.05 too large in the forward's output and in the backward that reads it (P there is
    formed from the true one: both kernels share the error)."""
    B, S, H, Hkv, D = case.B, case.S, case.H, case.Hkv, case.D
    G = H // Hkv
    q, qs, k, v, sc = _emu_operands(case)
    kg, vg = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    ds = case.doc_start
    if defect == "doc-1":
        ds = (ds - 1).clamp_min(0)
    vis = visible(B, S, case.causal, ds, extra=1 if defect == "causal+1" else 0)[:, None]
    ninf = float("-inf")
    s = (qs @ kg.transpose(-1, -2)).masked_fill(~vis, ninf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    pb = _bf(p)
    l = (pb if fwd == "v8" else p).sum(-1, keepdim=True)
    o = _bf(pb @ vg / l)
    lse = m + torch.log2(l)
    do = case.dout.float().view(B, S, H, D).transpose(1, 2)
    delta = (do * o).sum(-1, keepdim=True)
    dp = do @ vg.transpose(-1, -2) - delta
    if bwd == "split":
        pq = torch.exp2(s - lse)                                           # dQ kernel: scaled bf16 Q
        ksg = _bf(k * sc).repeat_interleave(G, 1)                          # dK/dV kernel: scaled bf16 K
        pk = torch.exp2((q @ ksg.transpose(-1, -2)).masked_fill(~vis, ninf) - lse)
    else:
        pq = pk = torch.exp2(((q @ kg.transpose(-1, -2)).masked_fill(~vis, ninf) - lse / sc) * sc)
    dsq, dsk = _bf(pq * dp), _bf(pk * dp)
    dq = case.scale * (dsq @ kg)
    grp = lambda t: t.view(B, Hkv, G, S, D).sum(2)  # noqa: E731
    dk = case.scale * grp(dsk.transpose(-1, -2) @ q)
    dv = grp(_bf(pk).transpose(-1, -2) @ do)
    if case.rope is not None:
        dq, dk = _rot(dq, case.cos, case.sin, inverse=True), _rot(dk, case.cos, case.sin, inverse=True)
    out = {"o": _rows(o).to(BF16), "lse": lse.squeeze(-1) + (0.05 if defect == "lse" else 0.0),
           "dq": _rows(dq).to(BF16), "dk": _rows(dk).to(BF16), "dv": _rows(dv).to(BF16)}
    return out


def forward_tiled(case, defect: str | None = None) -> dict[str, Tensor]:
    """The v8 forward tile by tile (64 keys; ``flash_attn_fwd_v4.hip:144-172``): P relative to the running ``m``; a
    tile whose rounded-P sum exceeds 2^8 -- and the first -- takes its max ``d``, ``m += d``, O and the row sum are
    scaled by ``alpha = 2^-d`` and P is formed again.  ``defect="alpha"``: O is not rescaled (the row sum is);
    ``"overread"``: the ragged last tile admits key ``S``, which in the fused layout is the next sequence's row 0
    (zeros after the last sequence).  -> bf16 ``o``, fp32 ``lse``."""
    B, S, H, Hkv, D = case.B, case.S, case.H, case.Hkv, case.D
    G = H // Hkv
    _, qs, k, v, _ = _emu_operands(case)
    nk = S
    vis = visible(B, S, case.causal, case.doc_start)
    if defect == "overread":
        nxt = lambda t: torch.cat([t[1:, :, :1], torch.zeros_like(t[:1, :, :1])])  # noqa: E731
        k, v, nk = torch.cat([k, nxt(k)], 2), torch.cat([v, nxt(v)], 2), S + 1
        vis = torch.cat([vis, torch.full((B, S, 1), not case.causal)], 2)
    kg, vg = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    s = (qs @ kg.transpose(-1, -2)).masked_fill(~vis[:, None], float("-inf"))
    m = torch.zeros(B, H, S, 1)
    l = torch.zeros(B, H, S, 1)
    o = torch.zeros(B, H, S, D)
    for t0 in range(0, nk, 64):
        st = s[..., t0:t0 + 64]
        pb = _bf(torch.exp2(st - m))
        lt = pb.sum(-1, keepdim=True)
        grow = ~(lt <= 256.0) if t0 else torch.ones_like(lt, dtype=torch.bool)
        d = torch.where(grow, (st - m).amax(-1, keepdim=True), torch.zeros_like(m))
        d = torch.where(torch.isinf(d), torch.zeros_like(d), d)  # (a fully masked tile: nothing to move to)
        alpha = torch.exp2(-d) if t0 else torch.zeros_like(d)
        m = m + d
        pb = _bf(torch.exp2(st - m))
        l = l * alpha + pb.sum(-1, keepdim=True)
        o = (o if defect == "alpha" else o * alpha) + pb @ vg[:, :, t0:t0 + 64]
    return {"o": _rows(o / l).to(BF16), "lse": (m + torch.log2(l)).squeeze(-1)}


# ------------------------------------------------------------------ error measures
def global_rel(got: Tensor, ref: Tensor) -> float:
    """``max|got - ref| / max|ref|``; NaN in ``got`` -> inf."""
    e = (f64(got).reshape(ref.shape) - ref).abs().nan_to_num(nan=math.inf)
    return float(e.max() / ref.abs().max().clamp_min(1e-300))


def need_of(got: Tensor, ref: Tensor, A: Tensor) -> float:
    """Worst element ``(|got - ref| - 2^-7 |ref| - FLOOR) / A``; NaN -> inf."""
    err = (f64(got).reshape(ref.shape) - ref).abs().nan_to_num(nan=math.inf)
    return float(((err - BF16_ULP * ref.abs() - FLOOR) / A.clamp_min(1e-300)).max())


def lse_need(got: Tensor, ref: dict) -> float:
    err = (f64(got) - ref["lse"]).abs().nan_to_num(nan=math.inf)
    return float((err / ref["A_lse"]).max())


def measures(got: dict, ref: dict) -> dict[str, tuple[float, float]]:
    """name -> (global rel, need) for every output present in ``got`` (lse: (max abs error, need))."""
    out = {n: (global_rel(got[n], ref[n]), need_of(got[n], ref[n], ref["A_" + n])) for n in NAMES if n in got}
    if "lse" in got:
        out["lse"] = (float((f64(got["lse"]) - ref["lse"]).abs().nan_to_num(nan=math.inf).max()), lse_need(got["lse"], ref))
    return out


def check(got: dict, ref: dict, what: str = "", old: bool = False) -> dict[str, tuple[float, float]]:
    """Assert the per-element bounds of the module docstring and, with ``old``, the old global bounds (they mean
    nothing where the reference is all but zero: the gradients of a one-hot softmax); -> :func:`measures`."""
    ms = measures(got, ref)
    for n, (g, need) in ms.items():
        if n != "lse" and old:
            assert g < (TOL_O if n == "o" else TOL_G), (what, n, "global", g)
        assert need <= C[n], (what, n, "per element", need, C[n])
    return ms


# ------------------------------------------------------------------ input builders (cached: treat as read-only)
def _case(qkv, dout, B, S, H, Hkv, D, causal, rope, doc, scale=None, **kw):
    cos = sin = None
    if rope is not None:
        cos, sin = R.rope_tables(D, S + 16, 10000.0)
    ds = None if doc is None else doc_start_of(DOCS[doc])
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    c = SimpleNamespace(qkv=qkv, dout=dout, B=B, S=S, H=H, Hkv=Hkv, D=D, causal=causal, rope=rope, doc=doc,
                        doc_start=ds, doc_rows=None if doc is None else DOCS[doc], cos=cos, sin=sin, scale=scale,
                        **kw)
    c.ref = reference(qkv, dout, B, S, H, Hkv, D, cos, sin, causal, ds, scale)
    return c


@functools.lru_cache(maxsize=None)
def random_case(S: int, H: int, Hkv: int, D: int, causal: bool = True, rope: str | None = None, doc: str | None = None,
                B: int = 2):
    W = (H + 2 * Hkv) * D
    qkv = randn(B * S, W, seed=(S, H, D, 1))
    dout = randn(B * S, H * D, seed=(S, H, D, 2))
    return _case(qkv, dout, B, S, H, Hkv, D, causal, rope, doc)


POW2_SCALE = 0.125 / LOG2E  # fp32(scale) * fp32(log2 e) = 0.125 (1 + O(2^-24)): the rounded scaled Q is q / 8 exactly


def _signs(*shape: int, seed) -> Tensor:
    return torch.sign(randn(*shape, seed=seed).float() + 1e-3)


@functools.lru_cache(maxsize=None)
def dominant_case(S: int, H: int, D: int, shift: int, causal: bool = True, rope: str | None = None, B: int = 2,
                  factor: float = 8.0):
    """G = 1.  Queries are +-1 vectors (``|q|^2 = D`` exactly, ``q_i . q_j ~ N(0, D)``); every key is a random row
    scaled by 0.1 except the heavy ones.  Causal, ``shift = 0``: key ``i`` is ``factor * q_i`` -- its score
    ``factor sqrt(D)`` stands ``factor (D - q_i . q_j) / sqrt(D)`` above any other heavy key's, so ``o_i = v_i``.
    ``shift = 1``: the heavy key of query ``i`` is key ``i + 1``, invisible to it (the forward look-ahead trap of
    ``cache_prefill_refs.dominant_case``).  Non-causal: sequence 0's queries are one +-1 vector per head plus 0.1
    noise, its key ``S - 1`` is ``factor`` times that vector (the last valid key must be admitted), and key 0 of
    sequence 1 -- row ``S`` of the fused layout -- is twice as heavy (``S`` must not be).
    -> case with ``rows``: what ``o`` must equal for ``shift = 0`` (float64, NaN where nothing is claimed)."""
    W = 3 * H * D
    x = randn(B * S, W, seed=(S, D, shift, 5)).float().view(B, S, 3 * H, D)
    x[:, :, H:2 * H] *= 0.1
    rows = torch.full((B, S, H, D), float("nan"), dtype=torch.float64)
    if causal:
        x[:, :, :H] = _signs(B, S, H, D, seed=(S, D, shift, 6))
        x[:, shift:, H:2 * H] = factor * x[:, :S - shift, :H]
        if shift == 0:
            rows = f64(x[:, :, 2 * H:].to(BF16))
    else:
        u = _signs(1, 1, H, D, seed=(S, D, 7))
        x[0, :, :H] = u + 0.1 * x[0, :, :H]
        x[0, S - 1, H:2 * H] = factor * u[0, 0]
        x[1, :, :H] *= 0.05  # (moderate scores against its heavy key 0)
        x[1, 0, H:2 * H] = 2 * factor * u[0, 0]
        rows[0] = f64(x[0, S - 1, 2 * H:].to(BF16))
    qkv = x.view(B * S, W).to(BF16)
    dout = randn(B * S, H * D, seed=(S, D, shift, 8))
    return _case(qkv, dout, B, S, H, H, D, causal, rope, None, scale=POW2_SCALE, rows=rows.reshape(B * S, H * D),
                 shift=shift)




@functools.lru_cache(maxsize=None)
def staircase_case(step: int, causal: bool = True, plateau: bool = False, H: int = 2, B: int = 2):
    """D = 64, S = 320 (five 64-key tiles).  ``q = 8 e_0`` and ``k_j = b_j e_0`` with ``scale log2(e) = 1/8``: the
    log2-unit score of key ``j`` is ``b_j`` exactly (bf16 operands ``1`` / ``b_j`` or ``8`` / ``b_j / 8``, one
    product).  ``b_j = t * step`` in tile ``t``; ``plateau``: ``b = 0, 0, 3, 3, 0`` -- tile 2 holds 64 keys each 3
    above the running max, P sum ``64 * 8 = 2^9 > 2^8`` with no score above the threshold.  V rows are random plus
    ``2 t`` per tile, so a wrong ``alpha`` shows in O.  ``scores``: the exact per-key score, float64 ``[S]``."""
    S, D = STAIR_S, 64
    W = 3 * H * D
    x = torch.zeros(B, S, 3 * H, D)
    t = torch.arange(S) // 64
    b = torch.tensor([0.0, 0.0, 3.0, 3.0, 0.0])[t] if plateau else (t * step).float()
    x[:, :, :H, 0] = 8.0
    x[:, :, H:2 * H, 0] = b[None, :, None]
    x[:, :, 2 * H:] = randn(B, S, H, D, seed=(step, 9)).float() + 2.0 * t.float()[None, :, None, None]
    dout = randn(B * S, H * D, seed=(step, 10))
    return _case(x.view(B * S, W).to(BF16), dout, B, S, H, H, D, causal, None, None, scale=POW2_SCALE,
                 scores=b.double())


def zero_sets(case, nonzero_rows: Tensor) -> tuple[Tensor, Tensor]:
    """bool ``[B*S]`` x 2: the query rows whose dQ, and the key rows whose dK / dV, are exactly zero when ``dout`` is
    nonzero only in ``nonzero_rows [B, S]``: dP = delta = 0 gives dS = 0 for a zero-``dout`` query, and a key seen
    by such queries only receives nothing."""
    vis = visible(case.B, case.S, case.causal, case.doc_start)
    seen = (vis & nonzero_rows[:, :, None]).any(1)  # [B, key]
    return (~nonzero_rows).reshape(-1), (~seen).reshape(-1)


@functools.lru_cache(maxsize=None)
def one_hot_dout(S: int, H: int, Hkv: int, D: int, j0: int, rope: str | None = None, doc: str | None = None,
                 B: int = 2):
    """``random_case`` with ``dout`` zeroed outside query rows ``i < j0`` (plain causal) or outside the third
    document of each batch row (``doc``; the second where a row has two).  -> case with ``zero_q``, ``zero_k``."""
    base = random_case(S, H, Hkv, D, True, rope, doc, B)
    nz = torch.zeros(B, S, dtype=torch.bool)
    if doc is None:
        nz[:, :j0] = True
    else:
        for b, lens in enumerate(DOCS[doc]):
            i = min(2, len(lens) - 1)
            nz[b, sum(lens[:i]):sum(lens[:i + 1])] = True
    dout = base.dout.clone()
    dout[~nz.reshape(-1)] = 0
    c = _case(base.qkv, dout, B, S, H, Hkv, D, True, rope, doc)
    c.nonzero = nz
    c.zero_q, c.zero_k = zero_sets(c, nz)
    return c


POISONS = ("nan", "inf", "big")


@functools.lru_cache(maxsize=None)
def poisoned_neighbour(S: int, H: int, Hkv: int, D: int, kind: str, causal: bool = True, rope: str | None = None,
                       doc: str | None = None, pad: int = 0, B: int = 3):
    """-> (poisoned case, twin case, keep): sequence 1's Q / K / V rows hold NaN (``"nan"``), ``+-inf`` alternating
    (``"inf"``) or ``+-3e38`` (``"big"``) in the first and ``randn`` in the twin; ``keep [B*S]`` marks the rows of
    sequences 0 and 2.  ``pad > 0``: each qkv is the column slice ``buf[:, :W]`` of a NaN-filled ``[B*S, W + pad]``
    buffer (``stride(0) % 8 == 0``).  The cases carry no reference (sequence 1 has none)."""
    W = (H + 2 * Hkv) * D
    assert (W + pad) % 8 == 0
    twin = randn(B * S, W, seed=(S, H, D, 11))
    bad = twin.clone()
    sgn = torch.ones(S, W)
    sgn[:, 1::2] = -1
    fill = {"nan": torch.full((S, W), float("nan")), "inf": sgn * float("inf"), "big": sgn * 3e38}[kind]
    bad[S:2 * S] = fill.to(BF16)
    dout = randn(B * S, H * D, seed=(S, H, D, 12))
    keep = torch.ones(B, S, dtype=torch.bool)
    keep[1] = False

    def mk(x):
        if pad:
            buf = torch.full((B * S, W + pad), float("nan"), dtype=BF16)
            buf[:, :W] = x
            x = buf[:, :W]
        cos = sin = None
        if rope is not None:
            cos, sin = R.rope_tables(D, S + 16, 10000.0)
        rows = None if doc is None else DOCS[doc] + DOCS[doc][:1]
        ds = None if doc is None else doc_start_of(rows)
        return SimpleNamespace(qkv=x, dout=dout, B=B, S=S, H=H, Hkv=Hkv, D=D, causal=causal, rope=rope, doc=doc,
                               doc_start=ds, doc_rows=rows, cos=cos, sin=sin, scale=1.0 / math.sqrt(D))

    return mk(bad), mk(twin), keep.reshape(-1)


# ------------------------------------------------------------------ the case lists of the GPU tests
def _cyc(seq, i):
    return seq[i % len(seq)]


def random_list() -> list[tuple]:
    """(S, H, Hkv, D, causal, rope, doc): every edge S with the three D = 64 RoPE modes, causal; one non-causal and
    one D = 128 each, heads and the remaining modes cycled; an odd GQA group (3, 1); the document layouts."""
    out = []
    for i, S in enumerate(EDGE_S):
        H, Hkv = _cyc(HEADS, i)
        out += [(S, H, Hkv, 64, True, r, None) for r in (None, "pre", "fused")]
        out.append((S, H, Hkv, 64, False, _cyc(("pre", None, "fused"), i), None))
        out.append((S, *_cyc(HEADS, i + 1), 128, i % 4 != 3, _cyc((None, "pre", "fused"), i), None))
    out += [(129, 3, 1, 64, True, "pre", None), (200, 3, 1, 128, True, None, None)]
    out += [(257, 4, 2, 64, True, "pre", "d257"), (257, 2, 2, 64, True, None, "d257"), (200, 4, 2, 128, True, "pre", "d200"),
            (200, 3, 1, 64, True, None, "d200"), (129, 8, 1, 64, True, "pre", "d129")]
    return out


def dominant_list() -> list[tuple]:
    """(S, H, D, shift, causal, rope)."""
    out = []
    for i, S in enumerate(EDGE_S):
        D = 128 if i % 4 == 2 else 64
        out += [(S, 2, D, 0, True, None), (S, 2, D, 1, True, _cyc((None, "pre"), i)), (S, 2, D, 0, False, None)]
    return out


def staircase_list() -> list[tuple]:
    """(step, causal, plateau)."""
    return [(s, c, False) for s in STEPS for c in (True, False)] + [(0, True, True), (0, False, True)]


def zero_dout_list() -> list[tuple]:
    """(S, H, Hkv, D, j0, rope, doc): j0 at and one off each tile edge (32-row steps, 64 / 128-row tiles)."""
    out = []
    for i, j0 in enumerate((31, 32, 33, 63, 64, 65, 127, 128, 129)):
        out.append((200, *_cyc(HEADS, i), 64, j0, _cyc((None, "pre", "fused"), i), None))
    out += [(200, 2, 2, 128, 64, "pre", None), (200, 4, 2, 128, 129, "fused", None), (136, 2, 2, 64, 128, None, None)]
    out += [(257, 4, 2, 64, 0, "pre", "d257"), (200, 2, 2, 128, 0, None, "d200")]
    return out


def poison_list() -> list[tuple]:
    """(S, H, Hkv, D, kind, causal, rope, doc, pad): S no multiple of 64 / of 128, each kind, both strides."""
    out = []
    for i, (S, kind) in enumerate([(65, "nan"), (129, "nan"), (200, "inf"), (136, "big"), (63, "nan"), (257, "inf")]):
        H, Hkv = _cyc(HEADS, i)
        for pad in (0, 8):
            out.append((S, H, Hkv, 64, kind, True, _cyc((None, "pre", "fused"), i), None, pad))
        out.append((S, H, Hkv, 64, kind, False, _cyc(("pre", None), i), None, 8 * (i % 2)))
        out.append((S, H, Hkv, 128, kind, i % 2 == 0, _cyc(("fused", None, "pre"), i), None, 8 * (i % 2)))
    out += [(200, 4, 2, 64, "nan", True, "pre", "d200", 8), (200, 2, 2, 128, "nan", True, None, "d200", 0)]
    return out


def tiny_list() -> list[tuple]:
    """(S, H, Hkv, D, causal, rope)."""
    out = []
    for i, S in enumerate(TINY_S):
        out += [(S, *_cyc(HEADS, i), 64, True, _cyc((None, "pre"), i)), (S, 2, 2, 64, True, "fused"),
                (S, *_cyc(HEADS, i + 1), 64, False, None), (S, *_cyc(HEADS, i + 2), 128, True, _cyc(("pre", "fused", None), i))]
    return out


def checked_inputs():
    """Every (label, case) whose outputs the GPU tests compare with the float64 reference."""
    for a in random_list():
        yield f"random{a}", random_case(*a)
    for a in dominant_list():
        yield f"dominant{a}", dominant_case(*a)
    for a in staircase_list():
        yield f"staircase{a}", staircase_case(*a)
    for a in tiny_list():
        yield f"tiny{a}", random_case(*a)
