"""Inputs, bounds and a rounding emulation for the flash prefill over the KV cache (``csrc/flash_attn_cache.hip``).

The float64 references are ``decode_refs.decode_attention`` (any ``T``) and ``ragged_refs.decode_attention``; they
give the reference ``o`` and ``A = sum_j p_j |V_j| / l``.  Added here:

* :func:`emulate` -- the kernel's own rounding points in plain PyTorch: ``q * scale * log2(e)`` rounded to bf16,
  fp32 scores in log2 units, ``P = exp2(s - m)`` rounded to bf16 before ``P.V`` while the row sum ``l`` adds the
  unrounded fp32 ``P``, fp32 accumulation, one bf16 rounding of ``o / l``.  ``tests/test_cache_prefill_refs.py``
  runs it over every input of the GPU tests and asserts the GPU tests' bounds on it, so inputs and bounds are known
  to be satisfiable before a GPU sees them.
* :func:`dominant_case` -- ``decode_refs.dominant_case`` extended to ``T`` tokens: key ``p0 + t + shift`` is
  ``factor * q[t]``, every other old key is scaled by 0.1.  ``shift = 0``: token ``t``'s own key carries the whole
  mass, so ``o[t] = V[p0 + t]``.  ``shift = 1``: the heavy key is the NEXT token's -- finite, inside the slab's
  extent, and invisible to token ``t``; a kernel whose causal limit is one too far returns ``V[p0 + t + 1]``.
* :func:`dominant_extra` -- what the bf16 ``q`` and ``P`` add to the dominant-key bound, derived: rounding
  ``q * scale * log2(e)`` to bf16 moves score ``j`` by at most ``d_j = 2^-8 sum_d |q_d k_jd| scale log2(e)`` (half
  an ulp of 2^-8 relative per element, taken whole), so the weight of key ``j`` relative to the dominant key ``k``
  changes by a factor of at most ``2^(d_j + d_k)``, and by ``1 + 2^-8`` more when ``P`` is rounded.  With
  ``g_j = 2^(d_j + d_k) (1 + 2^-8) - 1`` the output moves by at most ``sum_{j != k} p_j g_j (|V_j| + |V_k|)``
  (the weight change itself plus the renormalisation it causes).  Zero when the dominant key holds all the mass.
* the shape lists of the GPU tests, so that the CPU test walks exactly the same cases.
"""

from __future__ import annotations

import functools
import math

import torch
from torch import Tensor

from . import decode_refs as DR
from . import ragged_refs as RR
from .decode_refs import BF16, f64

LOG2E = 1.4426950408889634
TOL_GLOBAL = 2e-2  # max|got - ref| / max|ref| of the flash forward (tests/test_kernels_gpu.py)
TOL_KERNELS = 1e-2  # against another kernel on the same inputs (test_fa_fwd_v8_matches_v2)
TOL32 = 1e-5  # the project's fp32 threshold (tests/test_decode_kernels_gpu.py)

LMAX = 448
LENGTHS = [(T, p0) for T in (9, 31, 32, 33, 64, 65, 128, 129, 200) for p0 in (0, 1, 63, 64, 65, 200)
           if p0 + T <= LMAX]
GROUPS = (1, 2, 3, 4, 8)
RAGGED_POS = [0, 5, 63, 64, 130]
RAGGED_T = 70
DOMINANT = [(64, 65, 63), (64, 33, 200), (128, 129, 1)]  # (D, T, p0) of the dominant-key / look-ahead cases


@functools.lru_cache(maxsize=None)
def length_case(D: int, T: int, p0: int, Lmax: int = LMAX, G: int = 1, B: int = 2, Hkv: int = 2):
    """-> (q, K, V, H, ref o, A): random inputs, poison from row ``p0 + T`` on.  Cached: treat as read-only."""
    H = Hkv * G
    q = DR.queries(B, T, H, D, seed=p0 + Lmax + T)
    k, v = DR.caches(B, Hkv, Lmax, D, p0 + T, seed=p0 + T)
    ref, A = DR.decode_attention(f64(q), f64(k), f64(v), p0, H, T)
    return q, k, v, H, ref, A


@functools.lru_cache(maxsize=None)
def ragged_case(D: int = 64, G: int = 2, Hkv: int = 2, Lmax: int = LMAX):
    q, k, v, H = RR.attention_case(Hkv, G, D, Lmax, RAGGED_POS, RAGGED_T)
    ref, A = RR.decode_attention(q, k, v, RAGGED_POS, H, RAGGED_T)
    return q, k, v, H, ref, A


def full_case(D: int = 64, Lmax: int = 200, T: int = 10, B: int = 2, Hkv: int = 2):
    """``p0 = Lmax - 3``: three tokens fit, seven were dropped by ``kv_append``.  -> (q, K, V, H, p0, n, ref o, A)
    with the reference over the ``n = 3`` written tokens only (rows ``b * T + t``, ``t < n``, of the output)."""
    p0, n = Lmax - 3, 3
    q = DR.queries(B, T, Hkv, D, seed=991)
    k, v = DR.caches(B, Hkv, Lmax, D, Lmax, seed=991)
    qn = q.view(B, T, -1)[:, :n].reshape(B * n, -1)
    ref, A = DR.decode_attention(f64(qn), f64(k), f64(v), p0, Hkv, n)
    return q, k, v, Hkv, p0, n, ref, A


@functools.lru_cache(maxsize=None)
def dominant_case(D: int, T: int, p0: int, shift: int, Lmax: int = LMAX, B: int = 2, Hkv: int = 2,
                  factor: float = 8.0):
    """G = 1.  -> (q, K, V, ref o, A, rows): ``rows [B*T, H*D]`` are ``V[p0 + t + shift]`` laid out like ``o``
    (``shift = 0``: what ``o`` must be; ``shift = 1``: what a look-ahead kernel returns; the last token has no
    next one and gets NaN there).  ``factor = 8``: the heavy score is ``8 |q|^2 / sqrt(D) ~ 8 sqrt(D)``, the other
    new tokens' keys score ``8 q.q' / sqrt(D) ~ 8 N(0, 1)``, so even a 5-sigma one is e^-24 of the heavy one."""
    H = Hkv
    L = p0 + T
    q = DR.queries(B, T, H, D, seed=7 * p0 + T + shift)
    k, v = DR.caches(B, Hkv, Lmax, D, L, seed=7 * p0 + T + shift)
    k[:, :, :L] = (0.1 * k[:, :, :L].float()).to(BF16)
    qv = q.view(B, T, Hkv, D)
    n = T - shift
    k[:, :, p0 + shift:L] = (factor * qv[:, :n].float()).transpose(1, 2).to(BF16)
    rows = torch.full((B, T, Hkv, D), float("nan"), dtype=torch.float64)
    rows[:, :n] = f64(v[:, :, p0 + shift:L]).transpose(1, 2)
    ref, A = DR.decode_attention(f64(q), f64(k), f64(v), p0, H, T)
    return q, k, v, ref, A, rows.reshape(B * T, H * D)


def dominant_extra(q: Tensor, k: Tensor, v: Tensor, p0: int, T: int) -> Tensor:
    """The derived bf16-q / bf16-P term of the dominant-key bound (module docstring), ``[B*T, H*D]``; G = 1, token
    ``t``'s dominant key is ``p0 + t``."""
    B, Hkv, _, D = k.shape
    q, k, v = f64(q).view(B, T, Hkv, D), f64(k), f64(v)
    sc = LOG2E / math.sqrt(D)
    out = torch.zeros(B, T, Hkv, D, dtype=torch.float64)
    for t in range(T):
        n = p0 + t + 1
        s = torch.einsum("bhd,bhld->bhl", q[:, t], k[:, :, :n]) * sc  # log2 units
        d = 2.0 ** -8 * torch.einsum("bhd,bhld->bhl", q[:, t].abs(), k[:, :, :n].abs()) * sc
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        p = p / p.sum(-1, keepdim=True)
        g = torch.exp2(d + d[..., -1:]) * (1 + 2.0 ** -8) - 1
        w = (p * g)[..., :-1]  # every key but the dominant (last visible) one
        out[:, t] = torch.einsum("bhl,bhld->bhd", w, v[:, :, :n - 1].abs()) + w.sum(-1, keepdim=True) * v[:, :, n - 1].abs()
    return out.reshape(B * T, Hkv * D)


def dominant_bound(rows: Tensor, ref: Tensor, A: Tensor, extra: Tensor) -> Tensor:
    """``|got - V[p0 + t]|`` per element: one bf16 ulp of the row, the reference's own distance from it, the
    derived bf16 term, and the fp32 accumulation."""
    return DR.BF16_ULP * rows.abs() + (ref - rows).abs() + extra + TOL32 * A


# ------------------------------------------------------------------ the kernel's rounding points
def _emulate_one(q: Tensor, k: Tensor, v: Tensor, p0: int, H: int, T: int, scale: float | None) -> Tensor:
    B, Hkv, Lmax, D = k.shape
    G = H // Hkv
    sc = (1.0 / math.sqrt(D) if scale is None else scale) * LOG2E
    qs = (q.float() * torch.tensor(sc, dtype=torch.float32)).to(BF16).float().view(B, T, Hkv, G, D)
    L = min(p0 + T, Lmax)
    s = torch.einsum("bthgd,bhld->bthgl", qs, k[:, :, :L].float())
    visible = torch.arange(L)[None, :] <= (p0 + torch.arange(T))[:, None]
    s = s.masked_fill(~visible[None, :, None, None, :], float("-inf"))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    o = torch.einsum("bthgl,bhld->bthgd", p.to(BF16).float(), v[:, :, :L].float())
    return (o / p.sum(-1, keepdim=True)).reshape(B * T, H * D).to(BF16)


def emulate(q: Tensor, k: Tensor, v: Tensor, pos: int | list[int], H: int, T: int, scale: float | None = None) -> Tensor:
    """bf16 ``o [B*T, H*D]`` with the kernel's rounding points (fp32 arithmetic on the CPU)."""
    if isinstance(pos, int):
        return _emulate_one(q, k, v, pos, H, T, scale)
    qr = q.view(len(pos), T, -1)
    return torch.cat([_emulate_one(qr[b], k[b:b + 1], v[b:b + 1], p, H, T, scale) for b, p in enumerate(pos)])


# ------------------------------------------------------------------ error measures
def global_rel(got: Tensor, ref: Tensor) -> float:
    """``max|got - ref| / max|ref|``; NaN in ``got`` -> inf."""
    e = (f64(got).reshape(ref.shape) - ref).abs().nan_to_num(nan=math.inf)
    return float(e.max() / ref.abs().max())


def row_measures(got: Tensor, ref: Tensor, A: Tensor, D: int) -> tuple[float, float]:
    """Worst per-(token, head) row ``max|err| / max|ref|`` and worst element ``(err - 2^-7 |ref|) / A``."""
    g = f64(got).reshape(ref.shape)
    err = (g - ref).abs().nan_to_num(nan=math.inf)
    e, r = err.reshape(-1, D), ref.abs().reshape(-1, D)
    row = float((e.amax(-1) / r.amax(-1).clamp_min(1e-300)).max())
    need = float(((err - DR.BF16_ULP * ref.abs()) / A.clamp_min(1e-300)).max())
    return row, need
