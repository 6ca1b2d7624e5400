"""Plain float64 references and shared input builders for the KV-cache decode kernels.

``csrc/decode_attn.hip`` (``kv_append``, ``decode_attn`` and its split partials) and ``csrc/decode_gemv.hip``
(``decode_gemv``, ``decode_qkv``, ``decode_attn_proj``) compute in fp32 from bf16 inputs.  Every reference here
takes those bf16-rounded inputs upcast to float64 (``f64``) and returns the result in float64 together with the
per-element sum of absolute terms ``A`` that the GPU tests' error bound is scaled by.  The formulas are the
textbook ones; the only roundings are the rounding points the kernels document (bf16 residual sum, bf16
normalised row ``(s * rstd) * g``, bf16 GEMM output before SwiGLU / RoPE, bf16 combined attention row before
the output projection).  ``tests/test_decode_refs.py`` checks each against an independent float64 path (CPU);
``tests/test_decode_kernels_gpu.py`` checks the kernels against them.

The builders make the GPU tests' inputs (CPU tensors, fixed seed, rounded to bf16), so the CPU tests can guard
their invariants: cache poison never lies in a visible range, a "dominant" key really dominates, a selector hits
every row and column once.
"""

from __future__ import annotations

import functools
import math

import torch
from torch import Tensor

BF16 = torch.bfloat16
CH = 256             # keys per chunk of the split decode attention
BF16_ULP = 2.0 ** -7
NEG_INF = float("-inf")


def f64(t: Tensor) -> Tensor:
    return t.detach().to("cpu", torch.float64)


def rt(t: Tensor) -> Tensor:
    """float64 -> bf16 (through fp32, as the kernels round) -> float64."""
    return t.to(torch.float32).to(BF16).to(torch.float64)


def _gen(*key: int) -> torch.Generator:
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def randn(*shape: int, seed: tuple[int, ...] = (0,), scale: float = 1.0) -> Tensor:
    return (scale * torch.randn(*shape, generator=_gen(*seed, *shape))).to(BF16)


def bound(ref: Tensor, A: Tensor, tol32: float, extra: Tensor | float = 0.0) -> Tensor:
    """Per-element bound of a bf16 output computed in fp32 and rounded once: one bf16 ulp of the result plus the
    fp32 threshold times the element's sum of absolute terms (plus a derived ``extra``)."""
    return BF16_ULP * ref.abs() + tol32 * A + extra


# ------------------------------------------------------------------ RoPE / kv_append
def rope(x: Tensor, cos: Tensor, sin: Tensor, pos: Tensor) -> tuple[Tensor, Tensor]:
    """Interleaved pairs (x[2i], x[2i+1]) rotated by the table angle at ``pos`` (broadcast against
    ``x.shape[:-1]``).  -> (y, A) with A = |x1 c| + |x2 s| (resp. |x1 s| + |x2 c|)."""
    c, s = cos[pos], sin[pos]
    x1, x2 = x[..., 0::2], x[..., 1::2]
    y = torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).flatten(-2)
    a = torch.stack(((x1 * c).abs() + (x2 * s).abs(), (x1 * s).abs() + (x2 * c).abs()), dim=-1).flatten(-2)
    return y, a


def kv_append(qkv: Tensor, cos: Tensor | None, sin: Tensor | None, p0: int, B: int, T: int, H: int, Hkv: int,
              D: int, Lmax: int) -> dict[str, Tensor | int]:
    """Fused rows ``qkv [B*T, (H + 2 Hkv) D]`` of T new tokens per sequence at positions p0 .. p0+T-1.
    -> q [B, T, H, D] (+ its A), and the n = min(T, Lmax - p0) cache rows that are written: k [B, Hkv, n, D]
    (+ A), v [B, Hkv, n, D] (a copy).  Tokens at positions >= Lmax are dropped."""
    x = qkv.view(B, T, H + 2 * Hkv, D)
    q, k, v = x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]
    if cos is not None:
        pos = (p0 + torch.arange(T)).view(1, T, 1)
        q, aq = rope(q, cos, sin, pos)
        k, ak = rope(k, cos, sin, pos)
    else:
        aq, ak = q.abs(), k.abs()
    n = max(0, min(T, Lmax - p0))
    return {"q": q, "aq": aq, "n": n, "k": k[:, :n].transpose(1, 2), "ak": ak[:, :n].transpose(1, 2),
            "v": v[:, :n].transpose(1, 2)}


# ------------------------------------------------------------------ decode attention
def _scores(q: Tensor, kc: Tensor, H: int, T: int, scale: float | None) -> tuple[Tensor, float]:
    B, Hkv, _, D = kc.shape
    return q.view(B, T, Hkv, H // Hkv, D), (1.0 / math.sqrt(D) if scale is None else scale)


def decode_attention(q: Tensor, kc: Tensor, vc: Tensor, p0: int, H: int, T: int = 1,
                     scale: float | None = None) -> tuple[Tensor, Tensor]:
    """``q [B*T, H*D]`` (row b*T + t, head h = hk*G + g), caches ``[B, Hkv, Lmax, D]``; token t sees keys
    0 .. p0+t.  -> (o [B*T, H*D], A_o = sum_t p_t |V_t,d| / l)."""
    B, Hkv, Lmax, D = kc.shape
    qv, scale = _scores(q, kc, H, T, scale)
    o, a = torch.zeros_like(qv), torch.zeros_like(qv)
    for t in range(T):
        L = p0 + t + 1
        assert L <= Lmax
        s = torch.einsum("bhgd,bhld->bhgl", qv[:, t], kc[:, :, :L]) * scale
        e = torch.exp(s - s.amax(-1, keepdim=True))
        p = e / e.sum(-1, keepdim=True)
        o[:, t] = torch.einsum("bhgl,bhld->bhgd", p, vc[:, :, :L])
        a[:, t] = torch.einsum("bhgl,bhld->bhgd", p, vc[:, :, :L].abs())
    return o.reshape(B * T, H * D), a.reshape(B * T, H * D)


def decode_partials(q: Tensor, kc: Tensor, vc: Tensor, p0: int, H: int, T: int = 1,
                    scale: float | None = None) -> dict[str, Tensor]:
    """Per 256-key chunk c and row: o = sum_t exp(s_t - m) V_t, m = max s_t, l = sum exp(s_t - m) over the keys
    of the chunk that the row sees (natural-log units).  -> ``part [B*T, H, ns, D+2]`` = (o, m, l), ``A`` (the
    absolute-term sums of o), ``empty [B*T, H, ns]`` (the row sees no key of the chunk: m = -inf, l = 0, and o is
    0 here but unspecified in the kernel's output)."""
    B, Hkv, Lmax, D = kc.shape
    qv, scale = _scores(q, kc, H, T, scale)
    ns = (Lmax + CH - 1) // CH
    G = H // Hkv
    part = torch.zeros(B, T, Hkv, G, ns, D + 2, dtype=torch.float64)
    part[..., D] = NEG_INF
    A = torch.zeros(B, T, Hkv, G, ns, D, dtype=torch.float64)
    empty = torch.ones(B, T, Hkv, G, ns, dtype=torch.bool)
    for t in range(T):
        L = p0 + t + 1
        assert L <= Lmax
        for c in range(ns):
            s0, s1 = c * CH, min(L, (c + 1) * CH)
            if s0 >= s1:
                continue
            s = torch.einsum("bhgd,bhld->bhgl", qv[:, t], kc[:, :, s0:s1]) * scale
            m = s.amax(-1)
            e = torch.exp(s - m.unsqueeze(-1))
            part[:, t, :, :, c, :D] = torch.einsum("bhgl,bhld->bhgd", e, vc[:, :, s0:s1])
            part[:, t, :, :, c, D] = m
            part[:, t, :, :, c, D + 1] = e.sum(-1)
            A[:, t, :, :, c] = torch.einsum("bhgl,bhld->bhgd", e, vc[:, :, s0:s1].abs())
            empty[:, t, :, :, c] = False
    return {"part": part.view(B * T, H, ns, D + 2), "A": A.view(B * T, H, ns, D), "empty": empty.view(B * T, H, ns)}


def combine(part: Tensor, A: Tensor | None = None) -> tuple[Tensor, Tensor | None]:
    """Merge ``part [R, H, ns, D+2]`` over the chunks; chunks with m = -inf are ignored whatever their o holds.
    -> (o [R, H*D], A_o or None)."""
    R, H, ns, D2 = part.shape
    D = D2 - 2
    m, l = part[..., D], part[..., D + 1]
    live = m != NEG_INF
    w = torch.where(live, torch.exp(m - m.amax(-1, keepdim=True)), torch.zeros_like(m))
    den = (w * torch.where(live, l, torch.zeros_like(l))).sum(-1, keepdim=True)
    pick = lambda t: torch.where(live.unsqueeze(-1), t, torch.zeros_like(t))
    o = (w.unsqueeze(-1) * pick(part[..., :D])).sum(2) / den
    a = None if A is None else ((w.unsqueeze(-1) * pick(A)).sum(2) / den).reshape(R, H * D)
    return o.reshape(R, H * D), a


def hand_partials(ref: dict[str, Tensor]) -> Tensor:
    """fp32 partials as the kernel lays them out, from the reference, with NaN in the o part of every empty
    chunk (what uninitialised scratch may hold)."""
    p = ref["part"].to(torch.float32)
    D = p.shape[-1] - 2
    o = p[..., :D]
    o[ref["empty"]] = float("nan")
    return p


# ------------------------------------------------------------------ skinny GEMM
def silu(x: Tensor) -> Tensor:
    return x / (1.0 + torch.exp(-x))


def gemv(x: Tensor, w: Tensor, xd: Tensor | None = None, ln: Tensor | None = None, eps: float = 1e-5) -> dict:
    """``s = bf16(x + xd)``, ``h = bf16((s * rstd) * g)`` (each part optional), ``y = h W^T`` in float64 (the
    kernel rounds y to bf16 before any epilogue: see :func:`round_interval`).  -> s, h, y, A = sum_k |h_k w_nk|
    and flip = 2^-8 max_k |h_k w_nk| where a norm is applied (one element of h one rounding step off), else 0."""
    s = rt(x + xd) if xd is not None else x
    h = s
    if ln is not None:
        h = rt(s * torch.rsqrt((s * s).mean(-1, keepdim=True) + eps) * ln)
    y = h @ w.t()
    A = h.abs() @ w.abs().t()
    if ln is not None:
        # max_k |h_mk w_nk|, one weight row at a time (an [M, N, K] product is too large for the LM-head shapes)
        flip = 2.0 ** -8 * torch.stack([(h.abs() * wn.abs()).amax(-1) for wn in w], dim=-1)
    else:
        flip = torch.zeros_like(y)
    return {"s": s, "h": h, "y": y, "A": A, "flip": flip}


def round_interval(y: Tensor, e: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """The bf16 values a GEMM output within ``e`` of ``y`` can round to: (rt(y), rt(y - e), rt(y + e)).  Rounding
    is monotonic, so every admissible value lies between the last two."""
    return rt(y), rt(y - e), rt(y + e)


def _corner_slack(f, ref: Tensor, a: tuple[Tensor, Tensor], b: tuple[Tensor, Tensor]) -> Tensor:
    slack = torch.zeros_like(ref)
    for u in a:
        for v in b:
            slack = torch.maximum(slack, (f(u, v) - ref).abs())
    return slack


def swiglu_epilogue(y: Tensor, e: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """``silu(bf16(g)) * bf16(u)`` over ``y = [g | u]``.  -> (ref, A, slack): A = |ref| (one product), slack = the
    largest change of the result over the corners of the rounding interval of g and u (zero unless ``e``
    reaches a rounding boundary; silu is monotonic over one bf16 step except at its flat minimum)."""
    F = y.shape[-1] // 2
    g, glo, ghi = round_interval(y[..., :F], e[..., :F])
    u, ulo, uhi = round_interval(y[..., F:], e[..., F:])
    f = lambda a, b: silu(a) * b
    ref = f(g, u)
    return ref, ref.abs(), _corner_slack(f, ref, (glo, ghi), (ulo, uhi))


def qkv_epilogue(y: Tensor, e: Tensor, cos: Tensor | None, sin: Tensor | None, p0: int, H: int, Hkv: int,
                 D: int) -> tuple[Tensor, Tensor, Tensor]:
    """bf16-rounded fused-QKV rows ``y [M, (H + 2 Hkv) D]``, q and k heads rotated at position p0 (every row is
    one sequence's single new token), v copied.  -> (ref, A, slack) as [M, H + 2 Hkv, D]."""
    M = y.shape[0]
    r, lo, hi = (t.view(M, H + 2 * Hkv, D) for t in round_interval(y, e))
    if cos is None:
        return r, torch.zeros_like(r), torch.maximum((lo - r).abs(), (hi - r).abs())
    nr = H + Hkv
    c = cos[p0].repeat_interleave(2)
    s = sin[p0].repeat_interleave(2)
    sgn = torch.tensor([-1.0, 1.0], dtype=torch.float64).repeat(D // 2)  # even: me c - pa s, odd: me c + pa s
    partner = lambda t: t.view(M, -1, D // 2, 2).flip(-1).reshape(t.shape)
    f = lambda me, pa: me * c + sgn * pa * s
    ref = r.clone()
    ref[:, :nr] = f(r[:, :nr], partner(r[:, :nr]))
    A = torch.zeros_like(r)
    A[:, :nr] = (r[:, :nr] * c).abs() + (partner(r[:, :nr]) * s).abs()
    slack = torch.maximum((lo - r).abs(), (hi - r).abs())
    slack[:, :nr] = _corner_slack(f, ref[:, :nr], (lo[:, :nr], hi[:, :nr]), (partner(lo[:, :nr]), partner(hi[:, :nr])))
    return ref, A, slack


def attn_proj(part: Tensor, A_part: Tensor | None, w: Tensor, tol32: float) -> tuple[Tensor, Tensor, Tensor]:
    """``y = bf16(combine(part)) W^T``.  -> (y, A = sum_k |x_k w_nk|, slack).  The combined row x is rounded to
    bf16 before the projection; its fp32 error (``tol32`` times its absolute-term sum, |x| itself when
    ``A_part`` is not known) can move an element across a rounding boundary, so slack = sum_k |w_nk| (xhi_k -
    xlo_k) over the interval each element can round to (zero for almost every element)."""
    x64, a = combine(part, A_part)
    e = tol32 * (a if a is not None else x64.abs())
    x, lo, hi = round_interval(x64, e)
    return x @ w.t(), x.abs() @ w.abs().t(), (hi - lo) @ w.abs().t()


# ------------------------------------------------------------------ builders: caches and queries
def poison_like(t: Tensor) -> Tensor:
    """bf16 NaN, +inf, NaN, -inf, ... over the flattened elements."""
    n = t.numel()
    p = torch.full((n,), float("nan"))
    p[1::4] = float("inf")
    p[3::4] = NEG_INF
    return p.view(t.shape).to(BF16)


def caches(B: int, Hkv: int, Lmax: int, D: int, valid: int, seed: int = 0) -> tuple[Tensor, Tensor]:
    """K, V ``[B, Hkv, Lmax, D]``: finite random rows below ``valid``, poison from there on."""
    k = randn(B, Hkv, Lmax, D, seed=(seed, 1))
    v = randn(B, Hkv, Lmax, D, seed=(seed, 2))
    k[:, :, valid:] = poison_like(k[:, :, valid:])
    v[:, :, valid:] = poison_like(v[:, :, valid:])
    return k, v


def queries(B: int, T: int, H: int, D: int, seed: int = 0) -> Tensor:
    return randn(B * T, H * D, seed=(seed, 3))


def dominant_case(B: int, H: int, Hkv: int, D: int, Lmax: int, L: int, factor: float = 4.0, seed: int = 0):
    """"Last key dominant": ``K[L-1] = factor * q`` (head g = 0 of each kv head; G = 1 in the tests), every other
    key scaled by 0.1, ``V[L-1]`` a ramp that differs per (b, kv head); poison from row L on.
    -> (q, K, V, V[L-1] as [B, H*D] rows)."""
    G = H // Hkv
    q = queries(B, 1, H, D, seed=seed + 7)
    k, v = caches(B, Hkv, Lmax, D, L, seed=seed + 7)
    k[:, :, :L] = (0.1 * k[:, :, :L].float()).to(BF16)
    k[:, :, L - 1] = (factor * q.view(B, Hkv, G, D)[:, :, 0].float()).to(BF16)
    ramp = (torch.arange(D).float() - D / 2) / 8
    off = (torch.arange(B * Hkv).float().view(B, Hkv, 1) + 1) / 4
    v[:, :, L - 1] = (ramp + off).to(BF16)
    last = v[:, :, L - 1].unsqueeze(2).expand(B, Hkv, G, D).reshape(B, H * D)
    return q, k, v, last


SPREAD_SCALE = 2.0 ** -3


def spread_case(B: int, H: int, Hkv: int, D: int, Lmax: int, L: int, dominant: int, seed: int = 0):
    """Chunk maxima more than 100 apart with every score exactly representable in fp32: q and K hold small
    dyadic numbers (q in +-{1/2, 1}, K = noise in {-1.5 .. 1.5 step 0.5} + a_c sign(q), a_c = 0 in the
    ``dominant`` chunk and -32 elsewhere), and the scale is ``SPREAD_SCALE``, a power of two.  So the scores,
    their maxima and the differences are exact in any summation order, and only exp, the sums of p and p V and
    the combine are under test.  G = 1 (the sign pattern is per query head).  -> (q, K, V)."""
    assert H == Hkv
    g = _gen(seed, B, H, D, Lmax, L, dominant)
    q = (torch.randint(1, 3, (B, H * D), generator=g).float() / 2) * (2 * torch.randint(0, 2, (B, H * D), generator=g) - 1)
    noise = torch.randint(-3, 4, (B, Hkv, Lmax, D), generator=g).float() / 2
    a = torch.full((Lmax,), -32.0)
    a[dominant * CH:(dominant + 1) * CH] = 0.0
    k = noise + a.view(1, 1, Lmax, 1) * torch.sign(q).view(B, Hkv, 1, D)
    _, v = caches(B, Hkv, Lmax, D, L, seed=seed + 11)
    k = k.to(BF16)
    k[:, :, L:] = poison_like(k[:, :, L:])
    return q.to(BF16), k, v


@functools.lru_cache(maxsize=None)
def proj_case(B: int, ns: int, seed: int = 0):
    """Inputs of the ``decode_attn_proj`` tests: H = 4, Hkv = 2, D = 64 (K = 256), ``Lmax = 256 ns``, the
    position inside chunk 1 when there is one (chunks 2.. are empty), inside chunk 0 otherwise.
    -> (q, K, V, p0, H, reference partials)."""
    H, Hkv, D, Lmax = 4, 2, 64, CH * ns
    p0 = 300 if ns > 1 else 100
    q = queries(B, 1, H, D, seed=seed + 13)
    k, v = caches(B, Hkv, Lmax, D, p0 + 1, seed=seed + 13)
    return q, k, v, p0, H, decode_partials(f64(q), f64(k), f64(v), p0, H)


# ------------------------------------------------------------------ builders: skinny GEMM
def gemv_inputs(M: int, K: int, N: int, seed: int = 0) -> dict[str, Tensor]:
    return {"x": randn(M, K, seed=(seed, 4)), "xd": randn(M, K, seed=(seed, 5), scale=0.5),
            "ln": (1 + 0.1 * torch.randn(K, generator=_gen(seed, 6, K))).to(BF16),
            "w": randn(N, K, seed=(seed, 7), scale=K ** -0.5)}


def strided_rows(t: Tensor, pad: int, seed: int = 0) -> Tensor:
    """``t`` as the row-slice ``buf[:, :cols]`` of a wider random buffer."""
    buf = randn(t.shape[0], t.shape[1] + pad, seed=(seed, 8))
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


# VALU kernel: lane l of a weight row reads vectors l + 16 u; u < 8 are prefetched, the rest streams 4 at a time
VALU_PF_VECS, VALU_GROUP_VECS = 16 * 8, 16 * 4
MFMA_PF_STEPS = 8


def valu_partial_group(K: int) -> bool:
    nv = K // 8
    return nv > VALU_PF_VECS and (nv - VALU_PF_VECS) % VALU_GROUP_VECS != 0


def mfma_wave_steps(K: int) -> list[int]:
    """k-steps (of 32) of each of the 4 waves."""
    nks = K // 32
    per = (nks + 3) // 4
    return [max(0, min(nks, (w + 1) * per) - min(nks, w * per)) for w in range(4)]


def mfma_partial_tail(K: int) -> bool:
    return any(s > MFMA_PF_STEPS and (s - MFMA_PF_STEPS) % 4 != 0 for s in mfma_wave_steps(K))


def selector_columns(K: int, kernel: str, n: int) -> list[int]:
    """``n`` distinct columns: first the named ones -- inside the first vector, the last prefetched vector, the
    first streamed vector, a tail vector that only lane 0 of a row reads (VALU) / the last step of wave 0's
    partial tail group (MFMA), and K - 1 -- then seeded random others."""
    if kernel == "valu":
        nv = K // 8
        assert nv > VALU_PF_VECS and (nv - 1) % 16 == 0
        named = [3, 8 * (VALU_PF_VECS - 1) + 5, 8 * VALU_PF_VECS + 1, 8 * (nv - 1) + 2, K - 1]
    else:
        s0 = mfma_wave_steps(K)[0]
        assert s0 > MFMA_PF_STEPS and (s0 - MFMA_PF_STEPS) % 4 != 0
        named = [3, 32 * (MFMA_PF_STEPS - 1) + 31, 32 * MFMA_PF_STEPS, 32 * (s0 - 1) + 17, K - 1]
    assert len(set(named)) == len(named)
    rest = [c for c in torch.randperm(K, generator=_gen(K, 9)).tolist() if c not in named]
    return (named + rest)[:n]


def one_hot_rows(cols: list[int], K: int) -> Tensor:
    """[len(cols), K] bf16, row i is 1 at ``cols[i]``."""
    t = torch.zeros(len(cols), K)
    t[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    return t.to(BF16)
