"""The KV-cache decode kernels (``csrc/decode_attn.hip``, ``csrc/decode_gemv.hip``) against the float64 references
of ``tests/decode_refs.py``, at the lengths, group sizes, K tails and strides where each kernel takes another path.

Inputs are built on the CPU with a fixed seed, rounded to bf16 and copied to the GPU; the reference sees the same
rounded values in float64.  Cache rows past the valid length hold NaN / +-inf, so a kernel that reads one key too
many returns NaN, and NaN counts as failure everywhere.  The bound is the one of the row-wise suite
(``tests/test_rowwise_kernels_gpu.py``), per element:

* bf16 outputs: ``|got - ref| <= 2^-7 |ref| + TOL32 * A``.  The kernels compute in fp32 and round once; 2^-7 |ref|
  is one bf16 ulp, ``A`` is the reference's sum of absolute terms of that element (``sum_t p_t |V_td| / l`` for
  attention, ``sum_k |h_k w_nk|`` for the skinny GEMM, ``|x1 c| + |x2 s|`` for RoPE).
* fp32 partials: ``TOL32 * A`` for ``o``, ``TOL32 * l`` for ``l``, ``TOL32 * max(1, |m|)`` for ``m``; empty chunks
  have ``m == -inf`` and ``l == 0`` exactly and their ``o`` is not looked at.
* ``TOL32 = 1e-5`` is the project's fp32 forward threshold (``tests/test_kernels_gpu.py``), far below the classical
  ``n * 2^-24`` of the longest sums here (6.9e-5 for 1024 keys + 128 dims, 3.4e-4 for K = 5632).  It was not
  loosened: the worst required threshold ``(err - 2^-7 |ref| - extra) / A`` measured per op is printed at the end
  of the module (``-s``); see MEASURED below.
* derived extra terms, each zero unless an intermediate bf16 rounding can really go either way:
  - the normalised row ``h = bf16((s * rstd) * g)`` can differ from the reference by one bf16 step where the fp32
    ``rsqrtf`` crosses a rounding boundary: ``+ 2^-8 * max_k |h_k w_nk|`` wherever a norm weight is given (the
    term models one such element; the kernels stay inside it at every shape here);
  - SwiGLU / RoPE read the GEMM output rounded to bf16: where the reference's float64 output is within the
    bound of a rounding boundary, both neighbours are admissible, and the extra term is the largest change of
    the epilogue's result over them (``decode_refs.swiglu_epilogue`` / ``qkv_epilogue``);
  - ``decode_attn_proj`` reads the combined attention row rounded to bf16: the same, summed over the row's
    elements that can round either way (``decode_refs.attn_proj``).
* exact claims (V rows, untouched cache rows, the residual sum, selectors, empty-chunk statistics, determinism)
  with ``torch.equal``.

MEASURED on an MI355X with this file (``-s`` prints them again), worst required threshold per op; TOL32 = 1e-5 is
the project's value, kept with these margins, nothing here was fitted:

    partials m  8.3e-7 (12x below)    partials l  1.8e-6 (5.5x)    partials o  1.4e-6 (7x)
    decode_attention  7.6e-8          kv_append  1.4e-8
    decode_gemv, decode_gemv swiglu, decode_qkv, decode_attn_proj: negative (the bf16 ulp and the derived extra
    terms alone cover every element)

The CPU suite (``tests/test_decode_refs.py``) shows that plain fp32 arithmetic in another summation order stays
inside the same bound, so the bound is not tighter than fp32 itself.
"""

from __future__ import annotations

import functools
import math

import pytest
import torch

from bpe_transformer.ops import decode as OD
from bpe_transformer.ops import reference as R

from . import decode_refs as DR
from .decode_refs import BF16, f64

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
WORST: dict[str, float] = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for op in sorted(WORST):
        print(f"\nworst required fp32 threshold, {op}: {WORST[op]:.3e} (TOL32 = {TOL32:g})", end="")
    print()


def _note(op: str, ratio: float):
    WORST[op] = max(WORST.get(op, -math.inf), ratio)


def check(got: torch.Tensor, ref: torch.Tensor, A: torch.Tensor, op: str, extra=0.0, what: str = ""):
    """bf16 output against the module docstring's bound."""
    assert got.dtype == BF16, (what, got.dtype)
    g = f64(got).reshape(ref.shape)
    err = (g - ref).abs()
    bad = ~(err <= DR.bound(ref, A, TOL32, extra))  # NaN counts as bad
    need = ((err - DR.BF16_ULP * ref.abs() - extra) / A.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    _note(op, float(need.max()))
    assert not bad.any(), (what or op, int(bad.sum()), bad.numel(), float(need.max()))


def check32(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, op: str, what: str = ""):
    """fp32 output: ``|got - ref| <= TOL32 * scale`` per element."""
    assert got.dtype == torch.float32, (what, got.dtype)
    err = (f64(got) - ref).abs()
    need = (err / scale.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    if need.numel():
        _note(op, float(need.max()))
    assert bool((need <= TOL32).all()), (what or op, float(need.max()))


def _pos(dev, p0: int) -> torch.Tensor:
    return torch.tensor([p0], dtype=torch.int32, device=dev)


# ------------------------------------------------------------------ decode attention
def _check_partials(got: torch.Tensor, ref: dict, D: int, what: str):
    part, A, empty = ref["part"], ref["A"], ref["empty"]
    assert got.shape == part.shape and got.dtype == torch.float32, (what, got.shape, part.shape)
    g = got.cpu()
    live = ~empty
    assert torch.equal(g[..., D][empty], torch.full((int(empty.sum()),), -math.inf)), what
    assert torch.equal(g[..., D + 1][empty], torch.zeros(int(empty.sum()))), what
    mref, lref = part[..., D][live], part[..., D + 1][live]
    check32(g[..., D][live], mref, mref.abs().clamp_min(1.0), "partials m", what)
    check32(g[..., D + 1][live], lref, lref, "partials l", what)
    check32(g[..., :D][live], part[..., :D][live], A[live], "partials o", what)


def _run_attention(dev, q, k, v, p0, H, T=1, scale=None):
    """-> (combined output, partials) of the kernel, on the CPU."""
    D = k.shape[-1]
    sc = 1.0 / math.sqrt(D) if scale is None else scale
    qg, kg, vg, pos = q.to(dev), k.to(dev), v.to(dev), _pos(dev, p0)
    out = OD.decode_attention(qg, kg, vg, pos, H, scale, n_new=T)
    if T == 1:
        part = OD.decode_attention_partials(qg, kg, vg, pos, H, scale)
    else:  # the wrapper has no n_new: the op itself
        part = torch.ops.bpe_hip.decode_attn(qg, kg, vg, pos, H, sc, False, T)
    return out.cpu(), part.cpu()


def _attention_case(dev, q, k, v, p0, H, T=1, scale=None, what=""):
    B, Hkv, Lmax, D = k.shape
    assert p0 + T <= Lmax and not torch.isfinite(k[:, :, p0 + T:]).any()
    ref, A = DR.decode_attention(f64(q), f64(k), f64(v), p0, H, T, scale)
    pref = DR.decode_partials(f64(q), f64(k), f64(v), p0, H, T, scale)
    out, part = _run_attention(dev, q, k, v, p0, H, T, scale)
    assert out.shape == (B * T, H * D) and part.shape == (B * T, H, (Lmax + 255) // 256, D + 2)
    assert torch.isfinite(out).all(), what
    check(out, ref, A, "decode_attention", what=what)
    _check_partials(part, pref, D, what)
    return out, ref, A


def _random_case(dev, B, H, Hkv, D, Lmax, T, p0, what=""):
    q = DR.queries(B, T, H, D, seed=p0 + Lmax)
    k, v = DR.caches(B, Hkv, Lmax, D, p0 + T, seed=p0 + Lmax)
    return _attention_case(dev, q, k, v, p0, H, T, what=what)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [1, 2, 255, 256, 257, 511, 512, 513, 1024])
def test_attention_lengths(gpu_device, L, D):
    """One key, the chunk boundaries +- 1, the full cache; rows from L on are NaN / inf."""
    _random_case(gpu_device, 2, 4, 2, D, 1024, 1, L - 1)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Lmax", [8, 200, 264, 600])
@pytest.mark.parametrize("full", [True, False])
def test_attention_cache_size_not_a_chunk_multiple(gpu_device, full, Lmax, D):
    """``pos = Lmax - 1`` (the last chunk is partial by the cache's size, not by the position) and a shorter one."""
    _random_case(gpu_device, 3, 2, 1, D, Lmax, 1, Lmax - 1 if full else Lmax // 2)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6, 7, 8])
def test_attention_query_groups(gpu_device, G, D):
    """Every group size (G = 3: MR = 4 > R; 5, 6, 7: MR = 8 > R, ``r / G`` and ``r % G`` without a power of two),
    two live chunks and an empty one."""
    _random_case(gpu_device, 2, 2 * G, 2, D, 600, 1, 300)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("p0", [0, 254, 255, 256, 700])
@pytest.mark.parametrize("G,T", [(3, 2), (1, 3), (1, 7), (2, 3)])
def test_attention_multi_token(gpu_device, G, T, p0, D):
    """T new tokens on both sides of a chunk boundary (p0 = 254, 255: a chunk that only the later tokens see;
    its earlier rows must come out as m = -inf, l = 0), layout ``[B*T, H, ns, D+2]``."""
    _random_case(gpu_device, 2, 2 * G, 2, D, 1024, T, p0)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [1, 256, 257, 513, 1024])
def test_attention_last_key_dominant(gpu_device, L, D):
    """The last visible key carries the whole softmax mass: the output is ``V[L-1]``.  A dropped last key gives
    some average of the other rows instead."""
    B, H, Lmax = 2, 2, 1024
    q, k, v, last = DR.dominant_case(B, H, H, D, Lmax, L)
    out, ref, A = _attention_case(gpu_device, q, k, v, L - 1, H)
    # the reference differs from V[L-1] by less than TOL32 max|V[L-1]| (tests/test_decode_refs.py)
    check(out, f64(last), A, "decode_attention", extra=TOL32 * float(f64(last).abs().max()), what="V[L-1]")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dominant", [0, 1, 2])
def test_attention_chunk_maximum_spread(gpu_device, dominant, D):
    """Chunk maxima more than 100 apart (exp(m - M) underflows in fp32), the dominant chunk first, in the middle,
    last; the scores themselves are exact in fp32 by construction."""
    B, H, Lmax, L = 2, 2, 768, 700
    q, k, v = DR.spread_case(B, H, H, D, Lmax, L, dominant)
    _attention_case(gpu_device, q, k, v, L - 1, H, scale=DR.SPREAD_SCALE)


def test_attention_is_deterministic(gpu_device):
    dev = gpu_device
    q = DR.queries(2, 3, 4, 64).to(dev)
    k, v = (t.to(dev) for t in DR.caches(2, 2, 1024, 64, 703))
    pos = _pos(dev, 700)
    a, b = (OD.decode_attention(q, k, v, pos, 4, n_new=3) for _ in range(2))
    pa, pb = (torch.ops.bpe_hip.decode_attn(q, k, v, pos, 4, 0.125, False, 3) for _ in range(2))
    live = ~DR.decode_partials(f64(q), f64(k), f64(v), 700, 4, 3)["empty"]
    assert torch.equal(a, b) and torch.equal(pa.cpu()[live], pb.cpu()[live])


# ------------------------------------------------------------------ decode_attn_proj
@functools.lru_cache(maxsize=None)
def _proj_weight(N: int) -> torch.Tensor:
    return DR.randn(N, 256, seed=(N,), scale=1.0 / 16)


@pytest.mark.parametrize("N", [16, 40, 1000])
@pytest.mark.parametrize("ns", [1, 3, 5])
@pytest.mark.parametrize("B", [1, 2, 5, 9, 16])
@pytest.mark.parametrize("source", ["kernel", "hand"])
def test_attn_proj(gpu_device, source, B, ns, N):
    """``combine(part) W^T`` from the kernel's own partials and from the reference's with NaN in the ``o`` part of
    every empty chunk (B = 1: VALU kernel, B >= 2: MFMA, B > 8: only MFMA)."""
    dev = gpu_device
    q, k, v, p0, H, pref = DR.proj_case(B, ns)
    w = _proj_weight(N)
    if source == "kernel":
        part = torch.ops.bpe_hip.decode_attn(q.to(dev), k.to(dev), v.to(dev), _pos(dev, p0), H, 0.125, False, 1)
    else:
        part = DR.hand_partials(pref).to(dev)
        assert ns == 1 or torch.isnan(part).any()
    y = OD.decode_attn_proj(part, w.to(dev))
    assert y.shape == (B, N) and torch.isfinite(y).all()
    pc = f64(part)
    ref, A, slack = DR.attn_proj(pc, pref["A"], f64(w), TOL32)
    check(y, ref, A, "decode_attn_proj", extra=slack)


# ------------------------------------------------------------------ kv_append
def _kv_append_case(dev, B, T, H, Hkv, D, Lmax, p0, rope=True, pad=0, table_rows=None):
    W = (H + 2 * Hkv) * D
    qkv = DR.strided_rows(DR.randn(B * T, W, seed=(p0, T)), pad) if pad else DR.randn(B * T, W, seed=(p0, T))
    assert (qkv.stride(0) != W) == bool(pad)
    cos, sin = R.rope_tables(D, table_rows or Lmax, 10000.0)
    k0, v0 = DR.caches(B, Hkv, Lmax, D, Lmax, seed=91)  # finite sentinel rows everywhere
    buf = qkv._base.to(dev) if pad else qkv.to(dev)
    qg = buf[:, :W] if pad else buf
    kg, vg = k0.to(dev), v0.to(dev)
    q = OD.kv_append(qg, kg, vg, cos.to(dev) if rope else None, sin.to(dev) if rope else None, _pos(dev, p0), B, T, H)
    ref = DR.kv_append(f64(qkv), cos.double() if rope else None, sin.double() if rope else None, p0, B, T, H, Hkv, D,
                       Lmax)
    n = ref["n"]
    q, kc, vc = q.cpu(), kg.cpu(), vg.cpu()
    assert q.shape == (B * T, H * D)
    # rows of dropped tokens (position >= Lmax) are unspecified: compare the written tokens only
    check(q.view(B, T, H, D)[:, :n], ref["q"][:, :n], ref["aq"][:, :n], "kv_append", what="q")
    check(kc[:, :, p0:p0 + n], ref["k"], ref["ak"], "kv_append", what="k")
    assert torch.equal(f64(vc[:, :, p0:p0 + n]), ref["v"])
    if not rope:
        assert torch.equal(f64(q.view(B, T, H, D)[:, :n]), ref["q"][:, :n]) and torch.equal(f64(kc[:, :, p0:p0 + n]), ref["k"])
    # every other row of every (b, head) slab is untouched
    for got, old in ((kc, k0), (vc, v0)):
        assert torch.equal(got[:, :, :p0], old[:, :, :p0]) and torch.equal(got[:, :, p0 + n:], old[:, :, p0 + n:])
    return q, kc, vc, ref


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("pad", [0, 24])
def test_kv_append_slab_isolation(gpu_device, pad, rope, D):
    """Sentinel caches: only rows [p0, p0 + T) of each slab change, V bit-exactly; ``pad``: ``qkv`` is a row-slice
    of a wider buffer; ``rope = None`` copies q and k too."""
    _kv_append_case(gpu_device, 3, 4, 4, 2, D, 16, 5, rope=rope, pad=pad)


@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_nearly_full_cache(gpu_device, D):
    """``p0 = Lmax - 2``, five new tokens: two are written, three dropped, nothing lands in the next slab."""
    Lmax = 16
    *_, ref = _kv_append_case(gpu_device, 3, 5, 4, 2, D, Lmax, Lmax - 2, table_rows=Lmax + 8)
    assert ref["n"] == 2


def test_kv_append_grid_stride_loop(gpu_device):
    """2,098,176 vectors: 1024 more than the capped grid (8192 x 256) covers in one sweep; the last token rows
    are the second loop iteration."""
    B, T, H, Hkv, D = 1, 2049, 32, 16, 128
    assert B * T * (H + 2 * Hkv) * (D // 8) > 8192 * 256
    q, kc, vc, ref = _kv_append_case(gpu_device, B, T, H, Hkv, D, T + 7, 3)
    tail = slice(T - 2, T)
    check(q.view(B, T, H, D)[:, tail], ref["q"][:, tail], ref["aq"][:, tail], "kv_append", what="last rows")
    assert torch.equal(f64(vc[:, :, 3 + T - 1]), ref["v"][:, :, T - 1])


# ------------------------------------------------------------------ decode_gemv / decode_qkv
EPILOGUES = ["plain", "swiglu", "qkv64r", "qkv64", "qkv128r", "qkv128"]


@functools.lru_cache(maxsize=None)
def _gemv_inputs(M, K, N):
    return DR.gemv_inputs(M, K, N)


def _opt(i, name, on, dev, pad):
    if not on:
        return None, None
    t = i[name]
    if pad and name != "ln":
        t = DR.strided_rows(t, pad, seed=len(name))
        g = t._base.to(dev)[:, :t.shape[1]]
        assert g.stride(0) == t.shape[1] + pad
        return t, g
    return t, t.to(dev)


def _gemv_case(dev, M, K, epi, N=None, xd=True, ln=True, pad=False):
    """One skinny-GEMM call through ``decode_gemv`` / ``decode_qkv`` against the reference; ``pad``: x and xd are
    row-slices of [M, K + 16] buffers and w of [N, K + 8]."""
    qkv = epi.startswith("qkv")
    if qkv:
        D, rope, H, Hkv = int(epi[3:].rstrip("r")), epi.endswith("r"), 2, 1
        N = (H + 2 * Hkv) * D
    elif N is None:
        N = 40
    i = _gemv_inputs(M, K, N)
    x, xg = _opt(i, "x", True, dev, 16 if pad else 0)
    d, dg = _opt(i, "xd", xd, dev, 16 if pad else 0)
    g, gg = _opt(i, "ln", ln, dev, 0)
    w, wg = _opt(i, "w", True, dev, 8 if pad else 0)
    r = DR.gemv(f64(x), f64(w), None if d is None else f64(d), None if g is None else f64(g), 1e-5)
    e = TOL32 * r["A"] + r["flip"]
    what = f"M={M} K={K} {epi} N={N} xd={xd} ln={ln} pad={pad}"
    if not qkv:
        y, s = OD.decode_gemv(xg, wg, dg, gg, 1e-5, swiglu=epi == "swiglu")
        if epi == "swiglu":
            ref, A, slack = DR.swiglu_epilogue(r["y"], e)
            check(y, ref, A, "decode_gemv swiglu", extra=slack, what=what)
        else:
            check(y, r["y"], r["A"], "decode_gemv", extra=r["flip"], what=what)
    else:
        Lmax, p0 = 8, 5
        cos, sin = R.rope_tables(D, Lmax, 10000.0)
        k0, v0 = DR.caches(M, Hkv, Lmax, D, Lmax, seed=92)
        kg, vg = k0.to(dev), v0.to(dev)
        q, s = OD.decode_qkv(xg, wg, kg, vg, cos.to(dev) if rope else None, sin.to(dev) if rope else None,
                             _pos(dev, p0), H, dg, gg, 1e-5)
        ref, A, slack = DR.qkv_epilogue(r["y"], e, cos.double() if rope else None, sin.double() if rope else None,
                                        p0, H, Hkv, D)
        kc, vc = kg.cpu(), vg.cpu()
        got = torch.cat((q.cpu().view(M, H, D), kc[:, :, p0], vc[:, :, p0]), dim=1)
        check(got, ref, A, "decode_qkv", extra=slack, what=what)
        keep = torch.arange(Lmax) != p0
        assert torch.equal(kc[:, :, keep], k0[:, :, keep]) and torch.equal(vc[:, :, keep], v0[:, :, keep]), what
    if xd:
        assert s.shape == (M, K) and torch.equal(f64(s), r["s"]), what  # one rounding of x + xd
    else:
        assert s is None


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("K", [8, 24, 264, 1032, 1288])
def test_gemv_valu_kernel(gpu_device, K, M, epi):
    """K % 32 != 0: ``gemv_kernel<MM, EPI>`` for MM = 1, 2, 4, 8 (M = 3, 5: zero rows in the tile).  K = 8, 24: most
    lanes of a row have no vector; 264: prefetch only; 1032, 1288: a partial streaming group of 1 resp. 33 vectors."""
    assert K % 32 != 0
    _gemv_case(gpu_device, M, K, epi)


@pytest.mark.parametrize("epi", ["plain", "swiglu", "qkv64r", "qkv128"])
@pytest.mark.parametrize("M", [2, 9, 15, 16])
@pytest.mark.parametrize("K", [32, 96, 160, 1056, 1184, 1568])
def test_gemv_mfma_kernel(gpu_device, K, M, epi):
    """K % 32 == 0, M >= 2: ``gemv_mfma_kernel<EPI>``.  K = 32, 96, 160: idle waves; 1056, 1184, 1568: a partial
    4-step tail group of 1, 2 and 5 steps; M = 9 .. 16 exist on this kernel only."""
    _gemv_case(gpu_device, M, K, epi)


@pytest.mark.parametrize("M,K", [(1, 5632), (8, 5632), (5, 5640)])
@pytest.mark.parametrize("epi", ["plain", "swiglu"])
def test_gemv_large_k(gpu_device, epi, M, K):
    """K = 5632 at M = 1 (VALU) and M = 8 (MFMA, 94,592 bytes of dynamic LDS); M = 5, K = 5640: the VALU kernel's
    8-row tile, 90,240 bytes.  Both are above the 64 KiB that need ``hipFuncSetAttribute``."""
    _gemv_case(gpu_device, M, K, epi, N=48)


@pytest.mark.parametrize("M,K", [(3, 264), (3, 160)])
@pytest.mark.parametrize("epi,N", [("plain", n) for n in (1, 15, 16, 17)] + [("swiglu", 2 * f) for f in (1, 7, 8, 9)])
def test_gemv_n_edges(gpu_device, epi, N, M, K):
    """One output, one row short of a 16-row workgroup, exactly one, one more (SwiGLU: 8 column pairs per workgroup)."""
    _gemv_case(gpu_device, M, K, epi, N=N)


@pytest.mark.parametrize("M,K", [(1, 264), (3, 1288), (3, 1184), (16, 160)])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("xd,ln", [(False, False), (True, False), (False, True), (True, True)])
def test_gemv_prologue_parts_and_strides(gpu_device, xd, ln, pad, M, K):
    """``xd`` and ``ln`` independently; ``pad``: x, xd and w with a row stride that is not the row length.  The
    residual sum is exact and contiguous either way."""
    _gemv_case(gpu_device, M, K, "plain", xd=xd, ln=ln, pad=pad)
    _gemv_case(gpu_device, M, K, "qkv64r", xd=xd, ln=ln, pad=pad)


@pytest.mark.parametrize("kernel,K,M", [("valu", 1288, 5), ("valu", 1288, 1), ("mfma", 1184, 5), ("mfma", 1184, 16)])
def test_gemv_selectors_are_exact(gpu_device, kernel, K, M):
    """One-hot x rows pick weight columns, one-hot weight rows pick x columns, bit-exactly: a vector that is
    dropped, read twice or paired with the wrong input vector shows as a wrong or zero element."""
    dev = gpu_device
    assert (K % 32 != 0) == (kernel == "valu")
    cols = DR.selector_columns(K, kernel, 19)
    w = DR.randn(21, K, seed=(1,))
    for c0 in range(0, 19 if M == 1 else 1):  # M = 1: one call per hot column
        mine = cols[c0:c0 + M]
        y, _ = OD.decode_gemv(DR.one_hot_rows(mine, K).to(dev), w.to(dev))
        assert torch.equal(y.cpu(), w[:, mine].t().contiguous()), (kernel, K, M, mine)
    x = DR.randn(M, K, seed=(2,))
    y, _ = OD.decode_gemv(x.to(dev), DR.one_hot_rows(cols, K).to(dev))
    assert torch.equal(y.cpu(), x[:, cols]), (kernel, K, M)


@pytest.mark.parametrize("M,K", [(9, 264), (3, 12), (17, 256)])
def test_gemv_shape_refusals(gpu_device, M, K):
    """Host-side checks, no launch: more than 8 rows off the MFMA kernel's K, K no multiple of 8, more than 16 rows."""
    dev = gpu_device
    x, w = torch.zeros(M, K, dtype=BF16, device=dev), torch.zeros(16, K, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError):
        OD.decode_gemv(x, w)
