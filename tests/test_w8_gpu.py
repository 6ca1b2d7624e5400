"""fp8 weights for serving, GPU (``csrc/decode_gemv.hip``: the W8 switch of both skinny kernels, ``w_dequant``).

Kernel level: the call with ``(w8, w_scale)`` against the same call on ``weight_dequantize(w8, w_scale)`` -- bit for
bit, outputs and written cache rows.  Weight rows carry scales spread over ``2^-14 .. 2^6`` (magnitudes within
``2^-20 .. 2^10``) and inputs are ~N(0, 1), so nothing leaves the fp32 normal range, where a power-of-two row scale
commutes with every rounding.  Rows: M = 1 is the VALU kernel, M >= 2 the MFMA kernel when ``K % 32 == 0``
(``BPE_GEMV_MFMA_MIN_M`` default); ``K = 1160`` (``K % 32 == 8``) sends M = 3 and 8 to the VALU kernel's 4- and 8-row
tiles as well.  One case per epilogue is also held against the float64 references of ``tests/decode_refs.py`` on the
dequantised weights, with that file's bound and the fp32 threshold of ``tests/test_decode_kernels_gpu.py``.

Session level: the tiny model of ``tests/w8_refs.py`` in bf16, the fp8-weight session against the bf16 session on
the dequantised model, logits ``torch.equal``.
"""

from __future__ import annotations

import functools
import math

import pytest
import torch

from bpe_transformer.models import DecodeSession
from bpe_transformer.ops import decode as OD
from bpe_transformer.ops import reference as R

from . import decode_refs as DR
from . import w8_refs as WR
from .decode_refs import BF16, f64
from .test_decode_kernels_gpu import TOL32, check

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
ROWS = [1, 3, 5, 8, 9, 16]


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equality of two bf16 tensors (NaNs included)."""
    return a.shape == b.shape and a.dtype == b.dtype == BF16 and torch.equal(a.view(torch.int16), b.view(torch.int16))


@functools.lru_cache(maxsize=None)
def _weights(N: int, K: int, pad: bool = False):
    """-> (w8 [N, K], scale [N], dequantised bf16 [N, K]) on the CPU; rows ~N(0, 1/K) times 2^e, e cycling over
    -14 .. 6.  ``pad``: w8 is the row slice of a [N, K + 8] byte buffer whose pad bytes are e4m3 NaN."""
    w = DR.randn(N, K, seed=(N, K, 70), scale=K ** -0.5).float()
    w = w * (2.0 ** (torch.arange(N) % 21 - 14).float())[:, None]
    w8, s = OD.weight_quantize(w.to(BF16))
    wd = OD.weight_dequantize(w8, s)
    assert 2.0 ** -20 < float(wd.abs().max()) < 2.0 ** 10 and float(s.min()) >= 2.0 ** -29
    if pad:
        buf = torch.full((N, K + 8), 0x7F, dtype=torch.uint8)
        buf[:, :K] = w8.view(torch.uint8)
        w8 = buf.view(FP8)[:, :K]
    return w8, s, wd


def _dev_w8(w8: torch.Tensor, dev) -> torch.Tensor:
    if w8.is_contiguous():
        return w8.to(dev)
    g = w8._base.to(dev).view(FP8)[:, : w8.shape[1]]
    assert g.stride(0) == w8.shape[1] + 8
    return g


@functools.lru_cache(maxsize=None)
def _inputs(M: int, K: int):
    i = DR.gemv_inputs(M, K, 8)
    return i["x"], i["xd"], i["ln"]


def _pre(M, K, pre, dev):
    x, xd, ln = _inputs(M, K)
    return (x.to(dev), xd.to(dev) if pre else None, ln.to(dev) if pre else None), (x, xd if pre else None,
                                                                                  ln if pre else None)


# ------------------------------------------------------------------ decode_gemv
@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("K", [64, 160, 1184])
@pytest.mark.parametrize("M", ROWS)
def test_plain(gpu_device, M, K, N):
    """K = 160: 20 vectors, past one 16-lane sweep; K = 1184: past the prefetch, a streamed loop with a ragged tail;
    N = 40: invalid row slots.  With ``xd`` + ``ln`` and without either; padded weight rows."""
    dev = gpu_device
    for pre in (True, False):
        for pad in (False, True):
            w8, s, wd = _weights(N, K, pad)
            (x, xd, ln), _ = _pre(M, K, pre, dev)
            y8, s8 = OD.decode_gemv(x, _dev_w8(w8, dev), xd, ln, w_scale=s.to(dev))
            yb, sb = OD.decode_gemv(x, wd.to(dev), xd, ln)
            assert same(y8, yb) and y8.shape == (M, N) and torch.isfinite(y8).all(), (M, K, N, pre, pad)
            assert (s8 is None and sb is None) if not pre else same(s8, sb)


@pytest.mark.parametrize("epi", ["plain", "swiglu"])
@pytest.mark.parametrize("M", [3, 8])
def test_valu_kernel_multi_row_tiles(gpu_device, M, epi):
    """``K % 32 != 0`` keeps M >= 2 on the VALU kernel (tiles of 4 and 8 rows), streamed loop included."""
    dev, K, N = gpu_device, 1160, 40
    w8, s, wd = _weights(N, K)
    (x, xd, ln), _ = _pre(M, K, True, dev)
    y8, _ = OD.decode_gemv(x, w8.to(dev), xd, ln, swiglu=epi == "swiglu", w_scale=s.to(dev))
    yb, _ = OD.decode_gemv(x, wd.to(dev), xd, ln, swiglu=epi == "swiglu")
    assert same(y8, yb) and torch.isfinite(y8).all()


@pytest.mark.parametrize("F", [8, 20])
@pytest.mark.parametrize("K", [160, 1184])
@pytest.mark.parametrize("M", ROWS)
def test_swiglu(gpu_device, M, K, F):
    dev = gpu_device
    w8, s, wd = _weights(2 * F, K)
    for pre in (True, False):
        (x, xd, ln), _ = _pre(M, K, pre, dev)
        y8, _ = OD.decode_gemv(x, w8.to(dev), xd, ln, swiglu=True, w_scale=s.to(dev))
        yb, _ = OD.decode_gemv(x, wd.to(dev), xd, ln, swiglu=True)
        assert same(y8, yb) and y8.shape == (M, F) and torch.isfinite(y8).all(), (M, K, F, pre)


# ------------------------------------------------------------------ decode_qkv
def _qkv_pair(dev, M, K, D, G, rope, ragged, pre=True):
    """Both calls from the same sentinel caches -> (q8, qb, caches8, cachesb, positions, Lmax)."""
    Hkv, Lmax = 1, 8
    H = G * Hkv
    N = (H + 2 * Hkv) * D
    w8, s, wd = _weights(N, K)
    (x, xd, ln), _ = _pre(M, K, pre, dev)
    cos, sin = R.rope_tables(D, Lmax, 10000.0)
    c, sn = (cos.to(dev), sin.to(dev)) if rope else (None, None)
    P = [(3 * m + 1) % Lmax for m in range(M)]
    if ragged and M > 1:
        P[1] = Lmax  # a full sequence: dropped
    pos = torch.tensor(P if ragged else [5], dtype=torch.int32, device=dev)
    k0, v0 = DR.caches(M, Hkv, Lmax, D, Lmax, seed=93)
    out = []
    for w, ws in ((w8.to(dev), s.to(dev)), (wd.to(dev), None)):
        kg, vg = k0.to(dev), v0.to(dev)
        q, _ = OD.decode_qkv(x, w, kg, vg, c, sn, pos, H, xd, ln, w_scale=ws)
        out.append((q, kg, vg))
    return out, (P if ragged else [5] * M), Lmax, (k0, v0)


@pytest.mark.parametrize("ragged", [False, True], ids=["shared", "per-row"])
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("M", ROWS)
def test_qkv(gpu_device, M, D, G, rope, ragged):
    (a, b), P, Lmax, (k0, v0) = _qkv_pair(gpu_device, M, 160, D, G, rope, ragged)
    live = [m for m in range(M) if P[m] < Lmax]
    assert same(a[0][live], b[0][live])  # (the query row of a dropped sequence is unspecified)
    assert same(a[1], b[1]) and same(a[2], b[2])
    kc = a[1].cpu()
    for m in range(M):
        if P[m] < Lmax:
            assert not torch.equal(kc[m, :, P[m]], k0[m, :, P[m]])
        else:
            assert torch.equal(kc[m], k0[m]) and torch.equal(a[2].cpu()[m], v0[m])


# ------------------------------------------------------------------ decode_attn_proj
@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("B", ROWS)
def test_attn_proj(gpu_device, B, N):
    """H 4, D 64, three splits of which the last is empty (its ``o`` part NaN)."""
    dev = gpu_device
    *_, pref = DR.proj_case(B, 3)
    part = DR.hand_partials(pref).to(dev)
    assert bool(pref["empty"].any()) and torch.isnan(part).any()
    w8, s, wd = _weights(N, 256)
    y8 = OD.decode_attn_proj(part, w8.to(dev), s.to(dev))
    yb = OD.decode_attn_proj(part, wd.to(dev))
    assert same(y8, yb) and y8.shape == (B, N) and torch.isfinite(y8).all()


# ------------------------------------------------------------------ against the float64 references
@pytest.mark.parametrize("M", [1, 5])
def test_against_fp64_references(gpu_device, M):
    dev, K = gpu_device, 160
    (x, xd, ln), (xc, dc, gc) = _pre(M, K, True, dev)
    # plain and SwiGLU
    w8, s, wd = _weights(40, K)
    r = DR.gemv(f64(xc), f64(wd), f64(dc), f64(gc), 1e-5)
    e = TOL32 * r["A"] + r["flip"]
    y, xs = OD.decode_gemv(x, w8.to(dev), xd, ln, w_scale=s.to(dev))
    check(y, r["y"], r["A"], "decode_gemv w8", extra=r["flip"])
    assert torch.equal(f64(xs), r["s"])
    y, _ = OD.decode_gemv(x, w8.to(dev), xd, ln, swiglu=True, w_scale=s.to(dev))
    ref, A, slack = DR.swiglu_epilogue(r["y"], e)
    check(y, ref, A, "decode_gemv swiglu w8", extra=slack)
    # QKV + RoPE + cache write, shared position
    D, H, Hkv, Lmax, p0 = 64, 2, 1, 8, 5
    w8, s, wd = _weights((H + 2 * Hkv) * D, K)
    r = DR.gemv(f64(xc), f64(wd), f64(dc), f64(gc), 1e-5)
    e = TOL32 * r["A"] + r["flip"]
    cos, sin = R.rope_tables(D, Lmax, 10000.0)
    k0, v0 = DR.caches(M, Hkv, Lmax, D, Lmax, seed=92)
    kg, vg = k0.to(dev), v0.to(dev)
    q, _ = OD.decode_qkv(x, w8.to(dev), kg, vg, cos.to(dev), sin.to(dev),
                         torch.tensor([p0], dtype=torch.int32, device=dev), H, xd, ln, w_scale=s.to(dev))
    ref, A, slack = DR.qkv_epilogue(r["y"], e, cos.double(), sin.double(), p0, H, Hkv, D)
    got = torch.cat((q.cpu().view(M, H, D), kg.cpu()[:, :, p0], vg.cpu()[:, :, p0]), dim=1)
    check(got, ref, A, "decode_qkv w8", extra=slack)
    # the output projection from the partials
    *_, pref = DR.proj_case(M, 3)
    part = DR.hand_partials(pref).to(dev)
    w8, s, wd = _weights(40, 256)
    y = OD.decode_attn_proj(part, w8.to(dev), s.to(dev))
    ref, A, slack = DR.attn_proj(f64(part), pref["A"], f64(wd), TOL32)
    check(y, ref, A, "decode_attn_proj w8", extra=slack)


# ------------------------------------------------------------------ NaN scale, refusals, w_dequant
@pytest.mark.parametrize("M", [1, 5])
def test_nan_scale_row(gpu_device, M):
    """A row with a NaN scale (a non-finite weight) makes exactly its own output column NaN."""
    dev, K, N, bad = gpu_device, 160, 40, 21
    w8, s, _ = _weights(N, K)
    (x, xd, ln), _ = _pre(M, K, True, dev)
    sn = s.clone()
    sn[bad] = math.nan
    y, _ = OD.decode_gemv(x, w8.to(dev), xd, ln, w_scale=s.to(dev))
    yn, _ = OD.decode_gemv(x, w8.to(dev), xd, ln, w_scale=sn.to(dev))
    keep = torch.arange(N, device=dev) != bad
    assert torch.isnan(yn[:, bad]).all() and same(yn[:, keep], y[:, keep]) and torch.isfinite(y).all()


def test_refusals(gpu_device):
    dev = gpu_device
    w8, s, wd = _weights(16, 64)
    x = _inputs(1, 64)[0].to(dev)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        OD.decode_gemv(x, wd.to(dev), w_scale=s.to(dev))
    with pytest.raises(RuntimeError, match="bf16 required"):
        OD.decode_gemv(x, w8.to(dev))
    with pytest.raises(RuntimeError, match="w_scale"):
        OD.decode_gemv(x, w8.to(dev), w_scale=s[:8].to(dev))
    odd = torch.zeros(16, 68, dtype=torch.uint8, device=dev).view(FP8)[:, :64]  # row stride 68: not a multiple of 8
    with pytest.raises(RuntimeError, match="multiple of 8"):
        OD.decode_gemv(x, odd, w_scale=s.to(dev))


@pytest.mark.parametrize("N,K", [(40, 160), (301, 128)])
def test_w_dequant(gpu_device, N, K):
    dev = gpu_device
    for pad in (False, True):
        w8, s, wd = _weights(N, K, pad)
        out = torch.full((N + 1, K), 7.0, dtype=BF16, device=dev)
        OD.w_dequant(_dev_w8(w8, dev), s.to(dev), out[:N])
        assert same(out[:N].cpu(), wd) and bool((out[N] == 7.0).all())


# ------------------------------------------------------------------ sessions
@pytest.fixture(scope="module")
def models(gpu_device):
    m = WR.tiny_model(gpu_device, BF16)
    return m, WR.dequantised(m)


def _pair(models, B, **kw):
    model, ref = models
    kw.setdefault("use_graph", False)
    s8, sb = DecodeSession(model, B, weight_dtype="fp8", **kw), DecodeSession(ref, B, **kw)
    assert s8.fast and sb.fast
    return s8, sb


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("B", [1, 3, 8, 9])
def test_session_batches(models, B, kv):
    """Batch 1, 3, 8: the skinny kernels stream the e4m3 rows; 9: the library GEMMs on the scratch.  Prefill (flash,
    or for the fp8 cache ``cache_attn_fp8``), 3 decode steps, a second turn, one more step."""
    s8, sb = _pair(models, B, kv_dtype=kv)
    got, want = WR.run_session(s8, B), WR.run_session(sb, B)
    assert len(got) == 6
    for a, b in zip(got, want):
        assert torch.equal(a, b) and torch.isfinite(a).all()


def test_session_flash_then_cache_attn_then_decode(models):
    """Flash prefill of 17 tokens, a 9-token append (``cache_attn``), 4 decode steps; and every position's logits of
    a 3-token window (``score``: ``decode_attn`` with more than one token)."""
    B = 2
    s8, sb = _pair(models, B)
    got, want = WR.run_session(s8, B, 17, 0, 9), WR.run_session(sb, B, 17, 0, 9)
    for s, out in ((s8, got), (sb, want)):
        lg = out[-1]
        for _ in range(3):
            lg = s.decode(lg.argmax(-1)).float().cpu()
            out.append(lg)
        out.append(s.score(WR.prompt(B, 3, seed=4)).float().cpu())
    assert len(got) == 7 and s8.length == 17 + 9 + 4 + 3
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_session_ragged(models):
    B = 3
    outs = []
    for s in _pair(models, B, ragged=True):
        lg = [s.prefill(WR.prompt(B, 5), [5, 2, 4])]
        lg.append(s.decode(lg[-1].argmax(-1)))
        lg.append(s.decode(lg[-1].argmax(-1), active=[True, False, True])[[0, 2]])
        lg.append(s.prefill_slot(1, WR.prompt(1, 3, seed=2)[0]))
        assert s.cache.lengths == [7, 6, 6]
        outs.append(lg)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_session_graph(models):
    """The captured step (the scratch and the e4m3 matrices are static) replayed 4 times, against eager launches and
    against the bf16 session."""
    B = 2
    (g8, gb), (e8, _) = _pair(models, B, use_graph=True), _pair(models, B)
    outs = [WR.run_session(s, B, 5, 4, 0) for s in (g8, gb, e8)]
    assert g8._graph is not None and e8._graph is None
    for a, b, c in zip(*outs):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_session_holds_fp8_only(models):
    model, _ = models
    s = DecodeSession(model, 2, weight_dtype="fp8", use_graph=False)
    b = DecodeSession(model, 2, use_graph=False)
    shapes = set()
    for lw in s._w:
        for w in (lw[1], lw[2], lw[4], lw[5]):
            assert w[0].dtype == FP8 and w[1].dtype == torch.float32 and w[1].shape == (w[0].shape[0],)
            shapes.add(tuple(w[0].shape))
    assert s._head[0].dtype == FP8
    shapes.add(tuple(s._head[0].shape))
    assert shapes == {(384, 128), (128, 128), (512, 128), (128, 256), (WR.VOCAB, 128)}

    def tensors(o, seen):
        if isinstance(o, torch.Tensor):
            yield o
        elif isinstance(o, (list, tuple)):
            for x in o:
                yield from tensors(x, seen)
        elif isinstance(o, dict):
            yield from tensors(list(o.values()), seen)

    held = [t for k, v in vars(s).items() if k != "model" for t in tensors(v, None)]
    big = [t for t in held if t.dtype == BF16 and (tuple(t.shape) in shapes or t.numel() >= 128 * 128)]
    assert len(big) == 1 and big[0] is s._wscratch and big[0].numel() == 512 * 128
    # (K + 4) / (2 K) of the bf16 session's projection bytes, matrix by matrix
    want = sum(n * (k + 4) for n, k in ((384, 128), (128, 128), (512, 128), (128, 256))) * 2 + WR.VOCAB * 132
    assert s.weight_nbytes() == want and b.weight_nbytes() == 2 * (want - 4 * (2 * 1152 + WR.VOCAB))
