"""The fp8 KV cache kernels (``csrc/kv_fp8.hip``) and the fp8 ``DecodeSession`` on the MI355X.

* ``kv_append_fp8``: bytes and scales ``torch.equal`` to the oracle (``ops.decode.kv_append_fp8_reference``, whose
  quantiser ``tests/test_kv_fp8_refs.py`` pins to an independent float64 path), q ``torch.equal`` to ``kv_append``'s,
  every other cache row ``torch.equal`` to its old content.  K rows take the kernel's roped bf16 row, which may
  differ from the CPU oracle's by one bf16 rounding step of the fp32 rotation (``kv_append`` is bounded, not bit
  exact, against its reference); so K is compared with the oracle quantiser applied to the row the bf16 ``kv_append``
  kernel writes, which is the format's definition ("exactly what the bf16 cache would have held"), and V (no
  arithmetic before the quantiser) with the CPU oracle end to end.
* ``decode_attn_fp8``: the combined output and the partials against ``decode_refs.decode_attention`` /
  ``decode_partials`` in float64 on the dequantised caches, with the bound of ``tests/test_decode_kernels_gpu.py``
  unchanged: ``2^-7 |ref| + TOL32 * A``, ``TOL32 = 1e-5``, and its rules for the partials.  Poison past the valid
  length is byte 0x7F (e4m3 NaN) with scale NaN; NaN anywhere in an output fails.
* ``kv_dequant``: ``torch.equal`` to the oracle on the valid rows, the poisoned scratch untouched past them.
* sessions: bf16 model, fp8 cache, against the CPU fp32 oracle session on the same bf16-rounded weights with
  ``kv_dtype="fp8"``: ``rel < 3e-2``, the threshold ``test_session_matches_full_forward`` uses for the bf16 cache.

MEASURED on an MI355X with this file (``-s`` prints them again), worst required fp32 threshold per op against
``TOL32 = 1e-5``, which is the project's value and was not fitted:

    partials m  6.4e-7 (16x below)    partials l  1.5e-6 (6.5x)    partials o  1.2e-6 (8x)
    decode_attention_fp8  2.4e-8

* The device conversion (``v_cvt_pk_fp8_f32``) agreed with torch's e4m3 round-to-nearest-even on every planted row,
  the e4m3 subnormals and the exact ties included: no finding there.
* Reported, not asserted: ``decode_attn_fp8`` was bitwise the bf16 ``decode_attn`` on the dequantised bf16 cache in
  all 45 attention cases of this file.
* Reported, not asserted: the fp8 cache moves the logits of the 2-layer random-init test models by ``rel`` 2.2e-2
  (D 64), 2.8e-2 (G 2) and 1.7e-2 (D 128) from the bf16 cache's (max |diff| / max |logit| over prefill 30 + 10 decode
  steps).  Random-init weights say nothing about real-text quality.
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.ops import decode as OD
from bpe_transformer.ops import reference as R

from . import decode_refs as DR
from . import kv_fp8_refs as KR
from .decode_refs import BF16, f64

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
WORST: dict[str, float] = {}
BITWISE: dict[bool, int] = {True: 0, False: 0}
GAP: list[float] = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for op in sorted(WORST):
        print(f"\nworst required fp32 threshold, {op}: {WORST[op]:.3e} (TOL32 = {TOL32:g})", end="")
    print(f"\ndecode_attn_fp8 bitwise equal to decode_attn on the dequantised bf16 cache: {BITWISE[True]} cases, "
          f"different: {BITWISE[False]}", end="")
    for g in GAP:
        print(f"\nfp8-cache vs bf16-cache logits, rel: {g:.3e}", end="")
    print()


def _note(op: str, ratio: float):
    WORST[op] = max(WORST.get(op, -math.inf), ratio)


def check(got, ref, A, op, what=""):
    assert got.dtype == BF16, (what, got.dtype)
    g = f64(got).reshape(ref.shape)
    err = (g - ref).abs()
    bad = ~(err <= DR.bound(ref, A, TOL32))  # NaN counts as bad
    need = ((err - DR.BF16_ULP * ref.abs()) / A.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    _note(op, float(need.max()))
    assert not bad.any(), (what or op, int(bad.sum()), bad.numel(), float(need.max()))


def check32(got, ref, scale, op, what=""):
    assert got.dtype == torch.float32, (what, got.dtype)
    err = (f64(got) - ref).abs()
    need = (err / scale.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    if need.numel():
        _note(op, float(need.max()))
    assert bool((need <= TOL32).all()), (what or op, float(need.max()))


def _check_partials(got, ref, D, what):
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


# ------------------------------------------------------------------ kv_append_fp8
def _append_case(dev, B, T, H, Hkv, D, Lmax, pos, rope=True, pad=0, plant=False):
    W = (H + 2 * Hkv) * D
    qkv = DR.randn(B * T, W, seed=(sum(pos), T, D))
    if plant:  # the scale-boundary, zero and tiny rows into V of kv head 0, one per token row
        sp = KR.planted(D)
        for i in range(B * T):
            qkv.view(B * T, H + 2 * Hkv, D)[i, H + Hkv] = sp[i % sp.shape[0]]
    if pad:
        qkv = DR.strided_rows(qkv, pad)
        assert qkv.stride(0) == W + pad
    cos, sin = R.rope_tables(D, Lmax + 8, 10000.0) if rope else (None, None)
    old = KR.fp8_caches(B, Hkv, Lmax, D, 0, seed=5)  # poison everywhere
    g = lambda t: None if t is None else t.to(dev)  # noqa: E731
    qg = qkv._base.to(dev)[:, :W] if pad else qkv.to(dev)
    k8, v8, ks, vs = (old[n].to(dev) for n in ("k8", "v8", "ks", "vs"))
    p = torch.tensor(pos, dtype=torch.int32)
    q = OD.kv_append_fp8(qg, k8, v8, ks, vs, g(cos), g(sin), p.to(dev), B, T, H)
    # the bf16 kernel on zeroed bf16 caches: its q, and the rows the bf16 cache would have held
    kb, vb = (torch.zeros(B, Hkv, Lmax, D, dtype=BF16, device=dev) for _ in range(2))
    q_bf = OD.kv_append(qg, kb, vb, g(cos), g(sin), p.to(dev), B, T, H)
    # the CPU oracle end to end
    o = {n: old[n].clone() for n in ("k8", "v8", "ks", "vs")}
    OD.kv_append_fp8_reference(qkv.contiguous(), o["k8"], o["v8"], o["ks"], o["vs"], cos, sin, p, B, T, H)
    k8, v8, ks, vs, kb = k8.cpu(), v8.cpu(), ks.cpu(), vs.cpu(), kb.cpu()
    plist = pos if len(pos) > 1 else pos * B
    for b, p0 in enumerate(plist):
        n = max(0, min(T, Lmax - p0))
        w = slice(p0, p0 + n)
        rows = slice(b * T, b * T + n)  # query rows of dropped tokens are unspecified
        assert torch.equal(q[rows].cpu(), q_bf[rows].cpu()), "q is kv_append's, bit for bit"
        assert torch.equal(KR.codes(v8)[b, :, w], KR.codes(o["v8"])[b, :, w]) and torch.equal(vs[b, :, w], o["vs"][b, :, w])
        kq, kscale = OD.kv_quantize_reference(kb[b, :, w])
        assert torch.equal(KR.codes(k8)[b, :, w], KR.codes(kq)) and torch.equal(ks[b, :, w], kscale)
        if not rope:  # no arithmetic before the quantiser: the CPU oracle end to end for K too
            assert torch.equal(KR.codes(k8)[b, :, w], KR.codes(o["k8"])[b, :, w]) and torch.equal(ks[b, :, w], o["ks"][b, :, w])
        rest = torch.ones(Lmax, dtype=torch.bool)
        rest[w] = False
        for t8, ts, name in ((k8, ks, "k"), (v8, vs, "v")):
            assert torch.equal(KR.codes(t8)[b][:, rest], KR.codes(old[name + "8"])[b][:, rest]), "untouched bytes"
            assert bool(torch.isnan(ts[b][:, rest]).all()), "untouched scales"
    assert torch.isfinite(ks[torch.isfinite(o["ks"])]).all() and torch.equal(torch.isnan(ks), torch.isnan(o["ks"]))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("pad", [0, 24])
def test_kv_append_fp8(gpu_device, pad, rope, D):
    _append_case(gpu_device, 2, 3, 4, 2, D, 16, [5], rope=rope, pad=pad)


@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_fp8_nearly_full_cache(gpu_device, D):
    """``p0 = Lmax - 2``: the third token is dropped, nothing lands in the next slab."""
    _append_case(gpu_device, 2, 3, 4, 2, D, 16, [14])


@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_fp8_ragged(gpu_device, D):
    _append_case(gpu_device, 3, 3, 4, 2, D, 16, [0, 15, 7])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rope", [True, False])
def test_kv_append_fp8_special_rows(gpu_device, rope, D):
    """Scale boundaries, zero, clamped and huge rows, e4m3 subnormals and ties, planted into V."""
    _append_case(gpu_device, 4, 4, 2, 1, D, 32, [3], rope=rope, plant=True)


def test_kv_append_fp8_non_finite_row(gpu_device):
    dev = gpu_device
    B, T, H, Hkv, D, Lmax = 1, 2, 2, 1, 64, 8
    qkv = DR.randn(B * T, (H + 2 * Hkv) * D, seed=(9,))
    qkv.view(T, H + 2 * Hkv, D)[1, H + Hkv, 5] = float("inf")
    c = KR.fp8_caches(B, Hkv, Lmax, D, 0)
    k8, v8, ks, vs = (c[n].to(dev) for n in ("k8", "v8", "ks", "vs"))
    OD.kv_append_fp8(qkv.to(dev), k8, v8, ks, vs, None, None, torch.zeros(1, dtype=torch.int32, device=dev), B, T, H)
    vs = vs.cpu()
    assert torch.isfinite(vs[0, 0, 0]) and torch.isnan(vs[0, 0, 1]) and torch.isfinite(ks.cpu()[0, 0, :2]).all()


def test_kv_append_fp8_grid_stride_loop(gpu_device):
    """2,098,176 vectors: 1024 more than the capped grid (8192 x 256) covers in one sweep."""
    B, T, H, Hkv, D = 1, 2049, 32, 16, 128
    assert B * T * (H + 2 * Hkv) * (D // 8) > 8192 * 256
    _append_case(gpu_device, B, T, H, Hkv, D, T + 7, [3], rope=False)


# ------------------------------------------------------------------ decode_attn_fp8
def _attention_case(dev, B, H, Hkv, D, Lmax, T, pos, spread=False, what=""):
    """``pos``: one shared p0 or one per sequence."""
    plist = [pos] * B if isinstance(pos, int) else list(pos)
    c = KR.fp8_caches(B, Hkv, Lmax, D, [p + T for p in plist], seed=Lmax + T + sum(plist), spread=spread)
    q = DR.queries(B, T, H, D, seed=Lmax + sum(plist))
    sc = 1.0 / math.sqrt(D)
    pg = torch.tensor([pos] if isinstance(pos, int) else plist, dtype=torch.int32, device=dev)
    qg, k8, v8, ks, vs = (t.to(dev) for t in (q, c["k8"], c["v8"], c["ks"], c["vs"]))
    out = OD.decode_attention_fp8(qg, k8, v8, ks, vs, pg, H, n_new=T)
    part = OD.decode_attention_partials_fp8(qg, k8, v8, ks, vs, pg, H, n_new=T)
    ns = (Lmax + 255) // 256
    assert out.shape == (B * T, H * D) and part.shape == (B * T, H, ns, D + 2)
    out, part = out.cpu(), part.cpu()
    assert torch.isfinite(out).all(), what
    # float64 reference on the dequantised caches, one sequence at a time (its own position)
    kd = KR.dequantize64(KR.codes(c["k8"]), c["ks"])
    vd = KR.dequantize64(KR.codes(c["v8"]), c["vs"])
    for b, p0 in enumerate(plist):
        assert not torch.isfinite(kd[b, :, p0 + T:]).any()
        rows = slice(b * T, (b + 1) * T)
        ref, A = DR.decode_attention(f64(q[rows]), kd[b:b + 1], vd[b:b + 1], p0, H, T)
        check(out[rows], ref, A, "decode_attention_fp8", what=what)
        _check_partials(part[rows], DR.decode_partials(f64(q[rows]), kd[b:b + 1], vd[b:b + 1], p0, H, T), D, what)
    # reported, not asserted: the bf16 kernel on the dequantised bf16 cache (finite filler in place of the poison)
    kb, vb = c["k"].nan_to_num(0.0).to(dev), c["v"].nan_to_num(0.0).to(dev)
    BITWISE[bool(torch.equal(OD.decode_attention(qg, kb, vb, pg, H, n_new=T).cpu(), out))] += 1
    return qg, k8, v8, ks, vs, pg, out


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [1, 255, 256, 257, 513])
def test_attention_fp8_lengths(gpu_device, L, D):
    _attention_case(gpu_device, 2, 4, 2, D, 1024, 1, L - 1)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("full", [True, False])
def test_attention_fp8_cache_size_not_a_chunk_multiple(gpu_device, full, D):
    _attention_case(gpu_device, 3, 2, 1, D, 300, 1, 299 if full else 150)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_attention_fp8_query_groups(gpu_device, G, D):
    """Two live chunks and an empty one, every MR instantiation."""
    _attention_case(gpu_device, 2, 2 * G, 2, D, 600, 1, 300)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("p0", [0, 254])
@pytest.mark.parametrize("G,T", [(1, 8), (2, 4), (4, 2), (1, 3)])
def test_attention_fp8_multi_token(gpu_device, G, T, p0, D):
    """T new tokens on both sides of a chunk boundary (p0 = 254: a chunk that only the later tokens see)."""
    _attention_case(gpu_device, 2, 2 * G, 2, D, 1024, T, p0)


@pytest.mark.parametrize("D", [64, 128])
def test_attention_fp8_ragged_positions(gpu_device, D):
    """One sequence with a single key (its other chunks empty), one full cache, one in between."""
    _attention_case(gpu_device, 3, 4, 2, D, 600, 1, [0, 599, 300])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 3])
def test_attention_fp8_scales_2_to_20_apart(gpu_device, T, D):
    """Neighbouring keys' (and values') scales differ by 2^20: a dropped or misindexed scale changes the softmax
    weights or the output by orders of magnitude."""
    qg, k8, v8, ks, vs, pg, out = _attention_case(gpu_device, 2, 4, 2, D, 600, T, 300, spread=True)
    # (2^20 between the rows' magnitudes; each row's own maximum moves its scale by a binade or two)
    assert float((ks[0, 0, 0] / ks[0, 0, 1]).cpu()) >= 2.0 ** 17 and float((vs[0, 0, 1] / vs[0, 0, 0]).cpu()) >= 2.0 ** 17


def test_attention_fp8_is_deterministic(gpu_device):
    qg, k8, v8, ks, vs, pg, out = _attention_case(gpu_device, 2, 4, 2, 64, 1024, 3, 700)
    again = OD.decode_attention_fp8(qg, k8, v8, ks, vs, pg, 4, n_new=3)
    assert torch.equal(again.cpu(), out)


# ------------------------------------------------------------------ kv_dequant
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pos,T", [([37], 5), ([0, 299, 120], 9), ([296], 9)])
def test_kv_dequant(gpu_device, pos, T, D):
    """Shared and ragged positions; ``[296] + 9`` runs past ``Lmax``: the valid length is clamped."""
    dev = gpu_device
    B, Hkv, Lmax = 3, 2, 300
    plist = pos * B if len(pos) == 1 else pos
    valid = [min(p + T, Lmax) for p in plist]
    c = KR.fp8_caches(B, Hkv, Lmax, D, valid, seed=T, spread=True)
    ko, vo = (DR.poison_like(torch.empty(B, Hkv, Lmax, D)).to(dev) for _ in range(2))
    k0, v0 = ko.cpu().view(torch.int16).clone(), vo.cpu().view(torch.int16).clone()
    OD.kv_dequant(*(c[n].to(dev) for n in ("k8", "v8", "ks", "vs")), torch.tensor(pos, dtype=torch.int32, device=dev),
                  T, ko, vo)
    ko, vo = ko.cpu(), vo.cpu()
    for b, n in enumerate(valid):
        assert torch.equal(ko[b, :, :n], OD.kv_dequantize_reference(c["k8"][b, :, :n], c["ks"][b, :, :n]))
        assert torch.equal(vo[b, :, :n], OD.kv_dequantize_reference(c["v8"][b, :, :n], c["vs"][b, :, :n]))
        assert torch.isfinite(ko[b, :, :n]).all() and torch.isfinite(vo[b, :, :n]).all()
        assert torch.equal(ko.view(torch.int16)[b, :, n:], k0[b, :, n:]), "rows past the valid length are untouched"
        assert torch.equal(vo.view(torch.int16)[b, :, n:], v0[b, :, n:])


# ------------------------------------------------------------------ sessions
def rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-12))


MODELS = [{}, {"num_kv_heads": 2}, {"d_model": 512, "num_heads": 4, "d_ff": 1024}]  # D 64, G 2, D 128


def _models(dev, **kw):
    """The 2-layer model of ``tests/test_generation_gpu.py`` in bf16 on the GPU, and the same bf16-rounded weights
    in fp32 on the CPU (the oracle session's)."""
    torch.manual_seed(0)
    cfg = dict(vocab_size=1000, context_length=256, d_model=256, num_layers=2, num_heads=4, d_ff=512)
    cfg.update(kw)
    gm = TransformerLM(**cfg).to(dev, torch.bfloat16).eval()
    cm = TransformerLM(**cfg).eval()
    cm.load_state_dict({k: v.float().cpu() for k, v in gm.state_dict().items()})
    return gm, cm


def _codes(sess):
    c = sess.cache
    return [KR.codes(c.k).cpu(), KR.codes(c.v).cpu(), c.k_scale.cpu(), c.v_scale.cpu()]


@pytest.mark.parametrize("kw", MODELS)
def test_session_matches_the_cpu_oracle_session(gpu_device, kw):
    """Prefill 30 (fp8: ``kv_dequant`` + ``cache_attn`` on the empty cache), 10 decode steps, batch 3, graph on and
    off; the replayed graph leaves the cache bytes of the eager session."""
    gm, cm = _models(gpu_device, **kw)
    ids = torch.randint(0, 1000, (3, 40), generator=torch.Generator().manual_seed(1))
    oracle = DecodeSession(cm, 3, max_len=64, kv_dtype="fp8")
    assert not oracle.fast
    want = [oracle.prefill(ids[:, :30])] + [oracle.decode(ids[:, t]) for t in range(30, 40)]
    got = {}
    for use_graph in (True, False):
        sess = DecodeSession(gm, 3, max_len=64, use_graph=use_graph, kv_dtype="fp8")
        assert sess.fast and sess.cache.k.dtype == torch.float8_e4m3fn
        out = [sess.prefill(ids[:, :30])] + [sess.decode(ids[:, t]) for t in range(30, 40)]
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(out, want)):
            assert torch.isfinite(a).all() and rel(a, b) < 3e-2, (use_graph, i, rel(a, b))
        got[use_graph] = (out, _codes(sess))
    for a, b in zip(got[True][0], got[False][0]):
        assert rel(a, b) < 1e-3
    for a, b in zip(got[True][1], got[False][1]):
        assert torch.equal(a[:, :, :, :40], b[:, :, :, :40])
    # reported only: how far the fp8 cache moves the logits of this random-init model from the bf16 cache's
    bf = DecodeSession(gm, 3, max_len=64, use_graph=False)
    ref = [bf.prefill(ids[:, :30])] + [bf.decode(ids[:, t]) for t in range(30, 40)]
    GAP.append(max(rel(a, b) for a, b in zip(got[False][0], ref)))


@pytest.mark.parametrize("kw", MODELS[:2])
def test_ragged_session_matches_the_cpu_oracle_session(gpu_device, kw):
    gm, cm = _models(gpu_device, **kw)
    g = torch.Generator().manual_seed(2)
    lens = [5, 30, 17]
    pad = torch.randint(0, 1000, (3, 30), generator=g)
    nxt = torch.randint(0, 1000, (6, 3), generator=g)
    outs = []
    for model in (cm, gm):
        s = DecodeSession(model, 3, max_len=48, ragged=True, kv_dtype="fp8")
        o = [s.prefill(pad, lens)] + [s.decode(nxt[t]) for t in range(3)]
        o.append(s.decode(nxt[3], active=[True, False, True])[[0, 2]])
        s.reset_slot(1)
        o.append(s.prefill_slot(1, pad[1, :11]))
        o += [s.decode(nxt[t]) for t in (4, 5)]
        assert s.cache.lengths == [11, 13, 23]
        outs.append(o)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(outs[1], outs[0])):
        assert torch.isfinite(a).all() and rel(a, b) < 3e-2, (i, rel(a, b))


def test_skinny_route_matches_library_route(gpu_device, monkeypatch):
    """The batch <= 8 step (``decode_gemv`` + ``kv_append_fp8`` + ``decode_attn_fp8`` partials merged in Wo's
    prologue) against the library-GEMM step, as ``test_gemv_decode_matches_library_decode``."""
    from bpe_transformer.models import generation

    gm, _ = _models(gpu_device, num_kv_heads=2)
    ids = torch.randint(0, 1000, (6, 24), device=gpu_device)
    outs = []
    for cap in (8, 0):
        monkeypatch.setattr(generation, "_GEMV_MAX_BATCH", cap)
        sess = DecodeSession(gm, 6, max_len=32, use_graph=True, kv_dtype="fp8")
        sess.prefill(ids[:, :16])
        outs.append([sess.decode(ids[:, t]) for t in range(16, 24)])
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and rel(a, b) < 2e-2, rel(a, b)


@pytest.mark.parametrize("kw", MODELS)
def test_second_turn_and_chunked_prefill(gpu_device, kw):
    """16 tokens onto 20 (``kv_append_fp8`` -> ``kv_dequant`` -> ``cache_attn``) against the CPU oracle session, and
    ``prefill_chunk=7`` against unchunked: both to the oracle's threshold, and then one more step to each other's."""
    gm, cm = _models(gpu_device, **kw)
    ids = torch.randint(0, 1000, (2, 36), generator=torch.Generator().manual_seed(3))
    oracle = DecodeSession(cm, 2, max_len=48, kv_dtype="fp8")
    want = [oracle.prefill(ids[:, :20]), oracle.prefill(ids[:, 20:])]
    whole = DecodeSession(gm, 2, max_len=48, kv_dtype="fp8")
    cut = DecodeSession(gm, 2, max_len=48, kv_dtype="fp8", prefill_chunk=7)
    for sess in (whole, cut):
        got = [sess.prefill(ids[:, :20]), sess.prefill(ids[:, 20:])]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and rel(a, b) < 3e-2, rel(a, b)
    assert rel(cut.prefill(ids[:, :1]), whole.prefill(ids[:, :1])) < 3e-2


def test_generate_on_the_gpu(gpu_device):
    gm, _ = _models(gpu_device)
    prompt = torch.randint(0, 1000, (2, 8), device=gpu_device)
    out = gm.generate(prompt, 12, temperature=0.0, kv_dtype="fp8")
    assert out.shape == (2, 20) and torch.equal(out[:, :8], prompt)
    dev = gm.generate(prompt, 12, temperature=0.0, kv_dtype="fp8", sampler="device", seed=3)
    assert torch.equal(dev, out)
    lst = gm.generate([prompt[0], prompt[1, :5]], 6, temperature=0.0, kv_dtype="fp8")
    assert lst[0].numel() == 14 and lst[1].numel() == 11 and torch.equal(lst[1][:5], prompt[1, :5])
