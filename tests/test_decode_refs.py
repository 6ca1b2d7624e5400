"""The float64 references of ``tests/decode_refs.py`` against independent float64 paths and the fp32 oracles of
``ops/decode.py``, the invariants of the shared input builders, and a float32 evaluation in another summation
order against the GPU tests' bound (CPU only)."""

from __future__ import annotations

import math

import pytest
import torch
import torch.nn.functional as TF

from bpe_transformer.ops import decode as OD
from bpe_transformer.ops import reference as R

from . import decode_refs as DR
from .decode_refs import BF16, f64

F64 = torch.float64
TOL32 = 1e-5  # the GPU tests' fp32 threshold (tests/test_decode_kernels_gpu.py)


def close(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=1e-12)


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = f64(a), f64(b)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


ATTN_SHAPES = [(2, 4, 2, 64, 600, 1, 0), (2, 4, 2, 64, 600, 1, 599), (1, 6, 2, 128, 520, 2, 255),
               (3, 2, 2, 64, 264, 3, 254), (1, 7, 1, 64, 1024, 1, 700)]  # B, H, Hkv, D, Lmax, T, p0


def _attn_inputs(B, H, Hkv, D, Lmax, T, p0):
    q = DR.queries(B, T, H, D)
    k, v = DR.caches(B, Hkv, Lmax, D, p0 + T)
    return q, k, v


# ------------------------------------------------------------------ references vs independent float64 paths
@pytest.mark.parametrize("B,H,Hkv,D,Lmax,T,p0", ATTN_SHAPES)
def test_attention_ref_vs_sdpa(B, H, Hkv, D, Lmax, T, p0):
    q, k, v = _attn_inputs(B, H, Hkv, D, Lmax, T, p0)
    o, a = DR.decode_attention(f64(q), f64(k), f64(v), p0, H, T)
    L, G = p0 + T, H // Hkv
    mask = torch.arange(L)[None, :] <= (p0 + torch.arange(T))[:, None]  # [T, L], True = visible
    q4 = f64(q).view(B, T, H, D).transpose(1, 2)                          # [B, H, T, D]
    k4 = f64(k)[:, :, :L].repeat_interleave(G, dim=1)
    v4 = f64(v)[:, :, :L].repeat_interleave(G, dim=1)
    ref = TF.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask)
    assert close(o, ref.transpose(1, 2).reshape(B * T, H * D))
    assert bool((a >= o.abs() - 1e-12).all()) and torch.isfinite(o).all()


@pytest.mark.parametrize("B,H,Hkv,D,Lmax,T,p0", ATTN_SHAPES)
def test_combined_partials_equal_unsplit_attention(B, H, Hkv, D, Lmax, T, p0):
    q, k, v = _attn_inputs(B, H, Hkv, D, Lmax, T, p0)
    o, a = DR.decode_attention(f64(q), f64(k), f64(v), p0, H, T)
    p = DR.decode_partials(f64(q), f64(k), f64(v), p0, H, T)
    ns = (Lmax + 255) // 256
    assert p["part"].shape == (B * T, H, ns, D + 2)
    oc, ac = DR.combine(p["part"], p["A"])
    assert close(oc, o) and close(ac, a)
    # a row sees chunk c iff the chunk starts at or below its own position
    t = torch.arange(B * T) % T
    vis = (torch.arange(ns) * 256)[None, :] <= (p0 + t)[:, None]
    assert torch.equal(p["empty"], ~vis[:, None, :].expand(B * T, H, ns))
    m, l = p["part"][..., D], p["part"][..., D + 1]
    assert bool((m[p["empty"]] == DR.NEG_INF).all()) and bool((l[p["empty"]] == 0).all())
    # NaN in the o part of the empty chunks changes nothing
    hand = DR.hand_partials(p)
    if p["empty"].any():
        assert torch.isnan(hand[..., :D][p["empty"]]).all()
    assert not torch.isnan(hand[..., :D][~p["empty"]]).any()
    oh, _ = DR.combine(f64(hand))
    assert torch.isfinite(oh).all() and rel(oh, o) < 1e-6


@pytest.mark.parametrize("swiglu", [False, True])
@pytest.mark.parametrize("xd,ln", [(False, False), (True, False), (False, True), (True, True)])
def test_gemv_ref_vs_torch_functional(xd, ln, swiglu):
    M, K, N = 5, 264, 34
    i = DR.gemv_inputs(M, K, N)
    x, w = f64(i["x"]), f64(i["w"])
    r = DR.gemv(x, w, f64(i["xd"]) if xd else None, f64(i["ln"]) if ln else None, 1e-5)
    s = (i["x"].float() + i["xd"].float()).to(BF16).double() if xd else x
    h = DR.rt(TF.rms_norm(s, (K,), f64(i["ln"]), 1e-5)) if ln else s
    assert torch.equal(r["s"], s)
    assert float((r["h"] - h).abs().max()) <= 2.0 ** -7 * float(h.abs().max())  # a rounding step at the most
    y = TF.linear(r["h"], w)
    assert close(r["y"], y) and bool((r["A"] >= y.abs() - 1e-12).all())
    e = torch.zeros_like(y)
    if swiglu:
        ref, A, slack = DR.swiglu_epilogue(r["y"], e)
        g, u = DR.rt(y).chunk(2, dim=-1)
        assert close(ref, TF.silu(g) * u) and not slack.any()
    assert bool((r["flip"] > 0).all()) == ln


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("p0,T", [(0, 1), (5, 4), (30, 5)])
def test_kv_append_ref_vs_apply_rope(p0, T, rope):
    B, H, Hkv, D, Lmax = 2, 4, 2, 64, 32
    qkv = DR.randn(B * T, (H + 2 * Hkv) * D)
    cos, sin = R.rope_tables(D, Lmax + 8, 10000.0)
    c, s = (cos.double(), sin.double()) if rope else (None, None)
    r = DR.kv_append(f64(qkv), c, s, p0, B, T, H, Hkv, D, Lmax)
    x = f64(qkv).view(B, T, H + 2 * Hkv, D)
    tp = torch.arange(p0, p0 + T)
    rot = (lambda t: R.apply_rope(t.transpose(1, 2), cos.double(), sin.double(), tp).transpose(1, 2)) if rope \
        else (lambda t: t)
    n = max(0, min(T, Lmax - p0))
    assert r["n"] == n and n == (2 if p0 == 30 else T)
    assert close(r["q"], rot(x[:, :, :H]))
    assert close(r["k"], rot(x[:, :, H:H + Hkv])[:, :n].transpose(1, 2))
    assert torch.equal(r["v"], x[:, :, H + Hkv:][:, :n].transpose(1, 2))
    assert bool((r["aq"] >= r["q"].abs() - 1e-12).all())


def test_qkv_epilogue_is_gemv_then_kv_append():
    M, K, H, Hkv, D, p0 = 3, 264, 2, 1, 64, 9
    i = DR.gemv_inputs(M, K, (H + 2 * Hkv) * D)
    cos, sin = R.rope_tables(D, 16, 10000.0)
    r = DR.gemv(f64(i["x"]), f64(i["w"]), f64(i["xd"]), f64(i["ln"]))
    ref, A, slack = DR.qkv_epilogue(r["y"], torch.zeros_like(r["y"]), cos.double(), sin.double(), p0, H, Hkv, D)
    ka = DR.kv_append(DR.rt(r["y"]), cos.double(), sin.double(), p0, M, 1, H, Hkv, D, 16)
    assert close(ref[:, :H], ka["q"][:, 0]) and close(A[:, :H], ka["aq"][:, 0]) and not slack.any()
    assert close(ref[:, H:H + Hkv], ka["k"][:, :, 0]) and torch.equal(ref[:, H + Hkv:], ka["v"][:, :, 0])
    # an interval that reaches a rounding boundary shows up as slack of about one rounding step
    _, _, s2 = DR.qkv_epilogue(r["y"], 2.0 ** -9 * r["y"].abs(), cos.double(), sin.double(), p0, H, Hkv, D)
    assert s2.any() and float(s2.max()) <= 2.0 ** -6 * float(ref.abs().max())


# ------------------------------------------------------------------ references vs the fp32 oracles
def _pos(p0):
    return torch.tensor([p0], dtype=torch.int32)


@pytest.mark.parametrize("B,H,Hkv,D,Lmax,T,p0", ATTN_SHAPES)
def test_attention_ref_vs_fp32_oracle(B, H, Hkv, D, Lmax, T, p0):
    q, k, v = _attn_inputs(B, H, Hkv, D, Lmax, T, p0)
    o, _ = DR.decode_attention(f64(q), f64(k), f64(v), p0, H, T)
    assert rel(OD.decode_attention_reference(q, k, v, _pos(p0), H, None, T), o) < 2.0 ** -7
    if T == 1:
        p = DR.decode_partials(f64(q), f64(k), f64(v), p0, H)
        orc = OD.decode_partials_reference(q, k, v, _pos(p0), H)
        live = ~p["empty"]
        assert rel(orc[..., :D][live], p["part"][..., :D][live]) < TOL32
        assert rel(orc[..., D][live], p["part"][..., D][live]) < TOL32
        assert rel(orc[..., D + 1], p["part"][..., D + 1]) < TOL32
        assert bool((orc[..., D][~live] == DR.NEG_INF).all())
        w = DR.randn(40, H * D, scale=(H * D) ** -0.5)
        y, _, _ = DR.attn_proj(p["part"], p["A"], f64(w), TOL32)
        assert rel(OD.decode_attn_proj(orc, w), y) < 2.0 ** -7
        # the oracle skips an empty chunk's o part too (it used to scale it by 0: NaN stayed NaN)
        assert rel(OD.decode_attn_proj(DR.hand_partials(p), w), y) < 2.0 ** -7


@pytest.mark.parametrize("swiglu", [False, True])
def test_gemv_ref_vs_fp32_oracle(swiglu):
    i = DR.gemv_inputs(4, 1032, 48)
    r = DR.gemv(f64(i["x"]), f64(i["w"]), f64(i["xd"]), f64(i["ln"]))
    y, s = OD.decode_gemv_reference(i["x"], i["w"], i["xd"], i["ln"], 1e-5, swiglu)
    assert torch.equal(f64(s), r["s"])
    ref = DR.swiglu_epilogue(r["y"], torch.zeros_like(r["y"]))[0] if swiglu else r["y"]
    assert rel(y, ref) < 2e-2  # the oracle's own tolerance in tests/test_generation_gpu.py


def test_kv_append_ref_vs_fp32_oracle():
    B, T, H, Hkv, D, Lmax, p0 = 2, 5, 4, 2, 64, 32, 29
    qkv = DR.randn(B * T, (H + 2 * Hkv) * D)
    cos, sin = R.rope_tables(D, Lmax + 8, 10000.0)
    kc, vc = torch.zeros(B, Hkv, Lmax, D, dtype=BF16), torch.zeros(B, Hkv, Lmax, D, dtype=BF16)
    q = OD.kv_append_reference(qkv, kc, vc, cos, sin, _pos(p0), B, T, H)
    r = DR.kv_append(f64(qkv), cos.double(), sin.double(), p0, B, T, H, Hkv, D, Lmax)
    assert r["n"] == 3
    assert rel(q, r["q"].reshape(B * T, H * D)) < 2.0 ** -7
    assert rel(kc[:, :, p0:], r["k"]) < 2.0 ** -7 and torch.equal(f64(vc[:, :, p0:]), r["v"])
    assert not kc[:, :, :p0].any() and not vc[:, :, :p0].any()


# ------------------------------------------------------------------ builder invariants
@pytest.mark.parametrize("valid", [1, 255, 600])
def test_poison_never_in_visible_range(valid):
    k, v = DR.caches(2, 2, 600, 64, valid)
    for c in (k, v):
        assert torch.isfinite(c[:, :, :valid]).all()
        tail = c[:, :, valid:]
        assert not torch.isfinite(tail).any()
        if tail.numel():
            assert torch.isnan(tail).any() and (tail == math.inf).any() and (tail == -math.inf).any()
    assert torch.isfinite(DR.queries(2, 1, 4, 64)).all()


DOMINANT_LS = (1, 256, 257, 513, 1024)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", DOMINANT_LS)
def test_dominant_key_carries_the_mass(L, D):
    B, H, Lmax = 2, 2, 1024
    q, k, v, last = DR.dominant_case(B, H, H, D, Lmax, L)
    assert torch.isfinite(k[:, :, :L]).all() and not torch.isfinite(k[:, :, L:]).any()
    s = torch.einsum("bhd,bhld->bhl", f64(q).view(B, H, D), f64(k)[:, :, :L]) / math.sqrt(D)
    p = torch.softmax(s, -1)
    assert float(p[..., L - 1].min()) >= 0.99
    o, _ = DR.decode_attention(f64(q), f64(k), f64(v), L - 1, H)
    # the rest of the mass is below the fp32 threshold: the reference output IS the last value row
    assert float((o - f64(last)).abs().max()) <= TOL32 * float(f64(last).abs().max())
    assert len({tuple(r.tolist()) for r in last.view(B * H, D)}) == B * H  # a distinct ramp per (b, head)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dominant", [0, 1, 2])
def test_spread_scores_are_exact_and_maxima_far_apart(dominant, D):
    B, H, Lmax, L = 2, 2, 768, 700
    q, k, v = DR.spread_case(B, H, H, D, Lmax, L, dominant)
    assert torch.isfinite(k[:, :, :L]).all() and torch.isfinite(v[:, :, :L]).all()
    qv, kv = f64(q).view(B, H, D), f64(k)[:, :, :L]
    s = torch.einsum("bhd,bhld->bhl", qv, kv) * DR.SPREAD_SCALE
    # exact in fp32, also summed back to front
    s32 = torch.einsum("bhd,bhld->bhl", qv.float() * DR.SPREAD_SCALE, kv.float())
    s32r = torch.einsum("bhd,bhld->bhl", qv.float().flip(-1) * DR.SPREAD_SCALE, kv.float().flip(-1))
    assert torch.equal(s32.double(), s) and torch.equal(s32r.double(), s)
    mx = torch.stack([s[..., c * 256:min(L, (c + 1) * 256)].amax(-1) for c in range(3)], -1)
    others = [c for c in range(3) if c != dominant]
    assert float((mx[..., dominant:dominant + 1] - mx[..., others]).min()) > 100
    # the dominant chunk's softmax is spread over many keys, not one
    p = torch.softmax(s, -1)
    assert float(p.max()) < 0.5


@pytest.mark.parametrize("kernel,K", [("valu", 1288), ("mfma", 1184)])
def test_selectors_hit_every_row_and_column_once(kernel, K):
    n = 19
    cols = DR.selector_columns(K, kernel, n)
    assert len(cols) == n == len(set(cols)) and 0 <= min(cols) and max(cols) == K - 1
    sel = DR.one_hot_rows(cols, K)
    assert sel.shape == (n, K)
    assert torch.equal(sel.float().sum(1), torch.ones(n))
    hit = sel.float().sum(0)
    assert torch.equal(hit[cols], torch.ones(n)) and float(hit.sum()) == n
    # selecting is exact in float64 too: y[m, n] = W[n, k_m] and y[m, n] = x[m, k_n]
    w = DR.randn(21, K)
    assert torch.equal(DR.gemv(f64(sel), f64(w))["y"], f64(w)[:, cols].t())
    x = DR.randn(5, K)
    assert torch.equal(DR.gemv(f64(x), f64(sel))["y"], f64(x)[:, cols])
    if kernel == "valu":
        assert DR.valu_partial_group(K) and K % 32 != 0
        assert cols[1] // 8 == 127 and cols[2] // 8 == 128 and (cols[3] // 8) % 16 == 0 and cols[3] // 8 == K // 8 - 1
    else:
        assert DR.mfma_partial_tail(K) and K % 32 == 0
        assert cols[1] // 32 == 7 and cols[2] // 32 == 8 and cols[3] // 32 == DR.mfma_wave_steps(K)[0] - 1


def test_loop_tail_predicates():
    """The K values of the GPU sweep reach the tails they are named for."""
    assert [DR.valu_partial_group(K) for K in (8, 24, 264, 1024, 1032, 1288, 2048)] == \
        [False, False, False, False, True, True, False]
    assert DR.mfma_wave_steps(32) == [1, 0, 0, 0] and DR.mfma_wave_steps(96) == [1, 1, 1, 0]  # idle waves
    assert DR.mfma_wave_steps(160) == [2, 2, 1, 0]
    assert DR.mfma_wave_steps(1056) == [9, 9, 9, 6] and DR.mfma_wave_steps(1184) == [10, 10, 10, 7]
    assert DR.mfma_wave_steps(1568) == [13, 13, 13, 10] and DR.mfma_wave_steps(2048) == [16] * 4
    assert [DR.mfma_partial_tail(K) for K in (160, 1056, 1184, 1568, 2048)] == [False, True, True, True, False]


def test_proj_case_has_empty_chunks():
    for ns in (1, 3, 5):
        q, k, v, p0, H, ref = DR.proj_case(2, ns)
        assert ref["part"].shape == (2, H, ns, 66)
        assert int(ref["empty"][0, 0].sum()) == max(0, ns - 2)


# ------------------------------------------------------------------ fp32 in another order stays inside the bound
def _inside(got, ref, A, extra=0.0):
    err = (f64(got) - ref).abs()
    ratio = float(((err - DR.BF16_ULP * ref.abs() - extra) / A.clamp_min(1e-300)).max())
    return bool((err <= DR.bound(ref, A, TOL32, extra)).all()), ratio


@pytest.mark.parametrize("B,H,Hkv,D,Lmax,T,p0", [(2, 4, 2, 64, 1024, 1, 1023), (1, 6, 2, 128, 520, 2, 255)])
def test_fp32_attention_in_reverse_order_is_inside_the_bound(B, H, Hkv, D, Lmax, T, p0):
    """Unsplit fp32 softmax over the keys back to front (the kernel: 256-key chunks front to back, then a
    combine), rounded once to bf16."""
    q, k, v = _attn_inputs(B, H, Hkv, D, Lmax, T, p0)
    ref, A = DR.decode_attention(f64(q), f64(k), f64(v), p0, H, T)
    G = H // Hkv
    out = torch.empty(B, T, Hkv, G, D)
    qv = q.float().view(B, T, Hkv, G, D) / math.sqrt(D)
    for t in range(T):
        L = p0 + t + 1
        kf, vf = k[:, :, :L].float().flip(2), v[:, :, :L].float().flip(2)
        s = torch.einsum("bhgd,bhld->bhgl", qv[:, t].flip(-1), kf.flip(-1))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        out[:, t] = torch.einsum("bhgl,bhld->bhgd", e, vf) / e.sum(-1, keepdim=True)
    ok, ratio = _inside(out.reshape(B * T, H * D).to(BF16), ref, A)
    print(f"fp32 attention, reverse order: worst (err - ulp) / A = {ratio:.3e}")
    assert ok


@pytest.mark.parametrize("K", [264, 1288, 5632])
def test_fp32_gemv_in_reverse_order_is_inside_the_bound(K):
    i = DR.gemv_inputs(8, K, 48)
    r = DR.gemv(f64(i["x"]), f64(i["w"]), f64(i["xd"]), f64(i["ln"]))
    s = (i["x"].float() + i["xd"].float()).to(BF16).float()
    ss = (s.flip(-1) * s.flip(-1)).sum(-1, keepdim=True)
    h = (s * torch.rsqrt(ss / K + 1e-5) * i["ln"].float()).to(BF16).float()
    y = (h.flip(-1).unsqueeze(1) * i["w"].float().flip(-1).unsqueeze(0)).cumsum(-1)[..., -1]  # sequential fp32
    ok, ratio = _inside(y.to(BF16), r["y"], r["A"], r["flip"])
    print(f"fp32 gemv K={K}, reverse sequential order: worst (err - ulp - flip) / A = {ratio:.3e}")
    assert ok
    # and through the epilogues
    e = TOL32 * r["A"] + r["flip"]
    ref, A, slack = DR.swiglu_epilogue(r["y"], e)
    g, u = y.to(BF16).float().chunk(2, dim=-1)
    assert _inside((g * torch.sigmoid(g) * u).to(BF16), ref, A, slack)[0]
