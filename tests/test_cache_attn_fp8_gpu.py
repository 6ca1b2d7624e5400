"""``cache_attn`` over the fp8 KV cache (``csrc/flash_attn_cache.hip``, the ``Fp8Cache`` instantiation) and the fp8
``DecodeSession`` that routes every long window to it, on the MI355X.

* The op is bit for bit the route it replaces: ``kv_dequant`` into a zeroed bf16 pair followed by the bf16
  ``cache_attn`` (``tests/test_cache_attn_fp8.py`` checks the rounding argument on the same inputs on the CPU).
* Against float64 on the dequantised caches: ``cache_prefill_refs.TOL_GLOBAL``, unchanged.
* The cache past ``pos + T`` holds byte 0x7F with scale NaN; a NaN in any specified row fails.
* Sessions: the 2-layer models of ``tests/test_kv_fp8_gpu.py``.
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.models import generation as gen
from bpe_transformer.ops import decode as OD

from . import cache_attn_fp8_refs as FR
from . import cache_prefill_refs as CR
from . import decode_refs as DR
from . import kv_fp8_refs as KR
from .decode_refs import BF16

pytestmark = pytest.mark.gpu

NAMES = ("q", "k8", "v8", "ks", "vs", "pos")


def _to(dev, c):
    return [c[n].to(dev) for n in NAMES]


def _bits(t):
    return t.cpu().view(torch.int16)


def _new(c, a):
    return OD.prefill_attention_fp8(*a, c["H"], n_new=c["T"])


def _two_launch(c, a):
    """The route this op replaces: ``kv_dequant`` into a zeroed bf16 pair, then the bf16 ``cache_attn``."""
    q, k8, v8, ks, vs, pos = a
    kd, vd = (torch.zeros(k8.shape, dtype=BF16, device=q.device) for _ in range(2))
    OD.kv_dequant(k8, v8, ks, vs, pos, c["T"], kd, vd)
    return OD.prefill_attention(q, kd, vd, pos, c["H"], n_new=c["T"])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", FR.IDS)
def test_bitwise_the_two_launch_route_and_float64_bound(gpu_device, name, D):
    c = FR.case(D, name)
    a = _to(gpu_device, c)
    out, old = _new(c, a), _two_launch(c, a)
    assert out.shape == c["q"].shape and out.dtype == BF16
    out, old = out.cpu(), old.cpu()
    for b in range(len(c["plist"])):
        got = FR.specified(c, out, b)
        assert torch.isfinite(got).all(), (name, b, "poison or NaN in a specified row")
        r = CR.global_rel(got, c["ref"][b])
        print(f"\n{name} D {D} seq {b}: global rel {r:.3e} (TOL_GLOBAL {CR.TOL_GLOBAL:g})", end="")
        assert torch.equal(_bits(got), _bits(FR.specified(c, old, b))), (name, b)
        assert r < CR.TOL_GLOBAL, (name, b, r)


@pytest.mark.parametrize("D", [64, 128])
def test_batched_call_equals_one_call_per_slot(gpu_device, D):
    c = FR.case(D, "ragged positions")
    q, k8, v8, ks, vs, pos = _to(gpu_device, c)
    out = _new(c, (q, k8, v8, ks, vs, pos)).cpu()
    B, T = len(c["plist"]), c["T"]
    for b in range(B):
        one = OD.prefill_attention_fp8(q[b * T:(b + 1) * T], k8[b:b + 1], v8[b:b + 1], ks[b:b + 1], vs[b:b + 1],
                                       pos[b:b + 1], c["H"], n_new=T)
        assert torch.equal(_bits(one), _bits(out[b * T:(b + 1) * T])), b


@pytest.mark.parametrize("D", [64, 128])
def test_repeat_gives_equal_bits_and_inputs_are_untouched(gpu_device, D):
    c = FR.case(D, "second row block, diagonal across a tile edge")
    a = _to(gpu_device, c)
    first, again = _new(c, a), _new(c, a)
    assert torch.equal(_bits(first), _bits(again))
    q, k8, v8, ks, vs, pos = a
    assert torch.equal(q.cpu(), c["q"]) and torch.equal(pos.cpu(), c["pos"])
    assert torch.equal(KR.codes(k8).cpu(), KR.codes(c["k8"])) and torch.equal(KR.codes(v8).cpu(), KR.codes(c["v8"]))
    for g, w in ((ks, c["ks"]), (vs, c["vs"])):
        assert torch.equal(g.cpu().view(torch.int32), w.view(torch.int32))


@pytest.mark.parametrize("D", [64, 128])
def test_non_finite_value_row(gpu_device, D):
    """The V row of key ``p0 + 5`` carries scale NaN: the tokens that do not see it are bitwise the clean run's,
    the tokens that see it are NaN, as a bf16 cache holding that row gives."""
    c = FR.case(D, "diagonal inside tile 0")
    p0, T, B = c["plist"][0], c["T"], len(c["plist"])
    a = _to(gpu_device, c)
    clean = _new(c, a).cpu().view(B, T, -1)
    vs = a[4].clone()
    vs[:, :, p0 + 5] = math.nan
    a[4] = vs
    got = _new(c, a).cpu().view(B, T, -1)
    bf = _two_launch(c, a).cpu().view(B, T, -1)
    assert torch.isfinite(got[:, :5]).all()
    assert torch.equal(_bits(got[:, :5].contiguous()), _bits(clean[:, :5].contiguous()))
    assert torch.isnan(got[:, 5:]).all() and torch.isnan(bf[:, 5:]).all()


def test_argument_errors(gpu_device):
    dev = gpu_device
    op = torch.ops.bpe_hip.cache_attn_fp8

    def args(D=64, G=1, Hkv=2, B=2, T=9, Lmax=32):
        H = Hkv * G
        q = torch.zeros(B * T, H * D, dtype=BF16, device=dev)
        k8 = torch.zeros(B, Hkv, Lmax, D, dtype=torch.float8_e4m3fn, device=dev)
        s = torch.ones(B, Hkv, Lmax, device=dev)
        return [q, k8, k8.clone(), s, s.clone(), torch.zeros(1, dtype=torch.int32, device=dev), H, 0.125, T]

    assert op(*args()).shape == (18, 128)
    with pytest.raises(RuntimeError):
        op(*args(D=32))
    with pytest.raises(RuntimeError):
        op(*args(G=16))
    a = args()
    a[1] = torch.zeros(a[1].shape, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError):
        op(*a)
    a = args()
    a[3] = a[3][:, :, :-1].contiguous()
    with pytest.raises(RuntimeError):
        op(*a)
    a = args()
    a[4] = a[4][:, :1].contiguous()
    with pytest.raises(RuntimeError):
        op(*a)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ sessions
MODELS = [{}, {"num_kv_heads": 2}, {"d_model": 512, "num_heads": 4, "d_ff": 1024}]  # D 64, G 2, D 128


def rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-12))


def _models(dev, **kw):
    """The 2-layer model of ``tests/test_kv_fp8_gpu.py`` in bf16 on the GPU, and the same bf16-rounded weights in
    fp32 on the CPU (the oracle session's)."""
    torch.manual_seed(0)
    cfg = dict(vocab_size=1000, context_length=256, d_model=256, num_layers=2, num_heads=4, d_ff=512)
    cfg.update(kw)
    gm = TransformerLM(**cfg).to(dev, torch.bfloat16).eval()
    cm = TransformerLM(**cfg).eval()
    cm.load_state_dict({k: v.float().cpu() for k, v in gm.state_dict().items()})
    return gm, cm


class _Spy:
    """The HIP op namespace with the attention and dequantisation lookups recorded."""

    def __init__(self, h):
        self._h, self.seen = h, []

    def __getattr__(self, name):
        if name in ("cache_attn", "cache_attn_fp8", "kv_dequant", "decode_attn", "decode_attn_fp8", "fa_fwd"):
            self.seen.append(name)
        return getattr(self._h, name)


def _spied(monkeypatch, sess):
    spy = _Spy(sess._hip())
    monkeypatch.setattr(sess, "_hip", lambda: spy)
    return spy


@pytest.mark.parametrize("kw", MODELS)
def test_long_windows_are_one_cache_attn_fp8_per_layer(gpu_device, monkeypatch, kw):
    """Prefill 30 on the empty cache, and a second turn of 16 onto 20: ``cache_attn_fp8`` once per layer per window,
    never ``kv_dequant`` or ``cache_attn``."""
    gm, _ = _models(gpu_device, **kw)
    ids = torch.randint(0, 1000, (2, 36), device=gpu_device)
    nl = len(gm.layers)
    first = DecodeSession(gm, 2, max_len=48, kv_dtype="fp8")
    assert first.fast
    spy = _spied(monkeypatch, first)
    first.prefill(ids[:, :30])
    assert spy.seen == ["cache_attn_fp8"] * nl
    second = DecodeSession(gm, 2, max_len=48, kv_dtype="fp8")
    second.prefill(ids[:, :20])
    spy = _spied(monkeypatch, second)
    second.prefill(ids[:, 20:])
    torch.cuda.synchronize()
    assert spy.seen == ["cache_attn_fp8"] * nl
    assert not hasattr(second.cache, "dequant_scratch")


@pytest.mark.parametrize("kw", MODELS)
def test_sessions_match_the_cpu_oracle_session(gpu_device, kw):
    """Prefill 20, a second turn of 16 onto them, one decode step; graph on and off."""
    gm, cm = _models(gpu_device, **kw)
    ids = torch.randint(0, 1000, (2, 37), generator=torch.Generator().manual_seed(3))
    oracle = DecodeSession(cm, 2, max_len=48, kv_dtype="fp8")
    want = [oracle.prefill(ids[:, :20]), oracle.prefill(ids[:, 20:36]), oracle.decode(ids[:, 36])]
    for use_graph in (True, False):
        sess = DecodeSession(gm, 2, max_len=48, use_graph=use_graph, kv_dtype="fp8")
        got = [sess.prefill(ids[:, :20]), sess.prefill(ids[:, 20:36]), sess.decode(ids[:, 36])]
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.isfinite(a).all() and rel(a, b) < 3e-2, (use_graph, i, rel(a, b))


def _two_launch_attend(orig):
    """``KVView.attend`` as it was before ``cache_attn_fp8``: ``kv_dequant`` into a zero-filled one-layer bf16 scratch
    kept on the cache, then the bf16 ``cache_attn``."""

    def attend(self, h, q, li, T, H, kind, combine=True):
        if self.scales is None or kind != "cache":
            return orig(self, h, q, li, T, H, kind, combine)
        k, v, pos = self.k[li], self.v[li], self.pos
        if getattr(self.cache, "_test_scratch", None) is None:
            self.cache._test_scratch = tuple(torch.zeros(self.cache.k.shape[1:], device=k.device, dtype=BF16)
                                             for _ in range(2))
        kd, vd = (t[:k.shape[0]] for t in self.cache._test_scratch)
        h.kv_dequant(k, v, self.scales[0][li], self.scales[1][li], pos, T, kd, vd)
        return h.cache_attn(q, kd, vd, pos, H, 1.0 / math.sqrt(k.shape[-1]), T)

    return attend


@pytest.mark.parametrize("kw", MODELS)
def test_route_change_changes_no_output(gpu_device, monkeypatch, kw):
    """Prefill 30, a second turn, and the same with ``prefill_chunk=7``: logits, cache bytes and scales of the new
    route are ``torch.equal`` to those of the two-launch route it replaces."""
    gm, _ = _models(gpu_device, **kw)
    ids = torch.randint(0, 1000, (2, 46), device=gpu_device)

    def run(chunk):
        sess = DecodeSession(gm, 2, max_len=48, kv_dtype="fp8", prefill_chunk=chunk)
        out = [sess.prefill(ids[:, :30]), sess.prefill(ids[:, 30:])]
        torch.cuda.synchronize()
        c = sess.cache
        return [o.cpu() for o in out], [KR.codes(c.k).cpu(), KR.codes(c.v).cpu(), c.k_scale.cpu(), c.v_scale.cpu()]

    new = {chunk: run(chunk) for chunk in (None, 7)}
    monkeypatch.setattr(gen.KVView, "attend", _two_launch_attend(gen.KVView.attend))
    for chunk in (None, 7):
        lo, co = run(chunk)
        ln, cn = new[chunk]
        for a, b in zip(ln, lo):
            assert torch.isfinite(a).all() and torch.equal(a, b), chunk
        for a, b in zip(cn, co):
            assert torch.equal(a[..., :46, :] if a.dim() == 5 else a[..., :46], b[..., :46, :] if b.dim() == 5 else b[..., :46])


def test_long_window_allocates_no_scratch(gpu_device):
    """``memory_allocated`` after a long-window prefill exceeds its value before by less than one layer's bf16
    K + V, ``4 * B * Hkv * Lmax * D`` bytes: what the dequantisation scratch alone would take."""
    gm, _ = _models(gpu_device)
    B, Lmax = 3, 256
    ids = torch.randint(0, 1000, (B, 40), device=gpu_device)
    warm = DecodeSession(gm, B, max_len=Lmax, use_graph=False, kv_dtype="fp8")
    warm.prefill(ids)  # library workspaces and the like exist from here on
    del warm
    torch.cuda.synchronize()
    sess = DecodeSession(gm, B, max_len=Lmax, use_graph=False, kv_dtype="fp8")
    cap = 4 * B * sess.Hkv * Lmax * sess.D
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    logits = sess.prefill(ids)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    print(f"\nallocated by the prefill and still held: {grown} bytes (cap {cap})", end="")
    assert logits.shape[0] == B and grown < cap, (grown, cap)
