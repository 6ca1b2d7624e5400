"""Flash prefill over the KV cache (``csrc/flash_attn_cache.hip``, ``ops.decode.prefill_attention``) and the session
paths built on it (``models/generation.py``: multi-token append in one pass, ``prefill_chunk``, slot refill).

Inputs are built on the CPU with fixed seeds and rounded to bf16 (``tests/cache_prefill_refs.py``); the float64
references are those of ``tests/decode_refs.py`` / ``tests/ragged_refs.py``.  Cache rows from ``pos + T`` on hold
NaN / +-inf, and NaN anywhere in a specified output row counts as failure.  ``tests/test_cache_prefill_refs.py``
(CPU) shows every bound here to be met by an emulation of the kernel's rounding points on these same inputs.

* against float64: the flash forward's ``max|got - ref| / max|ref| < 2e-2`` (``tests/test_kernels_gpu.py``);
* against ``decode_attn`` (``G * T <= 8``) and the causal ``fa_fwd`` (``p0 = 0``) on the same inputs: ``< 1e-2``;
* sharp checks that do not depend on the tolerance: last key dominant (``o[t] = V[p0 + t]`` within one bf16 ulp
  plus derived terms), no look-ahead, determinism, inputs untouched, batched == slot by slot bit for bit;
* the session against the model's full forward at the project's ``rel < 3e-2``, with the number of passes over the
  layers counted.

MEASURED: the module prints (``-s``) the worst global ratio, the worst per-(token, head)-row ratio
``max|err| / max|ref|`` and the worst element ``(err - 2^-7 |ref|) / A`` over the op tests.  No per-row threshold
is asserted.  On an MI355X (also in docs/performance.md, "Prefill over a filled cache"): random-input cases
global 6.8e-3, per row 8.6e-3, element 5.6e-3; the look-ahead cases (scores spread over +-8 sigma) 1.1e-2, 2.8e-2
and 3.6e-2.
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.ops import decode as OD

from . import cache_prefill_refs as CR
from . import decode_refs as DR
from .decode_refs import f64

pytestmark = pytest.mark.gpu

WORST = {"global": 0.0, "row": 0.0, "need": -math.inf}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ncache_attn worst: global max|err|/max|ref| {WORST['global']:.3e} (bound {CR.TOL_GLOBAL:g}), "
          f"per-row max|err|/max|ref| {WORST['row']:.3e}, (err - 2^-7|ref|)/A {WORST['need']:.3e}")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16)  # NaN-proof equality


def _run(dev, q, k, v, pos, H, T) -> torch.Tensor:
    """The op on the GPU -> CPU output; checks that the inputs come back untouched."""
    pos = [pos] if isinstance(pos, int) else pos
    qg, kg, vg = q.to(dev), k.to(dev), v.to(dev)
    pg = torch.tensor(pos, dtype=torch.int32, device=dev)
    keep = [t.clone() for t in (qg, kg, vg, pg)]
    out = OD.prefill_attention(qg, kg, vg, pg, H, n_new=T)
    torch.cuda.synchronize()
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.equal(pg, keep[3]) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip((qg, kg, vg), keep))
    return out.cpu()


def _check(out, ref, A, D, what):
    assert torch.isfinite(out).all(), what
    g = CR.global_rel(out, ref)
    row, need = CR.row_measures(out, ref, A, D)
    WORST["global"], WORST["row"], WORST["need"] = max(WORST["global"], g), max(WORST["row"], row), max(WORST["need"], need)
    print(f"\n{what}: global {g:.3e} row {row:.3e} need {need:.3e}", end="")
    assert g < CR.TOL_GLOBAL, (what, g)


# ------------------------------------------------------------------ the op against float64
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T,p0", CR.LENGTHS)
def test_lengths(gpu_device, D, T, p0):
    q, k, v, H, ref, A = CR.length_case(D, T, p0)
    _check(_run(gpu_device, q, k, v, p0, H, T), ref, A, D, f"D{D} T{T} p0 {p0}")


@pytest.mark.parametrize("D", [64, 128])
def test_cache_not_a_tile_multiple(gpu_device, D):
    q, k, v, H, ref, A = CR.length_case(D, 64, 136, Lmax=200)
    _check(_run(gpu_device, q, k, v, 136, H, 64), ref, A, D, f"D{D} Lmax 200")


@pytest.mark.parametrize("G", CR.GROUPS)
def test_groups(gpu_device, G):
    q, k, v, H, ref, A = CR.length_case(64, 40, 70, G=G)
    _check(_run(gpu_device, q, k, v, 70, H, 40), ref, A, 64, f"G{G}")


def test_ragged_positions(gpu_device):
    q, k, v, H, ref, A = CR.ragged_case()
    out = _run(gpu_device, q, k, v, CR.RAGGED_POS, H, CR.RAGGED_T)
    _check(out, ref, A, 64, "ragged")
    # one slot at a time on its views of the caches, with a one-element position: bit for bit the batched call
    T = CR.RAGGED_T
    kg, vg = k.to(gpu_device), v.to(gpu_device)
    qg = q.to(gpu_device).view(len(CR.RAGGED_POS), T, -1)
    for b, p in enumerate(CR.RAGGED_POS):
        pg = torch.tensor([p], dtype=torch.int32, device=gpu_device)
        one = OD.prefill_attention(qg[b], kg[b:b + 1], vg[b:b + 1], pg, H, n_new=T).cpu()
        assert torch.equal(one, out[b * T:(b + 1) * T]), b


def test_full_cache(gpu_device):
    q, k, v, H, p0, n, ref, A = CR.full_case()
    B, T = k.shape[0], q.shape[0] // k.shape[0]
    out = _run(gpu_device, q, k, v, p0, H, T)  # (_run: nothing but o changed)
    _check(out.view(B, T, -1)[:, :n].reshape(B * n, -1), ref, A, 64, "full cache")


# ------------------------------------------------------------------ against the existing kernels
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G,T", [(1, 1), (1, 8), (2, 4), (8, 1), (4, 2)])
@pytest.mark.parametrize("p0", [0, 63, 300])
def test_matches_decode_attn(gpu_device, D, G, T, p0):
    q, k, v, H, ref, A = CR.length_case(D, T, p0, G=G)
    out = _run(gpu_device, q, k, v, p0, H, T)
    pg = torch.tensor([p0], dtype=torch.int32, device=gpu_device)
    old = OD.decode_attention(q.to(gpu_device), k.to(gpu_device), v.to(gpu_device), pg, H, n_new=T).cpu()
    assert CR.global_rel(out, f64(old)) < CR.TOL_KERNELS
    _check(out, ref, A, D, f"D{D} G{G} T{T} p0 {p0}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("T", [9, 64, 129, 200])
def test_matches_flash_forward_on_empty_cache(gpu_device, D, G, T):
    q, k, v, H, ref, A = CR.length_case(D, T, 0, G=G)
    out = _run(gpu_device, q, k, v, 0, H, T)
    B, Hkv = k.shape[:2]
    rows = lambda c: c[:, :, :T].transpose(1, 2).reshape(B * T, Hkv * D).contiguous().to(gpu_device)  # noqa: E731
    none = torch.empty(0, device=gpu_device, dtype=torch.float32)
    fa, _ = torch.ops.bpe_hip.fa_fwd(q.to(gpu_device), rows(k), rows(v), none, none, B, T, H, Hkv, D, True, False,
                                     1.0 / math.sqrt(D))
    assert CR.global_rel(out, f64(fa)) < CR.TOL_KERNELS


# ------------------------------------------------------------------ sharp checks
@pytest.mark.parametrize("D,T,p0", CR.DOMINANT)
def test_last_key_dominant(gpu_device, D, T, p0):
    q, k, v, ref, A, rows = CR.dominant_case(D, T, p0, 0)
    out = f64(_run(gpu_device, q, k, v, p0, k.shape[1], T))
    bound = CR.dominant_bound(rows, ref, A, CR.dominant_extra(q, k, v, p0, T))
    bad = ~((out - rows).abs() <= bound)  # NaN counts as bad
    assert not bad.any(), (int(bad.sum()), float(((out - rows).abs() - bound).max()))


@pytest.mark.parametrize("D,T,p0", CR.DOMINANT)
def test_no_look_ahead(gpu_device, D, T, p0):
    q, k, v, ref, A, nxt = CR.dominant_case(D, T, p0, 1)
    out = _run(gpu_device, q, k, v, p0, k.shape[1], T)
    _check(out, ref, A, D, f"look-ahead D{D} T{T} p0 {p0}")


def test_deterministic(gpu_device):
    q, k, v, H, ref, A = CR.length_case(64, 129, 65, G=1)
    assert torch.equal(_run(gpu_device, q, k, v, 65, H, 129), _run(gpu_device, q, k, v, 65, H, 129))


# ------------------------------------------------------------------ the session
def rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12))


def _bf16_model(gpu_device, **kw):
    torch.manual_seed(0)
    cfg = dict(vocab_size=1000, context_length=256, d_model=256, num_layers=2, num_heads=2, num_kv_heads=2, d_ff=512)
    cfg.update(kw)
    return TransformerLM(**cfg).to(gpu_device, torch.bfloat16).eval()


class _Spy:
    """The HIP op namespace with ``cache_attn`` / ``decode_attn`` lookups counted."""

    def __init__(self, h):
        self._h, self.seen = h, []

    def __getattr__(self, name):
        if name in ("cache_attn", "decode_attn", "fa_fwd"):
            self.seen.append(name)
        return getattr(self._h, name)


def _watch(monkeypatch, sess):
    """-> (list of ``_forward_fast`` calls, spy on the attention ops) from here on."""
    calls, fwd = [], sess._forward_fast
    spy = _Spy(sess._hip())

    def forward(ids, *a, **kw):
        calls.append(tuple(ids.shape))
        return fwd(ids, *a, **kw)

    monkeypatch.setattr(sess, "_forward_fast", forward)
    monkeypatch.setattr(sess, "_hip", lambda: spy)
    return calls, spy


def test_second_turn_is_one_pass(gpu_device, monkeypatch):
    model = _bf16_model(gpu_device)
    ids = torch.randint(0, 1000, (2, 64), device=gpu_device)
    sess = DecodeSession(model, 2, max_len=128)
    assert sess.fast and sess.H // sess.Hkv == 1
    with torch.no_grad():
        full = model(ids).float()
        got = [sess.prefill(ids[:, :20])]
        calls, spy = _watch(monkeypatch, sess)
        got.append(sess.prefill(ids[:, 20:60]))
        assert calls == [(2, 40)] and spy.seen == ["cache_attn"] * len(model.layers)
        monkeypatch.undo()
        for t in range(60, 64):
            got.append(sess.decode(ids[:, t]))
    torch.cuda.synchronize()
    assert sess.length == 64
    want = [full[:, 19], full[:, 59]] + [full[:, t] for t in range(60, 64)]
    for i, (a, b) in enumerate(zip(got, want)):
        assert rel(a, b) < 3e-2, (i, rel(a, b))


def test_prefill_chunk_from_empty_cache(gpu_device, monkeypatch):
    model = _bf16_model(gpu_device)
    ids = torch.randint(0, 1000, (2, 50), device=gpu_device)
    whole, sess = DecodeSession(model, 2, max_len=64), DecodeSession(model, 2, max_len=64, prefill_chunk=16)
    calls, spy = _watch(monkeypatch, sess)
    with torch.no_grad():
        full = model(ids).float()
        lw, lc = whole.prefill(ids), sess.prefill(ids)
    torch.cuda.synchronize()
    assert calls == [(2, 16), (2, 16), (2, 16), (2, 2)]
    nl = len(model.layers)
    assert spy.seen == ["fa_fwd"] * nl + ["cache_attn"] * (2 * nl) + ["decode_attn"] * nl
    assert sess.length == 50 and int(sess.cache.pos) == 50
    assert rel(lc, full[:, 49]) < 3e-2 and rel(lc, lw) < 3e-2


def test_slot_append_beside_graph_decode(gpu_device, monkeypatch):
    """Slot 1 is refilled in two pieces (12 tokens, then 30 more onto the 12 it holds) while slots 0 and 2 go on
    through the captured graph: their logits are those of an undisturbed twin, slot 1 follows a fresh session."""
    dev = gpu_device
    model = _bf16_model(dev)
    g = torch.Generator().manual_seed(3)
    lens = [9, 17, 13]
    ids = torch.randint(0, 1000, (3, 17), generator=g).to(dev)
    new = torch.randint(0, 1000, (42,), generator=g).to(dev)
    steps = torch.randint(0, 1000, (5, 3), generator=g).to(dev)
    a, twin = (DecodeSession(model, 3, max_len=96, ragged=True) for _ in range(2))
    fresh = DecodeSession(model, 1, max_len=96)
    with torch.no_grad():
        for s in (a, twin):
            s.prefill(ids, lens)
            for i in range(2):
                s.decode(steps[i])  # (the graph is captured here)
        assert a._graph is not None
        a.reset_slot(1)
        a.prefill_slot(1, new[:12])
        calls, spy = _watch(monkeypatch, a)
        lg = a.prefill_slot(1, new[12:])
        assert calls == [(1, 30)] and spy.seen == ["cache_attn"] * len(model.layers)
        monkeypatch.undo()
        assert a.cache.lengths == [11, 42, 15] and a.cache.pos.tolist() == [11, 42, 15]
        lf = fresh.prefill(new[None, :])
        assert rel(lg, lf) < 3e-2, rel(lg, lf)
        for i in range(2, 5):
            la, lt, lf = a.decode(steps[i]), twin.decode(steps[i]), fresh.decode(steps[i, 1:2])
            assert torch.equal(la[[0, 2]], lt[[0, 2]]), i
            assert rel(la[1], lf[0]) < 3e-2, (i, rel(la[1], lf[0]))
    torch.cuda.synchronize()


def test_short_append_stays_on_decode_attn(gpu_device, monkeypatch):
    model = _bf16_model(gpu_device)
    ids = torch.randint(0, 1000, (2, 27), device=gpu_device)
    sess = DecodeSession(model, 2, max_len=64)
    with torch.no_grad():
        full = model(ids).float()
        sess.prefill(ids[:, :20])
        calls, spy = _watch(monkeypatch, sess)
        lg = sess.prefill(ids[:, 20:])
    torch.cuda.synchronize()
    assert calls == [(2, 7)] and "cache_attn" not in spy.seen and spy.seen == ["decode_attn"] * len(model.layers)
    assert rel(lg, full[:, 26]) < 3e-2
