"""Ragged batches on the MI355X: the KV-cache kernels with one position per sequence, and the ragged session.

Kernel tests: the float64 references of ``tests/decode_refs.py``, called once per sequence with that sequence's
position (``tests/ragged_refs.py``), and the bound of ``tests/test_decode_kernels_gpu.py`` -- per element
``|got - ref| <= 2^-7 |ref| + TOL32 * A`` for bf16 outputs and ``TOL32 * scale`` for the fp32 partials, with the
project's ``TOL32 = 1e-5`` and that file's derived extra terms for ``decode_qkv``.  No new tolerance.  Every cache
row at or past ``pos[b] + T`` of sequence ``b`` holds NaN / +-inf, so reading sequence ``b`` with a neighbour's
position shows as NaN.  Exact claims (V rows, untouched cache rows, empty-chunk statistics, equal positions vs the
shared position) with ``torch.equal``.

Session tests: the model of ``tests/test_generation_gpu.py`` and its ``rel < 3e-2`` against the full forward of each
sequence alone.
"""

from __future__ import annotations

import functools
import math

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.ops import decode as OD
from bpe_transformer.ops import reference as R

from . import decode_refs as DR
from . import ragged_refs as RR
from .decode_refs import BF16, f64

pytestmark = pytest.mark.gpu

TOL32 = 1e-5


def check(got, ref, A, what, extra=0.0):
    assert got.dtype == BF16, (what, got.dtype)
    g = f64(got).reshape(ref.shape)
    err = (g - ref).abs()
    bad = ~(err <= DR.bound(ref, A, TOL32, extra))  # NaN counts as bad
    need = ((err - DR.BF16_ULP * ref.abs() - extra) / A.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    print(f"{what}: worst required fp32 threshold {float(need.max()):.3e} (TOL32 = {TOL32:g})")
    assert not bad.any(), (what, int(bad.sum()), bad.numel(), float(need.max()))


def check32(got, ref, scale, what):
    assert got.dtype == torch.float32, (what, got.dtype)
    need = ((f64(got) - ref).abs() / scale.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    print(f"{what}: worst required fp32 threshold {float(need.max()) if need.numel() else 0.0:.3e}")
    assert bool((need <= TOL32).all()), (what, float(need.max()))


def _pos(dev, p) -> torch.Tensor:
    return torch.tensor(list(p), dtype=torch.int32, device=dev)


# ------------------------------------------------------------------ decode attention
def _attention(dev, Hkv, G, D, Lmax, pos, T):
    q, k, v, H = RR.attention_case(Hkv, G, D, Lmax, pos, T)
    B = len(pos)
    assert RR.visible_is_finite(k, v, pos, T) and RR.poison_is_there(k, v, pos, T)
    ref, A = RR.decode_attention(q, k, v, pos, H, T)
    pref = RR.decode_partials(q, k, v, pos, H, T)
    qg, kg, vg, pg = q.to(dev), k.to(dev), v.to(dev), _pos(dev, pos)
    out = OD.decode_attention(qg, kg, vg, pg, H, n_new=T).cpu()
    part = torch.ops.bpe_hip.decode_attn(qg, kg, vg, pg, H, 1.0 / math.sqrt(D), False, T).cpu()
    ns = (Lmax + 255) // 256
    assert out.shape == (B * T, H * D) and part.shape == (B * T, H, ns, D + 2)
    assert torch.isfinite(out).all()
    check(out, ref, A, "decode_attention")
    empty, live = pref["empty"], ~pref["empty"]
    # per sequence: the chunks past its own length are empty, with m = -inf and l = 0 exactly
    assert torch.equal(part[..., D][empty], torch.full((int(empty.sum()),), -math.inf))
    assert torch.equal(part[..., D + 1][empty], torch.zeros(int(empty.sum())))
    mref, lref = pref["part"][..., D][live], pref["part"][..., D + 1][live]
    check32(part[..., D][live], mref, mref.abs().clamp_min(1.0), "partials m")
    check32(part[..., D + 1][live], lref, lref, "partials l")
    check32(part[..., :D][live], pref["part"][..., :D][live], pref["A"][live], "partials o")
    return pref


@pytest.mark.parametrize("D,G", [(64, 1), (64, 4), (128, 2)])
def test_attention_ragged_single_token(gpu_device, D, G):
    """Four sequences at 0, 255, 256 and 700 cached tokens over three chunks: 1, 1, 2 and 3 live chunks."""
    pos = [0, 255, 256, 700]
    pref = _attention(gpu_device, 2, G, D, 768, pos, 1)
    live = (~pref["empty"]).view(4, -1, 3)[:, 0]
    assert live.tolist() == [[True, False, False], [True, False, False], [True, True, False], [True, True, True]]


@pytest.mark.parametrize("D,G,T", [(64, 2, 4), (64, 1, 8)])
def test_attention_ragged_multi_token(gpu_device, D, G, T):
    """T new tokens per sequence: the causal window crosses the chunk boundary at 256 in the sequences at 253 and
    254 (from different tokens on) and in neither neighbour."""
    _attention(gpu_device, 2, G, D, 768, [0, 253, 254, 600], T)


# ------------------------------------------------------------------ kv_append
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rope", [True, False])
def test_kv_append_ragged(gpu_device, D, rope):
    """Three sequences at 0, 7 and 38 of 40: the last one drops 3 of its 5 tokens.  Sentinel caches: bitwise
    unchanged outside ``[pos[b], pos[b] + n_b)`` of each sequence, V an exact copy."""
    dev = gpu_device
    B, T, H, Hkv, Lmax, pos = 3, 5, 8, 2, 40, [0, 7, 38]
    W = (H + 2 * Hkv) * D
    qkv = DR.randn(B * T, W, seed=(D, T))
    cos, sin = R.rope_tables(D, Lmax + 8, 10000.0)
    k0, v0 = DR.caches(B, Hkv, Lmax, D, Lmax, seed=93)  # finite sentinel rows everywhere
    kg, vg = k0.to(dev), v0.to(dev)
    q = OD.kv_append(qkv.to(dev), kg, vg, cos.to(dev) if rope else None, sin.to(dev) if rope else None,
                     _pos(dev, pos), B, T, H)
    refs = RR.kv_append(qkv, cos.double() if rope else None, sin.double() if rope else None, pos, T, H, Hkv, D, Lmax)
    q, kc, vc = q.cpu().view(B, T, H, D), kg.cpu(), vg.cpu()
    assert [r["n"] for r in refs] == [5, 5, 2]
    for b, (p, r) in enumerate(zip(pos, refs)):
        n = r["n"]
        # query rows of dropped tokens are unspecified (ops/decode.py): the written tokens only
        check(q[b:b + 1, :n], r["q"][:, :n], r["aq"][:, :n], f"kv_append q[{b}]")
        check(kc[b:b + 1, :, p:p + n], r["k"], r["ak"], f"kv_append k[{b}]")
        assert torch.equal(f64(vc[b:b + 1, :, p:p + n]), r["v"])
        if not rope:
            assert torch.equal(f64(q[b:b + 1, :n]), r["q"][:, :n]) and torch.equal(f64(kc[b:b + 1, :, p:p + n]), r["k"])
        for got, old in ((kc, k0), (vc, v0)):
            assert torch.equal(got[b, :, :p], old[b, :, :p]) and torch.equal(got[b, :, p + n:], old[b, :, p + n:])


# ------------------------------------------------------------------ decode_qkv
@functools.lru_cache(maxsize=None)
def _qkv_inputs(M, K, N):
    return DR.gemv_inputs(M, K, N, seed=3)


QKV_POS = {4: [47, 0, 48, 13], 12: [5, 47, 0, 48, 1, 30, 46, 17, 2, 40, 23, 9]}


@pytest.mark.parametrize("M,K", [(4, 264), (12, 512)])
@pytest.mark.parametrize("D,G", [(64, 4), (128, 2)])
@pytest.mark.parametrize("rope", [True, False])
def test_decode_qkv_ragged(gpu_device, M, K, D, G, rope):
    """M = 4, K = 264: the VALU kernel (K % 32 != 0); M = 12, K = 512: the MFMA kernel.  Distinct positions with the
    first row (0), the last row (47) and a full cache (48 = Lmax: nothing is written for that sequence)."""
    dev = gpu_device
    Hkv, Lmax = 2, 48
    H = Hkv * G
    pos = QKV_POS[M]
    assert len(set(pos)) == M and {0, 47, 48} <= set(pos)
    i = _qkv_inputs(M, K, (H + 2 * Hkv) * D)
    cos, sin = R.rope_tables(D, Lmax + 8, 10000.0)
    k0, v0 = DR.caches(M, Hkv, Lmax, D, Lmax, seed=94)
    kg, vg = k0.to(dev), v0.to(dev)
    q, s = OD.decode_qkv(i["x"].to(dev), i["w"].to(dev), kg, vg, cos.to(dev) if rope else None,
                         sin.to(dev) if rope else None, _pos(dev, pos), H, i["xd"].to(dev), i["ln"].to(dev), 1e-5)
    r = DR.gemv(f64(i["x"]), f64(i["w"]), f64(i["xd"]), f64(i["ln"]), 1e-5)
    e = TOL32 * r["A"] + r["flip"]
    ref, A, slack = RR.qkv_rows(r, e, cos.double() if rope else None, sin.double() if rope else None, pos, H, Hkv, D)
    assert torch.equal(f64(s), r["s"])
    q, kc, vc = q.cpu().view(M, H, D), kg.cpu(), vg.cpu()
    for m, p in enumerate(pos):
        keep = torch.arange(Lmax) != p
        assert torch.equal(kc[m][:, keep], k0[m][:, keep]) and torch.equal(vc[m][:, keep], v0[m][:, keep]), m
        if p >= Lmax:  # dropped: no cache row, and like kv_append's its query row is unspecified
            continue
        got = torch.cat((q[m], kc[m, :, p], vc[m, :, p]), dim=0)
        check(got, ref[m], A[m], f"decode_qkv row {m} at {p}", extra=slack[m])


# ------------------------------------------------------------------ equal positions, refusals
def test_equal_positions_match_shared_position(gpu_device):
    """A ``[B]`` position with all elements equal gives bitwise what the one-element position gives."""
    dev = gpu_device
    B, Hkv, G, D, Lmax, p0 = 3, 2, 2, 64, 600, 300
    H = Hkv * G
    for T in (1, 2):
        q, k, v, _ = RR.attention_case(Hkv, G, D, Lmax, [p0] * B, T)
        qg, kg, vg = q.to(dev), k.to(dev), v.to(dev)
        one, per = _pos(dev, [p0]), _pos(dev, [p0] * B)
        assert torch.equal(OD.decode_attention(qg, kg, vg, one, H, n_new=T), OD.decode_attention(qg, kg, vg, per, H, n_new=T))
        pa, pb = (torch.ops.bpe_hip.decode_attn(qg, kg, vg, p, H, 0.125, False, T).cpu() for p in (one, per))
        live = ~DR.decode_partials(f64(q), f64(k), f64(v), p0, H, T)["empty"]
        assert torch.equal(pa[live], pb[live]) and torch.equal(pa[..., D:], pb[..., D:])
    cos, sin = (t.to(dev) for t in R.rope_tables(D, 48, 10000.0))
    qkv = DR.randn(B * 4, (H + 2 * Hkv) * D, seed=(5,)).to(dev)
    res = []
    for p in (_pos(dev, [7]), _pos(dev, [7] * B)):
        k0, v0 = (t.to(dev) for t in DR.caches(B, Hkv, 48, D, 48, seed=95))
        res.append((OD.kv_append(qkv, k0, v0, cos, sin, p, B, 4, H), k0, v0))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    for M, K in ((3, 264), (3, 512), (12, 512)):  # VALU, MFMA, MFMA > 8 rows
        i = {n: t.to(dev) for n, t in DR.gemv_inputs(M, K, (H + 2 * Hkv) * D, seed=4).items()}
        res = []
        for p in (_pos(dev, [7]), _pos(dev, [7] * M)):
            k0, v0 = (t.to(dev) for t in DR.caches(M, Hkv, 48, D, 48, seed=96))
            qo, s = OD.decode_qkv(i["x"], i["w"], k0, v0, cos, sin, p, H, i["xd"], i["ln"], 1e-5)
            res.append((qo, s, k0, v0))
        assert all(torch.equal(a, b) for a, b in zip(*res)), (M, K)


@pytest.mark.parametrize("bad", ["two of three", "int64", "cpu"])
def test_position_refusals(gpu_device, bad):
    """Host-side checks, no launch: a count that is neither 1 nor B, another dtype, another device."""
    dev = gpu_device
    B, Hkv, G, D, Lmax = 3, 2, 2, 64, 48
    H = Hkv * G
    pos = {"two of three": _pos(dev, [1, 2]), "int64": torch.tensor([1, 2, 3], device=dev),
           "cpu": torch.tensor([1, 2, 3], dtype=torch.int32)}[bad]
    k, v = (t.to(dev) for t in DR.caches(B, Hkv, Lmax, D, Lmax))
    q = DR.queries(B, 1, H, D).to(dev)
    qkv = DR.randn(B, (H + 2 * Hkv) * D).to(dev)
    i = {n: t.to(dev) for n, t in DR.gemv_inputs(B, 264, (H + 2 * Hkv) * D).items()}
    e = torch.empty(0, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        torch.ops.bpe_hip.decode_attn(q, k, v, pos, H, 0.125, True, 1)
    with pytest.raises(RuntimeError):
        torch.ops.bpe_hip.kv_append(qkv, k, v, e, e, pos, B, 1, H, False)
    with pytest.raises(RuntimeError):
        torch.ops.bpe_hip.decode_qkv(i["x"], None, None, 1e-5, i["w"], k, v, e, e, pos, H, False)


# ------------------------------------------------------------------ session
def rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12))


@functools.lru_cache(maxsize=None)
def _bf16_model(dev, gqa: bool):
    torch.manual_seed(0)
    cfg = dict(vocab_size=1000, context_length=256, d_model=256, num_layers=2, num_heads=4, d_ff=512)
    if gqa:
        cfg["num_kv_heads"] = 2
    return TransformerLM(**cfg).to(dev, torch.bfloat16).eval()


@functools.lru_cache(maxsize=None)
def _sequences(dev, gqa: bool, B: int, extra: int = 8):
    """B sequences of spread lengths + ``extra`` further tokens each, with the model's full forward of each
    sequence alone (computed once, shared by the tests below, never modified)."""
    g = torch.Generator().manual_seed(100 + B)
    lens = RR.spread_lengths(B)
    seqs = [torch.randint(0, 1000, (n + extra,), generator=g).to(dev) for n in lens]
    model = _bf16_model(dev, gqa)
    with torch.no_grad():
        full = [model(s[None])[0].float() for s in seqs]
    return lens, seqs, full


def _visible(sess, b):
    n = sess.cache.lengths[b]
    return sess.cache.k[:, b, :, :n], sess.cache.v[:, b, :, :n]


def _start(model, lens, seqs, use_graph, max_len=64):
    sess = DecodeSession(model, len(lens), max_len=max_len, use_graph=use_graph, ragged=True)
    assert sess.fast and sess.cache.pos.numel() == len(lens)
    ids = RR.padded([s[:n] for s, n in zip(seqs, lens)])
    return sess, sess.prefill(ids, lens)


@pytest.mark.parametrize("gqa", [False, True])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("B", [3, 12])
def test_ragged_session_matches_full_forward(gpu_device, gqa, use_graph, B):
    """Ragged prefill + 8 teacher-forced decode steps (B = 3: the fused skinny-GEMM step, B = 12: the library-GEMM
    step); every sequence against its own full forward at the same position."""
    model = _bf16_model(gpu_device, gqa)
    lens, seqs, full = _sequences(gpu_device, gqa, B)
    assert min(lens) == 5 and max(lens) == 30 and len(set(lens)) > 1
    sess, lg = _start(model, lens, seqs, use_graph)
    got = [lg]
    for t in range(8):
        got.append(sess.decode(torch.stack([s[n + t] for s, n in zip(seqs, lens)])))
    torch.cuda.synchronize()
    assert sess.cache.lengths == [n + 8 for n in lens] and sess.length == max(lens) + 8
    assert sess.cache.pos.tolist() == sess.cache.lengths
    for t, lg in enumerate(got):
        for b in range(B):
            r = rel(lg[b], full[b][lens[b] - 1 + t])
            assert r < 3e-2, (t, b, r)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("B", [3, 9])
def test_both_position_layouts_match_full_forward(gpu_device, use_graph, B):
    """The shared-position session and a ragged one with equal lengths run the same engine: empty-cache prefill
    (T = 6), filled-cache prefill (T = 5; G = 2: a chunk of 4 and a tail of 1) and 3 decode steps (B = 3: the fused
    skinny-GEMM step, B = 9: the library-GEMM step), each against the full forward under the bound of
    ``test_ragged_session_matches_full_forward``; both end at the same host length, in their own position layout."""
    dev = gpu_device
    model = _bf16_model(dev, True)
    L = 6 + 5 + 3
    seqs = torch.randint(0, 1000, (B, L), generator=torch.Generator().manual_seed(200 + B)).to(dev)
    with torch.no_grad():
        full = model(seqs).float()
    ends = []
    for ragged in (False, True):
        sess = DecodeSession(model, B, max_len=64, use_graph=use_graph, ragged=ragged)
        assert sess.fast and sess.cache.pos.numel() == (B if ragged else 1)
        got = {5: sess.prefill(seqs[:, :6], [6] * B) if ragged else sess.prefill(seqs[:, :6])}
        got[10] = sess.prefill(seqs[:, 6:11])
        for t in range(11, L):
            got[t] = sess.decode(seqs[:, t])
        torch.cuda.synchronize()
        assert sess.cache.pos.tolist() == ([L] * B if ragged else [L])
        assert sess.cache.lengths == ([L] * B if ragged else None)
        ends.append(sess.length)
        for t, lg in got.items():
            for b in range(B):
                r = rel(lg[b], full[b, t])
                assert r < 3e-2, (ragged, t, b, r)
    assert ends == [L, L]


@pytest.mark.parametrize("B", [3, 12])
def test_ragged_graph_replay_equals_eager(gpu_device, B):
    model = _bf16_model(gpu_device, False)
    lens, seqs, _ = _sequences(gpu_device, False, B)
    a, _ = _start(model, lens, seqs, True)
    b, _ = _start(model, lens, seqs, False)
    for t in range(8):
        ids = torch.stack([s[n + t] for s, n in zip(seqs, lens)])
        la, lb = a.decode(ids), b.decode(ids)
        assert rel(la, lb) < 1e-3
    assert a.cache.lengths == b.cache.lengths and torch.equal(a.cache.pos, b.cache.pos)
    for i in range(B):
        assert all(torch.equal(x, y) for x, y in zip(_visible(a, i), _visible(b, i))), i


@pytest.mark.parametrize("use_graph", [True, False])
def test_slot_replacement(gpu_device, use_graph):
    """4 steps, slot 1 is reset and given a new prompt of another length, 4 more steps: slot 1 follows the new
    sequence's full forward, and the other slots' visible cache rows are bitwise those of an undisturbed twin."""
    dev = gpu_device
    model = _bf16_model(dev, True)
    lens, seqs, full = _sequences(dev, True, 3)
    new_len = 11
    assert new_len != lens[1]
    new = torch.randint(0, 1000, (new_len + 4,), generator=torch.Generator().manual_seed(7)).to(dev)
    with torch.no_grad():
        new_full = model(new[None])[0].float()
    sess, _ = _start(model, lens, seqs, use_graph)
    twin, _ = _start(model, lens, seqs, use_graph)
    for t in range(4):
        ids = torch.stack([s[n + t] for s, n in zip(seqs, lens)])
        sess.decode(ids)
        twin.decode(ids)
    before = [[x.clone() for x in _visible(sess, b)] for b in (0, 2)]
    sess.reset_slot(1)
    assert sess.cache.lengths[1] == 0
    lg1 = sess.prefill_slot(1, new[:new_len])
    assert sess.cache.lengths == [lens[0] + 4, new_len, lens[2] + 4] and sess.cache.pos.tolist() == sess.cache.lengths
    assert all(torch.equal(x, y) for b, old in zip((0, 2), before) for x, y in zip(_visible(sess, b), old))
    assert rel(lg1[0], new_full[new_len - 1]) < 3e-2
    for t in range(4, 8):
        ids = torch.stack([s[n + t] for s, n in zip(seqs, lens)])
        twin.decode(ids)
        ids[1] = new[new_len + t - 4]
        lg = sess.decode(ids)
        assert rel(lg[1], new_full[new_len + t - 4]) < 3e-2, t
        for b in (0, 2):
            assert rel(lg[b], full[b][lens[b] + t]) < 3e-2, (t, b)
    torch.cuda.synchronize()
    for b in (0, 2):
        assert all(torch.equal(x, y) for x, y in zip(_visible(sess, b), _visible(twin, b))), b


@pytest.mark.parametrize("use_graph", [True, False])
def test_inactive_sequence_stands_still(gpu_device, use_graph):
    """Sequence 1 is inactive for two steps: its position, host length and visible rows do not change, and it
    resumes where it stopped; the others match their full forward throughout."""
    dev = gpu_device
    model = _bf16_model(dev, False)
    lens, seqs, full = _sequences(dev, False, 3)
    sess, _ = _start(model, lens, seqs, use_graph)
    fed = [0, 0, 0]  # tokens fed per sequence after the prompt

    def step(active):
        ids = torch.stack([s[n + f] for s, n, f in zip(seqs, lens, fed)])
        lg = sess.decode(ids, active=torch.tensor(active))
        for b in range(3):
            if active[b]:
                assert rel(lg[b], full[b][lens[b] + fed[b]]) < 3e-2, (b, fed)
                fed[b] += 1

    step([True, True, True])
    held = [x.clone() for x in _visible(sess, 1)]
    step([True, False, True])
    step([True, False, True])
    assert sess.cache.lengths == [lens[0] + 3, lens[1] + 1, lens[2] + 3] and sess.cache.pos.tolist() == sess.cache.lengths
    assert all(torch.equal(x, y) for x, y in zip(_visible(sess, 1), held))
    step([True, True, True])
    step([True, True, True])
    assert sess.cache.lengths == [lens[0] + 5, lens[1] + 3, lens[2] + 5]


def test_generate_list_on_gpu(gpu_device):
    """``model.generate([p0, p1, p2])`` (graph-captured): prompts kept, and every sequence greedy-continued as the
    model continues it alone."""
    dev = gpu_device
    model = _bf16_model(dev, False)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 1000, (n,), generator=g).to(dev) for n in (5, 17, 9)]
    outs = model.generate(prompts, 6, temperature=0.0)
    assert isinstance(outs, list) and [o.numel() for o in outs] == [11, 23, 15]
    for p, o in zip(prompts, outs):
        assert torch.equal(o[:p.numel()], p)
        alone = model.generate(p, 1, temperature=0.0, use_cache=False)
        assert int(o[p.numel()]) == int(alone[p.numel()])
