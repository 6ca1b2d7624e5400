"""Ragged batches on the CPU: the oracle path of the ragged session, the ``*_reference`` ops with ``[B]`` positions,
``generate`` with a list of prompts, and the invariants of the GPU tests' builders (``tests/ragged_refs.py``).

Session bound: ``rel <= 1e-9`` on a float64 model against each sequence alone through the full forward.  The two
sides differ only by float64 rounding over a few thousand terms (about 1e-12; the uniform float64 session measures
4.7e-16 against the full forward), so 1e-9 separates rounding from any indexing mistake.
"""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.ops import decode as dec
from bpe_transformer.ops.reference import rope_tables

from . import ragged_refs as RR

TOL = 1e-9


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _model(dtype=torch.float64, **kw):
    torch.manual_seed(0)
    cfg = dict(vocab_size=97, context_length=64, d_model=64, num_layers=2, num_heads=4, num_kv_heads=2, d_ff=128)
    cfg.update(kw)
    return TransformerLM(**cfg).to(dtype).eval()


def _seqs(lens, extra, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 97, (n + extra,), generator=g) for n in lens]


def _full(model, seqs):
    with torch.no_grad():
        return [model(s[None])[0] for s in seqs]


# ------------------------------------------------------------------ session (oracle path, float64)
def test_non_ragged_session_keeps_one_position():
    sess = DecodeSession(_model(), 3, max_len=32)
    assert sess.cache.pos.numel() == 1 and sess.cache.lengths is None
    sess.prefill(torch.randint(0, 97, (3, 4)))
    assert sess.cache.pos.tolist() == [4] and sess.length == 4


@pytest.mark.parametrize("kw", [{}, {"use_post_norm": True}, {"remove_rope": True}])
def test_ragged_prefill_decode_and_slot_replacement(kw):
    model = _model(**kw)
    lens = [5, 19, 1, 30]
    seqs = _seqs(lens, 8)
    full = _full(model, seqs)
    sess = DecodeSession(model, 4, max_len=48, ragged=True)
    assert not sess.fast and sess.cache.pos.numel() == 4
    lg = sess.prefill(RR.padded([s[:n] for s, n in zip(seqs, lens)]), lens)
    assert sess.cache.lengths == lens and sess.cache.pos.tolist() == lens and sess.length == 30
    for b in range(4):
        assert rel(lg[b], full[b][lens[b] - 1]) <= TOL, b
    for t in range(4):
        lg = sess.decode(torch.stack([s[n + t] for s, n in zip(seqs, lens)]))
        for b in range(4):
            assert rel(lg[b], full[b][lens[b] + t]) <= TOL, (t, b)
    # slot 1 goes to a new request of another length; the others go on
    others = [(sess.cache.k[:, b, :, :lens[b] + 4].clone(), sess.cache.v[:, b, :, :lens[b] + 4].clone()) for b in (0, 2, 3)]
    new = _seqs([9], 4, seed=1)[0]
    new_full = _full(model, [new])[0]
    sess.reset_slot(1)
    lg1 = sess.prefill_slot(1, new[:9])
    assert sess.cache.lengths == [9, 9, 5, 34] and sess.cache.pos.tolist() == [9, 9, 5, 34]
    assert rel(lg1[0], new_full[8]) <= TOL
    for b, (k0, v0) in zip((0, 2, 3), others):
        assert torch.equal(sess.cache.k[:, b, :, :lens[b] + 4], k0) and torch.equal(sess.cache.v[:, b, :, :lens[b] + 4], v0)
    for t in range(4, 8):
        ids = torch.stack([s[n + t] for s, n in zip(seqs, lens)])
        ids[1] = new[9 + t - 4]
        lg = sess.decode(ids)
        assert rel(lg[1], new_full[9 + t - 4]) <= TOL, t
        for b in (0, 2, 3):
            assert rel(lg[b], full[b][lens[b] + t]) <= TOL, (t, b)


@pytest.mark.parametrize("kw", [{}, {"use_post_norm": True}, {"remove_rope": True}])
def test_uniform_session_equals_ragged_with_equal_lengths(kw):
    """One engine: the shared position is the per-sequence one with equal lengths, bit for bit -- through the
    empty-cache prefill, a prefill onto the filled cache (5 tokens: with G = 2 a chunk of 4 and a tail of 1 where
    the session chunks) and decode steps."""
    model = _model(**kw)
    g = torch.Generator().manual_seed(4)
    uni = DecodeSession(model, 3, max_len=32)
    rag = DecodeSession(model, 3, max_len=32, ragged=True)
    ids = torch.randint(0, 97, (3, 6), generator=g)
    assert torch.equal(uni.prefill(ids), rag.prefill(ids, [6, 6, 6]))
    ids = torch.randint(0, 97, (3, 5), generator=g)
    assert torch.equal(uni.prefill(ids), rag.prefill(ids))
    for _ in range(3):
        ids = torch.randint(0, 97, (3,), generator=g)
        assert torch.equal(uni.decode(ids), rag.decode(ids))
    assert uni.length == rag.length == 14 and uni.cache.pos.tolist() == [14] and rag.cache.pos.tolist() == [14] * 3
    assert torch.equal(uni.cache.k, rag.cache.k) and torch.equal(uni.cache.v, rag.cache.v)


def _append_to_filled_cache(second):
    model = _model()
    first = [5, 12, 3]
    seqs = _seqs([a + b for a, b in zip(first, second)], 2)
    full = _full(model, seqs)
    sess = DecodeSession(model, 3, max_len=32, ragged=True)
    sess.prefill(RR.padded([s[:a] for s, a in zip(seqs, first)]), first)
    lg = sess.prefill(RR.padded([s[a:a + b] for s, a, b in zip(seqs, first, second)]), second)
    tot = [a + b for a, b in zip(first, second)]
    assert sess.cache.lengths == tot and sess.cache.pos.tolist() == tot
    for b in range(3):
        assert rel(lg[b], full[b][tot[b] - 1]) <= TOL, b
    lg = sess.decode(torch.stack([s[n] for s, n in zip(seqs, tot)]))
    for b in range(3):
        assert rel(lg[b], full[b][tot[b]]) <= TOL, b


def test_ragged_append_to_filled_cache():
    """``lengths`` on a filled cache: a second ragged turn on top of a ragged first one."""
    _append_to_filled_cache([7, 1, 4])


def test_ragged_append_chunk_tail():
    """A second turn of 5 tokens at most, which a session that chunks by 8 / G = 4 cuts into 4 + 1: the sequences
    end at the first token, at the chunk's last token and in the tail."""
    _append_to_filled_cache([5, 1, 4])


def test_inactive_sequence_stands_still():
    model = _model()
    lens = [6, 11, 4]
    seqs = _seqs(lens, 4)
    full = _full(model, seqs)
    sess = DecodeSession(model, 3, max_len=24, ragged=True)
    sess.prefill(RR.padded([s[:n] for s, n in zip(seqs, lens)]), lens)
    held = (sess.cache.k[:, 1, :, :11].clone(), sess.cache.v[:, 1, :, :11].clone())
    for t in range(2):
        lg = sess.decode(torch.stack([s[n + t] for s, n in zip(seqs, lens)]), active=[True, False, True])
        for b in (0, 2):
            assert rel(lg[b], full[b][lens[b] + t]) <= TOL
    assert sess.cache.lengths == [8, 11, 6] and sess.cache.pos.tolist() == [8, 11, 6]
    assert torch.equal(sess.cache.k[:, 1, :, :11], held[0]) and torch.equal(sess.cache.v[:, 1, :, :11], held[1])
    lg = sess.decode(torch.stack([seqs[0][8], seqs[1][11], seqs[2][6]]))
    for b, n in enumerate([8, 11, 6]):
        assert rel(lg[b], full[b][n]) <= TOL, b


# ------------------------------------------------------------------ generate with a list
def test_generate_list_matches_tensor_form_on_equal_lengths():
    model = _model()
    prompts = _seqs([6, 6, 6], 0, seed=2)
    sess_t = DecodeSession(model, 3, max_len=16)
    sess_l = DecodeSession(model, 3, max_len=16, ragged=True)
    want = sess_t.generate(torch.stack(prompts), 8, temperature=0.0)
    got = sess_l.generate(prompts, 8, temperature=0.0)
    assert isinstance(got, list) and all(torch.equal(g, w) for g, w in zip(got, want))


def test_generate_list_stops_each_sequence_at_its_eos():
    model = _model()
    lens = [4, 9, 6]
    prompts = _seqs(lens, 0, seed=3)
    free = model.generate(prompts, 10, temperature=0.0)
    assert [o.numel() for o in free] == [n + 10 for n in lens]
    assert all(torch.equal(o[:n], p) for o, n, p in zip(free, lens, prompts))
    # greedy continuation equals each sequence alone through the model without a cache
    for p, o in zip(prompts, free):
        assert torch.equal(o, model.generate(p, 10, temperature=0.0, use_cache=False))
    # an EOS id that sequence 0 emits as its 3rd new token
    eos = int(free[0][lens[0] + 2])
    outs = model.generate(prompts, 10, temperature=0.0, eos_token_id=eos)
    grew = False
    for p, o, f in zip(prompts, outs, free):
        new, ref = o[p.numel():].tolist(), f[p.numel():].tolist()
        stop = ref.index(eos) + 1 if eos in ref else len(ref)
        assert torch.equal(o[:p.numel()], p) and new == ref[:stop]  # ends at its first EOS, unchanged before it
        grew |= len(new) > 3
    assert outs[0].numel() <= lens[0] + 3
    assert grew, "no sequence went on after sequence 0 had finished: pick another seed"


def test_generate_list_needs_a_ragged_session():
    sess = DecodeSession(_model(), 2, max_len=16)
    with pytest.raises(AssertionError):
        sess.generate(_seqs([3, 5], 0), 2, temperature=0.0)


# ------------------------------------------------------------------ reference ops with [B] positions
def _ref_inputs(B, T, H, Hkv, D, Lmax):
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D, generator=g)
    kc, vc = torch.randn(B, Hkv, Lmax, D, generator=g), torch.randn(B, Hkv, Lmax, D, generator=g)
    return qkv, kc, vc


@pytest.mark.parametrize("rope", [True, False])
def test_kv_append_reference_per_sequence(rope):
    B, T, H, Hkv, D, Lmax, pos = 3, 5, 4, 2, 16, 40, [0, 7, 38]
    qkv, kc, vc = _ref_inputs(B, T, H, Hkv, D, Lmax)
    cos, sin = rope_tables(D, Lmax + 8, 10000.0) if rope else (None, None)
    k1, v1 = kc.clone(), vc.clone()
    q = dec.kv_append_reference(qkv, k1, v1, cos, sin, torch.tensor(pos, dtype=torch.int32), B, T, H)
    for b, p in enumerate(pos):
        k2, v2 = kc[b:b + 1].clone(), vc[b:b + 1].clone()
        qb = dec.kv_append_reference(qkv[b * T:(b + 1) * T], k2, v2, cos, sin, torch.tensor([p], dtype=torch.int32), 1, T, H)
        assert torch.equal(q[b * T:(b + 1) * T], qb) and torch.equal(k1[b:b + 1], k2) and torch.equal(v1[b:b + 1], v2)
    assert torch.equal(k1[2, :, :38], kc[2, :, :38]) and not torch.equal(k1[2, :, 38:], kc[2, :, 38:])


@pytest.mark.parametrize("T", [1, 3])
def test_decode_attention_reference_per_sequence(T):
    B, H, Hkv, D, Lmax, pos = 4, 4, 2, 16, 768, [0, 255, 256, 700]
    _, kc, vc = _ref_inputs(B, T, H, Hkv, D, Lmax)
    q = torch.randn(B * T, H * D, generator=torch.Generator().manual_seed(12))
    pt = torch.tensor(pos, dtype=torch.int32)
    o = dec.decode_attention_reference(q, kc, vc, pt, H, None, T)
    for b in range(B):
        ob = dec.decode_attention_reference(q[b * T:(b + 1) * T], kc[b:b + 1], vc[b:b + 1], pt[b:b + 1], H, None, T)
        assert torch.equal(o[b * T:(b + 1) * T], ob)
    if T == 1:
        part = dec.decode_partials_reference(q, kc, vc, pt, H)
        for b in range(B):
            pb = dec.decode_partials_reference(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], pt[b:b + 1], H)
            assert torch.equal(part[b:b + 1], pb)
        # the partials of [B] positions combine to the attention of [B] positions
        y = dec.decode_attn_proj(part, torch.eye(H * D))
        assert rel(y.double(), o.double()) < 1e-5
    # equal elements: what the one-element position gives
    same = dec.decode_attention_reference(q, kc, vc, torch.tensor([300] * B, dtype=torch.int32), H, None, T)
    assert torch.equal(same, dec.decode_attention_reference(q, kc, vc, torch.tensor([300], dtype=torch.int32), H, None, T))


# ------------------------------------------------------------------ the GPU tests' builders
@pytest.mark.parametrize("pos,T,Lmax", [([0, 255, 256, 700], 1, 768), ([0, 253, 254, 600], 4, 768), ([0, 253, 254, 600], 8, 768)])
def test_builders_keep_poison_out_of_every_visible_range(pos, T, Lmax):
    q, k, v, H = RR.attention_case(2, 2, 64, Lmax, pos, T)
    assert RR.visible_is_finite(k, v, pos, T) and RR.poison_is_there(k, v, pos, T)
    assert torch.isfinite(q).all()
    for b, p in enumerate(pos):  # and the poison starts right behind: row pos[b] + T is not finite
        assert not torch.isfinite(k[b, :, p + T]).any() and not torch.isfinite(v[b, :, p + T]).any()
    ref, A = RR.decode_attention(q, k, v, pos, H, T)
    assert torch.isfinite(ref).all() and torch.isfinite(A).all()
    pref = RR.decode_partials(q, k, v, pos, H, T)
    assert torch.isfinite(pref["part"][..., :64]).all() and pref["part"].shape[0] == len(pos) * T


def test_spread_lengths():
    for B in (3, 12):
        n = RR.spread_lengths(B)
        assert len(n) == B and min(n) == 5 and max(n) == 30 and len(set(n)) == B
