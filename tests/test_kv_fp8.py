"""``DecodeSession(kv_dtype="fp8")`` on the CPU (the oracle path): the fp8 cache is a bf16 cache that holds the
dequantised rows.

The comparison session is a plain session whose cache is ``kv_fp8_refs.DequantisedCache``: a bf16-dtype ``KVCache``
into which the test writes every row quantised and dequantised through the independent float64 path.  Both sessions
then run the same fp32 operations on the same values, so they agree to fp32 round-off; the bound is the one
``tests/test_ragged_decode.py`` uses between its two CPU paths, ``rel <= 1e-9``.
"""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.models import DecodeSession, SpeculativeSession, TransformerLM
from bpe_transformer.models.generation import KVCache, _append_plan

from . import kv_fp8_refs as KR
from . import ragged_refs as RR

TOL = 1e-9


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _model(**kw):
    torch.manual_seed(0)
    cfg = dict(vocab_size=97, context_length=64, d_model=64, num_layers=2, num_heads=4, num_kv_heads=2, d_ff=128)
    cfg.update(kw)
    return TransformerLM(**cfg).float().eval()


def _pair(model, batch, max_len, **kw):
    """(fp8 session, plain session on a bf16-dtype cache of dequantised rows)."""
    a = DecodeSession(model, batch, max_len=max_len, kv_dtype="fp8", **kw)
    b = DecodeSession(model, batch, max_len=max_len, **kw)
    c = a.cache
    b.cache = KR.DequantisedCache(c.k.shape[0], batch, c.k.shape[2], max_len, c.k.shape[4], dtype=torch.bfloat16,
                                  ragged=kw.get("ragged", False))
    assert not a.fast and not b.fast and c.k.dtype == torch.float8_e4m3fn and b.cache.k.dtype == torch.bfloat16
    return a, b


def _same_cache(a, b, lengths):
    from bpe_transformer.ops.decode import kv_dequantize_reference as deq

    for i, n in enumerate(lengths):
        assert torch.equal(deq(a.cache.k[:, i, :, :n], a.cache.k_scale[:, i, :, :n]), b.cache.k[:, i, :, :n])
        assert torch.equal(deq(a.cache.v[:, i, :, :n], a.cache.v_scale[:, i, :, :n]), b.cache.v[:, i, :, :n])


@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 4}, {"remove_rope": True}, {"use_post_norm": True}])
def test_uniform_session_is_a_bf16_cache_of_dequantised_rows(kw):
    model = _model(**kw)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 97, (3, 20), generator=g)
    a, b = _pair(model, 3, 32)
    assert rel(a.prefill(ids[:, :9]), b.prefill(ids[:, :9])) <= TOL
    assert rel(a.prefill(ids[:, 9:14]), b.prefill(ids[:, 9:14])) <= TOL  # a second turn
    for t in range(14, 20):
        assert rel(a.decode(ids[:, t]), b.decode(ids[:, t])) <= TOL, t
    assert a.cache.pos.tolist() == [20] and a.length == 20
    _same_cache(a, b, [20] * 3)


def test_ragged_session_is_a_bf16_cache_of_dequantised_rows():
    model = _model()
    lens = [5, 19, 1]
    g = torch.Generator().manual_seed(2)
    seqs = [torch.randint(0, 97, (n + 6,), generator=g) for n in lens]
    a, b = _pair(model, 3, 40, ragged=True)
    pad = RR.padded([s[:n] for s, n in zip(seqs, lens)])
    assert rel(a.prefill(pad, lens), b.prefill(pad, lens)) <= TOL
    for t in range(3):
        ids = torch.stack([s[n + t] for s, n in zip(seqs, lens)])
        assert rel(a.decode(ids), b.decode(ids)) <= TOL
    act = [True, False, True]
    ids = torch.stack([s[n + 3] for s, n in zip(seqs, lens)])
    la, lb = a.decode(ids, active=act), b.decode(ids, active=act)
    assert rel(la[[0, 2]], lb[[0, 2]]) <= TOL
    # slot 1 goes to a new request; the others keep their bytes
    keep = KR.codes(a.cache.k)[:, [0, 2]].clone()
    new = torch.randint(0, 97, (7,), generator=g)
    a.reset_slot(1), b.reset_slot(1)
    assert rel(a.prefill_slot(1, new), b.prefill_slot(1, new)) <= TOL
    assert torch.equal(KR.codes(a.cache.k)[:, [0, 2]], keep)
    assert a.cache.lengths == b.cache.lengths == [9, 7, 5]
    _same_cache(a, b, a.cache.lengths)


@pytest.mark.parametrize("ragged", [False, True])
def test_prefill_chunk_changes_neither_bytes_nor_logits(ragged):
    """A token attends to the cache as stored, its own window included, so the chunking cannot show.  The chunks are
    other matrix shapes, hence another summation order: the model is float64 here, as in ``test_ragged_decode.py``,
    where that round-off (about 1e-12) lies below the bound; in fp32 it is 2e-7 and says nothing about the cache."""
    model = _model().double()
    ids = torch.randint(0, 97, (2, 23), generator=torch.Generator().manual_seed(3))
    whole = DecodeSession(model, 2, max_len=32, kv_dtype="fp8", ragged=ragged)
    cut = DecodeSession(model, 2, max_len=32, kv_dtype="fp8", ragged=ragged, prefill_chunk=7)
    lens = [23, 11] if ragged else None
    assert rel(cut.prefill(ids, lens), whole.prefill(ids, lens)) <= TOL
    for n, i in zip(lens or [23, 23], range(2)):
        for name in ("k", "v"):
            assert torch.equal(KR.codes(getattr(cut.cache, name))[:, i, :, :n], KR.codes(getattr(whole.cache, name))[:, i, :, :n])
            assert torch.equal(getattr(cut.cache, name + "_scale")[:, i, :, :n], getattr(whole.cache, name + "_scale")[:, i, :, :n])


def test_fp8_plan_never_uses_the_flash_prefill():
    for T, G, chunk in ((30, 1, None), (30, 2, 7), (2, 4, None), (9, 1, None), (8, 1, None)):
        plan = _append_plan(T, G, False, chunk, flash=False)
        assert all(kind in ("cache", "decode") for _, _, kind in plan), plan
        assert sum(w for _, w, _ in plan) == T and all(G * w <= 8 for _, w, kind in plan if kind == "decode")
        assert _append_plan(T, G, False, chunk) == _append_plan(T, G, False, chunk, flash=True)
    assert _append_plan(30, 1, False)[0][2] == "flash"


@pytest.mark.parametrize("D", [16, 64, 128])
def test_nbytes_counts_the_scales(D):
    L, B, Hkv, Lmax = 3, 2, 2, 24
    bf = KVCache(L, B, Hkv, Lmax, D)
    f8 = KVCache(L, B, Hkv, Lmax, D, kv_dtype="fp8")
    assert bf.nbytes() == 2 * L * B * Hkv * Lmax * D * 2
    assert f8.nbytes() == 2 * L * B * Hkv * Lmax * (D + 4)
    assert f8.nbytes() * 2 * D == bf.nbytes() * (D + 4)
    assert f8.k.dtype == torch.float8_e4m3fn and f8.k_scale.shape == (L, B, Hkv, Lmax) and f8.k_scale.dtype == torch.float32


def test_generate_passes_kv_dtype_through():
    model = _model()
    prompt = torch.randint(0, 97, (2, 6), generator=torch.Generator().manual_seed(4))
    out = model.generate(prompt, 5, temperature=0.0, kv_dtype="fp8")
    sess = DecodeSession(model, 2, max_len=11, kv_dtype="fp8")
    assert torch.equal(out, sess.generate(prompt, 5, temperature=0.0))
    dev = model.generate(prompt, 5, temperature=0.0, kv_dtype="fp8", sampler="device", seed=1)
    assert torch.equal(dev, out)
    lst = model.generate([prompt[0], prompt[1, :4]], 5, temperature=0.0, kv_dtype="fp8")
    assert torch.equal(lst[0], out[0]) and lst[1].numel() == 9


def test_value_errors():
    model = _model()
    prompt = torch.randint(0, 97, (1, 4))
    with pytest.raises(ValueError, match="kv_dtype"):
        model.generate(prompt, 2, kv_dtype="int8")
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodeSession(model, 1, max_len=8, kv_dtype="e5m2")
    with pytest.raises(ValueError, match="not supported yet"):
        model.generate(prompt, 2, kv_dtype="fp8", draft_model=model.truncated(1))
    with pytest.raises(ValueError, match="not supported yet"):
        SpeculativeSession(model, model.truncated(1), 1, kv_dtype="fp8")
