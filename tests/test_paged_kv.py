"""The paged KV cache on the CPU: ``paged_gather`` / ``paged_scatter``, the paged ``*_reference`` ops, the oracle path
of a ``kv_layout="paged"`` session, its page allocator and ``fork_slot``.

Every comparison is ``torch.equal``: a paged op is defined as the slab op on the gathered slab, and a paged session
runs the arithmetic of the slab session on the same rows (``ops/decode.py``, "Paged cache").
"""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.ops import decode as dec
from bpe_transformer.ops.reference import rope_tables

PAGE = dec.KV_PAGE


def _model(**kw):
    torch.manual_seed(0)
    cfg = dict(vocab_size=97, context_length=640, d_model=32, num_layers=2, num_heads=2, num_kv_heads=1, d_ff=64)
    cfg.update(kw)
    return TransformerLM(**cfg).float().eval()


def _ids(*shape, seed=0):
    return torch.randint(0, 97, shape, generator=torch.Generator().manual_seed(seed))


def _table(B, NB, P, seed=0):
    """A non-identity page assignment, interleaved across the sequences (entry [b, j] is the (j * B + b)-th page of a
    shuffle of the pool)."""
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))[: B * NB]
    t = perm.view(NB, B).t().contiguous().int()
    assert not torch.equal(t, torch.arange(B * NB).view(B, NB).int())
    return t


# ------------------------------------------------------------------ gather / scatter
def test_page_constant_is_the_kernels():
    assert PAGE == 256


@pytest.mark.parametrize("Lmax", [600, 512])
def test_gather_scatter_round_trip(Lmax):
    B, Hkv, D, P = 3, 2, 8, 12
    NB = -(-Lmax // PAGE)
    table = _table(B, NB, P)
    slab = torch.randn(B, Hkv, Lmax, D)
    pool = torch.full((P, Hkv, PAGE, D), float("nan"))
    assert dec.paged_scatter(slab, pool, table) is pool
    assert torch.equal(dec.paged_gather(pool, table, Lmax), slab)
    used = set(table.flatten().tolist())
    for p in range(P):
        if p not in used:
            assert bool(pool[p].isnan().all()), p
    # a page holds the rows the table says, in place
    assert torch.equal(pool[int(table[1, 1])], slab[1, :, PAGE : 2 * PAGE])
    # rows of the last page past Lmax are left alone
    if Lmax % PAGE:
        assert bool(pool[int(table[0, NB - 1]), :, Lmax % PAGE :].isnan().all())
    # scales (one dim fewer) and unallocated entries
    sc = torch.rand(B, Hkv, Lmax)
    spool = torch.zeros(P, Hkv, PAGE)
    dec.paged_scatter(sc, spool, table)
    assert torch.equal(dec.paged_gather(spool, table, Lmax), sc)
    hole = table.clone()
    hole[2, NB - 1] = -1
    g = dec.paged_gather(pool, hole, Lmax)
    assert torch.equal(g[2, :, (NB - 1) * PAGE :], torch.zeros_like(g[2, :, (NB - 1) * PAGE :]))
    assert torch.equal(g[:2], slab[:2])


# ------------------------------------------------------------------ paged references = slab references on the gather
def _pools(B, Hkv, D, Lmax, P, fp8, seed=0):
    g = torch.Generator().manual_seed(seed)
    NB = -(-Lmax // PAGE)
    table = _table(B, NB, P, seed)
    k = torch.randn(P, Hkv, PAGE, D, generator=g).bfloat16()
    v = torch.randn(P, Hkv, PAGE, D, generator=g).bfloat16()
    if not fp8:
        return table, (k, v)
    k8, ks = dec.kv_quantize_reference(k)
    v8, vs = dec.kv_quantize_reference(v)
    return table, (k8, v8, ks, vs)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("pos", [[255], [0, 256, 598]])
def test_paged_attention_references(fp8, pos):
    B, H, Hkv, D, Lmax = 3, 4, 2, 16, 600
    table, pools = _pools(B, Hkv, D, Lmax, 12, fp8)
    slabs = [dec.paged_gather(p, table, Lmax) for p in pools]
    p = torch.tensor(pos, dtype=torch.int32)
    att = dec.decode_attention_fp8 if fp8 else dec.decode_attention
    pre = dec.prefill_attention_fp8 if fp8 else dec.prefill_attention
    par = dec.decode_attention_partials_fp8 if fp8 else dec.decode_attention_partials
    q = torch.randn(B, H * D).bfloat16()
    assert torch.equal(att(q, *pools, p, H, block_table=table, max_len=Lmax), att(q, *slabs, p, H))
    assert torch.equal(par(q, *pools, p, H, block_table=table, max_len=Lmax), par(q, *slabs, p, H))
    T = 2
    q = torch.randn(B * T, H * D).bfloat16()
    for fn in (att, pre):
        assert torch.equal(fn(q, *pools, p, H, n_new=T, block_table=table, max_len=Lmax), fn(q, *slabs, p, H, n_new=T))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("pos", [[250], [250, 255, 595]])
def test_paged_append_references(fp8, pos):
    B, H, Hkv, D, Lmax, T = 3, 4, 2, 16, 600, 12
    table, pools = _pools(B, Hkv, D, Lmax, 12, fp8, seed=1)
    slabs = [dec.paged_gather(p, table, Lmax) for p in pools]
    before = [p.clone() for p in pools]
    cos, sin = rope_tables(D, Lmax + T, 10000.0)  # (the oracle rotates the dropped tokens too)
    p = torch.tensor(pos, dtype=torch.int32)
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D).bfloat16()
    app = dec.kv_append_fp8 if fp8 else dec.kv_append
    q = app(qkv, *pools, cos, sin, p, B, T, H, block_table=table, max_len=Lmax)
    assert torch.equal(q, app(qkv, *slabs, cos, sin, p, B, T, H))
    used = set(table.flatten().tolist())
    for pool, slab, old in zip(pools, slabs, before):
        assert torch.equal(dec.paged_gather(pool, table, Lmax).float(), slab.float())
        assert not torch.equal(pool.float(), old.float())
        for pg in range(pool.shape[0]):
            if pg not in used:
                assert torch.equal(pool[pg].float(), old[pg].float()), pg
    # decode_qkv: the projection followed by the paged append
    x, w = torch.randn(B, 24).bfloat16(), torch.randn((H + 2 * Hkv) * D, 24).bfloat16()
    if not fp8:
        q, _ = dec.decode_qkv(x, w, *pools, cos, sin, p, H, block_table=table, max_len=Lmax)
        qs, _ = dec.decode_qkv(x, w, *slabs, cos, sin, p, H)
        assert torch.equal(q, qs)
        for pool, slab in zip(pools, slabs):
            assert torch.equal(dec.paged_gather(pool, table, Lmax), slab)


# ------------------------------------------------------------------ session (oracle path, fp32)
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_paged_session_equals_slab_across_a_page_boundary(kv_dtype):
    model = _model()
    ids = _ids(2, 250 + 12)
    out = {}
    for layout in ("slab", "paged"):
        sess = DecodeSession(model, 2, max_len=600, kv_dtype=kv_dtype, kv_layout=layout)
        assert not sess.fast
        lg = [sess.prefill(ids[:, :250])]
        for t in range(250, 262):
            lg.append(sess.decode(ids[:, t]))
        out[layout] = torch.stack(lg)
        if layout == "paged":
            assert sess.cache.pages_in_use == 4 and sess.cache.k.shape[1:] == (6, 1, PAGE, 16)
            assert sess.cache.block_table.dtype == torch.int32 and sess.cache.block_table.shape == (2, 3)
    assert torch.equal(out["paged"], out["slab"])


def test_paged_ragged_and_chunked_session_equals_slab():
    model = _model()
    lens = [10, 250, 300]
    ids = _ids(3, 300, seed=3)
    nxt = _ids(3, 8, seed=4)
    out = {}
    for layout in ("slab", "paged"):
        sess = DecodeSession(model, 3, max_len=600, ragged=True, prefill_chunk=128, kv_layout=layout, num_pages=7 if
                             layout == "paged" else None)
        lg = [sess.prefill(ids, lens)]
        for t in range(8):
            lg.append(sess.decode(nxt[:, t]))
        out[layout] = torch.stack(lg)
    assert torch.equal(out["paged"], out["slab"])
    assert sess.cache.pages_in_use == 1 + 2 + 2  # 18, 258 and 308 tokens


def test_generate_passes_the_layout_through():
    model = _model()
    prompt = _ids(2, 250, seed=5)
    a = model.generate(prompt, 10, temperature=0.0)
    b = model.generate(prompt, 10, temperature=0.0, kv_layout="paged", num_pages=4)
    assert torch.equal(a, b)
    c = model.generate(prompt, 10, temperature=0.0, kv_layout="paged", sampler="device", seed=1)
    assert torch.equal(a, c)
    with pytest.raises(RuntimeError, match="pages"):
        model.generate(prompt, 10, temperature=0.0, kv_layout="paged", num_pages=3)


# ------------------------------------------------------------------ allocator
def _state(sess):
    c = sess.cache
    return (c.pages_in_use, c.pages_free, list(c._len), c.pos.tolist(), c.block_table.tolist(), [list(r) for r in c._table],
            list(c._ref), sorted(c._free))


def test_allocator_counts_and_exhaustion():
    model = _model()
    sess = DecodeSession(model, 2, max_len=600, ragged=True, kv_layout="paged", num_pages=4)  # batch * NB = 6
    c = sess.cache
    assert (c.pages_in_use, c.pages_free) == (0, 4) and c.block_table.tolist() == [[-1] * 3] * 2
    assert c.nbytes() == 2 * c.k.numel() * 4 and c.k.shape == (2, 4, 1, PAGE, 16)
    ids = _ids(2, 300, seed=6)
    sess.prefill(ids, [300, 10])
    assert c.pages_in_use == 3 and c.pages_free == 1
    sess.decode(_ids(2, seed=7))
    assert c.pages_in_use == 3
    sess.prefill_slot(0, _ids(212, seed=8))  # 301 + 212 = 513 tokens: a third page
    assert c.lengths == [513, 11] and c.pages_in_use == 4
    assert c.block_table.tolist() == c._table and sorted(p for r in c._table for p in r if p >= 0) == [0, 1, 2, 3]
    # one more page than fits: nothing changes, and the session goes on
    before = _state(sess)
    with pytest.raises(RuntimeError, match=r"1 needed, 0 free"):
        sess.prefill_slot(1, _ids(250, seed=9))
    assert _state(sess) == before
    lg = sess.prefill_slot(1, _ids(100, seed=10))  # fits in the page it has
    assert lg.shape == (1, 97) and bool(lg.isfinite().all()) and c.lengths == [513, 111] and c.pages_in_use == 4
    # truncate releases the pages wholly past the new lengths; reset_slot all of a slot's
    sess.truncate([256, 5])
    assert c.pages_in_use == 2 and c.block_table[0].tolist()[1:] == [-1, -1]
    sess.truncate([255, 5])
    assert c.pages_in_use == 2
    sess.reset_slot(0)
    assert c.pages_in_use == 1 and c.block_table[0].tolist() == [-1] * 3
    sess.prefill_slot(0, _ids(600, seed=11))  # the pool serves whoever needs it
    assert c.pages_in_use == 4 and c.lengths == [600, 5]
    sess.reset()
    assert (c.pages_in_use, c.pages_free) == (0, 4) and c._ref == [0] * 4 and c.block_table.tolist() == [[-1] * 3] * 2


def test_default_pool_is_never_short():
    sess = DecodeSession(_model(), 2, max_len=600, kv_layout="paged")
    assert sess.cache.num_pages == 6
    sess.prefill(_ids(2, 600, seed=12))
    assert sess.cache.pages_free == 0
    with pytest.raises(ValueError):
        DecodeSession(_model(), 2, max_len=600, num_pages=4)
    with pytest.raises(ValueError):
        DecodeSession(_model(), 2, max_len=600, kv_layout="pages")


# ------------------------------------------------------------------ fork_slot
def _forked(model, prompt, layout, **kw):
    sess = DecodeSession(model, 3, max_len=600, ragged=True, kv_layout=layout, **kw)
    first = sess.prefill_slot(0, prompt)
    if layout == "paged":
        sess.fork_slot(0, 1)
        sess.fork_slot(0, 2)
    else:  # the slab session prefills the prompt into each slot
        for b in (1, 2):
            assert torch.equal(sess.prefill_slot(b, prompt), first)
    return sess


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_fork_slot_shares_the_prefix(kv_dtype):
    model = _model()
    prompt = _ids(300, seed=13)
    cont = _ids(3, 6, seed=14)  # three different continuations
    paged = _forked(model, prompt, "paged", kv_dtype=kv_dtype, num_pages=6)
    slab = _forked(model, prompt, "slab", kv_dtype=kv_dtype)
    c = paged.cache
    assert c.pages_in_use == 4 and c.lengths == [300] * 3 and c.pos.tolist() == [300] * 3
    shared = c._table[0][0]
    assert [r[0] for r in c._table] == [shared] * 3 and c._ref[shared] == 3
    assert len({r[1] for r in c._table}) == 3 and all(c._ref[r[1]] == 1 for r in c._table)
    for t in range(3):
        assert torch.equal(paged.decode(cont[:, t]), slab.decode(cont[:, t])), t
    assert c.pages_in_use == 4
    # truncate into the shared page: slot 1 gets its own copy, the siblings keep theirs
    paged.truncate([303, 100, 303])
    slab.truncate([303, 100, 303])
    assert c._table[1][0] != shared and c._ref[shared] == 2 and c._ref[c._table[1][0]] == 1
    assert c._table[1][1] == -1 and c.pages_in_use == 4  # its partial page went back, the copy came
    for t in range(3, 6):
        assert torch.equal(paged.decode(cont[:, t]), slab.decode(cont[:, t])), t
    # pages return only when the last holder lets go
    paged.reset_slot(1)
    assert c.pages_in_use == 3 and c._ref[shared] == 2
    paged.reset_slot(0)
    assert c.pages_in_use == 2 and c._ref[shared] == 1 and shared not in c._free
    lg = paged.decode(cont[:, 0], active=[False, False, True])
    assert torch.equal(lg[2], slab.decode(cont[:, 0], active=[False, False, True])[2])
    paged.reset_slot(2)
    assert c.pages_in_use == 0 and sorted(c._free) == list(range(6))


def test_fork_slot_limits():
    model = _model()
    prompt = _ids(300, seed=15)
    sess = DecodeSession(model, 3, max_len=600, ragged=True, kv_layout="paged", num_pages=3)
    sess.prefill_slot(0, prompt)
    sess.fork_slot(0, 1)
    before = _state(sess)
    with pytest.raises(RuntimeError, match=r"1 needed, 0 free"):
        sess.fork_slot(0, 2)
    assert _state(sess) == before
    with pytest.raises(AssertionError):
        sess.fork_slot(0, 1)  # dst is not empty
    with pytest.raises(ValueError, match="paged"):
        DecodeSession(model, 2, max_len=600, ragged=True).fork_slot(0, 1)
    # a prompt that ends on a page boundary needs no copy
    s2 = DecodeSession(model, 2, max_len=600, ragged=True, kv_layout="paged", num_pages=2)
    s2.prefill_slot(0, _ids(512, seed=16))
    s2.fork_slot(0, 1)
    assert s2.cache.pages_in_use == 2 and s2.cache._table[0] == s2.cache._table[1]


def test_truncate_of_several_holders_of_a_page():
    """Cuts are taken in order on the counts the earlier ones leave: of the holders that cut into one shared page the
    last keeps the original, and pages that all their holders let go in the call pay for the copies -- a pool with no
    free page serves it."""
    model = _model()
    prompt = _ids(300, seed=17)
    paged = _forked(model, prompt, "paged", num_pages=4)  # one shared page, three private ones: none free
    slab = _forked(model, prompt, "slab")
    c = paged.cache
    shared = c._table[0][0]
    assert c.pages_free == 0
    paged.truncate([100, 100, 100])
    slab.truncate([100, 100, 100])
    assert c.pages_in_use == 3 and c._table[2][0] == shared and c._ref[shared] == 1
    assert len({r[0] for r in c._table}) == 3 and all(r[1:] == [-1, -1] for r in c._table)
    cont = _ids(3, 2, seed=18)
    for t in range(2):
        assert torch.equal(paged.decode(cont[:, t]), slab.decode(cont[:, t])), t
    # a full page that only two forks still share goes back when both let go of it in one call
    long = _ids(520, seed=19)
    paged = _forked(model, long, "paged", num_pages=5)  # pages 0, 1 shared, three private third pages
    slab = _forked(model, long, "slab")
    c = paged.cache
    paged.reset_slot(0)
    slab.reset_slot(0)
    second = c._table[1][1]
    assert c.pages_in_use == 4 and c._ref[second] == 2
    paged.truncate([0, 100, 100])
    slab.truncate([0, 100, 100])
    assert c.pages_in_use == 2 and second in c._free and c._table[1][0] != c._table[2][0]
    assert torch.equal(paged.decode(cont[:, 0], active=[False, True, True])[1:],
                       slab.decode(cont[:, 0], active=[False, True, True])[1:])


def test_device_sampler_returns_the_pages_it_reserved_ahead():
    model = _model()
    sess = DecodeSession(model, 2, max_len=600, kv_layout="paged")
    out = sess.generate(_ids(2, 250, seed=20), 4, temperature=0.0, sampler="device", seed=1, sync_every=16)
    assert out.shape == (2, 254) and sess.cache._len == [253, 253]
    assert sess.cache.pages_in_use == 2  # 250 + 16 tokens were reserved: a second page each, given back
    rag = DecodeSession(model, 2, max_len=600, ragged=True, kv_layout="paged")
    rag.generate([_ids(250, seed=21), _ids(10, seed=22)], 4, temperature=0.0, sampler="device", seed=1, sync_every=16)
    assert rag.cache.lengths == [253, 13] and rag.cache.pages_in_use == 2


def test_a_slab_cache_has_no_pages():
    c = DecodeSession(_model(), 2, max_len=600).cache
    assert (c.pages_in_use, c.pages_free) == (0, 0)
    c.reserve([0, 1], [600, 600])
    c.release([0, 1], [0, 0])
    c.cut([0, 1], [0, 0])


# ------------------------------------------------------------------ what does not compose yet
def test_paged_with_speculative_decoding_is_refused():
    model = _model()
    prompt = _ids(1, 8)
    with pytest.raises(ValueError, match="not supported yet"):
        model.generate(prompt, 4, kv_layout="paged", draft_model=model)
    with pytest.raises(ValueError, match="not supported yet"):
        model.generate(prompt, 4, kv_layout="paged", prompt_lookup=3)
