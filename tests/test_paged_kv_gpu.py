"""The paged KV cache on the MI355X: every cache kernel with a block table against the same kernel on the slab, and
``kv_layout="paged"`` sessions against slab sessions.  Every comparison is ``torch.equal`` (NaN-carrying tensors by bit
pattern): a page is ``decode_attn``'s 256-key chunk and four of ``cache_attn``'s 64-key tiles, so a paged kernel runs
the slab kernel's arithmetic, in its order, on the same rows.

The pool is built from a slab (``paged_scatter``) so that a wrong address shows: ``P`` is larger than the pages in
use, the page assignment is a shuffle interleaved across the sequences, every unused page is NaN (fp8: byte 0x7F and
NaN scales), and so is every row at or past a sequence's length inside its last page.  Table entries past the pages a
sequence needs are ``-1``.  Shapes: ``B = 3``, ``Lmax = 600`` (``NB = 3``, a partial last page).
"""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.ops import decode as OD
from bpe_transformer.ops.reference import rope_tables

pytestmark = pytest.mark.gpu

PAGE = OD.KV_PAGE
B, LMAX, NB, P = 3, 600, 3, 12
SHAPES = [(4, 2, 64), (8, 1, 64), (4, 2, 128), (8, 1, 128)]
DEV = "cuda"


def bits(t):
    """A tensor as integers of its element width: equality of bit patterns (NaNs included)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def _gen(*seed):
    return torch.Generator().manual_seed(hash(seed) % (2**31))


def build(Hkv, D, fp8, lens, seed=0, alloc=None):
    """-> (table [B, NB] on the device, pools, slabs): caches whose first ``lens[b]`` rows are random and everything
    else is NaN, as a slab (rows past the allocated pages: zeros, what ``paged_gather`` gives) and scattered into a
    NaN pool.  Each sequence has the pages ``ceil(min(alloc[b], Lmax) / 256)`` needs (``alloc``: ``lens`` unless
    given), the other entries are -1."""
    g = _gen(Hkv, D, fp8, *lens, seed)
    perm = torch.randperm(P, generator=g)[: B * NB].view(NB, B).t().contiguous().int()  # [B, NB], interleaved
    assert not torch.equal(perm, torch.arange(B * NB).view(B, NB).int())
    table = torch.full((B, NB), -1, dtype=torch.int32)
    for b, n in enumerate(alloc or lens):
        nb = -(-min(n, LMAX) // PAGE)
        table[b, :nb] = perm[b, :nb]
    nan = float("nan")
    rows = [torch.randn(B, Hkv, LMAX, D, generator=g).bfloat16() for _ in range(2)]
    if fp8:
        q = [OD.kv_quantize_reference(r) for r in rows]
        slabs = [q[0][0], q[1][0], q[0][1], q[1][1]]
    else:
        slabs = rows
    pools = []
    for i, sl in enumerate(slabs):
        pool = torch.empty(P, Hkv, PAGE, *sl.shape[3:], dtype=sl.dtype)
        if sl.dtype == torch.float8_e4m3fn:
            pool.view(torch.uint8).fill_(0x7F)
        else:
            pool.fill_(nan)
        for b, n in enumerate(lens):  # poison the slab past the length, zero it past the allocated pages
            if sl.dtype == torch.float8_e4m3fn:
                sl.view(torch.uint8)[b, :, min(n, LMAX):] = 0x7F
            else:
                sl[b, :, min(n, LMAX):] = nan
        OD.paged_scatter(sl, pool, table)
        slabs[i] = OD.paged_gather(pool, table, LMAX)
        pools.append(pool.to(DEV))
    slabs = [s.to(DEV) for s in slabs]
    for b, n in enumerate(lens):
        assert same(slabs[0][b, :, :min(n, LMAX)].cpu(), (q[0][0] if fp8 else rows[0])[b, :, :min(n, LMAX)])
    return table.to(DEV), pools, slabs


def _pos(pos):
    return torch.tensor(pos, dtype=torch.int32, device=DEV)


def _q(rows, H, D, *seed):
    return torch.randn(rows, H * D, generator=_gen(rows, H, D, *seed)).bfloat16().to(DEV)


# ------------------------------------------------------------------ decode_attn and its partials
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,Hkv,D", SHAPES)
@pytest.mark.parametrize("pos", [[0, 255, 256], [511, 598, 0], [255], [598], [256]], ids=str)
def test_decode_attn_paged_equals_slab(H, Hkv, D, fp8, pos):
    full = pos if len(pos) == B else pos * B
    table, pools, slabs = build(Hkv, D, fp8, [p + 1 for p in full])
    p = _pos(pos)
    q = _q(B, H, D, *pos)
    att = OD.decode_attention_fp8 if fp8 else OD.decode_attention
    par = OD.decode_attention_partials_fp8 if fp8 else OD.decode_attention_partials
    out = att(q, *pools, p, H, block_table=table, max_len=LMAX)
    assert bool(out.isfinite().all())
    assert same(out, att(q, *slabs, p, H))
    got, ref = par(q, *pools, p, H, block_table=table, max_len=LMAX), par(q, *slabs, p, H)
    # (the o part of an empty chunk is unwritten memory in both: compare m and l everywhere, o where the chunk is live)
    assert same(got[..., D:], ref[..., D:])
    live = ~torch.isinf(ref[..., D])
    assert same(got[..., :D][live], ref[..., :D][live])


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,Hkv,D", [(4, 1, 64), (4, 1, 128)])
@pytest.mark.parametrize("pos", [[255], [255, 254, 510]], ids=str)
def test_decode_attn_window_across_a_page(H, Hkv, D, fp8, pos):
    """T = 2 with G = 4 (8 query rows per kv head) at pos 255: token 0 ends page 0, token 1 starts page 1."""
    T = 2
    full = pos if len(pos) == B else pos * B
    table, pools, slabs = build(Hkv, D, fp8, [p + T for p in full])
    p = _pos(pos)
    q = _q(B * T, H, D, *pos)
    att = OD.decode_attention_fp8 if fp8 else OD.decode_attention
    out = att(q, *pools, p, H, n_new=T, block_table=table, max_len=LMAX)
    assert bool(out.isfinite().all())
    assert same(out, att(q, *slabs, p, H, n_new=T))


# ------------------------------------------------------------------ appends
APPEND = [([250], 12), ([255], 1), ([256], 1), ([595], 12), ([250, 255, 595], 12), ([255, 256, 599], 1)]


def _after_append(pools, slabs, before, table):
    used = set(table.flatten().tolist())
    assert len(used - {-1}) < P
    for pool, slab, old in zip(pools, slabs, before):
        assert same(OD.paged_gather(pool.cpu(), table.cpu(), LMAX), slab.cpu())
        for pg in range(P):
            if pg not in used:
                assert same(pool[pg], old[pg]), pg


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,Hkv,D", SHAPES)
@pytest.mark.parametrize("pos,T", APPEND, ids=str)
def test_kv_append_paged_equals_slab(H, Hkv, D, fp8, pos, T):
    full = pos if len(pos) == B else pos * B
    # rows below pos hold the sequence, the window itself is NaN until the op writes it
    table, pools, slabs = build(Hkv, D, fp8, full, alloc=[p + T for p in full])
    before = [pl.clone() for pl in pools]
    cos, sin = (t.to(DEV) for t in rope_tables(D, LMAX + 16, 10000.0))
    p = _pos(pos)
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D, generator=_gen(H, D, T, *pos)).bfloat16().to(DEV)
    app = OD.kv_append_fp8 if fp8 else OD.kv_append
    q = app(qkv, *pools, cos, sin, p, B, T, H, block_table=table, max_len=LMAX)
    qs = app(qkv, *slabs, cos, sin, p, B, T, H)
    keep = torch.tensor([pb + t < LMAX for pb in full for t in range(T)], device=DEV)  # (a dropped token's q is unspecified)
    assert same(q[keep], qs[keep])
    _after_append(pools, slabs, before, table)
    assert not same(pools[0], before[0])


@pytest.mark.parametrize("K", [64, 40], ids=["mfma", "valu"])  # K % 32 != 0 keeps 3 rows on the VALU kernel
@pytest.mark.parametrize("H,Hkv,D", SHAPES)
@pytest.mark.parametrize("pos", [[255], [256], [600], [255, 256, 599], [0, 600, 511]], ids=str)
def test_decode_qkv_paged_equals_slab(H, Hkv, D, K, pos):
    full = pos if len(pos) == B else pos * B
    table, pools, slabs = build(Hkv, D, False, full, alloc=[p + 1 for p in full])  # the new row is NaN before
    before = [pl.clone() for pl in pools]
    cos, sin = (t.to(DEV) for t in rope_tables(D, LMAX + 16, 10000.0))
    g = _gen(H, D, K, *pos)
    x = torch.randn(B, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn((H + 2 * Hkv) * D, K, generator=g) / K ** 0.5).bfloat16().to(DEV)
    ln = torch.rand(K, generator=g).bfloat16().to(DEV)
    p = _pos(pos)
    q, _ = OD.decode_qkv(x, w, *pools, cos, sin, p, H, ln=ln, block_table=table, max_len=LMAX)
    qs, _ = OD.decode_qkv(x, w, *slabs, cos, sin, p, H, ln=ln)
    keep = torch.tensor([pb < LMAX for pb in full], device=DEV)
    assert same(q[keep], qs[keep])
    _after_append(pools, slabs, before, table)


def test_decode_qkv_single_row_paged_equals_slab():
    """One row runs the VALU kernel's shared-position epilogue."""
    H, Hkv, D, K = 4, 2, 64, 64
    table, pools, slabs = build(Hkv, D, False, [255, 0, 0], alloc=[256, 1, 1])
    before = [pl.clone() for pl in pools]
    cos, sin = (t.to(DEV) for t in rope_tables(D, LMAX + 16, 10000.0))
    g = _gen(1)
    x = torch.randn(1, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn((H + 2 * Hkv) * D, K, generator=g) / 8).bfloat16().to(DEV)
    p = _pos([255])
    q, _ = OD.decode_qkv(x, w, *pools, cos, sin, p, H, block_table=table[:1], max_len=LMAX)
    qs, _ = OD.decode_qkv(x, w, *[s[:1] for s in slabs], cos, sin, p, H)
    assert same(q, qs)
    _after_append(pools, slabs, before, table)


# ------------------------------------------------------------------ cache_attn
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,Hkv,D", SHAPES)
@pytest.mark.parametrize("T", [12, 130])
@pytest.mark.parametrize("pos", [[0], [250], [300], [0, 250, 300]], ids=str)
def test_cache_attn_paged_equals_slab(H, Hkv, D, fp8, T, pos):
    """Tiles that end mid-page (pos + T = 12, 262, 312, 380, 430), windows that cross a page (250 + 12, 250 + 130) and,
    at G = 8 and T = 130, nine 128-row query blocks."""
    full = pos if len(pos) == B else pos * B
    table, pools, slabs = build(Hkv, D, fp8, [p + T for p in full])
    p = _pos(pos)
    q = _q(B * T, H, D, T, *pos)
    fn = OD.prefill_attention_fp8 if fp8 else OD.prefill_attention
    out = fn(q, *pools, p, H, n_new=T, block_table=table, max_len=LMAX)
    assert bool(out.isfinite().all())
    assert same(out, fn(q, *slabs, p, H, n_new=T))


def test_bindings_check_the_pool_and_the_table():
    H, Hkv, D = 4, 2, 64
    table, pools, slabs = build(Hkv, D, False, [10, 10, 10])
    q, p = _q(B, H, D), _pos([9])
    for bad in (dict(block_table=table.long()), dict(block_table=table.t()), dict(block_table=table[:, :2]),
                dict(block_table=table, max_len=NB * PAGE + 1)):
        with pytest.raises(RuntimeError):
            OD.decode_attention(q, *pools, p, H, **{"max_len": LMAX, **bad})
    with pytest.raises(RuntimeError):  # a slab is no pool
        OD.decode_attention(q, *slabs, p, H, block_table=table, max_len=LMAX)
    with pytest.raises(RuntimeError):
        OD.prefill_attention(q, *pools, p, H, block_table=table.cpu(), max_len=LMAX)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_a_slab_smaller_than_the_batch_is_refused(fp8):
    """Without a table dim 0 of the caches is the batch: a slab of two sequences takes no append of three (the
    bindings refuse; nothing is launched)."""
    H, Hkv, D, K = 4, 2, 64, 64
    table, pools, slabs = build(Hkv, D, fp8, [10, 10, 10])
    small = [s[:2].contiguous() for s in slabs]
    keep = [s.clone() for s in small]
    cos, sin = (t.to(DEV) for t in rope_tables(D, LMAX + 16, 10000.0))
    qkv = torch.randn(B, (H + 2 * Hkv) * D).bfloat16().to(DEV)
    app = OD.kv_append_fp8 if fp8 else OD.kv_append
    for p in (_pos([5]), _pos([5, 6, 7])):
        with pytest.raises(RuntimeError, match="mismatch"):
            app(qkv, *small, cos, sin, p, B, 1, H)
        with pytest.raises(RuntimeError):  # and a table with fewer rows than the batch
            app(qkv, *pools, cos, sin, p, B, 1, H, block_table=table[:2].contiguous(), max_len=LMAX)
        if not fp8:
            x, w = torch.randn(B, K).bfloat16().to(DEV), torch.randn((H + 2 * Hkv) * D, K).bfloat16().to(DEV)
            with pytest.raises(RuntimeError, match="mismatch"):
                OD.decode_qkv(x, w, *small, cos, sin, p, H)
            with pytest.raises(RuntimeError):
                OD.decode_qkv(x, w, *pools, cos, sin, p, H, block_table=table[:2].contiguous(), max_len=LMAX)
    assert all(same(a, b) for a, b in zip(small, keep))


# ------------------------------------------------------------------ sessions
def _model():
    torch.manual_seed(0)
    return TransformerLM(vocab_size=211, context_length=640, d_model=128, num_layers=2, num_heads=2, num_kv_heads=1,
                         d_ff=256).to(DEV, torch.bfloat16).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


def _ids(*shape, seed=0):
    return torch.randint(0, 211, shape, generator=torch.Generator().manual_seed(seed))


SESSIONS = {
    "graph": dict(),
    "eager": dict(use_graph=False),
    "device": dict(gen=dict(sampler="device", seed=3, sync_every=8)),
    "fp8": dict(kv_dtype="fp8"),
    "w8": dict(weight_dtype="fp8"),
    "chunked": dict(prefill_chunk=100),
    "small_pool": dict(num_pages=4),  # batch * NB = 6
}


@pytest.mark.parametrize("name", list(SESSIONS))
def test_paged_generate_equals_slab(model, name):
    kw = dict(SESSIONS[name])
    gen = kw.pop("gen", {})
    pool = {"num_pages": kw.pop("num_pages")} if "num_pages" in kw else {}
    prompt = _ids(2, 250, seed=1)
    res = {}
    for layout in ("slab", "paged"):
        sess = DecodeSession(model, 2, max_len=LMAX, kv_layout=layout, **kw, **(pool if layout == "paged" else {}))
        assert sess.fast
        out = sess.generate(prompt, 20, temperature=0.0, **gen)
        res[layout] = (out, sess.decode(out[:, -1]))
        if layout == "paged":
            assert sess.cache.pages_in_use == 4 and sess.length == 270
    assert res["paged"][0].shape == (2, 270)
    assert torch.equal(res["paged"][0], res["slab"][0])
    assert same(res["paged"][1], res["slab"][1])


@pytest.mark.parametrize("name", ["graph", "device", "fp8", "small_pool"])
def test_paged_ragged_generate_equals_slab(model, name):
    kw = dict(SESSIONS[name])
    gen = kw.pop("gen", {})
    pool = {"num_pages": 6} if "num_pages" in kw else {}  # batch * NB = 9; 1 + 2 + 2 pages are needed
    kw.pop("num_pages", None)
    prompts = [_ids(n, seed=n) for n in (10, 250, 300)]
    res = {}
    for layout in ("slab", "paged"):
        sess = DecodeSession(model, 3, max_len=LMAX, ragged=True, kv_layout=layout, **kw,
                             **(pool if layout == "paged" else {}))
        outs = sess.generate(prompts, 20, temperature=0.0, **gen)
        res[layout] = (outs, sess.decode(torch.stack([o[-1] for o in outs])))
        if layout == "paged":
            assert sess.cache.pages_in_use == 5 and sess.cache.lengths == [30, 270, 320]
    for a, b in zip(res["paged"][0], res["slab"][0]):
        assert torch.equal(a, b)
    assert same(res["paged"][1], res["slab"][1])


def test_fork_slot_equals_three_prefills(model):
    prompt = _ids(300, seed=13)
    cont = _ids(3, 6, seed=14).to(DEV)
    sess = {}
    for layout in ("slab", "paged"):
        s = sess[layout] = DecodeSession(model, 3, max_len=LMAX, ragged=True, kv_layout=layout)
        first = s.prefill_slot(0, prompt)
        for b in (1, 2):
            if layout == "paged":
                s.fork_slot(0, b)
            else:
                assert same(s.prefill_slot(b, prompt), first)
    c = sess["paged"].cache
    assert c.pages_in_use == 4  # one shared page, three private ones
    for t in range(3):
        assert same(sess["paged"].decode(cont[:, t]), sess["slab"].decode(cont[:, t])), t
    for s in sess.values():
        s.truncate([303, 100, 303])  # slot 1 back into the shared page: it gets a copy
    assert c.pages_in_use == 4 and c._table[1][0] != c._table[0][0] == c._table[2][0]
    for t in range(3, 6):
        assert same(sess["paged"].decode(cont[:, t]), sess["slab"].decode(cont[:, t])), t
    for b, left in ((1, 3), (0, 2), (2, 0)):
        sess["paged"].reset_slot(b)
        assert c.pages_in_use == left
