"""The float64 references of ``tests/rowwise_refs.py`` against torch's own float64 ops and autograd, and the
invariants of the shared input builders (CPU only)."""

from __future__ import annotations

import pytest
import torch

from . import rowwise_refs as RR

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16]


def close(a: torch.Tensor, b: torch.Tensor, equal_nan: bool = False) -> bool:
    return a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=1e-12, equal_nan=equal_nan)


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def _autograd(fn, x, dy):
    xr = x.clone().requires_grad_(True)
    y = fn(xr)
    y.backward(dy)
    return y.detach(), xr.grad


# ------------------------------------------------------------------ references vs torch
@pytest.mark.parametrize("dim", [-1, 0, 1])
def test_softmax_ref(dim):
    x, dy = 3 * _rand(5, 7, 11), _rand(5, 7, 11, seed=1)
    y, gx = _autograd(lambda t: torch.softmax(t, dim), x, dy)
    assert close(RR.softmax(x, dim), y)
    assert close(RR.softmax_bwd(y, dy, dim), gx)


def test_softmax_ref_inf_as_torch():
    x = 3 * _rand(4, 9)
    x[0, 0] = x[1, ::2] = x[2, :-1] = RR.NEG_INF
    x[3] = RR.NEG_INF
    y, ref = RR.softmax(x), torch.softmax(x, -1)
    assert close(y, ref, equal_nan=True)
    assert torch.isnan(y[3]).all() and not torch.isnan(y[:3]).any()
    assert (y[:3][torch.isinf(x[:3])] == 0).all()
    dy = _rand(4, 9, seed=2)
    xr = x[:3].clone().requires_grad_(True)
    yr = torch.softmax(xr, -1)
    yr.backward(dy[:3])
    assert close(RR.softmax_bwd(y[:3], dy[:3]), xr.grad)


@pytest.mark.parametrize("D", [8, 96])
def test_rope_ref(D):
    from bpe_transformer.ops import reference as R

    cos, sin = R.rope_tables(D, RR.ROPE_MAX_SEQ, 10000.0)
    cos, sin = cos.double(), sin.double()
    x, dy = _rand(*RR.ROPE_SHAPE, D), _rand(*RR.ROPE_SHAPE, D, seed=1)
    for kind in ("none", "s", "b1s"):
        pos = RR.rope_positions(kind)
        p = torch.arange(RR.ROPE_SHAPE[2]) if pos is None else pos
        y, gx = _autograd(lambda t: R.apply_rope(t, cos, sin, pos), x, dy)
        assert close(RR.rope(x, cos, sin, p), y)
        assert close(RR.rope(dy, cos, sin, p, inverse=True), gx)
        # the round trip scales each pair by cos^2 + sin^2 of the fp32 table entries (1 within fp32 rounding)
        n2 = (cos[p] ** 2 + sin[p] ** 2).repeat_interleave(2, dim=-1)
        assert float((n2 - 1).abs().max()) < 2.0 ** -22
        assert close(RR.rope(RR.rope(x, cos, sin, p), cos, sin, p, inverse=True), x * n2)
    # complex multiplication is the same rotation
    p = RR.rope_positions("s")
    z = torch.view_as_complex(x.reshape(*x.shape[:-1], D // 2, 2)) * torch.complex(cos[p], sin[p])
    assert close(RR.rope(x, cos, sin, p), torch.view_as_real(z).flatten(-2))


@pytest.mark.parametrize("case", RR.EMBED_ID_CASES)
def test_embedding_ref(case):
    ids = RR.embedding_ids(case)
    W, dy = _rand(RR.EMBED_VOCAB, 12), _rand(ids.numel(), 12, seed=1)
    y, gW = _autograd(lambda w: torch.nn.functional.embedding(ids, w), W, dy)
    assert torch.equal(RR.embedding(W, ids), y)
    assert close(RR.embedding_bwd(dy, ids, RR.EMBED_VOCAB), gW)


def test_activation_refs():
    x, dy = 4 * _rand(33, 24), _rand(33, 24, seed=1)
    y, gx = _autograd(torch.nn.functional.silu, x, dy)
    assert close(RR.silu(x), y) and close(RR.silu_bwd(x, dy), gx)
    y, gx = _autograd(lambda t: torch.nn.functional.gelu(t, approximate="tanh"), x, dy)
    assert close(RR.gelu(x), y) and close(RR.gelu_bwd(x, dy), gx)
    d = dy[:, :12]
    y, gx = _autograd(lambda t: torch.nn.functional.silu(t[:, :12]) * t[:, 12:], x, d)
    assert close(RR.swiglu(x), y) and close(RR.swiglu_bwd(x, d), gx)


@pytest.mark.parametrize("dtype", DTYPES)
def test_activation_refs_finite_at_the_edges(dtype):
    x = RR.f64(RR.act_edge_input(dtype))
    assert x.shape[1] % RR.vec_elems(dtype) == 0 and (x[0] == 0).all() and torch.signbit(x[0]).any()
    dy = torch.ones_like(x)
    outs = [RR.silu(x), RR.silu_bwd(x, dy), RR.gelu(x), RR.gelu_bwd(x, dy)]
    for flip in (False, True):
        gu = RR.f64(RR.swiglu_edge_input(dtype, flip))
        assert torch.equal(gu[:, : x.shape[1]], x) and gu.shape == (x.shape[0], 2 * x.shape[1])
        outs += [RR.swiglu(gu), RR.swiglu_bwd(gu, dy)]
    for t in outs:
        # finite, and nothing the fp32 arithmetic of the kernels cannot hold: 0 or at least the smallest normal
        assert torch.isfinite(t).all() and ((t == 0) | (t.abs() >= 2.0 ** -126)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_rmsnorm_ref(dtype):
    x, d, w = RR.add_rmsnorm_input(7, 520 if dtype == torch.bfloat16 else 4100, dtype)
    s, y, rstd = RR.add_rmsnorm(RR.f64(x), RR.f64(d), RR.f64(w), 1e-5, dtype)
    assert torch.equal(s, (x.float() + d.float()).to(dtype).double())
    ref = torch.nn.functional.rms_norm(s, (s.shape[-1],), RR.f64(w), 1e-5)
    assert close(y, ref)
    assert close(rstd, 1.0 / torch.sqrt(s.pow(2).mean(-1) + 1e-5))


def test_cross_entropy_ref():
    x = 3 * _rand(9, 50)
    t = torch.randint(0, 50, (9,), generator=torch.Generator().manual_seed(3))
    t[2] = t[7] = RR.IGNORE
    x[0, 5:21] = x[4, ::3] = RR.NEG_INF
    x[0, t[0]] = x[4, t[4]] = 0.25
    xr = x.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(xr, t, ignore_index=RR.IGNORE)
    ref.backward()
    loss, rows, lse, grad = RR.cross_entropy(x, t)
    assert close(loss, ref.detach()) and close(grad, xr.grad)
    assert close(lse, torch.logsumexp(x, -1))
    assert close(rows, torch.nn.functional.cross_entropy(x, t, ignore_index=RR.IGNORE, reduction="none"))
    assert (grad[torch.isinf(x)] == 0).all() and (grad[[2, 7]] == 0).all() and (rows[[2, 7]] == 0).all()
    # no valid row: loss 0, gradient 0, nothing NaN
    loss, rows, _, grad = RR.cross_entropy(x, torch.full((9,), RR.IGNORE))
    assert loss == 0 and (rows == 0).all() and (grad == 0).all()


# ------------------------------------------------------------------ builder invariants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern,N", [(p, n) for p, ns in RR.SOFTMAX_INF_PATTERNS.items() for n in ns])
def test_softmax_inf_builders_keep_a_finite_entry(pattern, N, dtype):
    x = RR.softmax_inf_input(pattern, N, dtype)
    mask = RR.softmax_inf_mask(pattern, N)
    assert x.dtype == dtype and torch.equal(torch.isinf(x), mask) and mask.any()
    assert torch.isfinite(x).any(dim=-1).all()
    assert not torch.isnan(RR.softmax(RR.f64(x))).any()


def test_softmax_inf_patterns_hit_what_they_name():
    assert RR.softmax_inf_mask("first256", 600)[0].nonzero().flatten().tolist() == list(range(256))
    w2 = RR.softmax_inf_mask("wave2", 600)[0].nonzero().flatten().tolist()
    assert w2 == list(range(128, 192)) + list(range(384, 448))
    assert RR.softmax_inf_mask("all_but_last", 5)[0].tolist() == [True] * 4 + [False]
    c = RR.softmax_inf_mask("causal65", 65)
    assert c.shape == (65, 65) and not c[:, 0].any() and c[0, 1:].all() and not c[64].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [600, 5])
def test_softmax_masked_row_builder(N, dtype):
    x, r = RR.softmax_masked_row_input(N, dtype)
    others = [i for i in range(x.shape[0]) if i != r]
    assert torch.isinf(x[r]).all() and torch.isfinite(x[others]).all() and 0 < r < x.shape[0] - 1
    y = RR.softmax(RR.f64(x))
    assert torch.isnan(y[r]).all() and not torch.isnan(y[others]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_spread_builder_underflows_fp32(dtype):
    x = RR.softmax_spread_input(600, dtype)
    assert float(x.float().amax() - x.float().amin()) == 200.0
    assert (torch.softmax(x.float(), -1) == 0).any() and (RR.softmax(RR.f64(x)) > 0).all()


def test_rope_positions_inside_the_table():
    for kind in ("s", "b1s"):
        p = RR.rope_positions(kind)
        assert int(p.min()) == 0 and int(p.max()) == RR.ROPE_MAX_SEQ - 1
    assert RR.rope_positions("none") is None and RR.ROPE_SHAPE[2] <= RR.ROPE_MAX_SEQ


@pytest.mark.parametrize("case", RR.EMBED_ID_CASES)
def test_embedding_id_builders(case):
    ids = RR.embedding_ids(case)
    assert ids.dtype == torch.int64 and int(ids.min()) >= 0 and int(ids.max()) < RR.EMBED_VOCAB
    assert ids.numel() == {"one": 1, "seven": 7}.get(case, 301)
    s = ids.sort().values
    if case == "all_equal":
        assert ids.unique().numel() == 1
    if case == "all_distinct":
        assert ids.unique().numel() == 301
    if case == "last_run":
        assert s[-1] == RR.EMBED_VOCAB - 1 and s[-2] != s[-1] and s[0] == 0
    if case == "seven":
        assert s[0] == 0 and s[-1] == RR.EMBED_VOCAB - 1


def test_embedding_widths_cover_every_chunk_count():
    for dtype, ds in RR.EMBED_DS.items():
        v = RR.vec_elems(dtype)
        chunks = [(d // v + 63) // 64 for d in ds]
        assert all(d % v == 0 for d in ds) and chunks == [1, 2, 3, 5, 9, 16]  # -> C = 1, 2, 4, 8, 16, 16


def test_add_rmsnorm_widths_cover_every_chunk_count():
    ns = RR.ADD_RMS_NS[torch.bfloat16]
    assert [(n // 8 + 63) // 64 for n in ns] == [1, 1, 2, 2, 4, 5, 8]  # C = 1, 1, 2, 2, 4, generic, generic


@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_boundary_vocabs_straddle_the_switch(dtype):
    lo, hi = RR.ce_boundary_vocabs(dtype)
    assert (lo, hi) == ((65535, 65537) if dtype == torch.bfloat16 else (32767, 32769))
    assert lo % 2 == 1 and hi % 2 == 1
    assert RR.ce_uses_register_kernel(lo, dtype) and not RR.ce_uses_register_kernel(lo + 1, dtype)
    assert not RR.ce_uses_register_kernel(hi, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", [0, 1])
def test_ce_position_targets_cover_head_body_tail_last(dtype, side):
    V = RR.ce_boundary_vocabs(dtype)[side]
    t, where = RR.ce_position_targets(V, dtype)
    assert sorted(where) == ["body", "head", "last", "tail"] and sorted(where.values()) == [1, 2, 3, 4]
    for r in range(RR.CE_M):
        head, body_end = RR.ce_row_split(r, V, dtype)
        assert (head > 0) == (r % RR.vec_elems(dtype) != 0)  # odd V: only every vn-th row starts aligned
        if t[r] == RR.IGNORE:
            continue
        assert 0 <= t[r] < V
    h, be = RR.ce_row_split(where["head"], V, dtype)
    assert t[where["head"]] < h
    h, be = RR.ce_row_split(where["tail"], V, dtype)
    assert be <= t[where["tail"]] < V - 1
    h, be = RR.ce_row_split(where["body"], V, dtype)
    assert h <= t[where["body"]] < be
    assert t[where["last"]] == V - 1 and t[5] == RR.IGNORE
    h, be = RR.ce_row_split(0, V, dtype)
    assert h == 0 and t[0] < be
    x = RR.ce_logits(V, dtype)
    ok = t != RR.IGNORE
    assert torch.isfinite(x[ok, t[ok]]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("pattern", RR.CE_INF_PATTERNS)
def test_ce_inf_builders_have_finite_targets(pattern, side, dtype):
    V = RR.ce_boundary_vocabs(dtype)[side]
    x, t, mask = RR.ce_inf_case(pattern, V, dtype)
    vn = RR.vec_elems(dtype)
    assert torch.equal(torch.isinf(x), mask) and mask.any()
    ok = t != RR.IGNORE
    assert ok.sum() == RR.CE_M - 1 and torch.isfinite(x[ok, t[ok]]).all()
    for r in range(RR.CE_M):
        head, body_end = RR.ce_row_split(r, V, dtype)
        cols = mask[r].nonzero().flatten()
        body = mask[r, head:body_end].view(-1, vn)
        whole = int(body.all(dim=1).sum())
        if pattern == "aligned_run16":
            assert cols.numel() == 16 and whole == 16 // vn and (cols[0] - head) % vn == 0
            assert (cols[0] - head) // vn >= 256  # not a thread's first vector (256 threads per row)
        elif pattern == "scattered5":
            assert cols.numel() == 5 and whole == 0
        else:
            assert cols.tolist() == list(range(head)) and whole == 0
    loss, _, _, grad = RR.cross_entropy(RR.f64(x), t)
    assert torch.isfinite(loss) and torch.isfinite(grad).all() and (grad[mask] == 0).all()
