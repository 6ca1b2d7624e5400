"""Packed multi-request prefill on the MI355X: ``kv_append_packed`` / ``prefill_attention_packed`` (bf16 and fp8
caches, slab and paged) bit for bit against the existing kernels called slot by slot, the attention against float64,
the dominant-key and look-ahead cases embedded among packed neighbours, ``DecodeSession.prefill_slots`` and the
engine's ``prefill_tokens`` admission.  Inputs: ``tests/packed_prefill_refs.py`` (``tests/test_packed_prefill.py``
shows on the CPU that they meet the bounds asserted here).

Bounds: the bit-for-bit checks need none; the attention is within ``CR.TOL_GLOBAL`` (2e-2, the flash forward's) of
float64; session logits within the project's ``rel < 3e-2`` of the model's full forward.  The engine check is
numerical, because a packed admission's first logits equal the unpacked ones only up to GEMM rounding: every emitted
token of the greedy request must be an argmax of the fp32 teacher-forced forward up to ``3e-2 * max|logits|``, and its
log-prob within that margin of the reference's -- asserted on the unpacked engine first, so the bound rejects only
what the reference path itself does not produce."""

from __future__ import annotations

import copy
import functools
import math

import pytest
import torch

from bpe_transformer.models import DecodeSession, ServingEngine, SamplingParams, TransformerLM
from bpe_transformer.ops import decode as OD

from . import cache_prefill_refs as CR
from . import packed_prefill_refs as PR
from .decode_refs import f64

pytestmark = pytest.mark.gpu

BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float8_e4m3fn: torch.uint8,
        torch.int32: torch.int32}
WORST = {"global": 0.0, "row": 0.0, "need": -math.inf}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ncache_attn_packed worst: global max|err|/max|ref| {WORST['global']:.3e} (bound {CR.TOL_GLOBAL:g}), "
          f"per-row max|err|/max|ref| {WORST['row']:.3e}, (err - 2^-7|ref|)/A {WORST['need']:.3e}")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(BITS[t.dtype])  # NaN-proof equality


def same(a, b) -> bool:
    return torch.equal(bits(a), bits(b))


def packed(c: PR.Case, dev) -> OD.PackedPrompts:
    return OD.PackedPrompts(c.slots, c.lens, dev, pos_host=c.pos)


def dev_pos(c: PR.Case, dev) -> torch.Tensor:
    return torch.tensor(c.pos_all, dtype=torch.int32, device=dev)


def fp8_caches(c: PR.Case, dev):
    k8, ks = OD.kv_quantize_reference(c.k)
    v8, vs = OD.kv_quantize_reference(c.v)
    return [t.to(dev) for t in (k8, v8, ks, vs)]


def attend(c: PR.Case, dev, fmt: str = "bf16"):
    """The packed attention of a case -> (CPU output, the per-slot outputs of the existing op); inputs, the idle slot
    and every position are checked to come back untouched."""
    q, pos, pk = c.q.to(dev), dev_pos(c, dev), packed(c, dev)
    caches = [c.k.to(dev), c.v.to(dev)] if fmt == "bf16" else fp8_caches(c, dev)
    keep = [t.clone() for t in (q, pos, *caches)]
    if fmt == "bf16":
        out = OD.prefill_attention_packed(q, *caches, pos, pk, c.H)
    else:
        out = OD.prefill_attention_packed_fp8(q, *caches, pos, pk, c.H)
    one = []
    for i, s, o, n, p in c.seqs():
        views = [t[s:s + 1] for t in caches]
        fn = OD.prefill_attention if fmt == "bf16" else OD.prefill_attention_fp8
        one.append(fn(q[o:o + n], *views, pos[s:s + 1], c.H, n_new=n).cpu())
    torch.cuda.synchronize()
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert all(same(a, b) for a, b in zip((q, pos, *caches), keep))
    return out.cpu(), one


def check64(out, ref, A, D, what):
    assert torch.isfinite(out).all(), what
    g = CR.global_rel(out, ref)
    row, need = CR.row_measures(out, ref, A, D)
    WORST["global"], WORST["row"], WORST["need"] = max(WORST["global"], g), max(WORST["row"], row), max(WORST["need"], need)
    print(f"\n{what}: global {g:.3e} row {row:.3e} need {need:.3e}", end="")
    assert g < CR.TOL_GLOBAL, (what, g)


# ------------------------------------------------------------------ the attention
@pytest.mark.parametrize("D", PR.DIMS)
@pytest.mark.parametrize("G", PR.GROUPS)
def test_attention_bits_and_float64(gpu_device, D, G):
    c = PR.base_case(D, G)
    out, one = attend(c, gpu_device)
    for (i, s, o, n, p), single, (ref, A) in zip(c.seqs(), one, PR.reference(D, G)):
        assert same(out[o:o + n], single), (i, s)
        check64(out[o:o + n], ref, A, D, f"D{D} G{G} seq {i} (slot {s}, n {n}, pos {p})")


@pytest.mark.parametrize("D", PR.DIMS)
@pytest.mark.parametrize("G", (1, 4))
def test_attention_fp8_bits(gpu_device, D, G):
    c = PR.base_case(D, G)
    out, one = attend(c, gpu_device, "fp8")
    for (i, s, o, n, p), single in zip(c.seqs(), one):
        assert same(out[o:o + n], single) and torch.isfinite(out[o:o + n]).all(), (i, s)


def test_attention_at_lmax(gpu_device):
    c = PR.full_case()
    out, one = attend(c, gpu_device)
    for (i, s, o, n, p), single, (ref, A) in zip(c.seqs(), one, PR.reference(c.D, c.G, "full")):
        w = PR.written(c, i)  # the rows of dropped tokens are unspecified
        assert same(out[o:o + w], single[:w]), i
        check64(out[o:o + w], ref, A, c.D, f"Lmax seq {i} ({w} of {n} tokens fit)")


def pools(c: PR.Case, tensors, dev):
    """The slabs ``tensors`` scattered into pools through a permuted block table; unnamed pool rows hold poison (bf16)
    or zeros."""
    nb = -(-PR.LMAX // OD.KV_PAGE)
    table = PR.page_table(nb)
    out = []
    for t in tensors:
        pool = torch.zeros(PR.B * nb, PR.HKV, OD.KV_PAGE, *t.shape[3:], dtype=t.dtype)
        if t.dtype == torch.bfloat16:
            pool.fill_(math.nan)
        out.append(OD.paged_scatter(t.cpu(), pool, table).to(dev))
    return out, table.to(dev)


@pytest.mark.parametrize("fmt", ("bf16", "fp8"))
@pytest.mark.parametrize("D,G", [(64, 2), (128, 3)])
def test_paged_equals_slab(gpu_device, fmt, D, G):
    dev = gpu_device
    c = PR.base_case(D, G)
    q, qkv, pos, pk = c.q.to(dev), c.qkv.to(dev), dev_pos(c, dev), packed(c, dev)
    cos, sin = (t.to(dev) for t in PR.rope_tables(D))
    slabs = [c.k.to(dev), c.v.to(dev)] if fmt == "bf16" else fp8_caches(c, dev)
    pool, table = pools(c, slabs, dev)
    tail = dict(block_table=table, max_len=PR.LMAX)
    att = OD.prefill_attention_packed if fmt == "bf16" else OD.prefill_attention_packed_fp8
    app = OD.kv_append_packed if fmt == "bf16" else OD.kv_append_packed_fp8
    assert same(att(q, *pool, pos, pk, c.H, **tail), att(q, *slabs, pos, pk, c.H))
    assert same(app(qkv, *pool, cos, sin, pos, pk, c.H, **tail), app(qkv, *slabs, cos, sin, pos, pk, c.H))
    torch.cuda.synchronize()
    for p, s in zip(pool, slabs):
        assert same(OD.paged_gather(p, table, PR.LMAX), s)
    assert pos.tolist() == c.pos_all


# ------------------------------------------------------------------ the append
@pytest.mark.parametrize("fmt", ("bf16", "fp8"))
@pytest.mark.parametrize("D,G,which", [(64, 1, "base"), (64, 2, "full"), (128, 3, "base"), (128, 8, "base")])
def test_append_bits(gpu_device, fmt, D, G, which):
    dev = gpu_device
    c = PR.base_case(D, G) if which == "base" else PR.full_case(D, G)
    qkv, pos, pk = c.qkv.to(dev), dev_pos(c, dev), packed(c, dev)
    cos, sin = (t.to(dev) for t in PR.rope_tables(D))
    start = [c.k.to(dev), c.v.to(dev)] if fmt == "bf16" else fp8_caches(c, dev)
    a, b = [t.clone() for t in start], [t.clone() for t in start]
    keep = qkv.clone()
    if fmt == "bf16":
        q = OD.kv_append_packed(qkv, *a, cos, sin, pos, pk, c.H)
    else:
        q = OD.kv_append_packed_fp8(qkv, *a, cos, sin, pos, pk, c.H)
    fn = OD.kv_append if fmt == "bf16" else OD.kv_append_fp8
    for i, s, o, n, p in c.seqs():
        one = fn(qkv[o:o + n], *[t[s:s + 1] for t in b], cos, sin, pos[s:s + 1], 1, n, c.H)
        w = PR.written(c, i)  # the q rows of dropped tokens are unspecified
        assert same(q[o:o + w], one[:w]), (i, s)
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(a, b))
    assert all(same(x[PR.IDLE], y[PR.IDLE]) for x, y in zip(a, start)) and not same(a[0], start[0])
    assert same(qkv, keep) and pos.tolist() == c.pos_all


# ------------------------------------------------------------------ sharp cases
@pytest.mark.parametrize("D,T,p0", CR.DOMINANT)
def test_last_key_dominant_among_neighbours(gpu_device, D, T, p0):
    c, ref, A, rows = PR.dominant_case(D, T, p0, 0)
    out, one = attend(c, gpu_device)
    s = c.slots[0]
    bound = CR.dominant_bound(rows, ref, A, CR.dominant_extra(c.q[:T], c.k[s:s + 1], c.v[s:s + 1], p0, T))
    bad = ~((f64(out[:T]) - rows).abs() <= bound)  # NaN counts as bad
    assert not bad.any(), (int(bad.sum()), float(((f64(out[:T]) - rows).abs() - bound).max()))
    assert same(out[:T], one[0])


@pytest.mark.parametrize("D,T,p0", CR.DOMINANT)
def test_no_look_ahead_among_neighbours(gpu_device, D, T, p0):
    c, ref, A, nxt = PR.dominant_case(D, T, p0, 1)
    out, one = attend(c, gpu_device)
    check64(out[:T], ref, A, D, f"look-ahead D{D} T{T} p0 {p0}")
    assert same(out[:T], one[0])


def test_deterministic(gpu_device):
    c = PR.base_case(64, 2)
    assert same(attend(c, gpu_device)[0], attend(c, gpu_device)[0])
    assert same(attend(c, gpu_device, "fp8")[0], attend(c, gpu_device, "fp8")[0])


def test_bindings_refuse_a_bad_table(gpu_device):
    dev = gpu_device
    c = PR.base_case(64, 1)
    q, k, v, pos = c.q.to(dev), c.k.to(dev), c.v.to(dev), dev_pos(c, dev)
    ops = OD.ops()
    pk = packed(c, dev)
    work, scale = pk.work(1), 0.125
    with pytest.raises(RuntimeError, match="outside the cache"):
        far = [x + (PR.B if j % 3 == 0 else 0) for j, x in enumerate(pk.seq_host)]
        ops.cache_attn_packed(q, k, v, pos, pk.seq, far, work, c.H, scale)
    with pytest.raises(RuntimeError, match="int32"):
        ops.cache_attn_packed(q, k, v, pos, pk.seq.long(), pk.seq_host, work, c.H, scale)
    with pytest.raises(RuntimeError):
        ops.cache_attn_packed(q, k, v, pos, pk.seq.cpu(), pk.seq_host, work, c.H, scale)
    with pytest.raises(RuntimeError, match="rows"):
        ops.cache_attn_packed(q[:-1], k, v, pos, pk.seq, pk.seq_host, work, c.H, scale)
    with pytest.raises(RuntimeError, match="twice"):
        twice = list(pk.seq_host)
        twice[3] = twice[0]
        ops.cache_attn_packed(q, k, v, pos, pk.seq, twice, work, c.H, scale)


# ------------------------------------------------------------------ the session
def rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12))


def _bf16_model(gpu_device, **kw):
    torch.manual_seed(0)
    cfg = dict(vocab_size=1000, context_length=256, d_model=256, num_layers=2, num_heads=2, num_kv_heads=2, d_ff=512)
    cfg.update(kw)
    return TransformerLM(**cfg).to(gpu_device, torch.bfloat16).eval()


WATCHED = ("kv_append_packed", "kv_append_packed_fp8", "cache_attn_packed", "cache_attn_packed_fp8", "cache_attn",
           "cache_attn_fp8", "fa_fwd")


class _Spy:
    """The HIP op namespace with the prefill ops' lookups counted."""

    def __init__(self, h):
        self._h, self.seen = h, []

    def __getattr__(self, name):
        if name in WATCHED:
            self.seen.append(name)
        return getattr(self._h, name)


def _watch(monkeypatch, sess) -> _Spy:
    spy = _Spy(sess._hip())
    monkeypatch.setattr(sess, "_hip", lambda: spy)
    return spy


@pytest.mark.parametrize("fmt", ("bf16", "kv_fp8", "w_fp8", "paged"))
def test_prefill_slots_beside_graph_decode(gpu_device, monkeypatch, fmt):
    """Slots 2 and 0 are refilled by one ``prefill_slots`` call (70 and 9 tokens) while slot 1 goes on through the
    captured graph: one pass over the layers, slot 1's logits are those of an undisturbed twin bit for bit, and the
    new rows' logits are the model's (bf16 slab and paged: the full forward; fp8 formats: ``prefill_slot`` of a
    session of the same format, which is what those sessions are tested against)."""
    dev = gpu_device
    kw = {"bf16": {}, "kv_fp8": dict(kv_dtype="fp8"), "w_fp8": dict(weight_dtype="fp8"),
          "paged": dict(kv_layout="paged")}[fmt]
    model = _bf16_model(dev)
    nl = len(model.layers)
    g = torch.Generator().manual_seed(3)
    lens = [9, 17, 13]
    ids = torch.randint(0, 1000, (3, 17), generator=g).to(dev)
    pa, pb = torch.randint(0, 1000, (70,), generator=g).to(dev), torch.randint(0, 1000, (9,), generator=g).to(dev)
    steps = torch.randint(0, 1000, (5, 3), generator=g).to(dev)
    a, twin, single = (DecodeSession(model, 3, max_len=96, ragged=True, **kw) for _ in range(3))
    assert a.fast
    with torch.no_grad():
        for s in (a, twin):
            s.prefill(ids, lens)
            for i in range(2):
                s.decode(steps[i])  # (the graph is captured here)
        assert a._graph is not None
        a.reset_slot(2)
        a.reset_slot(0)
        spy = _watch(monkeypatch, a)
        lg = a.prefill_slots([2, 0], [pa, pb])
        f8 = "_fp8" if fmt == "kv_fp8" else ""
        assert spy.seen == ["kv_append_packed" + f8, "cache_attn_packed" + f8] * nl, spy.seen
        monkeypatch.undo()
        assert lg.shape == (2, 1000) and torch.isfinite(lg).all()
        assert a.cache.lengths == [9, 19, 70] and a.cache.pos.tolist() == [9, 19, 70]
        if fmt in ("bf16", "paged"):
            want = torch.stack([model(pa[None])[0, -1], model(pb[None])[0, -1]])
        else:
            want = torch.cat([single.prefill_slot(2, pa), single.prefill_slot(0, pb)])
        for i in range(2):
            assert rel(lg[i], want[i]) < 3e-2, (i, rel(lg[i], want[i]))
        for i in range(2, 5):
            la, lt = a.decode(steps[i]), twin.decode(steps[i])
            assert torch.equal(la[1], lt[1]), i
        # a second turn onto the slots that now hold tokens: every sequence attends the cache as stored
        more = a.prefill_slots([0, 2], [pa[:20], pb])
        assert a.cache.lengths == [32, 22, 82] and torch.isfinite(more).all()
        if fmt in ("bf16", "paged"):
            seq0 = torch.cat([pb, steps[2:5, 0], pa[:20]])
            assert rel(more[0], model(seq0[None])[0, -1]) < 3e-2
    torch.cuda.synchronize()


def test_prefill_chunk_splits_at_sequence_boundaries(gpu_device, monkeypatch):
    dev = gpu_device
    model = _bf16_model(dev)
    nl = len(model.layers)
    g = torch.Generator().manual_seed(5)
    ps = [torch.randint(0, 1000, (n,), generator=g).to(dev) for n in (20, 11, 45, 9)]
    sess = DecodeSession(model, 4, max_len=64, ragged=True, prefill_chunk=32)
    spy = _watch(monkeypatch, sess)
    with torch.no_grad():
        lg = sess.prefill_slots([3, 1, 0, 2], ps)
        # [20, 11] packed; 45 > 32 alone through prefill_slot (flash chunk of 32, then cache_attn of 13); [9] packed
        assert spy.seen == (["kv_append_packed", "cache_attn_packed"] * nl + ["fa_fwd"] * nl + ["cache_attn"] * nl
                            + ["kv_append_packed", "cache_attn_packed"] * nl), spy.seen
        assert sess.cache.lengths == [45, 11, 9, 20]
        for i, p in enumerate(ps):
            assert rel(lg[i], model(p[None])[0, -1]) < 3e-2, i
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the engine
V = 1000
LENS = [(250, 12), (17, 9), (40, 14), (5, 6), (300, 5), (33, 11), (9, 13), (120, 7), (64, 10), (21, 8), (7, 12)]
CHOSEN = 0
BATCH, PAGES, SYNC, BUDGET = 9, 10, 4, 512


@functools.lru_cache(maxsize=None)
def engine_model(dev):
    torch.manual_seed(0)
    cfg = dict(vocab_size=V, context_length=1024, d_model=256, num_layers=2, num_heads=4, d_ff=512)
    return TransformerLM(**cfg).to(dev, torch.bfloat16).eval()


def prompt(n, seed):
    return torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(seed))


def tenant_params(i: int, n: int) -> SamplingParams:
    sets = [
        dict(temperature=0.0),
        dict(temperature=0.7, top_k=20, seed=3),
        dict(temperature=1.2, top_p=0.8, seed=5, repetition_penalty=1.3),
        dict(temperature=1.0, min_p=0.1, seed=7, presence_penalty=0.4),
        dict(temperature=0.5, top_k=100, top_p=0.9, min_p=0.01, seed=9, frequency_penalty=0.3),
        dict(temperature=2.0, seed=11, logprobs=True),
    ]
    return SamplingParams(max_new_tokens=n, **sets[i % len(sets)])


def groups_of(lens, budget):
    out = []
    for n in lens:
        if out and sum(out[-1]) + n <= budget:
            out[-1].append(n)
        else:
            out.append([n])
    return out


def expected_groups(lens, batch, pages, sync, budget) -> int:
    """The packed passes the engine spends on ``lens`` = (prompt, new tokens) submitted up front: a host model of its
    windows (FCFS into free slots under the page budget, a window draws up to ``sync`` tokens, finished requests
    leave at its end), with each window's admissions cut into groups of at most ``budget`` prompt tokens."""
    need = lambda i: -(-(lens[i][0] + lens[i][1]) // 256)  # noqa: E731
    waiting, running, groups = list(range(len(lens))), {}, 0
    while waiting or running:
        picked = []
        while waiting and len(running) < batch and sum(need(i) for i in running) + need(waiting[0]) <= pages:
            running[waiting[0]] = 1
            picked.append(waiting.pop(0))
        groups += len(groups_of([lens[i][0] for i in picked], budget))
        n = min(sync, max(lens[i][1] - c for i, c in running.items()))
        running = {i: c + n for i, c in running.items() if c + n < lens[i][1]}
    return groups


@functools.lru_cache(maxsize=None)
def teacher(dev):
    return copy.deepcopy(engine_model(dev)).float()  # the same bf16 weights, fp32 arithmetic


def check_against_teacher(dev, p, out, what):
    """Every emitted token within ``3e-2 * max|logits|`` of its position's reference maximum, every log-prob within
    the same margin of the reference's."""
    toks = out.tokens.to(dev)
    seq = torch.cat([p.to(dev), toks])[None]
    with torch.no_grad():
        lg = teacher(dev)(seq)[0, p.numel() - 1 : -1].float()  # row j: the distribution token j was drawn from
    margin = 3e-2 * lg.abs().amax(-1)
    picked = lg.gather(1, toks[:, None])[:, 0]
    gap = lg.amax(-1) - picked
    lp = torch.log_softmax(lg, -1).gather(1, toks[:, None])[:, 0]
    dlp = (out.logprobs.to(dev) - lp).abs()
    print(f"\n{what}: worst argmax gap / margin {float((gap / margin).max()):.3e}, "
          f"worst |logprob - ref| / margin {float((dlp / margin).max()):.3e}", end="")
    assert torch.isfinite(out.logprobs).all()
    assert bool((gap <= margin).all()), (what, gap.tolist(), margin.tolist())
    assert bool((dlp <= margin).all()), (what, dlp.tolist(), margin.tolist())


def run_engine(dev, monkeypatch, prefill_tokens):
    eng = ServingEngine(engine_model(dev), batch=BATCH, max_len=1024, kv_layout="paged", num_pages=PAGES,
                        sync_every=SYNC, penalties=True, logprobs=True, prefill_tokens=prefill_tokens)
    spy = _watch(monkeypatch, eng.session)
    rids = []
    for i, (n, new) in enumerate(LENS):
        sp = SamplingParams(temperature=0.0, max_new_tokens=new, logprobs=True) if i == CHOSEN else tenant_params(i, new)
        rids.append(eng.submit(prompt(n, 1 if i == CHOSEN else 100 + i), sp))
    outs = {o.rid: o for o in eng.step()}
    waited = eng.num_waiting
    outs.update(eng.run())
    monkeypatch.undo()
    return eng, [outs[r] for r in rids], spy, waited


def test_engine_packed_admission(gpu_device, monkeypatch):
    dev = gpu_device
    nl = len(engine_model(dev).layers)
    p = prompt(LENS[CHOSEN][0], 1)
    eng0, outs0, spy0, _ = run_engine(dev, monkeypatch, None)
    assert spy0.seen.count("kv_append_packed") == 0
    check_against_teacher(dev, p, outs0[CHOSEN], "prefill_tokens=None")
    eng, outs, spy, waited = run_engine(dev, monkeypatch, BUDGET)
    for i, o in enumerate(outs):
        assert len(o.tokens) == LENS[i][1] and o.finish_reason == "length", i
    assert eng.pages_in_use == 0 and eng.captures == 1 and waited > 0
    passes = spy.seen.count("kv_append_packed") // nl
    want = expected_groups(LENS, BATCH, PAGES, SYNC, BUDGET)
    assert spy.seen.count("cache_attn_packed") == passes * nl and spy.seen.count("kv_append_packed") == passes * nl
    assert spy.seen.count("fa_fwd") == 0 and spy.seen.count("cache_attn") == 0  # no per-request prefill pass
    assert passes == want and passes < len(LENS), (passes, want)
    check_against_teacher(dev, p, outs[CHOSEN], f"prefill_tokens={BUDGET}")
