"""Packed multi-request prefill on the CPU: the packed reference ops against the per-slot references, the GPU tests'
inputs against their float64 bound through the kernel's rounding emulation, ``DecodeSession.prefill_slots`` and the
engine's ``prefill_tokens`` admission off the fast path (where ``prefill_slots`` is a loop over ``prefill_slot``, so
the two engine settings are the same function and only the admission logic differs)."""

from __future__ import annotations

import functools

import pytest
import torch

from bpe_transformer.models import DecodeSession, ServingEngine, SamplingParams, TransformerLM
from bpe_transformer.ops import decode as OD

from . import cache_prefill_refs as CR
from . import packed_prefill_refs as PR

BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float8_e4m3fn: torch.uint8}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(BITS[t.dtype])  # NaN-proof equality


def packed(c: PR.Case) -> OD.PackedPrompts:
    return OD.PackedPrompts(c.slots, c.lens, pos_host=c.pos)


# ------------------------------------------------------------------ the packed references are the per-slot ones
@pytest.mark.parametrize("which", ("base", "full"))
def test_append_reference_is_the_per_slot_reference(which):
    c = PR.base_case(64, 2) if which == "base" else PR.full_case()
    cos, sin = PR.rope_tables(c.D)
    pos = torch.tensor(c.pos_all, dtype=torch.int32)
    k1, v1, k2, v2 = c.k.clone(), c.v.clone(), c.k.clone(), c.v.clone()
    q1 = OD.kv_append_packed(c.qkv, k1, v1, cos, sin, pos, packed(c), c.H)
    for i, s, o, n, p in c.seqs():
        one = OD.kv_append_reference(c.qkv[o:o + n], k2[s:s + 1], v2[s:s + 1], cos, sin, pos[s:s + 1], 1, n, c.H)
        assert torch.equal(bits(q1[o:o + n]), bits(one)), i
    assert torch.equal(bits(k1), bits(k2)) and torch.equal(bits(v1), bits(v2))
    assert torch.equal(bits(k1[PR.IDLE]), bits(c.k[PR.IDLE])) and pos.tolist() == c.pos_all
    assert not torch.equal(bits(k1), bits(c.k))  # (something was written)


def test_attention_reference_is_the_per_slot_reference():
    c = PR.base_case(64, 2)
    pos = torch.tensor(c.pos_all, dtype=torch.int32)
    out = OD.prefill_attention_packed(c.q, c.k, c.v, pos, packed(c), c.H)
    for i, s, o, n, p in c.seqs():
        one = OD.decode_attention_reference(c.q[o:o + n], c.k[s:s + 1], c.v[s:s + 1], pos[s:s + 1], c.H, None, n)
        assert torch.equal(bits(out[o:o + n]), bits(one)), i
    assert torch.isfinite(out).all()


def test_fp8_and_paged_references_are_the_per_slot_references():
    c = PR.base_case(64, 2)
    cos, sin = PR.rope_tables(c.D)
    pos = torch.tensor(c.pos_all, dtype=torch.int32)
    k8, ks = OD.kv_quantize_reference(c.k)
    v8, vs = OD.kv_quantize_reference(c.v)
    a = [t.clone() for t in (k8, v8, ks, vs)]
    b = [t.clone() for t in (k8, v8, ks, vs)]
    q1 = OD.kv_append_packed_fp8(c.qkv, *a, cos, sin, pos, packed(c), c.H)
    for i, s, o, n, p in c.seqs():
        one = OD.kv_append_fp8_reference(c.qkv[o:o + n], *[t[s:s + 1] for t in b], cos, sin, pos[s:s + 1], 1, n, c.H)
        assert torch.equal(bits(q1[o:o + n]), bits(one)), i
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    out = OD.prefill_attention_packed_fp8(c.q, *a, pos, packed(c), c.H)
    for i, s, o, n, p in c.seqs():
        one = OD.decode_attention_fp8_reference(c.q[o:o + n], *[t[s:s + 1] for t in a], pos[s:s + 1], c.H, None, n)
        assert torch.equal(bits(out[o:o + n]), bits(one)), i
    # paged: the packed op through a block table is the slab packed op on the gathered slab
    nb = -(-PR.LMAX // OD.KV_PAGE)
    table = PR.page_table(nb)
    pool = lambda t: OD.paged_scatter(t, torch.zeros(PR.B * nb, PR.HKV, OD.KV_PAGE, c.D, dtype=t.dtype), table)  # noqa: E731
    kp, vp = pool(c.k), pool(c.v)
    got = OD.prefill_attention_packed(c.q, kp, vp, pos, packed(c), c.H, block_table=table, max_len=PR.LMAX)
    want = OD.prefill_attention_packed(c.q, c.k, c.v, pos, packed(c), c.H)
    assert torch.equal(bits(got), bits(want))
    k1, v1 = c.k.clone(), c.v.clone()
    qs = OD.kv_append_packed(c.qkv, k1, v1, cos, sin, pos, packed(c), c.H)
    qp = OD.kv_append_packed(c.qkv, kp, vp, cos, sin, pos, packed(c), c.H, block_table=table, max_len=PR.LMAX)
    assert torch.equal(bits(qs), bits(qp))
    assert torch.equal(bits(OD.paged_gather(kp, table, PR.LMAX)), bits(k1))
    assert torch.equal(bits(OD.paged_gather(vp, table, PR.LMAX)), bits(v1))


def test_work_list_covers_every_block_once_heaviest_first():
    for G in PR.GROUPS:
        pk = OD.PackedPrompts(PR.SLOTS, PR.LENS, pos_host=PR.POS)
        items = pk.work_items(G)
        want = {(i, qb) for i, n in enumerate(PR.LENS) for qb in range((G * n + 127) // 128)}
        assert len(items) == len(want) and set(items) == want
        keys = [PR.POS[i] + min((128 * qb + 127) // G, PR.LENS[i] - 1) + 1 for i, qb in items]
        assert keys == sorted(keys, reverse=True)
    assert pk.seq.tolist() == [[3, 0, 33], [0, 33, 1], [4, 34, 129], [1, 163, 9]] and pk.N == 172


# ------------------------------------------------------------------ the GPU tests' inputs and bound are satisfiable
@pytest.mark.parametrize("D", PR.DIMS)
@pytest.mark.parametrize("G", PR.GROUPS)
def test_emulation_meets_the_gpu_bound(D, G):
    c = PR.base_case(D, G)
    for (i, s, o, n, p), (ref, A) in zip(c.seqs(), PR.reference(D, G)):
        out = CR.emulate(c.q[o:o + n], c.k[s:s + 1], c.v[s:s + 1], p, c.H, n)
        assert torch.isfinite(out).all() and CR.global_rel(out, ref) < CR.TOL_GLOBAL, (i, CR.global_rel(out, ref))


def test_emulation_meets_the_gpu_bound_at_lmax():
    c = PR.full_case()
    for (i, s, o, n, p), (ref, A) in zip(c.seqs(), PR.reference(c.D, c.G, "full")):
        w = PR.written(c, i)
        assert w == (3 if i == PR.FULL_SEQ else n)
        out = CR.emulate(c.q[o:o + w], c.k[s:s + 1], c.v[s:s + 1], p, c.H, w)
        assert torch.isfinite(out).all() and CR.global_rel(out, ref) < CR.TOL_GLOBAL, i


@pytest.mark.parametrize("D,T,p0", CR.DOMINANT)
@pytest.mark.parametrize("shift", (0, 1))
def test_emulation_meets_the_dominant_bounds(D, T, p0, shift):
    c, ref, A, rows = PR.dominant_case(D, T, p0, shift)
    s = c.slots[0]
    out = CR.emulate(c.q[:T], c.k[s:s + 1], c.v[s:s + 1], p0, c.H, T)
    if shift:
        assert torch.isfinite(out).all() and CR.global_rel(out, ref) < CR.TOL_GLOBAL
        return
    bound = CR.dominant_bound(rows, ref, A, CR.dominant_extra(c.q[:T], c.k[s:s + 1], c.v[s:s + 1], p0, T))
    assert not (~((PR.f64(out) - rows).abs() <= bound)).any()


# ------------------------------------------------------------------ the session off the fast path
V = 64


@functools.lru_cache(maxsize=None)
def model():
    torch.manual_seed(0)
    return TransformerLM(vocab_size=V, context_length=1024, d_model=32, num_layers=2, num_heads=2, d_ff=64).eval()


def prompt(n, seed=0):
    return torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("layout", ("slab", "paged"))
def test_prefill_slots_is_a_loop_over_prefill_slot(layout):
    kw = dict(max_len=300, ragged=True, kv_layout=layout)
    a, b = DecodeSession(model(), 3, **kw), DecodeSession(model(), 3, **kw)
    assert not a.fast
    pa, pb = prompt(70, 1), prompt(9, 2)
    got = a.prefill_slots([2, 0], [pa, pb])
    want = torch.cat([b.prefill_slot(2, pa), b.prefill_slot(0, pb)])
    assert got.shape == (2, V) and torch.equal(got, want)
    assert a.cache.lengths == [9, 0, 70] and a.cache.pos.tolist() == [9, 0, 70]
    full = model()(pa[None])[0, -1]
    torch.testing.assert_close(got[0], full, rtol=1e-4, atol=1e-4)


def test_prefill_slots_rejects_duplicate_rows():
    s = DecodeSession(model(), 3, max_len=64, ragged=True)
    with pytest.raises(AssertionError, match="distinct"):
        s.prefill_slots([1, 1], [prompt(4), prompt(5)])
    with pytest.raises(AssertionError, match="ragged"):
        DecodeSession(model(), 3, max_len=64).prefill_slots([0], [prompt(4)])
    assert s.cache.lengths == [0, 0, 0]


def test_prefill_slots_raises_before_anything_is_written_when_the_pool_runs_out():
    s = DecodeSession(model(), 3, max_len=600, ragged=True, kv_layout="paged", num_pages=2)
    with pytest.raises(RuntimeError, match="out of pages"):
        s.prefill_slots([0, 1], [prompt(300, 1), prompt(5, 2)])  # 2 + 1 pages
    assert s.cache.lengths == [0, 0, 0] and s.cache.pages_in_use == 0


# ------------------------------------------------------------------ the engine's admission logic
LENS = [(250, 12), (17, 9), (40, 14), (5, 6), (300, 5), (33, 11), (9, 13), (120, 7), (64, 10), (21, 8), (7, 12)]
BATCH, PAGES, SYNC, BUDGET = 9, 10, 4, 64


def params(i: int, n: int) -> SamplingParams:
    sets = [
        dict(temperature=0.0),
        dict(temperature=0.7, top_k=20, seed=3),
        dict(temperature=1.2, top_p=0.8, seed=5, repetition_penalty=1.3),  # (the first to need the penalty table)
        dict(temperature=1.0, min_p=0.1, seed=7, presence_penalty=0.4),
        dict(temperature=0.5, top_k=100, top_p=0.9, min_p=0.01, seed=9, frequency_penalty=0.3),
        dict(temperature=2.0, seed=11, logprobs=True),  # (the first to ask for log-probs)
    ]
    return SamplingParams(max_new_tokens=n, **sets[i % len(sets)])


def groups_of(lens: list[int], budget: int) -> list[list[int]]:
    """The specification, written apart from the code under test: arrival order, a group's prompt tokens sum to at most
    the budget, a longer prompt alone."""
    out: list[list[int]] = []
    for n in lens:
        if out and sum(out[-1]) + n <= budget:
            out[-1].append(n)
        else:
            out.append([n])
    return out


def expected_calls(lens, batch: int, pages: int, sync: int, budget: int) -> list[list[int]]:
    """The ``prefill_slots`` calls of the engine on ``lens`` = (prompt, new tokens) submitted up front: a host model
    of its windows (FCFS into free slots under the page budget, nobody overtakes; a window draws up to ``sync``
    tokens; finished requests leave at its end)."""
    need = lambda i: -(-(lens[i][0] + lens[i][1]) // 256)  # noqa: E731
    waiting, running, calls = list(range(len(lens))), {}, []
    while waiting or running:
        picked = []
        while waiting and len(running) < batch and sum(need(i) for i in running) + need(waiting[0]) <= pages:
            running[waiting[0]] = 1  # its first token comes with the prefill
            picked.append(waiting.pop(0))
        calls += groups_of([lens[i][0] for i in picked], budget)
        n = min(sync, max(lens[i][1] - c for i, c in running.items()))
        running = {i: c + n for i, c in running.items() if c + n < lens[i][1]}
    return calls


def run_engine(prefill_tokens):
    eng = ServingEngine(model(), batch=BATCH, max_len=1024, kv_layout="paged", num_pages=PAGES, sync_every=SYNC,
                        prefill_tokens=prefill_tokens)
    calls, inner = [], eng.session.prefill_slots
    slots = []

    def spy(rows, prompts):
        calls.append([int(p.numel()) for p in prompts])
        slots.append(list(rows))
        return inner(rows, prompts)

    eng.session.prefill_slots = spy
    rids = [eng.submit(prompt(n, 100 + i), params(i, new)) for i, (n, new) in enumerate(LENS)]
    first = {o.rid: o for o in eng.step()}
    waited = eng.num_waiting
    first.update(eng.run())
    assert eng.pages_in_use == 0 and eng.num_running == 0
    return [first[r] for r in rids], calls, slots, waited


def test_engine_packed_admission_equals_unpacked_admission():
    base, calls0, _, waited0 = run_engine(None)
    got, calls, slots, waited = run_engine(BUDGET)
    assert calls0 == [] and waited0 == waited > 0  # the pool holds back request 8 and those behind it
    for i, (a, b) in enumerate(zip(base, got)):
        assert len(a.tokens) == LENS[i][1] and torch.equal(a.tokens, b.tokens), i
        assert (a.logprobs is None) == (b.logprobs is None)
        if a.logprobs is not None:
            assert torch.equal(a.logprobs, b.logprobs) and torch.isfinite(a.logprobs).all()
    want = expected_calls(LENS, BATCH, PAGES, SYNC, BUDGET)
    assert calls == want, (calls, want)
    assert any(len(c) > 1 for c in calls) and [250] in calls and [300] in calls  # groups, and prompts over the budget
    assert all(sum(c) <= BUDGET or len(c) == 1 for c in calls)
    assert [n for c in calls for n in c] == [n for n, _ in LENS]  # first come first served
    used = [s for c in slots for s in c]
    assert used[:8] == list(range(8)) and len(set(used[8:]) & set(used[:8])) > 0  # lowest free slot; slots reused
    # a structural switch inside a group: request 2 (penalties) is not the first of its group
    assert any(LENS[2][0] in c[1:] for c in calls)


def test_prefill_tokens_must_be_positive():
    for bad in (0, -5):
        with pytest.raises(ValueError, match="prefill_tokens"):
            ServingEngine(model(), batch=2, max_len=64, prefill_tokens=bad)
    assert ServingEngine(model(), batch=2, max_len=64, prefill_tokens=1).prefill_tokens == 1
