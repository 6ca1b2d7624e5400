"""The ``*_rows_reference`` functions of ``ops/sampling.py`` on the CPU: against the fp64 oracle of
``tests/sample_rows_refs.py`` (min-p and the per-row rules), and against the existing scalar ``*_reference`` on each
row alone, exactly.  The min-p cases keep every mass a relative ``MARGIN = 1e-3`` away from the threshold
(``sample_rows_refs``); the margin is asserted here."""

from __future__ import annotations

import functools

import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import sample_refs as SR
from . import sample_rows_refs as RR

DTYPES = (torch.bfloat16, torch.float32)
SEEDS = (11, 2**40 + 5, 3, 2**63 + 9, 0)
COUNTS = (0, 3, 2**33 + 1, 7, 1)


@functools.lru_cache(maxsize=None)
def case(V, dtype):
    x, params = RR.rows_case(V, dtype)
    return x, params, [RR.oracle_of(SR.f64(x)[b], params[b]) for b in range(5)]


def table(params, limit=1000, eos=None):
    t = S.SamplingTable(len(params))
    for b, p in enumerate(params):
        t.set(b, S.SamplingParams(seed=SEEDS[b], max_new_tokens=limit, eos_token_id=eos, **p))
    return t


def buffers(B=5, N=8):
    return torch.full((B, 1), -7, dtype=torch.long), torch.full((B, N), -1, dtype=torch.long)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", RR.VS)
def test_min_p_margin_and_oracle(V, dtype):
    x, params, oracles = case(V, dtype)
    assert oracles[4].margin >= RR.MARGIN, (V, oracles[4].margin)
    u = SR.uniforms(V, 5)
    t = table(params)
    ids, out = buffers()
    S.sample_rows_reference(x, t, ids, out, None, u)
    for b in range(5):
        assert int(ids[b]) in oracles[b].acceptable(float(u[b])), (b, int(ids[b]))
        assert int(out[b, 0]) == int(ids[b]) and int(t.count[b]) == 1
    if V >= 257:  # the filter does something: it drops tokens that top-k and top-p kept
        o = oracles[4]
        assert o.kept.sum() < SR.Oracle(SR.f64(x)[4], 1.3, int(params[4]["top_k"]), params[4]["top_p"]).kept.sum()


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", RR.VS)
def test_rows_equal_scalar_reference(V, dtype):
    x, params, _ = case(V, dtype)
    u = SR.uniforms(V + 1, 5)
    t = table(params)
    ids, out = buffers()
    S.sample_rows_reference(x, t, ids, out, None, u)
    for b in range(4):  # (the scalar function has no min_p)
        p = params[b]
        ref = S.sample_logits_reference(x[b : b + 1], p["temperature"], int(p.get("top_k") or 0),
                                        p.get("top_p", 1.0), u[b : b + 1])
        assert int(ids[b]) == int(ref), b
    # Philox: a one-row sample_step at rng = (seed[b], count[b])
    t = table(params)
    t.count.copy_(torch.tensor(COUNTS))
    ids, out = buffers()
    S.sample_rows_reference(x, t, ids, out)
    for b in range(4):
        p = params[b]
        seed = SEEDS[b] - 2**64 if SEEDS[b] >= 2**63 else SEEDS[b]
        i1, o1 = buffers(1, 1)
        S.sample_step_reference(x[b : b + 1], p["temperature"], int(p.get("top_k") or 0), p.get("top_p", 1.0),
                                torch.tensor([seed, COUNTS[b]]), i1, o1, None, torch.zeros(1, dtype=torch.int32), -1)
        assert int(ids[b]) == int(i1), b
        assert int(t.count[b]) == COUNTS[b] + 1


def test_rules_follow_oracle():
    x, params, _ = case(257, torch.float32)
    greedy = int(SR.Oracle(SR.f64(x)[0], 0.0).order[0])
    t = table(params, limit=2)
    t.eos[0:1].fill_(greedy)  # slot 0 ends on its first token, the others at 2 tokens
    t.done[3:4].fill_(1)  # idle
    t.step[4:5].zero_()  # idle
    ids, out = buffers()
    state = [(0, 2, greedy if b == 0 else -1, int(t.done[b]), int(t.step[b])) for b in range(5)]
    for _ in range(3):
        before = (ids.clone(), out.clone(), t.count.clone())
        S.sample_rows_reference(x, t, ids, out)
        for b in range(5):
            count, limit, eos, done, step = state[b]
            wrote, count, done, step = RR.step_rules(int(ids[b]), count, limit, eos, done, step)
            state[b] = (count, limit, eos, done, step)
            assert (int(t.count[b]), int(t.done[b]), int(t.step[b])) == (count, done, step), b
            if not wrote:
                assert torch.equal(ids[b], before[0][b]) and torch.equal(out[b], before[1][b])
    assert t.count.tolist() == [1, 2, 2, 0, 0] and t.done.tolist() == [1, 1, 1, 1, 0]
    assert t.step.tolist() == [0, 0, 0, 1, 0]  # (slot 3 idles on `done` alone: its step is not touched)


def test_rows_map_reference():
    x, params, _ = case(257, torch.float32)
    t = table(params)
    ids, out = buffers()
    S.sample_rows_reference(x[3:4], t, ids, out, torch.tensor([3], dtype=torch.int32))
    assert t.count.tolist() == [0, 0, 0, 1, 0] and (ids.view(-1)[[0, 1, 2, 4]] == -7).all() and int(ids[3]) >= 0


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_process_and_commit_rows_equal_scalar_reference(dtype):
    V, B = 257, 4
    x = SR.random_rows(5, B, V, dtype)
    g = torch.Generator().manual_seed(1)
    hist = torch.randint(0, 5, (B, V), generator=g, dtype=torch.int32) * (torch.rand(B, V, generator=g) < 0.2)
    hist = hist.to(torch.int32)
    bias = torch.zeros(V)
    bias[3], bias[100] = 1.5, -torch.inf
    pen = [(1.3, 0.0, 0.0), (1.0, 0.0, 0.0), (0.8, 0.5, 0.25), (1.0, 0.7, 0.0)]
    t = S.SamplingTable(B)
    for b, (rp, pp, fp) in enumerate(pen):
        t.set(b, S.SamplingParams(temperature=0.0, repetition_penalty=rp, presence_penalty=pp, frequency_penalty=fp))
    for bs in (None, bias):
        out, lse = torch.zeros_like(x), torch.zeros(B)
        S.logit_process_rows_reference(x, t, hist, bs, out, lse)
        for b, (rp, pp, fp) in enumerate(pen):
            o1, l1 = torch.zeros_like(x[b : b + 1]), torch.zeros(1)
            S.logit_process_reference(x[b : b + 1], hist[b : b + 1], bs, rp, pp, fp, o1, l1)
            if b != 1:
                assert torch.equal(out[b].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   o1[0].view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), b
            assert torch.equal(lse[b], l1[0])
        if bs is None:  # neutral penalties: every bit stays
            assert torch.equal(out[1].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               x[1].view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    # commit: draw, then commit; against token_commit_reference on each row with rng = (., count - 1)
    ids, toks = buffers(B, 4)
    S.sample_rows_reference(x, t, ids, toks)
    t.done[2:3].fill_(1)  # finished by its draw: still commits it
    h2, lp = hist.clone(), torch.full((B, 4), float("nan"))
    S.token_commit_rows_reference(toks, t, h2, x, lse, lp)
    for b in range(B):
        h1, lp1 = hist[b : b + 1].clone(), torch.full((1, 4), float("nan"))
        S.token_commit_reference(toks[b : b + 1], torch.tensor([0, 0]), h1, x[b : b + 1], lse[b : b + 1], lp1)
        assert torch.equal(h2[b], h1[0]) and torch.equal(lp[b, :1], lp1[0, :1])
    again = (h2.clone(), lp.clone())
    S.token_commit_rows_reference(toks, t, h2, x, lse, lp)  # nothing drawn since: nothing committed
    assert torch.equal(h2, again[0]) and torch.equal(lp.nan_to_num(), again[1].nan_to_num())


MODES = ((0.0, 0, 1.0), (0.8, 50, 1.0), (0.8, 0, 0.95), (0.8, 50, 0.95))  # greedy, top-k, top-p, both


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_philox_row_is_sample_step_row(dtype):
    """One seed in every slot and ``philox_row[b] = b``: ``sample_step``'s stream at ``rng = (seed, count)``, token
    for token (how ``generate`` runs on the table); a slot left at the default 0 is a one-row ``sample_step``."""
    V, B, seed = 1025, 4, 2**40 + 5
    x = SR.random_rows(V + 2, B, V, dtype)
    for T, k, p in MODES:
        for count in (0, 1, 2**32 + 5):
            t = S.SamplingTable(B)
            for b in range(B):
                t.set(b, S.SamplingParams(temperature=T, top_k=k, top_p=p, seed=seed, max_new_tokens=2**31 - 1,
                                          **({"philox_row": b} if b < 3 else {})))
            assert t.philox_row.tolist() == [0, 1, 2, 0]
            t.count.fill_(count)
            ids, out = buffers(B)
            S.sample_rows_reference(x, t, ids, out)
            rng = torch.tensor([seed, count])
            i1, o1 = buffers(B, 1)
            S.sample_step_reference(x, T, k, p, rng, i1, o1, None, torch.zeros(B, dtype=torch.int32), -1)
            i2, o2 = buffers(1, 1)
            S.sample_step_reference(x[3:4], T, k, p, rng, i2, o2, None, torch.zeros(1, dtype=torch.int32), -1)
            assert ids.view(-1).tolist() == i1.view(-1).tolist()[:3] + [int(i2)], (T, k, p, count)
            fin = int(count + 1 >= 2**31 - 1)  # (the limit is the table's largest: only a count past it ends a slot)
            assert t.count.tolist() == [count + 1] * B and t.done.tolist() == [fin] * B and t.step.tolist() == [1 - fin] * B
    # the row word is read: rows 1 and 2 draw other uniforms than row 0
    assert len({float(u) for u in S.philox_uniform(seed, 1, 3)}) == 3
