"""The per-row sampling kernels (``csrc/sample_rows.hip``, the ``*_rows`` kernels of ``csrc/logit_process.hip``) on
the GPU.  Five rows, one sampling mode each (``tests/sample_rows_refs.py``), V in {1, 7, 257, 1000, 50257} -- below
one 16-byte vector, across a tile edge, and an odd V whose rows start unaligned -- in bf16 and fp32.

Every claim is exact: a row's token equals the scalar kernel's on that row alone (given uniforms: ``sample_logits``;
Philox: a one-row ``sample_step`` at ``rng = (seed[b], count[b])``); the processed rows and the commits equal the scalar
kernels' bit for bit.  Only the min-p row, which the scalar kernel cannot compute, is checked against the fp64
oracle, with every mass a relative 1e-3 away from the threshold (asserted)."""

from __future__ import annotations

import functools

import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import sample_refs as SR
from . import sample_rows_refs as RR

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
SEEDS = (11, 2**40 + 5, 3, 2**63 + 9, 0)
COUNTS = (0, 3, 2**33 + 1, 7, 1)
N_OUT = 8


@functools.lru_cache(maxsize=None)
def case(V, dtype):
    x, params = RR.rows_case(V, dtype)
    return x, params, [RR.oracle_of(SR.f64(x)[b], params[b]) for b in range(5)]


def table(dev, params, limit=1000, eos=None):
    t = S.SamplingTable(len(params), dev)
    for b, p in enumerate(params):
        t.set(b, S.SamplingParams(seed=SEEDS[b], max_new_tokens=limit, eos_token_id=eos, **p))
    return t


def buffers(dev, B=5, N=N_OUT):
    return (torch.full((B, 1), -7, dtype=torch.long, device=dev), torch.full((B, N), -1, dtype=torch.long, device=dev))


def scalar_args(p):
    return p["temperature"], int(p.get("top_k") or 0), p.get("top_p", 1.0)


def bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", RR.VS)
def test_given_uniforms_equal_scalar_kernel(gpu_device, V, dtype):
    x, params, oracles = case(V, dtype)
    xg = x.to(gpu_device)
    u = SR.uniforms(V, 5)
    t = table(gpu_device, params)
    ids, out = buffers(gpu_device)
    S.sample_rows(xg, t, ids, out, u=u)
    got = ids.view(-1).tolist()
    for b in range(4):
        ref = S.sample_logits(xg[b : b + 1], *scalar_args(params[b]), u[b : b + 1])
        assert got[b] == int(ref), (b, got[b], int(ref))
    assert oracles[4].margin >= RR.MARGIN
    assert got[4] in oracles[4].acceptable(float(u[4])), got[4]
    assert out[:, 0].tolist() == got and t.count.tolist() == [1] * 5 and t.done.tolist() == [0] * 5


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", RR.VS)
def test_philox_equals_one_row_sample_step(gpu_device, V, dtype):
    x, params, oracles = case(V, dtype)
    xg = x.to(gpu_device)
    t = table(gpu_device, params)
    t.count.copy_(torch.tensor(COUNTS))
    ids, out = buffers(gpu_device)
    S.sample_rows(xg, t, ids, out)
    got = ids.view(-1).tolist()
    for b in range(4):
        seed = SEEDS[b] - 2**64 if SEEDS[b] >= 2**63 else SEEDS[b]
        i1, o1 = buffers(gpu_device, 1, 1)
        S.sample_step(xg[b : b + 1], *scalar_args(params[b]), torch.tensor([seed, COUNTS[b]], device=gpu_device), i1,
                      o1, None, torch.zeros(1, dtype=torch.int32, device=gpu_device), -1)
        assert got[b] == int(i1), (b, got[b], int(i1))
    u4 = float(S.philox_uniform(SEEDS[4], COUNTS[4], 1)[0])
    assert got[4] in oracles[4].acceptable(u4), got[4]
    assert t.count.tolist() == [c + 1 for c in COUNTS]
    small = [b for b in range(5) if COUNTS[b] < N_OUT]  # a count past the last column writes no column
    assert [int(out[b, COUNTS[b]]) for b in small] == [got[b] for b in small]
    assert int((out >= 0).sum()) == len(small)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", (7, 50257))
def test_idle_limit_eos(gpu_device, V, dtype):
    x, params, oracles = case(V, dtype)
    xg = x.to(gpu_device)
    greedy = int(oracles[0].order[0])
    t = table(gpu_device, params, limit=2)
    t.eos[0:1].fill_(greedy)  # slot 0 ends on its first token, slots 1 and 2 at their limit of 2
    t.done[3:4].fill_(1)  # idle: done
    t.step[4:5].zero_()  # idle: step == 0
    ids, out = buffers(gpu_device)
    want = [([1, 1, 1, 0, 0], [1, 0, 0, 1, 0], [0, 1, 1, 1, 0]),
            ([1, 2, 2, 0, 0], [1, 1, 1, 1, 0], [0, 0, 0, 1, 0]),
            ([1, 2, 2, 0, 0], [1, 1, 1, 1, 0], [0, 0, 0, 1, 0])]
    for count, done, step in want:
        before = (ids.clone(), out.clone(), t.count.clone())
        idle = [b for b in range(5) if int(t.done[b]) != 0 or int(t.step[b]) == 0]
        S.sample_rows(xg, t, ids, out)
        assert (t.count.tolist(), t.done.tolist(), t.step.tolist()) == (count, done, step)
        for b in idle:  # bit-identical
            assert torch.equal(ids[b], before[0][b]) and torch.equal(out[b], before[1][b])
            assert torch.equal(t.count[b], before[2][b])
    assert int(ids[0]) == greedy and out[0].tolist() == [greedy] + [-1] * (N_OUT - 1)
    assert (out[1:3, :2] >= 0).all() and (out[1:3, 2:] == -1).all() and (out[3:] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_rows_map_selects_one_slot(gpu_device, dtype):
    V = 1000
    x, params, _ = case(V, dtype)
    xg = x.to(gpu_device)
    u = SR.uniforms(3, 5)
    t = table(gpu_device, params)
    ids, out = buffers(gpu_device)
    # one launched row: the logits of slot 3 alone
    S.sample_rows(xg[3:4], t, ids, out, rows=[3], u=u[3:4])
    ref = S.sample_logits(xg[3:4], *scalar_args(params[3]), u[3:4])
    assert t.count.tolist() == [0, 0, 0, 1, 0]
    assert ids.view(-1).tolist() == [-7, -7, -7, int(ref), -7]
    assert int(out[3, 0]) == int(ref) and int((out >= 0).sum()) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", (7, 257, 50257))
def test_process_and_commit_rows_equal_scalar_kernels(gpu_device, V, dtype):
    B, dev = 5, gpu_device
    x = SR.random_rows(V, B, V, dtype).to(dev)
    g = torch.Generator().manual_seed(V)
    hist = (torch.randint(0, 5, (B, V), generator=g) * (torch.rand(B, V, generator=g) < 0.3)).to(torch.int32).to(dev)
    bias = torch.zeros(V)
    bias[V // 2], bias[V - 1] = 1.5, -torch.inf
    bias = bias.to(dev)
    pen = [(1.3, 0.0, 0.0), (1.0, 0.0, 0.0), (0.8, 0.5, 0.25), (1.0, 0.7, 0.0), (1.7, -0.3, 0.1)]
    t = S.SamplingTable(B, dev)
    for b, (rp, pp, fp) in enumerate(pen):
        t.set(b, S.SamplingParams(temperature=0.0, repetition_penalty=rp, presence_penalty=pp, frequency_penalty=fp))
    lse = torch.zeros(B, device=dev)
    for bs in (None, bias):
        out, lse = torch.full_like(x, 7.0), torch.zeros(B, device=dev)
        S.logit_process_rows(x, t, hist, bs, out, lse)
        for b, (rp, pp, fp) in enumerate(pen):
            o1, l1 = torch.zeros_like(x[b : b + 1]), torch.zeros(1, device=dev)
            S.logit_process(x[b : b + 1], hist[b : b + 1], bs, rp, pp, fp, o1, l1)
            assert torch.equal(bits(out[b]), bits(o1[0])), b
            assert torch.equal(lse[b], l1[0]), b
        if bs is None:  # neutral penalties: every bit stays
            assert torch.equal(bits(out[1]), bits(x[1]))
    # an idle slot's row and lse are not written; a rows map processes the named slot alone
    t.done[2:3].fill_(1)
    out2, lse2 = torch.full_like(x, 7.0), torch.full((B,), 7.0, device=dev)
    S.logit_process_rows(x, t, hist, bias, out2, lse2)
    assert (out2[2] == 7).all() and float(lse2[2]) == 7.0 and torch.equal(bits(out2[[0, 1, 3, 4]]), bits(out[[0, 1, 3, 4]]))
    o1, lse3 = torch.full_like(x[4:5], 7.0), torch.full((B,), 7.0, device=dev)
    S.logit_process_rows(x[4:5].contiguous(), t, hist, bias, o1, lse3, rows=[4])
    assert torch.equal(bits(o1[0]), bits(out[4])) and lse3.tolist()[:4] == [7.0] * 4 and torch.equal(lse3[4], lse[4])
    t.done[2:3].zero_()
    # commit: draw (greedy), then commit, against token_commit on each row alone at its column
    ids, toks = buffers(dev, B, 4)
    S.sample_rows(x, t, ids, toks)
    t.done[2:3].fill_(1)  # finished by its draw: still commits it
    h2, lp = hist.clone(), torch.full((B, 4), float("nan"), device=dev)
    S.token_commit_rows(toks, t, h2, x, lse, lp)
    for b in range(B):
        h1, lp1 = hist[b : b + 1].clone(), torch.full((1, 4), float("nan"), device=dev)
        S.token_commit(toks[b : b + 1], torch.tensor([0, 0], device=dev), h1, x[b : b + 1], lse[b : b + 1], lp1)
        assert torch.equal(h2[b], h1[0]) and torch.equal(lp[b, :1], lp1[0, :1]), b
    assert torch.isnan(lp[:, 1:]).all() and t.committed.tolist() == [1] * B
    again = (h2.clone(), lp.clone())
    S.token_commit_rows(toks, t, h2, x, lse, lp)  # nothing drawn since: nothing committed
    assert torch.equal(h2, again[0]) and torch.equal(lp.nan_to_num(), again[1].nan_to_num())


MODES = ((0.0, 0, 1.0), (0.8, 50, 1.0), (0.8, 0, 0.95), (0.8, 50, 0.95))  # greedy, top-k, top-p, both


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", (1025, 50257))
def test_philox_row_is_sample_step_row(gpu_device, V, dtype):
    """One seed in every slot and ``philox_row[b] = b``: ``sample_step``'s stream at ``rng = (seed, count)``, token
    for token (how ``generate`` runs on the table); a slot left at the default 0 is a one-row ``sample_step``."""
    B, seed, dev = 4, 2**40 + 5, gpu_device
    x = SR.random_rows(V + 2, B, V, dtype).to(dev)
    for T, k, p in MODES if V == 1025 else MODES[3:]:
        for count in (0, 1, 2**32 + 5):
            t = S.SamplingTable(B, dev)
            t.set(slice(0, B), S.SamplingParams(temperature=T, top_k=k, top_p=p, seed=seed, max_new_tokens=2**31 - 1))
            t.philox_row.copy_(torch.tensor([0, 1, 2, 0], dtype=torch.int32))
            t.count.fill_(count)
            ids, out = buffers(dev, B)
            S.sample_rows(x, t, ids, out)
            rng = torch.tensor([seed, count], device=dev)
            i1, o1 = buffers(dev, B, 1)
            S.sample_step(x, T, k, p, rng, i1, o1, None, torch.zeros(B, dtype=torch.int32, device=dev), -1)
            i2, o2 = buffers(dev, 1, 1)
            S.sample_step(x[3:4], T, k, p, rng, i2, o2, None, torch.zeros(1, dtype=torch.int32, device=dev), -1)
            assert ids.view(-1).tolist() == i1.view(-1).tolist()[:3] + [int(i2)], (T, k, p, count)
            fin = int(count + 1 >= 2**31 - 1)  # (the limit is the table's largest: only a count past it ends a slot)
            assert t.count.tolist() == [count + 1] * B and t.done.tolist() == [fin] * B and t.step.tolist() == [1 - fin] * B
            if count < N_OUT:
                assert out[:, count].tolist() == ids.view(-1).tolist()
