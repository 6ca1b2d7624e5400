"""The prompt-lookup kernel (``ops/csrc/lookup_draft.hip``) on the MI355X against the brute-force oracle of
``tests/lookup_refs.py``, exact equality of every ``win`` row over the case list that ``tests/test_lookup_refs.py``
validates on the CPU; and point-mass verification (``spec_verify(..., point_mass=True)``, ``ops/csrc/spec_verify.hip``)
against the same kernel called with one-hot draft logits, the fp64 oracle of ``tests/spec_refs.py``, the in-graph
contract of ``spec_verify_step`` and the distribution of what it emits."""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import lookup_refs as L
from . import spec_refs as R
from .point_mass_cases import dist_first_tokens, onehot, peaked_fixture, sampling_cases

pytestmark = pytest.mark.gpu

CASES = L.all_cases()


# ---------------------------------------------------------------- the lookup kernel
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_lookup_equals_the_oracle(gpu_device, case):
    win, after, before = case.run(S.lookup_draft, gpu_device)
    want = case.expected()
    bad = (win != want).any(1).nonzero().flatten().tolist()
    assert not bad, (case.name, bad[:4], win[bad[:4]].tolist(), want[bad[:4]].tolist())
    assert all(torch.equal(after[k], before[k]) for k in before)  # nothing else is written


def test_lookup_fuzz(gpu_device):
    rows = 0
    for case in L.fuzz_cases():
        win, _, _ = case.run(S.lookup_draft, gpu_device)
        assert torch.equal(win, case.expected()), case.name
        rows += win.shape[0]
    assert rows >= 300


def test_lookup_is_a_pure_function(gpu_device):
    for case in (CASES[0], CASES[-1]):
        a = case.run(S.lookup_draft, gpu_device)[0]
        assert all(torch.equal(a, case.run(S.lookup_draft, gpu_device)[0]) for _ in range(3))


def test_lookup_reads_strided_rows(gpu_device):
    """``out`` as the session passes it: the first columns of a wider buffer (rows dense, row stride larger)."""
    case = CASES[0]
    dev = gpu_device
    wide = torch.full((case.out.shape[0], case.out.shape[1] + 5), 7, dtype=torch.long, device=dev)
    out = wide[:, : case.out.shape[1]]
    out.copy_(case.out)
    win = case.win.clone().to(dev)
    S.lookup_draft(case.prompt.to(dev), case.n_prompt.to(dev), out, case.n_out.to(dev), win, case.step.to(dev),
                   case.done.to(dev), case.n_hi, case.n_lo)
    assert torch.equal(win.cpu(), case.expected())


# ---------------------------------------------------------------- point-mass verification
def _pair(c, dev, t=None):
    """(n, y) of the point-mass form and of the existing kernel on one-hot draft logits."""
    t = c.t.to(dev) if t is None else t
    d, ua, us = c.d.to(dev), c.ua.to(dev), c.us.to(dev)
    a = S.spec_verify(t, d, None, c.T, ua, us, point_mass=True)
    b = S.spec_verify(t, d, onehot(c.d, c.t).to(dev), c.T, ua, us)
    assert a[0].dtype == torch.int32 and a[1].dtype == torch.int64
    return [v.cpu() for v in a], [v.cpu() for v in b]


@pytest.mark.parametrize("case", sampling_cases(), ids=lambda c: c.name)
def test_point_mass_equals_one_hot_draft_logits(gpu_device, case):
    a, b = _pair(case, gpu_device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (a, b)
    R.Case(case.name, case.t, case.d, onehot(case.d, case.t), case.T, case.ua, case.us).check(*a)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_point_mass_peaked_fixture(gpu_device, dtype):
    t, d, ua, us = peaked_fixture(dtype=dtype)
    ref_n, _ = S.spec_verify_reference(t, d, None, 1.0, ua, us, point_mass=True)
    assert int(ref_n[0]) >= 1 and int(ref_n[1]) == 0  # a draft stands, a draft falls: on the CPU reference first
    c = R.Case("peaked", t[:2], d[:2], onehot(d, t)[:2], 1.0, ua[:2], us[:2])
    a, b = _pair(c, gpu_device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c.check(*a)
    assert int(a[0][0]) >= 1 and int(a[0][1]) == 0
    # a draft outside the vocabulary never stands; the token after it is the draw from p itself
    dev = gpu_device
    n, y = S.spec_verify(t.to(dev), d.to(dev), None, 1.0, ua.to(dev), us.to(dev), point_mass=True)
    want = S.sample_logits(t[2, :1].to(dev).contiguous(), 1.0, 0, 1.0, us[2:].to(dev))
    assert int(n[2]) == 0 and int(y[2]) == int(want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shift", [1, 3, 5])
def test_point_mass_rows_at_any_element_offset(gpu_device, dtype, shift):
    c = next(c for c in sampling_cases() if c.name == f"random-V1000-K4-B3-{str(dtype)[6:]}")
    buf = torch.zeros(c.t.numel() + 16, dtype=dtype, device=gpu_device)
    v = buf[shift : shift + c.t.numel()].view(c.t.shape)
    v.copy_(c.t)
    a, b = _pair(c, gpu_device, v)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    aligned, _ = _pair(c, gpu_device)
    assert torch.equal(a[0], aligned[0]) and torch.equal(a[1], aligned[1])


def test_point_mass_false_is_unchanged(gpu_device):
    """The keyword at its default, given explicitly, and absent: the same (n, y), inside the oracle's sets."""
    dev = gpu_device
    names = ("random-V97-K4-B3-bfloat16", "random-V50257-K7-B3-float32", "greedy-V1000-K4-B3-bfloat16",
             "p-zero-V97-K4-B3-float32", "reject-first-V50257-K4-B3-bfloat16")
    for c in [c for c in R.all_cases() if c.name in names]:
        args = (c.t.to(dev), c.d.to(dev), c.s.to(dev) if c.T > 0 else None, c.T, c.ua.to(dev), c.us.to(dev))
        a, b = S.spec_verify(*args), S.spec_verify(*args, point_mass=False)
        c.check(a[0].cpu(), a[1].cpu())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if c.T <= 0:  # greedy is unchanged by the keyword
            g = S.spec_verify(args[0], args[1], None, c.T, None, None, point_mass=True)
            assert torch.equal(a[0], g[0]) and torch.equal(a[1], g[1])


def _state(dev, B, K, d, N=12):
    return dict(
        win=torch.cat([torch.full((B, 1), 5), d], 1).to(dev), ids=torch.full((B, 1), -5, device=dev),
        out=torch.full((B, N), -7, device=dev), n_out=torch.tensor([2, 0, 3, 1, 4], dtype=torch.int32, device=dev),
        base=torch.tensor([10, 20, 30, 40, 50], dtype=torch.int32, device=dev),
        pos_t=torch.tensor([10, 20, 30, 40, 50], dtype=torch.int32, device=dev),
        pos_d=torch.tensor([15, 25, 35, 40, 55], dtype=torch.int32, device=dev),
        step_t=torch.tensor([1, 1, 1, 0, 1], dtype=torch.int32, device=dev),
        step_d=torch.tensor([1, 1, 1, 0, 1], dtype=torch.int32, device=dev),
        done=torch.tensor([0, 0, 0, 0, 1], dtype=torch.int32, device=dev))


@pytest.mark.parametrize("T", [0.0, 1.0])
def test_point_mass_step_contract(gpu_device, T):
    """``spec_verify_step(point_mass=True)``: ua / us are philox_uniform at streams 1 / 2; out, n_out, win[:, 0], ids,
    both positions, done and both steps follow the plain-Python model of ``test_spec_verify_gpu.py``; rng untouched;
    idle rows (3: step 0, 4: done) write nothing."""
    dev, B, K, V, N, seed, cnt = gpu_device, 5, 4, 1000, 12, 2**40 + 12345, 2**32 + 3
    t, d, _ = R.related_rows(21, B, K, V, torch.bfloat16, noise=0.3)
    t[1, torch.arange(K), t[1, :K].float().argmax(-1)] += 12.0  # row 1: peaked rows, and it drafts their argmax
    d[1] = t[1, :K].float().argmax(-1)
    t = t.to(dev)
    ua = torch.stack([S.philox_uniform(seed, cnt + i, B, dev, stream=1) for i in range(K)], 1)
    us = S.philox_uniform(seed, cnt, B, dev, stream=2)
    n, y = (v.cpu().tolist() for v in S.spec_verify(t, d.to(dev), None, T, ua, us, point_mass=True))
    R.Case("step", t.cpu(), d, onehot(d, t.cpu()), T, ua.cpu(), us.cpu()).check(torch.tensor(n), torch.tensor(y))
    assert n[1] >= 2, "the fixture must accept drafts in row 1"
    rng = torch.tensor([seed, cnt], device=dev)
    active = [0, 1, 2]
    emitted = [d[b, : n[b]].tolist() + [y[b]] for b in range(B)]

    def expect(eos, width):
        st0 = {k: v.cpu().clone() for k, v in _state(dev, B, K, d, width).items()}
        for b in active:
            o, m, fin = int(st0["n_out"][b]), 0, False
            for tok in emitted[b]:
                if fin or o + m >= width:
                    break
                st0["out"][b, o + m] = tok
                m += 1
                fin = tok == eos
            fin = fin or o + m >= width
            st0["n_out"][b] = o + m
            if m:
                st0["win"][b, 0] = st0["ids"][b, 0] = emitted[b][m - 1]
                st0["pos_t"][b] = st0["pos_d"][b] = int(st0["base"][b]) + m
            if fin:
                st0["done"][b], st0["step_t"][b], st0["step_d"][b] = 1, 0, 0
        return st0

    # no EOS; EOS as an accepted draft in the middle of the window; EOS as y; `out` too narrow for row 2
    for eos, width in ((-1, N), (emitted[1][1], N), (y[0], N), (-1, 4)):
        st = _state(dev, B, K, d, width)
        S.spec_verify_step(t, None, T, rng, st["win"], st["ids"], st["out"], st["n_out"], st["base"], st["pos_t"],
                           st["pos_d"], st["step_t"], st["step_d"], st["done"], eos, point_mass=True)
        torch.cuda.synchronize()
        want = expect(eos, width)
        for k in want:
            assert torch.equal(st[k].cpu(), want[k]), (eos, width, k, st[k].tolist(), want[k].tolist())
        assert rng.tolist() == [seed, cnt]
    assert want["done"][2] == 1 and want["n_out"][2] == 4  # the narrow `out` finished row 2


def test_point_mass_first_token_distribution(gpu_device):
    """20 000 sequences, K = 1, a deterministic draft per row: the first emitted token is distributed as p within
    5 sigma per token -- the statistic, bound and draws of the draft-model form's test."""
    N, seed = 20000, 11
    dev = gpu_device
    t, d, _, _ = dist_first_tokens(N, seed)
    win = torch.cat([torch.zeros(N, 1, dtype=torch.long), d[:, None]], 1).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = torch.full((N, 2), -1, device=dev)
    z, pos = torch.zeros(N, **i32), torch.zeros(N, **i32)
    S.spec_verify_step(t.to(dev), None, 1.0, torch.tensor([seed, 0], device=dev), win,
                       torch.zeros(N, 1, dtype=torch.long, device=dev), out, torch.zeros(N, **i32), z, pos, pos.clone(),
                       torch.ones(N, **i32), torch.ones(N, **i32), torch.zeros(N, **i32), -1, point_mass=True)
    worst = R.dist_check(out[:, 0].cpu().numpy(), N)
    print(f"first-token deviation: {worst:.2f} sigma")
    assert worst <= 5.0
