"""The speculative-verification kernel (``ops/csrc/spec_verify.hip``) on the MI355X against the fp64 oracle of
``tests/spec_refs.py``, over the case list that ``tests/test_spec_refs.py`` validates on the CPU; rows at any element
offset; the in-graph contract of ``spec_verify_step``; the distribution of what it emits; ``sample_step(col=j)``."""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import sample_refs as SR
from . import spec_refs as R

pytestmark = pytest.mark.gpu

CASES = R.all_cases()


def _verify(c, dev, t=None, s=None):
    t = c.t.to(dev) if t is None else t
    s = c.s.to(dev) if s is None else s
    n, y = S.spec_verify(t, c.d.to(dev), s if c.T > 0 else None, c.T, c.ua.to(dev), c.us.to(dev))
    assert n.dtype == torch.int32 and y.dtype == torch.int64 and n.shape == y.shape == (c.t.shape[0],)
    return n.cpu(), y.cpu()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_spec_verify_matches_oracle(gpu_device, case):
    case.check(*_verify(case, gpu_device))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shift", [1, 3, 5])
def test_rows_at_any_element_offset(gpu_device, dtype, shift):
    """Target and draft logits that start ``shift`` and ``shift + 2`` elements into their buffers: no row is 16-byte
    aligned, and the two arrays' rows are aligned differently."""
    c = next(c for c in CASES if c.name == f"random-V1000-K4-B3-{str(dtype)[6:]}")
    views = []
    for x, sh in ((c.t, shift), (c.s, shift + 2)):
        buf = torch.zeros(x.numel() + 16, dtype=dtype, device=gpu_device)
        v = buf[sh : sh + x.numel()].view(x.shape)
        v.copy_(x)
        views.append(v)
    for T in (1.0, 0.0):
        cc = R.Case(c.name, c.t, c.d, c.s, T, c.ua, c.us)
        cc.check(*_verify(cc, gpu_device, *views))


def test_spec_verify_is_a_pure_function(gpu_device):
    c = next(c for c in CASES if c.name == "random-V50257-K7-B3-bfloat16")
    a = _verify(c, gpu_device)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for b in (_verify(c, gpu_device) for _ in range(3)))


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


def _step(t, s, T, rng, st, eos):
    S.spec_verify_step(t, s, T, rng, st["win"], st["ids"], st["out"], st["n_out"], st["base"], st["pos_t"],
                       st["pos_d"], st["step_t"], st["step_d"], st["done"], eos)
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in st.items()}


@pytest.mark.parametrize("T", [0.0, 1.0])
def test_spec_verify_step_contract(gpu_device, T):
    """ua / us are philox_uniform at streams 1 / 2 exactly; out, n_out, win[:, 0], ids, both pos, done and both step as
    specified; rng untouched; idle rows (3: step 0, 4: done) write nothing; a second call on the same state is
    identical."""
    dev, B, K, V, N, seed, cnt = gpu_device, 5, 4, 1000, 12, 2**40 + 12345, 2**32 + 3
    t, d, s = R.related_rows(21, B, K, V, torch.bfloat16, noise=0.3)
    d[1] = t[1, :K].float().argmax(-1)  # row 1 drafts the target's likeliest tokens: some draft stands
    t, s = t.to(dev), s.to(dev)
    ua = torch.stack([S.philox_uniform(seed, cnt + i, B, dev, stream=1) for i in range(K)], 1)
    us = S.philox_uniform(seed, cnt, B, dev, stream=2)
    n, y = (v.cpu().tolist() for v in S.spec_verify(t, d.to(dev), s, T, ua, us))
    R.Case("step", t.cpu(), d, s.cpu(), T, ua.cpu(), us.cpu()).check(torch.tensor(n), torch.tensor(y))
    assert max(n[:3]) >= 1, "the fixture must accept a draft somewhere"
    rng = torch.tensor([seed, cnt], device=dev)
    active = [0, 1, 2]
    emitted = [d[b, : n[b]].tolist() + [y[b]] for b in range(B)]

    def expect(eos, width):
        """Plain-Python model of the contract."""
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

    acc = next(b for b in active if n[b] >= 1)
    # no EOS; EOS as an accepted draft; EOS as y; `out` too narrow for row 2 (n_out 3 of 4 columns)
    for eos, width in ((-1, N), (emitted[acc][0], N), (y[0], N), (-1, 4)):
        st = _state(dev, B, K, d, width)
        got = _step(t, s if T > 0 else None, T, rng, st, eos)
        want = expect(eos, width)
        for k in want:
            assert torch.equal(got[k], want[k]), (eos, width, k, got[k].tolist(), want[k].tolist())
        assert rng.tolist() == [seed, cnt]
        st2 = _state(dev, B, K, d, width)
        again = _step(t, s if T > 0 else None, T, rng, st2, eos)
        assert all(torch.equal(got[k], again[k]) for k in got)
    assert want["done"][2] == 1 and want["n_out"][2] == 4  # the narrow `out` finished row 2


def test_first_token_distribution(gpu_device):
    """20 000 sequences, K = 1, d_1 ~ q by sample_logits at Philox stream 0: the first emitted token is distributed as
    p within 5 sigma per token (tests/test_spec_refs.py shows a verifier that corrects from p instead of the
    residual missing this by tens of sigma)."""
    N, seed = 20000, 11
    t, s, (u0, _, _) = R.dist_inputs(N, seed)
    dev = gpu_device
    t, s = t.to(dev), s.to(dev)
    d = S.sample_logits(s[:, 0].contiguous(), 1.0, 0, 1.0, u0.to(dev))
    win = torch.cat([torch.zeros(N, 1, dtype=torch.long, device=dev), d[:, None]], 1)
    i32 = dict(dtype=torch.int32, device=dev)
    out = torch.full((N, 2), -1, device=dev)
    z, pos = torch.zeros(N, **i32), torch.zeros(N, **i32)
    S.spec_verify_step(t, s, 1.0, torch.tensor([seed, 0], device=dev), win, torch.zeros(N, 1, dtype=torch.long, device=dev),
                       out, torch.zeros(N, **i32), z, pos, pos.clone(), torch.ones(N, **i32), torch.ones(N, **i32),
                       torch.zeros(N, **i32), -1)
    worst = R.dist_check(out[:, 0].cpu().numpy(), N)
    print(f"first-token deviation: {worst:.2f} sigma")
    assert worst <= 5.0


def test_sample_step_col(gpu_device):
    """col = j writes column j (an idle row leaves it); col = -1 is today's behaviour, bit for bit."""
    dev, B, V, N, seed, count = gpu_device, 4, 1000, 6, 99, 3
    x = SR.random_rows(8, B, V).to(dev)
    want = S.sample_logits(x, 0.9, 0, 1.0, S.philox_uniform(seed, count, B, dev)).cpu().tolist()
    rng = torch.tensor([seed, count], device=dev)
    done = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device=dev)
    step = torch.tensor([1, 1, 0, 1], dtype=torch.int32, device=dev)
    res = {}
    for col in (-1, 5, None):
        ids = torch.full((B, 1), -5, device=dev)
        out = torch.full((B, N), -7, device=dev)
        kw = {} if col is None else {"col": col}
        S.sample_step(x, 0.9, 0, 1.0, rng, ids, out, step, done, -1, **kw)
        assert ids[:, 0].tolist() == want
        res[col] = out.cpu()
    assert torch.equal(res[-1], res[None])
    assert res[-1][:, count].tolist() == [want[0], -1, -1, want[3]] and (res[-1][:, 5] == -7).all()
    assert res[5][:, 5].tolist() == [want[0], -7, -7, want[3]] and (res[5][:, :5] == -7).all()
