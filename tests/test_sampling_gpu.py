"""The sampling kernel (``ops/csrc/sample.hip``) on the MI355X against the fp64 oracle of ``tests/sample_refs.py``:
every token ``sample_logits`` returns must be in the oracle's acceptable set (or be the one exact token where the
case has one), over the case list that ``tests/test_sample_refs.py`` validates on the CPU; and ``sample_step``'s
in-graph contract."""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import sample_refs as SR

pytestmark = pytest.mark.gpu

CASES = SR.all_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_sample_logits_matches_oracle(gpu_device, case):
    tok = S.sample_logits(case.logits.to(gpu_device), case.temperature, case.top_k, case.top_p, case.u.to(gpu_device))
    assert tok.dtype == torch.int64 and tok.shape == (case.logits.shape[0],)
    case.check(tok.cpu())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shift", [1, 3, 5])
def test_rows_at_any_element_offset(gpu_device, dtype, shift):
    """Logits that start ``shift`` elements into their buffer: no row, the first included, is 16-byte aligned."""
    B, V = 3, 4099
    x = SR.random_rows(shift, B, V, dtype)
    buf = torch.zeros(B * V + 8, dtype=dtype, device=gpu_device)
    view = buf[shift : shift + B * V].view(B, V)
    view.copy_(x)
    u = SR.uniforms(shift, B)
    for T, k, p in [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.8, 7, 1.0), (0.8, 50, SR.top_p_mid(SR.f64(x)[0], 0.8, 1, 50)[0])]:
        rows = view if p == 1.0 else view[:1]
        tok = S.sample_logits(rows, T, k, p, u[: rows.shape[0]].to(gpu_device))
        SR.check_tokens(x[: rows.shape[0]], tok.cpu(), T, k, p, u)


def test_sampling_is_a_pure_function(gpu_device):
    x = SR.random_rows(SR.VOCAB_SEED, 2, SR.VOCAB).to(gpu_device)
    u = SR.uniforms(1, 2).to(gpu_device)
    a = S.sample_logits(x, 0.8, 50, 0.95, u)
    assert all(torch.equal(a, S.sample_logits(x, 0.8, 50, 0.95, u)) for _ in range(3))


@pytest.mark.parametrize("ragged", [False, True])
def test_sample_step_contract(gpu_device, ragged):
    """u is philox_uniform exactly; ids, out[:, count], done and the ragged step as specified; rng untouched."""
    B, V, N, seed, count = 5, 4099, 6, 2**40 + 12345, 3
    x = SR.random_rows(8, B, V).to(gpu_device)
    T, k, p = 0.9, 40, 0.9
    want = S.sample_logits(x, T, k, p, S.philox_uniform(seed, count, B, gpu_device)).cpu()
    eos = int(want[3])
    rng = torch.tensor([seed, count], device=gpu_device)
    ids = torch.full((B, 1), -5, dtype=torch.long, device=gpu_device)
    out = torch.full((B, N), -7, dtype=torch.long, device=gpu_device)
    done = torch.tensor([0, 1, 0, 0, 0], dtype=torch.int32, device=gpu_device)
    step = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32, device=gpu_device) if ragged else None
    S.sample_step(x, T, k, p, rng, ids, out, step, done, eos)
    torch.cuda.synchronize()
    assert torch.equal(ids[:, 0].cpu(), want)
    assert rng.tolist() == [seed, count]
    idle = [False, True, ragged, False, False]
    assert out[:, count].tolist() == [-1 if i else int(t) for i, t in zip(idle, want.tolist())]
    assert (out.cpu()[:, [c for c in range(N) if c != count]] == -7).all()
    hit = [not i and int(t) == eos for i, t in zip(idle, want.tolist())]
    assert done.tolist() == [1 if h or b == 1 else 0 for b, h in enumerate(hit)] and hit[3]
    if ragged:
        assert step.tolist() == [0 if h else s for h, s in zip(hit, [1, 1, 0, 1, 1])]
    # no EOS: nothing is marked; a count outside `out` writes no column
    done.zero_()
    rng[1] = N
    S.sample_step(x, T, k, p, rng, ids, out, step, done, -1)
    assert done.tolist() == [0] * B and (out.cpu()[:, [c for c in range(N) if c != count]] == -7).all()
    assert torch.equal(ids[:, 0].cpu(), S.sample_logits(x, T, k, p, S.philox_uniform(seed, N, B, gpu_device)).cpu())
