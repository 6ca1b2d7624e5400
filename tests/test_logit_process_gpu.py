"""``logit_process`` / ``token_commit`` (``ops/csrc/logit_process.hip``) on the MI355X against the fp64 oracle of
``tests/logit_refs.py``, on the same rounded inputs and the case table ``test_logit_refs.py`` validates on the CPU.
Every output tensor sits between guard words that must survive the launch.

``lse``: the bound is ``logit_refs.lse_bound`` -- 4x the larger of torch's own fp32 ``logsumexp`` error on these rows
(1.122e-06, CPU) and ``2^-22 * max(1, |max x|)``, i.e. 4.5e-06 here.  The kernel's worst ``|lse - lse64|`` over the same
rows, measured on the MI355X: 9.363e-07 on fp32 rows, 8.478e-07 on bf16 rows (both at V = 50257).
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer import ops

from . import logit_refs as LR

pytestmark = pytest.mark.gpu

CASES = LR.all_cases()
PAD = 16  # guard elements on either side (a multiple of 16 bytes for every dtype used)


class Guarded:
    """``t`` copied into the middle of a sentinel-filled device buffer, ``shift`` elements past a 16-byte boundary."""

    def __init__(self, t: torch.Tensor, dev, shift: int = 0, sentinel=77):
        self.buf = torch.full((t.numel() + 2 * PAD + 8,), sentinel, dtype=t.dtype, device=dev)
        self.lo = PAD + shift
        self.view = self.buf[self.lo : self.lo + t.numel()].view(t.shape)
        self.view.copy_(t)
        self.before = self.buf.clone()

    def guards_intact(self) -> bool:
        n = self.view.numel()
        bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.buf.element_size()]
        a, b = self.buf.view(bits), self.before.view(bits)
        return torch.equal(a[: self.lo], b[: self.lo]) and torch.equal(a[self.lo + n :], b[self.lo + n :])

    def unchanged(self) -> bool:
        bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.buf.element_size()]
        return torch.equal(self.buf.view(bits), self.before.view(bits))


def _launch(case, inp, dev):
    x = Guarded(inp["x"], dev, case.shift)
    hist = Guarded(inp["hist"], dev) if case.hist else None
    bias = Guarded(inp["bias"], dev) if case.bias else None
    out = None
    if case.out:
        out = x if case.out_shift < 0 else Guarded(torch.full_like(inp["x"], 5.0), dev, case.out_shift)
    lse = Guarded(torch.full((case.B,), 5.0), dev) if case.lse else None
    ops.logit_process(x.view, hist.view if hist else None, bias.view if bias else None, case.rp, case.pp, case.fp,
                      out.view if out else None, lse.view if lse else None)
    torch.cuda.synchronize()
    return x, hist, bias, out, lse


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_logit_process_matches_oracle(gpu_device, case):
    inp = LR.make(case)
    x, hist, bias, out, lse = _launch(case, inp, gpu_device)
    for g in (x, out, lse):
        assert g is None or g.guards_intact(), "a word outside the tensor was written"
    for g in (hist, bias) + ((x,) if out is not x else ()):
        assert g is None or g.unchanged(), "an input was written"
    if case.out:
        LR.check_processed(case, inp, out.view.cpu())
    if case.lse:
        err = (lse.view.cpu().double() - LR.lse64(inp["x"])).abs()
        print(f"{case.name}: kernel worst |lse - lse64| = {float(err.max()):.3e}")
        assert bool((err <= LR.lse_bound(inp["x"].float().amax(-1))).all()), float(err.max())
    # a pure function of its inputs: a second launch on the same inputs gives the same bits
    x2, _, _, out2, lse2 = _launch(case, inp, gpu_device)
    assert out is None or torch.equal(out.buf, out2.buf)
    assert lse is None or torch.equal(lse.buf, lse2.buf)


def test_untouched_bits_and_minus_inf_bias(gpu_device):
    x = torch.tensor([[-0.0, 0.0, 1.5, -2.5, -math.inf, 3.0, -0.0, 1e-40, 2.0]])
    hist = torch.tensor([[0, 0, 0, 1, 0, 2, 1, 0, 2001]], dtype=torch.int32)
    bias = torch.zeros(9)
    bias[8] = -math.inf
    for dt, bits in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
        xi = x.to(dt)
        for h, b in ((None, None), (hist, None), (None, bias), (hist, bias)):
            out = torch.full_like(xi, 9.0).to(gpu_device)
            ops.logit_process(xi.to(gpu_device), None if h is None else h.to(gpu_device),
                              None if b is None else b.to(gpu_device), 1.7, 0.5, 0.25, out)
            want = torch.full_like(xi, 9.0)
            ops.logit_process_reference(xi, h, b, 1.7, 0.5, 0.25, want)
            keep = torch.ones(9, dtype=torch.bool)
            if h is not None:
                keep &= h[0] == 0
            if b is not None:
                keep &= b == 0
            got = out.cpu()
            assert torch.equal(got.view(bits)[0][keep], xi.view(bits)[0][keep])
            # the reference's bits: every count here is 0 or 1 (or under the -inf bias), so fp * c is exact and an FMA
            # contraction of y - fp * c cannot round differently
            assert torch.equal(got.view(bits), want.view(bits))
            if b is not None:
                assert float(got[0, 8]) == -math.inf


def test_binding_checks(gpu_device):
    x = torch.zeros(2, 8, device=gpu_device)
    out = torch.empty_like(x)
    with pytest.raises(ValueError):
        ops.logit_process(x, None, None, 0.0, 0.0, 0.0, out)
    hip = torch.ops.bpe_hip
    with pytest.raises(RuntimeError, match="repetition_penalty"):
        hip.logit_process(x, None, None, -1.0, -1.0, 0.0, 0.0, out, None)
    with pytest.raises(RuntimeError, match="hist"):
        hip.logit_process(x, torch.zeros(2, 7, dtype=torch.int32, device=gpu_device), None, 1.0, 1.0, 0.0, 0.0, out, None)
    with pytest.raises(RuntimeError, match="bias"):
        hip.logit_process(x, None, torch.zeros(9, device=gpu_device), 1.0, 1.0, 0.0, 0.0, out, None)
    with pytest.raises(RuntimeError, match="out"):
        hip.logit_process(x, None, None, 1.0, 1.0, 0.0, 0.0, torch.empty(2, 8, dtype=torch.bfloat16, device=gpu_device), None)
    with pytest.raises(RuntimeError, match="raw_logits"):
        hip.token_commit(torch.zeros(2, 3, dtype=torch.long, device=gpu_device),
                         torch.zeros(2, dtype=torch.long, device=gpu_device),
                         torch.zeros(2, 8, dtype=torch.int32, device=gpu_device), torch.zeros(2, 9, device=gpu_device),
                         torch.zeros(2, device=gpu_device), torch.zeros(2, 3, device=gpu_device))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("count", [2, 5, 6, 9])
def test_token_commit_contract(gpu_device, dtype, count):
    """Active and idle rows, the token at 0 and at V - 1, ``count`` inside, at the last column of ``logprob`` (5), past
    it (``hist`` still moves) and past the tokens' columns (nothing moves); guard words around ``hist`` and
    ``logprob``; the result is the reference's, bit for bit, and the same on a second launch."""
    B, V, N, M = 5, 1025, 8, 6
    g = torch.Generator().manual_seed(count)
    tokens = torch.full((B, N), -7, dtype=torch.long)
    if count < N:
        tokens[:, count] = torch.tensor([0, -1, V - 1, 517, -1])
    raw = (torch.randn(B, V, generator=g) * 4).to(dtype)
    lse = torch.randn(B, generator=g) + 9
    hist0 = torch.randint(0, 5, (B, V), generator=g, dtype=torch.int32)
    rng = torch.tensor([2**40 + 3, count])
    want_h, want_lp = hist0.clone(), torch.full((B, M), math.nan)
    ops.token_commit_reference(tokens, rng, want_h, raw, lse, want_lp)
    moved = (want_h != hist0).sum().item()
    assert moved == (3 if count < N else 0) and (~torch.isnan(want_lp)).sum().item() == (3 if count < M else 0)

    def run():
        hist, lp = Guarded(hist0, gpu_device), Guarded(torch.full((B, M), math.nan), gpu_device)
        d = [t.to(gpu_device) for t in (tokens, rng, raw, lse)]
        ops.token_commit(d[0], d[1], hist.view, d[2], d[3], lp.view)
        torch.cuda.synchronize()
        assert hist.guards_intact() and lp.guards_intact()
        assert d[1].tolist() == rng.tolist()
        return hist, lp

    hist, lp = run()
    assert torch.equal(hist.view.cpu(), want_h)
    assert torch.equal(lp.view.cpu().view(torch.int32), want_lp.view(torch.int32))
    hist2, lp2 = run()
    assert torch.equal(hist.buf, hist2.buf) and torch.equal(lp.buf.view(torch.int32), lp2.buf.view(torch.int32))
    # either half alone
    h = Guarded(hist0, gpu_device)
    ops.token_commit(tokens.to(gpu_device), rng.to(gpu_device), h.view)
    assert torch.equal(h.view.cpu(), want_h) and h.guards_intact()
    lp3 = Guarded(torch.full((B, M), math.nan), gpu_device)
    ops.token_commit(tokens.to(gpu_device), rng.to(gpu_device), None, raw.to(gpu_device), lse.to(gpu_device), lp3.view)
    assert torch.equal(lp3.buf.view(torch.int32), lp.buf.view(torch.int32))
