"""The sampling controls on the CPU: the torch references of ``ops/sampling.py`` (``logit_process_reference``,
``token_commit_reference``, ``prompt_hist``) against the fp64 oracle of ``tests/logit_refs.py`` under its derived
bounds, and the fixture's own guarantees (``test_logit_process_gpu.py`` runs the same cases on the kernels)."""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer import ops
from bpe_transformer.ops import sampling as S

from . import logit_refs as LR

CASES = LR.all_cases()


@pytest.fixture(scope="module")
def inputs():
    return {c.name: LR.make(c) for c in CASES}


def test_case_table_reaches_every_shape():
    assert {c.V for c in CASES} >= set(LR.SIZES) and {c.B for c in CASES} == {1, 3}
    for dt in (torch.float32, torch.bfloat16):
        mine = [c for c in CASES if c.dtype == dt]
        assert {c.shift for c in mine} >= {0, 1, 3, 5} and {c.rp for c in mine} == {1.0, 1.3, 0.7}
        assert any(c.out_shift < 0 for c in mine) and any(c.out_shift >= 0 and c.out_shift != c.shift for c in mine)
        assert any(not c.hist and c.out for c in mine) and any(not c.bias and c.out for c in mine)
        assert any(not c.lse for c in mine) and any(not c.out for c in mine)


def test_fixture_is_clear_of_bf16_rounding(inputs):
    """No processed value of a bf16 row lies within the fp32 bound of a bf16 rounding boundary, and every hist row has
    the counts 0, 1 and 1000, on and off the prompt."""
    for c in CASES:
        inp = inputs[c.name]
        if c.hist and c.V >= 63:
            assert set(inp["hist"].unique().tolist()) == {0, 1, 2, 3, 2000, 2001}
        if c.dtype != torch.bfloat16 or not c.out:
            continue
        ref = LR.process64(inp["x"], inp["hist"], inp["bias"], c.rp, c.pp, c.fp)
        t = LR.touched(inp["hist"], inp["bias"], ref.shape)
        d = LR.bf16_boundary_distance(ref)
        assert bool((d[t] > LR.process_bound(inp["x"], inp["hist"], inp["bias"], c.rp, c.pp, c.fp)[t]).all()), c.name


def test_boundary_distance():
    y = torch.tensor([1.0, 1.00390625, 1.005, -3.0, 0.0, math.inf], dtype=torch.float64)  # 1 + 2^-8 is a midpoint
    d = LR.bf16_boundary_distance(y)
    assert d[0] == 2.0**-8 and d[1] == 0 and abs(float(d[2]) - (1.005 - 1.00390625)) < 1e-12
    assert d[3] == 2.0**-7 and math.isinf(d[4]) and math.isinf(d[5])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_matches_oracle(inputs, case):
    inp = inputs[case.name]
    x = inp["x"].clone()
    out = None if not case.out else (x if case.out_shift < 0 else torch.full_like(x, 7.0))
    lse = torch.full((case.B,), 7.0) if case.lse else None
    ops.logit_process(x, inp["hist"], inp["bias"], case.rp, case.pp, case.fp, out, lse)
    if case.out:
        LR.check_processed(case, inp, out)
    if case.out_shift >= 0 or not case.out:
        assert torch.equal(x.view(torch.uint8), inp["x"].view(torch.uint8)), "out of place: the input is read only"
    if case.lse:
        ref = LR.lse64(inp["x"])
        err = (lse.double() - ref).abs()
        assert bool((err <= LR.lse_bound(inp["x"].float().amax(-1))).all()), float(err.max())


def test_torch_logsumexp_error_is_what_the_bound_rests_on(inputs):
    """``LSE_CPU_ERR`` is torch's own fp32 ``logsumexp`` error over the table's rows, as measured on the CPU; it may
    come out a little differently on another CPU, not by a factor of two."""
    worst = max(float((torch.logsumexp(inputs[c.name]["x"].float(), -1).double() - LR.lse64(inputs[c.name]["x"])).abs()
                      .max()) for c in CASES)
    print(f"torch fp32 logsumexp: worst |err| = {worst:.3e}")
    assert worst <= 2 * LR.LSE_CPU_ERR


def test_untouched_elements_keep_their_bits():
    x = torch.tensor([[-0.0, 0.0, 1.5, -2.5, -math.inf, 3.0, -0.0, 1e-40]])
    hist = torch.tensor([[0, 0, 0, 1, 0, 2, 1, 0]], dtype=torch.int32)
    for dt in (torch.float32, torch.bfloat16):
        xi = x.to(dt)
        bits = torch.int32 if dt == torch.float32 else torch.int16
        for h, b in ((None, None), (hist, None), (hist, torch.zeros(8)), (None, torch.zeros(8)),
                     (None, torch.tensor([0.0, -0.0, 0, 0, 0, 0, 0, 0]))):
            out = torch.full_like(xi, 9.0)
            S.logit_process_reference(xi, h, b, 1.0, 0.0, 0.0, out)
            # rp = 1: x * 1.0 == x too.  (A seen -0.0 under a bias of 0 is touched: step 1 makes it -0.0 + 0.0 = +0.0.)
            same = torch.ones(8, dtype=torch.bool)
            same[6] = h is None or b is None
            assert torch.equal(out.view(bits)[0][same], xi.view(bits)[0][same]), (dt, h is None, b is None)
            out = torch.full_like(xi, 9.0)
            S.logit_process_reference(xi, h, b, 1.7, 0.5, 0.25, out)
            keep = torch.ones(8, dtype=torch.bool) if h is None else (h[0] == 0)
            assert torch.equal(out.view(bits)[0][keep], xi.view(bits)[0][keep])
            if h is not None:  # -0.0 times rp stays -0.0; the seen negative grows, the emitted positive shrinks
                assert b is not None or out.view(bits)[0, 6] == xi.view(bits)[0, 6]
                assert float(out[0, 3]) == float((xi[0, 3].float() * S._f32(1.7)).to(dt))
                assert float(out[0, 5]) < float(xi[0, 5])


def test_minus_inf_bias_survives():
    x = torch.tensor([[2.0, -1.0, 0.5, 4.0]])
    hist = torch.tensor([[3, 2001, 0, 0]], dtype=torch.int32)
    bias = torch.tensor([-math.inf, -math.inf, -math.inf, 0.0])
    for dt in (torch.float32, torch.bfloat16):
        out = torch.empty(1, 4, dtype=dt)
        lse = torch.empty(1)
        ops.logit_process(x.to(dt), hist, bias, 0.7, 2.0, 0.5, out, lse)
        assert out[0, :3].tolist() == [-math.inf] * 3 and float(out[0, 3]) == 4.0
        assert abs(float(lse) - float(torch.logsumexp(x.double(), -1))) < 1e-6  # the unprocessed row


def test_rp_must_be_positive():
    x = torch.zeros(1, 4)
    for rp in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            ops.logit_process(x, None, None, rp, 0.0, 0.0, torch.empty_like(x))


def test_prompt_hist_ignores_padding():
    ids = torch.tensor([[5, 2, 5, 9, 9], [1, 9, 9, 9, 9], [0, 1, 2, 3, 4]])
    h = ops.prompt_hist(ids, [3, 1, 5], 10)
    assert h.dtype == torch.int32 and h.shape == (3, 10)
    assert h[0].nonzero().flatten().tolist() == [2, 5] and h[1].nonzero().flatten().tolist() == [1]
    assert h[2].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0] and int(h.max()) == 1
    assert torch.equal(ops.prompt_hist(ids, None, 10)[0].nonzero().flatten(), torch.tensor([2, 5, 9]))
    pad = ids.clone()
    pad[0, 3:] = 7
    pad[1, 1:] = 3
    assert torch.equal(ops.prompt_hist(pad, [3, 1, 5], 10), h)


def _commit_setup():
    V, N = 11, 4
    tokens = torch.full((4, N), -7, dtype=torch.long)
    tokens[:, 2] = torch.tensor([0, -1, V - 1, 4])  # row 1 is idle
    raw = torch.arange(4 * V, dtype=torch.float32).view(4, V) / 8
    lse = torch.tensor([1.0, 2.0, 3.0, 4.0])
    hist = torch.ones(4, V, dtype=torch.int32)
    return V, N, tokens, raw, lse, hist


def test_token_commit_reference_contract():
    V, N, tokens, raw, lse, hist = _commit_setup()
    rng = torch.tensor([99, 2])
    lp = torch.full((4, N), math.nan)
    h = hist.clone()
    ops.token_commit(tokens, rng, h, raw, lse, lp)
    want = hist.clone()
    want[0, 0] += 2
    want[2, V - 1] += 2
    want[3, 4] += 2
    assert torch.equal(h, want) and rng.tolist() == [99, 2]
    assert lp[:, 2].tolist()[0] == 0.0 - 1.0 and math.isnan(float(lp[1, 2]))
    assert float(lp[2, 2]) == float(raw[2, V - 1]) - 3.0 and float(lp[3, 2]) == float(raw[3, 4]) - 4.0
    assert bool(torch.isnan(lp[:, [0, 1, 3]]).all())
    # bf16 raw logits: the value is the bf16 logit itself, widened
    lp2 = torch.full((4, N), math.nan)
    ops.token_commit(tokens, rng, None, raw.bfloat16(), lse, lp2)
    assert float(lp2[3, 2]) == float(raw.bfloat16()[3, 4].float() - lse[3])
    # either half alone
    h = hist.clone()
    ops.token_commit(tokens, rng, h)
    assert torch.equal(h, want)
    # count past logprob's columns (the last column of a narrower logprob is still written), past the tokens' too
    h, short = hist.clone(), torch.full((4, 2), math.nan)
    ops.token_commit(tokens, rng, h, raw, lse, short)
    assert torch.equal(h, want) and bool(torch.isnan(short).all())
    last = torch.full((4, 3), math.nan)
    ops.token_commit(tokens, rng, None, raw, lse, last)
    assert float(last[0, 2]) == -1.0
    h = hist.clone()
    ops.token_commit(tokens, torch.tensor([99, N]), h, raw, lse, lp := torch.full((4, N), math.nan))
    assert torch.equal(h, hist) and bool(torch.isnan(lp).all())
