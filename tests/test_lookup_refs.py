"""The brute-force oracle of the prompt-lookup proposer (``tests/lookup_refs.py``) on hand-computed histories, the
torch ``lookup_draft_reference`` of ``ops/sampling.py`` against it over every case of the GPU test, and the
point-mass form of the verification reference (``spec_verify_reference(point_mass=True)``) against the fp64 oracle
of ``tests/spec_refs.py`` called with one-hot draft logits."""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import lookup_refs as L
from . import spec_refs as R
from .point_mass_cases import dist_first_tokens, onehot, peaked_fixture, sampling_cases

CASES = L.all_cases()
FUZZ = L.fuzz_cases()


def test_oracle_on_hand_computed_histories():
    assert L.lookup([5], 3, 3) == [5, 5, 5]
    assert L.lookup([5, 6], 2, 3) == [6, 6]
    assert L.lookup([5, 5], 2, 3) == [5, 5]
    assert L.lookup([1, 2, 3, 7, 8, 3, 6, 1, 2, 3], 4, 3) == [7, 8, 3, 6]  # the longer, earlier match
    assert L.lookup([1, 2, 3, 7, 8, 3, 6, 1, 2, 3], 4, 1) == [6, 1, 2, 3]  # n_hi = 1: the later [3]
    assert L.lookup([1, 2, 5, 1, 2, 6, 1, 2], 4, 2) == [6, 1, 2, 6]  # the later of two, then periodic (p = 3)
    assert L.lookup([1, 2, 1, 2], 5, 3) == [1, 2, 1, 2, 1]
    assert L.lookup([4, 7, 7], 3, 3) == [7, 7, 7]
    assert L.lookup([1, 2, 3, 9, 2, 3], 4, 3, 2) == [9, 2, 3, 9]
    assert L.lookup([1, 2, 3, 4, 3], 2, 3, 2) == [3, 3]  # one token matches, below n_lo
    assert L.lookup([1, 2, 21, 22, 21, 22, 21], 4, 3) == [22, 21, 22, 21]


@pytest.mark.parametrize("case", CASES + FUZZ, ids=lambda c: c.name)
def test_reference_equals_the_oracle(case):
    win, after, before = case.run(S.lookup_draft_reference)
    assert torch.equal(win, case.expected()), (win.tolist(), case.expected().tolist())
    assert all(torch.equal(after[k], before[k]) for k in before)  # nothing else is written
    win2, _, _ = case.run(S.lookup_draft)  # the public op on the CPU is the reference
    assert torch.equal(win2, win)


def test_the_fuzz_has_matches_and_non_matches():
    hits = [m for c in FUZZ for m in c.matched()]
    assert len(hits) >= 300 and sum(hits) >= 100 and len(hits) - sum(hits) >= 30, (len(hits), sum(hits))


def test_bounds_are_checked():
    c = CASES[0]
    for n_hi, n_lo in ((0, 0), (2, 0), (2, 3)):
        with pytest.raises(ValueError, match="n_lo"):
            S.lookup_draft(c.prompt, c.n_prompt, c.out, c.n_out, c.win.clone(), c.step, c.done, n_hi, n_lo)


# ---------------------------------------------------------------- point-mass verification, the CPU reference
@pytest.mark.parametrize("case", sampling_cases(), ids=lambda c: c.name)
def test_point_mass_reference_inside_the_one_hot_oracle(case):
    """The reference with ``point_mass=True`` is an acceptable outcome of the fp64 oracle given one-hot draft logits,
    and equals the reference itself given them."""
    n, y = S.spec_verify_reference(case.t, case.d, None, case.T, case.ua, case.us, point_mass=True)
    R.Case(case.name, case.t, case.d, onehot(case.d, case.t), case.T, case.ua, case.us).check(n, y)
    n1, y1 = S.spec_verify_reference(case.t, case.d, onehot(case.d, case.t), case.T, case.ua, case.us)
    assert torch.equal(n, n1) and torch.equal(y, y1)


def test_point_mass_peaked_fixture_accepts_and_rejects():
    t, d, ua, us = peaked_fixture()
    n, y = S.spec_verify_reference(t, d, None, 1.0, ua, us, point_mass=True)
    R.Case("peaked", t[:2], d[:2], onehot(d, t)[:2], 1.0, ua[:2], us[:2]).check(n[:2], y[:2])
    assert int(n[0]) >= 1 and int(n[1]) == 0 and int(y[1]) != int(d[1, 0]), (n.tolist(), y.tolist())
    # a draft outside the vocabulary never stands, and the token after it is drawn from p itself
    assert int(n[2]) == 0 and int(y[2]) == int(S.sample_logits_reference(t[2, :1], 1.0, 0, 1.0, us[2:]))


def test_point_mass_false_is_unchanged_and_greedy_ignores_it():
    for c in [c for c in R.all_cases() if c.t.shape[2] == 97][:6]:
        a = S.spec_verify_reference(c.t, c.d, c.s if c.T > 0 else None, c.T, c.ua, c.us)
        b = S.spec_verify_reference(c.t, c.d, c.s if c.T > 0 else None, c.T, c.ua, c.us, point_mass=False)
        c.check(*b)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if c.T <= 0:
            g = S.spec_verify_reference(c.t, c.d, None, c.T, None, None, point_mass=True)
            assert torch.equal(a[0], g[0]) and torch.equal(a[1], g[1])


def test_point_mass_distribution_on_the_cpu_reference():
    """20 000 rows, K = 1, a deterministic draft per row: the first emitted token is distributed as p within the
    5 sigma per token of the draft-model form's test."""
    N, seed = 20000, 11
    t, d, ua, us = dist_first_tokens(N, seed)
    n, y = S.spec_verify_reference(t, d[:, None], None, 1.0, ua[:, None], us, point_mass=True)
    worst = R.dist_check(torch.where(n > 0, d, y).numpy(), N)
    print(f"first-token deviation: {worst:.2f} sigma")
    assert worst <= 5.0
