"""The fp64 oracle of speculative verification (``tests/spec_refs.py``) against hand-computed rows, the torch
``*_reference`` functions of ``ops/sampling.py`` inside the oracle's sets over every case of the GPU test, the bound
on ambiguous cases, and the distribution test on the CPU reference."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import spec_refs as R

CASES = R.all_cases()


def _logs(*rows):
    return np.log(np.array(rows, dtype=np.float64))


def test_oracle_on_hand_computed_rows():
    t = _logs([0.5, 0.25, 0.125, 0.125], [0.1, 0.2, 0.3, 0.4])
    s = _logs([0.25, 0.25, 0.25, 0.25])
    # d = 0: ua * 0.25 < 0.5 whatever ua -> stands; the bonus token from p_2: cum 0.1 0.3 0.6 1.0
    assert R.outcomes(t, [0], s, 1.0, [0.99], 0.35) == {(1, 2)}
    assert R.outcomes(t, [0], s, 1.0, [0.99], 0.95) == {(1, 3)}
    # d = 3: q = 0.25, p = 0.125 -> stands iff ua < 0.5; the residual max(p - q, 0) = (0.25, 0, 0, 0) -> y = 0
    assert R.outcomes(t, [3], s, 1.0, [0.4], 0.35) == {(1, 2)}
    assert R.outcomes(t, [3], s, 1.0, [0.6], 0.35) == {(0, 0)}
    assert R.outcomes(t, [3], s, 1.0, [0.5 * (1 + 0.5 * R.DELTA)], 0.35) == {(0, 0), (1, 2)}  # inside the tolerance
    # a residual with two tokens: p = (.5 .25 .125 .125), q = (.125 .125 .25 .5) -> r = (.375 .125 0 0), R = .5
    s2 = _logs([0.125, 0.125, 0.25, 0.5])
    assert R.outcomes(t, [3], s2, 1.0, [0.9], 0.70) == {(0, 0)}  # 0.9 * 0.5 >= 0.125; us * R = 0.35 < 0.375
    assert R.outcomes(t, [3], s2, 1.0, [0.9], 0.80) == {(0, 1)}
    assert R.outcomes(t, [3], s2, 1.0, [0.9], 0.75) == {(0, 0), (0, 1)}  # on the edge
    # -inf target logit: never stands; greedy: lowest index on ties, n counts the leading matches
    tz = t.copy()
    tz[0, 3] = -np.inf
    assert {n for n, _ in R.outcomes(tz, [3], s, 1.0, [1e-7], 0.5)} == {0}
    tg = np.array([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 1.0, 0.0], [0.0, 0.0, 0.0, 5.0]])
    assert R.outcomes(tg, [1, 0], None, 0.0) == {(2, 3)}
    assert R.outcomes(tg, [2, 0], None, 0.0) == {(0, 1)}
    assert R.outcomes(tg, [1, 1], None, 0.0) == {(1, 0)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_inside_the_oracle_sets(case):
    n, y = S.spec_verify_reference(case.t, case.d, case.s, case.T, case.ua, case.us)
    assert n.dtype == torch.int32 and y.dtype == torch.int64
    case.check(n, y)
    if case.exact_n is not None:  # the property holds for the oracle itself, not only for what the reference chose
        assert all({m for m, _ in ok} == {e} for ok, e in zip(case.sets(), case.exact_n)), case.name


def test_few_cases_are_ambiguous():
    """At most 5 % of the (case, row) pairs may have more than one acceptable outcome: the oracle alone decides."""
    sets = [ok for c in CASES for ok in c.sets()]
    many = sum(len(ok) > 1 for ok in sets)
    assert many <= 0.05 * len(sets), (many, len(sets))


def test_random_fixtures_keep_residual_mass():
    for c in CASES:
        if c.name.startswith("random"):
            info: dict = {}
            c.sets(info)
            assert all(r >= R.R_MIN for r in info.get("R", [])), c.name


def test_philox_streams():
    for stream in (0, 1, 2):
        want = torch.from_numpy(R.uniform_stream(2**40 + 7, 2**33 + 5, 4, stream))
        assert torch.equal(S.philox_uniform(2**40 + 7, 2**33 + 5, 4, stream=stream), want)
    assert torch.equal(S.philox_uniform(9, 3, 4), S.philox_uniform(9, 3, 4, stream=0))
    assert not torch.equal(S.philox_uniform(9, 3, 4, stream=1), S.philox_uniform(9, 3, 4))


def test_step_reference_contract():
    """The torch twin of the in-graph form: the state the GPU contract test checks, on the CPU."""
    c = next(c for c in CASES if c.name == "random-V97-K4-B3-float32")
    B, K, seed, cnt = 3, 4, 77, 5
    ua = torch.stack([S.philox_uniform(seed, cnt + i, B, stream=1) for i in range(K)], 1)
    us = S.philox_uniform(seed, cnt, B, stream=2)
    n, y = S.spec_verify_reference(c.t, c.d, c.s, 1.0, ua, us)
    win = torch.cat([torch.full((B, 1), 96), c.d], 1)
    st = dict(ids=torch.zeros(B, 1, dtype=torch.long), out=torch.full((B, 12), -7), n_out=torch.tensor([2, 0, 3]),
              base=torch.tensor([10, 20, 30]), pt=torch.tensor([10, 20, 30]), pd=torch.tensor([15, 25, 30]),
              st=torch.tensor([1, 1, 0]), sd=torch.tensor([1, 1, 0]), done=torch.zeros(B, dtype=torch.int32))
    rng = torch.tensor([seed, cnt])
    S.spec_verify_step(c.t, c.s, 1.0, rng, win, st["ids"], st["out"], st["n_out"], st["base"], st["pt"], st["pd"],
                       st["st"], st["sd"], st["done"], -1)
    for b in range(2):
        m = int(n[b]) + 1
        o = [2, 0][b]
        assert st["out"][b, o : o + m].tolist() == c.d[b, : m - 1].tolist() + [int(y[b])]
        assert int(st["n_out"][b]) == o + m and int(win[b, 0]) == int(st["ids"][b, 0]) == int(y[b])
        assert int(st["pt"][b]) == int(st["pd"][b]) == [10, 20][b] + m
    assert st["out"][2].tolist() == [-7] * 12 and int(st["pd"][2]) == 30 and int(win[2, 0]) == 96  # idle
    assert rng.tolist() == [seed, cnt] and st["done"].tolist() == [0, 0, 0]


def _wrong_first_tokens(d, ua, us):
    """A verifier that draws the correction from p instead of the residual (numpy, K = 1)."""
    ok = ua * R.DIST_Q[d] < R.DIST_P[d]
    y = np.minimum(np.searchsorted(np.cumsum(R.DIST_P), us * R.DIST_P.sum(), side="right"), 7)
    return np.where(ok, d, y)


def test_distribution_on_the_cpu_reference():
    """20 000 rows, K = 1: the first emitted token is distributed as p within 5 sigma per token, and a verifier that
    draws the correction from p instead of the residual misses that bound by tens of sigma."""
    N, seed = 20000, 11
    t, s, (u0, ua, us) = R.dist_inputs(N, seed)
    d = S.sample_logits_reference(s[:, 0], 1.0, 0, 1.0, u0)
    n, y = S.spec_verify_reference(t, d[:, None], s, 1.0, ua[:, None], us)
    first = torch.where(n > 0, d, y)
    worst = R.dist_check(first.numpy(), N)
    print(f"first-token deviation: {worst:.2f} sigma")
    assert worst <= 5.0
    wrong = R.dist_check(_wrong_first_tokens(d.numpy(), ua.numpy().astype(np.float64), us.numpy().astype(np.float64)), N)
    print(f"correction drawn from p: {wrong:.1f} sigma")
    assert wrong >= 20.0
