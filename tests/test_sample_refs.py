"""The sampling oracle (``tests/sample_refs.py``) checked on the CPU: Philox against its published vectors, the
oracle against brute force, ``ops.sampling``'s torch reference against the oracle on every fixture of the GPU tests,
and the conditions the fixtures themselves promise."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from bpe_transformer.ops import sampling as S

from . import sample_refs as SR

# Random123 known-answer vectors for philox4x32_10: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(v) for v in SR.philox4x32_10(key, ctr)) == want
    assert S.philox4x32(key, ctr) == want


def test_philox_uniform_agrees_and_is_open():
    for seed, count in [(0, 0), (7, 3), (2**40 + 5, 2**33 + 1), (2**62 - 1, 17)]:
        a, b = SR.philox_uniform(seed, count, 5), S.philox_uniform(seed, count, 5).numpy()
        assert a.dtype == np.float32 and np.array_equal(a, b)
        assert (a > 0).all() and (a <= 1).all()
    x0 = SR.philox4x32_10((7, 0), (3, 0, 2, 0))[0]
    assert SR.philox_uniform(7, 3, 3)[2] == np.float32((float(x0 >> 8) + 0.5) * 2.0**-24)


def _brute(x, T, k, p, u):
    """The specification, literally: sort, walk, cumulate (python floats are fp64)."""
    V = len(x)
    rank = sorted(range(V), key=lambda i: (-x[i], i))
    if T <= 0:
        return {rank[0]}, rank[0]
    mx = max(x)
    z = [0.0 if x[i] == -np.inf else float(np.exp((x[i] - mx) / T)) for i in range(V)]
    kept = rank[: min(k, V)] if k > 0 else list(rank)
    if p < 1.0:
        Z, before, out = sum(z[i] for i in kept), 0.0, []
        for j, i in enumerate(kept):
            if j == 0 or before < p * Z:
                out.append(i)
            before += z[i]
        kept = out
    ks = set(kept)
    M, cum = sum(z[i] for i in sorted(ks)), 0.0
    for i in sorted(ks):
        cum += z[i]
        if z[i] > 0 and cum > u * M:
            return ks, i
    return ks, max(i for i in ks if z[i] > 0)


@pytest.mark.parametrize("V", [1, 2, 7, 33, 64])
def test_oracle_matches_brute_force(V):
    rng = np.random.default_rng(V)
    for trial in range(40):
        x = np.round(rng.normal(0, 2, V) * 4) / 4  # a coarse grid: plenty of ties
        if trial % 5 == 0 and V > 2:
            x[rng.integers(0, V, 2)] = -np.inf
            x[rng.integers(0, V)] = 1.0
        T = [0.0, 1.0, 0.7, 0.01][trial % 4]
        k = [0, 1, 3, V, V + 5][trial % 5]
        p = [1.0, 0.9, 0.31, 1e-6][trial % 4 if trial % 3 else 0]
        o = SR.Oracle(x, T, k, p)
        for u in rng.random(6):
            ks, tok = _brute(list(x), T, k, p, u)
            assert set(np.nonzero(o.kept)[0].tolist()) == ks
            assert tok in o.acceptable(u, delta=0.0)
            assert tok in o.acceptable(u)


CASES = SR.all_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_torch_reference_matches_oracle(case):
    """``sample_logits_reference`` on every case of the GPU test (the oracle's acceptable set, or the exact token)."""
    tok = S.sample_logits_reference(case.logits, case.temperature, case.top_k, case.top_p, case.u)
    case.check(tok)
    if case.logits.shape[1] <= 4099:  # (the CPU dispatch of the public op is the same function)
        assert torch.equal(S.sample_logits(case.logits, case.temperature, case.top_k, case.top_p, case.u), tok)


@pytest.fixture(scope="module")
def vocab_rows():
    return SR.random_rows(SR.VOCAB_SEED, 2, SR.VOCAB)


@pytest.mark.parametrize("T", [1.0, 0.7])
def test_random_rows_are_mostly_unambiguous(vocab_rows, T):
    """Random-row fixture (bf16, N(0, 4^2), V = 50257, 64 uniforms per row): at most 20 % of the cases may have more
    than one acceptable token (15 % and 4 % measured for one seed; about 40 % at sigma = 3)."""
    us = SR.uniforms(3, 64).tolist()
    multi = total = 0
    for b in range(vocab_rows.shape[0]):
        o = SR.Oracle(SR.f64(vocab_rows)[b], T)
        for u in us:
            multi += len(o.acceptable(u)) > 1
            total += 1
    assert multi / total <= 0.20, multi / total


def test_top_p_fixture_is_clear_of_rounding(vocab_rows):
    x = SR.f64(vocab_rows)[0]
    for n in (0, 1, 5):
        p, pr = SR.top_p_mid(x, 0.8, n)
        assert pr >= 20 * SR.DELTA
        assert int(SR.Oracle(x, 0.8, 0, p).kept.sum()) == n + 1


def test_sample_step_reference_contract():
    x = SR.random_rows(2, 4, 97, torch.float32)
    rng = torch.tensor([12345, 2])
    ids, out = torch.zeros(4, 1, dtype=torch.long), torch.full((4, 6), -7, dtype=torch.long)
    u = S.philox_uniform(12345, 2, 4)
    tok = S.sample_logits_reference(x, 0.9, 10, 0.9, u)
    done, step = torch.tensor([0, 1, 0, 0], dtype=torch.int32), torch.tensor([1, 1, 0, 1], dtype=torch.int32)
    S.sample_step(x, 0.9, 10, 0.9, rng, ids, out, step, done, int(tok[3]))
    assert torch.equal(ids[:, 0], tok) and rng.tolist() == [12345, 2]
    assert out[:, 2].tolist() == [int(tok[0]), -1, -1, int(tok[3])]
    assert (out[:, [0, 1, 3, 4, 5]] == -7).all()
    assert done[3] == 1 and step[3] == 0 and done[1] == 1 and step[2] == 0
