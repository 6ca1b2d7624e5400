"""Fixtures of the point-mass verification tests (``spec_verify(..., point_mass=True)``), shared by the CPU and the
GPU test files: the sampling cases of ``tests/spec_refs.py`` with their one-hot draft logits, a peaked fixture in
which drafts both stand and fall, and the inputs of the distribution test."""

from __future__ import annotations

import functools

import numpy as np
import torch

from . import spec_refs as R


@functools.lru_cache(maxsize=1)
def sampling_cases() -> list:
    """Every sampling case of ``spec_refs.all_cases()`` (all of their drafts lie inside the vocabulary)."""
    return [c for c in R.all_cases() if c.T > 0]


def onehot(d: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """Draft logits ``[B, K, V]`` of ``t``'s dtype that put all mass on ``d``: 0 there, -inf elsewhere (all -inf for
    a ``d`` outside the vocabulary)."""
    B, K = d.shape
    V = t.shape[2]
    s = torch.full((B, K, V), -torch.inf, dtype=t.dtype)
    ok = (d >= 0) & (d < V)
    s.scatter_(2, d.clamp(0, V - 1)[..., None], torch.where(ok, 0.0, -torch.inf).to(t.dtype)[..., None])
    return s


def peaked_fixture(V: int = 97, K: int = 3, dtype=torch.float32):
    """``(t [3, K + 1, V], d [3, K], ua, us)``: row 0 drafts the argmax of rows peaked by +12 (p > 0.99: stands at
    ua = 0.5), row 1 drafts its first row's least likely token (p < 1 / V: falls at ua = 0.5), row 2 drafts a token
    outside the vocabulary."""
    g = torch.Generator().manual_seed(3)
    t = torch.randn(3, K + 1, V, generator=g)
    peak = torch.randint(0, V, (K,), generator=g)
    t[0, torch.arange(K), peak] += 12.0
    t = t.to(dtype)
    d = t[:, :K].float().argmax(-1)
    d[1, 0] = t[1, 0].float().argmin()
    d[2, 0] = V + 3
    return t, d, torch.full((3, K), 0.5), torch.tensor([0.3, 0.6, 0.9])


def dist_first_tokens(N: int, seed: int):
    """K = 1, V = 8, ``N`` rows of the distribution test of ``spec_refs``: target rows ``log p``, the deterministic
    draft ``d[b] = b mod 8``, and the Philox uniforms of streams 1 (accept) and 2 (final) at counter 0.  Whatever
    ``d`` is, the first emitted token is distributed as ``p``: ``p(d) [x = d] + (1 - p(d)) p(x) / (1 - p(d)) [x !=
    d]``."""
    t = torch.tensor(np.log(np.stack([R.DIST_P, R.DIST_P])), dtype=torch.float32).repeat(N, 1, 1)
    d = torch.arange(N) % 8
    ua, us = (torch.from_numpy(R.uniform_stream(seed, 0, N, st)) for st in (1, 2))
    return t, d, ua, us
