"""fp64 numpy oracle of ``min_p`` and of the per-row rules of ``sample_rows`` (``bpe_transformer/ops/sampling.py``,
"Per-row forms"; ``ops/csrc/sample_rows.hip``), written independently of ``ops/sampling.py`` on top of the oracle of
``tests/sample_refs.py``, plus the fixture builders of the per-row tests.

``min_p``: of what top-k and top-p keep, a token stays iff ``z_i >= min_p * max z`` (``max z = 1``); the argmax always
stays.  The kernel decides on fp32 ``exp`` values floored to 2^-40, the oracle in fp64, so a case is only fair if no
token's mass lies near the threshold: ``MinPOracle.margin`` is the smallest relative distance ``|z_i - min_p| /
min_p`` over the row, and the fixtures (``min_p_mid``) keep it above ``MARGIN = 1e-3`` -- three orders of magnitude
above the fp32 ``exp``'s ~1e-6 relative error and the 2^-40 floor.  The tests assert that margin, so no case needs
leaving out.
"""

from __future__ import annotations

import numpy as np
import torch

from . import sample_refs as SR

MARGIN = 1e-3
VS = (1, 7, 257, 1000, 50257)
MODES = ("greedy", "temperature", "top_k", "top_p", "all_min_p")


class MinPOracle(SR.Oracle):
    """``sample_refs.Oracle`` with the min-p filter applied to its kept set."""

    def __init__(self, x, temperature, top_k=0, top_p=1.0, min_p=0.0):
        super().__init__(x, temperature, top_k, top_p)
        self.min_p = float(np.float32(min_p))
        self.margin = np.inf
        if self.greedy or not self.min_p > 0:
            return
        z = self.z
        pos = z > 0
        self.margin = float(np.min(np.abs(z[pos] - self.min_p)) / self.min_p)
        keep = z >= self.min_p * z.max()
        keep[self.order[0]] = True
        self.kept = self.kept & keep
        zk = z * self.kept
        self.tok = np.nonzero(zk > 0)[0]
        self.hi = np.cumsum(zk[self.tok])
        self.lo = self.hi - zk[self.tok]
        self.M = float(self.hi[-1])


def min_p_mid(x: np.ndarray, temperature: float, n: int) -> float:
    """A ``min_p`` (an fp32 value) that keeps at least the ``n + 1`` highest-mass tokens of the row and sits in the
    geometric middle of the first gap below them whose ratio exceeds ``1 + 4 * MARGIN``; 0.5 where the row has no
    such gap (every token then has mass 1 or lies far below)."""
    o = SR.Oracle(x, temperature)
    z = np.unique(o.z[o.z > 0])[::-1]  # distinct masses, descending
    for i in range(min(n, len(z) - 1), len(z) - 1):
        if z[i] / z[i + 1] > 1 + 4 * MARGIN:
            return float(np.float32(np.sqrt(z[i] * z[i + 1])))
    return 0.5


def rows_case(V: int, dtype, seed: int = 0):
    """Five rows ``[5, V]``, one sampling mode each (``MODES``), and their parameter dicts.  The top-k row has equal
    logits on both sides of its cut, the top-p row a run of equal logits that its cut falls into."""
    x = SR.random_rows(100 + seed + V, 5, V, dtype).float()
    k = max(1, min(5, V - 1))
    order = np.lexsort((np.arange(V), -x[2].double().numpy()))
    if V > k:  # ranks k-1 and k (0-based) equal: the k-th place is a tie
        x[2, order[k]] = x[2, order[k - 1]]
    order = np.lexsort((np.arange(V), -x[3].double().numpy()))
    if V >= 5:  # ranks 1..3 equal: top_p cuts inside the run
        x[3, order[2]] = x[3, order[1]]
        x[3, order[3]] = x[3, order[1]]
    x = x.to(dtype)
    xs = SR.f64(x)
    top_p3, _ = SR.top_p_mid(xs[3], 0.9, min(2, V - 1))
    k4 = max(1, min(40, V))
    top_p4, _ = SR.top_p_mid(xs[4], 1.3, min(6, k4 - 1), k4)
    params = [
        dict(temperature=0.0),
        dict(temperature=0.7),
        dict(temperature=1.1, top_k=k),
        dict(temperature=0.9, top_p=top_p3),
        dict(temperature=1.3, top_k=k4, top_p=top_p4, min_p=min_p_mid(xs[4], 1.3, min(2, V - 1))),
    ]
    return x, params


def oracle_of(xrow: np.ndarray, p: dict) -> MinPOracle:
    return MinPOracle(xrow, p.get("temperature", 1.0), int(p.get("top_k") or 0),
                      1.0 if p.get("top_p") is None else p["top_p"], p.get("min_p", 0.0))


def step_rules(tok: int, count: int, limit: int, eos: int, done: int, step: int):
    """The per-row rules after the draw: ``(writes, count, done, step)``."""
    if done != 0 or step == 0:
        return False, count, done, step
    count += 1
    if (eos >= 0 and tok == eos) or count >= limit:
        return True, count, 1, 0
    return True, count, 0, 1
