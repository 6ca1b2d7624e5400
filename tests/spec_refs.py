"""fp64 numpy oracle of speculative verification (``bpe_transformer/ops/sampling.py``, ``ops/csrc/spec_verify.hip``),
written independently of ``ops/sampling.py``, plus the fixture builders of its tests.

For one sequence the oracle returns the set of *acceptable* ``(n, y)`` outcomes:

* an accept decision counts either way when ``|ua * q - p| <= DELTA * max(ua * q, p)`` (and that maximum is not 0),
  unless the two logits rows are the same numbers, where ``q == p`` under any rounding;
* the final draw from the residual ``r = max(p - q, 0)`` is acceptable when its cumulative interval, widened by
  ``DELTA`` in absolute probability mass, contains ``us * R`` -- the residual is a difference of two normalised
  rows, so its error is absolute, not relative to ``R``;
* the final draw from ``p`` (all drafts accepted, or ``R == 0``) is ``sample_refs.Oracle.acceptable``.

``DELTA`` and its derivation are those of ``tests/sample_refs.py``.
"""

from __future__ import annotations

import numpy as np
import torch

from .sample_refs import DELTA, Oracle, f64, philox4x32_10, random_rows, uniforms

R_MIN = 0.05  # the fixtures keep every reachable residual's mass above this


def softmax64(x: np.ndarray, T: float) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        z = np.exp((x - x.max()) / float(T))
    z[np.isneginf(x)] = 0.0
    return z / z.sum()


def argmax_low(x: np.ndarray) -> int:
    return int(np.nonzero(x == x.max())[0][0])


def residual_acceptable(p: np.ndarray, q: np.ndarray, us: float, delta: float = DELTA):
    """(acceptable tokens of the draw from max(p - q, 0), its mass R); R == 0: (None, 0)."""
    r = np.maximum(p - q, 0.0)
    R = float(r.sum())
    if R == 0.0:
        return None, 0.0
    tok = np.nonzero(r > 0)[0]
    hi = np.cumsum(r[tok])
    lo = hi - r[tok]
    t = float(us) * R
    j0 = int(np.searchsorted(hi, t - delta, side="left"))
    j1 = int(np.searchsorted(lo, t + delta, side="right")) - 1
    j0, j1 = min(j0, len(tok) - 1), max(j1, 0)
    return tok[j0 : j1 + 1], R


def outcomes(t: np.ndarray, d, s, T: float, ua=None, us: float = 0.5, delta: float = DELTA, info: dict | None = None):
    """Acceptable ``(n, y)`` of one sequence: ``t [K + 1, V]``, ``d [K]``, ``s [K, V]`` (fp64 values of the rounded
    logits).  ``info["R"]`` collects the residual mass of every reachable rejection."""
    K, V = t.shape[0] - 1, t.shape[1]
    d = [int(v) for v in d]
    if T <= 0:
        n = 0
        while n < K and d[n] == argmax_low(t[n]):
            n += 1
        return {(n, argmax_low(t[n]))}
    res = set()
    for n in range(K + 1):
        if n == K:  # all stand: the bonus token from p_{K+1}
            res |= {(K, int(y)) for y in Oracle(t[K], T).acceptable(us, delta)}
            break
        p, q = softmax64(t[n], T), softmax64(s[n], T)
        a, pv = float(ua[n]) * q[d[n]], p[d[n]]
        either = max(a, pv) > 0 and abs(a - pv) <= delta * max(a, pv)
        if np.array_equal(t[n], s[n]):  # the same row twice: q == p whatever the rounding, so ua < 1 decides exactly
            either = False
        if not (a < pv) or either:  # a rejection here is possible
            ys, R = residual_acceptable(p, q, us, delta)
            if info is not None:
                info.setdefault("R", []).append(R)
            if ys is None:
                ys = Oracle(t[n], T).acceptable(us, delta)
            res |= {(n, int(y)) for y in ys}
        if not (a < pv or either):
            break
    return res


def uniform_stream(seed: int, count: int, B: int, stream: int) -> np.ndarray:
    """fp32 ``[B]``: Philox key ``seed`` at counter (count, row, stream), ``((x0 >> 8) + 0.5) * 2^-24``."""
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    ctr = np.zeros((B, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = count & 0xFFFFFFFF, (count >> 32) & 0xFFFFFFFF, np.arange(B), stream
    x0 = philox4x32_10(np.broadcast_to(key, (B, 2)), ctr)[:, 0]
    return (((x0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0**-24).astype(np.float32)


# ---------------------------------------------------------------- the cases of the verification tests
class Case:
    """``t [B, K + 1, V]``, ``d [B, K]``, ``s [B, K, V]`` verified at temperature ``T`` with ``ua [B, K]``, ``us
    [B]``; ``exact_n``: the ``n`` every acceptable outcome of each row must have (a property of the case)."""

    def __init__(self, name, t, d, s, T, ua, us, exact_n=None):
        self.name, self.t, self.d, self.s, self.T = name, t, d, s, T
        self.ua = torch.as_tensor(ua, dtype=torch.float32).reshape(d.shape)
        self.us = torch.as_tensor(us, dtype=torch.float32).reshape(-1)
        self.exact_n = exact_n
        self._sets = None

    def sets(self, info=None) -> list[set]:
        if self._sets is None or info is not None:
            t, s = f64(self.t), f64(self.s)
            self._sets = [outcomes(t[b], self.d[b].tolist(), s[b], self.T, self.ua[b].tolist(), float(self.us[b]),
                                   info=info) for b in range(t.shape[0])]
        return self._sets

    def check(self, n, y) -> None:
        got = list(zip((int(v) for v in n.reshape(-1).tolist()), (int(v) for v in y.reshape(-1).tolist())))
        for b, (g, ok) in enumerate(zip(got, self.sets())):
            assert g in ok, f"{self.name} row {b}: {g} not among {sorted(ok)[:6]}"
            if self.exact_n is not None:
                assert g[0] == self.exact_n[b], (self.name, b, g, self.exact_n)


def settle(c: Case, seed: int) -> Case:
    """Replace the ``us`` of every row whose final draw is ambiguous (a full-vocabulary row has thousands of tokens
    lighter than DELTA) by the first of 32 further uniforms that the oracle finds unambiguous, if any."""
    if c.T <= 0:
        return c
    t, s = f64(c.t), f64(c.s)
    for b in range(t.shape[0]):
        for u in [float(c.us[b]), *uniforms(seed + b, 32).tolist()]:
            if len(outcomes(t[b], c.d[b].tolist(), s[b], c.T, c.ua[b].tolist(), u)) == 1:
                c.us[b] = u
                break
    c._sets = None
    return c


def _name(kind, V, K, B, dtype):
    return f"{kind}-V{V}-K{K}-B{B}-{str(dtype)[6:]}"


def related_rows(seed: int, B: int, K: int, V: int, dtype, noise: float = 1.0):
    """Draft rows ``s`` (sigma 4), target rows ``t[:, :K] = s + noise * N(0, 1)`` and an unrelated ``t[:, K]``,
    draft tokens drawn from ``softmax(s)``."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, K, V, generator=g) * 4.0
    t = torch.cat([s + noise * torch.randn(B, K, V, generator=g), torch.randn(B, 1, V, generator=g) * 4.0], 1)
    s, t = s.to(dtype), t.to(dtype)
    d = torch.multinomial(torch.softmax(s.float().reshape(B * K, V), -1), 1, generator=g).reshape(B, K)
    return t, d, s


def random_case(V, K, B, dtype, T=1.0) -> Case:
    """The first seed whose reachable residuals all have mass >= R_MIN (decided by the oracle alone)."""
    for seed in range(V * 31 + K * 7 + B, V * 31 + K * 7 + B + 64):
        t, d, s = related_rows(seed, B, K, V, dtype)
        c = settle(Case(_name("random", V, K, B, dtype), t, d, s, T, uniforms(seed + 1, B * K),
                        uniforms(seed + 2, B)), seed + 3)
        info: dict = {}
        c.sets(info)
        if all(R >= R_MIN for R in info.get("R", [])):
            return c
    raise AssertionError("no seed keeps the residual mass above R_MIN")


def all_cases() -> list[Case]:
    """Every case the GPU kernel is tested on (tests/test_spec_verify_gpu.py); tests/test_spec_refs.py runs the
    torch reference over the same list and bounds how many are ambiguous."""
    cases: list[Case] = []
    dtypes = (torch.bfloat16, torch.float32)
    for V in (1, 8, 97, 1000, 50257):
        for K in (1, 4, 7):
            for B in (1, 3):
                for dtype in dtypes:
                    c = random_case(V, K, B, dtype)
                    cases.append(c)
                    cases.append(Case(_name("greedy", V, K, B, dtype), c.t, c.t[:, :K].float().argmax(-1) if K % 2
                                      else c.d, c.s, 0.0, c.ua, c.us))
    V, K = 50257, 4
    for dtype in dtypes:
        # greedy ties at the maximum on either side of a vector (8), wave-tile (256) and block (8192) boundary:
        # the lowest index wins, so d = a stands and d = b does not
        for a, b in ((7, 8), (255, 256), (8191, 8192)):
            t = random_rows(a, 2 * (K + 1), V, dtype).reshape(2, K + 1, V).clone()
            t[:, :, a], t[:, :, b] = 30.0, 30.0
            d = torch.tensor([[a, a, b, a], [a, a, a, a]])
            cases.append(Case(f"greedy-tie-{a}-{b}-{str(dtype)[6:]}", t, d, t[:, :K], 0.0, torch.zeros(2, K),
                              torch.zeros(2), exact_n=[2, 4]))
        for V2 in (97, V):
            t, d, s = related_rows(V2 + 5, 3, K, V2, dtype)
            d = s.float().argmax(-1)  # the draft's likeliest tokens: what a rejection leaves has mass
            ua, us = uniforms(V2, 3 * K).reshape(3, K), uniforms(V2 + 1, 3)
            # a draft token the target gives no mass (-inf): rejected whatever ua -- at draft 3, 1 and 2
            t0 = t.clone()
            for b, i in enumerate((2, 0, 1)):
                t0[b, i, d[b, i]] = -torch.inf
            ua0 = ua.clone().fill_(2.0**-25)
            cases.append(settle(Case(_name("p-zero", V2, K, 3, dtype), t0, d, s, 1.0, ua0, us.clone(),
                                     exact_n=[2, 0, 1]), V2))
            # q == p exactly: every draft stands (ua < 1) and the bonus token is drawn from p_{K+1}
            te = torch.cat([s, t[:, K:]], 1)
            cases.append(settle(Case(_name("q-is-p", V2, K, 3, dtype), te, d, s, 1.0,
                                     ua.clone().fill_(1 - 2.0**-24), us.clone(), exact_n=[K] * 3), V2))
            # rejection at draft 1: the target likes d_1 e^-12 times as much as the draft does
            t1 = torch.cat([s, t[:, K:]], 1).clone()
            for b in range(3):
                t1[b, 0, d[b, 0]] -= 12.0
            cases.append(settle(Case(_name("reject-first", V2, K, 3, dtype), t1, d, s, 1.0, ua.clone().fill_(0.5),
                                     us.clone(), exact_n=[0] * 3), V2))
            # ua 2 * DELTA inside either side of the accept boundary p / q of draft 1 (a token with p < q)
            t2 = torch.cat([s, t[:, K:]], 1).clone()
            for b in range(3):
                t2[b, 0, d[b, 0]] -= 1.0
            p = [softmax64(f64(t2)[b, 0], 1.0)[d[b, 0]] / softmax64(f64(s)[b, 0], 1.0)[d[b, 0]] for b in range(3)]
            for side, sign in (("in", -1), ("out", 1)):
                ue = ua.clone().fill_(2.0**-25)
                for b in range(3):
                    ue[b, 0] = p[b] * (1 + sign * 2 * DELTA)
                cases.append(settle(Case(_name(f"edge-{side}", V2, K, 3, dtype), t2, d, s, 1.0, ue, us.clone(),
                                         exact_n=[K] * 3 if sign < 0 else [0] * 3), V2))
    return cases


# ---------------------------------------------------------------- the distribution test
DIST_P = np.array([0.30, 0.05, 0.20, 0.05, 0.10, 0.02, 0.08, 0.20])
DIST_Q = np.array([0.05, 0.30, 0.05, 0.25, 0.05, 0.20, 0.05, 0.05])
assert 0.5 * np.abs(DIST_P - DIST_Q).sum() >= 0.3  # total variation 0.6


def dist_inputs(N: int, seed: int):
    """K = 1, V = 8, ``N`` rows: target rows ``log p`` / a bonus row, draft rows ``log q`` (fp32), and the Philox
    uniforms of streams 0 (the draft's own draw), 1 (accept) and 2 (final) at counter 0."""
    t = torch.tensor(np.log(np.stack([DIST_P, DIST_P])), dtype=torch.float32).repeat(N, 1, 1)
    s = torch.tensor(np.log(DIST_Q), dtype=torch.float32).reshape(1, 1, 8).repeat(N, 1, 1)
    u = [torch.from_numpy(uniform_stream(seed, 0, N, st)) for st in (0, 1, 2)]
    return t, s, u


def dist_check(first_tokens, N: int) -> float:
    """``|count_i - N p_i| <= 5 sqrt(N p_i (1 - p_i))`` for every i; returns the largest deviation in sigmas."""
    cnt = np.bincount(np.asarray(first_tokens, dtype=np.int64), minlength=8).astype(np.float64)
    sig = np.abs(cnt - N * DIST_P) / np.sqrt(N * DIST_P * (1 - DIST_P))
    return float(sig.max())
