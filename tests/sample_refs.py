"""fp64 numpy oracle of the sampling function (``bpe_transformer/ops/sampling.py``, ``ops/csrc/sample.hip``),
written independently of ``ops/sampling.py``, plus a numpy Philox4x32-10 and the fixture builders of the sampling
tests.

The oracle reads the same rounded bf16 / fp32 logits as the code under test (``f64``), computes the kept set in
fp64, and for a uniform ``u`` returns the set of *acceptable* tokens: every kept token with mass whose fp64 interval
``[cum_{t-1}, cum_t]`` of the cumulative kept mass (index order), widened by ``DELTA * M`` on both sides, contains
``u * M``.

``DELTA = 1e-4``: a kernel that sums fp32 in per-thread strips of ``V / 256`` and then a tree has a worst-case
relative error of about ``(V / 256 + 16) * 2^-24 ~ 1.3e-5`` at ``V = 50257``; a fast ``exp`` adds about ``1e-6``;
``1e-4`` leaves roughly 8x.
"""

from __future__ import annotations

import numpy as np
import torch

DELTA = 1e-4
VOCAB, VOCAB_SEED = 50257, 12  # the random full-vocabulary rows of the fixtures: random_rows(VOCAB_SEED, 2, VOCAB)


def f64(logits: torch.Tensor) -> np.ndarray:
    """The logits as the kernels see them (bf16 / fp32 values), exactly, in fp64."""
    return logits.detach().cpu().double().numpy()


# ---------------------------------------------------------------- Philox4x32-10 (numpy, uint64 lanes)
def philox4x32_10(key, counter) -> np.ndarray:
    """``key [..., 2]``, ``counter [..., 4]`` (uint32 values) -> ``[..., 4]`` uint32."""
    m = np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64)
    c = np.asarray(counter, dtype=np.uint64)
    k0, k1 = k[..., 0], k[..., 1]
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def philox_uniform(seed: int, count: int, B: int) -> np.ndarray:
    """fp32 ``[B]``: key (seed_lo, seed_hi), counter (count_lo, count_hi, row, 0), ``((x0 >> 8) + 0.5) * 2^-24``."""
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    ctr = np.array([[count & 0xFFFFFFFF, (count >> 32) & 0xFFFFFFFF, b, 0] for b in range(B)], dtype=np.uint64)
    x0 = philox4x32_10(np.broadcast_to(key, (B, 2)), ctr)[:, 0]
    return (((x0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0**-24).astype(np.float32)


# ---------------------------------------------------------------- the oracle
class Oracle:
    """One row ``x [V]`` (fp64 values of the rounded logits) under one parameter set."""

    def __init__(self, x: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0):
        x = np.asarray(x, dtype=np.float64)
        V = x.shape[0]
        self.V, self.greedy = V, temperature <= 0
        idx = np.arange(V)
        self.order = np.lexsort((idx, -x))  # rank order: descending x, ascending index among equal x
        if self.greedy:
            self.kept = np.zeros(V, dtype=bool)
            self.kept[self.order[0]] = True
            return
        with np.errstate(invalid="ignore"):
            z = np.exp((x - x.max()) / float(temperature))
        z[np.isneginf(x)] = 0.0
        self.z = z
        zs = z[self.order]
        keep = np.ones(V, dtype=bool)
        if top_k > 0:
            keep &= idx < min(int(top_k), V)
        if top_p < 1.0:
            zk = zs * keep
            before = np.cumsum(zk) - zk
            keep &= before < float(top_p) * zk.sum()
            keep[0] = True
        self.kept = np.zeros(V, dtype=bool)
        self.kept[self.order[keep]] = True
        zk = z * self.kept
        self.tok = np.nonzero(zk > 0)[0]  # kept tokens with mass, by index
        self.hi = np.cumsum(zk[self.tok])
        self.lo = self.hi - zk[self.tok]
        self.M = float(self.hi[-1])

    def acceptable(self, u: float, delta: float = DELTA) -> np.ndarray:
        """Token ids the draw may return for ``u``."""
        if self.greedy:
            return self.order[:1]
        t, w = float(u) * self.M, delta * self.M
        j0 = int(np.searchsorted(self.hi, t - w, side="left"))
        j1 = int(np.searchsorted(self.lo, t + w, side="right")) - 1
        j0, j1 = min(j0, len(self.tok) - 1), max(j1, 0)
        return self.tok[j0 : j1 + 1]

    def prob(self, t: int) -> float:
        return float(self.z[t] * self.kept[t] / self.M)


def check_tokens(logits: torch.Tensor, tokens, temperature, top_k, top_p, u, oracles=None) -> list:
    """Every ``tokens[b]`` must be acceptable for row ``b``; returns the oracles (to reuse for the same rows)."""
    x = f64(logits)
    toks = [int(t) for t in torch.as_tensor(tokens).reshape(-1).tolist()]
    us = [float(v) for v in torch.as_tensor(u).reshape(-1).tolist()]
    assert len(toks) == x.shape[0]
    oracles = oracles or [Oracle(x[b], temperature, top_k, top_p) for b in range(x.shape[0])]
    for b, (t, o) in enumerate(zip(toks, oracles)):
        ok = o.acceptable(us[b])
        assert t in ok, f"row {b}: token {t} not acceptable for u={us[b]!r}: {ok.tolist()[:8]} (T={temperature}, " \
                        f"top_k={top_k}, top_p={top_p})"
    return oracles


# ---------------------------------------------------------------- fixtures
def random_rows(seed: int, B: int, V: int, dtype=torch.bfloat16, sigma: float = 4.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * sigma).to(dtype)


def uniforms(seed: int, n: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g).clamp_(2.0**-25, 1 - 2.0**-24)


def top_p_mid(x: np.ndarray, temperature: float, n: int, top_k: int = 0) -> tuple[float, float]:
    """``top_p`` in the middle of the mass of the ``n``-th ranked token (0-based) of what ``top_k`` keeps, and that
    token's probability there: with it ``>= 20 * DELTA`` the kept set is the same in fp32 and fp64."""
    o = Oracle(x, temperature, top_k, 1.0)
    zs = (o.z * o.kept)[o.order]
    before = np.cumsum(zs) - zs
    return float((before[n] + 0.5 * zs[n]) / o.M), float(zs[n] / o.M)


def hot_row(V: int, dtype=torch.bfloat16):
    """Hot tokens at indices 0, 255, 256, V/2 and V-1 (those that exist, once each), the rest at -40: the draw is
    exact.  Returns (logits [1, V], hot indices ascending)."""
    hot = sorted({i for i in (0, 255, 256, V // 2, V - 1) if 0 <= i < V})
    x = torch.full((1, V), -40.0)
    for j, i in enumerate(hot):
        x[0, i] = 3.0 - 0.5 * j
    return x.to(dtype), hot


def edge_uniforms(o: Oracle, t: int, delta: float = DELTA) -> list[float]:
    """``u`` at the middle of token ``t``'s interval and ``2 * delta`` inside each of its edges."""
    j = int(np.nonzero(o.tok == t)[0][0])
    lo, hi = o.lo[j] / o.M, o.hi[j] / o.M
    return [0.5 * (lo + hi), lo + 2 * delta, hi - 2 * delta]


# ---------------------------------------------------------------- the cases of the sampling tests
class Case:
    """``logits [B, V]`` sampled with ``u [B]``; ``exact``: the one token each row must return (else: the oracle's
    acceptable set); ``same_row``: all rows are copies of row 0 (one oracle serves them)."""

    def __init__(self, name, logits, temperature, top_k, top_p, u, exact=None, same_row=False):
        self.name, self.logits, self.temperature, self.top_k, self.top_p = name, logits, temperature, top_k, top_p
        self.u = torch.as_tensor(u, dtype=torch.float32).reshape(-1)
        self.exact, self.same_row = exact, same_row
        assert self.u.numel() == logits.shape[0]

    def check(self, tokens) -> None:
        toks = [int(t) for t in torch.as_tensor(tokens).reshape(-1).tolist()]
        assert all(0 <= t < self.logits.shape[1] for t in toks), toks
        if self.exact is not None:
            assert toks == [int(t) for t in self.exact], (self.name, toks, self.exact)
            return
        oracles = None
        if self.same_row:
            oracles = [Oracle(f64(self.logits[:1])[0], self.temperature, self.top_k, self.top_p)] * len(toks)
        check_tokens(self.logits, toks, self.temperature, self.top_k, self.top_p, self.u, oracles)


def _name(kind, V, B, dtype):
    return f"{kind}-V{V}-B{B}-{str(dtype)[6:]}"


def _run_row(V: int, dtype) -> tuple[torch.Tensor, list[int]]:
    """10 and 9 on top, then a run of four equal 8s spread over the row, the rest N(0, 1) clipped to <= 5."""
    x = random_rows(V + 3, 1, V, torch.float32, sigma=1.0).clamp_(max=5.0)
    run = [V // 40, V // 7, V // 2 + 1, V - 2]
    x[0, 0], x[0, 1] = 10.0, 9.0
    for i in run:
        x[0, i] = 8.0
    return x.to(dtype), run


def all_cases() -> list[Case]:
    """Every case the GPU kernel is tested on (tests/test_sampling_gpu.py); tests/test_sample_refs.py runs the torch
    reference over the same list."""
    cases: list[Case] = []
    dtypes = (torch.bfloat16, torch.float32)
    for V in (1, 7, 64, 255, 257, 4099, VOCAB):
        for dtype in dtypes:
            for B in (1, 3):
                x = random_rows(V * 7 + B, B, V, dtype)
                u = uniforms(V + B, B)
                cases.append(Case(_name("plain", V, B, dtype), x, 1.0, 0, 1.0, u))
                cases.append(Case(_name("greedy", V, B, dtype), x, 0.0, 0, 1.0, u))
                cases.append(Case(_name("topk5", V, B, dtype), x, 0.8, min(5, V), 1.0, u))
                cases.append(Case(_name("topk-all", V, B, dtype), x, 0.8, V + 3, 1.0, u))
                amax = [Oracle(r, 0.0).order[0] for r in f64(x)]
                cases.append(Case(_name("topk1", V, B, dtype), x, 0.8, 1, 1.0, u, exact=amax))
                cases.append(Case(_name("topp-tiny", V, B, dtype), x, 0.8, 0, 1e-6, u, exact=amax))
                cases.append(Case(_name("cold", V, B, dtype), x, 0.01, 0, 1.0, u))
                if V >= 7:  # top-p in the middle of the third-ranked token's mass; the rows are copies of row 0
                    xr = x[:1].repeat(B, 1)
                    for k in (0, 5):
                        # (the lowest-ranked of the first three tokens that is likely enough)
                        p, pr = next(r for r in (top_p_mid(f64(xr)[0], 0.8, n, k) for n in (2, 1, 0))
                                     if r[1] >= 20 * DELTA)
                        cases.append(Case(_name(f"topp-mid-k{k}", V, B, dtype), xr, 0.8, k, p, u, same_row=True))
    for dtype in dtypes:
        # greedy ties at the maximum on either side of a vector (8), wave-tile (256 / 512) and block (8192) boundary
        for a, b in ((7, 8), (255, 256), (511, 512), (8191, 8192), (3, VOCAB - 1)):
            x = random_rows(a, 2, VOCAB, dtype)
            x[:, a], x[:, b] = 30.0, 30.0
            cases.append(Case(f"greedy-tie-{a}-{b}-{str(dtype)[6:]}", x, 0.0, 0, 1.0, [0.5, 0.5], exact=[a, a]))
        for V in (4099, VOCAB):
            x, run = _run_row(V, dtype)
            us = uniforms(V, 8)
            xr = x.repeat(8, 1)
            # top-k cuts the run of four after its second member (by index); top-p does, alone and under a top-k
            cases.append(Case(_name("run-topk4", V, 8, dtype), xr, 1.0, 4, 1.0, us, same_row=True))
            p, pr = top_p_mid(f64(x)[0], 1.0, 3)
            assert pr >= 20 * DELTA
            cases.append(Case(_name("run-topp", V, 8, dtype), xr, 1.0, 0, p, us, same_row=True))
            p, pr = top_p_mid(f64(x)[0], 1.0, 3, 5)
            cases.append(Case(_name("run-topk5-topp", V, 8, dtype), xr, 1.0, 5, p, us, same_row=True))
            # ... and the draw at the far end of the kept run members
            cases.append(Case(_name("run-topk4-ends", V, 2, dtype), x.repeat(2, 1), 1.0, 4, 1.0, [2.0**-25, 1.0],
                              exact=[0, run[1]]))
        for V in (7, 64, 257, 4099, VOCAB):
            x, hot = hot_row(V, dtype)
            o = Oracle(f64(x)[0], 1.0)
            us, want = [], []
            for t in hot:
                us += edge_uniforms(o, t)
                want += [t] * 3
            cases.append(Case(_name("hot", V, len(us), dtype), x.repeat(len(us), 1), 1.0, 0, 1.0, us, exact=want))
            # u = 2^-25 and u = 1 - 2^-25 (which fp32 rounds to 1): the first and the last kept index
            ends = [2.0**-25, 1 - 2.0**-25]
            cases.append(Case(_name("hot-ends", V, 2, dtype), x.repeat(2, 1), 1.0, 0, 1.0, ends,
                              exact=[hot[0], hot[-1]]))
            if len(hot) >= 4:
                cases.append(Case(_name("hot-ends-k3", V, 2, dtype), x.repeat(2, 1), 1.0, 3, 1.0, ends,
                                  exact=[min(hot[:3]), max(hot[:3])]))
        for V in (64, 4099, VOCAB):
            x = random_rows(V + 1, 3, V, dtype)
            x[torch.rand(3, V, generator=torch.Generator().manual_seed(V)) < 0.3] = -torch.inf
            x[:, V // 2] = 1.0
            u = uniforms(V + 2, 3)
            cases.append(Case(_name("inf", V, 3, dtype), x, 1.0, 0, 1.0, u))
            cases.append(Case(_name("inf-topk", V, 3, dtype), x, 1.0, V - 1, 1.0, u))
            cases.append(Case(_name("inf-topp", V, 3, dtype), x, 1.0, 0, 0.999, u))
            lone = torch.full((3, V), -torch.inf).to(dtype)
            lone[0, V - 1], lone[1, 0], lone[2, V // 3] = 2.0, -3.0, 0.0
            for k, p in ((0, 1.0), (3, 1.0), (0, 0.5), (V, 0.9)):
                cases.append(Case(_name(f"lone-k{k}-p{p}", V, 3, dtype), lone, 0.7, k, p, u, exact=[V - 1, 0, V // 3]))
    # fp32 logits of magnitude 3e4
    x = random_rows(9, 3, 4099, torch.float32, sigma=3e4)
    for T in (1.0, 5000.0):
        cases.append(Case(f"big-T{T}", x, T, 0, 1.0, uniforms(9, 3)))
        cases.append(Case(f"big-topk-T{T}", x, T, 40, 1.0, uniforms(9, 3)))
    # the random full-vocabulary rows, 64 uniforms each
    rows = random_rows(VOCAB_SEED, 2, VOCAB)
    us = uniforms(3, 64)
    for b in range(2):
        for T in (1.0, 0.7):
            cases.append(Case(f"random-row{b}-T{T}", rows[b : b + 1].repeat(64, 1), T, 0, 1.0, us, same_row=True))
    return cases
