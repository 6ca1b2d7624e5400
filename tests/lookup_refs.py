"""Brute-force oracle of the prompt-lookup proposer (``bpe_transformer/ops/sampling.py``: ``lookup_draft``,
``ops/csrc/lookup_draft.hip``), written from the *other* formulation -- try ``n = n_hi`` down to ``n_lo``, scan the
starts from the latest, extend periodically -- and independently of ``lookup_draft_reference``; plus the case list of
its tests (``tests/test_lookup_refs.py`` on the CPU reference, ``tests/test_lookup_gpu.py`` on the kernel).

The oracle also serves as the proposer of the hand loop in ``tests/test_prompt_lookup.py``.
"""

from __future__ import annotations

import random

import torch

WG = 256  # the kernel's workgroup size (lookup_draft.hip: LK_NT)
STAGE = 8192  # the longest history the kernel stages in LDS (LK_STAGE); past it it scans global memory
SENTINEL = -9  # what win[:, 1:] holds before the call


def lookup(h: list[int], K: int, n_hi: int, n_lo: int = 1) -> list[int]:
    """The K drafts for the history ``h`` (Python ints)."""
    L = len(h)
    for n in range(min(n_hi, L - 1), n_lo - 1, -1):  # (an occurrence needs a token after it: n <= L - 1)
        tail = h[L - n:]
        for s in range(L - 1 - n, -1, -1):  # the latest start first
            if h[s : s + n] == tail:
                after, p = s + n, L - (s + n)
                return [h[after + j % p] for j in range(K)]
    return [h[-1]] * K


class Case:
    """A batch of histories for one ``(K, n_hi, n_lo)``.  ``rows``: ``(h, n_prompt, idle)`` with ``idle`` one of
    ``None``, ``"done"``, ``"step"``.  The padding of ``prompt`` and the tail of ``out`` are poisoned with the end of
    the row's own history, cyclically -- read as history, it is a longer and later match than any real one."""

    def __init__(self, name, rows, K=4, n_hi=3, n_lo=1, slack=4):
        self.name, self.K, self.n_hi, self.n_lo = name, K, n_hi, n_lo
        self.rows = [(list(h), int(np_), idle) for h, np_, idle in rows]
        B = len(self.rows)
        P = max(np_ for _, np_, _ in self.rows) + slack
        N = max(len(h) - np_ for h, np_, _ in self.rows) + slack
        self.prompt, self.out = torch.zeros(B, P, dtype=torch.long), torch.zeros(B, N, dtype=torch.long)
        self.n_prompt = torch.tensor([np_ for _, np_, _ in self.rows], dtype=torch.int32)
        self.n_out = torch.tensor([len(h) - np_ for h, np_, _ in self.rows], dtype=torch.int32)
        self.done = torch.tensor([int(idle == "done") for *_, idle in self.rows], dtype=torch.int32)
        self.step = torch.tensor([int(idle != "step") for *_, idle in self.rows], dtype=torch.int32)
        self.win = torch.full((B, K + 1), SENTINEL, dtype=torch.long)
        for b, (h, np_, _) in enumerate(self.rows):
            assert 0 <= np_ <= len(h) and len(h) >= 1
            tail = h[-min(len(h), max(n_hi, 2)):]
            poison = [tail[i % len(tail)] for i in range(P + N)]
            self.prompt[b] = torch.tensor(h[:np_] + poison[: P - np_])
            self.out[b] = torch.tensor(h[np_:] + poison[: N - (len(h) - np_)])
            self.win[b, 0] = h[-1]

    def expected(self) -> torch.Tensor:
        want = self.win.clone()
        for b, (h, _, idle) in enumerate(self.rows):
            if idle is None:
                want[b, 1:] = torch.tensor(lookup(h, self.K, self.n_hi, self.n_lo))
        return want

    def matched(self) -> list[bool]:
        """Per active row: did the lookup find a match (it differs from the no-match answer for some K)?"""
        res = []
        for h, _, idle in self.rows:
            if idle is None:
                L = len(h)
                res.append(any(h[s : s + n] == h[L - n:] for n in range(self.n_lo, min(self.n_hi, L - 1) + 1)
                               for s in range(L - n)))
        return res

    def run(self, fn, dev="cpu"):
        """``fn`` = ``lookup_draft`` or its reference on copies of the inputs on ``dev``; returns (win, the other
        tensors after the call, the same before it)."""
        names = ("prompt", "n_prompt", "out", "n_out", "step", "done")
        before = {k: getattr(self, k).clone() for k in names}
        args = {k: v.to(dev) for k, v in before.items()}
        win = self.win.clone().to(dev)
        fn(args["prompt"], args["n_prompt"], args["out"], args["n_out"], win, args["step"], args["done"], self.n_hi,
           self.n_lo)
        return win.cpu(), {k: v.cpu() for k, v in args.items()}, before


def _planted(L: int, at: int) -> list[int]:
    """``L`` distinct tokens (1000 + i) whose last two are 7, 8, with ``7, 8, 9`` planted at ``at`` -- the unique
    2-token match -- and a lone 8 at every 37th position elsewhere (1-token matches, later than the planted one when
    it sits at the front: the reduction must order by length first)."""
    h = [1000 + i for i in range(L)]
    for i in range(5, L - 4, 37):
        if not at - 2 <= i <= at + 4:
            h[i] = 8
    h[at : at + 3] = [7, 8, 9]
    h[L - 2:] = [7, 8]
    return h


def fuzz_cases(seed: int = 20250) -> list[Case]:
    """A few hundred rows over an alphabet of 3-4 tokens, L in 1..40, every (n_hi, n_lo, K) of the issue's grid."""
    rnd = random.Random(seed)
    cases = []
    for n_hi in (1, 2, 3, 5):
        for n_lo in range(1, n_hi + 1):
            for K in (1, 4, 9):
                rows = []
                for _ in range(10):
                    L = rnd.randint(1, 40)
                    A = rnd.choice((3, 4))
                    h = [rnd.randrange(A) + 11 for _ in range(L)]
                    rows.append((h, rnd.randint(0, L), None))
                cases.append(Case(f"fuzz-hi{n_hi}-lo{n_lo}-K{K}", rows, K, n_hi, n_lo))
    return cases


def all_cases() -> list[Case]:
    """The case list of the issue, the smallest shapes at which the lookup can go wrong."""
    x, y = 21, 22
    basic = [
        ([5], 1, None),  # L = 1
        ([5], 0, None),  # L = 1, all of it in `out`
        ([5, 5], 1, None),  # L = 2, a match: e = 0, p = 1
        ([5, 6], 2, None),  # L = 2, none
        (list(range(30, 40)), 4, None),  # all distinct: no match
        ([1, 2, 3, 7, 8, 3, 6, 1, 2, 3], 5, None),  # 3 tokens at the front against 1 token later: the longer wins
        ([1, 2, 5, 1, 2, 6, 1, 2, 4, 2], 3, None),  # one token: [2] at 1, 4, 7 -- the latest wins
        ([2, 3, 9, 1, 2, 3], 2, None),  # [2, 3] at the very start: the candidate e = 1 is cut at t <= e + 1 = 2
        ([3, 9, 1, 2, 3], 5, None),  # the same with e = 0, t <= 1
        ([1, 2, x, y, x, y, x], 3, None),  # straddles the prompt / out boundary: match over indices 2..4
        ([50256, 50000, 50256, 123, 50256, 50000], 3, None),  # ids up to 50256
        ([1, 2, 3, 1, 2, 3], 6, "done"),  # idle rows keep their win row
        ([1, 2, 3, 1, 2, 3], 0, "step"),
        ([4, 7, 7], 1, None),
    ]
    cases = [Case("basic", basic), Case("basic-K1", basic, K=1), Case("basic-K9", basic, K=9),
             Case("n_hi-above-L", [([1, 2, 1], 2, None), ([6], 1, None), ([6, 6], 0, None)], n_hi=5),
             Case("equal-lengths-later-wins", [([1, 2, 5, 1, 2, 6, 1, 2], 3, None)], n_hi=2),
             # only n_lo = 2 matches ([9, 2, 3] does not occur); one token alone is below n_lo: no match
             Case("match-only-at-n_lo", [([1, 2, 3, 9, 2, 3], 3, None), ([1, 2, 3, 4, 3], 1, None)], n_hi=3, n_lo=2),
             # continuations past the end of the history, periods 1, 2, 3
             Case("periodic-K7", [([4, 7, 7], 2, None), ([1, 2, 1, 2], 1, None), ([1, 2, 3, 1, 2, 3], 4, None)], K=7)]
    L = 2 * WG + 3
    cases.append(Case("strided-first-wave", [(_planted(L, 10), 300, None), (_planted(L, 10), 0, None)], n_hi=2))
    cases.append(Case("strided-last-wave", [(_planted(L, L - 7), 300, None), (_planted(L, L - 7), L, None)], n_hi=2))
    rnd = random.Random(5)
    long_rows = [(_planted(STAGE + 1, 4000), 5000, None), (_planted(STAGE + 1, STAGE - 8), 100, None),
                 ([rnd.randrange(50) for _ in range(STAGE + 9)], 4100, None),
                 ([rnd.randrange(50) for _ in range(STAGE)], 4100, None)]  # (the last L that is staged)
    cases.append(Case("past-the-staging-limit", long_rows, K=4, n_hi=3))
    return cases
