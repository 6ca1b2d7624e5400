"""Inputs of the packed-prefill tests (``kv_append_packed`` / ``prefill_attention_packed``), shared by the CPU and the
GPU module so that both walk exactly the same cases.

The case: a cache of ``B = 5`` slots, ``Hkv = 2``, ``Lmax = 448``; the packed call names four of them in non-monotonic
order, slots ``[3, 0, 4, 1]`` with lengths ``[33, 1, 129, 9]`` at positions ``[64, 130, 0, 5]``.  Slot 2 is not named:
it holds poison (NaN / inf) everywhere and a position of its own.  Every named slot holds finite rows below ``pos + n``
and poison from there on, as in ``cache_prefill_refs.length_case``.  The lengths cover one row, less than a wave's 32
rows, more than one 128-row block (129, and ``G * n`` beyond that), and the positions put diagonals inside the first
key tile, across tiles and at a tile boundary (64).

:func:`full_case` lets one sequence run into ``Lmax`` (``pos = Lmax - 3``, ``n = 10``: three tokens fit, seven are
dropped); :func:`dominant_case` embeds ``cache_prefill_refs.dominant_case`` as one sequence among the others.
"""

from __future__ import annotations

import dataclasses
import functools

import torch
from torch import Tensor

from . import cache_prefill_refs as CR
from . import decode_refs as DR
from .decode_refs import f64

HKV, LMAX, B = 2, CR.LMAX, 5
SLOTS = [3, 0, 4, 1]
LENS = [33, 1, 129, 9]
POS = [64, 130, 0, 5]
IDLE, IDLE_POS = 2, 77  # the slot no call names
DIMS = (64, 128)
GROUPS = CR.GROUPS
FULL_SEQ = 1  # the sequence of full_case that runs into Lmax


@dataclasses.dataclass
class Case:
    D: int
    G: int
    slots: list[int]
    lens: list[int]
    pos: list[int]  # of the named slots, in call order
    q: Tensor  # [N, H*D] bf16
    qkv: Tensor  # [N, (H + 2 Hkv) D] bf16
    k: Tensor  # [B, Hkv, Lmax, D] bf16
    v: Tensor

    @property
    def H(self) -> int:
        return HKV * self.G

    @property
    def offs(self) -> list[int]:
        return [sum(self.lens[:i]) for i in range(len(self.lens))]

    @property
    def pos_all(self) -> list[int]:
        """One position per slot of the cache."""
        p = [IDLE_POS] * B
        for s, x in zip(self.slots, self.pos):
            p[s] = x
        return p

    def seqs(self):
        return list(zip(range(len(self.slots)), self.slots, self.offs, self.lens, self.pos))


def rope_tables(D: int, rows: int = LMAX + 16) -> tuple[Tensor, Tensor]:
    """fp32 ``cos`` / ``sin [rows, D/2]`` as the ops take them (longer than ``Lmax``: the CPU oracle rotates the
    tokens past the cache's end too, before it drops them)."""
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float(), ang.sin().float()


def _build(D: int, G: int, slots, lens, pos, seed: int) -> Case:
    H, N = HKV * G, sum(lens)
    k = DR.poison_like(torch.empty(B, HKV, LMAX, D)).reshape(B, HKV, LMAX, D).to(DR.BF16)
    v = k.clone()
    for s, n, p in zip(slots, lens, pos):
        valid = min(p + n, LMAX)
        ks, vs = DR.caches(1, HKV, LMAX, D, valid, seed=seed + 31 * s)
        k[s], v[s] = ks[0], vs[0]
    q = DR.queries(1, N, H, D, seed=seed + 5)
    qkv = DR.randn(N, (H + 2 * HKV) * D, seed=(seed, 9))
    return Case(D, G, list(slots), list(lens), list(pos), q, qkv, k, v)


@functools.lru_cache(maxsize=None)
def base_case(D: int, G: int) -> Case:
    """Cached: treat as read-only."""
    return _build(D, G, SLOTS, LENS, POS, seed=D + G)


@functools.lru_cache(maxsize=None)
def full_case(D: int = 64, G: int = 2) -> Case:
    """Sequence ``FULL_SEQ`` (slot 0) at ``pos = Lmax - 3`` with ``n = 10``: the semantics of
    ``cache_prefill_refs.full_case`` -- three tokens are written and attended, the rows of the other seven are
    unspecified."""
    lens, pos = list(LENS), list(POS)
    lens[FULL_SEQ], pos[FULL_SEQ] = 10, LMAX - 3
    return _build(D, G, SLOTS, lens, pos, seed=991)


@functools.lru_cache(maxsize=None)
def dominant_case(D: int, T: int, p0: int, shift: int):
    """``CR.dominant_case(D, T, p0, shift)``'s first sequence as sequence 0 (slot 3) of a packed call, G = 1, the
    others as in the base case.  -> (case, ref o, A, rows) with the last three for that sequence's ``T`` rows.  The
    packed neighbour that follows it in ``q`` (slot 0's single token) is what a look-ahead across sequences would
    read."""
    q, k, v, ref, A, rows = CR.dominant_case(D, T, p0, shift)
    lens, pos = list(LENS), list(POS)
    lens[0], pos[0] = T, p0
    c = _build(D, 1, SLOTS, lens, pos, seed=7 * p0 + T + shift)
    c.q[:T] = q[:T]
    c.k[SLOTS[0]], c.v[SLOTS[0]] = k[0], v[0]
    return c, ref[:T], A[:T], rows[:T]


def written(c: Case, i: int) -> int:
    """Tokens of sequence ``i`` that fit the cache."""
    return max(0, min(c.lens[i], LMAX - c.pos[i]))


@functools.lru_cache(maxsize=None)
def reference(D: int, G: int, which: str = "base"):
    """float64 ``(o, A)`` per sequence of a case, over the tokens that fit the cache
    (``decode_refs.decode_attention`` on the slot alone).  Computed once and shared."""
    c = base_case(D, G) if which == "base" else full_case(D, G)
    out = []
    for i, s, o, n, p in c.seqs():
        w = written(c, i)
        out.append(DR.decode_attention(f64(c.q[o:o + w]), f64(c.k[s:s + 1]), f64(c.v[s:s + 1]), p, c.H, w))
    return out


def page_table(nb: int) -> Tensor:
    """A block table ``[B, nb]`` whose pages are a fixed permutation of a pool of ``B * nb`` pages."""
    g = torch.Generator().manual_seed(4242)
    return torch.randperm(B * nb, generator=g).to(torch.int32).view(B, nb)
