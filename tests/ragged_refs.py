"""Builders and per-sequence references for the ragged (one position per sequence) KV-cache tests.

The float64 references are the ones of ``tests/decode_refs.py``, called once per sequence on the ``b:b+1`` slice of
the inputs with that sequence's position, then concatenated; nothing new is derived here.  The builders make the
GPU tests' inputs on the CPU (fixed seed, rounded to bf16) with bf16 NaN / +-inf poison in every cache row at or
past ``pos[b] + T`` of sequence ``b``, so a kernel that reads sequence ``b`` with a neighbour's position returns NaN.
``tests/test_ragged_decode.py`` (CPU) asserts that no poison lies in any visible range.
"""

from __future__ import annotations

import torch
from torch import Tensor

from . import decode_refs as DR
from .decode_refs import f64


def ragged_caches(Hkv: int, Lmax: int, D: int, pos: list[int], T: int, seed: int = 0) -> tuple[Tensor, Tensor]:
    """K, V ``[B, Hkv, Lmax, D]``: sequence b has finite random rows below ``pos[b] + T`` and poison from there on."""
    B = len(pos)
    k, v = DR.caches(B, Hkv, Lmax, D, Lmax, seed=seed)
    for b, p in enumerate(pos):
        k[b, :, p + T:] = DR.poison_like(k[b, :, p + T:])
        v[b, :, p + T:] = DR.poison_like(v[b, :, p + T:])
    return k, v


def visible_is_finite(k: Tensor, v: Tensor, pos: list[int], T: int) -> bool:
    return all(bool(torch.isfinite(t[b, :, :p + T]).all()) for t in (k, v) for b, p in enumerate(pos))


def poison_is_there(k: Tensor, v: Tensor, pos: list[int], T: int) -> bool:
    """Every row at or past ``pos[b] + T`` is non-finite in every element (where there is such a row)."""
    return all(not bool(torch.isfinite(t[b, :, p + T:]).any()) for t in (k, v) for b, p in enumerate(pos))


def attention_case(Hkv: int, G: int, D: int, Lmax: int, pos: list[int], T: int, seed: int = 0):
    """-> (q [B*T, H*D], K, V, H) with the poison layout above."""
    B, H = len(pos), Hkv * G
    q = DR.queries(B, T, H, D, seed=seed + 17)
    k, v = ragged_caches(Hkv, Lmax, D, pos, T, seed=seed + 17)
    return q, k, v, H


def decode_attention(q: Tensor, k: Tensor, v: Tensor, pos: list[int], H: int, T: int = 1):
    """Per-sequence ``decode_refs.decode_attention`` -> (o [B*T, H*D], A)."""
    B = len(pos)
    qr = f64(q).view(B, T, -1)
    outs = [DR.decode_attention(qr[b], f64(k[b:b + 1]), f64(v[b:b + 1]), pos[b], H, T) for b in range(B)]
    return torch.cat([o for o, _ in outs]), torch.cat([a for _, a in outs])


def decode_partials(q: Tensor, k: Tensor, v: Tensor, pos: list[int], H: int, T: int = 1) -> dict[str, Tensor]:
    """Per-sequence ``decode_refs.decode_partials``, concatenated over the ``B*T`` rows."""
    B = len(pos)
    qr = f64(q).view(B, T, -1)
    outs = [DR.decode_partials(qr[b], f64(k[b:b + 1]), f64(v[b:b + 1]), pos[b], H, T) for b in range(B)]
    return {key: torch.cat([o[key] for o in outs]) for key in ("part", "A", "empty")}


def kv_append(qkv: Tensor, cos, sin, pos: list[int], T: int, H: int, Hkv: int, D: int, Lmax: int) -> list[dict]:
    """Per-sequence ``decode_refs.kv_append`` (B = 1 each): a list of its result dicts."""
    rows = f64(qkv).view(len(pos), T, -1)
    return [DR.kv_append(rows[b], cos, sin, p, 1, T, H, Hkv, D, Lmax) for b, p in enumerate(pos)]


def qkv_rows(r: dict, e: Tensor, cos, sin, pos: list[int], H: int, Hkv: int, D: int):
    """``decode_refs.qkv_epilogue`` of row m at ``pos[m]`` -> (ref, A, slack), each ``[M, H + 2 Hkv, D]``."""
    outs = [DR.qkv_epilogue(r["y"][m:m + 1], e[m:m + 1], cos, sin, p, H, Hkv, D) for m, p in enumerate(pos)]
    return tuple(torch.cat([o[i] for o in outs]) for i in range(3))


# ------------------------------------------------------------------ session tests
def spread_lengths(B: int, lo: int = 5, hi: int = 30) -> list[int]:
    """B lengths spread over lo..hi, both ends included, not sorted (neighbours differ)."""
    if B == 1:
        return [hi]
    up = [lo + round(i * (hi - lo) / (B - 1)) for i in range(B)]
    return up[0::2] + up[1::2][::-1]


def padded(seqs: list[Tensor], width: int | None = None, pad: int = 0) -> Tensor:
    """Right-padded ``[B, width]`` ids of 1-D sequences."""
    width = width or max(int(s.numel()) for s in seqs)
    out = torch.full((len(seqs), width), pad, dtype=torch.long, device=seqs[0].device)
    for b, s in enumerate(seqs):
        out[b, :s.numel()] = s
    return out
