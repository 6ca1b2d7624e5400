"""Cases and a rounding emulation for ``cache_attn`` over the fp8 KV cache (``csrc/flash_attn_cache.hip``, the
``Fp8Cache`` instantiation), shared by ``tests/test_cache_attn_fp8.py`` (CPU) and ``tests/test_cache_attn_fp8_gpu.py``
so that both walk exactly the same inputs.

The kernel converts every staged e4m3 tile into the bf16 LDS image with ``kv_dequant``'s arithmetic -- fp32
``e4m3 * scale``, rounded to bf16 -- and is the bf16 kernel from there on.  :func:`emulate_fp8` does that in plain
PyTorch in front of ``cache_prefill_refs.emulate`` (the bf16 kernel's rounding points); the CPU test asserts that its
result is, bit for bit, ``emulate`` on the dequantised bf16 cache built through the independent float64 path of
``kv_fp8_refs``, which is the argument for the GPU test's bitwise assertion.
"""

from __future__ import annotations

import functools

import torch

from . import cache_prefill_refs as CR
from . import decode_refs as DR
from . import kv_fp8_refs as KR
from .decode_refs import BF16, f64

LMAX = 256
# (name, G, T, positions (one shared int or one per sequence), Lmax, spread)
CASES = [
    ("smallest routed window, empty cache", 1, 9, 0, LMAX, False),
    ("diagonal inside tile 0", 1, 9, 63, LMAX, False),
    ("tail tile, cache not a tile multiple", 1, 64, 136, 200, False),
    ("second row block, diagonal across a tile edge", 1, 129, 63, LMAX, False),
    ("rows to tokens, G 2", 2, 40, 70, LMAX, False),
    ("rows to tokens, G 4", 4, 40, 70, LMAX, False),
    ("rows to tokens, G 8", 8, 40, 70, LMAX, False),
    ("ragged positions", 2, 20, (0, 150, 37), LMAX, False),
    ("dropped tokens", 1, 9, 200 - 3, 200, False),
    ("scales 2^20 apart", 1, 64, 136, 200, True),
]
IDS = [c[0] for c in CASES]
HKV = 2


def positions(pos) -> list[int]:
    """One position per sequence (a shared one: batch 2)."""
    return [pos] * 2 if isinstance(pos, int) else list(pos)


@functools.lru_cache(maxsize=None)
def case(D: int, name: str):
    """-> dict: ``q`` bf16 ``[B*T, H*D]``, the fp8 cache (``k8, v8, ks, vs``; byte 0x7F and scale NaN from row
    ``pos[b] + T`` on), its dequantised bf16 twin ``k, v`` (float64 path; poison rows NaN), ``plist``, ``pos`` (the
    int32 tensor the ops take), ``H, T, Lmax, n`` (tokens per sequence that fit) and per sequence the float64
    reference ``ref[b]``, ``A[b]`` over the ``n[b]`` specified tokens.  Cached: treat as read-only."""
    _, G, T, pos, Lmax, spread = CASES[IDS.index(name)]
    plist = positions(pos)
    B, H = len(plist), HKV * G
    valid = [min(p + T, Lmax) for p in plist]
    c = dict(KR.fp8_caches(B, HKV, Lmax, D, valid, seed=Lmax + T + sum(plist) + G, spread=spread))
    c["q"] = DR.queries(B, T, H, D, seed=Lmax + sum(plist) + T)
    kd = KR.dequantize64(KR.codes(c["k8"]), c["ks"])
    vd = KR.dequantize64(KR.codes(c["v8"]), c["vs"])
    c["n"] = [min(T, Lmax - p) for p in plist]
    c["ref"], c["A"] = [], []
    for b, (p, n) in enumerate(zip(plist, c["n"])):
        qn = f64(c["q"]).view(B, T, -1)[b, :n]
        r, a = DR.decode_attention(qn, kd[b:b + 1], vd[b:b + 1], p, H, n)
        c["ref"].append(r)
        c["A"].append(a)
    c.update(plist=plist, H=H, T=T, Lmax=Lmax, D=D,
             pos=torch.tensor([pos] if isinstance(pos, int) else plist, dtype=torch.int32))
    return c


def specified(c, out: torch.Tensor, b: int) -> torch.Tensor:
    """The rows of ``out [B*T, H*D]`` that sequence ``b``'s tokens below ``Lmax`` own."""
    return out.view(len(c["plist"]), c["T"], -1)[b, :c["n"][b]]


def convert(codes8: torch.Tensor, s: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The conversion pass: fp32 ``e4m3 * scale`` and its bf16 rounding."""
    x = codes8.float() * s.float().unsqueeze(-1)
    return x, x.to(BF16)


def emulate_fp8(c) -> torch.Tensor:
    """The fp8 kernel's rounding points, per sequence over its own ``L = pos + T`` rows (rows past them are zeros
    to the kernel and masked): conversion pass, then the bf16 kernel's."""
    B = len(c["plist"])
    out = []
    for b, p in enumerate(c["plist"]):
        L = min(p + c["T"], c["Lmax"])
        kb = torch.zeros(1, HKV, c["Lmax"], c["D"], dtype=BF16)
        vb = torch.zeros_like(kb)
        kb[0, :, :L] = convert(c["k8"][b, :, :L], c["ks"][b, :, :L])[1]
        vb[0, :, :L] = convert(c["v8"][b, :, :L], c["vs"][b, :, :L])[1]
        out.append(CR.emulate(c["q"].view(B, c["T"], -1)[b], kb, vb, p, c["H"], c["T"]))
    return torch.cat(out)


def emulate_dequantised(c) -> torch.Tensor:
    """``cache_prefill_refs.emulate`` on the dequantised bf16 cache (zeros in place of the poison, as the zeroed
    scratch of the two-launch route holds)."""
    return CR.emulate(c["q"], c["k"].nan_to_num(0.0), c["v"].nan_to_num(0.0), c["plist"], c["H"], c["T"])
