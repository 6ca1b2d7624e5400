"""Independent float64 path and shared builders for the fp8 KV cache tests (``csrc/kv_fp8.hip``, the oracles of
``bpe_transformer/ops/decode.py``).

The format's one definition is ``ops.decode.kv_quantize_reference`` (``frexp`` / ``ldexp`` / torch's e4m3 cast).
:func:`quantize64` states it again without any of the three: the scale by comparing ``a`` with ``448 * 2^k`` in
float64, the bytes by a nearest-value search over the table of the 127 non-negative finite e4m3 values, ties to the
even code.  The CPU tests compare the two; the GPU tests compare the kernels with the oracle.

The builders make the special rows every layer of tests plants (scale boundaries, zero, below the clamp) and the
poison of an fp8 cache: byte ``0x7F`` (e4m3 NaN) with scale NaN past the valid length.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from bpe_transformer.models.generation import KVCache

from . import decode_refs as DR

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
MIN_SCALE = 2.0 ** -64
NAN_BYTE = 0x7F


def e4m3_table() -> Tensor:
    """The finite non-negative e4m3fn values by code 0 .. 126 (float64), from the bit fields."""
    out = []
    for c in range(127):
        e, m = c >> 3, c & 7
        out.append(m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return torch.tensor(out, dtype=torch.float64)


def scale64(a: Tensor) -> Tensor:
    """Smallest power of two ``s`` with ``a / s <= 448`` (float64 ``a >= 0``), clamped at 2^-64; 1 for 0; NaN for a
    non-finite ``a``.  The guess from log2 is corrected by comparing with the exact products ``448 * 2^k``."""
    fin = torch.isfinite(a) & (a > 0)
    k = torch.ceil(torch.log2(torch.where(fin, a, torch.ones_like(a)) / 448.0))
    for _ in range(2):
        k = torch.where(a > 448.0 * torch.exp2(k), k + 1, k)
        k = torch.where(a <= 448.0 * torch.exp2(k - 1), k - 1, k)
    s = torch.exp2(k).clamp_min(MIN_SCALE)
    s = torch.where(a == 0, torch.ones_like(s), s)
    return torch.where(torch.isfinite(a), s, torch.full_like(s, math.nan))


def e4m3_rne64(y: Tensor) -> Tensor:
    """float64 ``|y| <= 448`` -> e4m3fn code (uint8): nearest table value, ties to the even code, sign kept."""
    tab = e4m3_table()
    mag = y.abs()
    hi = torch.searchsorted(tab, mag.contiguous()).clamp(1, 126)  # tab[hi - 1] <= mag <= tab[hi] (or mag is tab[0])
    lo = hi - 1
    dl, dh = mag - tab[lo], tab[hi] - mag
    code = torch.where(dl < dh, lo, torch.where(dh < dl, hi, torch.where(lo % 2 == 0, lo, hi)))
    neg = torch.signbit(y)
    return (code + 128 * neg.long()).to(torch.uint8)


def quantize64(x: Tensor) -> tuple[Tensor, Tensor]:
    """bf16-valued rows ``x [..., D]`` -> (codes uint8 ``[..., D]``, scale float64 ``[...]``).  Rows with a
    non-finite element: scale NaN, codes unspecified (0x7F here)."""
    x = DR.f64(x)
    s = scale64(x.abs().amax(-1))
    bad = torch.isnan(s)
    y = torch.where(bad.unsqueeze(-1), torch.zeros_like(x), x) / torch.where(bad, torch.ones_like(s), s).unsqueeze(-1)
    codes = e4m3_rne64(y)
    codes[bad] = NAN_BYTE
    return codes, s


def dequantize64(codes: Tensor, s: Tensor) -> Tensor:
    """codes uint8 + scale -> float64 values (NaN for code 0x7F / 0xFF)."""
    tab = torch.cat([e4m3_table(), torch.tensor([math.nan], dtype=torch.float64)])
    c = codes.long()
    return torch.where(c >= 128, -tab[c % 128], tab[c % 128]) * s.to(torch.float64).unsqueeze(-1)


def codes(q: Tensor) -> Tensor:
    """A float8 tensor's bytes."""
    return q.view(torch.uint8)


# ------------------------------------------------------------------ special rows
def special_rows(D: int) -> dict[str, Tensor]:
    """bf16 rows ``[D]`` at the corners of the scale rule; every row also holds small elements that land in the
    e4m3 subnormals (|x / s| < 2^-6) and exact rounding ties."""
    base = torch.zeros(D)
    filler = torch.tensor([1.0, -0.75, 0.3125, 2.0 ** -7, -(2.0 ** -8), 3 * 2.0 ** -10, 2.0 ** -10, 5 * 2.0 ** -10])
    rows = {}

    def row(amax: float, shift: int = 0) -> Tensor:
        r = base.clone()
        r[1:1 + filler.numel()] = filler * 2.0 ** shift
        r[0] = amax
        return r.to(BF16)

    for k in (-3, 0, 5):
        rows[f"448*2^{k}"] = row(448.0 * 2.0 ** k, k)            # a / s = 448 exactly: s = 2^k
        rows[f"450*2^{k}"] = row(450.0 * 2.0 ** k, k)            # the next bf16 above: s = 2^(k+1)
    rows["m=0.875"] = row(-0.875 * 2.0 ** 3, -6)                 # m = 0.875 exactly (negative maximum)
    rows["m>0.875"] = row(0.87890625 * 2.0 ** 3, -6)             # 0.875 + 2^-8: the next bf16
    rows["zero"] = base.to(BF16)
    rows["clamped"] = row(2.0 ** -80, -88)                       # s = 2^-64, a / s = 2^-16: all bytes zero
    rows["clamp edge"] = row(448.0 * 2.0 ** -64, -64)            # the last row the clamp leaves alone
    rows["below edge"] = row(2.0 ** -57, -66)                    # a / s = 128 under the clamp: still s = 2^-64
    rows["huge"] = row(3.0e38, 118)
    return rows


def planted(D: int) -> Tensor:
    """The special rows stacked: ``[n, D]`` bf16."""
    return torch.stack(list(special_rows(D).values()))


# ------------------------------------------------------------------ caches
def fp8_caches(B: int, Hkv: int, Lmax: int, D: int, valid, seed: int = 0, spread: bool = False):
    """Quantised K / V of ``DR.caches``-like random bf16 rows, valid below ``valid`` (an int or one per sequence),
    poison (byte 0x7F, scale NaN) from there on.  ``spread``: neighbouring rows' magnitudes -- hence scales --
    differ by 2^20 (odd rows of K, even rows of V), with q . k kept moderate by the small side.
    -> dict with fp8 ``k8, v8``, fp32 ``ks, vs`` and the dequantised bf16 ``k, v`` (poison rows NaN)."""
    from bpe_transformer.ops.decode import kv_quantize_reference

    k = DR.randn(B, Hkv, Lmax, D, seed=(seed, 1))
    v = DR.randn(B, Hkv, Lmax, D, seed=(seed, 2))
    if spread:
        k[:, :, 1::2] = (k[:, :, 1::2].float() * 2.0 ** -20).to(BF16)
        v[:, :, 0::2] = (v[:, :, 0::2].float() * 2.0 ** -20).to(BF16)
    valid = [valid] * B if isinstance(valid, int) else list(valid)
    out = {}
    for name, t in (("k", k), ("v", v)):
        q8, s = kv_quantize_reference(t)
        by = codes(q8).clone()
        for b, n in enumerate(valid):
            by[b, :, n:] = NAN_BYTE
            s[b, :, n:] = math.nan
        out[name + "8"] = by.view(FP8)
        out[name + "s"] = s
        out[name] = dequantize64(by, s).to(torch.float32).to(BF16)
    return out


class DequantisedCache(KVCache):
    """A bf16-dtype ``KVCache`` whose oracle-path writes store quantise -> dequantise of each row through the
    independent float64 path above: "the fp8 cache as a bf16 cache that holds the dequantised values"."""

    def write(self, layer, row, lo, hi, k, v):
        for dst, t in ((self.k, k), (self.v, v)):
            c, s = quantize64(t.to(BF16))
            dst[layer, row, :, lo:hi] = dequantize64(c, s).to(torch.float32).to(BF16)
