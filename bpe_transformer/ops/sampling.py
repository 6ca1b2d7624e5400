"""Token sampling on the device (``csrc/sample.hip``): greedy, temperature, top-k and top-p in one kernel, one
workgroup per logits row, without sorting the vocabulary.

The sampling function, per row ``x [V]`` with a uniform ``u``:

1. ``temperature <= 0``: the argmax, lowest index on ties.
2. Otherwise ``z_i = exp((x_i - max x) / temperature)``; a ``-inf`` logit has ``z = 0`` and is never returned.
3. *Rank order* is descending ``x`` and, among equal ``x``, ascending index.
4. ``top_k > 0`` keeps the first ``min(top_k, V)`` tokens in rank order (``0``: off).
5. ``top_p < 1`` keeps, of what top-k kept, a token iff the mass of the tokens ranked strictly before it is
   ``< top_p * Z``, with ``Z`` the mass top-k kept (the first token always stays).
6. With ``M`` the kept mass, the result is the lowest kept index whose inclusive cumulative kept mass, in index order,
   exceeds ``u * M``; if rounding finds none, the last kept index that has mass.

:func:`sample_logits` is that function for given uniforms.  :func:`sample_step` is the form that runs inside a
captured decode graph: it draws ``u`` itself -- Philox4x32-10, key ``seed``, counter ``(count, row, 0)``,
``u = ((x0 >> 8) + 0.5) * 2^-24`` rounded to fp32 -- from a device ``rng = (seed, count)`` tensor, writes the token into
``ids[b, 0]`` (the graph's own input) and ``out[b, count]``, and marks EOS in ``done`` / ``step``.  It never writes
``rng``; the caller advances ``rng[1]`` after it.

On the GPU both run the HIP kernel (fp32 ``exp``, masses summed in 2^-40 fixed point); on the CPU the
``*_reference`` functions below compute the same function in torch with fp64 masses and Philox in integer
arithmetic, so ``sampler="device"`` means the same thing on either device.
"""

from __future__ import annotations

import torch
from torch import Tensor

from ._ext import ops

_M32 = 0xFFFFFFFF


def philox4x32(key: tuple[int, int], counter: tuple[int, int, int, int], rounds: int = 10) -> tuple[int, ...]:
    """Philox4x32 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) on Python ints."""
    k0, k1 = key
    c0, c1, c2, c3 = counter
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def philox_uniform(seed: int, count: int, B: int, device=None) -> Tensor:
    """The uniforms :func:`sample_step` draws for rows ``0 .. B-1`` at ``rng = (seed, count)``: fp32 ``[B]``."""
    seed, count = int(seed) & (2**64 - 1), int(count) & (2**64 - 1)
    key = (seed & _M32, seed >> 32)
    x0 = [philox4x32(key, (count & _M32, count >> 32, b, 0))[0] for b in range(B)]
    u = (torch.tensor([x >> 8 for x in x0], dtype=torch.float64) + 0.5) * 2.0**-24
    return u.to(torch.float32).to(device)


def _check(logits: Tensor, temperature: float, top_k: int, top_p: float) -> None:
    assert logits.dim() == 2 and logits.shape[1] >= 1, "logits: [B, V]"
    assert logits.dtype in (torch.bfloat16, torch.float32), "logits: bf16 or fp32"
    assert int(top_k) >= 0, "top_k: 0 (off) or a positive count"


def sample_logits(logits: Tensor, temperature: float, top_k: int, top_p: float, u: Tensor) -> Tensor:
    """One token per row of ``logits [B, V]`` (bf16 / fp32) for the uniforms ``u [B]``; returns int64 ``[B]``."""
    _check(logits, temperature, top_k, top_p)
    if logits.is_cuda:
        return ops().sample_logits(logits.contiguous(), float(temperature), int(top_k), float(top_p),
                                   u.to(logits.device, torch.float32).contiguous())
    return sample_logits_reference(logits, temperature, top_k, top_p, u)


def sample_logits_reference(logits: Tensor, temperature: float, top_k: int, top_p: float, u: Tensor) -> Tensor:
    """The function of the module docstring in torch: fp64 masses, a stable sort for the rank order."""
    x = logits.double()
    B, V = x.shape
    if temperature <= 0:
        return (x == x.amax(-1, keepdim=True)).int().argmax(-1)  # (argmax of a 0/1 row: its first 1)
    z = torch.exp((x - x.amax(-1, keepdim=True)) / float(temperature))
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices  # equal x stay in index order
    zs = z.gather(-1, order)
    keep = torch.ones_like(zs, dtype=torch.bool)
    if top_k > 0:
        keep &= torch.arange(V, device=x.device)[None, :] < min(int(top_k), V)
    if top_p < 1.0:
        zk = zs * keep
        keep &= zk.cumsum(-1) - zk < float(top_p) * zk.sum(-1, keepdim=True)
        keep[:, 0] = True
    kept = torch.zeros_like(keep).scatter_(-1, order, keep)
    zk = z * kept
    cum = zk.cumsum(-1)
    M = cum[:, -1:]
    hit = (cum > u.to(x.device).double().reshape(B, 1) * M) & (zk > 0)
    idx = torch.arange(V, device=x.device)
    last = torch.where(zk > 0, idx, torch.zeros_like(idx)).amax(-1)  # rounding found none: the last one with mass
    return torch.where(hit.any(-1), hit.int().argmax(-1), last)


def sample_step(logits: Tensor, temperature: float, top_k: int, top_p: float, rng: Tensor, ids: Tensor, out: Tensor,
                step: Tensor | None, done: Tensor, eos: int) -> None:
    """Sample one token per row in place, for a decode loop that never leaves the device.

    ``rng`` int64 ``[2]`` = (seed, count), read only; ``ids`` int64 ``[B, 1]`` takes the token; ``out`` int64
    ``[B, N]`` takes it in column ``count``, or ``-1`` if the row is already done (``done[b] != 0``) or inactive
    (``step[b] == 0``); ``done`` int32 ``[B]`` is set where an active row draws ``eos`` (``eos < 0``: none), and a
    ragged session's ``step`` int32 ``[B]`` is cleared there, so that sequence stops advancing."""
    _check(logits, temperature, top_k, top_p)
    if logits.is_cuda:
        ops().sample_step(logits.contiguous(), float(temperature), int(top_k), float(top_p), rng, ids, out, step, done,
                          int(eos))
        return
    sample_step_reference(logits, temperature, top_k, top_p, rng, ids, out, step, done, eos)


def sample_step_reference(logits, temperature, top_k, top_p, rng, ids, out, step, done, eos) -> None:
    B = logits.shape[0]
    seed, count = (int(v) for v in rng.tolist())
    tok = sample_logits_reference(logits, temperature, top_k, top_p, philox_uniform(seed, count, B, logits.device))
    idle = done != 0
    if step is not None:
        idle = idle | (step == 0)
    ids.view(-1).copy_(tok)
    if 0 <= count < out.shape[1]:
        out[:, count] = torch.where(idle, torch.full_like(tok, -1), tok)
    if eos >= 0:
        hit = ~idle & (tok == eos)
        done[hit] = 1
        if step is not None:
            step[hit] = 0
