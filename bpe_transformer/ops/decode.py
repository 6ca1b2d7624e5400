"""KV-cache ops of the serving path (``csrc/decode_attn.hip``).

The reference has no inference engine ("absent layers"); these ops
let ``models.generation`` decode with a KV cache instead of re-running the
whole prefix for every new token.

* :func:`kv_append` takes the fused QKV projection of ``T`` new tokens per
  sequence, applies RoPE at their absolute positions (``pos .. pos+T-1``, with
  ``pos`` a device int32 tensor), writes K (roped) and V into the caches
  ``[B, Hkv, Lmax, D]``, and returns the roped queries ``[B*T, H*D]``.  A token whose position is at or past
  ``Lmax`` is dropped: nothing is written to the caches for it, and its query rows in the result are unspecified
  (the GPU kernel leaves them uninitialised, the CPU oracle fills them in).
* :func:`decode_gemv` / :func:`decode_qkv` are the M <= 8 skinny projections of
  the decode step with RMSNorm / residual-add prologues and SwiGLU / RoPE +
  cache-write epilogues (``csrc/decode_gemv.hip``).
* :func:`decode_attention` is single-token attention of ``q [B, H*D]`` over the
  first ``pos + 1`` cache rows (split-K "flash-decoding" with a combine pass).
* :func:`prefill_attention` is the attention of any number of new tokens per
  sequence over the cache (``csrc/flash_attn_cache.hip``: MFMA flash attention
  whose keys are the cache slabs and whose causal diagonal starts at ``pos``).

All read the position from device memory, so a decode step is shape-static and
can be captured in a HIP graph.  The CPU versions are the oracle.

``pos`` holds one int32 (a position shared by the batch) or one per sequence
(``[B]``: ragged batches, every sequence at its own length).  With ``[B]``
everything above holds per sequence: sequence ``b`` is placed, rotated, dropped
at ``Lmax`` and attended from ``pos[b]``.

**fp8 cache** (``csrc/kv_fp8.hip``).  A cache row -- the ``D`` values of one
(sequence, KV head, position), exactly what the bf16 cache would have held: K
roped and rounded to bf16, V as is -- is stored as ``D`` ``float8_e4m3fn`` bytes
(``k8``, ``v8 [B, Hkv, Lmax, D]``) and one fp32 scale (``k_scale``, ``v_scale
[B, Hkv, Lmax]``).  The scale ``s`` is the smallest power of two with ``max|x| /
s <= 448`` (:func:`kv_quantize_reference` states the corner cases), the bytes
are ``e4m3_rne(x / s)`` and the value read back is ``q * s`` -- exact in fp32
and representable in bf16.  So an fp8 cache *is* a bf16 cache that holds the
dequantised values, and that is how its consumers are defined:

* :func:`kv_append_fp8` is :func:`kv_append` with the K / V rows quantised (the
  returned ``q`` is bit-identical);
* :func:`decode_attention_fp8` (and ``decode_attention_partials_fp8``) is
  :func:`decode_attention` on the dequantised caches, reading half the bytes;
* :func:`prefill_attention_fp8` (``cache_attn_fp8``) is
  :func:`prefill_attention` on the dequantised caches, computed from the e4m3
  rows as stored: on the GPU bit for bit :func:`kv_dequant` into a zeroed pair
  followed by :func:`prefill_attention`, in one launch and with no scratch;
* :func:`kv_dequant` writes the valid rows of a K / V pair as bf16 into a
  caller's pair -- a utility, and the oracle of that equality.

**fp8 weights**.  The same row format applied to a projection matrix ``w [N,
K]``, one row per output feature: :func:`weight_quantize` gives ``w8
float8_e4m3fn [N, K]`` and ``w_scale fp32 [N]``, :func:`weight_dequantize` the
bf16 matrix they stand for, exactly.  :func:`decode_gemv`, :func:`decode_qkv`
and :func:`decode_attn_proj` take the pair (``w=w8, w_scale=...``) and stream
half the weight bytes; each is, bit for bit on the GPU, the same call on
``weight_dequantize(w8, w_scale)``.  :func:`w_dequant` writes that matrix into
a caller's bf16 buffer (for a library GEMM).

**Paged cache** (``csrc/kv_cache.h``: ``PagedLayout``).  Every function above that takes a cache also takes
``block_table=None`` and ``max_len=None``.  With a table, ``k_cache`` / ``v_cache`` / ``k8`` / ``v8`` are *pools*
``[P, Hkv, KV_PAGE, D]`` (bf16 or ``float8_e4m3fn``; an fp8 pool has ``k_scale`` / ``v_scale [P, Hkv, KV_PAGE]``) of
pages of ``KV_PAGE = 256`` rows in the unchanged row format, and ``block_table`` is a device int32 ``[B, NB]`` with
``NB * KV_PAGE >= Lmax``: entry ``[b, j]`` is the pool page that holds positions ``256 j .. 256 j + 255`` of sequence
``b``, ``-1`` where none is allocated.  ``Lmax`` is ``max_len`` (default ``NB * KV_PAGE``) and keeps its meaning: a
token at or past it is dropped; it need not be a multiple of the page.  The caller guarantees a valid entry for every
``j < ceil(min(pos[b] + T, Lmax) / 256)`` before a call that reads or writes there.  The kernels do not trust the
table any more than ``pos``: a reader clamps a page id into ``[0, P - 1]``, and an append whose entry is outside ``[0,
P)`` writes nothing to the pool.  A paged call gives, bit for bit, what the slab call gives on
:func:`paged_gather` of the pool -- a page is ``decode_attn``'s 256-key chunk and four of ``cache_attn``'s 64-key
tiles, so only the row addresses differ -- and the CPU oracles are defined that way: the slab reference on the
gathered slab, appends scattered back (:func:`paged_scatter`).  :func:`kv_dequant` stays slab-only.

**Packed prefill** (``csrc/kv_cache.h``: ``PackedMap``).  :func:`kv_append_packed` / :func:`prefill_attention_packed`
(and their ``_fp8`` forms) take the prompts of several sequences in one launch: ``qkv`` / ``q`` are ``[N, ...]`` with
the ``n_i`` rows of sequence ``i`` laid end to end, no padding, and a :class:`PackedPrompts` says where each goes --
per sequence ``(slot_i, off_i, n_i)``: the cache slot (row of ``pos``, of the slab batch and of the block table), its
first packed row and its token count, as a device int32 table ``[S, 3]`` written by the host.  The slots are distinct,
and ``pos`` is the cache's own per-slot ``[B]`` tensor, read on the device as ``pos[slot_i]``: token ``t`` of sequence
``i`` is rotated at, written to and attends from position ``pos[slot_i] + t`` of slot ``slot_i``; slots not named are
not touched.  The attention additionally takes a host-built work list ``[W, 2]`` of ``(sequence, 128-row query
block)`` items, heaviest first; a sequence's blocks start at its own row 0, so each sequence's rows are, bit for bit,
those of the unpacked op called on that slot alone.  The CPU references are defined that way: a loop over the
sequences of the unpacked reference on the slot's slice.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from . import reference as F
from ._ext import ops


def _rope_args(x: Tensor, cos: Tensor | None, sin: Tensor | None) -> tuple[Tensor, Tensor, bool]:
    """``(cos, sin, use_rope)`` as the HIP ops take them: empty tables and ``False`` where there is no RoPE."""
    if cos is not None:
        return cos, sin, True
    e = x.new_empty(0, dtype=torch.float32)
    return e, e, False


def _scale(cache: Tensor, scale: float | None) -> float:
    """The softmax scale: ``1 / sqrt(D)`` of the cache's head dim unless given."""
    return 1.0 / math.sqrt(cache.shape[-1]) if scale is None else scale


# ------------------------------------------------------------------ paged cache (csrc/kv_cache.h)
KV_PAGE = 256  # rows of a page: kvc::KV_PAGE, decode_attn's chunk and four of cache_attn's key tiles


def _pg(block_table: Tensor | None, max_len: int | None) -> tuple:
    """The trailing ``block_table, max_len`` arguments of a HIP op: absent for a slab (the call is then what it
    always was)."""
    return () if block_table is None else (block_table, 0 if max_len is None else int(max_len))


def _paged_len(block_table: Tensor, max_len: int | None) -> int:
    n = block_table.shape[1] * KV_PAGE
    assert max_len is None or 1 <= max_len <= n, "max_len: at most NB * KV_PAGE"
    return n if max_len is None else int(max_len)


def paged_gather(pool: Tensor, block_table: Tensor, max_len: int | None = None) -> Tensor:
    """The slab a block table stands for: ``pool [P, Hkv, KV_PAGE, ...]`` (cache rows, or an fp8 pool's scales) and
    ``block_table [B, NB]`` -> ``[B, Hkv, Lmax, ...]`` with positions ``256 j ..`` of sequence ``b`` taken from page
    ``block_table[b, j]``; positions of an unallocated entry (``-1``) are zeros."""
    Lmax = _paged_len(block_table, max_len)
    B, NB = block_table.shape
    t = block_table.to(pool.device).long()
    pages = pool[t.clamp(min=0)]  # [B, NB, Hkv, KV_PAGE, ...]
    hole = (t < 0).view(B, NB, *[1] * (pool.dim() - 1))
    pages = torch.where(hole, torch.zeros((), dtype=pool.dtype, device=pool.device), pages)
    return pages.transpose(1, 2).reshape(B, pool.shape[1], NB * KV_PAGE, *pool.shape[3:])[:, :, :Lmax].contiguous()


def paged_scatter(slab: Tensor, pool: Tensor, block_table: Tensor) -> Tensor:
    """The inverse of :func:`paged_gather`: the rows of ``slab [B, Hkv, Lmax, ...]`` are written into the pages the
    table names (in place; entries ``-1`` are skipped, pool rows past ``Lmax`` in a last page and pages in no table
    row are left as they are).  Returns ``pool``."""
    Lmax = slab.shape[2]
    for b, row in enumerate(block_table.tolist()):
        for j, pg in enumerate(row):
            n = min(KV_PAGE, Lmax - KV_PAGE * j)
            if pg >= 0 and n > 0:
                pool[pg, :, :n] = slab[b, :, KV_PAGE * j : KV_PAGE * j + n]
    return pool


def _on_slab(fn, pools: tuple, block_table: Tensor, max_len: int | None, write: bool = False):
    """A paged reference: ``fn(*slabs)`` on the gathered slabs of ``pools``; ``write``: the slabs are scattered back."""
    slabs = [paged_gather(p, block_table, max_len) for p in pools]
    out = fn(*slabs)
    if write:
        for sl, p in zip(slabs, pools):
            paged_scatter(sl, p, block_table)
    return out


def kv_append(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, cos: Tensor | None, sin: Tensor | None, pos: Tensor,
              batch: int, n_new: int, n_heads: int, block_table: Tensor | None = None,
              max_len: int | None = None) -> Tensor:
    if qkv.is_cuda:
        c, s, use_rope = _rope_args(qkv, cos, sin)
        return ops().kv_append(qkv, k_cache, v_cache, c, s, pos, batch, n_new, n_heads, use_rope,
                               *_pg(block_table, max_len))
    return kv_append_reference(qkv, k_cache, v_cache, cos, sin, pos, batch, n_new, n_heads, block_table, max_len)


def _per_sequence(pos: Tensor) -> bool:
    """``pos`` is ``[B]`` (one position per sequence) rather than one shared element."""
    return pos.numel() > 1


def kv_append_reference(qkv, k_cache, v_cache, cos, sin, pos, batch, n_new, n_heads, block_table=None,
                        max_len=None) -> Tensor:
    if block_table is not None:
        return _on_slab(lambda k, v: kv_append_reference(qkv, k, v, cos, sin, pos, batch, n_new, n_heads),
                        (k_cache, v_cache), block_table, max_len, write=True)
    if _per_sequence(pos):  # one sequence at a time on its slab of the caches (views: written in place)
        assert pos.numel() == batch
        rows = qkv.view(batch, n_new, -1)
        return torch.cat([kv_append_reference(rows[b], k_cache[b : b + 1], v_cache[b : b + 1], cos, sin,
                                              pos.reshape(-1)[b : b + 1], 1, n_new, n_heads) for b in range(batch)])
    _, Hkv, Lmax, D = k_cache.shape
    H = n_heads
    p0 = int(pos.reshape(-1)[0])
    x = qkv.view(batch, n_new, H + 2 * Hkv, D)
    q, k, v = x[:, :, :H], x[:, :, H : H + Hkv], x[:, :, H + Hkv :]
    if cos is not None:
        tp = torch.arange(p0, p0 + n_new, device=qkv.device)
        q = F.apply_rope(q.float().transpose(1, 2), cos, sin, tp).transpose(1, 2).to(qkv.dtype)
        k = F.apply_rope(k.float().transpose(1, 2), cos, sin, tp).transpose(1, 2).to(qkv.dtype)
    n = max(0, min(n_new, Lmax - p0))
    k_cache[:, :, p0 : p0 + n] = k[:, :n].transpose(1, 2).to(k_cache.dtype)
    v_cache[:, :, p0 : p0 + n] = v[:, :n].transpose(1, 2).to(v_cache.dtype)
    return q.reshape(batch * n_new, H * D)


def decode_attention(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, n_heads: int,
                     scale: float | None = None, n_new: int = 1, block_table: Tensor | None = None,
                     max_len: int | None = None) -> Tensor:
    """Attention of ``n_new`` new tokens per sequence (``q [B*n_new, H*D]``, already appended to the caches at
    positions ``pos .. pos + n_new - 1``) over the cache; token t sees keys ``0 .. pos + t``."""
    scale = _scale(k_cache, scale)
    if q.is_cuda:
        return ops().decode_attn(q.contiguous(), k_cache, v_cache, pos, n_heads, scale, True, n_new,
                                 *_pg(block_table, max_len))
    return decode_attention_reference(q, k_cache, v_cache, pos, n_heads, scale, n_new, block_table, max_len)


def decode_attention_reference(q, k_cache, v_cache, pos, n_heads, scale=None, n_new: int = 1, block_table=None,
                               max_len=None) -> Tensor:
    if block_table is not None:
        return _on_slab(lambda k, v: decode_attention_reference(q, k, v, pos, n_heads, scale, n_new),
                        (k_cache, v_cache), block_table, max_len)
    B, Hkv, Lmax, D = k_cache.shape
    H, T = n_heads, n_new
    if _per_sequence(pos):
        assert pos.numel() == B
        qr = q.view(B, T, -1)
        return torch.cat([decode_attention_reference(qr[b], k_cache[b : b + 1], v_cache[b : b + 1],
                                                     pos.reshape(-1)[b : b + 1], H, scale, T) for b in range(B)])
    p0 = int(pos.reshape(-1)[0])
    L = min(p0 + T, Lmax)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    qf = q.float().view(B, T, Hkv, H // Hkv, D)
    k = k_cache[:, :, :L].float()
    v = v_cache[:, :, :L].float()
    s = torch.einsum("bthgd,bhld->bthgl", qf, k) * scale
    visible = torch.arange(L, device=q.device)[None, :] <= (p0 + torch.arange(T, device=q.device))[:, None]
    s = s.masked_fill(~visible[None, :, None, None, :], float("-inf"))
    o = torch.einsum("bthgl,bhld->bthgd", F.softmax(s, -1), v)
    return o.reshape(B * T, H * D).to(q.dtype)


def prefill_attention(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, n_heads: int,
                      scale: float | None = None, n_new: int = 1, block_table: Tensor | None = None,
                      max_len: int | None = None) -> Tensor:
    """Flash prefill over the cache (``csrc/flash_attn_cache.hip``): the contract of :func:`decode_attention` --
    ``q [B*n_new, H*D]`` already appended at ``pos .. pos + n_new - 1``, token t sees keys ``0 .. pos + t`` -- for
    any ``n_new`` (MFMA flash attention whose keys are the cache slabs), where ``decode_attention`` takes at most
    ``8 / G`` tokens.  The row of a token at or past ``Lmax`` is unspecified."""
    scale = _scale(k_cache, scale)
    if q.is_cuda:
        return ops().cache_attn(q.contiguous(), k_cache, v_cache, pos, n_heads, scale, n_new,
                                *_pg(block_table, max_len))
    return decode_attention_reference(q, k_cache, v_cache, pos, n_heads, scale, n_new, block_table, max_len)


# ------------------------------------------------------------------ packed prefill (csrc/kv_cache.h: PackedMap)
class PackedPrompts:
    """Where the rows of a packed call go (module docstring, "Packed prefill"): sequence ``i`` has ``lens[i]`` rows
    from row ``offs[i]`` on and belongs to cache slot ``slots[i]`` (distinct).  ``seq`` is the device int32 table
    ``[S, 3]`` of ``(slot, off, n)``, ``seq_host`` its flat host copy (the ops check that one, so no launch waits for
    a read-back).  ``pos_host`` (optional): the host's mirror of ``pos[slots[i]]``, used only to order the attention's
    work list heaviest first -- it changes the order workgroups start in, never a result."""

    def __init__(self, slots, lens, device=None, pos_host=None):
        self.slots, self.lens = [int(s) for s in slots], [int(n) for n in lens]
        assert len(self.slots) == len(self.lens) >= 1, "one length per slot, at least one sequence"
        assert len(set(self.slots)) == len(self.slots), "packed prefill: the slots must be distinct"
        assert all(n >= 1 for n in self.lens) and all(s >= 0 for s in self.slots), "slots >= 0, lengths >= 1"
        self.offs = [sum(self.lens[:i]) for i in range(len(self.lens))]
        self.N = sum(self.lens)
        self.pos_host = [0] * len(self.lens) if pos_host is None else [int(p) for p in pos_host]
        self.seq_host = [x for t in zip(self.slots, self.offs, self.lens) for x in t]
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self.seq = torch.tensor(self.seq_host, dtype=torch.int32).view(-1, 3).to(self.device)
        self._work: dict[int, Tensor] = {}

    def work_items(self, G: int) -> list[tuple[int, int]]:
        """The attention's work list for ``G`` query heads per kv head: one ``(sequence, block)`` per 128 rows of the
        ``G * n_i`` rows of every sequence, ordered by the keys the block's last row sees, descending."""
        items = [(p + min((128 * qb + 127) // G, n - 1) + 1, i, qb)
                 for i, (n, p) in enumerate(zip(self.lens, self.pos_host)) for qb in range((G * n + 127) // 128)]
        items.sort(key=lambda t: -t[0])  # (stable: equal weights keep sequence / block order)
        return [(i, qb) for _, i, qb in items]

    def work(self, G: int) -> Tensor:
        """:meth:`work_items` as the device int32 ``[W, 2]`` tensor the op takes (built once per ``G``)."""
        if G not in self._work:
            self._work[G] = torch.tensor(self.work_items(G), dtype=torch.int32).view(-1, 2).to(self.device)
        return self._work[G]


def _packed_loop(fn, packed: PackedPrompts, rows: Tensor, pos: Tensor, caches: tuple) -> Tensor:
    """``fn(rows_i, *slot views, pos_i, n_i)`` for each sequence of ``packed`` on its slot's one-row views of the slab
    ``caches`` (views: written in place) and its one-element ``pos``; the results concatenated in packed order."""
    out = []
    for s, o, n in zip(packed.slots, packed.offs, packed.lens):
        out.append(fn(rows[o : o + n], *[c[s : s + 1] for c in caches], pos.reshape(-1)[s : s + 1], n))
    return torch.cat(out)


def kv_append_packed(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, cos: Tensor | None, sin: Tensor | None,
                     pos: Tensor, packed: PackedPrompts, n_heads: int, block_table: Tensor | None = None,
                     max_len: int | None = None) -> Tensor:
    """:func:`kv_append` of the packed rows ``qkv [N, (H + 2 Hkv) D]``: sequence ``i``'s ``n_i`` tokens go to slot
    ``slots[i]`` at positions ``pos[slot] ..``; returns the roped ``q [N, H*D]``.  ``pos`` is the per-slot ``[B]``."""
    if qkv.is_cuda:
        c, s, use_rope = _rope_args(qkv, cos, sin)
        return ops().kv_append_packed(qkv, k_cache, v_cache, c, s, pos, packed.seq, packed.seq_host, n_heads, use_rope,
                                      *_pg(block_table, max_len))
    return kv_append_packed_reference(qkv, k_cache, v_cache, cos, sin, pos, packed, n_heads, block_table, max_len)


def kv_append_packed_reference(qkv, k_cache, v_cache, cos, sin, pos, packed, n_heads, block_table=None,
                               max_len=None) -> Tensor:
    if block_table is not None:
        return _on_slab(lambda k, v: kv_append_packed_reference(qkv, k, v, cos, sin, pos, packed, n_heads),
                        (k_cache, v_cache), block_table, max_len, write=True)
    return _packed_loop(lambda x, k, v, p, n: kv_append_reference(x, k, v, cos, sin, p, 1, n, n_heads),
                        packed, qkv, pos, (k_cache, v_cache))


def prefill_attention_packed(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, packed: PackedPrompts,
                             n_heads: int, scale: float | None = None, block_table: Tensor | None = None,
                             max_len: int | None = None) -> Tensor:
    """:func:`prefill_attention` of the packed rows ``q [N, H*D]`` (already appended by :func:`kv_append_packed`, with
    ``pos`` not yet advanced): token ``t`` of sequence ``i`` sees keys ``0 .. pos[slot_i] + t`` of its slot.  Each
    sequence's rows are bit for bit those of :func:`prefill_attention` on its slot alone."""
    scale = _scale(k_cache, scale)
    if q.is_cuda:
        G = n_heads // k_cache.shape[1]
        return ops().cache_attn_packed(q.contiguous(), k_cache, v_cache, pos, packed.seq, packed.seq_host,
                                       packed.work(G), n_heads, scale, *_pg(block_table, max_len))
    return prefill_attention_packed_reference(q, k_cache, v_cache, pos, packed, n_heads, scale, block_table, max_len)


def prefill_attention_packed_reference(q, k_cache, v_cache, pos, packed, n_heads, scale=None, block_table=None,
                                       max_len=None) -> Tensor:
    if block_table is not None:
        return _on_slab(lambda k, v: prefill_attention_packed_reference(q, k, v, pos, packed, n_heads, scale),
                        (k_cache, v_cache), block_table, max_len)
    return _packed_loop(lambda x, k, v, p, n: decode_attention_reference(x, k, v, p, n_heads, scale, n),
                        packed, q, pos, (k_cache, v_cache))


def decode_attention_partials(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, n_heads: int,
                              scale: float | None = None, block_table: Tensor | None = None,
                              max_len: int | None = None) -> Tensor:
    """Split-K decode attention without the combine: fp32 ``[B, H, nsplit, D + 2]`` = (o, m, l) per 256-key chunk
    (natural-log units), consumed by :func:`decode_attn_proj`.  A chunk past the valid length has ``m = -inf`` and
    ``l = 0``; its ``o`` part is unspecified (the GPU kernel leaves it unwritten) and every consumer skips it."""
    scale = _scale(k_cache, scale)
    if q.is_cuda:
        return ops().decode_attn(q.contiguous(), k_cache, v_cache, pos, n_heads, scale, False, 1,
                                 *_pg(block_table, max_len))
    return decode_partials_reference(q, k_cache, v_cache, pos, n_heads, scale, block_table=block_table,
                                     max_len=max_len)


def decode_partials_reference(q, k_cache, v_cache, pos, n_heads, scale=None, chunk: int = 256, block_table=None,
                              max_len=None) -> Tensor:
    if block_table is not None:
        return _on_slab(lambda k, v: decode_partials_reference(q, k, v, pos, n_heads, scale, chunk),
                        (k_cache, v_cache), block_table, max_len)
    B, Hkv, Lmax, D = k_cache.shape
    H = n_heads
    if _per_sequence(pos):
        assert pos.numel() == B
        return torch.cat([decode_partials_reference(q[b : b + 1], k_cache[b : b + 1], v_cache[b : b + 1],
                                                    pos.reshape(-1)[b : b + 1], H, scale, chunk) for b in range(B)])
    L = min(int(pos.reshape(-1)[0]) + 1, Lmax)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    ns = (Lmax + chunk - 1) // chunk
    out = torch.zeros(B, H, ns, D + 2, dtype=torch.float32, device=q.device)
    out[..., D] = -math.inf
    qf = q.float().view(B, Hkv, H // Hkv, D)
    for c in range(ns):
        s0, s1 = c * chunk, min(L, (c + 1) * chunk)
        if s0 >= s1:
            continue
        s = torch.einsum("bhgd,bhld->bhgl", qf, k_cache[:, :, s0:s1].float()) * scale
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        o = torch.einsum("bhgl,bhld->bhgd", p, v_cache[:, :, s0:s1].float())
        out[:, :, c, :D] = o.reshape(B, H, D)
        out[:, :, c, D] = m.reshape(B, H)
        out[:, :, c, D + 1] = p.sum(-1).reshape(B, H)
    return out


def decode_attn_proj(part: Tensor, w: Tensor, w_scale: Tensor | None = None) -> Tensor:
    """Output projection of the decode attention from its partials: ``combine(part) @ w.T`` (bf16 rounding of
    the combined rows as in the unfused path).  With ``w_scale``, ``w`` is the e4m3 matrix of
    :func:`weight_quantize`."""
    if part.is_cuda:
        return ops().decode_attn_proj(part, w) if w_scale is None else ops().decode_attn_proj(part, w, w_scale)
    if w_scale is not None:
        w = weight_dequantize(w, w_scale)
    B, H, _, D2 = part.shape
    D = D2 - 2
    m = part[..., D]
    mx = m.amax(-1, keepdim=True)
    c = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - mx))
    # the o part of an empty chunk (m = -inf) is unspecified (the kernel leaves it unwritten): skipped, not scaled by 0
    po = torch.where(torch.isinf(m)[..., None], torch.zeros_like(part[..., :D]), part[..., :D])
    o = (c[..., None] * po).sum(2) / (c * part[..., D + 1]).sum(-1, keepdim=True).clamp_min(1e-30)
    x = o.reshape(B, H * D).to(w.dtype)
    return (x.float() @ w.float().t()).to(w.dtype)


def decode_gemv(x: Tensor, w: Tensor, xd: Tensor | None = None, ln: Tensor | None = None, eps: float = 1e-5,
                swiglu: bool = False, w_scale: Tensor | None = None) -> tuple[Tensor, Tensor | None]:
    """Skinny projection of ``M <= 8`` decode rows (``csrc/decode_gemv.hip``): ``h = RMSNorm(x + xd) * ln``
    (each part optional), then ``y = h W^T`` or, with ``swiglu``, ``silu(h W1^T) * (h W3^T)`` for
    ``w = [W1; W3]``.  Returns ``(y, x + xd)`` (the second is ``None`` without ``xd``).  With ``w_scale``, ``w`` is
    the e4m3 matrix of :func:`weight_quantize`."""
    if x.is_cuda:
        y, s = ops().decode_gemv(x, xd, ln, eps, w, 1 if swiglu else 0, *_ws(w_scale))
        return y, (s if xd is not None else None)
    return decode_gemv_reference(x, w, xd, ln, eps, swiglu, w_scale)


def _ws(w_scale: Tensor | None) -> tuple:
    """The trailing ``w_scale`` argument of a HIP op: absent for bf16 weights (the call is then what it always was)."""
    return () if w_scale is None else (w_scale,)


def decode_gemv_reference(x, w, xd=None, ln=None, eps=1e-5, swiglu=False, w_scale=None):
    """fp32 oracle with the kernel's rounding points (bf16 residual sum, bf16 GEMM outputs before SwiGLU); fp8
    weights are dequantised first."""
    if w_scale is not None:
        w = weight_dequantize(w, w_scale, x.dtype)
    s = (x.float() + xd.float()).to(x.dtype) if xd is not None else x
    h = s.float()
    if ln is not None:
        h = (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * ln.float()).to(x.dtype).float()
    y = (h @ w.float().t()).to(x.dtype)
    if swiglu:
        g, u = y.float().chunk(2, dim=-1)
        y = (g * torch.sigmoid(g) * u).to(x.dtype)
    return y, (s if xd is not None else None)


def decode_qkv(x: Tensor, w: Tensor, k_cache: Tensor, v_cache: Tensor, cos: Tensor | None, sin: Tensor | None,
               pos: Tensor, n_heads: int, xd: Tensor | None = None, ln: Tensor | None = None,
               eps: float = 1e-5, w_scale: Tensor | None = None, block_table: Tensor | None = None,
               max_len: int | None = None) -> tuple[Tensor, Tensor | None]:
    """Fused decode QKV: ``qkv = RMSNorm(x + xd) W^T`` for one new token per sequence, RoPE at the device-side
    position, K / V written into the caches; returns ``(q [M, H*D], x + xd)``.  With ``pos [M]`` row ``m`` is
    sequence ``m`` at ``pos[m]``; a row at ``Lmax`` or past it writes nothing, and its query row is unspecified
    (as for :func:`kv_append`).  With ``w_scale``, ``w`` is the e4m3 matrix of :func:`weight_quantize`."""
    if x.is_cuda:
        c, sn, use_rope = _rope_args(x, cos, sin)
        tail = _ws(w_scale) if block_table is None else (w_scale, *_pg(block_table, max_len))
        q, s = ops().decode_qkv(x, xd, ln, eps, w, k_cache, v_cache, c, sn, pos, n_heads, use_rope, *tail)
        return q, (s if xd is not None else None)
    qkv, s = decode_gemv_reference(x, w, xd, ln, eps, w_scale=w_scale)
    return kv_append_reference(qkv, k_cache, v_cache, cos, sin, pos, x.shape[0], 1, n_heads, block_table, max_len), s


# ------------------------------------------------------------------ fp8 cache (csrc/kv_fp8.hip)
FP8 = torch.float8_e4m3fn
KV_FP8_MIN_SCALE = 2.0 ** -64


def kv_quantize_reference(x: Tensor) -> tuple[Tensor, Tensor]:
    """The definition of the fp8 cache format.  ``x [..., D]`` (bf16 values in any float dtype) -> (``float8_e4m3fn``
    bytes ``[..., D]``, fp32 scales ``[...]``).  Per row, with ``a = max|x| = m 2^e`` (``m`` in ``[0.5, 1)``): ``s =
    2^(e-9)`` if ``m <= 0.875`` else ``2^(e-8)``, the smallest power of two with ``a / s <= 448``; clamped below at
    ``2^-64``; ``s = 1`` for an all-zero row; ``s = NaN`` for a row with a non-finite element (its bytes are
    unspecified: NaN here).  Bytes: ``e4m3_rne(x * (1 / s))`` -- the product is exact and never exceeds 448."""
    xf = x.float()
    a = xf.abs().amax(-1)
    m, e = torch.frexp(a)
    s = torch.ldexp(torch.ones_like(a), torch.where(m <= 0.875, e - 9, e - 8))
    s = s.clamp_min(KV_FP8_MIN_SCALE)
    s = torch.where(a == 0, torch.ones_like(s), s)
    s = torch.where(torch.isfinite(a), s, torch.full_like(s, math.nan))
    q = (xf * (1.0 / s).unsqueeze(-1)).to(FP8)
    return q, s


def kv_dequantize_reference(q: Tensor, s: Tensor, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """``q * s`` (exact in fp32, representable in bf16)."""
    return (q.float() * s.float().unsqueeze(-1)).to(dtype)


def kv_append_fp8(qkv: Tensor, k8: Tensor, v8: Tensor, k_scale: Tensor, v_scale: Tensor, cos: Tensor | None,
                  sin: Tensor | None, pos: Tensor, batch: int, n_new: int, n_heads: int,
                  block_table: Tensor | None = None, max_len: int | None = None) -> Tensor:
    """:func:`kv_append` into an fp8 cache: the rows it would have written to bf16 caches are quantised into ``k8`` /
    ``v8 [B, Hkv, Lmax, D]`` with their scales in ``k_scale`` / ``v_scale [B, Hkv, Lmax]``; returns the same ``q``."""
    if qkv.is_cuda:
        c, s, use_rope = _rope_args(qkv, cos, sin)
        return ops().kv_append_fp8(qkv, k8, v8, k_scale, v_scale, c, s, pos, batch, n_new, n_heads, use_rope,
                                   *_pg(block_table, max_len))
    return kv_append_fp8_reference(qkv, k8, v8, k_scale, v_scale, cos, sin, pos, batch, n_new, n_heads, block_table,
                                   max_len)


def kv_append_fp8_reference(qkv, k8, v8, k_scale, v_scale, cos, sin, pos, batch, n_new, n_heads, block_table=None,
                            max_len=None) -> Tensor:
    """:func:`kv_append_reference` into bf16-valued staging rows (``qkv``'s dtype rounded to bf16), which are then
    quantised row by row; only the rows ``kv_append`` writes change."""
    if block_table is not None:
        return _on_slab(lambda k, v, ks, vs: kv_append_fp8_reference(qkv, k, v, ks, vs, cos, sin, pos, batch, n_new,
                                                                     n_heads),
                        (k8, v8, k_scale, v_scale), block_table, max_len, write=True)
    B, Hkv, Lmax, D = k8.shape
    P = pos.reshape(-1).tolist()
    P = P if _per_sequence(pos) else P * batch
    kt = torch.zeros(B, Hkv, Lmax, D, dtype=torch.bfloat16, device=qkv.device)
    vt = torch.zeros_like(kt)
    q = kv_append_reference(qkv, kt, vt, cos, sin, pos, batch, n_new, n_heads)
    for b, p0 in enumerate(P):
        w = slice(p0, p0 + max(0, min(n_new, Lmax - p0)))
        for t, t8, ts in ((kt, k8, k_scale), (vt, v8, v_scale)):
            t8[b, :, w], ts[b, :, w] = kv_quantize_reference(t[b, :, w])
    return q


def decode_attention_fp8(q: Tensor, k8: Tensor, v8: Tensor, k_scale: Tensor, v_scale: Tensor, pos: Tensor,
                         n_heads: int, scale: float | None = None, n_new: int = 1, block_table: Tensor | None = None,
                         max_len: int | None = None) -> Tensor:
    """:func:`decode_attention` over an fp8 cache."""
    scale = _scale(k8, scale)
    if q.is_cuda:
        return ops().decode_attn_fp8(q.contiguous(), k8, v8, k_scale, v_scale, pos, n_heads, scale, True, n_new,
                                     *_pg(block_table, max_len))
    return decode_attention_fp8_reference(q, k8, v8, k_scale, v_scale, pos, n_heads, scale, n_new, block_table,
                                          max_len)


def decode_attention_fp8_reference(q, k8, v8, k_scale, v_scale, pos, n_heads, scale=None, n_new: int = 1,
                                   block_table=None, max_len=None) -> Tensor:
    """:func:`decode_attention_reference` on the dequantised caches (fp32 values, so nothing is rounded twice)."""
    if block_table is not None:
        return _on_slab(lambda k, v, ks, vs: decode_attention_fp8_reference(q, k, v, ks, vs, pos, n_heads, scale,
                                                                            n_new),
                        (k8, v8, k_scale, v_scale), block_table, max_len)
    return decode_attention_reference(q, kv_dequantize_reference(k8, k_scale, torch.float32),
                                      kv_dequantize_reference(v8, v_scale, torch.float32), pos, n_heads, scale, n_new)


def prefill_attention_fp8(q: Tensor, k8: Tensor, v8: Tensor, k_scale: Tensor, v_scale: Tensor, pos: Tensor,
                          n_heads: int, scale: float | None = None, n_new: int = 1,
                          block_table: Tensor | None = None, max_len: int | None = None) -> Tensor:
    """:func:`prefill_attention` over an fp8 cache (``csrc/flash_attn_cache.hip``, the ``Fp8Cache`` instantiation):
    any ``n_new``, the e4m3 rows and their scales read as stored."""
    scale = _scale(k8, scale)
    if q.is_cuda:
        return ops().cache_attn_fp8(q.contiguous(), k8, v8, k_scale, v_scale, pos, n_heads, scale, n_new,
                                    *_pg(block_table, max_len))
    return decode_attention_fp8_reference(q, k8, v8, k_scale, v_scale, pos, n_heads, scale, n_new, block_table,
                                          max_len)


def kv_append_packed_fp8(qkv: Tensor, k8: Tensor, v8: Tensor, k_scale: Tensor, v_scale: Tensor, cos: Tensor | None,
                         sin: Tensor | None, pos: Tensor, packed: PackedPrompts, n_heads: int,
                         block_table: Tensor | None = None, max_len: int | None = None) -> Tensor:
    """:func:`kv_append_packed` into an fp8 cache (the rows quantised as :func:`kv_append_fp8` does); the same ``q``."""
    if qkv.is_cuda:
        c, s, use_rope = _rope_args(qkv, cos, sin)
        return ops().kv_append_packed_fp8(qkv, k8, v8, k_scale, v_scale, c, s, pos, packed.seq, packed.seq_host,
                                          n_heads, use_rope, *_pg(block_table, max_len))
    return kv_append_packed_fp8_reference(qkv, k8, v8, k_scale, v_scale, cos, sin, pos, packed, n_heads, block_table,
                                          max_len)


def kv_append_packed_fp8_reference(qkv, k8, v8, k_scale, v_scale, cos, sin, pos, packed, n_heads, block_table=None,
                                   max_len=None) -> Tensor:
    if block_table is not None:
        return _on_slab(lambda k, v, ks, vs: kv_append_packed_fp8_reference(qkv, k, v, ks, vs, cos, sin, pos, packed,
                                                                            n_heads),
                        (k8, v8, k_scale, v_scale), block_table, max_len, write=True)
    return _packed_loop(lambda x, k, v, ks, vs, p, n: kv_append_fp8_reference(x, k, v, ks, vs, cos, sin, p, 1, n,
                                                                              n_heads),
                        packed, qkv, pos, (k8, v8, k_scale, v_scale))


def prefill_attention_packed_fp8(q: Tensor, k8: Tensor, v8: Tensor, k_scale: Tensor, v_scale: Tensor, pos: Tensor,
                                 packed: PackedPrompts, n_heads: int, scale: float | None = None,
                                 block_table: Tensor | None = None, max_len: int | None = None) -> Tensor:
    """:func:`prefill_attention_packed` over an fp8 cache, the e4m3 rows and their scales read as stored."""
    scale = _scale(k8, scale)
    if q.is_cuda:
        G = n_heads // k8.shape[1]
        return ops().cache_attn_packed_fp8(q.contiguous(), k8, v8, k_scale, v_scale, pos, packed.seq, packed.seq_host,
                                           packed.work(G), n_heads, scale, *_pg(block_table, max_len))
    return prefill_attention_packed_fp8_reference(q, k8, v8, k_scale, v_scale, pos, packed, n_heads, scale,
                                                  block_table, max_len)


def prefill_attention_packed_fp8_reference(q, k8, v8, k_scale, v_scale, pos, packed, n_heads, scale=None,
                                           block_table=None, max_len=None) -> Tensor:
    if block_table is not None:
        return _on_slab(lambda k, v, ks, vs: prefill_attention_packed_fp8_reference(q, k, v, ks, vs, pos, packed,
                                                                                    n_heads, scale),
                        (k8, v8, k_scale, v_scale), block_table, max_len)
    return _packed_loop(lambda x, k, v, ks, vs, p, n: decode_attention_fp8_reference(x, k, v, ks, vs, p, n_heads,
                                                                                     scale, n),
                        packed, q, pos, (k8, v8, k_scale, v_scale))


def decode_attention_partials_fp8(q: Tensor, k8: Tensor, v8: Tensor, k_scale: Tensor, v_scale: Tensor, pos: Tensor,
                                  n_heads: int, scale: float | None = None, n_new: int = 1,
                                  block_table: Tensor | None = None, max_len: int | None = None) -> Tensor:
    """:func:`decode_attention_partials` over an fp8 cache: the same layout, for :func:`decode_attn_proj`."""
    scale = _scale(k8, scale)
    if q.is_cuda:
        return ops().decode_attn_fp8(q.contiguous(), k8, v8, k_scale, v_scale, pos, n_heads, scale, False, n_new,
                                     *_pg(block_table, max_len))
    assert n_new == 1
    if block_table is not None:
        return _on_slab(lambda k, v, ks, vs: decode_attention_partials_fp8(q, k, v, ks, vs, pos, n_heads, scale),
                        (k8, v8, k_scale, v_scale), block_table, max_len)
    return decode_partials_reference(q, kv_dequantize_reference(k8, k_scale, torch.float32),
                                     kv_dequantize_reference(v8, v_scale, torch.float32), pos, n_heads, scale)


def kv_dequant(k8: Tensor, v8: Tensor, k_scale: Tensor, v_scale: Tensor, pos: Tensor, n_new: int, k_out: Tensor,
               v_out: Tensor) -> None:
    """Rows ``[0, min(pos[b] + n_new, Lmax))`` of every K and V slab, dequantised, into the bf16 ``k_out`` / ``v_out
    [B, Hkv, Lmax, D]``; the rows past them are left as they are.  ``pos`` is read on the device."""
    if k8.is_cuda:
        ops().kv_dequant(k8, v8, k_scale, v_scale, pos, n_new, k_out, v_out)
        return
    B, _, Lmax, _ = k8.shape
    P = pos.reshape(-1).tolist()
    P = P if _per_sequence(pos) else P * B
    for b, p0 in enumerate(P):
        n = max(0, min(p0 + n_new, Lmax))
        k_out[b, :, :n] = kv_dequantize_reference(k8[b, :, :n], k_scale[b, :, :n], k_out.dtype)
        v_out[b, :, :n] = kv_dequantize_reference(v8[b, :, :n], v_scale[b, :, :n], v_out.dtype)


# ------------------------------------------------------------------ fp8 weights (csrc/decode_gemv.hip)
def weight_quantize(w: Tensor) -> tuple[Tensor, Tensor]:
    """``w [N, K]`` -> (``w8 float8_e4m3fn [N, K]``, ``w_scale fp32 [N]``): :func:`kv_quantize_reference` on the rows,
    one row per output feature -- the same scale rule, corner cases and clamp.  Plain torch on ``w``'s device: it
    runs once per session."""
    assert w.dim() == 2, "weight_quantize: a [N, K] matrix"
    return kv_quantize_reference(w)


def weight_dequantize(w8: Tensor, w_scale: Tensor, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """The matrix an fp8 weight pair stands for: ``w8 * w_scale`` per row (exact in fp32, representable in bf16)."""
    return kv_dequantize_reference(w8, w_scale, dtype)


def w_dequant(w8: Tensor, w_scale: Tensor, out: Tensor) -> Tensor:
    """:func:`weight_dequantize` into the caller's contiguous bf16 ``out [N, K]`` (``K % 8 == 0``); returns it."""
    if w8.is_cuda:
        ops().w_dequant(w8, w_scale, out)
    else:
        out.copy_(weight_dequantize(w8, w_scale, out.dtype))
    return out
