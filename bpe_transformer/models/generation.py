"""KV-cache inference: prefill + single-token decode, HIP-graph-captured on MI355X.

The reference has no inference engine (SURVEY §1 lists serving among the
absent layers; its only "generation" is the contract model's logits,
``tests/adapters.py:282-361``).  :meth:`TransformerLM.generate` used to re-run
the whole prefix for each new token; :class:`DecodeSession` keeps a KV cache
instead:

* **prefill** (``T`` prompt tokens, empty cache): the training kernels --
  RMSNorm, the fused [Wq;Wk;Wv] GEMM, flash attention with fused RoPE -- plus
  ``kv_append``, which writes the roped K and the V of all ``T`` tokens into
  the cache in one launch;
* **append** to a filled cache (a new turn of a conversation, a slot that keeps
  a shared prefix, a chunk of a long prompt): one pass over the layers for the
  whole window, each layer a multi-token ``kv_append`` + ``cache_attn``
  (``csrc/flash_attn_cache.hip``: MFMA flash attention whose keys are the cache
  slabs and in which token ``t`` sees the cache and its own causal prefix,
  ``pos + t``).  A window of at most ``8 / G`` tokens (draft tokens to verify)
  is one ``kv_append`` + ``decode_attn`` step instead, the VALU kernel of the
  decode step, which takes up to 8 query rows per KV head;
* **chunked prefill** (``prefill_chunk=c``): every prefill or append is cut into
  chunks of at most ``c`` tokens -- on an empty cache the first through the
  flash path, the later ones through ``cache_attn`` -- so activation memory is
  bounded by ``B * c`` rows whatever the prompt length;
* **decode** (one token per sequence): ``kv_append`` (RoPE at the device-side
  position, cache write, roped q) -> ``decode_attn`` (split-K flash-decoding
  over the cache) for every layer, residual adds fused into the next RMSNorm,
  then the LM head.  The position lives in a device int32 tensor, so the whole
  step has static shapes and is captured once into a HIP graph
  (``torch.cuda.CUDAGraph`` is hipGraph on ROCm) and replayed per token: one
  graph launch instead of ~10 kernel launches per layer.

Cache layout: ``k, v: [num_layers, B, Hkv, Lmax, D]`` bf16 (RoPE already
applied to K), i.e. each (sequence, kv head) is one contiguous ``Lmax x D``
slab the decode kernel streams.  GPT-2-small at Lmax 1024 needs 36 MiB per
sequence, so a 288 GB MI355X holds thousands of sequences.

**fp8 cache** (``kv_dtype="fp8"``, opt-in): the same layout in
``float8_e4m3fn`` bytes plus one power-of-two fp32 scale per row (``k_scale,
v_scale: [num_layers, B, Hkv, Lmax]``), ``(D + 4) / (2 D)`` of the bytes, which
is what the memory-bound decode attention reads.  It behaves as a bf16 cache
that holds the dequantised rows (``ops/decode.py`` states the format).  Every
step is ``kv_append_fp8`` + attention over the cache as stored --
``decode_attn_fp8``, or ``cache_attn_fp8`` (the MFMA ``cache_attn`` reading the
e4m3 rows and their scales directly) for windows of more than ``8 / G`` tokens
-- with the launch count of the bf16 cache and no scratch.  The flash prefill
is not used, so a prompt token sees the quantised keys of its own window too,
whatever the chunking.  Not available with a draft model yet.

**fp8 weights** (``weight_dtype="fp8"``, opt-in): the projection matrices --
``[Wq; Wk; Wv]``, ``Wo``, ``[W1; W3]``, ``W2`` and the LM head -- are held as
``float8_e4m3fn`` rows with one power-of-two fp32 scale per output feature
(``ops/decode.py: weight_quantize``, the row format of the fp8 cache), ``(K +
4) / (2 K)`` of the bf16 bytes; embeddings and norm weights stay bf16.  A
session with fp8 weights is a bf16 session on a model whose projection weights
are the dequantised rows -- bit for bit, on every path.  The batch <= 8 decode
step streams the e4m3 rows in the skinny GEMMs (``csrc/decode_gemv.hip``),
which is where the halved bytes count.  Every other step -- flash prefill,
``cache_attn`` appends, ``decode_attn`` windows of more than one token,
``score``, batch > 8 -- dequantises each matrix into one session-owned bf16
scratch (``w_dequant``) just before its library GEMM, so there it costs a
launch and a write per matrix.  Composes with ``kv_dtype="fp8"``, ``ragged``,
``prefill_chunk``, the device sampler and the graph (the scratch is static).
Not available with a draft model yet.

**Paged cache** (``kv_layout="paged"``, opt-in, with ``num_pages``): instead of one ``Lmax``-row slab per slot,
``k, v: [num_layers, P, Hkv, 256, D]`` are pools of ``P`` pages of 256 rows (either row format; an fp8 pool has
``k_scale, v_scale: [num_layers, P, Hkv, 256]``), and a device int32 ``block_table [B, NB]``, ``NB = ceil(Lmax /
256)``, says which page holds positions ``256 j .. 256 j + 255`` of sequence ``b`` (``-1``: none; page ``p`` means
page ``p`` of every layer's pool; ``ops/decode.py`` states the format).  A sequence costs the pages it uses, not its
worst-case context.  A page is ``decode_attn``'s key chunk and four of ``cache_attn``'s key tiles, so every cache
kernel takes the table with one lookup per chunk / per four tiles and runs the slab kernel's arithmetic on the same
rows: a paged session's tokens and logits are the slab session's, bit for bit.  The allocator lives on the host
(:class:`KVCache`: a mirror of the table, a free list, one reference count per page):

* pages are allocated from the length mirror *before* the launch that needs them -- prefill, append and chunked
  prefill reserve up to ``len + n``, a host-sampled decode step ``len + 1`` for the active sequences, and the device
  sampler ``min(len + sync_every, max_len)`` before each run of replays (it does not know on the host which sequences
  have finished; at most one page per sequence too many, given back when ``generate`` returns).  The table is a
  static device tensor updated in stream order, like ``step``: the graph is captured once and nothing new syncs;
* a pool that runs out raises ``RuntimeError`` (pages needed, pages free) before the call that needed the pages has
  launched or changed anything, and the session stays usable.  That holds per call: a ``generate`` that runs out
  part-way raises with the prompt and the tokens so far in the cache.  ``num_pages=None`` means ``batch * NB``, which
  is never short;
* ``reset_slot``, ``reset`` and ``truncate`` give back the pages wholly past the new length;
* ``fork_slot(src, dst)`` (ragged, ``dst`` empty) is prefix sharing: ``dst`` takes ``src``'s length, shares every
  page wholly below it by reference count and gets a private copy of the partial last page.  Appends only write at
  or past a sequence's own length, so a shared page is never written; ``truncate`` to a length inside a shared page
  first gives the slot a private copy.  A page returns to the pool when its last holder lets go.

The kernels do not trust the table any more than ``pos``: readers clamp a page id into the pool, an append without a
valid entry writes nothing (a ragged prefill's pad tokens past a sequence's reserved pages are dropped that way).
Composes with ``kv_dtype="fp8"``, ``weight_dtype="fp8"``, ``ragged``, ``prefill_chunk``, both samplers and the
graph.  Not available with a draft model or prompt lookup yet.

On the CPU, in fp32, or with the reference ablations (post-norm, no RMSNorm,
non-SwiGLU FFN) the same session runs the oracle math over the same cache
(with fp8 weights: on a copy of the model that holds the dequantised rows).

**One engine, two position layouts.**  The host side is written once, as "the
first ``n[i]`` tokens of ``ids[i]`` go to sequence ``rows[i]``", and every
kernel above places, rotates and attends sequence ``b`` from ``pos[b * stride]``.
The default session keeps one int32 for the whole batch (``cache.pos [1]``,
stride 0) and always appends whole windows: ``n[i] == T``.  A step in which
every sequence takes the whole window ends in ``pos += T`` and reads the logits
of the last token, whatever the layout; only a step whose lengths really differ
builds a device ``step`` / ``last`` pair.

**Ragged batches** (``DecodeSession(..., ragged=True)``) keep one int32 per
sequence (``cache.pos [B]``, stride 1, host mirror ``cache.lengths``).  So

* ``prefill(ids, lengths)`` takes right-padded prompts of different lengths and
  returns each sequence's logits after its own last token.  On an empty cache
  it is still one causal flash prefill over the padded window plus one
  ``kv_append`` (right padding under a causal mask cannot reach a valid token),
  with the hidden rows gathered at ``lengths - 1`` before the LM head.
* ``decode(ids, active)`` advances only the active sequences: inside the
  captured graph the step is ``pos += step`` with ``step`` a static device
  int32 ``[B]`` filled before the replay, so the graph is still captured once.
* ``reset_slot(b)`` / ``prefill_slot(b, ids)`` give one slot to a new request
  while the others go on: the single-sequence prefill runs on the views
  ``cache.k[:, b:b+1]``, ``cache.v[:, b:b+1]``, ``cache.pos[b:b+1]`` (contiguous
  slabs in the layout above, same addresses, so the graph stays valid).
* ``generate`` takes a list of 1-D prompts and returns a list of 1-D tensors,
  each ending with its first EOS; a finished sequence becomes inactive.

**One device sampler.**  ``generate(sampler="device")`` and the request engine (``models/serving.py``) share one
state (``_sampler_state``): a ``SamplingTable`` with every sampling parameter per slot, and one captured step --
decode -> [``logit_process_rows``] -> ``sample_rows`` -> [``token_commit_rows``] -- per set of structural switches
(penalty table, log-probs, bias).  ``generate`` fills every slot with the call's values, one seed and the row as the
Philox row word, and bounds the count on the host; the engine fills a slot per request.  Values never capture.
Every graph of this module is captured by ``_capture_graph``.

Cache rows at and past ``pos[b]`` may hold pad-token (or inactive-step) values.
They are never visible -- every read of sequence ``b`` stops at ``pos[b]`` plus
its own new tokens -- and are overwritten as the sequence grows.

**Speculative decoding** is one round engine with two proposers, each round
captured into one graph with no host sync inside: :class:`SpeculativeSession`
drafts with a second model (its own ragged session and cache), and
:class:`PromptLookupSession` drafts from the sequence's own history
(``lookup_draft``: the continuation of the most recent earlier occurrence of
the last few tokens), which needs no second model, cache or decode step.
Either way the target scores the ``K + 1`` window in one pass and
``spec_verify_step`` keeps the drafts that stand; greedy output is the
target's own, sampled output is distributed as the target's.  Neither
composes with the fp8 cache, fp8 weights or the paged cache yet.
"""

from __future__ import annotations

import copy
import math
import os

import torch
from torch import Tensor

from ..ops import reference as F
from ..ops.decode import KV_PAGE  # rows of a page of the paged cache (csrc/kv_cache.h)

# decode steps of up to this many sequences run on the fused skinny-GEMM kernels (they take up to 16 -- one MFMA
# column block -- but every workgroup re-normalises all rows in its prologue, so past ~12 rows the library
# GEMMs (hipBLASLt) win: GPT-2-small at 16 sequences 0.737 vs 0.699 ms, at 8 0.499 vs 0.672)
_GEMV_MAX_BATCH = int(os.environ.get("BPE_DECODE_GEMV_MAX_BATCH", "8"))


# A window appended to a filled cache runs on cache_attn (one pass over the layers) from this many query rows per KV
# head (G * T) on; below it, on decode_attn steps of 8 // G tokens.  decode_attn takes at most 8 rows, so 9 sends
# it exactly the windows it serves in one step (speculative verification), bit for bit as before cache_attn.
# Measured at 9 rows, the first window that needs two decode_attn steps (profiles/bench/append_prefill.log, 512
# tokens cached): GPT-2-small 2.167 -> 1.738 ms at batch 1, 2.108 -> 1.441 at batch 8; no shape lost, so 9 it is.
_CACHE_ATTN_MIN_ROWS = 9


def _chunks(T: int, prefill_chunk: int | None) -> list[tuple[int, int]]:
    """``(t0, w)`` pieces of a ``T``-token window, each of at most ``prefill_chunk`` tokens (``None``: the whole)."""
    c = T if prefill_chunk is None else max(1, min(prefill_chunk, T))
    return [(t0, min(c, T - t0)) for t0 in range(0, T, c)]


def _append_plan(T: int, G: int, filled: bool, prefill_chunk: int | None = None,
                 flash: bool = True) -> list[tuple[int, int, str]]:
    """Steps ``(t0, w, kind)`` in which a window of ``T`` tokens is appended: tokens ``t0 .. t0 + w - 1`` in one pass
    over the layers whose attention is ``kind``: ``"flash"`` (empty cache: the training kernel, causal inside the
    window), ``"cache"`` (``cache_attn`` over the cache) or ``"decode"`` (``decode_attn``, ``G * w <= 8``).
    ``filled``: some sequence already holds tokens.  ``prefill_chunk`` bounds ``w``.  ``flash=False`` (an fp8 cache)
    never plans ``"flash"``: a token always attends to the cache as stored, its own window included."""
    assert T >= 1 and G >= 1
    plan = []
    for t0, w in _chunks(T, prefill_chunk):
        if flash and t0 == 0 and not filled and w > 1:
            plan.append((t0, w, "flash"))
        elif G * w >= _CACHE_ATTN_MIN_ROWS:
            plan.append((t0, w, "cache"))
        else:
            d = max(1, 8 // G)
            plan += [(t0 + u, min(d, w - u), "decode") for u in range(0, w, d)]
    return plan


def _packed_groups(n: list[int], budget: int | None) -> list[list[int]]:
    """Indices ``0 .. len(n) - 1`` cut, in order, into groups whose token counts ``n[i]`` sum to at most ``budget``
    (``None``: one group).  A sequence is never split: one longer than the budget is a group of its own."""
    groups, tot = [], 0
    for i, x in enumerate(n):
        if groups and (budget is None or tot + x <= budget):
            groups[-1].append(i)
            tot += x
        else:
            groups.append([i])
            tot = x
    return groups


def _capture_graph(device, run, restore):
    """``run`` captured into a HIP graph -> ``(graph, what run returned inside the capture)``: a warm-up run on a side
    stream (first-use allocations and lazy initialisation must not happen inside a capture), then the capture on the
    current stream -- one stream, so the graph has no parallel branches.  ``restore`` puts back what the warm-up run
    wrote and the caller needs as it was; it runs after the warm-up and again after the capture (which executes
    nothing, but the invariant stays explicit)."""
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream(device).wait_stream(s)
    restore()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    restore()
    return g, out


def _gemv_ok(m: int, k: int) -> bool:
    """Mirror of ``gemv_ok`` (csrc/decode_gemv.hip): rows x K that the skinny kernels take."""
    if m < 1 or k % 8:
        return False
    mfma = m <= 16 and k % 32 == 0 and m * (k + 8) * 2 + 4352 <= 160 * 1024
    if m > 8:
        return mfma
    rows = 1 << (m - 1).bit_length()  # the VALU kernel's LDS holds m rounded up to 1, 2, 4 or 8 rows
    return rows * k * 2 <= 160 * 1024 or mfma




class KVCache:
    """Per-layer K/V caches ``[L, B, Hkv, Lmax, D]`` plus the device-side fill position: one int32 shared by the
    batch, or with ``ragged`` one per sequence (``pos [B]``, host mirror ``lengths``).

    ``kv_dtype="fp8"``: ``k`` / ``v`` are ``float8_e4m3fn`` bytes and ``k_scale`` / ``v_scale [L, B, Hkv, Lmax]`` hold
    one power-of-two fp32 scale per row (``ops/decode.py`` states the format); ``dtype`` is then only the dtype in
    which :meth:`read` hands rows back.

    ``kv_layout="paged"``: ``k`` / ``v`` (and the fp8 scales) are pools ``[L, P, Hkv, 256, D]`` (``[L, P, Hkv, 256]``)
    of ``num_pages`` pages -- page ``p`` means page ``p`` of every layer's pool -- behind the device ``block_table
    [B, NB]`` (int32, ``NB = ceil(max_len / 256)``, ``-1`` = unallocated; ``ops/decode.py`` states the format).  The
    host keeps a mirror of the table, a free list and one reference count per page.  :meth:`reserve` allocates, from
    the length mirror and before the launch that needs the pages; :meth:`release` gives back the pages wholly past a
    length; :meth:`fork` lets a second sequence share a prefix by reference.  Table updates go into the static
    device tensor in stream order, so a captured graph that reads it stays valid.  ``num_pages=None`` means ``batch *
    NB``, which is never short."""

    def __init__(self, num_layers: int, batch: int, num_kv_heads: int, max_len: int, head_dim: int, device=None,
                 dtype=torch.bfloat16, ragged: bool = False, kv_dtype: str = "bf16", kv_layout: str = "slab",
                 num_pages: int | None = None):
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype: 'bf16' or 'fp8', got {kv_dtype!r}")
        if kv_layout not in ("slab", "paged"):
            raise ValueError(f"kv_layout: 'slab' or 'paged', got {kv_layout!r}")
        if num_pages is not None and kv_layout != "paged":
            raise ValueError("num_pages needs kv_layout='paged'")
        self.kv_layout = kv_layout
        self.paged = kv_layout == "paged"
        shape = (num_layers, batch, num_kv_heads, max_len, head_dim)
        if self.paged:
            self.pages_per_seq = nb = (max_len + KV_PAGE - 1) // KV_PAGE
            self.num_pages = batch * nb if num_pages is None else int(num_pages)
            if self.num_pages < 1:
                raise ValueError(f"num_pages: at least one page, got {num_pages!r}")
            shape = (num_layers, self.num_pages, num_kv_heads, KV_PAGE, head_dim)
            self.block_table = torch.full((batch, nb), -1, device=device, dtype=torch.int32)
            self._table = [[-1] * nb for _ in range(batch)]  # host mirror of block_table
            self._free = list(range(self.num_pages - 1, -1, -1))  # popped from the end: lowest page first
            self._ref = [0] * self.num_pages  # table entries that name the page
        self.kv_dtype = kv_dtype
        self.fp8 = kv_dtype == "fp8"
        self.dtype = dtype
        if self.fp8:
            self.k = torch.zeros(shape, device=device, dtype=torch.float8_e4m3fn)
            self.v = torch.zeros(shape, device=device, dtype=torch.float8_e4m3fn)
            self.k_scale = torch.ones(shape[:-1], device=device, dtype=torch.float32)
            self.v_scale = torch.ones(shape[:-1], device=device, dtype=torch.float32)
        else:
            self.k = torch.zeros(shape, device=device, dtype=dtype)
            self.v = torch.zeros(shape, device=device, dtype=dtype)
        self.ragged = ragged
        self.pos = torch.zeros(batch if ragged else 1, device=device, dtype=torch.int32)  # tokens already cached
        self._len = [0] * batch  # host mirror of pos (never read back), per sequence: all equal unless ragged
        self.max_len = max_len
        self.batch = batch

    def view(self, b: int | None = None) -> "KVView":
        """What a forward pass runs on: the whole batch, or slot ``b`` alone."""
        return KVView(self, b)

    @property
    def length(self) -> int:
        """Tokens cached; ragged: of the longest sequence."""
        return max(self._len)

    @property
    def lengths(self) -> list[int] | None:
        """Ragged: tokens cached per sequence (the live list); otherwise ``None``."""
        return self._len if self.ragged else None

    def reset(self) -> None:
        self.pos.zero_()
        self._len = [0] * self.batch
        if self.paged:
            self.release(range(self.batch), [0] * self.batch)

    # ---- paged layout: the allocator (host side).  On a slab cache reserve / release / cut do nothing and the page
    # counts are 0; fork is refused.
    @property
    def pages_free(self) -> int:
        return len(self._free) if self.paged else 0

    @property
    def pages_in_use(self) -> int:
        return self.num_pages - len(self._free) if self.paged else 0

    @staticmethod
    def _npages(n: int) -> int:
        return (n + KV_PAGE - 1) // KV_PAGE

    def _take(self, need: int) -> None:
        if need > len(self._free):
            raise RuntimeError(f"KV cache out of pages: {need} needed, {len(self._free)} free "
                               f"(of {self.num_pages}; a page is {KV_PAGE} tokens of one sequence)")

    def _alloc(self) -> int:
        p = self._free.pop()
        self._ref[p] = 1
        return p

    def _drop(self, p: int) -> None:
        self._ref[p] -= 1
        if self._ref[p] == 0:
            self._free.append(p)

    def _sync_table(self) -> None:
        """The host mirror -> the static device table, in stream order (like the decode step's ``step``)."""
        self.block_table.copy_(torch.tensor(self._table, dtype=torch.int32))

    def reserve(self, rows, upto) -> None:
        """Sequence ``rows[i]`` is about to hold up to ``upto[i]`` tokens (clamped to ``max_len``): allocate the pages
        it lacks.  Raises ``RuntimeError`` (pages needed, pages free) before anything is changed."""
        if not self.paged:
            return
        want = [(r, j) for r, n in zip(rows, upto) for j in range(self._npages(min(int(n), self.max_len)))
                if self._table[r][j] < 0]
        if not want:
            return
        self._take(len(want))
        for r, j in want:
            self._table[r][j] = self._alloc()
        self._sync_table()

    def release(self, rows, lengths) -> None:
        """Give back the pages of sequence ``rows[i]`` that lie wholly past its first ``lengths[i]`` tokens (a page
        returns to the pool when no table entry names it any more)."""
        if not self.paged:
            return
        changed = False
        for r, n in zip(rows, lengths):
            for j in range(self._npages(int(n)), self.pages_per_seq):
                if self._table[r][j] >= 0:
                    self._drop(self._table[r][j])
                    self._table[r][j] = -1
                    changed = True
        if changed:
            self._sync_table()

    def _copy_page(self, src: int, dst: int) -> None:
        for t in (self.k, self.v) + ((self.k_scale, self.v_scale) if self.fp8 else ()):
            t[:, dst] = t[:, src]

    def cut(self, rows, lengths) -> None:
        """Sequence ``rows[i]`` is cut back to ``lengths[i]`` tokens: :meth:`release` what lies wholly past them, and
        where the new end lies inside a page that another sequence still shares, give this one a private copy of it
        -- its next tokens will be written there.  The sequences are taken in order, on the reference counts as the
        cuts before them leave them: of several holders that cut into the same page the last keeps the original, and
        a page that all its holders let go in this call counts as free for the copies.  Raises ``RuntimeError``
        before anything is changed."""
        if not self.paged:
            return
        rows, lengths = list(rows), [int(n) for n in lengths]
        ref, freed, cow = list(self._ref), 0, []  # the call played through on a copy of the counts
        for r, n in zip(rows, lengths):
            for j in range(self._npages(n), self.pages_per_seq):
                p = self._table[r][j]
                if p >= 0:
                    ref[p] -= 1
                    freed += ref[p] == 0
        for r, n in zip(rows, lengths):
            p = self._table[r][n // KV_PAGE] if n % KV_PAGE else -1
            if p >= 0 and ref[p] > 1:
                ref[p] -= 1
                cow.append((r, n // KV_PAGE))
        self._take(max(len(cow) - freed, 0))
        self.release(rows, lengths)
        if not cow:
            return
        for r, j in cow:
            old, new = self._table[r][j], self._alloc()
            self._copy_page(old, new)
            self._drop(old)
            self._table[r][j] = new
        self._sync_table()

    def fork(self, src: int, dst: int) -> None:
        """Prefix sharing: the empty sequence ``dst`` becomes a copy of ``src``.  It takes ``src``'s length, shares
        (by reference count) every page wholly below it, and gets a private copy -- all layers, K, V and scales --
        of the partial last page.  Appends only write at or past a sequence's own length, so a shared page is never
        written (``truncate`` into one unshares it first)."""
        assert self.paged and self.ragged, "fork needs a ragged session with kv_layout='paged'"
        assert src != dst and self._len[dst] == 0, "fork: dst must be another, empty slot"
        n = self._len[src]
        full, part = n // KV_PAGE, int(n % KV_PAGE > 0)
        held = sum(p >= 0 and self._ref[p] == 1 for p in self._table[dst])  # (its own, freed first: none if emptied)
        self._take(max(part - held, 0))
        self.release([dst], [0])
        for j in range(full):
            p = self._table[dst][j] = self._table[src][j]
            self._ref[p] += 1
        if part:
            p = self._table[dst][full] = self._alloc()
            self._copy_page(self._table[src][full], p)
        self._sync_table()
        self._len[dst] = n
        self.pos[dst : dst + 1].fill_(n)

    def _pool(self, t: Tensor, rows: list[int], n: int) -> Tensor:
        """Oracle path: the first ``n`` rows of the sequences ``rows`` of one layer's pool, through the table."""
        from ..ops.decode import paged_gather

        return paged_gather(t, torch.tensor([self._table[r] for r in rows]), self.max_len)[:, :, :n]

    def advance(self, rows, steps) -> None:
        """Host mirror: sequence ``rows[i]`` grew by ``steps[i]`` tokens."""
        for r, n in zip(rows, steps):
            self._len[r] += int(n)

    def nbytes(self) -> int:
        """Bytes of K and V, the fp8 cache's scales included: ``(D + 4) / (2 D)`` of the bf16 cache's."""
        n = 2 * self.k.numel() * self.k.element_size()  # (paged: of the pool)
        return n + 2 * self.k_scale.numel() * 4 if self.fp8 else n

    def write(self, layer: int, row: int, lo: int, hi: int, k: Tensor, v: Tensor) -> None:
        """Oracle path: ``k`` / ``v [Hkv, hi - lo, D]`` become rows ``lo .. hi - 1`` of sequence ``row`` (fp8: rounded
        to bf16, as the bf16 cache would hold them, then quantised).  Paged: page by page through the table;
        rows without a page are dropped, as the kernels drop them."""
        if self.paged:
            a = lo
            while a < hi:
                b = min(hi, (a // KV_PAGE + 1) * KV_PAGE)
                page = self._table[row][a // KV_PAGE]
                if page >= 0:  # (no page: dropped, as the kernels drop it -- an inactive sequence's token, a pad token)
                    self._write(layer, page, a % KV_PAGE, a % KV_PAGE + b - a, k[:, a - lo : b - lo],
                                v[:, a - lo : b - lo])
                a = b
            return
        self._write(layer, row, lo, hi, k, v)

    def _write(self, layer: int, row: int, lo: int, hi: int, k: Tensor, v: Tensor) -> None:
        if not self.fp8:
            self.k[layer, row, :, lo:hi] = k.to(self.k.dtype)
            self.v[layer, row, :, lo:hi] = v.to(self.v.dtype)
            return
        from ..ops.decode import kv_quantize_reference

        self.k[layer, row, :, lo:hi], self.k_scale[layer, row, :, lo:hi] = kv_quantize_reference(k.to(torch.bfloat16))
        self.v[layer, row, :, lo:hi], self.v_scale[layer, row, :, lo:hi] = kv_quantize_reference(v.to(torch.bfloat16))

    def read(self, layer: int, rows: list[int], n: int, dtype) -> tuple[Tensor, Tensor]:
        """Oracle path: the first ``n`` rows of the sequences ``rows`` as ``dtype`` (fp8: dequantised, exactly)."""
        if self.paged:
            get = lambda t: self._pool(t[layer], rows, n)
        else:
            get = lambda t: t[layer, rows, :, :n]
        if not self.fp8:
            return get(self.k).to(dtype), get(self.v).to(dtype)
        from ..ops.decode import kv_dequantize_reference as deq

        return deq(get(self.k), get(self.k_scale), dtype), deq(get(self.v), get(self.v_scale), dtype)


class KVView:
    """The cache as one pass over the layers sees it -- ``k`` / ``v [L, n, Hkv, Lmax, D]``, ``pos`` and, for fp8, the
    row ``scales`` -- of the whole batch or of one slot (``cache.k[:, b:b+1]`` ...: contiguous slabs at the same
    addresses, so a captured graph stays valid).  Every HIP op call that depends on the cache format is made here:
    the engine appends and attends, and does not know what a row is stored as, nor where.  ``h`` is the HIP ops
    handle, ``rope`` the session's ``(cos, sin, use_rope)``.  A paged cache's view holds the whole pools, and the slot
    is a row of the block table (``block_table[b:b+1]``); ``pg`` is then the ``(block_table, max_len)`` tail of every
    op call, and empty for slabs, whose calls are what they always were."""

    def __init__(self, cache: KVCache, b: int | None = None):
        one = (lambda t: t) if b is None or cache.paged else (lambda t: t[:, b : b + 1])
        self.cache = cache
        self.k, self.v = one(cache.k), one(cache.v)
        self.pos = cache.pos if b is None else cache.pos[b : b + 1]
        self.scales = (one(cache.k_scale), one(cache.v_scale)) if cache.fp8 else None
        self.pg = ()
        if cache.paged:
            self.pg = (cache.block_table if b is None else cache.block_table[b : b + 1], cache.max_len)
        self.n = cache.batch if b is None else 1  # sequences

    def append(self, h, qkv: Tensor, li: int, T: int, H: int, rope) -> Tensor:
        """RoPE and cache write of layer ``li``'s fused-QKV rows, ``T`` new tokens per sequence; returns the roped q."""
        B = self.n
        if self.scales is None:
            return h.kv_append(qkv, self.k[li], self.v[li], rope[0], rope[1], self.pos, B, T, H, rope[2], *self.pg)
        ks, vs = self.scales
        return h.kv_append_fp8(qkv, self.k[li], self.v[li], ks[li], vs[li], rope[0], rope[1], self.pos, B, T, H, rope[2],
                               *self.pg)

    def attend(self, h, q: Tensor, li: int, T: int, H: int, kind: str, combine: bool = True) -> Tensor:
        """Attention of the appended tokens over the cache as stored: ``kind`` ``"cache"`` (``cache_attn``; fp8:
        ``cache_attn_fp8``) or ``"decode"`` (``decode_attn``; ``combine=False``: its split partials)."""
        k, v, pos = self.k[li], self.v[li], self.pos
        scale = 1.0 / math.sqrt(k.shape[-1])
        if self.scales is None:
            if kind == "cache":
                return h.cache_attn(q, k, v, pos, H, scale, T, *self.pg)
            return h.decode_attn(q, k, v, pos, H, scale, combine, T, *self.pg)
        ks, vs = self.scales[0][li], self.scales[1][li]
        if kind == "cache":
            return h.cache_attn_fp8(q, k, v, ks, vs, pos, H, scale, T, *self.pg)
        return h.decode_attn_fp8(q, k, v, ks, vs, pos, H, scale, combine, T, *self.pg)

    def append_packed(self, h, qkv: Tensor, li: int, H: int, rope, pk) -> Tensor:
        """:meth:`append` of packed rows (``ops/decode.py``, "Packed prefill"; ``pk`` a ``PackedPrompts``): each
        sequence to its own slot of the whole cache's view, at that slot's position."""
        assert self.n == self.cache.batch, "a packed pass runs on the whole cache"
        if self.scales is None:
            return h.kv_append_packed(qkv, self.k[li], self.v[li], rope[0], rope[1], self.pos, pk.seq, pk.seq_host, H,
                                      rope[2], *self.pg)
        ks, vs = self.scales
        return h.kv_append_packed_fp8(qkv, self.k[li], self.v[li], ks[li], vs[li], rope[0], rope[1], self.pos, pk.seq,
                                      pk.seq_host, H, rope[2], *self.pg)

    def attend_packed(self, h, q: Tensor, li: int, H: int, pk) -> Tensor:
        """``cache_attn_packed`` (fp8: ``cache_attn_packed_fp8``) of the packed rows just appended."""
        k, v = self.k[li], self.v[li]
        scale, work = 1.0 / math.sqrt(k.shape[-1]), pk.work(H // k.shape[1])
        if self.scales is None:
            return h.cache_attn_packed(q, k, v, self.pos, pk.seq, pk.seq_host, work, H, scale, *self.pg)
        return h.cache_attn_packed_fp8(q, k, v, self.scales[0][li], self.scales[1][li], self.pos, pk.seq, pk.seq_host,
                                       work, H, scale, *self.pg)

    def decode_qkv(self, h, xr: Tensor, xd, ln1: Tensor, eps: float, wqkv: Tensor, li: int, H: int, rope, ws=()):
        """QKV step of the skinny decode route -> ``(q, x + xd)``: the fused ``decode_qkv`` (projection, RoPE, cache
        write), or for fp8 ``decode_gemv`` with the plain epilogue followed by :meth:`append` (a row's amax spans
        several workgroups of the fused epilogue).  ``ws``: ``(w_scale,)`` when ``wqkv`` is an e4m3 matrix."""
        if self.scales is None:
            tail = ws if not self.pg else (ws[0] if ws else None, *self.pg)  # (w_scale precedes the table)
            return h.decode_qkv(xr, xd, ln1, eps, wqkv, self.k[li], self.v[li], rope[0], rope[1], self.pos, H, rope[2],
                                *tail)
        qkv, s = h.decode_gemv(xr, xd, ln1, eps, wqkv, 0, *ws)
        return self.append(h, qkv, li, 1, H, rope), s


_W8_PROJECTIONS = (("attn", ("q_proj", "k_proj", "v_proj", "output_proj")), ("ffn", ("w1", "w2", "w3")))


def _dequantised_copy(model):
    """A copy of ``model`` whose five projection families -- Wq / Wk / Wv, Wo, W1 / W3, W2 and the LM head -- hold
    ``weight_dequantize(weight_quantize(W))`` in the model's dtype: what a session with fp8 weights computes with.
    (Rows are quantised one by one, so the separate matrices give what the concatenated ones do.)  Embeddings and norm
    weights are the originals' values; a tied embedding is untied, the head alone being quantised."""
    from ..ops.decode import weight_dequantize, weight_quantize

    def deq(lin) -> None:
        w = lin.weight.detach()
        lin.weight = torch.nn.Parameter(weight_dequantize(*weight_quantize(w), w.dtype), requires_grad=False)

    m = copy.deepcopy(model)
    for layer in m.layers:
        for part, names in _W8_PROJECTIONS:
            for name in names:
                lin = getattr(getattr(layer, part), name, None)
                if lin is not None:
                    deq(lin)
    if m.lm_head.weight is m.token_embeddings.weight:
        m.token_embeddings.weight = torch.nn.Parameter(m.token_embeddings.weight.detach().clone(), requires_grad=False)
    deq(m.lm_head)
    return m


def _top_k_logits(logits: Tensor, top_k: int | None) -> Tensor:
    """``logits`` with everything outside each row's ``top_k`` largest set to ``-inf`` (``None`` / 0 / >= V: as is)."""
    if not top_k or top_k >= logits.shape[-1]:
        return logits
    idx = logits.topk(int(top_k), dim=-1).indices
    return torch.full_like(logits, -math.inf).scatter_(-1, idx, logits.gather(-1, idx))


def _sample(logits: Tensor, temperature: float, top_p: float | None, generator, top_k: int | None = None) -> Tensor:
    """Next token per row of ``logits [B, V]`` (greedy when ``temperature <= 0``); returns ``[B]`` int64.  ``top_k``
    is applied before ``top_p``."""
    logits = logits.float()
    if temperature <= 0:
        return logits.argmax(-1)
    logits = _top_k_logits(logits, top_k)
    probs = torch.softmax(logits / temperature, dim=-1)
    if top_p is not None and top_p < 1.0:
        sp, si = probs.sort(dim=-1, descending=True)
        keep = sp.cumsum(-1) - sp < top_p
        sp = sp * keep
        probs = torch.zeros_like(probs).scatter_(-1, si, sp)
        probs = probs / probs.sum(-1, keepdim=True)
    return torch.multinomial(probs, 1, generator=generator).squeeze(-1)


class _Controls:
    """The sampling controls of one ``generate`` call that are not at their defaults (``ops/sampling.py``, "Sampling
    controls"): ``penal`` -- a penalty is on, so the token history is kept; ``proc`` -- the sampler reads processed
    logits; ``logprobs`` -- the log-sum-exp and the emitted tokens' log-probs are wanted."""

    def __init__(self, rp: float, pp: float, fp: float, bias: Tensor | None, logprobs: bool):
        self.rp, self.pp, self.fp, self.bias, self.logprobs = float(rp), float(pp), float(fp), bias, bool(logprobs)
        self.penal = self.rp != 1.0 or self.pp != 0.0 or self.fp != 0.0
        self.proc = self.penal or bias is not None


def _controls(V: int, device, repetition_penalty, presence_penalty, frequency_penalty, logit_bias,
              return_logprobs) -> _Controls | None:
    """``None`` when every control is at its default (then nothing new runs), else the :class:`_Controls`, with
    ``logit_bias`` -- a ``{token: value}`` dict or a ``[V]`` tensor -- as an fp32 ``[V]`` tensor on ``device``."""
    if not float(repetition_penalty) > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
    bias = None
    if isinstance(logit_bias, dict):
        if logit_bias:
            bad = [t for t in logit_bias if not 0 <= int(t) < V]
            if bad:
                raise ValueError(f"logit_bias: token {bad[0]} outside the vocabulary of {V}")
            bias = torch.zeros(V, dtype=torch.float32)
            for t, v in logit_bias.items():
                bias[int(t)] = float(v)
            bias = bias.to(device)
    elif logit_bias is not None:
        if tuple(logit_bias.shape) != (V,):
            raise ValueError(f"logit_bias: a {{token: value}} dict or a [{V}] tensor, got {tuple(logit_bias.shape)}")
        bias = logit_bias.detach().to(device, torch.float32).contiguous()
    c = _Controls(repetition_penalty, presence_penalty, frequency_penalty, bias, return_logprobs)
    return c if c.proc or c.logprobs else None


class _HostControls:
    """The controls around the host sampler: the history, the emitted tokens and their log-probs on the logits'
    device, ``logit_process`` before ``_sample`` and ``token_commit`` after it."""

    def __init__(self, ctl: _Controls, ids: Tensor, lengths, V: int, max_new_tokens: int):
        from ..ops import sampling

        B, dev = ids.shape[0], ids.device
        self.ctl, self.ops = ctl, sampling
        self.hist = sampling.prompt_hist(ids, lengths, V) if ctl.penal else None
        self.toks = torch.full((B, max(max_new_tokens, 1)), -1, dtype=torch.long, device=dev)
        self.rng = torch.zeros(2, dtype=torch.long, device=dev)  # (unused seed, the column)
        self.lse = torch.empty(B, dtype=torch.float32, device=dev) if ctl.logprobs else None
        self.logprob = torch.full(self.toks.shape, math.nan, dtype=torch.float32, device=dev) if ctl.logprobs else None
        self.raw = None

    def process(self, logits: Tensor) -> Tensor:
        """The logits the sampler reads (the processed copy, or ``logits`` itself with log-probs alone)."""
        c = self.ctl
        if logits.dtype not in (torch.bfloat16, torch.float32):
            logits = logits.float()
        self.raw = logits = logits.contiguous()
        out = torch.empty_like(logits) if c.proc else None
        self.ops.logit_process(logits, self.hist, c.bias, c.rp, c.pp, c.fp, out, self.lse)
        return out if c.proc else logits

    def commit(self, i: int, nxt: Tensor, idle=None) -> None:
        """Token ``i`` of every row (``idle [B]`` bool: rows that emit nothing) into the history and the log-probs."""
        c = self.ctl
        self.toks[:, i] = nxt if idle is None else torch.where(idle.to(nxt.device), torch.full_like(nxt, -1), nxt)
        if c.penal or c.logprobs:
            self.rng[1] = i
            self.ops.token_commit(self.toks, self.rng, self.hist, self.raw, self.lse, self.logprob)


class DecodeSession:
    """Incremental decoding of ``batch`` sequences with a KV cache.

    ``prefill(ids [B, T])`` and ``decode(ids [B])`` return the next-token logits ``[B, V]`` of the last position.
    With ``use_graph`` (GPU only) the decode step is captured into a HIP graph on first use and replayed after.

    One engine serves both position layouts: ``_append`` and ``decode`` work per sequence, and the default session is
    the caller whose sequences all take the whole window.  With ``ragged`` every sequence has its own position:
    ``prefill`` takes right-padded ``ids`` with host ``lengths``, ``decode`` an ``active`` mask, ``reset_slot`` /
    ``prefill_slot`` hand one slot to a new request, and ``generate`` takes a list of prompts of different lengths
    (module docstring).

    ``prefill`` / ``prefill_slot`` on a cache that already holds tokens (a second turn, a slot with a kept prefix)
    is one pass over the layers for the whole window (``cache_attn``), as on an empty cache.  ``prefill_chunk=c``
    cuts every prefill or append, ragged or not, into chunks of at most ``c`` tokens, which bounds activation memory
    by ``B * c`` rows.  ``prefill_slots`` hands several slots to new requests in one pass over the layers on their
    packed prompts (no padding: ``kv_append_packed`` + ``cache_attn_packed``, each sequence at its slot's own position).

    ``kv_dtype="fp8"`` keeps the cache as e4m3 rows with one power-of-two scale each (``csrc/kv_fp8.hip``;
    ``ops/decode.py`` states the format): ``(D + 4) / (2 D)`` of the bf16 cache's bytes.  Every step appends with
    ``kv_append_fp8`` and attends to the cache as stored, its own window included -- ``decode_attn_fp8`` up to ``8 /
    G`` tokens, ``cache_attn_fp8`` (``cache_attn`` reading the e4m3 rows directly) beyond; the flash prefill is never used,
    so prefill, chunked prefill and decode have one semantics, that of a bf16 cache holding the dequantised rows.  At
    batch <= 8 the QKV projection is ``decode_gemv`` followed by ``kv_append_fp8`` (a row's amax spans several
    workgroups of the fused ``decode_qkv`` epilogue): 6 launches per layer instead of 5.

    ``weight_dtype="fp8"`` holds ``[Wq; Wk; Wv]``, ``Wo``, ``[W1; W3]``, ``W2`` and the LM head as e4m3 rows with one
    power-of-two scale per output feature (``ops/decode.py: weight_quantize``), ``(K + 4) / (2 K)`` of the bf16 bytes,
    and no bf16 copy of them; embeddings and norm weights stay bf16.  The session is a bf16 session on a model whose
    projection weights are the dequantised rows, bit for bit.  The batch <= 8 decode step streams the e4m3 rows in
    the skinny GEMMs; prefill, appends, ``score`` and batch > 8 dequantise each matrix into one static bf16 scratch
    (sized for the largest, reused in stream order) just before its GEMM, and pay for that.  Off the fast path the
    session runs the oracle math on a copy of the model that holds the dequantised rows.  No draft model yet.

    ``kv_layout="paged"`` keeps the cache as a pool of ``num_pages`` 256-row pages behind a block table (module
    docstring: format, allocator rules, ``RuntimeError`` on exhaustion): the same launches with the table as a
    trailing argument, the same bits.  ``cache.pages_in_use`` / ``cache.pages_free`` report the pool;
    :meth:`fork_slot` shares a prefix between slots of a ragged session.
    """

    def __init__(self, model, batch: int, max_len: int | None = None, use_graph: bool = True, ragged: bool = False,
                 prefill_chunk: int | None = None, kv_dtype: str = "bf16", weight_dtype: str = "bf16",
                 kv_layout: str = "slab", num_pages: int | None = None):
        assert prefill_chunk is None or prefill_chunk >= 1, "prefill_chunk: a positive number of tokens, or None"
        if weight_dtype not in ("bf16", "fp8"):
            raise ValueError(f"weight_dtype: 'bf16' or 'fp8', got {weight_dtype!r}")
        self.weight_dtype = weight_dtype
        self.w8 = weight_dtype == "fp8"
        self.model = model
        self.ragged = ragged
        self.prefill_chunk = prefill_chunk
        cfg = model.config
        self.batch = batch
        self.max_len = max_len or model.context_length
        blk = model.layers[0] if len(model.layers) else None
        attn = blk.attn if blk is not None else None
        self.H = attn.num_heads if attn else cfg.num_heads
        self.Hkv = attn.num_kv_heads if attn else cfg.num_heads
        self.D = attn.d_k if attn else cfg.d_model // cfg.num_heads
        if attn is not None and attn.rope is not None:
            assert self.max_len <= attn.rope.max_seq_len, "KV cache longer than the RoPE table (context_length)"
        p = model.lm_head.weight
        self.device = p.device
        self.cache = KVCache(len(model.layers), batch, self.Hkv, self.max_len, self.D, self.device, p.dtype, ragged,
                             kv_dtype, kv_layout, num_pages)
        self.fp8 = self.cache.fp8
        self.kv_layout = kv_layout
        self.fast = self._fast_ok()
        self.use_graph = use_graph and self.fast
        # ragged: per-sequence advance of the decode step (1 = active), static so that the captured graph reads it
        self._step = torch.ones(batch, device=self.device, dtype=torch.int32) if ragged and self.fast else None
        self._step_host = [1] * batch  # what _step holds
        self._graph = None
        self._samp = None  # the device sampler's table, buffers and graphs (_sampler_state)
        if self.fast:
            self._prepare_weights()
        elif self.w8:  # the definition of the feature: the oracle math on the dequantised model
            self.model = _dequantised_copy(model)

    # ------------------------------------------------------------------ setup
    def _fast_ok(self) -> bool:
        m = self.model
        if not (self.device.type == "cuda" and m.lm_head.weight.dtype == torch.bfloat16 and len(m.layers)):
            return False
        from .. import ops

        for layer in m.layers:
            if layer.use_post_norm or layer.remove_rmsnorm or layer.ffn_type != "swiglu":
                return False
        G = self.H // self.Hkv
        return self.D in ops.attention.SUPPORTED_HEAD_DIMS and G in (1, 2, 4, 8) and self.H % self.Hkv == 0

    def _prepare_weights(self) -> None:
        """``_w``: per layer ``(ln1, wqkv, wo, ln2, w13, w2, eps)``; ``_head``: the LM head.  A projection is ``(w,)``
        (bf16) or ``(w8, w_scale)`` (fp8 weights: no bf16 copy is kept) -- the trailing arguments of its skinny op."""
        from ..ops.decode import weight_quantize
        from .fused_block import _cat_weights

        pack = (lambda w: weight_quantize(w.detach())) if self.w8 else (lambda w: (w.detach(),))
        self._w = []
        for layer in self.model.layers:
            a, f = layer.attn, layer.ffn
            self._w.append((
                layer.ln1.weight.detach(), pack(_cat_weights([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight])),
                pack(a.output_proj.weight), layer.ln2.weight.detach(), pack(_cat_weights([f.w1.weight, f.w3.weight])),
                pack(f.w2.weight), layer.ln1.eps,
            ))
        self._head = pack(self.model.lm_head.weight)
        self._wscratch = None
        if self.w8:  # one bf16 scratch for the wide steps, sized for the largest matrix (static: graph-safe)
            n = max(w[0].numel() for lw in self._w for w in (lw[1], lw[2], lw[4], lw[5]))
            self._wscratch = torch.empty(max(n, self._head[0].numel()), device=self.device, dtype=torch.bfloat16)
        rope = self.model.layers[0].attn.rope
        if rope is not None:  # (cos, sin, use_rope) as the kernels take them
            self._rope = (rope.cos.float().contiguous(), rope.sin.float().contiguous(), True)
        else:  # empty tables and use_rope = False
            self._rope = (*[torch.empty(0, device=self.device, dtype=torch.float32)] * 2, False)

    def _wide(self, h, w) -> Tensor:
        """The bf16 matrix of projection ``w`` for a library GEMM: itself, or (fp8 weights) dequantised into the
        session's scratch, which the next call overwrites -- stream order keeps the GEMM in between safe."""
        if len(w) == 1:
            return w[0]
        out = self._wscratch[: w[0].numel()].view(w[0].shape)
        h.w_dequant(w[0], w[1], out)
        return out

    def weight_nbytes(self) -> int:
        """Bytes of the session's projection weights (fp8: bytes and scales; the scratch is not counted)."""
        ws = [w for lw in self._w for w in (lw[1], lw[2], lw[4], lw[5])] + [self._head] if self.fast else []
        return sum(t.numel() * t.element_size() for w in ws for t in w)

    def reset(self) -> None:
        self.cache.reset()

    @property
    def length(self) -> int:
        return self.cache.length

    # ------------------------------------------------------------------ public API
    @torch.no_grad()
    def prefill(self, ids: Tensor, lengths=None) -> Tensor:
        """Append ``ids [B, T]`` to the cache; returns the logits ``[B, V]`` after the last token.

        Ragged sessions: ``ids`` is right-padded and ``lengths [B]`` (host ints, ``1 <= lengths[b] <= T``, default
        ``T``) says how many tokens of each row count; row ``b`` of the result are the logits after token
        ``lengths[b] - 1``."""
        ids = ids.to(self.device)
        B, T = ids.shape
        assert B == self.batch, f"session batch is {self.batch}, got {B}"
        assert lengths is None or self.ragged, "per-sequence lengths need DecodeSession(..., ragged=True)"
        n = [T] * B if lengths is None else [int(x) for x in lengths]
        assert len(n) == B and all(1 <= x <= T for x in n), "lengths: one int in [1, T] per sequence"
        return self._append(ids, n, list(range(B)))

    @torch.no_grad()
    def decode(self, ids: Tensor, active=None) -> Tensor:
        """Append one token per sequence (``ids [B]``); returns the next logits ``[B, V]``.

        Ragged sessions: ``active`` (bool ``[B]``, default all) -- an inactive sequence is fed as usual, but its
        position does not advance and its logits are unspecified."""
        B = self.batch
        assert active is None or self.ragged, "an active mask needs DecodeSession(..., ragged=True)"
        step = [1] * B if active is None else [int(bool(a)) for a in torch.as_tensor(active).reshape(-1).tolist()]
        assert len(step) == B, "active: one flag per sequence"
        rows = list(range(B))
        assert all(c + s <= self.max_len for c, s in zip(self.cache._len, step)), "KV cache full"
        self.cache.reserve(rows, [c + s for c, s in zip(self.cache._len, step)])
        ids = ids.reshape(B, 1).to(self.device)
        if self._step is not None and step != self._step_host:
            # (the mask changes only when a sequence finishes or a slot is refilled)
            self._step.copy_(torch.tensor(step, dtype=torch.int32))
            self._step_host = step
        if not self.fast:
            out = self._forward_reference(ids, step, rows)
        elif not self.use_graph:
            out = self._forward_fast(ids, "decode", step=self._step)
        else:
            if self._graph is None:
                self._capture()
            self._static_ids.copy_(ids)
            self._graph.replay()
            out = self._static_logits.clone()  # the graph's output buffer is rewritten by the next replay
        self.cache.advance(rows, step)
        return out

    @torch.no_grad()
    def score(self, ids: Tensor) -> Tensor:
        """Append the window ``ids [B, T]`` like :meth:`prefill`, every sequence the whole of it, and return the
        logits of every position, ``[B, T, V]``: row ``t`` is the distribution of the token after ``ids[:, t]``.
        Routing is ``_append_plan``'s: a window of at most ``8 // G`` tokens on a filled cache is one ``decode_attn``
        step, a larger one ``cache_attn`` -- what verifying draft tokens needs."""
        ids = ids.to(self.device)
        B, T = ids.shape
        assert B == self.batch, f"session batch is {self.batch}, got {B}"
        c = self.cache
        rows = list(range(B))
        assert all(p + T <= self.max_len for p in c._len), "KV cache full"
        c.reserve(rows, [p + T for p in c._len])
        if not self.fast:  # the oracle math reads the host lengths, which therefore move chunk by chunk
            out = []
            for t0, w in _chunks(T, self.prefill_chunk):
                out.append(self._forward_reference(ids[:, t0 : t0 + w], [w] * B, rows, all_logits=True))
                c.advance(rows, [w] * B)
            return torch.cat(out, 1)
        out = [self._forward_fast(ids[:, t0 : t0 + w], kind, all_logits=True).view(B, w, -1)
               for t0, w, kind in _append_plan(T, self.H // self.Hkv, max(c._len) > 0, self.prefill_chunk, not self.fp8)]
        c.advance(rows, [T] * B)
        return out[0] if len(out) == 1 else torch.cat(out, 1)

    @torch.no_grad()
    def truncate(self, lengths) -> None:
        """Ragged sessions: cut sequence ``b`` back to its first ``lengths[b]`` tokens (at most what it holds).  The
        cache rows past the new position become invisible, like everything at and past ``pos[b]``.  A paged cache
        takes back the pages wholly past the new length; where the new end lies inside a page shared with a fork, the
        sequence first gets a private copy of that page (``RuntimeError`` if the pool has none left)."""
        assert self.ragged, "truncate needs DecodeSession(..., ragged=True)"
        n = [int(x) for x in (lengths.tolist() if isinstance(lengths, Tensor) else lengths)]
        c = self.cache
        assert len(n) == self.batch and all(0 <= x <= p for x, p in zip(n, c._len)), \
            "lengths: one int per sequence, at most its cached length"
        c.cut(range(self.batch), n)
        c.pos.copy_(torch.tensor(n, dtype=torch.int32))
        c._len[:] = n

    @torch.no_grad()
    def reset_slot(self, b: int) -> None:
        """Ragged sessions: empty slot ``b`` for a new request; the other sequences are untouched.  A paged cache
        takes its pages back (a page shared with a fork stays until its last holder lets go)."""
        assert self.ragged, "slots need DecodeSession(..., ragged=True)"
        self.cache.pos[b : b + 1].zero_()
        self.cache.lengths[b] = 0
        self.cache.release([b], [0])

    @torch.no_grad()
    def fork_slot(self, src: int, dst: int) -> None:
        """Prefix sharing (ragged sessions, ``kv_layout="paged"``): the empty slot ``dst`` becomes a copy of sequence
        ``src`` without prefilling or storing the common prefix again -- it takes ``src``'s length, shares every full
        page below it by reference and gets a private copy of the partial last page (:meth:`KVCache.fork`).  Decode
        ``dst`` like any slot afterwards: feed it the token that follows the prefix.  ``RuntimeError`` if the pool has
        no page for the copy; nothing has changed then."""
        assert self.ragged, "slots need DecodeSession(..., ragged=True)"
        if not self.cache.paged:
            raise ValueError("fork_slot needs kv_layout='paged': slabs cannot share rows")
        self.cache.fork(src, dst)

    @torch.no_grad()
    def prefill_slot(self, b: int, ids: Tensor) -> Tensor:
        """Ragged sessions: append ``ids [T]`` to sequence ``b`` alone (the single-sequence prefill on that slot's
        slabs of the cache); returns its logits ``[1, V]``.  Positions and cache rows of the other slots do not
        change, and neither do any addresses, so a captured decode graph stays valid."""
        assert self.ragged, "slots need DecodeSession(..., ragged=True)"
        ids = ids.reshape(1, -1).to(self.device)
        return self._append(ids, [ids.shape[1]], [b])

    @torch.no_grad()
    def prefill_slots(self, rows: list[int], prompts: list[Tensor]) -> Tensor:
        """Ragged sessions: append ``prompts[i]`` (``[T_i]`` ids) to sequence ``rows[i]`` for several distinct slots
        at once; returns their logits ``[len(rows), V]``.  On the fast path the prompts are *packed* -- concatenated,
        no padding -- and take one pass over the layers (``kv_append_packed`` + ``cache_attn_packed`` on the whole
        cache, every sequence at its slot's own position; ``ops/decode.py``, "Packed prefill").  A slot may already
        hold tokens (a second turn, a forked prefix): every sequence attends the cache as stored.  Pages for all the
        rows are reserved first, so a pool that runs out raises before anything is launched.  The other slots' cache
        rows and positions do not change and no address does, so a captured decode graph stays valid.

        ``prefill_chunk`` splits a call whose packed token count exceeds it at sequence boundaries into several
        passes; a single prompt longer than it goes through :meth:`prefill_slot`, which chunks it.  A row's logits
        are those of :meth:`prefill_slot` up to GEMM rounding (the GEMMs' M is the packed count).  Off the fast path
        the call is a loop over :meth:`prefill_slot`, the same function with the same bits."""
        assert self.ragged, "slots need DecodeSession(..., ragged=True)"
        rows = [int(r) for r in rows]
        assert len(rows) == len(prompts) >= 1, "prefill_slots: one prompt per row, at least one"
        assert len(set(rows)) == len(rows), "prefill_slots: rows must be distinct"
        assert all(0 <= r < self.batch for r in rows), "prefill_slots: a row outside the batch"
        prompts = [p.reshape(-1) for p in prompts]
        n = [int(p.numel()) for p in prompts]
        assert all(x >= 1 for x in n), "prefill_slots: empty prompt"
        c = self.cache
        assert all(c._len[r] + x <= self.max_len for r, x in zip(rows, n)), "KV cache full"
        c.reserve(rows, [c._len[r] + x for r, x in zip(rows, n)])
        if not self.fast:
            return torch.cat([self.prefill_slot(r, p) for r, p in zip(rows, prompts)])
        out = [None] * len(rows)
        for grp in _packed_groups(n, self.prefill_chunk):
            if len(grp) == 1 and self.prefill_chunk is not None and n[grp[0]] > self.prefill_chunk:
                out[grp[0]] = self.prefill_slot(rows[grp[0]], prompts[grp[0]])
                continue
            lg = self._forward_packed([rows[i] for i in grp], [prompts[i] for i in grp])
            for j, i in enumerate(grp):
                out[i] = lg[j : j + 1]
        return out[0] if len(out) == 1 else torch.cat(out)

    def _append(self, ids: Tensor, n: list[int], rows: list[int]) -> Tensor:
        """Every prefill: the first ``n[i]`` tokens of ``ids[i]`` (right-padded) go to sequence ``rows[i]`` -- the
        whole batch, or one slot.  Returns every sequence's logits after its last valid token."""
        c = self.cache
        cur = [c._len[r] for r in rows]
        assert all(p + x <= self.max_len for p, x in zip(cur, n)), "KV cache full"
        c.reserve(rows, [p + x for p, x in zip(cur, n)])
        ids = ids[:, : max(n)]
        B, T = ids.shape
        G = self.H // self.Hkv
        if not self.fast:  # the oracle math reads the host lengths, which therefore move chunk by chunk
            plan = [(t0, w, "reference") for t0, w in _chunks(T, self.prefill_chunk)]
        else:
            # empty cache: one causal flash prefill over the (padded) window + one kv_append; a pad token sits to the
            # right of every valid one, so no valid token sees it, and its cache rows lie at or past pos[b].
            # Filled cache (multi-turn serving, a chunk of a long prompt): kv_append + cache_attn over the whole
            # window, every token attending the cache plus its own causal prefix; a window of up to 8 / G tokens
            # (speculative verification) is one decode_attn step (_append_plan)
            plan = _append_plan(T, G, max(cur) > 0, self.prefill_chunk, not self.fp8)
            kv = None if B == self.batch else c.view(rows[0])
        out = None
        for t0, w, kind in plan:
            # sequence i advances by the part of its length that falls in the chunk, and its logits come from
            # the chunk holding its last valid token; the device step / last exist only where the parts differ
            part = [min(max(x - t0, 0), w) for x in n]
            if kind == "reference":
                lg = self._forward_reference(ids[:, t0 : t0 + w], part, rows)
                c.advance(rows, part)
            else:
                step = last = None
                if min(part) < w:
                    step = torch.tensor(part, dtype=torch.int32).to(self.device)
                    last = torch.tensor([max(p - 1, 0) for p in part]).to(self.device)
                lg = self._forward_fast(ids[:, t0 : t0 + w], kind, step=step, last=last, kv=kv)
            here = [i for i, p in enumerate(part) if p]  # sequences with a valid token in this chunk
            if len(here) == B:
                out = lg
            else:
                out[here] = lg[here]
        if self.fast:
            c.advance(rows, n)
        return out

    @torch.no_grad()
    def generate(self, prompt, max_new_tokens: int, temperature: float = 1.0, top_p: float | None = None,
                 eos_token_id: int | None = None, generator: torch.Generator | None = None,
                 top_k: int | None = None, sampler: str = "host", seed: int | None = None, sync_every: int = 16,
                 repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                 logit_bias=None, return_logprobs: bool = False):
        """``prompt [B, S]`` -> ``[B, S + n]`` (stops early once every row emitted ``eos_token_id``).

        Ragged sessions also take a list of ``B`` 1-D prompts of different lengths and return a list of 1-D tensors:
        each prompt plus its continuation, ending with the first ``eos_token_id`` if one was emitted.  A sequence
        that has emitted EOS becomes inactive; the loop ends when all are done or at ``max_new_tokens``.

        ``top_k`` keeps the ``top_k`` most likely tokens (applied before ``top_p``; ``None``: off).

        ``sampler="host"`` (default) samples in PyTorch from ``generator`` and looks at every token on the host.
        ``sampler="device"`` samples with ``ops.sample_rows`` on the session's sampling table (``ops/sampling.py``
        states the function: ``ops.sample_step``'s, row by row), on the fast path inside a second captured graph --
        decode step -> ``sample_rows`` -- that writes the next token straight into its own input and advances the
        token counters itself.  Temperature, ``top_k``, ``top_p``, EOS, the seed and the penalty values are read from
        the table, so one graph serves every call and a change of values never captures.  EOS and the ragged active
        mask are handled on the device, and the host only reads the ``done`` flags every ``sync_every`` tokens (never,
        without ``eos_token_id``).  Its random
        stream is Philox keyed by ``seed`` at counter (token index, row); ``seed=None`` draws one from ``generator``
        (else from torch's default generator), which is all ``generator`` is used for in this mode.  The results have
        the shapes of the host sampler's; ``prompt + max_new_tokens <= max_len`` is checked once, up front.

        Sampling controls (``ops/sampling.py`` states the function; all default to off, and then nothing new runs):
        ``repetition_penalty`` (> 0; over prompt and output), ``presence_penalty`` / ``frequency_penalty`` (over the
        output) and ``logit_bias`` (a ``{token: value}`` dict or a ``[V]`` tensor; ``-inf`` bans a token) change the
        logits the sampler reads -- ``ops.logit_process`` before every sample, ``ops.token_commit`` after it, with the
        per-sequence token history on the device; with ``sampler="device"`` their per-row forms run inside the
        captured step: decode -> ``logit_process_rows`` -> ``sample_rows`` -> ``token_commit_rows``.  Which of them
        run is decided per call by three switches -- a penalty is on, log-probs are wanted, there is a bias -- and a
        graph is captured once per set of switches it meets; a call with none replays the plain graph, whatever the
        calls before it used.  ``return_logprobs`` makes
        the result ``(tokens, logprobs)``: fp32 ``[B, n]`` (a list of 1-D tensors for list prompts), aligned with the
        emitted tokens and trimmed as they are, each the token's log-probability under the model's own
        distribution (unprocessed logits, T = 1, no filters), not under the warped one it was sampled from."""
        assert sampler in ("host", "device"), "sampler: 'host' or 'device'"
        ctl = _controls(self.model.lm_head.weight.shape[0], self.device, repetition_penalty, presence_penalty,
                        frequency_penalty, logit_bias, return_logprobs)
        if sampler == "device":
            return self._generate_device(prompt, max_new_tokens, temperature, top_k, top_p, eos_token_id, generator,
                                         seed, sync_every, ctl)
        if isinstance(prompt, (list, tuple)):
            return self._generate_ragged(prompt, max_new_tokens, temperature, top_p, eos_token_id, generator, top_k,
                                         ctl)
        self.reset()
        logits = self.prefill(prompt)
        outs = [prompt.to(self.device)]
        done = None
        hc = None if ctl is None else _HostControls(ctl, outs[0], None, logits.shape[-1], max_new_tokens)
        for i in range(max_new_tokens):
            nxt = _sample(logits if hc is None else hc.process(logits), temperature, top_p, generator, top_k)
            if hc is not None:
                hc.commit(i, nxt)
            outs.append(nxt[:, None])
            if eos_token_id is not None:
                hit = nxt == eos_token_id
                done = hit if done is None else (done | hit)
                if bool(done.all()):
                    break
            if i + 1 < max_new_tokens:
                logits = self.decode(nxt)
        if ctl is not None and ctl.logprobs:
            return torch.cat(outs, 1), hc.logprob[:, : len(outs) - 1]
        return torch.cat(outs, 1)

    def _pad_prompts(self, prompts):
        """A list of 1-D prompts -> (the prompts on the device, their lengths, right-padded ``ids [B, max]``)."""
        assert self.ragged, "a list of prompts needs DecodeSession(..., ragged=True)"
        B = self.batch
        assert len(prompts) == B, f"session batch is {B}, got {len(prompts)} prompts"
        prompts = [p.reshape(-1).to(self.device) for p in prompts]
        n = [int(p.numel()) for p in prompts]
        assert min(n) >= 1, "empty prompt"
        ids = torch.zeros(B, max(n), dtype=torch.long, device=self.device)  # right-padded (the pad id is never seen)
        for b, p in enumerate(prompts):
            ids[b, : n[b]] = p
        return prompts, n, ids

    def _generate_ragged(self, prompts, max_new_tokens, temperature, top_p, eos_token_id, generator,
                         top_k=None, ctl=None):
        B = self.batch
        prompts, n, ids = self._pad_prompts(prompts)
        self.reset()
        logits = self.prefill(ids, n)
        new: list[list[int]] = [[] for _ in range(B)]
        done = [False] * B
        hc = None if ctl is None else _HostControls(ctl, ids, n, logits.shape[-1], max_new_tokens)
        for i in range(max_new_tokens):
            nxt = _sample(logits if hc is None else hc.process(logits), temperature, top_p, generator, top_k)
            if hc is not None:
                hc.commit(i, nxt, torch.tensor(done))
            for b, tok in enumerate(nxt.tolist()):
                if not done[b]:
                    new[b].append(tok)
                    done[b] = eos_token_id is not None and tok == eos_token_id
            if all(done):
                break
            if i + 1 < max_new_tokens:
                logits = self.decode(nxt, active=[not d for d in done])
                if any(done):  # an inactive row's logits are unspecified: keep the sampler's input finite
                    logits[[b for b in range(B) if done[b]]] = 0.0
        out = [torch.cat([p, torch.tensor(t, dtype=p.dtype, device=self.device)]) for p, t in zip(prompts, new)]
        if ctl is not None and ctl.logprobs:
            return out, [hc.logprob[b, : len(t)].clone() for b, t in enumerate(new)]
        return out

    # ------------------------------------------------------------------ device sampler
    def _sampler_state(self, penal: bool = False, logprobs: bool = False, bias: Tensor | None = None):
        """The device sampler's static state, shared by ``generate(sampler="device")`` and ``models/serving.py``: a
        :class:`~bpe_transformer.ops.sampling.SamplingTable` (its ``step`` is a ragged fast session's own decode step,
        else the table's own), ``ids [B, 1]`` (the next token: the step's input), ``out [B, max_len]`` (token ``i`` of
        a slot in column ``i``) and, once a switch asks for them, ``hist [B, V]``, ``proc [B, V]``, ``lse [B]``,
        ``logprob [B, max_len]``, ``bias [V]``; their contents are the caller's to initialise.  Every sampling
        parameter is read from the table, so only the three structural switches select what runs: a penalty table is
        in use (``penal``), log-probs are recorded (``logprobs``), there is a shared bias.  They are this call's, not
        sticky: ``st["key"]`` holds them, :meth:`_sample_rows` passes only the buffers they name, and with all three
        off nothing but ``sample_rows`` runs.  With ``use_graph`` the step -- decode -> ``logit_process_rows`` ->
        ``sample_rows`` -> ``token_commit_rows`` -- is captured once per key (``st["graphs"]``; ``st["captures"]``
        counts them) and a change of parameter values never captures.  During a capture's warm-up run every slot is
        idle, so it writes nothing the running requests would see."""
        from ..ops.sampling import SamplingTable

        B, dev, V = self.batch, self.device, self.model.lm_head.weight.shape[0]
        st = self._samp
        if st is None:
            st = self._samp = {
                "table": SamplingTable(B, dev, self._step),
                "ids": torch.zeros(B, 1, dtype=torch.long, device=dev),
                "out": torch.full((B, self.max_len), -1, dtype=torch.long, device=dev),
                "hist": None, "proc": None, "lse": None, "logprob": None, "bias": None,
                "key": None, "graphs": {}, "captures": 0,
            }
            self._step_host = [0] * B  # (what the table's step holds: every slot idle)
        if penal and st["hist"] is None:
            st["hist"] = torch.zeros(B, V, dtype=torch.int32, device=dev)
        if logprobs and st["lse"] is None:
            st["lse"] = torch.zeros(B, dtype=torch.float32, device=dev)
            st["logprob"] = torch.full((B, self.max_len), math.nan, dtype=torch.float32, device=dev)
        if bias is not None:
            if st["bias"] is None:
                st["bias"] = torch.zeros(V, dtype=torch.float32, device=dev)
            st["bias"].copy_(bias)
        if (penal or bias is not None) and st["proc"] is None and self.fast:
            st["proc"] = torch.empty(B, V, dtype=self.model.lm_head.weight.dtype, device=dev)
        st["key"] = key = (bool(penal), bool(logprobs), bias is not None)
        if self.use_graph and key not in st["graphs"]:
            t = st["table"]
            pos0, done0, step0 = self.cache.pos.clone(), t.done.clone(), t.step.clone()
            t.done.fill_(1)
            t.step.zero_()
            st["graphs"][key], _ = _capture_graph(
                dev, lambda: self._sample_rows(st, self._forward_fast(st["ids"], "decode", step=self._step)),
                lambda: self.cache.pos.copy_(pos0))
            t.done.copy_(done0)
            t.step.copy_(step0)
            st["captures"] += 1
        return st

    def _sample_rows(self, st, logits: Tensor, rows=None) -> None:
        """One sampling step on the sampler's state, for the switches in ``st["key"]``: ``logit_process_rows`` (only
        with a penalty table, a bias or log-probs) -> ``sample_rows`` -> ``token_commit_rows`` (only with a penalty
        table or log-probs).  ``logits`` are the whole batch's, or with ``rows`` those of the named slots (an
        admission's prefill)."""
        from ..ops import sampling

        t = st["table"]
        penal, logprobs, biased = st["key"]
        hist = st["hist"] if penal else None
        bias = st["bias"] if biased else None
        lse, logprob = (st["lse"], st["logprob"]) if logprobs else (None, None)
        if logits.dtype not in (torch.bfloat16, torch.float32):  # (an fp64 model off the fast path)
            logits = logits.float()
        logits = logits.contiguous()
        src = logits
        proc = penal or biased
        if proc:
            full = st["proc"]
            if rows is not None or full is None or full.dtype != logits.dtype:
                src = torch.empty_like(logits)  # (an admission's single row; off the fast path)
            else:
                src = full
        if proc or logprobs:
            sampling.logit_process_rows(logits, t, hist, bias, src if proc else None, lse, rows)
        sampling.sample_rows(src, t, st["ids"], st["out"], rows)
        if penal or logprobs:
            sampling.token_commit_rows(st["out"], t, hist, logits, lse, logprob, rows)

    def _device_step(self, st) -> None:
        """Decode the tokens in ``st["ids"]`` and sample the next ones into it: one replay on the fast path."""
        if self.use_graph:
            st["graphs"][st["key"]].replay()
            return
        if self.fast:
            logits = self._forward_fast(st["ids"], "decode", step=self._step)
        else:  # the oracle math reads host lengths: the step comes back per token
            rows = list(range(self.batch))
            n = [int(x) for x in st["table"].step.tolist()]
            logits = self._forward_reference(st["ids"], n, rows)
            self.cache.advance(rows, n)
        self._sample_rows(st, logits)

    def _generate_device(self, prompt, max_new_tokens, temperature, top_k, top_p, eos_token_id, generator, seed,
                         sync_every, ctl=None):
        from ..ops import sampling

        B = self.batch
        as_list = isinstance(prompt, (list, tuple))
        if as_list:
            prompts, n, ids = self._pad_prompts(prompt)
        else:
            ids = prompt.to(self.device)
            n = [ids.shape[1]] * B
        assert sync_every >= 1, "sync_every: a positive number of tokens"
        assert max(n) + max_new_tokens <= self.max_len, "KV cache full: prompt + max_new_tokens exceeds max_len"
        lp = ctl is not None and ctl.logprobs
        if max_new_tokens <= 0:
            res = prompts if as_list else ids
            none = torch.empty(B, 0, dtype=torch.float32, device=self.device)
            return (res, list(none) if as_list else none) if lp else res
        if seed is None:
            gdev = generator.device if generator is not None else "cpu"
            seed = int(torch.randint(0, 2**62, (1,), generator=generator, device=gdev))
        eos = -1 if eos_token_id is None else int(eos_token_id)
        assert int(top_k or 0) >= 0, "top_k: 0 (off) or a positive count"
        penal, bias = ctl is not None and ctl.penal, None if ctl is None else ctl.bias
        self.reset()
        st = self._sampler_state(penal, lp, bias)
        # Every slot takes the call's parameters and one seed; the Philox row word is the row, so row b draws token i
        # at counter (i, b): `sample_step`'s stream.  The host loop bounds the count (no limit in the table: a row
        # that has not finished keeps step 1).  A tensor prompt's finished rows keep generating until every row has
        # finished, as with the host sampler, so their tokens are needed: no EOS for the kernel there, and `done` is
        # read off `out` at each sync instead.
        t = st["table"]
        rp, pp, fp = (ctl.rp, ctl.pp, ctl.fp) if ctl is not None else (1.0, 0.0, 0.0)
        t.set(slice(0, B), sampling.SamplingParams(
            temperature=temperature, top_k=top_k, top_p=top_p, min_p=0.0, seed=seed, max_new_tokens=2**31 - 1,
            eos_token_id=eos if as_list and eos >= 0 else None, repetition_penalty=rp, presence_penalty=pp,
            frequency_penalty=fp))
        t.philox_row.copy_(torch.arange(B, dtype=torch.int32))
        self._step_host = [1] * B
        st["out"].fill_(-1)
        if penal:
            st["hist"].copy_(sampling.prompt_hist(ids, n if as_list else None, st["hist"].shape[1]))
        if lp:
            st["logprob"].fill_(math.nan)
        self._sample_rows(st, self.prefill(ids, n if as_list else None))
        made = 1  # tokens sampled per row
        upto = 0  # a paged cache has pages for the first `upto` fed tokens of every row
        while made < max_new_tokens:
            if eos >= 0 and made % sync_every == 0:  # the only host sync of the loop
                done = t.done != 0 if as_list else (st["out"][:, :made] == eos).any(1)
                if bool(done.all()):
                    break
            if made > upto:
                # the host does not know which rows have finished: every row gets the pages of the next sync_every
                # tokens (at most one page too many each), before the replays that write them
                upto = made - 1 + sync_every
                self.cache.reserve(range(B), [x + upto for x in n])
            self._device_step(st)
            made += 1
        out = st["out"][:, :made].cpu()
        hit = out == eos if eos >= 0 else torch.zeros_like(out, dtype=torch.bool)
        first = torch.where(hit.any(1), hit.int().argmax(1), torch.full((B,), made)).tolist()  # first EOS, or `made`
        c = self.cache
        if as_list:
            # row b was fed first[b] of its tokens (its EOS is not fed; a row that never finished, all but the last);
            # pos[b] already says so on the device: rebuild the host mirrors
            for b in range(B):
                c._len[b] = n[b] + min(first[b], made - 1)
            if self._step is not None:
                self._step_host = [int(f >= made) for f in first]
            c.release(range(B), c._len)  # (pages reserved ahead for rows that finished early)
            res = [torch.cat([p, out[b, : min(first[b] + 1, made)].to(self.device, p.dtype)])
                   for b, p in enumerate(prompts)]
            return (res, [st["logprob"][b, : min(first[b] + 1, made)].clone() for b in range(B)]) if lp else res
        # tensor prompt: keep the steps up to the one at which every row had emitted EOS; the replays past it (up to
        # sync_every - 1) are dropped, from the cache too
        keep = min(max(first) + 1, made)
        c.pos.fill_(n[0] + keep - 1)
        c._len[:] = [n[0] + keep - 1] * B
        c.release(range(B), c._len)
        res = torch.cat([ids, out[:, :keep].to(self.device, ids.dtype)], 1)
        return (res, st["logprob"][:, :keep].clone()) if lp else res

    # ------------------------------------------------------------------ HIP path
    def _capture(self) -> None:
        """Capture one decode step (all layers + LM head) into a HIP graph.  The warm-up run writes the cache at
        the current position (rewritten by the first replay) and the position is restored afterwards."""
        self._static_ids = torch.zeros(self.batch, 1, dtype=torch.long, device=self.device)
        pos0 = self.cache.pos.clone()
        self._graph, self._static_logits = _capture_graph(
            self.device, lambda: self._forward_fast(self._static_ids, "decode", step=self._step),
            lambda: self.cache.pos.copy_(pos0))

    def _hip(self):
        """The HIP ops handle both fast forwards run on (the one seam: a test substitutes a spy here)."""
        from ..ops._ext import ops as hip

        return hip()

    def _forward_fast(self, ids: Tensor, kind: str, step: Tensor | None = None, last: Tensor | None = None,
                      kv: KVView | None = None, all_logits: bool = False, advance: bool = True) -> Tensor:
        """``kind`` (``_append_plan``): ``"flash"``, flash attention inside the window (empty cache); ``"cache"``,
        ``cache_attn`` over the cache (a window of more than ``8 / G`` tokens); ``"decode"``, ``decode_attn``.
        ``step``: device int32 advance per sequence instead of ``T``; ``last``: index of the token whose logits
        each sequence returns instead of ``T - 1`` (both only where the sequences differ); ``kv``: the view to run
        on -- one slot's instead of the whole cache's; ``all_logits``: the logits of every position, ``[B * T, V]``,
        instead of the last one's; ``advance=False`` leaves the position where it was (a speculative round sets it
        after the verification)."""
        kv = kv or self.cache.view()
        if kind == "decode" and ids.shape[1] == 1 and not all_logits and ids.shape[0] <= _GEMV_MAX_BATCH and self._gemv_fits(ids.shape[0]):
            return self._decode_gemv(ids, step, kv)
        assert kind != "flash" or not self.fp8, "an fp8 session attends to the cache as stored (no flash prefill)"
        h, rope = self._hip(), self._rope
        m = self.model
        B, T = ids.shape
        H, Hkv, D = self.H, self.Hkv, self.D
        xr = m.token_embeddings(ids).reshape(B * T, -1)
        xd = None
        for li, (ln1, wqkv, wo, ln2, w13, w2, eps) in enumerate(self._w):
            if xd is None:
                h1, _ = h.rmsnorm_fwd(xr, ln1, eps)
            else:
                xr, h1, _ = h.add_rmsnorm_fwd(xr, xd, ln1, eps)
            qkv = torch.matmul(h1, self._wide(h, wqkv).t())
            if kind == "flash":
                q, k, v = qkv[:, : H * D], qkv[:, H * D : (H + Hkv) * D], qkv[:, (H + Hkv) * D :]
                o, _ = h.fa_fwd(q, k, v, rope[0], rope[1], B, T, H, Hkv, D, True, rope[2], 1.0 / math.sqrt(D))
                kv.append(h, qkv, li, T, H, rope)
            else:
                o = kv.attend(h, kv.append(h, qkv, li, T, H, rope), li, T, H, kind)
            g1 = torch.matmul(o, self._wide(h, wo).t())
            xr, h2, _ = h.add_rmsnorm_fwd(xr, g1, ln2, eps)
            a = h.swiglu_fwd(torch.matmul(h2, self._wide(h, w13).t()))
            xd = torch.matmul(a, self._wide(h, w2).t())
        if all_logits:
            pass
        elif T > 1 and last is not None:  # ragged: each sequence's own last valid token
            rows = torch.arange(B, device=last.device)
            xr = xr.view(B, T, -1)[rows, last].contiguous()
            xd = xd.view(B, T, -1)[rows, last].contiguous()
        elif T > 1:  # only the last position's logits are needed
            xr = xr.view(B, T, -1)[:, -1].contiguous()
            xd = xd.view(B, T, -1)[:, -1].contiguous()
        fin = m.ln_final
        _, hf, _ = h.add_rmsnorm_fwd(xr, xd, fin.weight, fin.eps)
        logits = torch.matmul(hf, self._wide(h, self._head).t())
        if advance:
            kv.pos.add_(T if step is None else step)
        return logits

    def _forward_packed(self, rows: list[int], prompts: list[Tensor]) -> Tensor:
        """One pass over the layers on the packed tokens of ``prompts`` (``prefill_slots``): ``_forward_fast``'s
        launches on ``[N, .]`` rows, with ``kv_append_packed`` + ``cache_attn_packed`` on the whole cache; each
        sequence's last row goes through the final norm and the head; ``pos[rows]`` advances by a device index add
        and the host mirror follows.  Pages are reserved by the caller."""
        from ..ops.decode import PackedPrompts

        h, rope = self._hip(), self._rope
        m, c, H = self.model, self.cache, self.H
        n = [int(p.numel()) for p in prompts]
        pk = PackedPrompts(rows, n, self.device, pos_host=[c._len[r] for r in rows])
        kv = c.view()
        xr = m.token_embeddings(torch.cat(prompts).to(self.device)).reshape(pk.N, -1)
        xd = None
        for li, (ln1, wqkv, wo, ln2, w13, w2, eps) in enumerate(self._w):
            if xd is None:
                h1, _ = h.rmsnorm_fwd(xr, ln1, eps)
            else:
                xr, h1, _ = h.add_rmsnorm_fwd(xr, xd, ln1, eps)
            qkv = torch.matmul(h1, self._wide(h, wqkv).t())
            o = kv.attend_packed(h, kv.append_packed(h, qkv, li, H, rope, pk), li, H, pk)
            g1 = torch.matmul(o, self._wide(h, wo).t())
            xr, h2, _ = h.add_rmsnorm_fwd(xr, g1, ln2, eps)
            a = h.swiglu_fwd(torch.matmul(h2, self._wide(h, w13).t()))
            xd = torch.matmul(a, self._wide(h, w2).t())
        last = torch.tensor([off + x - 1 for off, x in zip(pk.offs, n)]).to(self.device)
        fin = m.ln_final
        _, hf, _ = h.add_rmsnorm_fwd(xr[last].contiguous(), xd[last].contiguous(), fin.weight, fin.eps)
        logits = torch.matmul(hf, self._wide(h, self._head).t())
        c.pos.index_add_(0, torch.tensor(rows).to(self.device), torch.tensor(n, dtype=torch.int32).to(self.device))
        c.advance(rows, n)
        return logits

    def _gemv_fits(self, m: int) -> bool:
        cfg = self.model.config
        return all(_gemv_ok(m, k) for k in (cfg.d_model, self.H * self.D, self._w[0][5][0].shape[1]))

    def _decode_gemv(self, ids: Tensor, step: Tensor | None, kv: KVView) -> Tensor:
        """Decode step for batch <= 16 on the fused skinny-GEMM kernels (``csrc/decode_gemv.hip``): per layer
        qkv (+RMSNorm, +RoPE, +cache write) -> split-K decode attention -> Wo (+ the split combine) -> [W1; W3]
        (+residual add, +RMSNorm, +SwiGLU) -> W2; the residual add of W2's output is folded into the next layer's
        QKV prologue: 5 launches per layer.  An fp8 cache takes 6: the QKV projection with the plain epilogue, then
        ``kv_append_fp8`` (RoPE, quantisation, cache write), and ``decode_attn_fp8``.  fp8 weights: the same launches,
        every projection called with its ``(w8, w_scale)`` pair."""
        h, rope = self._hip(), self._rope
        m = self.model
        H = self.H
        B = ids.shape[0]
        xr = m.token_embeddings(ids).reshape(B, -1)
        xd = None
        for li, (ln1, wqkv, wo, ln2, w13, w2, eps) in enumerate(self._w):
            q, s = kv.decode_qkv(h, xr, xd, ln1, eps, wqkv[0], li, H, rope, wqkv[1:])
            if xd is not None:
                xr = s
            part = kv.attend(h, q, li, 1, H, "decode", combine=False)
            g1 = h.decode_attn_proj(part, *wo)  # the flash-decoding combine runs in Wo's prologue
            a, xr = h.decode_gemv(xr, g1, ln2, eps, w13[0], 1, *w13[1:])
            xd, _ = h.decode_gemv(a, None, None, 0.0, w2[0], 0, *w2[1:])
        fin = m.ln_final
        logits, _ = h.decode_gemv(xr, xd, fin.weight, fin.eps, self._head[0], 0, *self._head[1:])
        kv.pos.add_(1 if step is None else step)
        return logits

    # ------------------------------------------------------------------ oracle path
    def _forward_reference(self, ids: Tensor, n: list[int], rows: list[int], all_logits: bool = False) -> Tensor:
        """Plain-PyTorch math over the same cache (any dtype / device / ablation): ``ids [len(rows), T]``
        (right-padded), of which the first ``n[i]`` tokens are appended to sequence ``rows[i]`` at its own position
        (RoPE positions and visibility per sequence; with one shared position they all agree).  Returns the logits
        after each sequence's last valid token (token 0 where ``n[i] == 0``: an inactive decode step, unspecified).
        Pad tokens are written at and past the new position, where nothing reads them, or dropped at the end of the
        cache."""
        m = self.model
        R, T = ids.shape
        H, Hkv, D, Lmax = self.H, self.Hkv, self.D, self.max_len
        dev = ids.device
        cur = [self.cache._len[r] for r in rows]
        p0 = torch.tensor(cur, device=dev)
        Lk = min(max(cur) + T, Lmax)
        tp = p0[:, None] + torch.arange(T, device=dev)[None, :]  # [R, T] absolute positions
        mask = (torch.arange(Lk, device=dev)[None, None, :] <= tp[:, :, None])[:, None]  # [R, 1, T, Lk]
        tpr = tp.clamp(max=Lmax - 1)[:, None, :]  # (a pad token past the cache has no table row; it is dropped)
        x = m.token_embeddings(ids)
        for li, layer in enumerate(m.layers):
            attn = layer.attn

            def attend(z: Tensor) -> Tensor:
                q = attn.q_proj(z).view(R, T, H, D).transpose(1, 2)
                k = attn.k_proj(z).view(R, T, Hkv, D).transpose(1, 2)
                v = attn.v_proj(z).view(R, T, Hkv, D).transpose(1, 2)
                if attn.rope is not None:
                    q = attn.rope(q, tpr)
                    k = attn.rope(k, tpr)
                for i, r in enumerate(rows):
                    w = max(0, min(T, Lmax - cur[i]))
                    self.cache.write(li, r, cur[i], cur[i] + w, k[i, :, :w], v[i, :, :w])
                kk, vv = self.cache.read(li, rows, Lk, q.dtype)
                if Hkv != H:
                    kk = kk.repeat_interleave(H // Hkv, dim=1)
                    vv = vv.repeat_interleave(H // Hkv, dim=1)
                o = F.scaled_dot_product_attention(q, kk, vv, mask)
                return attn.output_proj(o.transpose(1, 2).reshape(R, T, H * D))

            if layer.use_post_norm:
                x = layer.ln1(x + attend(x))
                x = layer.ln2(x + layer.ffn(x))
            else:
                x = x + attend(layer.ln1(x))
                x = x + layer.ffn(layer.ln2(x))
        if all_logits:  # every position's, [R, T, V]
            logits = m.lm_head(m.ln_final(x))
        else:
            last = torch.tensor([max(c - 1, 0) for c in n], device=dev)
            logits = m.lm_head(m.ln_final(x[torch.arange(R, device=dev), last]))
        if self.ragged:
            self.cache.pos[rows] += torch.tensor(n, dtype=torch.int32, device=dev)
        else:  # one shared position: every sequence took the whole window
            self.cache.pos.add_(T)
        return logits


class SpeculativeSession:
    """Speculative decoding with a draft model (Leviathan et al., ICML 2023; Chen et al., 2023): every round the
    draft proposes ``num_draft_tokens`` tokens one decode step at a time, the target scores the whole window in one
    pass, and ``ops.spec_verify_step`` (``ops/sampling.py`` states the function) keeps the drafts that stand and adds
    one token of the target's own.  Greedy decoding emits exactly the target's tokens; temperature sampling emits
    tokens distributed as the target's.  ``top_k`` / ``top_p`` are not supported with a draft model.

    It owns two ragged :class:`DecodeSession` s.  At the start of a round both caches hold every emitted token but
    the last, which sits in ``win[:, 0]`` (the target's window) and in the draft's ``ids``.  One round:

    1. ``base = pos``;
    2. K draft steps, each a decode step + ``sample_step(col=j)``, which writes draft ``j`` into ``win[:, j]``;
    3. one more draft step that only feeds draft ``K`` into the draft cache (its logits are unused), so the draft
       cache is whole when all K drafts stand;
    4. the target's pass over ``win [B, K + 1]``, every position's logits (``decode_attn`` up to ``8 // G`` tokens,
       ``cache_attn`` beyond), which leaves the target's position at ``base``;
    5. ``spec_verify_step``: emits into ``out``, sets both positions to ``base + emitted``, puts the last emitted
       token into ``win[:, 0]`` and ``ids``, finishes a row at EOS or at ``max_new_tokens``;
    6. ``rng[1] += K + 1``.

    On the fast path the round is captured once into one graph on one stream (no parallel branches) and replayed
    with no host sync inside; the host reads ``done`` every ``sync_every`` rounds.  Off the fast path (CPU, fp32,
    ablations) the same round runs eagerly on the oracle ops.  The random stream is Philox keyed by ``seed``: the
    first token is the target's own draw at counter ``(0, row, stream 2)``, round ``r`` starts at ``c = 1 + r (K +
    1)`` and draws draft ``j`` at ``(c + j - 1, row, stream 0)``, its accept test at ``(c + j - 1, row, stream 1)``
    and the final token at ``(c, row, stream 2)``.

    The proposer is the two hooks ``_propose`` (step 2 and 3) and ``_prefill_proposer``;
    :class:`PromptLookupSession` replaces them with the n-gram lookup and shares everything else.
    """

    def __init__(self, target, draft, batch: int, num_draft_tokens: int = 4, max_len: int | None = None,
                 use_graph: bool = True, kv_dtype: str = "bf16"):
        K = int(num_draft_tokens)
        if K < 1:
            raise ValueError("num_draft_tokens must be at least 1")
        if target.config.vocab_size != draft.config.vocab_size:
            raise ValueError(f"the draft's vocabulary ({draft.config.vocab_size}) is not the target's "
                             f"({target.config.vocab_size})")
        self.K = K
        self.batch = batch
        self.max_len = max_len or min(target.context_length, draft.context_length)
        if self.max_len > min(target.context_length, draft.context_length):
            raise ValueError("max_len exceeds the context length of the target or the draft")
        if kv_dtype != "bf16":  # (left for later: the verify step would set positions of an fp8 cache as it does here)
            raise ValueError(f"kv_dtype={kv_dtype!r} with a draft model is not supported yet: speculative decoding "
                             "runs on the bf16 cache only")
        self.target = DecodeSession(target, batch, self.max_len, use_graph, ragged=True)
        self.draft = DecodeSession(draft, batch, self.max_len, use_graph, ragged=True)
        self._setup(use_graph)

    def _setup(self, use_graph: bool) -> None:
        """The round's state, for either proposer: ``self.draft`` is the draft's session, or ``None`` when the
        drafts come from the lookup (``pos_d`` / ``step_d`` / ``ids`` are then scratch for ``spec_verify_step``)."""
        t, d, K, batch = self.target, self.draft, self.K, self.batch
        self._sessions = [(t, "step_t")] + ([(d, "step_d")] if d is not None else [])
        self.device = dev = t.device
        self.fast = all(s.fast for s, _ in self._sessions)
        self.use_graph = use_graph and self.fast
        if self.fast:  # the target's window must be one pass over the layers (no position moves inside the round)
            plan = _append_plan(K + 1, t.H // t.Hkv, True)
            assert len(plan) == 1, plan
            self._win_kind = plan[0][2]
        i32 = dict(dtype=torch.int32, device=dev)
        self._st = {
            "win": torch.zeros(batch, K + 1, dtype=torch.long, device=dev),
            "ids": torch.zeros(batch, 1, dtype=torch.long, device=dev),
            "out": torch.full((batch, self.max_len), -1, dtype=torch.long, device=dev),
            "n_out": torch.zeros(batch, **i32), "base": torch.zeros(batch, **i32), "done": torch.zeros(batch, **i32),
            # row j = (seed, c + j): the counters of draft j + 1, and row 0 the verifier's
            "rngs": torch.zeros(K + 1, 2, dtype=torch.long, device=dev),
            # a session off the fast path has no static step: the round's own
            "step_t": t._step if t._step is not None else torch.ones(batch, **i32),
            "step_d": d._step if d is not None and d._step is not None else torch.ones(batch, **i32),
            "pos_d": d.cache.pos if d is not None else torch.zeros(batch, **i32),
        }
        self._graph, self._key = None, None

    # ------------------------------------------------------------------ one round
    def _decode_draft(self) -> Tensor:
        d, st = self.draft, self._st
        if d.fast:
            return d._forward_fast(st["ids"], "decode", step=st["step_d"])
        rows = list(range(self.batch))
        n = [int(x) for x in st["step_d"].tolist()]
        logits = d._forward_reference(st["ids"], n, rows)
        d.cache.advance(rows, n)
        return logits

    def _score_window(self) -> Tensor:
        t, st = self.target, self._st
        B, K = self.batch, self.K
        if t.fast:
            return t._forward_fast(st["win"], self._win_kind, all_logits=True, advance=False).view(B, K + 1, -1)
        return t._forward_reference(st["win"], [0] * B, list(range(B)), all_logits=True)  # (0: no advance)

    def _propose(self, temperature: float, out: Tensor) -> list[Tensor]:
        """Write the K drafts into ``win[:, 1:]``; returns the draft logits of a sampling round (else nothing)."""
        from ..ops import sampling

        st, K = self._st, self.K
        kept = []
        for j in range(1, K + 1):
            logits = self._decode_draft()
            sampling.sample_step(logits, temperature, 0, 1.0, st["rngs"][j - 1], st["ids"], st["win"], st["step_d"],
                                 st["done"], -1, col=j)
            if temperature > 0:
                kept.append(logits)
        self._decode_draft()
        return kept

    def _prefill_proposer(self, ids: Tensor, n: list[int]) -> None:
        self.draft.prefill(ids, n)

    def _round(self, temperature: float, eos: int, out: Tensor) -> None:
        from ..ops import sampling

        st, K = self._st, self.K
        st["base"].copy_(self.target.cache.pos)
        kept = self._propose(temperature, out)
        tl = self._score_window()
        sl = torch.stack(kept, 1).to(tl.dtype) if kept else None  # the one gathering launch of a sampling round
        sampling.spec_verify_step(tl, sl, temperature, st["rngs"][0], st["win"], st["ids"], out, st["n_out"],
                                  st["base"], self.target.cache.pos, st["pos_d"], st["step_t"], st["step_d"],
                                  st["done"], eos, point_mass=self.draft is None)
        st["rngs"][:, 1].add_(K + 1)

    def _sync_mirrors(self) -> None:
        for s, _ in self._sessions:
            s.cache._len[:] = [int(x) for x in s.cache.pos.tolist()]

    def _capture(self, key) -> None:
        """Capture one round for ``key = (temperature, eos, max_new_tokens)`` (baked into the graph) with
        ``_capture_graph``, on benign state at position 0 (the caller initialises every buffer afterwards)."""
        temperature, eos, n = key
        out = self._st["out"][:, :n]
        self._graph, _ = _capture_graph(self.device, lambda: self._round(temperature, eos, out),
                                        lambda: self._init_state(0))
        self._key = key

    def _init_state(self, seed: int) -> None:
        st, K = self._st, self.K
        st["win"].zero_()
        st["ids"].zero_()
        st["out"].fill_(-1)
        for k in ("n_out", "base", "done"):
            st[k].zero_()
        st["step_d"].fill_(1)
        for s, k in self._sessions:
            s.reset()
            st[k].fill_(1)
            s._step_host = [1] * self.batch
        st["rngs"].copy_(torch.tensor([[seed, 1 + j] for j in range(K + 1)], dtype=torch.long))

    # ------------------------------------------------------------------ public API
    @torch.no_grad()
    def generate(self, prompt, max_new_tokens: int, temperature: float = 1.0, eos_token_id: int | None = None,
                 seed: int | None = None, generator: torch.Generator | None = None, sync_every: int = 4):
        """``prompt [B, S]`` -> ``[B, S + n]``, or a list of ``B`` 1-D prompts -> a list of 1-D tensors, with the
        shapes and EOS rules of :meth:`DecodeSession.generate`.  ``seed=None`` draws the Philox seed from
        ``generator`` (else torch's default generator).  The host reads the ``done`` flags every ``sync_every``
        rounds.  ``prompt + max_new_tokens + num_draft_tokens + 1 <= max_len`` is checked once, up front."""
        from ..ops import sampling

        t, st, K, B = self.target, self._st, self.K, self.batch
        as_list = isinstance(prompt, (list, tuple))
        if as_list:
            prompts, n, ids = t._pad_prompts(prompt)
        else:
            ids = prompt.to(self.device)
            assert ids.dim() == 2 and ids.shape[0] == B, f"session batch is {B}"
            n = [ids.shape[1]] * B
        assert sync_every >= 1, "sync_every: a positive number of rounds"
        if max(n) + max_new_tokens + K + 1 > self.max_len:
            raise ValueError(f"KV cache full: prompt ({max(n)}) + max_new_tokens ({max_new_tokens}) + "
                             f"num_draft_tokens + 1 ({K + 1}) exceeds max_len ({self.max_len})")
        if max_new_tokens <= 0:
            return prompts if as_list else ids
        if seed is None:
            gdev = generator.device if generator is not None else "cpu"
            seed = int(torch.randint(0, 2**62, (1,), generator=generator, device=gdev))
        eos = -1 if eos_token_id is None else int(eos_token_id)
        # a tensor prompt's finished rows keep generating until every row has finished (DecodeSession.generate), so
        # the kernel sees no EOS there and the host looks for it in `out` at each sync
        key = (float(temperature), eos if as_list else -1, int(max_new_tokens))
        self._init_state(seed)
        if self.use_graph and self._key != key:
            self._capture(key)
            self._init_state(seed)
        out = st["out"][:, :max_new_tokens]
        # the first token is the target's own: prefill both, draw at Philox counter (0, row, stream 2)
        logits = t.prefill(ids, n)
        self._prefill_proposer(ids, n)
        first = sampling.sample_logits(logits, temperature, 0, 1.0, sampling.philox_uniform(seed, 0, B, stream=2))
        first = first.to(self.device)
        out[:, 0] = first
        st["win"][:, 0] = first
        st["ids"][:, 0] = first
        st["n_out"].fill_(1)
        fin = torch.full_like(first, max_new_tokens <= 1, dtype=torch.bool)
        if key[1] >= 0:
            fin |= first == key[1]
        st["done"].copy_(fin)
        st["step_d"].copy_(~fin)
        for s, k in self._sessions:
            st[k].copy_(~fin)
            s._step_host = None  # the device owns the steps until the end
        rounds = 0
        while rounds < max_new_tokens - 1:
            if rounds % sync_every == 0 and self._finished(as_list, eos, out):  # the only host sync of the loop
                break
            if self.use_graph:
                self._graph.replay()
            else:
                self._round(*key[:2], out)
                self._sync_mirrors()
            rounds += 1
        made = [int(x) for x in st["n_out"].tolist()]
        res = out.cpu()
        for s, k in self._sessions:
            s._step_host = [int(x) for x in st[k].tolist()]
        if as_list:
            # both caches hold every emitted token but the last; pos[b] already says so on the device
            for s, _ in self._sessions:
                s.cache._len[:] = [n[b] + made[b] - 1 for b in range(B)]
            return [torch.cat([p, res[b, : made[b]].to(self.device, p.dtype)]) for b, p in enumerate(prompts)]
        # tensor prompt: keep the tokens up to the one at which every row had emitted EOS, as DecodeSession does
        keep = min(made)
        if eos >= 0:
            hit = res[:, :keep] == eos
            if bool(hit.any(1).all()):
                keep = min(keep, int(hit.int().argmax(1).max()) + 1)
        for s, _ in self._sessions:
            s.cache.pos.fill_(n[0] + keep - 1)
            s.cache._len[:] = [n[0] + keep - 1] * B
        return torch.cat([ids, res[:, :keep].to(self.device, ids.dtype)], 1)

    def _finished(self, as_list: bool, eos: int, out: Tensor) -> bool:
        st = self._st
        if bool((st["done"] != 0).all()):
            return True
        if as_list or eos < 0:
            return False
        made = st["n_out"].tolist()
        hit = out.cpu() == eos
        first = [int(h[:m].int().argmax()) if bool(h[:m].any()) else -1 for h, m in zip(hit, made)]
        return min(first) >= 0 and min(made) >= max(first) + 1


def _lookup_bounds(prompt_lookup) -> tuple[int, int]:
    """``prompt_lookup=n_hi`` or ``(n_hi, n_lo)`` -> the checked n-gram bounds ``(n_hi, n_lo)``; an int means
    ``n_lo = 1``."""
    n_hi, n_lo = prompt_lookup if isinstance(prompt_lookup, (tuple, list)) else (prompt_lookup, 1)
    n_hi, n_lo = int(n_hi), int(n_lo)
    if not 1 <= n_lo <= n_hi:
        raise ValueError(f"prompt_lookup: n-gram bounds need 1 <= n_lo <= n_hi, got n_hi={n_hi}, n_lo={n_lo}")
    return n_hi, n_lo


class PromptLookupSession(SpeculativeSession):
    """Speculative decoding without a draft model (prompt lookup / n-gram drafting): every round
    ``ops.lookup_draft`` finds the most recent earlier occurrence of the last ``n_lo .. n_hi`` tokens in the
    sequence's own history (prompt + emitted tokens) and proposes what followed it; the target verifies the proposal
    in one pass, with ``spec_verify_step(point_mass=True)`` (``ops/sampling.py`` states both functions).  Greedy
    decoding emits exactly the target's tokens, sampling emits tokens distributed as the target's, whatever is
    proposed.  No second model, no second KV cache, no draft decode steps.

    It is :class:`SpeculativeSession`'s round and ``generate`` with another proposer.  It owns the target's ragged
    :class:`DecodeSession` only, a static device copy of the padded prompts (``prompt [B, max_len]``, ``n_prompt
    [B]``, filled per ``generate`` call; columns at and past ``n_prompt[b]`` are never read) and int32 ``[B]``
    scratch in the place of the draft's ``pos`` / ``step``.  One round, one graph on one stream: ``base = pos``;
    ``lookup_draft`` writes ``win[:, 1:]``; the target's window pass; ``spec_verify_step``; ``rngs[:, 1] += K + 1``.
    The Philox counters are the draft-model form's, stream 0 unused.
    """

    def __init__(self, target, batch: int, num_draft_tokens: int = 4, prompt_lookup=3, max_len: int | None = None,
                 use_graph: bool = True, kv_dtype: str = "bf16", weight_dtype: str = "bf16"):
        K = int(num_draft_tokens)
        if K < 1:
            raise ValueError("num_draft_tokens must be at least 1")
        self.n_hi, self.n_lo = _lookup_bounds(prompt_lookup)
        for name, v in (("kv_dtype", kv_dtype), ("weight_dtype", weight_dtype)):
            if v != "bf16":  # (left for later, as with a draft model)
                raise ValueError(f"{name}={v!r} with prompt_lookup is not supported yet: speculative decoding runs "
                                 "on the bf16 cache and bf16 weights only")
        self.K = K
        self.batch = batch
        self.max_len = max_len or target.context_length
        if self.max_len > target.context_length:
            raise ValueError("max_len exceeds the context length of the target")
        self.target = DecodeSession(target, batch, self.max_len, use_graph, ragged=True)
        self.draft = None
        self._setup(use_graph)
        self._st["prompt"] = torch.zeros(batch, self.max_len, dtype=torch.long, device=self.device)
        self._st["n_prompt"] = torch.zeros(batch, dtype=torch.int32, device=self.device)

    def _propose(self, temperature: float, out: Tensor) -> list[Tensor]:
        from ..ops import sampling

        st = self._st
        sampling.lookup_draft(st["prompt"], st["n_prompt"], out, st["n_out"], st["win"], st["step_t"], st["done"],
                              self.n_hi, self.n_lo)
        return []

    def _prefill_proposer(self, ids: Tensor, n: list[int]) -> None:
        st = self._st
        st["prompt"][:, : ids.shape[1]] = ids
        st["n_prompt"].copy_(torch.tensor(n, dtype=torch.int32))
