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

**Speculative verification** (``csrc/spec_verify.hip``; the rejection scheme of Leviathan et al., "Fast Inference
from Transformers via Speculative Decoding", ICML 2023, and Chen et al., "Accelerating Large Language Model Decoding
with Speculative Sampling", 2023).  Per sequence, with target logits ``t[0..K]`` (each ``[V]``; ``t[i-1]`` is the
target's row for the position of draft ``i``), draft tokens ``d[1..K]`` and, for sampling, draft logits ``s[1..K]``,
a temperature ``T`` and uniforms ``ua[1..K]`` and ``us``:

Greedy (``T <= 0``):

1. ``n`` is the number of leading ``i`` with ``d[i] == argmax t[i-1]``, lowest index on ties.
2. ``y = argmax t[n]``.

Sampling (``T > 0``):

1. ``p_i = softmax(t[i-1] / T)`` and ``q_i = softmax(s[i] / T)``; a ``-inf`` logit has mass 0.
2. Draft ``i`` is accepted iff ``ua[i] * q_i(d[i]) < p_i(d[i])``.
3. ``n`` is the number accepted before the first rejection.
4. If ``n < K``, ``y`` is drawn from ``r = max(p_{n+1} - q_{n+1}, 0)``: the lowest index whose inclusive cumulative
   ``r``, in index order, exceeds ``us * R`` with ``R = sum r``; if rounding finds none, the last index with
   ``r > 0``; if ``R == 0``, from ``p_{n+1}`` in the same way.
5. If ``n == K``, ``y`` is drawn the same way from ``p_{K+1}``.

The result is ``(n, y)``; the emitted tokens are ``d[1..n], y``.  For greedy decoding they are exactly the target's
own; for sampling ``d[i] ~ q_i`` makes them distributed as the target's.  ``top_k`` / ``top_p`` are not part of
this function: the warped ``p`` and ``q`` would both need the radix-select cut, so a draft model cannot be combined
with either.

:func:`spec_verify` is that function for given uniforms.  :func:`spec_verify_step` is the form inside the captured
graph of a speculative round.  With ``rng = (seed, c)`` it draws ``ua[i]`` with Philox at counter
``(c + i - 1, row, 1)`` and ``us`` at ``(c, row, 2)`` -- the fourth counter word is the *stream*; stream 0 stays
``sample_step``'s -- and per active row writes the emitted tokens into ``out[b, n_out[b] ..]``, advances
``n_out[b]`` by their number ``m``, puts the last of them into ``win[b, 0]`` (the next round's first target token)
and the draft's ``ids[b, 0]``, and sets ``pos_target[b] = pos_draft[b] = base[b] + m``: both caches then hold every
emitted token but the last.  Emission stops, inclusive, at the first ``eos`` or at the last column of ``out``;
either sets ``done[b]`` and clears the row's ``step`` in both sessions (without them ``m = n + 1``).  A row with
``done`` set or ``step == 0`` writes nothing.  ``rng`` is read only.

**Point-mass drafts** (``point_mass=True``): the proposer is deterministic, so ``q_i`` is the point mass at ``d[i]``
and there are no draft logits (``draft_logits`` is ``None``).  Sampling then reads:

2. draft ``i`` is accepted iff ``ua[i] < p_i(d[i])``;
4. if ``n < K``, ``y`` is drawn from ``p_{n+1}`` with ``d[n+1]`` zeroed -- the index-order inverse CDF at ``us`` as
   above -- and from ``p_{n+1}`` itself if that leaves no mass or if ``d[n+1]`` lies outside ``[0, V)`` (such a
   ``d`` never stands and is never read).

Greedy is unchanged.  It is the function above for one-hot draft logits (``0`` at ``d[i]``, ``-inf`` elsewhere), and
the kernel computes it in the same fixed-point arithmetic, so the two agree exactly; what is saved is the ``[B, K, V]``
draft-logits tensor and its row passes.

**Prompt-lookup drafts** (``csrc/lookup_draft.hip``; n-gram drafting from the sequence's own history, as in Saxena,
"Prompt Lookup Decoding", 2023).  Per sequence ``b`` the history is ``h = prompt[b, :n_prompt[b]] ++ out[b,
:n_out[b]]`` of length ``L`` (never materialised); its last token ``h[L-1]`` is the last emitted one, ``win[b, 0]``.
With ``K`` drafts and n-gram bounds ``1 <= n_lo <= n_hi``:

1. A candidate is an end position ``e``, ``0 <= e <= L-2``; its match length ``m(e)`` is the largest ``t <=
   min(n_hi, e+1)`` with ``h[e-t+1+u] == h[L-t+u]`` for all ``0 <= u < t``.
2. The chosen ``e`` has the largest ``m(e)`` and, among equal lengths, is the largest (the most recent); it is a
   match iff that ``m >= n_lo``.  (The same as trying ``n = n_hi`` down to ``n_lo`` and taking the latest earlier
   occurrence of the last ``n`` tokens that has at least one token after it.)
3. With a match and ``p = L-1-e >= 1``: ``d[j] = h[e + 1 + (j mod p)]`` for ``j = 0..K-1`` -- the continuation is
   extended periodically past the end of the history, so a period-``p`` loop yields ``K`` drafts, not ``p``.
4. With no match, or ``L == 1``: ``d[j] = h[L-1]`` for all ``j``.

Any drafts are valid for the verifier: the proposal is deterministic, so with ``point_mass=True`` the emitted tokens
remain the target's (greedy) or distributed as the target's (sampling) whatever is proposed.  :func:`lookup_draft`
writes ``d`` into ``win[b, 1..K]`` inside the captured round; token ids must fit int32.

**Sampling controls** (``csrc/logit_process.hip``: logit bias, the repetition penalty of Keskar et al., "CTRL", 2019,
as HF / vLLM apply it over prompt and output, and the OpenAI / vLLM presence and frequency penalties over the output
only).  The state of sequence ``b`` is one row of an int32 table ``hist [B, V]``: ``hist[b, v] = 2 * (times v was
emitted so far) + (1 if v occurs in the prompt)``, so ``seen = hist != 0`` and ``c = hist >> 1``.

:func:`logit_process` takes a row ``x [V]`` (fp32 or bf16), an optional ``bias [V]`` (fp32, shared by all rows) and
``rp > 0``, ``pp``, ``fp``; all arithmetic is fp32, in this order:

1. ``y = x + bias[v]``.  A ``-inf`` bias is allowed and stays ``-inf`` through every later step; NaN is not supported.
2. Where ``seen``: ``y = y * (1 / rp)`` if ``y > 0`` else ``y * rp``; ``1 / rp`` is computed once on the host in fp32
   and passed in, so nothing divides on the device.
3. ``y = y - fp * c - pp * (c > 0)``.
4. ``y`` is rounded once to the row's dtype and written to ``out [B, V]``, which may be the input itself.

An element with ``hist == 0`` and ``bias == 0`` (or without either) comes out bit-identical to its input -- its
arithmetic is skipped, so ``-0.0`` stays ``-0.0``.  The same pass computes ``lse[b] = logsumexp(x[b, :])`` over the
**unprocessed** row: an fp32 max and an fp32 sum of ``exp(x - max)``, a ``-inf`` logit contributing 0 (a row of
``-inf`` has ``lse = -inf``).  Any of ``hist``, ``bias``, ``out``, ``lse`` may be absent: with only ``lse`` this is a
log-sum-exp, with only the penalties no ``lse`` is written.

:func:`token_commit` runs after :func:`sample_step` and before the caller advances ``rng[1]``.  For row ``b``, ``tok =
tokens[b, count]`` with ``count = rng[1]``; if ``tok >= 0`` (the sampler wrote a token: an idle row holds the ``-1``
``sample_step`` leaves in that column and writes nothing) then ``hist[b, tok] += 2`` and ``logprob[b, count] =
float(raw_logits[b, tok]) - lse[b]``.  Either half (``hist``; ``raw_logits`` / ``lse`` / ``logprob``) may be absent, and
a ``count`` outside ``logprob``'s columns writes nothing.  The log-prob is the token's log-probability under the
model's own distribution -- unprocessed logits, T = 1, no filters -- and **not** under the warped distribution the
token was sampled from (bias, penalties, temperature, top-k / top-p).

:func:`prompt_hist` builds the table of a fresh batch: bit 0 for every prompt token, right-padding untouched.

**Per-row forms** (``csrc/sample_rows.hip``, ``csrc/logit_process.hip``; continuous batching).  :func:`sample_rows`,
:func:`logit_process_rows` and :func:`token_commit_rows` are the three in-graph functions above with every parameter
read per *slot* from a :class:`SamplingTable` of ``B`` slots, so that requests with different parameters, seeds and
lengths share one captured graph and a change of values never captures again.  ``R`` rows are launched; an optional
int32 ``rows [R]`` maps launched row ``r`` to slot ``b = rows[r]`` (``None``: ``b = r``, ``R = B``).  What is shaped
like the logits (``logits``, ``out`` of ``logit_process_rows``, ``raw_logits``: ``[R, V]``) is indexed by ``r``;
every table and ``ids [B, 1]``, ``out [B, N]``, ``hist [B, V]``, ``lse [B]``, ``logprob [B, N]`` by ``b``.

A slot is *idle* iff ``done[b] != 0`` or ``step[b] == 0``.  An idle slot does nothing at all in any of the three: it
writes nothing and its counter stands (``spec_verify_step``'s rule, not ``sample_step``'s ``-1``).

:func:`sample_rows`, for an active slot, with ``c = count[b]``:

1. ``u = u[r]`` if uniforms are given, else Philox4x32-10 keyed by ``seed[b]`` at counter ``(c, philox_row[b], 0)``.
   The row word is a column of the table, not the slot.  Its default 0 is a served request's: the random stream
   depends on neither the slot nor its neighbours, and equals a one-row ``sample_step`` at ``rng = (seed[b], c)``.
   ``philox_row[b] = b`` with one seed in every slot is ``sample_step``'s stream at ``rng = (seed, c)``, which is
   how ``generate(sampler="device")`` runs on this function.
2. The token is the sampling function at the top of this docstring with ``temperature[b]`` (fp32), ``top_k[b]``
   (int32), ``top_p[b]`` (fp64: the kernel computes ``ceil(top_p * Z)`` in double, as the scalar one does on its
   double argument) and one more filter between steps 5 and 6: ``min_p[b] > 0`` (fp32; the min-p sampling of Nguyen
   et al., "Turning Up the Heat: Min-p Sampling for Creative and Coherent LLM Outputs", 2024) keeps, of what top-k
   and top-p kept, a token iff its mass is at least ``min_p`` times the largest mass.  In the kernel's fixed-point
   masses ``zq_i = floor(z_i * 2^40)``: a token stays iff ``zq_i >= ceil(min_p * zq_max)`` (the product in fp64),
   where ``zq_max = 2^40`` is the argmax's; the threshold is capped at ``zq_max``, so the argmax token always stays.
   The reference applies the same integers to its fp64 ``z``.
3. ``ids[b, 0] = out[b, c] = token`` (``out`` only where ``c`` is one of its columns) and ``count[b] = c + 1``.
4. If ``token == eos[b]`` (``eos[b] < 0``: none) or ``count[b] >= limit[b]``: ``done[b] = 1`` and ``step[b] = 0``.

The kernel advances the counter itself, so no ``rng[1] += 1`` launch follows it.

:func:`logit_process_rows` is :func:`logit_process` with ``rp[b]``, ``1 / rp[b]``, ``pp[b]``, ``fp[b]`` (fp32
``[B]``, the reciprocal made on the host when the slot is set).  A slot whose three penalties are neutral (``rp ==
1``, ``pp == fp == 0``) is processed without its history: every element the shared ``bias [V]`` does not touch keeps
its bits.  The bias is one ``[V]`` tensor for all slots; a per-request bias is not supported.

:func:`token_commit_rows` is :func:`token_commit` at column ``count[b] - 1``, for every slot whose counter has moved
since its last commit: the table keeps ``committed[b]``, a slot commits iff ``count[b] > committed[b]`` and then
``committed[b] = count[b]``.  So the slot that has just drawn its last token (and is ``done`` now) still commits
it, and a slot that drew nothing commits nothing.
"""

from __future__ import annotations

import dataclasses
import math

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


def philox_uniform(seed: int, count: int, B: int, device=None, stream: int = 0, row0: int = 0) -> Tensor:
    """The uniforms :func:`sample_step` draws for rows ``row0 .. row0 + B - 1`` at ``rng = (seed, count)``: fp32
    ``[B]``.  ``stream`` is the fourth counter word (1, 2: the accept tests and the final draw of
    :func:`spec_verify_step`)."""
    seed, count = int(seed) & (2**64 - 1), int(count) & (2**64 - 1)
    key = (seed & _M32, seed >> 32)
    x0 = [philox4x32(key, (count & _M32, count >> 32, (row0 + b) & _M32, int(stream)))[0] for b in range(B)]
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


def sample_logits_reference(logits: Tensor, temperature: float, top_k: int, top_p: float, u: Tensor,
                            min_p: float = 0.0) -> Tensor:
    """The function of the module docstring in torch: fp64 masses, a stable sort for the rank order.  ``temperature``
    counts as the kernels receive it, rounded to fp32.  ``min_p > 0`` adds the min-p filter of "Per-row forms"."""
    x = logits.double()
    B, V = x.shape
    temperature = _f32(temperature)
    if temperature <= 0:
        return (x == x.amax(-1, keepdim=True)).int().argmax(-1)  # (argmax of a 0/1 row: its first 1)
    z = torch.exp((x - x.amax(-1, keepdim=True)) / temperature)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices  # equal x stay in index order
    zs = z.gather(-1, order)
    keep = torch.ones_like(zs, dtype=torch.bool)
    if top_k > 0:
        keep &= torch.arange(V, device=x.device)[None, :] < min(int(top_k), V)
    if top_p < 1.0:
        zk = zs * keep
        keep &= zk.cumsum(-1) - zk < float(top_p) * zk.sum(-1, keepdim=True)
        keep[:, 0] = True
    if min_p > 0:
        thr = min(math.ceil(_f32(min_p) * 2.0**40), 2**40)  # ceil(min_p * zq_max), zq_max = 2^40
        keep &= torch.floor(zs * 2.0**40) >= thr
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
                step: Tensor | None, done: Tensor, eos: int, col: int = -1) -> None:
    """Sample one token per row in place, for a decode loop that never leaves the device.

    ``rng`` int64 ``[2]`` = (seed, count), read only; ``ids`` int64 ``[B, 1]`` takes the token; ``out`` int64
    ``[B, N]`` takes it in column ``count``, or ``-1`` if the row is already done (``done[b] != 0``) or inactive
    (``step[b] == 0``); ``done`` int32 ``[B]`` is set where an active row draws ``eos`` (``eos < 0``: none), and a
    ragged session's ``step`` int32 ``[B]`` is cleared there, so that sequence stops advancing.

    ``col >= 0`` names the column of ``out`` that takes the token instead of ``count`` (a draft model writes draft
    ``j`` straight into the target's window, ``win[:, j]``); a done or inactive row then leaves that column as it is,
    so a window only ever holds tokens."""
    _check(logits, temperature, top_k, top_p)
    if logits.is_cuda:
        ops().sample_step(logits.contiguous(), float(temperature), int(top_k), float(top_p), rng, ids, out, step, done,
                          int(eos), int(col))
        return
    sample_step_reference(logits, temperature, top_k, top_p, rng, ids, out, step, done, eos, col)


def sample_step_reference(logits, temperature, top_k, top_p, rng, ids, out, step, done, eos, col: int = -1) -> None:
    B = logits.shape[0]
    seed, count = (int(v) for v in rng.tolist())
    tok = sample_logits_reference(logits, temperature, top_k, top_p, philox_uniform(seed, count, B, logits.device))
    idle = done != 0
    if step is not None:
        idle = idle | (step == 0)
    ids.view(-1).copy_(tok)
    if col >= 0:
        if col < out.shape[1]:
            out[:, col] = torch.where(idle, out[:, col], tok)
    elif 0 <= count < out.shape[1]:
        out[:, count] = torch.where(idle, torch.full_like(tok, -1), tok)
    if eos >= 0:
        hit = ~idle & (tok == eos)
        done[hit] = 1
        if step is not None:
            step[hit] = 0


# ---------------------------------------------------------------- speculative verification
def _check_spec(target_logits: Tensor, draft_tokens: Tensor, draft_logits: Tensor | None, temperature: float,
                point_mass: bool = False) -> None:
    assert target_logits.dim() == 3 and draft_tokens.dim() == 2, "target_logits [B, K + 1, V], draft_tokens [B, K]"
    B, K1, V = target_logits.shape
    assert K1 >= 2 and V >= 1 and tuple(draft_tokens.shape) == (B, K1 - 1), "target_logits [B, K + 1, V], K >= 1"
    assert target_logits.dtype in (torch.bfloat16, torch.float32), "logits: bf16 or fp32"
    if point_mass:
        assert draft_logits is None, "point-mass drafts have no draft logits"
    elif temperature > 0:
        assert draft_logits is not None and tuple(draft_logits.shape) == (B, K1 - 1, V) \
            and draft_logits.dtype == target_logits.dtype, "sampling needs draft_logits [B, K, V] of the target's dtype"


def spec_verify(target_logits: Tensor, draft_tokens: Tensor, draft_logits: Tensor | None, temperature: float,
                ua: Tensor | None = None, us: Tensor | None = None, point_mass: bool = False) -> tuple[Tensor, Tensor]:
    """``(n [B] int32, y [B] int64)`` of the module docstring for ``target_logits [B, K + 1, V]``, ``draft_tokens
    [B, K]``, ``draft_logits [B, K, V]`` (``None`` for greedy and for ``point_mass``) and the uniforms ``ua [B, K]``,
    ``us [B]`` (unused for greedy)."""
    _check_spec(target_logits, draft_tokens, draft_logits, temperature, point_mass)
    if not target_logits.is_cuda:
        return spec_verify_reference(target_logits, draft_tokens, draft_logits, temperature, ua, us, point_mass)
    dev = target_logits.device
    if temperature > 0:
        ua, us = ua.to(dev, torch.float32).contiguous(), us.to(dev, torch.float32).contiguous()
        draft_logits = None if point_mass else draft_logits.contiguous()
    else:
        ua = us = draft_logits = None
    return ops().spec_verify(target_logits.contiguous(), draft_tokens.to(dev, torch.long).contiguous(), draft_logits,
                             float(temperature), ua, us, bool(point_mass))


def _inv_cdf(w: Tensor, u: float) -> int:
    """Lowest index whose inclusive cumulative ``w`` (fp64, index order) exceeds ``u * sum w``; if rounding finds
    none, the last index with ``w > 0``; ``-1`` when there is no mass."""
    cum = w.cumsum(0)
    if not float(cum[-1]) > 0:
        return -1
    hit = ((cum > u * cum[-1]) & (w > 0)).nonzero()
    return int(hit[0]) if hit.numel() else int((w > 0).nonzero()[-1])


def _argmax_low(x: Tensor) -> int:
    return int((x == x.max()).nonzero()[0])


def spec_verify_reference(target_logits, draft_tokens, draft_logits, temperature, ua=None, us=None,
                          point_mass: bool = False):
    """The verification function in torch, fp64 masses, one sequence at a time."""
    t = target_logits.double()
    B, K1, V = t.shape
    K = K1 - 1
    ns, ys = [], []
    for b in range(B):
        d = [int(v) for v in draft_tokens[b].tolist()]
        if temperature <= 0:
            n = 0
            while n < K and d[n] == _argmax_low(t[b, n]):
                n += 1
            ns.append(n)
            ys.append(_argmax_low(t[b, n]))
            continue
        soft = lambda x: torch.softmax(x / float(temperature), -1)  # noqa: E731  (exp(-inf) = 0)
        s = None if point_mass else draft_logits[b].double()
        n, r = 0, None
        while n < K:
            p = soft(t[b, n])
            if point_mass:  # q: the point mass at d[n]
                ok = 0 <= d[n] < V and float(ua[b, n]) < float(p[d[n]])
                if not ok:
                    r = p.clone()
                    if 0 <= d[n] < V:
                        r[d[n]] = 0
                    break
                n += 1
                continue
            q = soft(s[n])
            ok = 0 <= d[n] < V and float(ua[b, n]) * float(q[d[n]]) < float(p[d[n]])
            if not ok:
                r = (p - q).clamp_(min=0)
                break
            n += 1
        u = float(us[b])
        y = _inv_cdf(r, u) if r is not None else -1
        if y < 0:
            y = _inv_cdf(soft(t[b, n]), u)
        ns.append(n)
        ys.append(y if y >= 0 else _argmax_low(t[b, n]))
    dev = target_logits.device
    return torch.tensor(ns, dtype=torch.int32, device=dev), torch.tensor(ys, dtype=torch.long, device=dev)


def spec_verify_step(target_logits: Tensor, draft_logits: Tensor | None, temperature: float, rng: Tensor, win: Tensor,
                     ids: Tensor, out: Tensor, n_out: Tensor, base: Tensor, pos_target: Tensor, pos_draft: Tensor,
                     step_target: Tensor, step_draft: Tensor, done: Tensor, eos: int, point_mass: bool = False) -> None:
    """Verify one speculative round in place (module docstring): ``win`` int64 ``[B, K + 1]`` holds the last
    emitted token and the K drafts, ``rng`` int64 ``[2]`` = (seed, c) is read only; ``ids`` int64 ``[B, 1]``, ``out``
    int64 ``[B, N]``, ``n_out`` / ``base`` / ``pos_*`` / ``step_*`` / ``done`` int32 ``[B]``; ``eos < 0``: none.
    With ``point_mass`` (no draft model) ``ids``, ``pos_draft`` and ``step_draft`` are scratch of those shapes."""
    _check_spec(target_logits, win[:, 1:], draft_logits, temperature, point_mass)
    if target_logits.is_cuda:
        ops().spec_verify_step(target_logits.contiguous(),
                               draft_logits.contiguous() if temperature > 0 and not point_mass else None,
                               float(temperature), rng, win, ids, out, n_out, base, pos_target, pos_draft, step_target,
                               step_draft, done, int(eos), bool(point_mass))
        return
    spec_verify_step_reference(target_logits, draft_logits, temperature, rng, win, ids, out, n_out, base, pos_target,
                               pos_draft, step_target, step_draft, done, eos, point_mass)


def spec_verify_step_reference(target_logits, draft_logits, temperature, rng, win, ids, out, n_out, base, pos_target,
                               pos_draft, step_target, step_draft, done, eos, point_mass: bool = False) -> None:
    B, K = win.shape[0], win.shape[1] - 1
    seed, c = (int(v) for v in rng.tolist())
    dev = target_logits.device
    ua = us = None
    if temperature > 0:
        ua = torch.stack([philox_uniform(seed, c + i, B, dev, stream=1) for i in range(K)], 1)
        us = philox_uniform(seed, c, B, dev, stream=2)
    ns, ys = spec_verify_reference(target_logits, win[:, 1:], draft_logits, temperature, ua, us, point_mass)
    N = out.shape[1]
    for b in range(B):
        if int(done[b]) != 0 or int(step_target[b]) == 0:
            continue
        n, o = int(ns[b]), int(n_out[b])
        toks = [int(v) for v in win[b, 1 : 1 + n].tolist()] + [int(ys[b])]
        m, fin = 0, False
        for tok in toks:
            if o + m >= N or fin:
                break
            out[b, o + m] = tok
            m += 1
            fin = eos >= 0 and tok == eos
        fin = fin or o + m >= N
        n_out[b] = o + m
        if m:
            win[b, 0] = ids[b, 0] = toks[m - 1]
            pos_target[b] = pos_draft[b] = int(base[b]) + m
        if fin:
            done[b] = 1
            step_target[b] = 0
            step_draft[b] = 0


# ---------------------------------------------------------------- prompt-lookup drafts
def lookup_draft(prompt: Tensor, n_prompt: Tensor, out: Tensor, n_out: Tensor, win: Tensor, step: Tensor, done: Tensor,
                 n_hi: int, n_lo: int = 1) -> None:
    """Write the ``K = win.shape[1] - 1`` prompt-lookup drafts of the module docstring into ``win[b, 1..K]``, in
    place.  ``prompt`` int64 ``[B, P]`` and ``out`` int64 ``[B, N]`` hold the history, of which only ``prompt[b,
    :n_prompt[b]]`` and ``out[b, :n_out[b]]`` are read; ``n_prompt`` / ``n_out`` / ``step`` / ``done`` int32 ``[B]``.
    A row with ``done[b] != 0`` or ``step[b] == 0`` keeps its ``win`` row; nothing else is written."""
    assert win.dim() == 2 and win.shape[1] >= 2, "win: [B, K + 1], K >= 1"
    assert prompt.dim() == 2 and out.dim() == 2 and prompt.shape[0] == out.shape[0] == win.shape[0], "[B, *] rows"
    if not 1 <= int(n_lo) <= int(n_hi):
        raise ValueError(f"lookup_draft: 1 <= n_lo <= n_hi, got n_lo={n_lo}, n_hi={n_hi}")
    if win.is_cuda:
        ops().lookup_draft(prompt, n_prompt, out, n_out, win, step, done, int(n_hi), int(n_lo))
        return
    lookup_draft_reference(prompt, n_prompt, out, n_out, win, step, done, n_hi, n_lo)


def lookup_draft_reference(prompt, n_prompt, out, n_out, win, step, done, n_hi: int, n_lo: int = 1) -> None:
    """The lookup function in torch, one sequence at a time: every candidate's match length at once."""
    B, K = win.shape[0], win.shape[1] - 1
    for b in range(B):
        if int(done[b]) != 0 or int(step[b]) == 0:
            continue
        h = torch.cat([prompt[b, : int(n_prompt[b])], out[b, : int(n_out[b])]])
        L = h.numel()
        if L < 1:
            continue
        start, p = L - 1, 1  # no match: the last token, K times
        if L >= 2:
            e = torch.arange(L - 1, device=h.device)
            m = torch.zeros_like(e)
            alive = torch.ones_like(e, dtype=torch.bool)
            for t in range(min(int(n_hi), L - 1)):  # token t from the end of the suffix against h[e - t]
                alive = alive & (e >= t) & (h[(e - t).clamp(min=0)] == h[L - 1 - t])
                m = m + alive
            best = int(m.max())
            if best >= int(n_lo):
                end = int((m == best).nonzero()[-1])  # the most recent of the longest
                start, p = end + 1, L - 1 - end
        win[b, 1:] = h[start + torch.arange(K, device=h.device) % p]


# ---------------------------------------------------------------- sampling controls
def _f32(v: float) -> float:
    """``v`` rounded to fp32 (as a Python float)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _inv_f32(rp: float) -> float:
    """``1 / rp`` as the kernel receives it: one fp32 division of the fp32-rounded ``rp``, on the host."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(rp), dtype=torch.float32))


def _check_process(logits: Tensor, hist, bias, rp: float, out, lse) -> None:
    assert logits.dim() == 2 and logits.shape[1] >= 1 and logits.is_contiguous(), "logits: contiguous [B, V]"
    assert logits.dtype in (torch.bfloat16, torch.float32), "logits: bf16 or fp32"
    if not float(rp) > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {rp}")
    B, V = logits.shape
    assert hist is None or (hist.dtype == torch.int32 and tuple(hist.shape) == (B, V)), "hist: int32 [B, V]"
    assert bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (V,)), "bias: fp32 [V]"
    assert out is None or (out.dtype == logits.dtype and tuple(out.shape) == (B, V)), "out: [B, V] of the logits' dtype"
    assert lse is None or (lse.dtype == torch.float32 and lse.numel() == B), "lse: fp32 [B]"


def logit_process(logits: Tensor, hist: Tensor | None = None, bias: Tensor | None = None,
                  repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                  out: Tensor | None = None, lse: Tensor | None = None) -> None:
    """Bias and penalties (module docstring, "Sampling controls") of ``logits [B, V]`` into ``out [B, V]`` (may be
    ``logits``), and the log-sum-exp of the unprocessed rows into ``lse [B]``; ``hist`` int32 ``[B, V]``, ``bias``
    fp32 ``[V]``.  Whatever is ``None`` is left out."""
    _check_process(logits, hist, bias, repetition_penalty, out, lse)
    if logits.is_cuda:
        ops().logit_process(logits, hist, bias, _f32(repetition_penalty), _inv_f32(repetition_penalty),
                            float(presence_penalty), float(frequency_penalty), out, lse)
        return
    logit_process_reference(logits, hist, bias, repetition_penalty, presence_penalty, frequency_penalty, out, lse)


def logit_process_reference(logits, hist=None, bias=None, repetition_penalty=1.0, presence_penalty=0.0,
                            frequency_penalty=0.0, out=None, lse=None) -> None:
    """The same function in torch: fp32 arithmetic in the kernel's order (without relying on FMA), one rounding to
    the row's dtype, untouched elements copied."""
    x = logits.float()
    if lse is not None:
        m = x.amax(-1)
        s = torch.exp(x - m[:, None]).sum(-1, dtype=torch.float32)  # exp(-inf) = 0
        lse.view(-1).copy_(torch.where(m == -torch.inf, m, m + torch.log(s)))
    if out is None:
        return
    y = x
    touched = torch.zeros_like(x, dtype=torch.bool)
    if bias is not None:
        y = y + bias[None, :]
        touched = touched | (bias != 0)[None, :]
    if hist is not None:
        one = torch.ones((), dtype=torch.float32, device=x.device)
        rp, inv = one * _f32(repetition_penalty), one * _inv_f32(repetition_penalty)
        pp, fp = one * _f32(presence_penalty), one * _f32(frequency_penalty)
        seen = hist != 0
        c = (hist >> 1).float()
        y = torch.where(seen, torch.where(y > 0, y * inv, y * rp), y)
        y = torch.where(c > 0, (y - fp * c) - pp, y)
        touched = touched | seen
    out.copy_(torch.where(touched, y.to(logits.dtype), logits))


def token_commit(tokens: Tensor, rng: Tensor, hist: Tensor | None = None, raw_logits: Tensor | None = None,
                 lse: Tensor | None = None, logprob: Tensor | None = None) -> None:
    """After :func:`sample_step` (module docstring, "Sampling controls"): ``tokens`` int64 ``[B, N]`` is its ``out``
    and ``rng`` its ``(seed, count)``.  Adds the token of column ``count`` to ``hist`` int32 ``[B, V]`` and writes
    its log-probability ``float(raw_logits[b, tok]) - lse[b]`` into ``logprob`` fp32 ``[B, M]``, column ``count``; a
    row that holds ``-1`` there writes nothing.  ``hist``, or ``raw_logits`` / ``lse`` / ``logprob``, may be ``None``."""
    assert tokens.dim() == 2 and tokens.dtype == torch.long, "tokens: int64 [B, N]"
    assert hist is not None or logprob is not None, "token_commit: hist, logprob or both"
    assert logprob is None or (raw_logits is not None and lse is not None), "logprob needs raw_logits and lse"
    if tokens.is_cuda:
        if logprob is None:
            raw_logits = lse = None
        ops().token_commit(tokens, rng, hist, raw_logits, lse, logprob)
        return
    token_commit_reference(tokens, rng, hist, raw_logits, lse, logprob)


def token_commit_reference(tokens, rng, hist=None, raw_logits=None, lse=None, logprob=None) -> None:
    count = int(rng[1])
    if not 0 <= count < tokens.shape[1]:
        return
    tok = tokens[:, count]
    rows = (tok >= 0).nonzero().flatten()
    tok = tok[rows]
    if hist is not None:
        hist[rows, tok] += 2
    if logprob is not None and count < logprob.shape[1]:
        logprob[rows, count] = raw_logits[rows, tok].float() - lse.view(-1)[rows]


def prompt_hist(ids: Tensor, lengths, V: int) -> Tensor:
    """The history table of a fresh batch: int32 ``[B, V]`` with bit 0 set for every token of ``ids[b, :lengths[b]]``
    (``ids`` int64 ``[B, T]``, right-padded; ``lengths`` ``None``: the whole row).  The padding is not read."""
    B, T = ids.shape
    hist = torch.zeros(B, int(V), dtype=torch.int32, device=ids.device)
    valid = torch.ones(B, T, dtype=torch.bool, device=ids.device)
    if lengths is not None:
        n = torch.as_tensor(lengths, device=ids.device).reshape(B, 1)
        valid = torch.arange(T, device=ids.device)[None, :] < n
    rows = torch.arange(B, device=ids.device)[:, None].expand(B, T)
    hist[rows[valid], ids[valid]] = 1
    return hist


# ---------------------------------------------------------------- per-row forms (continuous batching)
@dataclasses.dataclass
class SamplingParams:
    """One request's sampling parameters: what :meth:`SamplingTable.set` writes into a slot."""

    temperature: float = 1.0
    top_k: int | None = None
    top_p: float | None = None
    min_p: float = 0.0
    seed: int = 0
    max_new_tokens: int = 16
    eos_token_id: int | None = None
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logprobs: bool = False
    logit_bias: object = None  # not supported per request (the bias is one [V] tensor for all slots): ValueError
    philox_row: int = 0  # the Philox row word: the request's stream is (seed, its own token index, philox_row)

    @property
    def penal(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0


class SamplingTable:
    """The per-slot device tables of the ``*_rows`` functions (module docstring, "Per-row forms"), ``B`` slots:
    ``temperature``, ``min_p``, ``rp``, ``inv_rp``, ``pp``, ``fp`` fp32; ``top_p`` fp64; ``top_k``, ``limit``, ``eos``,
    ``done``, ``philox_row``, ``step`` int32; ``seed``, ``count``, ``committed`` int64 -- all ``[B]``, contiguous and
    static, so a captured graph reads them.  Tables of one type are the rows of one tensor: :meth:`set` is one small copy per
    type, in stream order.  ``step`` may be a tensor the caller already owns (a ragged session's decode step).
    Every slot starts idle (``done = 1``, ``step = 0``)."""

    def __init__(self, B: int, device=None, step: Tensor | None = None):
        self.B, self.device = int(B), device
        self._f32 = torch.zeros(6, B, dtype=torch.float32, device=device)
        self._f64 = torch.ones(1, B, dtype=torch.float64, device=device)
        self._i32 = torch.zeros(5, B, dtype=torch.int32, device=device)
        self._i64 = torch.zeros(3, B, dtype=torch.long, device=device)
        self.temperature, self.min_p, self.rp, self.inv_rp, self.pp, self.fp = self._f32.unbind(0)
        self.top_p = self._f64[0]
        self.top_k, self.limit, self.eos, self.done, self.philox_row = self._i32.unbind(0)
        self.seed, self.count, self.committed = self._i64.unbind(0)
        self.step = torch.zeros(B, dtype=torch.int32, device=device) if step is None else step
        assert self.step.dtype == torch.int32 and self.step.numel() == B and self.step.is_contiguous()
        self.rp.fill_(1.0)
        self.inv_rp.fill_(1.0)
        self.eos.fill_(-1)
        self.done.fill_(1)
        self.step.zero_()

    def set(self, b: int | slice, p: SamplingParams) -> None:
        """Slot ``b`` (a slice: every slot of it) takes the request ``p`` and becomes active at token 0."""
        if not float(p.repetition_penalty) > 0:
            raise ValueError(f"repetition_penalty must be > 0, got {p.repetition_penalty}")
        if getattr(p, "logit_bias", None) is not None:
            raise ValueError("a per-request logit_bias is not supported: the bias is shared by all slots")
        top_k = int(p.top_k or 0)
        if top_k < 0:
            raise ValueError(f"top_k: 0 / None (off) or a positive count, got {p.top_k}")
        s = b if isinstance(b, slice) else slice(b, b + 1)
        self._f32[:, s].copy_(torch.tensor(
            [[float(p.temperature)], [float(p.min_p or 0.0)], [_f32(p.repetition_penalty)],
             [_inv_f32(p.repetition_penalty)], [float(p.presence_penalty)], [float(p.frequency_penalty)]],
            dtype=torch.float32))
        self._f64[:, s].copy_(torch.tensor([[1.0 if p.top_p is None else float(p.top_p)]], dtype=torch.float64))
        eos = -1 if p.eos_token_id is None else int(p.eos_token_id)
        row = int(p.philox_row) & _M32
        self._i32[:, s].copy_(torch.tensor([[min(top_k, 2**31 - 1)], [int(p.max_new_tokens)], [eos], [0],
                                            [row - 2**32 if row >= 2**31 else row]], dtype=torch.int32))
        seed = int(p.seed) & (2**64 - 1)
        self._i64[:, s].copy_(torch.tensor([[seed - 2**64 if seed >= 2**63 else seed], [0], [0]], dtype=torch.long))
        self.step[s].fill_(1)

    def clear(self, b: int) -> None:
        """Slot ``b`` becomes idle."""
        self.done[b : b + 1].fill_(1)
        self.step[b : b + 1].zero_()


def _rows_arg(rows, R: int, B: int, device) -> Tensor | None:
    if rows is None:
        assert R == B, "without a rows map the logits have one row per slot"
        return None
    rows = torch.as_tensor(rows, dtype=torch.int32).reshape(-1).to(device)
    assert rows.numel() == R, "rows: one slot per launched row"
    return rows.contiguous()


def sample_rows(logits: Tensor, table: SamplingTable, ids: Tensor, out: Tensor, rows=None,
                u: Tensor | None = None) -> None:
    """Sample one token per launched row of ``logits [R, V]`` in place, every parameter from ``table`` (module
    docstring, "Per-row forms"): ``ids`` int64 ``[B, 1]`` and ``out`` int64 ``[B, N]`` take the token of slot ``b``,
    ``table.count`` advances, ``table.done`` / ``table.step`` mark the end (EOS, or ``limit`` tokens).  ``rows``:
    int32 ``[R]`` slots of the launched rows (``None``: all ``B``, in order); ``u``: fp32 ``[R]`` uniforms in place
    of Philox."""
    assert logits.dim() == 2 and logits.shape[1] >= 1, "logits: [R, V]"
    assert logits.dtype in (torch.bfloat16, torch.float32), "logits: bf16 or fp32"
    t = table
    rows = _rows_arg(rows, logits.shape[0], t.B, logits.device)
    if logits.is_cuda:
        ops().sample_rows(logits.contiguous(), rows, None if u is None else u.to(logits.device, torch.float32).contiguous(),
                          t.temperature, t.top_k, t.top_p, t.min_p, t.seed, t.philox_row, t.count, t.limit, t.eos,
                          t.step, t.done, ids, out)
        return
    sample_rows_reference(logits, table, ids, out, rows, u)


def sample_rows_reference(logits, table, ids, out, rows=None, u=None) -> None:
    t = table
    R = logits.shape[0]
    for r in range(R):
        b = r if rows is None else int(rows[r])
        if not 0 <= b < t.B or int(t.done[b]) != 0 or int(t.step[b]) == 0:
            continue
        c = int(t.count[b])
        ur = u[r : r + 1].float() if u is not None else philox_uniform(int(t.seed[b]), c, 1, logits.device,
                                                                       row0=int(t.philox_row[b]))
        tok = int(sample_logits_reference(logits[r : r + 1], float(t.temperature[b]), int(t.top_k[b]),
                                          float(t.top_p[b]), ur, float(t.min_p[b])))
        ids.view(-1)[b] = tok
        if 0 <= c < out.shape[1]:
            out[b, c] = tok
        t.count[b] = c + 1
        eos = int(t.eos[b])
        if (eos >= 0 and tok == eos) or c + 1 >= int(t.limit[b]):
            t.done[b] = 1
            t.step[b] = 0


def logit_process_rows(logits: Tensor, table: SamplingTable, hist: Tensor | None = None, bias: Tensor | None = None,
                       out: Tensor | None = None, lse: Tensor | None = None, rows=None) -> None:
    """:func:`logit_process` with the penalties of ``table`` per slot (module docstring, "Per-row forms"): ``logits``
    and ``out`` are ``[R, V]``, ``hist`` int32 ``[B, V]``, ``lse`` fp32 ``[B]``, ``bias`` fp32 ``[V]`` shared.  An idle
    slot writes nothing; a slot with neutral penalties keeps every bit the bias does not touch."""
    t = table
    R, V = logits.shape
    assert logits.is_contiguous() and logits.dtype in (torch.bfloat16, torch.float32), "logits: contiguous bf16 / fp32"
    assert hist is None or (hist.dtype == torch.int32 and tuple(hist.shape) == (t.B, V)), "hist: int32 [B, V]"
    assert bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (V,)), "bias: fp32 [V]"
    assert out is None or (out.dtype == logits.dtype and tuple(out.shape) == (R, V)), "out: [R, V] of the logits' dtype"
    assert lse is None or (lse.dtype == torch.float32 and lse.numel() == t.B), "lse: fp32 [B]"
    rows = _rows_arg(rows, R, t.B, logits.device)
    if logits.is_cuda:
        ops().logit_process_rows(logits, rows, hist, bias, t.rp, t.inv_rp, t.pp, t.fp, t.step, t.done, out, lse)
        return
    logit_process_rows_reference(logits, table, hist, bias, out, lse, rows)


def logit_process_rows_reference(logits, table, hist=None, bias=None, out=None, lse=None, rows=None) -> None:
    """One :func:`logit_process_reference` call per active slot, with that slot's values."""
    t = table
    for r in range(logits.shape[0]):
        b = r if rows is None else int(rows[r])
        if not 0 <= b < t.B or int(t.done[b]) != 0 or int(t.step[b]) == 0:
            continue
        rp, pp, fp = float(t.rp[b]), float(t.pp[b]), float(t.fp[b])
        h = hist[b : b + 1] if hist is not None and not (rp == 1.0 and pp == 0.0 and fp == 0.0) else None
        logit_process_reference(logits[r : r + 1], h, bias, rp, pp, fp, None if out is None else out[r : r + 1],
                                None if lse is None else lse.view(-1)[b : b + 1])


def token_commit_rows(tokens: Tensor, table: SamplingTable, hist: Tensor | None = None,
                      raw_logits: Tensor | None = None, lse: Tensor | None = None, logprob: Tensor | None = None,
                      rows=None) -> None:
    """:func:`token_commit` on the per-slot counter (module docstring, "Per-row forms"): every launched slot with
    ``count[b] > committed[b]`` adds ``tokens[b, count[b] - 1]`` to ``hist [B, V]``, writes its log-probability
    ``float(raw_logits[r, tok]) - lse[b]`` into ``logprob [B, M]`` at that column, and sets ``committed[b] =
    count[b]``.  ``raw_logits`` is ``[R, V]``; ``rows`` as in :func:`sample_rows`."""
    assert tokens.dim() == 2 and tokens.dtype == torch.long and tokens.shape[0] == table.B, "tokens: int64 [B, N]"
    assert hist is not None or logprob is not None, "token_commit_rows: hist, logprob or both"
    assert logprob is None or (raw_logits is not None and lse is not None), "logprob needs raw_logits and lse"
    t = table
    R = t.B if rows is None else len(rows)
    if raw_logits is not None:
        R = raw_logits.shape[0]
    rows = _rows_arg(rows, R, t.B, tokens.device)
    if tokens.is_cuda:
        if logprob is None:
            raw_logits = lse = None
        ops().token_commit_rows(tokens, rows, t.count, t.committed, hist, raw_logits, lse, logprob)
        return
    token_commit_rows_reference(tokens, table, hist, raw_logits, lse, logprob, rows)


def token_commit_rows_reference(tokens, table, hist=None, raw_logits=None, lse=None, logprob=None, rows=None) -> None:
    t = table
    R = t.B if rows is None else len(rows)
    for r in range(R):
        b = r if rows is None else int(rows[r])
        if not 0 <= b < t.B:
            continue
        n = int(t.count[b])
        if n <= int(t.committed[b]):
            continue
        t.committed[b] = n
        col = n - 1
        if not 0 <= col < tokens.shape[1]:
            continue
        tok = int(tokens[b, col])
        if tok < 0 or (hist is not None and tok >= hist.shape[1]):
            continue
        if hist is not None:
            hist[b, tok] += 2
        if logprob is not None and col < logprob.shape[1]:
            logprob[b, col] = raw_logits[r, tok].float() - lse.view(-1)[b]
