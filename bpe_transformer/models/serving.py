"""Continuous batching: a request engine over one ragged :class:`~bpe_transformer.models.generation.DecodeSession`.

``generate`` is static batching: every row starts together and the batch runs until its slowest row ends.
:class:`ServingEngine` serves requests that arrive at different times with different sampling parameters:

    eng = ServingEngine(model, batch=8, max_len=2048, kv_layout="paged", num_pages=64)
    rid = eng.submit(prompt_ids, SamplingParams(temperature=0.8, top_k=50, top_p=0.95, min_p=0.05, seed=7,
                                                max_new_tokens=64, eos_token_id=eos))
    finished = eng.step()   # one window; the RequestOutputs that finished in it
    outs = eng.run()        # step() until nothing is waiting or running: {rid: RequestOutput}

A request lives in one of ``batch`` *slots* of the session.  Its sampling parameters, seed, token counter and length
limit are one column of the session's :class:`~bpe_transformer.ops.sampling.SamplingTable`, read on the device by
``sample_rows`` / ``logit_process_rows`` / ``token_commit_rows`` (``ops/sampling.py``, "Per-row forms"), so one
captured graph -- decode step, then those three -- serves every mix of requests: ``eng.captures`` stays 1 whatever
the parameters are (a request that is the first to use a penalty, or the first to ask for log-probs, switches the
corresponding table on and captures once more; the session's switches are per call, so the engine asks with what
it has used so far and a switch stays on once it is on).  A request's random stream is Philox keyed by its own seed
at its own token index, so its tokens do not depend on its slot, its neighbours or its arrival time.
``DecodeSession.generate(sampler="device")`` runs on the same table and the same captured step.

One :meth:`ServingEngine.step` is one *window*:

1. **admit** waiting requests, first come first served, each into the lowest free slot: the slot's table column is
   set, its history row filled from the prompt, the prompt prefilled into the slot (``prefill_slot``: the others'
   cache rows and positions do not change), and one ``sample_rows`` launch on that slot's logits draws its first
   token;
2. **reserve** each running slot's cache pages for the next ``sync_every`` tokens, capped at its own limit;
3. **replay** the one graph up to ``sync_every`` times (fewer when every running request ends sooner).  A slot whose
   request ends inside the window -- its EOS, or its ``max_new_tokens`` -- marks itself ``done`` on the device and
   idles until the window ends: that is what ``sync_every`` trades against host syncs;
4. **sync once**: read ``done``, ``count`` and the new columns of ``out`` / ``logprob``, rebuild the host length
   mirrors, and **retire** the finished slots (``reset_slot``: their pages return to the pool), so they are free
   for the next step's admissions.

**Admission is by page budget** (``kv_layout="paged"``): a request is admitted only if ``ceil((prompt +
max_new_tokens) / 256)``, summed over the running requests and itself, fits ``num_pages``.  Pages are still allocated
lazily, window by window, and the whole budget of a request that ends early returns when it retires -- so the pool
cannot run out mid-flight, and no request is ever preempted (preemption with recompute is the follow-up).  A request
whose budget does not fit waits, and those behind it wait with it (first come first served).  With
``kv_layout="slab"`` the rule is simply a free slot.

**Packed admission** (``prefill_tokens=N``, off by default).  A window's admissions are selected first, by the same
rules -- first come first served, lowest free slot, page budget, nobody overtakes a request that does not fit -- and
then prefilled together: in arrival order they are cut into groups of at most ``N`` prompt tokens (a longer prompt is
a group of its own), and a group costs one ``prefill_slots`` call -- one pass over the layers on the packed prompts,
no padding -- and one ``sample_rows`` launch for all its first tokens, where the default pays one pass and one launch
per request.  A structural switch that a request of the group needs is made before the group is prefilled.  What the
option changes about the invariance claim above: a request's prompt now goes through GEMMs whose M depends on the
requests admitted with it, so its first logits are equal up to GEMM rounding, not bit for bit, to those it would get
alone, and a sampled or greedy near-tie may resolve differently.  The decode steps, the random stream (keyed by the
request's seed and token index) and everything under ``prefill_tokens=None`` are unchanged; off the fast path
``prefill_slots`` is a loop over ``prefill_slot`` and the two settings give the same tokens.

Works with the fp8 cache, fp8 weights, chunked prefill, ``use_graph=False``, and off the fast path (CPU, fp32) on
the reference ops, where it computes the same function.
"""

from __future__ import annotations

import collections
import dataclasses
import math

import torch
from torch import Tensor

from ..ops.decode import KV_PAGE
from ..ops.sampling import SamplingParams, prompt_hist
from .generation import DecodeSession, _controls, _packed_groups

__all__ = ["RequestOutput", "SamplingParams", "ServingEngine"]


@dataclasses.dataclass
class RequestOutput:
    """``tokens``: the generated tokens (int64, on the CPU; the EOS included if one ended the request);
    ``logprobs``: their log-probabilities under the model's own distribution (fp32, aligned with ``tokens``) if the
    request asked for them, else ``None``; ``finish_reason``: ``"eos"`` or ``"length"``."""

    rid: int
    tokens: Tensor
    logprobs: Tensor | None
    finish_reason: str


@dataclasses.dataclass
class _Request:
    rid: int
    prompt: Tensor
    params: SamplingParams
    pages: int  # its page budget
    got: int = 0  # tokens read back so far


class ServingEngine:
    """The request engine of the module docstring.  ``batch`` slots over one ragged session with ``max_len``,
    ``kv_layout`` / ``num_pages``, ``kv_dtype``, ``weight_dtype``, ``prefill_chunk`` and ``use_graph`` as
    :class:`DecodeSession` takes them; ``sync_every`` is the window.  ``logit_bias`` (a ``{token: value}`` dict or a
    ``[V]`` tensor) is one bias for every request of the engine.  ``penalties`` / ``logprobs`` switch the penalty
    table / the log-prob record on from the start, so that the first request to use one does not capture again.
    ``prefill_tokens``: ``None``, one prefill pass and one sampling launch per admitted request; a positive token
    budget, packed admission (module docstring)."""

    def __init__(self, model, batch: int, max_len: int | None = None, kv_layout: str = "slab",
                 num_pages: int | None = None, kv_dtype: str = "bf16", weight_dtype: str = "bf16",
                 sync_every: int = 8, prefill_chunk: int | None = None, use_graph: bool = True, logit_bias=None,
                 penalties: bool = False, logprobs: bool = False, prefill_tokens: int | None = None):
        if int(sync_every) < 1:
            raise ValueError(f"sync_every: a positive number of tokens, got {sync_every}")
        if prefill_tokens is not None and int(prefill_tokens) < 1:
            raise ValueError(f"prefill_tokens: None or a positive number of tokens, got {prefill_tokens}")
        self.prefill_tokens = None if prefill_tokens is None else int(prefill_tokens)
        self.session = DecodeSession(model, batch, max_len=max_len, use_graph=use_graph, ragged=True,
                                     prefill_chunk=prefill_chunk, kv_dtype=kv_dtype, weight_dtype=weight_dtype,
                                     kv_layout=kv_layout, num_pages=num_pages)
        s = self.session
        self.batch, self.max_len, self.sync_every = int(batch), s.max_len, int(sync_every)
        self.vocab = model.lm_head.weight.shape[0]
        ctl = _controls(self.vocab, s.device, 1.0, 0.0, 0.0, logit_bias, False)
        self._st = s._sampler_state(penal=penalties, logprobs=logprobs, bias=None if ctl is None else ctl.bias)
        self._slots: list[_Request | None] = [None] * self.batch
        self._waiting: collections.deque[_Request] = collections.deque()
        self._next_rid = 0

    # ------------------------------------------------------------------ state
    @property
    def captures(self) -> int:
        """Graphs captured so far (0 without ``use_graph`` or off the fast path)."""
        return self._st["captures"]

    @property
    def pages_in_use(self) -> int:
        return self.session.cache.pages_in_use

    @property
    def num_waiting(self) -> int:
        return len(self._waiting)

    @property
    def num_running(self) -> int:
        return sum(r is not None for r in self._slots)

    def slot_of(self, rid: int) -> int | None:
        """The slot a running request occupies (``None``: waiting, finished or unknown)."""
        for b, r in enumerate(self._slots):
            if r is not None and r.rid == rid:
                return b
        return None

    def _pages(self, n_prompt: int, p: SamplingParams) -> int:
        return (n_prompt + int(p.max_new_tokens) + KV_PAGE - 1) // KV_PAGE if self.session.cache.paged else 0

    # ------------------------------------------------------------------ requests
    def submit(self, prompt_ids, params: SamplingParams | None = None, draft_model=None, prompt_lookup=None) -> int:
        """Queue a request; returns its id.  ``ValueError`` for a request that can never run: one that does not fit
        ``max_len`` or the page pool, speculative decoding (``draft_model`` / ``prompt_lookup``), a per-request
        ``logit_bias``."""
        p = params if params is not None else SamplingParams()
        if draft_model is not None or prompt_lookup is not None:
            raise ValueError("the serving engine does not run speculative decoding (draft_model / prompt_lookup)")
        if p.logit_bias is not None:
            raise ValueError("a per-request logit_bias is not supported: pass logit_bias to the engine (one bias for "
                             "all requests)")
        prompt = torch.as_tensor(prompt_ids, dtype=torch.long).reshape(-1)
        n = int(prompt.numel())
        if n < 1:
            raise ValueError("empty prompt")
        if int(p.max_new_tokens) < 1:
            raise ValueError(f"max_new_tokens: at least 1, got {p.max_new_tokens}")
        if not float(p.repetition_penalty) > 0:
            raise ValueError(f"repetition_penalty must be > 0, got {p.repetition_penalty}")
        if int(p.top_k or 0) < 0:
            raise ValueError(f"top_k: None / 0 (off) or a positive count, got {p.top_k}")
        if bool((prompt < 0).any()) or bool((prompt >= self.vocab).any()):
            raise ValueError(f"prompt token outside the vocabulary of {self.vocab}")
        if p.eos_token_id is not None and not 0 <= int(p.eos_token_id) < self.vocab:
            raise ValueError(f"eos_token_id outside the vocabulary of {self.vocab}")
        if n + int(p.max_new_tokens) > self.max_len:
            raise ValueError(f"prompt ({n}) + max_new_tokens ({p.max_new_tokens}) exceeds max_len ({self.max_len})")
        pages = self._pages(n, p)
        if self.session.cache.paged and pages > self.session.cache.num_pages:
            raise ValueError(f"the request needs {pages} pages, the pool has {self.session.cache.num_pages}")
        req = _Request(self._next_rid, prompt, p, pages)
        self._next_rid += 1
        self._waiting.append(req)
        return req.rid

    def _switch(self, reqs) -> tuple[bool, bool]:
        """Make the structural switches the requests ``reqs`` need (on once they are on: the session's are per call,
        so ask with what was used so far; captures once more) -> the ``(penal, logprobs)`` in force."""
        s, st = self.session, self._st
        penal, logprobs, biased = st["key"]
        want = (penal or any(r.params.penal for r in reqs), logprobs or any(r.params.logprobs for r in reqs))
        if want != (penal, logprobs):
            s._sampler_state(want[0], want[1], st["bias"] if biased else None)
        return want

    def _admit_packed(self) -> None:
        """Packed admission (module docstring): select by :meth:`_admit`'s rules, then one ``prefill_slots`` and one
        ``sample_rows`` per group of at most ``prefill_tokens`` prompt tokens."""
        s, st = self.session, self._st
        c = s.cache
        free = [b for b, r in enumerate(self._slots) if r is None]
        used = sum(r.pages for r in self._slots if r is not None)
        picked: list[tuple[int, _Request]] = []
        while self._waiting and free:
            req = self._waiting[0]
            if c.paged and used + req.pages > c.num_pages:
                break  # first come first served: nobody overtakes it
            self._waiting.popleft()
            b = free.pop(0)
            used += req.pages
            self._slots[b] = req
            picked.append((b, req))
        for grp in _packed_groups([int(r.prompt.numel()) for _, r in picked], self.prefill_tokens):
            members = [picked[i] for i in grp]
            penal, logprobs = self._switch([r for _, r in members])
            for b, req in members:
                st["table"].set(b, req.params)
                if penal:
                    st["hist"][b].copy_(prompt_hist(req.prompt[None].to(s.device), None, self.vocab)[0])
                if logprobs:
                    st["logprob"][b].fill_(math.nan)
                st["out"][b].fill_(-1)
            rows = [b for b, _ in members]
            logits = s.prefill_slots(rows, [r.prompt for _, r in members])
            s._sample_rows(st, logits, rows=rows)

    def _admit(self) -> None:
        if self.prefill_tokens is not None:
            return self._admit_packed()
        s, st = self.session, self._st
        c = s.cache
        while self._waiting:
            free = [b for b, r in enumerate(self._slots) if r is None]
            if not free:
                return
            req = self._waiting[0]
            if c.paged and sum(r.pages for r in self._slots if r is not None) + req.pages > c.num_pages:
                return  # first come first served: nobody overtakes it
            self._waiting.popleft()
            b, p = free[0], req.params
            penal, logprobs, biased = st["key"]
            if (p.penal and not penal) or (p.logprobs and not logprobs):
                # a structural switch, on once it is on (the session's are per call: ask with what was used so far);
                # captures once more
                penal, logprobs = penal or p.penal, logprobs or p.logprobs
                s._sampler_state(penal, logprobs, st["bias"] if biased else None)
            st["table"].set(b, p)
            if penal:
                st["hist"][b].copy_(prompt_hist(req.prompt[None].to(s.device), None, self.vocab)[0])
            if logprobs:
                st["logprob"][b].fill_(math.nan)
            st["out"][b].fill_(-1)
            self._slots[b] = req
            logits = s.prefill_slot(b, req.prompt)
            s._sample_rows(st, logits, rows=[b])

    @torch.no_grad()
    def step(self) -> list[RequestOutput]:
        """One window (module docstring); returns the outputs of the requests that finished in it."""
        s, st = self.session, self._st
        c, t = s.cache, st["table"]
        self._admit()
        live = [b for b, r in enumerate(self._slots) if r is not None]
        if not live:
            return []
        total = [int(self._slots[b].prompt.numel()) + int(self._slots[b].params.max_new_tokens) for b in live]
        # a running slot holds len tokens and has count = len - prompt + 1 (its last token is not fed yet)
        left = [tot - 1 - c._len[b] for b, tot in zip(live, total)]  # tokens it can still draw
        n = min(self.sync_every, max(left))
        if n > 0:
            c.reserve(live, [min(c._len[b] + n, tot) for b, tot in zip(live, total)])
            for _ in range(n):
                s._device_step(st)
        done, count = t.done.tolist(), t.count.tolist()  # the window's one sync
        finished = []
        for b in live:
            req = self._slots[b]
            n_prompt = int(req.prompt.numel())
            c._len[b] = n_prompt + count[b] - 1
            req.got = count[b]
            if not done[b]:
                continue
            toks = st["out"][b, : count[b]].to("cpu", copy=True)  # (a copy on the CPU too: the slot is reused)
            eos = req.params.eos_token_id
            reason = "eos" if eos is not None and int(toks[-1]) == int(eos) else "length"
            lp = st["logprob"][b, : count[b]].to("cpu", copy=True) if req.params.logprobs else None
            finished.append(RequestOutput(req.rid, toks, lp, reason))
            self._slots[b] = None
            s.reset_slot(b)
        s._step_host = [int(r is not None) for r in self._slots]
        return finished

    def run(self) -> dict[int, RequestOutput]:
        """:meth:`step` until nothing is waiting or running; every finished request's output by id."""
        outs: dict[int, RequestOutput] = {}
        while self._waiting or self.num_running:
            for o in self.step():
                outs[o.rid] = o
        return outs
