"""Decoder-only Transformer language model (reference contract K12,
``tests/adapters.py:282-361``).

``TransformerLM.forward(ids)`` returns logits ``[B, S, V]`` (the contract).
``TransformerLM.loss(ids, targets)`` is the training entry point: on the GPU
it fuses the LM head with softmax-cross-entropy (``ops.lm_head_cross_entropy``)
so the ``[tokens, vocab]`` logits are written once and overwritten in place by
their gradient.
"""

from __future__ import annotations

import dataclasses

import torch
from torch import Tensor, nn

from .. import ops
from .config import ModelConfig
from .layers import Embedding, Linear, RMSNorm, TransformerBlock

# LM-head rows padded (with zero rows, inside the flat parameter buffer) to a multiple of this, so the vocab
# dimension of the head GEMMs and the logits row stride are aligned (profiles/bench/lm_head_vocab_pad.log)
_VOCAB_PAD = 256

FP8_WGRAD = True  # enable_fp8's default for fp8 weight gradients (module flag: A/B runs set it)


class TransformerLM(nn.Module):
    # sharded data parallelism (parallel/zero.py) sets this to a callable(module) that waits for the in-flight
    # all-gather of that module's weights; the forward calls it right before each module's weights are read
    _bpe_param_fence = None

    def _fence(self, module: nn.Module) -> None:
        f = self._bpe_param_fence
        if f is not None:
            f(module)

    def __init__(
        self,
        vocab_size: int,
        context_length: int,
        d_model: int,
        num_layers: int,
        num_heads: int,
        d_ff: int,
        rope_theta: float = 10000.0,
        num_kv_heads: int | None = None,
        remove_rmsnorm: bool = False,
        use_post_norm: bool = False,
        remove_rope: bool = False,
        ffn_type: str | None = None,
        eps: float = 1e-5,
        device=None,
        dtype=None,
    ):
        super().__init__()
        self.config = ModelConfig(
            vocab_size=vocab_size, context_length=context_length, d_model=d_model, num_layers=num_layers,
            num_heads=num_heads, d_ff=d_ff, rope_theta=rope_theta, num_kv_heads=num_kv_heads,
            remove_rmsnorm=remove_rmsnorm, use_post_norm=use_post_norm, remove_rope=remove_rope, ffn_type=ffn_type,
            eps=eps,
        )
        self.context_length = context_length
        self.token_embeddings = Embedding(vocab_size, d_model, device=device, dtype=dtype)
        self.layers = nn.ModuleList(
            TransformerBlock(
                d_model, num_heads, d_ff, context_length, rope_theta, num_kv_heads=num_kv_heads,
                remove_rmsnorm=remove_rmsnorm, use_post_norm=use_post_norm, remove_rope=remove_rope,
                ffn_type=ffn_type, eps=eps, device=device, dtype=dtype,
            )
            for _ in range(num_layers)
        )
        self.ln_final = RMSNorm(d_model, eps, device=device, dtype=dtype) if not remove_rmsnorm else nn.Identity()
        self.lm_head = Linear(d_model, vocab_size, device=device, dtype=dtype)
        if _VOCAB_PAD > 0 and vocab_size % _VOCAB_PAD:
            self.lm_head.pad_rows = -(-vocab_size // _VOCAB_PAD) * _VOCAB_PAD

    @classmethod
    def from_config(cls, cfg: ModelConfig, device=None, dtype=None) -> "TransformerLM":
        return cls(
            cfg.vocab_size, cfg.context_length, cfg.d_model, cfg.num_layers, cfg.num_heads, cfg.d_ff, cfg.rope_theta,
            num_kv_heads=cfg.num_kv_heads, remove_rmsnorm=cfg.remove_rmsnorm, use_post_norm=cfg.use_post_norm,
            remove_rope=cfg.remove_rope, ffn_type=cfg.ffn_type, eps=cfg.eps, device=device, dtype=dtype,
        )

    fp8_state = None
    fp8_grad_state = None
    # document masking (off by default): the separator token id (``<|endoftext|>``).  When set, ``forward`` and
    # ``loss`` compute ``ops.doc_bounds(in_indices, doc_mask_token)`` unless bounds are passed, and every block's
    # attention is restricted to the query's own document.  ``generate`` and the KV-cache decode path ignore it.
    doc_mask_token: int | None = None

    def _doc_bounds(self, in_indices: Tensor, doc_bounds):
        if doc_bounds is None and self.doc_mask_token is not None:
            shape = in_indices.shape  # [..., S]: every row of the leading dims is one window
            start, end = ops.doc_bounds(in_indices.reshape(-1, shape[-1]), int(self.doc_mask_token))
            doc_bounds = (start.view(shape), end.view(shape))
        return doc_bounds

    def enable_fp8(self, history: int = 16, margin: float = 1.0, dgrad: bool = True, wgrad: bool | None = None,
                   grad_margin: float = 2.0):
        """Run the block projections in fp8 with delayed scaling: forward GEMMs e4m3 x e4m3; with ``dgrad`` the
        input-gradient GEMMs e5m2 (gradient) x e4m3 (weight) as well, and with ``wgrad`` (needs ``dgrad``) the
        weight-gradient GEMMs e5m2 (gradient^T) x e4m3 (activation^T) from the same gradient cast (None: the
        module default ``FP8_WGRAD``).

        Only the fused GPU block path quantises (``models/fused_block.py``); every block owns 8 e4m3 scale
        slots (4 activations + 4 weights) and 4 e5m2 slots (output gradients).  The training engine calls
        ``update()`` on both states once per optimizer step.  ``margin`` / ``grad_margin``: headroom factors of
        the e4m3 and e5m2 scales over their amax history (the gradient state uses the larger of the two).
        """
        from ..ops.fp8 import Fp8State

        dev = self.lm_head.weight.device
        L = len(self.layers)
        self.fp8_state = Fp8State(8 * L, dev, history=history, margin=margin)
        # gradients: a 2x margin by default (changed in round 5 from the e4m3 margin: a caller that wants a gradient
        # margin below 2 now has to pass grad_margin).  e5m2 spans ~2^32, so the headroom costs nothing measurable;
        # with margin 1 the Llama-shape parity run saturated its gradient casts by up to 2.9x at a loss-spike step,
        # with 2 once by 1.5x (benchmarks/fp8_spike_probe.py, profiles/bench/fp8_spike_probe_margins_r5.log).  The
        # margin bounds that saturation; it is not shown to remove the spike (step 18 of the parity run: loss
        # 5.7844 -> 5.7836), whose cause stays unpinned.
        self.fp8_grad_state = (Fp8State(4 * L, dev, history=history, margin=max(margin, grad_margin), fmt="e5m2")
                               if dgrad else None)
        for i, layer in enumerate(self.layers):
            layer.fp8 = (self.fp8_state, 8 * i, self.fp8_grad_state, 4 * i,
                         bool(dgrad and (FP8_WGRAD if wgrad is None else wgrad)))
        return self.fp8_state

    def fp8_states(self) -> list:
        return [s for s in (self.fp8_state, self.fp8_grad_state) if s is not None]

    def hidden_states(self, in_indices: Tensor, doc_bounds=None) -> Tensor:
        """Final-norm hidden states.  ``doc_bounds``: the ``(doc_start, doc_end)`` pair of ``ops.doc_bounds`` for
        document-masked attention (explicit only; ``forward`` / ``loss`` derive it from ``doc_mask_token``).  RoPE
        positions stay ``0..S-1``: RoPE scores depend on ``i - j`` only, so within a document the result equals the
        one with positions restarted at the document's first token, up to rounding."""
        assert in_indices.shape[-1] <= self.context_length, "sequence longer than context_length"
        fence = self._bpe_param_fence
        if fence is not None:
            fence(self.token_embeddings)
        x = self.token_embeddings(in_indices)
        if (len(self.layers) and x.dim() == 3
                and all(layer._fused_ok(x) for layer in self.layers)):
            from .fused_block import fused_stack_forward

            return fused_stack_forward(self.layers, self.ln_final, x, fence, doc_bounds)
        for layer in self.layers:
            if fence is not None:
                fence(layer)
            x = layer(x, doc_bounds=doc_bounds) if doc_bounds is not None else layer(x)
        if fence is not None:
            fence(self.ln_final)
        return self.ln_final(x)

    def forward(self, in_indices: Tensor, doc_bounds=None) -> Tensor:
        h = self.hidden_states(in_indices, self._doc_bounds(in_indices, doc_bounds))
        self._fence(self.lm_head)
        return self.lm_head(h)

    def loss(self, in_indices: Tensor, targets: Tensor, ignore_index: int = ops.IGNORE_INDEX,
             doc_bounds=None) -> Tensor:
        """Mean next-token cross-entropy; fused LM head + CE on the GPU.  ``doc_bounds`` / ``doc_mask_token``:
        document-masked attention (:meth:`hidden_states`)."""
        h = self.hidden_states(in_indices, self._doc_bounds(in_indices, doc_bounds))
        self._fence(self.lm_head)
        return ops.lm_head_cross_entropy(h, self.lm_head.weight, targets, ignore_index,
                                         chunk=getattr(self, "lm_head_chunk", None),
                                         mode=getattr(self, "lm_head_mode", None))

    def load_reference_state_dict(self, state_dict: dict, strict: bool = True):
        """Load a reference-format state dict (strips ``torch.compile``'s ``_orig_mod.`` prefix,
        ``tests/conftest.py:201`` in the reference)."""
        sd = {k.replace("_orig_mod.", ""): v for k, v in state_dict.items()}
        return self.load_state_dict(sd, strict=strict)

    def truncated(self, n_layers: int) -> "TransformerLM":
        """A draft model for speculative decoding made of this model's own weights: its embeddings, first
        ``n_layers`` blocks, final norm and LM head, shared with this model (no weight is copied)."""
        assert 1 <= n_layers <= len(self.layers), "n_layers: between 1 and the number of blocks"
        m = TransformerLM.__new__(TransformerLM)
        nn.Module.__init__(m)
        m.config = dataclasses.replace(self.config, num_layers=n_layers)
        m.context_length = self.context_length
        m.token_embeddings = self.token_embeddings
        m.layers = nn.ModuleList(list(self.layers[:n_layers]))
        m.ln_final = self.ln_final
        m.lm_head = self.lm_head
        m.train(self.training)
        return m

    def _generate_speculative(self, prompt, max_new_tokens, temperature, top_p, eos_token_id, generator, top_k, seed,
                              draft_model, num_draft_tokens, prompt_lookup=None):
        from .generation import PromptLookupSession, SpeculativeSession

        if top_k or (top_p is not None and top_p < 1.0):
            if draft_model is None:
                raise ValueError("top_k / top_p cannot be combined with prompt_lookup: speculative verification "
                                 "needs the unwarped distribution of the target")
            raise ValueError("top_k / top_p cannot be combined with draft_model: speculative verification needs "
                             "the unwarped distributions of both models")
        K = int(num_draft_tokens)
        self._fence(self)
        as_list = isinstance(prompt, (list, tuple))
        squeeze = not as_list and prompt.dim() == 1
        ids = list(prompt) if as_list else (prompt.unsqueeze(0) if squeeze else prompt)
        longest = max(int(p.numel()) for p in ids) if as_list else ids.shape[1]
        need = longest + max(max_new_tokens, 0) + K + 1
        if need > min(self.context_length, (self if draft_model is None else draft_model).context_length):
            raise ValueError(f"prompt + max_new_tokens + num_draft_tokens + 1 = {need} exceeds the context length")
        if draft_model is None:
            sess = PromptLookupSession(self, len(ids), K, prompt_lookup, max_len=need)
        else:
            sess = SpeculativeSession(self, draft_model, len(ids), K, max_len=need)
        out = sess.generate(ids, max_new_tokens, temperature, eos_token_id, seed, generator)
        return out[0] if squeeze else out

    @torch.no_grad()
    def generate(
        self,
        prompt: Tensor,
        max_new_tokens: int,
        temperature: float = 1.0,
        top_p: float | None = None,
        eos_token_id: int | None = None,
        generator: torch.Generator | None = None,
        use_cache: bool = True,
        top_k: int | None = None,
        sampler: str = "host",
        seed: int | None = None,
        draft_model: "TransformerLM | None" = None,
        num_draft_tokens: int = 4,
        kv_dtype: str = "bf16",
        weight_dtype: str = "bf16",
        prompt_lookup: "int | tuple[int, int] | None" = None,
        kv_layout: str = "slab",
        num_pages: int | None = None,
        repetition_penalty: float = 1.0,
        presence_penalty: float = 0.0,
        frequency_penalty: float = 0.0,
        logit_bias=None,
        return_logprobs: bool = False,
    ) -> Tensor:
        """Autoregressive sampling (temperature, top-k, nucleus).  ``prompt``: ``[S]`` or ``[B, S]``.

        With ``use_cache`` (and prompt + new tokens within ``context_length``) decoding runs through a KV-cache
        :class:`~bpe_transformer.models.generation.DecodeSession` (HIP-graph-captured decode step on the GPU);
        otherwise every step re-runs the model on the last ``context_length`` tokens.

        A list of 1-D prompts of different lengths is served as one ragged batch (every sequence at its own cache
        position) and returns a list of 1-D tensors, each its prompt plus its continuation up to and including its
        first ``eos_token_id``.

        ``top_k`` keeps the ``top_k`` most likely tokens and is applied before ``top_p``.  ``sampler="device"`` samples
        inside the captured decode graph, from a Philox stream keyed by ``seed`` (``None``: drawn from ``generator``,
        which is otherwise unused in this mode), and syncs with the host every few tokens instead of every token
        (:meth:`DecodeSession.generate`); it needs the KV-cache path.

        ``draft_model`` turns on speculative decoding (:class:`~bpe_transformer.models.generation.SpeculativeSession`):
        the draft proposes ``num_draft_tokens`` tokens per round and this model verifies them in one pass; greedy
        output is this model's own, sampled output is distributed as this model's.  It implies the device sampler
        and cannot be combined with ``top_k`` or ``top_p`` (``ValueError``).  :meth:`truncated` gives a draft
        without a second checkpoint.

        ``kv_dtype="fp8"`` keeps the KV cache as e4m3 rows with power-of-two scales (``DecodeSession(...,
        kv_dtype="fp8")``: about half the cache bytes); it needs the KV-cache path and is not yet supported together
        with ``draft_model`` (``ValueError``).

        ``weight_dtype="fp8"`` decodes with the projection matrices held as e4m3 rows with power-of-two scales
        (``DecodeSession(..., weight_dtype="fp8")``: about half the weight bytes a decode step streams).  The output
        is that of this call on a model whose projection weights are the dequantised rows.  It needs the KV-cache
        path and is not yet supported together with ``draft_model`` (``ValueError``).

        ``kv_layout="paged"`` keeps the KV cache as a pool of 256-token pages behind a block table
        (``DecodeSession(..., kv_layout="paged", num_pages=...)``): a sequence holds the pages it uses, not its
        worst-case context, and the output is that of the slab cache, bit for bit.  ``num_pages`` sizes the pool
        (default: enough for every sequence at full length; a pool that runs out raises ``RuntimeError``).  It needs the
        KV-cache path and is not yet supported together with ``draft_model`` or ``prompt_lookup`` (``ValueError``).

        ``prompt_lookup=n_hi`` (or ``(n_hi, n_lo)``; an int means ``n_lo = 1``) turns on speculative decoding without
        a draft model (:class:`~bpe_transformer.models.generation.PromptLookupSession`): every round proposes the
        ``num_draft_tokens`` tokens that followed the most recent earlier occurrence of the last ``n_lo .. n_hi``
        tokens in the sequence's own prompt and output, and this model verifies them in one pass.  The output
        guarantees, the implied device sampler and the ``ValueError`` with ``top_k`` / ``top_p``, ``kv_dtype="fp8"``
        or ``weight_dtype="fp8"`` are those of ``draft_model``; the two cannot be combined (``ValueError``).

        Sampling controls, all off by default (:meth:`DecodeSession.generate`; ``ops/sampling.py`` states the
        function): ``repetition_penalty`` (> 0, over prompt and output), ``presence_penalty`` and
        ``frequency_penalty`` (over the output), ``logit_bias`` (a ``{token: value}`` dict or a ``[V]`` tensor; ``-inf``
        bans a token) and ``return_logprobs``, which makes the result ``(tokens, logprobs)`` with the log-probability
        of every emitted token under the model's own distribution (not the warped one it was sampled from).  They
        need the KV-cache path, work with either sampler -- with ``sampler="device"`` inside the captured step -- and
        are not yet supported together with ``draft_model`` or ``prompt_lookup`` (``ValueError``).
        """
        assert sampler in ("host", "device"), "sampler: 'host' or 'device'"
        controls = dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                        frequency_penalty=frequency_penalty, logit_bias=logit_bias, return_logprobs=return_logprobs)
        controlled = (repetition_penalty != 1.0 or presence_penalty != 0.0 or frequency_penalty != 0.0
                      or logit_bias is not None or return_logprobs)
        if controlled and (draft_model is not None or prompt_lookup is not None):
            raise ValueError("repetition_penalty / presence_penalty / frequency_penalty / logit_bias / return_logprobs "
                             f"with {'draft_model' if draft_model is not None else 'prompt_lookup'} are not supported "
                             "yet: the verifier's p and q would both need the processing")
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype: 'bf16' or 'fp8', got {kv_dtype!r}")
        if kv_layout not in ("slab", "paged"):
            raise ValueError(f"kv_layout: 'slab' or 'paged', got {kv_layout!r}")
        if num_pages is not None and kv_layout != "paged":
            raise ValueError("num_pages needs kv_layout='paged'")
        if kv_layout != "slab" and (draft_model is not None or prompt_lookup is not None):
            raise ValueError(f"kv_layout={kv_layout!r} with {'draft_model' if draft_model is not None else 'prompt_lookup'}"
                             " is not supported yet: speculative decoding runs on the slab cache only")
        if weight_dtype not in ("bf16", "fp8"):
            raise ValueError(f"weight_dtype: 'bf16' or 'fp8', got {weight_dtype!r}")
        if prompt_lookup is not None:
            from .generation import _lookup_bounds

            if draft_model is not None:
                raise ValueError("prompt_lookup cannot be combined with draft_model: a round has one proposer")
            _lookup_bounds(prompt_lookup)
            for name, v in (("kv_dtype", kv_dtype), ("weight_dtype", weight_dtype)):
                if v != "bf16":
                    raise ValueError(f"{name}='fp8' with prompt_lookup is not supported yet: speculative decoding "
                                     "runs on the bf16 cache and bf16 weights only")
            return self._generate_speculative(prompt, max_new_tokens, temperature, top_p, eos_token_id, generator,
                                              top_k, seed, None, num_draft_tokens, prompt_lookup)
        if draft_model is not None:
            if weight_dtype != "bf16":
                raise ValueError("weight_dtype='fp8' with draft_model is not supported yet: speculative decoding runs "
                                 "on bf16 weights only")
            if kv_dtype != "bf16":
                raise ValueError("kv_dtype='fp8' with draft_model is not supported yet: speculative decoding runs on "
                                 "the bf16 cache only")
            return self._generate_speculative(prompt, max_new_tokens, temperature, top_p, eos_token_id, generator,
                                              top_k, seed, draft_model, num_draft_tokens)
        kw = dict(top_k=top_k, sampler=sampler, seed=seed)
        if controlled:
            kw.update(controls)
        if isinstance(prompt, (list, tuple)):
            self._fence(self)
            longest = max(int(p.numel()) for p in prompt)
            if use_cache and longest + max_new_tokens <= self.context_length and max_new_tokens > 0:
                from .generation import DecodeSession

                sess = DecodeSession(self, len(prompt), max_len=longest + max_new_tokens, ragged=True,
                                     kv_dtype=kv_dtype, weight_dtype=weight_dtype, kv_layout=kv_layout,
                                     num_pages=num_pages)
                return sess.generate(list(prompt), max_new_tokens, temperature, top_p, eos_token_id, generator, **kw)
            # without the cache: one sequence at a time through the loop below (which stops at its EOS)
            return [self.generate(p.reshape(-1), max_new_tokens, temperature, top_p, eos_token_id, generator, use_cache,
                                  kv_dtype=kv_dtype, weight_dtype=weight_dtype, kv_layout=kv_layout,
                                  num_pages=num_pages, **kw) for p in prompt]
        squeeze = prompt.dim() == 1
        ids = prompt.unsqueeze(0) if squeeze else prompt
        self._fence(self)  # the decode session packs / reads every weight up front
        if use_cache and ids.shape[1] + max_new_tokens <= self.context_length and max_new_tokens > 0:
            from .generation import DecodeSession

            sess = DecodeSession(self, ids.shape[0], max_len=ids.shape[1] + max_new_tokens, kv_dtype=kv_dtype,
                                 weight_dtype=weight_dtype, kv_layout=kv_layout, num_pages=num_pages)
            out = sess.generate(ids, max_new_tokens, temperature, top_p, eos_token_id, generator, **kw)
            if return_logprobs:
                return (out[0][0], out[1][0]) if squeeze else out
            return out[0] if squeeze else out
        assert not controlled or max_new_tokens <= 0, "the sampling controls need the KV-cache path (use_cache, and " \
            "prompt + max_new_tokens within context_length)"
        assert sampler == "host" or max_new_tokens <= 0, "sampler='device' needs the KV-cache path (use_cache, and " \
            "prompt + max_new_tokens within context_length)"
        assert kv_dtype == "bf16" or max_new_tokens <= 0, "kv_dtype='fp8' needs the KV-cache path (use_cache, and " \
            "prompt + max_new_tokens within context_length)"
        assert weight_dtype == "bf16" or max_new_tokens <= 0, "weight_dtype='fp8' needs the KV-cache path (use_cache, " \
            "and prompt + max_new_tokens within context_length)"
        assert kv_layout == "slab" or max_new_tokens <= 0, "kv_layout='paged' needs the KV-cache path (use_cache, and " \
            "prompt + max_new_tokens within context_length)"
        for _ in range(max_new_tokens):
            ctx = ids[:, -self.context_length :]
            # (sampling is not document-masked: hidden_states takes explicit bounds only, never doc_mask_token)
            logits = self.lm_head(self.hidden_states(ctx))[:, -1, :].float()
            if temperature <= 0:
                nxt = logits.argmax(-1, keepdim=True)
            else:
                if top_k:
                    from .generation import _top_k_logits

                    logits = _top_k_logits(logits, top_k)
                probs = torch.softmax(logits / temperature, dim=-1)
                if top_p is not None and top_p < 1.0:
                    sp, si = probs.sort(dim=-1, descending=True)
                    keep = sp.cumsum(-1) - sp < top_p
                    sp = sp * keep
                    probs = torch.zeros_like(probs).scatter_(-1, si, sp)
                    probs = probs / probs.sum(-1, keepdim=True)
                nxt = torch.multinomial(probs, 1, generator=generator)
            ids = torch.cat([ids, nxt], dim=1)
            if eos_token_id is not None and bool((nxt == eos_token_id).all()):
                break
        return ids[0] if squeeze else ids
