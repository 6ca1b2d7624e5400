"""Shared pieces of the fp8-weight tests (``tests/test_w8.py``, ``tests/test_w8_gpu.py``).

The feature is defined by an equality: a session with fp8 weights is a bf16 (or fp32) session on a model whose
projection weights are ``weight_dequantize(weight_quantize(W))``.  :func:`dequantised` builds that model here, from
the public quantiser alone, so the tests do not lean on the session's own helper.
"""

from __future__ import annotations

import copy

import torch
from torch import Tensor

from bpe_transformer.models import TransformerLM
from bpe_transformer.ops.decode import weight_dequantize, weight_quantize

VOCAB = 301


def tiny_model(device="cpu", dtype=torch.float32, seed: int = 0) -> TransformerLM:
    """2 layers, d_model 128, 2 heads of 64, d_ff 256, vocab 301."""
    torch.manual_seed(seed)
    return TransformerLM(vocab_size=VOCAB, context_length=64, d_model=128, num_layers=2, num_heads=2, d_ff=256,
                         device=device, dtype=dtype).eval()


def dequantised(model: TransformerLM) -> TransformerLM:
    """A copy of ``model`` with Wq, Wk, Wv, Wo, W1, W2, W3 and the LM head replaced by their dequantised rows."""
    m = copy.deepcopy(model)
    lins = [m.lm_head]
    for layer in m.layers:
        a, f = layer.attn, layer.ffn
        lins += [a.q_proj, a.k_proj, a.v_proj, a.output_proj, f.w1, f.w2, f.w3]
    with torch.no_grad():
        for lin in lins:
            w = lin.weight
            w.copy_(weight_dequantize(*weight_quantize(w), w.dtype))
    return m


def prompt(B: int, T: int, seed: int = 0) -> Tensor:
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(0, VOCAB, (B, T), generator=g)


def run_session(sess, B: int, first: int = 5, steps: int = 3, second: int = 4, lengths=None) -> list[Tensor]:
    """Prefill ``first`` tokens, ``steps`` greedy decode steps, a second-turn append of ``second`` tokens, one more
    decode step; -> every logits tensor on the way (CPU)."""
    out = []
    lg = sess.prefill(prompt(B, first), lengths)
    out.append(lg)
    for _ in range(steps):
        lg = sess.decode(lg.float().argmax(-1))
        out.append(lg)
    if second:
        lg = sess.prefill(prompt(B, second, seed=1))
        out.append(lg)
        out.append(sess.decode(lg.float().argmax(-1)))
    return [t.detach().float().cpu() for t in out]
