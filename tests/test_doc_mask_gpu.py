"""Document-masked flash attention on the GPU: the DOC variants of fa_fwd_kernel and the split backward against the
fp32 oracle (``ops.attention_qkv_reference``), their isolation, routing and refusals, and the fused block / model."""

from __future__ import annotations

import copy
import functools

import pytest
import torch

from bpe_transformer import ops
from bpe_transformer.models import TransformerLM
from bpe_transformer.ops import reference as R

pytestmark = pytest.mark.gpu

# Row 0: a length-1 document and boundaries on a 32-step (32), a 64-tile (64), a 128-block (128) edge and in mid-tile
# (193); row 1: a boundary in the last partial query block, no skippable tile; row 2: the last query block skips three
# key tiles and the first key blocks end their query sweep early.
S320 = [[1, 31, 32, 64, 65, 127], [300, 20], [200, 120]]
# D = 128 (64-key / 64-query tiles), GQA 4:2: one boundary in mid-tile, one row that is a single document
S192 = [[70, 122], [192]]
# boundary at 96: wave 3 of the only query block (queries 96..127) finds its first processed tile (keys 0..63) fully
# masked in the forward
S128 = [[96, 32]]


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def bounds_from_lengths(rows, device):
    S = sum(rows[0])
    start = torch.empty(len(rows), S, dtype=torch.int32)
    end = torch.empty(len(rows), S, dtype=torch.int32)
    for b, lens in enumerate(rows):
        assert sum(lens) == S
        p = 0
        for n in lens:
            start[b, p : p + n] = p
            end[b, p : p + n] = p + n
            p += n
    return start.to(device), end.to(device)


def _inputs(B, S, H, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    do = torch.randn(B * S, H * D, generator=g).to(torch.bfloat16)
    return qkv, do


def _run_gpu(dev, qkv, do, B, S, H, Hkv, D, cos, sin, doc):
    x = qkv.to(dev).requires_grad_(True)
    o = ops.flash_attention_qkv(x, B, S, H, Hkv, D, cos, sin, True, doc_bounds=doc)
    o.backward(do.to(dev))
    return o.detach().cpu(), x.grad.cpu()


@functools.lru_cache(maxsize=None)
def _oracle(name: str, rope: bool):
    """The fp32 oracle's O and dqkv for one layout, computed once and shared (never modified)."""
    rows, H, Hkv, D = {"s320": (S320, 4, 4, 64), "s192": (S192, 4, 2, 128), "s128": (S128, 4, 4, 64)}[name]
    B, S = len(rows), sum(rows[0])
    qkv, do = _inputs(B, S, H, Hkv, D, seed=len(name) + S)
    cos = sin = None
    if rope:
        cos, sin = R.rope_tables(D, S + 16, 10000.0)
    start, _ = bounds_from_lengths(rows, "cpu")
    x = qkv.float().requires_grad_(True)
    o = ops.attention_qkv_reference(x, B, S, H, Hkv, D, cos, sin, True, doc_start=start)
    o.backward(do.float())
    return (rows, B, S, H, Hkv, D), qkv, do, cos, sin, o.detach(), x.grad


def _check_against_oracle(o, g, o_ref, g_ref, H, Hkv, D):
    e = rel(o, o_ref)
    print(f"O rel {e:.3e}")
    errs = {"o": e}
    q, kv = H * D, Hkv * D
    for name, sl in (("dq", slice(0, q)), ("dk", slice(q, q + kv)), ("dv", slice(q + kv, q + 2 * kv))):
        errs[name] = rel(g[:, sl], g_ref[:, sl])
        print(f"{name} rel {errs[name]:.3e}")
    assert errs["o"] < 2e-2, errs
    assert max(errs["dq"], errs["dk"], errs["dv"]) < 3e-2, errs


@pytest.mark.parametrize("name,rope", [("s320", True), ("s320", False), ("s192", True), ("s128", False)])
def test_doc_kernels_match_oracle(gpu_device, name, rope):
    """Forward and dq / dk / dv of the DOC kernels against the masked fp32 oracle, at the tolerances of
    tests/test_kernels_gpu.py's flash-attention tests (rel < 2e-2 on O, < 3e-2 on the gradients)."""
    (rows, B, S, H, Hkv, D), qkv, do, cos, sin, o_ref, g_ref = _oracle(name, rope)
    doc = bounds_from_lengths(rows, gpu_device)
    c, s = (None, None) if cos is None else (cos.to(gpu_device), sin.to(gpu_device))
    o, g = _run_gpu(gpu_device, qkv, do, B, S, H, Hkv, D, c, s, doc)
    assert torch.isfinite(o.float()).all() and torch.isfinite(g.float()).all()
    _check_against_oracle(o, g, o_ref, g_ref, H, Hkv, D)


def test_doc_path_ignores_kernel_selectors(gpu_device):
    """A document-masked call takes fa_fwd_kernel and the split 32-row backward whatever fa_fwd_config,
    fa_bwd_config and fa_dq_config select: its results do not change, bit for bit, when they do."""
    (rows, B, S, H, Hkv, D), qkv, do, cos, sin, _, _ = _oracle("s320", True)
    doc = bounds_from_lengths(rows, gpu_device)
    c, s = cos.to(gpu_device), sin.to(gpu_device)
    hip = torch.ops.bpe_hip
    o0, g0 = _run_gpu(gpu_device, qkv, do, B, S, H, Hkv, D, c, s, doc)
    prev = hip.fa_fwd_config(2), hip.fa_bwd_config(1), hip.fa_dq_config(1)
    try:
        o1, g1 = _run_gpu(gpu_device, qkv, do, B, S, H, Hkv, D, c, s, doc)
    finally:
        hip.fa_fwd_config(prev[0]), hip.fa_bwd_config(prev[1]), hip.fa_dq_config(prev[2])
    assert torch.equal(o0, o1) and torch.equal(g0, g1)


def test_doc_isolation_is_bitwise(gpu_device):
    """Other finite random values in the qkv and dO rows of document 4 of batch row 0 (tokens 128..192) leave O, dq,
    dk and dv of every other document's rows bitwise unchanged: the kernels are deterministic and a masked
    probability is an exact zero, so any difference is a leak."""
    (rows, B, S, H, Hkv, D), qkv, do, cos, sin, _, _ = _oracle("s320", True)
    doc = bounds_from_lengths(rows, gpu_device)
    c, s = cos.to(gpu_device), sin.to(gpu_device)
    o0, g0 = _run_gpu(gpu_device, qkv, do, B, S, H, Hkv, D, c, s, doc)
    g = torch.Generator().manual_seed(99)
    qkv2, do2 = qkv.clone(), do.clone()
    lo, hi = 128, 193  # document 4 of row 0 (starts 0, 1, 32, 64, 128, 193)
    qkv2[lo:hi] = (3 * torch.randn(hi - lo, qkv.shape[1], generator=g)).to(torch.bfloat16)
    do2[lo:hi] = (3 * torch.randn(hi - lo, do.shape[1], generator=g)).to(torch.bfloat16)
    o1, g1 = _run_gpu(gpu_device, qkv2, do2, B, S, H, Hkv, D, c, s, doc)
    keep = torch.ones(B * S, dtype=torch.bool)
    keep[lo:hi] = False
    assert not torch.equal(o0[~keep], o1[~keep])  # the replaced document did change
    assert torch.equal(o0[keep], o1[keep])
    assert torch.equal(g0[keep], g1[keep])


def test_one_document_bounds_match_plain_causal(gpu_device):
    """doc_start = 0, doc_end = S: the document path (general forward, 32-row split backward) agrees with the plain
    causal call (the default kernels) within the oracle tolerances, at S = 200."""
    B, S, H, Hkv, D = 2, 200, 4, 4, 64
    qkv, do = _inputs(B, S, H, Hkv, D, seed=5)
    cos, sin = R.rope_tables(D, S, 10000.0, device=gpu_device)
    doc = bounds_from_lengths([[S]] * B, gpu_device)
    o0, g0 = _run_gpu(gpu_device, qkv, do, B, S, H, Hkv, D, cos, sin, None)
    o1, g1 = _run_gpu(gpu_device, qkv, do, B, S, H, Hkv, D, cos, sin, doc)
    _check_against_oracle(o1, g1, o0, g0, H, Hkv, D)


def test_refusals(gpu_device):
    B, S, H, Hkv, D = 1, 64, 2, 2, 64
    qkv, _ = _inputs(B, S, H, Hkv, D, seed=6)
    x = qkv.to(gpu_device)
    start, end = bounds_from_lengths([[40, 24]], gpu_device)

    def call(doc, causal=True):
        return ops.flash_attention_qkv(x, B, S, H, Hkv, D, None, None, causal, doc_bounds=doc)

    call((start, end))  # the accepted form
    with pytest.raises(ValueError, match="causal"):
        call((start, end), causal=False)
    with pytest.raises(TypeError, match="int32"):
        call((start.long(), end))
    with pytest.raises(TypeError, match="int32"):
        call((start, end.float()))
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        call((start[:, :32], end))
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        call((start, end.expand(2, S)))
    with pytest.raises(ValueError, match="cpu"):
        call((start.cpu(), end))
    with pytest.raises(TypeError):
        call(start)
    # the ops themselves check too (callers that go around the wrapper: the fused block)
    q, k, v = x[:, : H * D], x[:, H * D : (H + Hkv) * D], x[:, (H + Hkv) * D :]
    hip = torch.ops.bpe_hip
    with pytest.raises(RuntimeError, match="causal"):
        hip.fa_fwd_doc(q, k, v, start, end, B, S, H, Hkv, D, False, False, 0.125)
    with pytest.raises(RuntimeError, match="int32"):
        hip.fa_fwd_doc(q, k, v, start.long(), end, B, S, H, Hkv, D, True, False, 0.125)
    with pytest.raises(RuntimeError, match="device"):
        hip.fa_fwd_doc(q, k, v, start, end.cpu(), B, S, H, Hkv, D, True, False, 0.125)
    with pytest.raises(RuntimeError, match=r"\[B, S\]"):
        hip.fa_fwd_doc(q, k, v, start.t().contiguous(), end, B, S, H, Hkv, D, True, False, 0.125)


def _model_pair(gpu_device, eot):
    torch.manual_seed(0)
    ref = TransformerLM(vocab_size=1000, context_length=320, d_model=256, num_layers=2, num_heads=4, d_ff=512)
    gpu = copy.deepcopy(ref).to(gpu_device, torch.bfloat16)
    ref.doc_mask_token = gpu.doc_mask_token = eot
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 1000, (2, 320), generator=g)
    tgt = torch.randint(1, 1000, (2, 320), generator=g)
    for b, cuts in enumerate(([0, 31, 63, 127, 192], [299])):  # separators: row 0 as S320's row 0, row 1 [300, 20]
        ids[b, cuts] = eot
    return ref, gpu, ids, tgt


def _grad_errs(ref, gpu):
    return {n: float((pg.grad.float().cpu() - pr.grad).norm() / pr.grad.norm().clamp_min(1e-12))
            for (n, pr), (_, pg) in zip(ref.named_parameters(), gpu.named_parameters())}


def test_fused_model_matches_masked_oracle(gpu_device):
    """The bf16 model on the fused blocks (d 256, 4 heads, 2 layers, S 320, B 2) with doc_mask_token set against the
    same model in fp32 on the CPU (``_forward_reference`` with the mask): loss and every parameter's gradient at
    the bounds of tests/test_model_gpu.py's fused-vs-oracle test (|loss| < 3e-2, gradient rel. norm < 0.08)."""
    ref, gpu, ids, tgt = _model_pair(gpu_device, eot=0)
    l_ref = ref.loss(ids, tgt)
    l_ref.backward()
    l_gpu = gpu.loss(ids.to(gpu_device), tgt.to(gpu_device))
    l_gpu.backward()
    errs = _grad_errs(ref, gpu)
    print(f"loss gpu {l_gpu.item():.5f} ref {l_ref.item():.5f}; worst grad rel {max(errs.values()):.3e}")
    assert abs(l_gpu.item() - l_ref.item()) < 3e-2
    for n, e in errs.items():
        assert e < 0.08, (n, e)
    # explicit bounds give the same result as the attribute, bit for bit
    gpu.doc_mask_token = None
    l_exp = gpu.loss(ids.to(gpu_device), tgt.to(gpu_device), doc_bounds=ops.doc_bounds(ids.to(gpu_device), 0))
    assert torch.equal(l_exp, l_gpu)


def test_fp8_model_matches_masked_oracle(gpu_device):
    """The same comparison on the fp8 path (enable_fp8 takes this width: 640 tokens and d 256 meet the fp8 shape
    rules, the QKV projection falling back from the hand RoPE-epilogue kernel to the library GEMM + ``rope_qk_`` at
    a token count that is no multiple of 256), after one calibration step.  Bounds: this project's fp8-vs-bf16 bounds
    (tests/test_model_gpu.py test_fp8_close_to_bf16: |loss| < 2e-2, gradient rel. norm < 0.2) added to its
    bf16-vs-oracle bounds (3e-2, 0.08) -- the triangle inequality over the two comparisons it already makes."""
    ref, gpu, ids, tgt = _model_pair(gpu_device, eot=0)
    gpu.enable_fp8()
    x, y = ids.to(gpu_device), tgt.to(gpu_device)
    gpu.loss(x, y).backward()  # calibration step
    for st in gpu.fp8_states():
        st.update()
    gpu.zero_grad()
    l_ref = ref.loss(ids, tgt)
    l_ref.backward()
    l_gpu = gpu.loss(x, y)
    l_gpu.backward()
    errs = _grad_errs(ref, gpu)
    print(f"loss fp8 {l_gpu.item():.5f} ref {l_ref.item():.5f}; worst grad rel {max(errs.values()):.3e}")
    assert abs(l_gpu.item() - l_ref.item()) < 5e-2
    for n, e in errs.items():
        assert e < 0.28, (n, e)
