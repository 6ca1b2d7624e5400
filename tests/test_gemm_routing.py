"""CPU tests of the weight-gradient routing decisions in ``ops/gemm.py`` (no kernel runs here; the kernels' numerics
are in tests/test_kernels_gpu.py)."""

from __future__ import annotations

import torch

from bpe_transformer.ops import gemm


def test_accumulate_weight_grad_on_cpu_tensors_takes_the_library_route():
    """Off the GPU ``accumulate_weight_grad`` accumulates through ``addmm_``: right against the fp32 product and the
    same on two runs."""
    t = 256
    dy = torch.randn(t, 256, dtype=torch.bfloat16)
    x = torch.randn(t, 512, dtype=torch.bfloat16)
    g1 = torch.zeros(256, 512, dtype=torch.bfloat16)
    g2 = torch.zeros(256, 512, dtype=torch.bfloat16)
    gemm.accumulate_weight_grad(g1, dy, x)
    gemm.accumulate_weight_grad(g2, dy, x)
    ref = dy.float().t() @ x.float()
    assert torch.allclose(g1.float(), ref, rtol=2e-2, atol=2e-1) and torch.equal(g1, g2)


def test_removed_ops_are_gone_and_groups_summary_is_empty():
    """The grouped dW launch and the fused fp8 SwiGLU-backward GEMM were removed: the library registers neither op
    (loading it needs no GPU), and ``groups_summary()``, which bench.py still prints as "dw_gemm_groups", is empty."""
    from bpe_transformer.ops._ext import ops

    h = ops()
    assert hasattr(h, "gemm_pp") and hasattr(h, "gemm_fp8_swiglu")  # the namespace is the loaded library's
    assert not hasattr(h, "gemm_pp_dw_group") and not hasattr(h, "gemm_fp8_swiglu_bwd")
    assert gemm.groups_summary() == {}


def test_ppt_candidate_only_when_the_transpose_fits_32_bit_offsets():
    assert "ppt" in gemm._candidates(2304, 768, 131072)
    big = 2**31 // 256 + 64  # X^T's leading dimension T times 256 rows past 2^31
    cands = gemm._candidates(2304, 768, big - big % 64)
    assert "ppt" not in cands and "pp" in cands


def test_swiglu_forward_fusion_rule(monkeypatch):
    """The fused [W1;W3] + gate GEMM: d_model <= 1024 at any token count; wider only at >= 65 536 tokens per
    micro-batch (where the L2-aware tile order made it win, profiles/bench/ab_llama_swiglu_fwd_fused_r6.log); an
    explicit BPE_FUSE_SWIGLU_FWD_MAX_D cap replaces the rule."""
    from bpe_transformer.models import fused_block as fb

    def probe(t, d, f):
        x = torch.empty(t, d, device="meta", dtype=torch.bfloat16)
        return fb._fuse_swiglu_fwd(x, torch.empty(2 * f, d, device="meta", dtype=torch.bfloat16))

    monkeypatch.setattr(fb, "_FUSE_SWIGLU_FWD_MAX_D", 0)
    assert probe(131072, 768, 2048) and probe(512, 768, 2048)
    assert probe(65536, 2048, 5632) and not probe(16384, 2048, 5632)
    assert not probe(65536 + 64, 2048, 5632)  # tokens not a multiple of the 256-row tiles
    monkeypatch.setattr(fb, "_FUSE_SWIGLU_FWD_MAX_D", 1024)
    assert not probe(65536, 2048, 5632) and probe(256, 1024, 512)
