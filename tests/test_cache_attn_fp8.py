"""``prefill_attention_fp8`` on the CPU, the rounding argument of the fp8 ``cache_attn`` kernel, and the session
without a dequantisation scratch (``csrc/flash_attn_cache.hip``, ``Fp8Cache``; ``models/generation.py``).

The cases are those of ``tests/test_cache_attn_fp8_gpu.py`` (``tests/cache_attn_fp8_refs.py``).
"""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.models.generation import KVCache
from bpe_transformer.ops import decode as OD

from . import cache_attn_fp8_refs as FR
from . import cache_prefill_refs as CR
from . import kv_fp8_refs as KR


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", FR.IDS)
def test_prefill_attention_fp8_cpu(name, D):
    """The CPU path against float64 on the ``dequantize64`` caches, each sequence at its own position."""
    c = FR.case(D, name)
    out = OD.prefill_attention_fp8(c["q"], c["k8"], c["v8"], c["ks"], c["vs"], c["pos"], c["H"], n_new=c["T"])
    assert out.shape == c["q"].shape and out.dtype == c["q"].dtype
    for b in range(len(c["plist"])):
        got = FR.specified(c, out, b)
        assert torch.isfinite(got).all(), (name, b)
        assert CR.global_rel(got, c["ref"][b]) < CR.TOL_GLOBAL, (name, b, CR.global_rel(got, c["ref"][b]))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", FR.IDS)
def test_conversion_pass_is_exact_and_emulations_agree_bitwise(name, D):
    """Design (a): the tile conversion ``bf16(e4m3 * scale)`` rounds nothing (the fp32 product is a bf16 value) and
    gives the bits of the dequantised bf16 cache; the kernel's rounding points after it are the bf16 kernel's, so
    the two emulations agree bit for bit, and both meet the GPU test's float64 bound."""
    c = FR.case(D, name)
    for b, p in enumerate(c["plist"]):
        L = min(p + c["T"], c["Lmax"])
        for t8, ts, td in ((c["k8"], c["ks"], c["k"]), (c["v8"], c["vs"], c["v"])):
            x32, xb = FR.convert(t8[b, :, :L], ts[b, :, :L])
            assert torch.equal(xb.float(), x32), "the fp32 product is representable in bf16"
            assert torch.equal(xb.view(torch.int16), td[b, :, :L].view(torch.int16))
            assert torch.equal(xb, OD.kv_dequantize_reference(t8[b, :, :L], ts[b, :, :L]))
    a, d = FR.emulate_fp8(c), FR.emulate_dequantised(c)
    for b in range(len(c["plist"])):
        ga, gd = FR.specified(c, a, b), FR.specified(c, d, b)
        assert torch.isfinite(ga).all()
        assert torch.equal(ga.view(torch.int16), gd.view(torch.int16)), (name, b)
        assert CR.global_rel(ga, c["ref"][b]) < CR.TOL_GLOBAL, (name, b, CR.global_rel(ga, c["ref"][b]))


def test_spread_case_has_scales_2_to_17_apart():
    c = FR.case(64, "scales 2^20 apart")
    assert float(c["ks"][0, 0, 0] / c["ks"][0, 0, 1]) >= 2.0 ** 17 and float(c["vs"][0, 0, 1] / c["vs"][0, 0, 0]) >= 2.0 ** 17


def test_poison_is_where_the_cases_say():
    for name in FR.IDS:
        c = FR.case(64, name)
        for b, p in enumerate(c["plist"]):
            L = min(p + c["T"], c["Lmax"])
            assert torch.isfinite(c["ks"][b, :, :L]).all() and torch.isfinite(c["vs"][b, :, :L]).all()
            assert torch.isnan(c["ks"][b, :, L:]).all() and bool((KR.codes(c["v8"])[b, :, L:] == KR.NAN_BYTE).all())


def test_fp8_session_has_no_dequant_scratch():
    torch.manual_seed(0)
    m = TransformerLM(vocab_size=100, context_length=64, d_model=128, num_layers=2, num_heads=2, d_ff=256).eval()
    sess = DecodeSession(m, 2, max_len=48, kv_dtype="fp8")
    assert not sess.fast
    ids = torch.randint(0, 100, (2, 30))
    sess.prefill(ids[:, :20])
    sess.prefill(ids[:, 20:])
    assert not hasattr(sess.cache, "dequant_scratch") and not hasattr(sess.cache, "_deq")
    assert not hasattr(KVCache, "dequant_scratch")


def test_fp8_cache_nbytes_unchanged():
    L, B, Hkv, Lmax, D = 3, 2, 4, 40, 64
    c = KVCache(L, B, Hkv, Lmax, D, kv_dtype="fp8")
    assert c.nbytes() == 2 * L * B * Hkv * Lmax * (D + 4)
    assert KVCache(L, B, Hkv, Lmax, D).nbytes() == 2 * L * B * Hkv * Lmax * D * 2
