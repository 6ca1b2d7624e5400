"""fp8 weights for serving, CPU: the format (``ops/decode.py: weight_quantize`` / ``weight_dequantize``) and the
definition of the session mode -- ``DecodeSession(..., weight_dtype="fp8")`` is a session on the model whose
projection weights are the dequantised rows, logits ``torch.equal``.

Nothing here has a tolerance of its own: the checks are bitwise, except the quantisation error bound, which is the
format's (e4m3 has 3 mantissa bits: half an ulp is ``2^-4`` relative for normal values, ``|w| >= 2^-6 s``; below that
the subnormal spacing is ``2^-9 s``, half of it ``2^-10 s``).
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models import DecodeSession
from bpe_transformer.ops import decode as OD

from . import w8_refs as WR

FP8 = torch.float8_e4m3fn


def _format_matrix() -> torch.Tensor:
    """Rows: scales spread over 2^-20 .. 2^10 (31 rows), an all-zero row, a row whose amax is exactly 448 s, a row
    with e4m3-subnormal entries, a row with inf.  bf16 values, K = 64."""
    g = torch.Generator().manual_seed(7)
    K = 64
    rows = [torch.randn(K, generator=g) * 2.0 ** e for e in range(-20, 11)]
    rows.append(torch.zeros(K))
    edge = torch.randn(K, generator=g)
    edge = edge / edge.abs().max() * 40.0
    edge[3] = -56.0  # 56 = 0.875 * 2^6: s = 2^-3 and 56 / s = 448 exactly
    rows.append(edge)
    sub = torch.zeros(K)
    sub[0] = 448.0  # s = 1: e4m3 subnormals are the multiples of 2^-9 below 2^-6
    sub[1:7] = torch.tensor([2.0 ** -9, 3 * 2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -7, 2.0 ** -10, 2.0 ** -6])
    rows.append(sub)
    bad = torch.randn(K, generator=g)
    bad[5] = math.inf
    rows.append(bad)
    return torch.stack(rows).to(torch.bfloat16)


def test_weight_quantize_is_the_cache_quantiser_row_by_row():
    w = _format_matrix()
    w8, s = OD.weight_quantize(w)
    assert w8.dtype == FP8 and w8.shape == w.shape and s.dtype == torch.float32 and s.shape == (w.shape[0],)
    for n in range(w.shape[0]):
        q, sn = OD.kv_quantize_reference(w[n])
        if n == w.shape[0] - 1:  # the inf row: s = NaN, bytes unspecified
            assert math.isnan(float(sn)) and math.isnan(float(s[n]))
            continue
        assert float(s[n]) == float(sn), n
        assert torch.equal(w8[n].view(torch.uint8), q.view(torch.uint8)), n
    assert float(s[31]) == 1.0  # the all-zero row
    assert float(s[32]) == 2.0 ** -3 and float(w8[32].float().abs().max()) == 448.0
    assert torch.equal(w8[33].float()[:7], w[33].float()[:7].where(w[33].float()[:7] != 2.0 ** -10, torch.zeros(())))
    fin = s[:31]
    assert bool((fin == 2.0 ** torch.log2(fin).round()).all()) and float(fin.min()) < 2.0 ** -20 < 1 < float(fin.max())


def test_weight_dequantize_is_exact():
    w = _format_matrix()[:-1]
    w8, s = OD.weight_quantize(w)
    d32 = OD.weight_dequantize(w8, s, torch.float32)
    assert torch.equal(d32, w8.float() * s[:, None])
    d16 = OD.weight_dequantize(w8, s)
    assert d16.dtype == torch.bfloat16 and torch.equal(d16.float(), d32)  # representable in bf16
    assert torch.equal(d32.to(torch.bfloat16).float(), d32)
    out = torch.empty_like(d16)
    assert OD.w_dequant(w8, s, out) is out and torch.equal(out, d16)
    # quantising the dequantised rows again changes nothing (the property the session equality rests on)
    w8b, sb = OD.weight_quantize(d16)
    assert torch.equal(OD.weight_dequantize(w8b, sb), d16)


def test_weight_quantisation_error_bound():
    w = _format_matrix()[:-1].float()
    w8, s = OD.weight_quantize(w)
    err = (OD.weight_dequantize(w8, s, torch.float32) - w).abs()
    sc = s[:, None]
    normal = w.abs() >= 2.0 ** -6 * sc
    assert bool((err[normal] <= 2.0 ** -4 * w.abs()[normal]).all())
    assert bool((err[~normal] <= (2.0 ** -10 * sc).expand_as(w)[~normal]).all())
    assert normal.any() and (~normal).any()


def test_cpu_references_dequantise():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 64, generator=g).to(torch.bfloat16)
    w = (torch.randn(16, 64, generator=g) / 8).to(torch.bfloat16)
    w8, s = OD.weight_quantize(w)
    wd = OD.weight_dequantize(w8, s)
    for swiglu in (False, True):
        a, _ = OD.decode_gemv(x, w8, swiglu=swiglu, w_scale=s)
        b, _ = OD.decode_gemv(x, wd, swiglu=swiglu)
        assert torch.equal(a, b)
    part = torch.randn(2, 1, 2, 66, generator=g)
    part[..., 65] = part[..., 65].abs() + 0.5
    assert torch.equal(OD.decode_attn_proj(part, w8, s), OD.decode_attn_proj(part, wd))


@pytest.fixture(scope="module")
def models():
    m = WR.tiny_model()
    return m, WR.dequantised(m)


@pytest.mark.parametrize("kw", [{}, {"prefill_chunk": 3}, {"kv_dtype": "fp8"}, {"kv_dtype": "fp8", "prefill_chunk": 3}],
                         ids=["plain", "chunk3", "kv8", "kv8-chunk3"])
def test_session_is_a_session_on_the_dequantised_model(models, kw):
    model, ref = models
    B = 2
    got = WR.run_session(DecodeSession(model, B, weight_dtype="fp8", **kw), B)
    want = WR.run_session(DecodeSession(ref, B, **kw), B)
    plain = WR.run_session(DecodeSession(model, B, **kw), B)
    assert len(got) == 6
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], plain[0])  # the quantisation is really there


@pytest.mark.parametrize("kw", [{}, {"kv_dtype": "fp8"}], ids=["bf16kv", "kv8"])
def test_ragged_session(models, kw):
    model, ref = models
    B = 2
    outs = []
    for m, extra in ((model, {"weight_dtype": "fp8"}), (ref, {})):
        s = DecodeSession(m, B, ragged=True, **kw, **extra)
        lg = [s.prefill(WR.prompt(B, 5), [5, 2])]
        lg.append(s.decode(lg[-1].argmax(-1)))
        lg.append(s.decode(lg[-1].argmax(-1), active=[True, False])[:1])
        lg.append(s.prefill_slot(1, WR.prompt(1, 3, seed=2)[0]))
        assert s.cache.lengths == [7, 6]
        outs.append(lg)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_generate(models):
    model, ref = models
    p = WR.prompt(2, 4, seed=5)
    a = model.generate(p, 6, temperature=0.0, weight_dtype="fp8")
    assert a.shape == (2, 10) and torch.equal(a, ref.generate(p, 6, temperature=0.0))
    kw = dict(temperature=1.0, top_k=20, sampler="device", seed=11)
    assert torch.equal(model.generate(p, 6, weight_dtype="fp8", **kw), ref.generate(p, 6, **kw))
    lp = [p[0], p[1, :2]]
    for x, y in zip(model.generate(lp, 5, temperature=0.0, weight_dtype="fp8"), ref.generate(lp, 5, temperature=0.0)):
        assert torch.equal(x, y)


def test_the_model_is_left_alone(models):
    model, _ = models
    before = {k: v.clone() for k, v in model.state_dict().items()}
    s = DecodeSession(model, 1, weight_dtype="fp8")
    s.prefill(WR.prompt(1, 3))
    assert s.model is not model and s.weight_dtype == "fp8"
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert torch.equal(s.model.token_embeddings.weight, model.token_embeddings.weight)


def test_refusals(models):
    model, _ = models
    with pytest.raises(ValueError, match="weight_dtype"):
        DecodeSession(model, 1, weight_dtype="int4")
    p = WR.prompt(1, 3)
    with pytest.raises(ValueError, match="weight_dtype"):
        model.generate(p, 2, weight_dtype="int4")
    with pytest.raises(ValueError, match="not supported yet"):
        model.generate(p, 2, weight_dtype="fp8", draft_model=model)
