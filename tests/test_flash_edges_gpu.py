"""The training flash-attention kernels at their edges, against float64 (``tests/flash_refs.py``): every forward and
backward form the run-time selectors reach (v8 / v2 forward, split backward with the 32-row and both 16-row dQ
kernels, fused RoPE, D 128, fused atomics, GQA sweep, DOC, and ``ops.flash_attention_qkv`` with autograd).

Asserted per element: ``|got - ref| <= 2^-7 |ref| + C[name] A[name]`` for O, dQ, dK, dV and
``|lse - ref| <= C["lse"] A_lse`` (``C`` = twice what an emulation of the kernels' rounding points needs on these
same inputs, ``tests/test_flash_refs.py``), beside the old ``max|err| / max|ref| < 2e-2 / 3e-2`` on the random inputs.
Sharp checks without a tolerance: dominant key and look-ahead trap, exact zeros for zero-``dout`` rows, a poisoned
neighbour sequence that is never read, batch independence.  NaN anywhere counts as failure.

MEASURED on an MI355X (``-s`` prints them; also docs/performance.md, attention): the ``MEASURED`` table below.
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import pytest
import torch

from bpe_transformer import ops
from bpe_transformer.ops._ext import ops as hip

from . import flash_refs as FR
from .decode_refs import BF16_ULP, f64
from .test_doc_mask_gpu import bounds_from_lengths

pytestmark = pytest.mark.gpu

# Worst values per form over the module on an MI355X: ``max|err| / max|ref|`` over the random inputs (lse: largest
# absolute error, log2 units, all inputs) / worst element ``(err - 2^-7 |ref|) / A`` over all inputs (lse: err /
# A_lse), against C = o 0.07, dq 0.8, dk 0.2, dv 0.1, lse 0.6.  The worst elements are those of the CPU emulation
# (NEED in tests/flash_refs.py: the look-ahead inputs, and dq of the S 17, D 128 case): they come from the rounding of
# the operands, which the kernels and the emulation share.  Random inputs alone stay below 7e-3 (o), 2.2e-2 (dq),
# 1.3e-2 (dk), 6e-3 (dv).  Every sharp check (exact zeros, poisoned neighbour, batch independence) held bit for bit.
MEASURED = """
form               o              dq             dk             dv             lse
v8+split32         7.6e-3/3.1e-2  8.0e-3/1.6e-1  6.8e-3/5.8e-2  7.8e-3/4.9e-2  6.9e-2/2.8e-1
v8+dq16nw8         7.6e-3/3.1e-2  8.0e-3/1.6e-1  6.8e-3/5.8e-2  7.8e-3/4.9e-2  6.9e-2/2.8e-1
v8+dq16nw4         7.6e-3/3.1e-2  8.0e-3/1.6e-1  6.8e-3/5.8e-2  7.8e-3/4.9e-2  6.9e-2/2.8e-1
v2+split32         7.6e-3/3.1e-2  8.0e-3/1.4e-1  6.4e-3/5.8e-2  5.6e-3/4.9e-2  6.9e-2/2.8e-1
v8+fused           7.6e-3/3.1e-2  8.3e-3/1.6e-1  1.0e-2/5.8e-2  8.1e-3/4.9e-2  6.9e-2/2.8e-1
v2rope+splitrope   4.5e-3/5.6e-3  5.6e-3/2.2e-2  1.1e-2/1.1e-2  6.2e-3/5.2e-3  9.7e-3/2.1e-1
d128+split         5.5e-3/6.8e-3  1.1e-2/4.0e-1  7.0e-3/3.8e-2  4.5e-3/6.0e-3  1.1e-2/2.2e-1
d128+fused         2.3e-3/4.0e-3  5.2e-3/9.4e-3  5.0e-3/1.1e-2  4.6e-3/6.0e-3  7.2e-3/1.5e-1
doc                3.5e-3/6.9e-3  6.2e-3/1.4e-2  6.3e-3/1.3e-2  5.0e-3/5.5e-3  1.1e-2/2.8e-1
public             3.6e-3/6.9e-3  6.2e-3/1.8e-2  6.3e-3/1.3e-2  5.0e-3/5.5e-3  -
"""

WORST: dict[str, dict[str, list[float]]] = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nflash edges, worst per form: output global-rel / need (C " + ", ".join(f"{n} {v:g}" for n, v in FR.C.items()) + ")")
    for form, d in WORST.items():
        print(f"  {form:18s} " + "  ".join(f"{n} {g:.2e}/{v:.2e}" for n, (g, v) in d.items()))


def _note(form, ms, randomlike):
    d = WORST.setdefault(form, {})
    for n, (g, v) in ms.items():
        w = d.setdefault(n, [0.0, -math.inf])
        if randomlike or n == "lse":
            w[0] = max(w[0], g)
        w[1] = max(w[1], v)


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _to_dev(t: torch.Tensor, dev) -> torch.Tensor:
    """A column slice of a wider buffer keeps its row stride on the device."""
    if t.is_contiguous():
        return t.to(dev)
    return t._base.to(dev)[:, :t.shape[1]]


def _run(dev, case, form) -> dict[str, torch.Tensor]:
    """One forward + backward of ``case`` on the kernels ``form`` selects -> CPU o, lse (not ``public``), dq, dk, dv."""
    h = hip()
    B, S, H, Hkv, D = case.B, case.S, case.H, case.Hkv, case.D
    x, do = _to_dev(case.qkv, dev), case.dout.to(dev)
    use_rope, pre = case.rope is not None, case.rope == "pre"
    cos = case.cos.to(dev) if use_rope else torch.empty(0, 0, device=dev)
    sin = case.sin.to(dev) if use_rope else torch.empty(0, 0, device=dev)
    doc = None if case.doc is None else bounds_from_lengths([list(r) for r in case.doc_rows], dev)
    lse = None
    if form == "public":
        x = x.detach().requires_grad_(True)
        o = ops.flash_attention_qkv(x, B, S, H, Hkv, D, cos if use_rope else None, sin if use_rope else None,
                                    case.causal, scale=case.scale, prerotate=pre, doc_bounds=doc)
        o.backward(do)
        g = x.grad
    else:
        fwd_v, bwd_m, dq_f = FR.FORMS[form][:3]
        prev = h.fa_fwd_config(fwd_v), h.fa_bwd_config(bwd_m), h.fa_dq_config(dq_f)
        try:
            if pre:
                x = x.clone() if x.is_contiguous() else x._base.clone()[:, :x.shape[1]]  # (keeps the row stride)
                h.rope_qk_(x, cos, sin, B, S, H, Hkv, D)
            q, k, v = x[:, :H * D], x[:, H * D:(H + Hkv) * D], x[:, (H + Hkv) * D:]
            if doc is not None:
                o, lse = h.fa_fwd_doc(q, k, v, doc[0], doc[1], B, S, H, Hkv, D, True, use_rope, case.scale)
                g = h.fa_bwd_doc(do, q, k, v, o, lse, cos, sin, doc[0], doc[1], B, S, H, Hkv, D, True, use_rope,
                                 case.scale)
            else:
                o, lse = h.fa_fwd(q, k, v, cos, sin, B, S, H, Hkv, D, case.causal, use_rope, case.scale, pre)
                g = h.fa_bwd(do, q, k, v, o, lse, cos, sin, B, S, H, Hkv, D, case.causal, use_rope, case.scale, pre)
            torch.cuda.synchronize()
        finally:
            h.fa_fwd_config(prev[0]), h.fa_bwd_config(prev[1]), h.fa_dq_config(prev[2])
    g = g.cpu()
    out = {"o": o.detach().cpu(), "dq": g[:, :H * D], "dk": g[:, H * D:(H + Hkv) * D], "dv": g[:, (H + Hkv) * D:]}
    if lse is not None:
        assert lse.shape == (B, H, S) and lse.dtype == torch.float32
        out["lse"] = lse.cpu()
    return out


def _check(dev, case, form, old=False):
    got = _run(dev, case, form)
    ms = FR.measures(got, case.ref)
    _note(form, ms, old)
    print(f"\n  {form}: " + "  ".join(f"{n} {g:.2e}/{v:.2e}" for n, (g, v) in ms.items()), end="")
    FR.check(got, case.ref, form, old=old)
    return got


# ------------------------------------------------------------------ against float64
@pytest.mark.parametrize("i,args", list(enumerate(FR.random_list())), ids=str)
def test_random_vs_fp64(gpu_device, i, args):
    case = FR.random_case(*args)
    for form in FR.forms_for(case, public=i % 4 == 0 or case.doc is not None):
        _check(gpu_device, case, form, old=True)


def test_odd_gqa_group_is_accepted(gpu_device):
    """(H, Hkv) = (3, 1): the split dK/dV kernel sweeps an odd group (in ``random_list``); the fused form sums
    per-query-head partials and takes it too."""
    case = FR.random_case(129, 3, 1, 64, True, "pre", None)
    assert "v8+fused" in FR.forms_for(case)
    _check(gpu_device, case, "v8+fused", old=True)


@pytest.mark.parametrize("args", FR.dominant_list(), ids=str)
def test_dominant_and_lookahead(gpu_device, args):
    case = FR.dominant_case(*args)
    rows, ref = case.rows, case.ref
    claim = ~torch.isnan(rows)
    bound = BF16_ULP * rows.abs() + (ref["o"] - rows).abs() + FR.C["o"] * ref["A_o"] + FR.FLOOR
    for form in FR.forms_for(case):
        got = _check(gpu_device, case, form)  # shift = 1: the reference holds no v[i + 1]
        bad = ~((f64(got["o"]) - rows).abs() <= bound) & claim  # NaN counts as bad
        assert not bad.any(), (form, int(bad.sum()))


@pytest.mark.parametrize("args", FR.staircase_list(), ids=str)
def test_staircase_rescale(gpu_device, args):
    case = FR.staircase_case(*args)
    for form in FR.forms_for(case):  # v8 and, for comparison, v2; every D = 64 backward
        _check(gpu_device, case, form)


def _zero(t: torch.Tensor) -> torch.Tensor:
    """Exactly zero, either sign (the inverse rotation of a zero pair by negative cos and sin gives -0)."""
    return (_bits(t) & 0x7FFF) == 0


@pytest.mark.parametrize("args", FR.zero_dout_list(), ids=str)
def test_zero_dout_rows_give_exact_zeros(gpu_device, args):
    case = FR.one_hot_dout(*args)
    for form in FR.forms_for(case):
        got = _check(gpu_device, case, form)
        assert _zero(got["dq"][case.zero_q]).all(), form
        assert _zero(got["dk"][case.zero_k]).all() and _zero(got["dv"][case.zero_k]).all(), form


def _same(a: dict, b: dict, keep, seqs, form):
    for n in ("o", "dq", "dk", "dv"):
        x, y = a[n][keep], b[n][keep]
        assert torch.isfinite(x.float()).all(), (form, n)
        if n == "dq" and "fused" in form:  # fp32 atomics: the order varies (test_flash_dq_acc_zeroed_by_forward)
            assert float((x.float() - y.float()).abs().max() / y.float().abs().max()) < 1e-3, (form, n)
        else:
            assert torch.equal(_bits(x), _bits(y)), (form, n)
    if "lse" in a:
        assert torch.isfinite(a["lse"][seqs]).all() and torch.equal(_bits(a["lse"][seqs]), _bits(b["lse"][seqs])), form


@pytest.mark.parametrize("args", FR.poison_list(), ids=str)
def test_neighbour_sequence_is_never_read(gpu_device, args):
    bad, twin, keep = FR.poisoned_neighbour(*args)
    for form in FR.forms_for(bad, public=True):
        _same(_run(gpu_device, bad, form), _run(gpu_device, twin, form), keep, [0, 2], form)


@pytest.mark.parametrize("i,args", list(enumerate(FR.tiny_list())), ids=str)
def test_tiny_sequences(gpu_device, i, args):
    case = FR.random_case(*args)
    for form in FR.forms_for(case, public=i % 4 == 0):
        _check(gpu_device, case, form)


@pytest.mark.parametrize("args", [(200, 4, 2, 64, True, "pre", None), (129, 2, 2, 64, False, None, None),
                                  (65, 2, 2, 64, True, "fused", None), (136, 8, 1, 128, True, "fused", None),
                                  (200, 4, 2, 128, True, "pre", None)], ids=str)
def test_batch_and_head_independence(gpu_device, args):
    """B = 2 equals two B = 1 runs bit for bit (the fused-atomics dQ: ``rel < 1e-3``)."""
    case = FR.random_case(*args)
    S = case.S
    for form in FR.forms_for(case):
        both = _run(gpu_device, case, form)
        for b in range(case.B):
            one = SimpleNamespace(**{**case.__dict__, "B": 1, "qkv": case.qkv[b * S:(b + 1) * S],
                                     "dout": case.dout[b * S:(b + 1) * S]})
            got = _run(gpu_device, one, form)
            part = {n: (t[b:b + 1] if n == "lse" else t[b * S:(b + 1) * S]) for n, t in both.items()}
            _same(part, got, slice(None), [0], form)
