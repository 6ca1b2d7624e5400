"""CPU checks of ``tests/flash_refs.py``: the closed-form float64 reference against autograd and the fp32 oracle; the
emulation of the kernels' rounding points on every input of ``tests/test_flash_edges_gpu.py`` against every bound
and sharp identity asserted there (inputs and bounds are satisfiable, with the factor-2 margin, before a GPU sees
them); the builders' invariants; and negative tests -- the emulation broken the way a kernel could be, with the
check that must then fail."""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer import ops

from . import flash_refs as FR
from .decode_refs import BF16_ULP, f64


def _emu(case, form, **kw):
    fwd, bwd = FR.emu_form(case, form)
    cache = case.__dict__.setdefault("_emu", {})
    key = (fwd, bwd, tuple(sorted(kw.items())))
    if key not in cache:
        cache[key] = FR.emulate(case, fwd, bwd, **kw)
    return cache[key]


def _bits_zero(t: torch.Tensor) -> torch.Tensor:
    return (t.contiguous().view(torch.int16) & 0x7FFF) == 0


# ------------------------------------------------------------------ the reference
SAMPLE = [(65, 2, 2, 64, True, None, None), (129, 4, 2, 64, True, "pre", None), (136, 8, 1, 64, False, "pre", None),
          (64, 2, 2, 128, True, "fused", None), (257, 4, 2, 64, True, "pre", "d257"), (200, 3, 1, 64, True, None, "d200"),
          (17, 3, 1, 128, True, "pre", None)]


def _plain(case, dtype):
    """softmax(Q K^T) V with autograd in ``dtype`` -> (o, lse, dqkv) in the fused layout."""
    B, S, H, Hkv, D = case.B, case.S, case.H, case.Hkv, case.D
    x = case.qkv.to(dtype).requires_grad_(True)
    q, k, v = FR._split(x, B, S, H, Hkv, D)
    if case.rope is not None:
        q, k = FR._rot(q, case.cos.to(dtype), case.sin.to(dtype)), FR._rot(k, case.cos.to(dtype), case.sin.to(dtype))
    k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    s = q @ k.transpose(-1, -2) * case.scale
    s = s.masked_fill(~FR.visible(B, S, case.causal, case.doc_start)[:, None], float("-inf"))
    o = FR._rows(torch.softmax(s, -1) @ v)
    o.backward(case.dout.to(dtype))
    return o.detach(), torch.logsumexp(s.detach(), -1) * FR.LOG2E, x.grad


def _slices(case, g):
    q, kv = case.H * case.D, case.Hkv * case.D
    return {"dq": g[:, :q], "dk": g[:, q:q + kv], "dv": g[:, q + kv:]}


@pytest.mark.parametrize("args", SAMPLE, ids=str)
def test_reference_matches_float64_autograd(args):
    case = FR.random_case(*args)
    o, lse, g = _plain(case, torch.float64)
    got = {"o": o, "lse": lse, **_slices(case, g)}
    for n, t in got.items():
        e = float((t - case.ref[n]).abs().max() / case.ref[n].abs().max())
        assert e < 1e-10, (n, e)


@pytest.mark.parametrize("args", SAMPLE, ids=str)
def test_reference_matches_fp32_oracle(args):
    """``ops.attention_qkv_reference`` (fp32) and its autograd: within fp32 rounding (1e-5 of the largest value;
    sums of a few hundred terms)."""
    case = FR.random_case(*args)
    x = case.qkv.float().requires_grad_(True)
    o = ops.attention_qkv_reference(x, case.B, case.S, case.H, case.Hkv, case.D, case.cos, case.sin, case.causal,
                                    case.scale, doc_start=case.doc_start)
    o.backward(case.dout.float())
    for n, t in {"o": o.detach(), **_slices(case, x.grad)}.items():
        assert FR.global_rel(t, case.ref[n]) < 1e-5, n


def test_no_reference_row_is_empty():
    for _, case in FR.checked_inputs():
        assert torch.isfinite(case.ref["lse"]).all()
        assert bool((case.ref["P"].sum(-1) - 1).abs().max() < 1e-12)


# ------------------------------------------------------------------ the emulation on the GPU tests' inputs
def test_need_within_half_c():
    """``need <= C / 2`` for each output over every (input, form) pair; prints the measured maxima (``NEED``)."""
    need = {n: -math.inf for n in FR.C}
    for label, case in FR.checked_inputs():
        for form in FR.forms_for(case, public=True):
            for n, (_, v) in FR.measures(_emu(case, form), case.ref).items():
                need[n] = max(need[n], v)
                assert v <= FR.C[n] / 2, (label, form, n, v)
    print("\nneed:", {n: f"{v:.3g}" for n, v in need.items()}, " C:", FR.C)
    for n, v in need.items():  # the documented values are the measured ones
        assert abs(v - FR.NEED[n]) <= 0.01 * FR.NEED[n], (n, v, FR.NEED[n])
        assert FR.C[n] >= 2 * v and FR.C[n] <= 2 * v * 2, n  # 2 * need, one significant digit, rounded up


@pytest.mark.parametrize("args", FR.random_list(), ids=str)
def test_emulation_meets_old_global_bounds(args):
    case = FR.random_case(*args)
    for form in FR.forms_for(case):
        FR.check(_emu(case, form), case.ref, form, old=True)


def _dominant_ok(case, o) -> bool:
    rows, ref = case.rows, case.ref
    claim = ~torch.isnan(rows)
    bound = BF16_ULP * rows.abs() + (ref["o"] - rows).abs() + FR.C["o"] * ref["A_o"] + FR.FLOOR
    return bool(((f64(o) - rows).abs() <= bound)[claim].all())


@pytest.mark.parametrize("args", FR.dominant_list(), ids=str)
def test_dominant_under_emulation(args):
    case = FR.dominant_case(*args)
    for form in FR.forms_for(case):
        got = _emu(case, form)
        FR.check(got, case.ref, form)
        assert _dominant_ok(case, got["o"])
    if not case.causal or case.shift == 0:  # the dominant key really dominates
        P = case.ref["P"]
        top = P.amax(-1)
        assert bool((top[0] if not case.causal else top).min() > 1 - 2.0 ** -9)


@pytest.mark.parametrize("args", FR.staircase_list(), ids=str)
def test_staircase_under_emulation(args):
    case = FR.staircase_case(*args)
    # the scores are exact in bf16 operands and fp32 products, in both kernels' scalings
    q, qs, k, _, sc = FR._emu_operands(case)
    want = case.scores.float()[None, None, None, :].expand(case.B, case.H, case.S, case.S)
    assert torch.equal(qs @ k.transpose(-1, -2), want)
    assert torch.equal(q @ FR._bf(k * sc).transpose(-1, -2), want)
    assert torch.equal(FR._bf(want), want)
    for form in FR.forms_for(case):
        FR.check(_emu(case, form), case.ref, form)
    FR.check(FR.forward_tiled(case), case.ref, "tiled")  # the deferred rescale itself


@pytest.mark.parametrize("args", FR.zero_dout_list(), ids=str)
def test_zero_dout_under_emulation(args):
    case = FR.one_hot_dout(*args)
    assert case.zero_q.any() and case.zero_k.any() and not case.zero_k.all()
    for form in FR.forms_for(case):
        got = _emu(case, form)
        FR.check(got, case.ref, form)
        assert _bits_zero(got["dq"][case.zero_q]).all()
        assert _bits_zero(got["dk"][case.zero_k]).all() and _bits_zero(got["dv"][case.zero_k]).all()
        assert not _bits_zero(got["dv"][~case.zero_k]).all()


@pytest.mark.parametrize("args", FR.poison_list(), ids=str)
def test_poison_never_in_a_compared_row(args):
    bad, twin, keep = FR.poisoned_neighbour(*args)
    S = bad.S
    assert torch.isfinite(bad.qkv[keep].float()).all() and torch.isfinite(twin.qkv.float()).all()
    assert torch.equal(bad.qkv[keep], twin.qkv[keep]) and not keep[S:2 * S].any() and keep[:S].all() and keep[2 * S:].all()
    assert not torch.isfinite(bad.qkv[S:2 * S].float()).any() or args[4] == "big"
    if args[8]:
        base = bad.qkv._base
        assert bad.qkv.stride(0) % 8 == 0 and base.shape[1] == bad.qkv.shape[1] + args[8]
        assert torch.isnan(base[:, bad.qkv.shape[1]:].float()).all() and torch.isnan(twin.qkv._base[:, bad.qkv.shape[1]:].float()).all()
    for form in FR.forms_for(bad):  # sequences are independent under the emulation
        a, b = FR.emulate(bad, *FR.emu_form(bad, form)), FR.emulate(twin, *FR.emu_form(twin, form))
        for n in ("o", "dq", "dk", "dv"):
            assert torch.equal(a[n][keep].view(torch.int16), b[n][keep].view(torch.int16)), (form, n)
        assert torch.equal(a["lse"][[0, 2]], b["lse"][[0, 2]])


# ------------------------------------------------------------------ negative tests: a broken kernel is caught
def _fails(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("defect", ["causal+1", "doc-1", "lse", "alpha", "overread"])
def test_broken_emulation_is_caught(defect):
    """Each defect is caught by the named check of ``tests/test_flash_edges_gpu.py`` (and, where that can be
    asserted, invisible to the old ``rel < 2e-2 / 3e-2`` on the same inputs)."""
    if defect == "causal+1":  # -> test_dominant_and_lookahead (shift = 1)
        rnd = FR.random_case(257, 2, 2, 64, True, None, None)
        g = FR.measures(FR.emulate(rnd, defect=defect), rnd.ref)["o"][0]
        print(f"\nrandn, S 257: old global rel of O with the defect {g:.3e} (bound {FR.TOL_O:g}): a matter of luck")
        case = FR.dominant_case(257, 2, 64, 1, True, None)
        FR.check(FR.emulate(case), case.ref)
        assert _fails(lambda: FR.check(FR.emulate(case, defect=defect), case.ref))
    elif defect == "doc-1":  # -> test_zero_dout_rows_give_exact_zeros (doc)
        case = FR.one_hot_dout(257, 4, 2, 64, 0, "pre", "d257")
        good, bad = FR.emulate(case, "v2"), FR.emulate(case, "v2", defect=defect)
        assert _bits_zero(good["dk"][case.zero_k]).all() and _bits_zero(good["dv"][case.zero_k]).all()
        assert not _bits_zero(bad["dv"][case.zero_k]).all() and not _bits_zero(bad["dk"][case.zero_k]).all()
    elif defect == "lse":  # -> the LSE bound of every test (o and the gradients are those of the sound kernel)
        case = FR.random_case(200, 4, 2, 64, True, "pre", None)
        good, bad = FR.emulate(case), FR.emulate(case, defect=defect)
        assert all(torch.equal(good[n], bad[n]) for n in FR.NAMES)
        FR.check(good, case.ref, old=True)
        assert _fails(lambda: FR.check(bad, case.ref, old=True))
    elif defect == "alpha":  # -> test_staircase_rescale
        for args in [(9, True, False), (100, False, False), (0, False, True)]:
            case = FR.staircase_case(*args)
            FR.check(FR.forward_tiled(case), case.ref)
            assert _fails(lambda: FR.check(FR.forward_tiled(case, defect=defect), case.ref)), args
    else:  # overread -> test_dominant_and_lookahead (non-causal), test_neighbour_sequence_is_never_read
        case = FR.dominant_case(65, 2, 64, 0, False, None)
        assert _dominant_ok(case, FR.forward_tiled(case)["o"])
        assert not _dominant_ok(case, FR.forward_tiled(case, defect=defect)["o"])
        bad, twin, keep = FR.poisoned_neighbour(65, 2, 2, 64, "nan", False, None, None, 0)
        a, b = FR.forward_tiled(bad, defect=defect)["o"], FR.forward_tiled(twin, defect=defect)["o"]
        assert torch.equal(FR.forward_tiled(bad)["o"][keep].view(torch.int16), FR.forward_tiled(twin)["o"][keep].view(torch.int16))
        assert not torch.equal(a[keep].view(torch.int16), b[keep].view(torch.int16))
