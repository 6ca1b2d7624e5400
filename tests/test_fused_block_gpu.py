"""The fused transformer block (``models/fused_block.py``: ``FusedBlockFn`` forward and backward, ``AddRMSNormFn``) on
the GPU against the float64 reference of ``tests/block_refs.py``: the smallest shapes that take each route (every case
first asserts the shape predicates it is meant to hit), the variants (no residual delta, no RoPE, document mask,
in-kernel RoPE, the fused-atomics attention backward with the forward-zeroed ``dq_acc``), the gradient-storage modes
(autograd / adjacent bf16 ``main_grad`` / separately allocated ``main_grad`` with column-sliced ``dy`` / fp32
``main_grad``; ``_NORM_DW_ACC`` on and off), every dW route of ``gemm._candidates`` pinned, and sharp bitwise checks.

Bound per element: ``|got - ref| <= 2^-7 |ref| + C[name] * A[name]`` (``block_refs``: ``C = 2 * NEED`` of the CPU
emulation; fp32 slots without the ulp term).  ``-s`` prints the measured need per case and output at module end.

MEASURED on an MI355X: the ``MEASURED`` table below (``_table`` prints it in this form).
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models import TransformerLM, fused_block
from bpe_transformer.models.layers import TransformerBlock
from bpe_transformer.ops import gemm
from bpe_transformer.ops._ext import ops as hip
from bpe_transformer.optim.flat import FlatParameters

from . import block_refs as BR

pytestmark = pytest.mark.gpu

# Worst ``(err - 2^-7 |ref|) / A`` x 100 per group of runs and output on an MI355X (fp32 slots, which have no ulp term,
# in their parameter's column), under the C rows.  Every run stayed within C; most within the emulation's NEED = C / 2.
# Above NEED, below C: the fp32 norm slots with ``_NORM_DW_ACC`` off (dln1 3.3 against NEED 2.6) -- ``rmsnorm_bwd``
# then returns dW rounded to bf16 and the caller adds that to the fp32 slot, a rounding point the emulation (fp32
# ``G0 + dW``) does not have; with the kernel adding in place the same slots need 2.6 - 2.8.  The four dW routes of a
# shape agree to the digits shown: the error is that of the bf16 operands they share.  Every sharp check held bit for bit.
MEASURED = """
need x 100                    xm    g2   dxr   dxd  dln1   dwq   dwk   dwv   dwo  dln2   dw1   dw3   dw2
C                           2.14  5.96  4.52  4.52  4.64  9.60  8.66  7.44  6.98  3.44  5.94  6.22  6.18
C, fp32 slots                  -     -     -     -  5.24 10.06  8.76  8.02  7.00  4.36  6.76  6.56  6.44
fused64-True-True-False     0.78  2.22  1.66  1.66  1.92  3.59  4.28  3.66  2.95  1.23  2.74  2.52  2.39
fallback-True-True-False    0.67  2.79  1.53  1.53  1.62  3.64  3.57  2.93  3.29  1.31  2.67  2.54  2.16
short-True-True-False       0.80  2.40  2.11  2.11  2.43  3.30  3.25  2.90  3.38  1.18  2.42  2.86  2.52
d128-True-True-False        1.06  2.34  1.61  1.61  2.26  3.67  3.89  3.30  3.50  1.42  2.71  2.65  2.65
d128odd-True-True-False     1.04  2.22  1.79  1.79  2.09  3.97  3.81  3.58  3.40  1.38  2.51  2.68  2.66
qkvoff-True-True-False      0.72  2.56  2.11  2.11  1.46  3.81  3.05  3.33  3.29  1.55  2.72  2.90  2.53
bwdoff-True-True-False      0.78  2.53  1.54  1.54  1.81  3.51  4.22  3.56  2.84  1.82  2.88  2.57  2.48
fused64-False-True-False    0.78  2.31  1.67     -  1.68  3.65  3.41  3.12  3.21  1.36  2.38  2.78  2.08
fused64-True-False-False    0.71  2.21  1.67  1.67  1.65  3.41  3.77  3.03  3.20  1.67  3.04  2.55  2.52
fused64-True-True-True      0.83  2.15  1.95  1.95  1.89  3.32  3.33  3.02  2.85  1.48  3.05  2.73  2.48
fallback-False-True-False   0.87  2.62  1.66     -  1.86  2.73  2.85  2.40  2.52  1.33  2.34  2.46  2.20
fallback-True-False-False   0.59  2.44  1.63  1.63  1.57  3.01  2.79  2.89  2.52  1.24  2.36  2.43  2.70
fallback-True-True-True     0.76  2.26  1.93  1.93  1.27  4.08  3.32  3.32  2.41  1.04  3.31  2.23  2.44
fused64/in-kernel-rope      0.78  2.89  1.67  1.67  2.28  3.91  3.62  3.17  2.52  1.55  2.52  2.91  2.38
d128odd/in-kernel-rope      1.04  2.50  2.00  2.00  2.09  4.25  3.65  3.23  3.13  1.61  3.18  2.76  2.59
fallback/fused-atomics      0.67  2.79  2.17  2.17  1.63  3.60  3.44  2.74  3.29  1.31  2.67  2.54  2.16
d128odd/fused-atomics       1.04  2.22  1.45  1.45  2.48  4.19  3.59  3.38  3.40  1.38  2.51  2.68  2.66
fused64/flat-bf16           0.78  2.22  1.66  1.66  2.04  4.04  3.90  3.79  3.11  1.23  2.70  2.62  2.63
fused64/split-bf16          0.78  2.22  1.66  1.66  2.04  4.04  3.90  3.79  3.11  1.23  2.70  2.62  2.63
fused64/flat-fp32           0.78  2.22  1.66  1.66  3.32  4.19  4.63  4.03  3.28  1.88  2.87  2.82  2.69
fused64/split-fp32          0.78  2.22  1.66  1.66  3.32  4.19  4.63  4.03  3.28  1.88  2.87  2.82  2.69
fallback/flat-bf16          0.67  2.79  1.53  1.53  1.61  3.71  3.50  3.03  2.57  1.19  2.68  2.47  2.49
fallback/split-bf16         0.67  2.79  1.53  1.53  1.61  3.71  3.50  3.03  2.57  1.19  2.68  2.47  2.49
fallback/flat-fp32          0.67  2.79  1.53  1.53  1.87  3.84  3.59  3.13  3.50  1.79  3.03  2.71  2.68
fallback/split-fp32         0.67  2.79  1.53  1.53  1.87  3.84  3.59  3.13  3.50  1.79  3.03  2.71  2.68
d128/flat-bf16              1.06  2.34  1.61  1.61  2.51  3.93  4.15  3.32  3.07  1.29  2.73  2.71  2.71
d128/split-bf16             1.06  2.34  1.61  1.61  2.51  3.93  4.15  3.32  3.07  1.29  2.73  2.71  2.71
d128/flat-fp32              1.06  2.34  1.61  1.61  3.12  4.06  4.89  3.69  3.98  2.20  3.46  3.14  2.97
d128/split-fp32             1.06  2.34  1.61  1.61  3.12  4.06  4.89  3.69  3.98  2.20  3.46  3.14  2.97
fused64/routes/flat-bf16    0.78  2.22  1.66  1.66  2.04  4.04  3.90  3.79  3.11  1.23  2.70  2.62  2.63
fused64/routes/flat-fp32    0.78  2.22  1.66  1.66  2.55  4.19  4.63  4.03  3.28  1.71  2.87  2.82  2.69
d128/routes/flat-bf16       1.06  2.34  1.61  1.61  2.29  3.93  4.15  3.32  3.07  1.29  2.73  2.71  2.71
d128/routes/flat-fp32       1.06  2.34  1.61  1.61  2.84  4.06  4.89  3.69  3.98  1.66  3.46  3.14  2.97
d128odd/routes/flat-bf16    1.04  2.22  1.79  1.79  2.03  4.13  3.80  3.48  3.20  1.40  2.55  2.73  2.59
d128odd/routes/flat-fp32    1.04  2.22  1.79  1.79  2.74  4.46  4.03  3.81  3.44  2.41  3.14  3.62  2.84
stack (need / C, x 100)    s_y 2.00 / 5.34  s_dx 3.07 / 6.10  s_dw 5.38 / 12.08  s_dln 2.64 / 4.88
"""

WORST: dict[str, dict[str, float]] = {}
PARAMS = {"ln1": "ln1.weight", "wq": "attn.q_proj.weight", "wk": "attn.k_proj.weight", "wv": "attn.v_proj.weight",
          "wo": "attn.output_proj.weight", "ln2": "ln2.weight", "w1": "ffn.w1.weight", "w3": "ffn.w3.weight",
          "w2": "ffn.w2.weight"}
# gradient storage: (a) autograd, (b) adjacent bf16 main_grad, (c) separately allocated main_grad, (d) fp32 main_grad
STORES = ("autograd", "flat-bf16", "split-bf16", "flat-fp32")
MODE_OF = {"autograd": "autograd", "flat-bf16": "bf16", "split-bf16": "bf16", "flat-fp32": "fp32", "split-fp32": "fp32"}


COLS = ("xm", "g2", "dxr", "dxd", "dln1", "dwq", "dwk", "dwv", "dwo", "dln2", "dw1", "dw3", "dw2")


def _table() -> str:
    """Worst need x 100 per group of runs and output (fp32 slots in their parameter's column), under the two C rows."""
    row = lambda label, vals: f"{label:26s} " + " ".join("    -" if v is None else f"{100 * v:5.2f}" for v in vals)  # noqa: E731
    lines = [f"{'need x 100':26s} " + " ".join(f"{n:>5s}" for n in COLS), row("C", [BR.C[n] for n in COLS]),
             row("C, fp32 slots", [BR.C.get(n + "32") for n in COLS])]
    for label, d in WORST.items():
        if label == "stack":
            lines.append("stack (need / C, x 100)    " + "  ".join(f"{n} {100 * v:.2f} / {100 * BR.C[n]:.2f}" for n, v in d.items()))
        else:
            lines.append(row(label, [d.get(n, d.get(n + "32")) for n in COLS]))
    return "\n".join(lines)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n" + _table())


@pytest.fixture(autouse=True)
def _routes():
    """dW routes chosen (timed) or pinned during a test do not outlive it."""
    saved = dict(gemm._route)
    yield
    gemm._route.clear()
    gemm._route.update(saved)


def _note(label: str, ms: dict[str, float]) -> None:
    d = WORST.setdefault(label, {})
    for n, v in ms.items():
        d[n] = max(d.get(n, -math.inf), v)


def _param(block, name: str):
    obj = block
    for part in PARAMS[name].split("."):
        obj = getattr(obj, part)
    return obj


def _load(block, w: dict) -> None:
    with torch.no_grad():
        for n in BR.WEIGHTS:
            p = _param(block, n)
            assert p.shape == w[n].shape and p.dtype == torch.bfloat16, n
            p.copy_(w[n])


def _block(dev, spec) -> TransformerBlock:
    c, p = BR.BY_NAME[spec.case], BR.inputs(spec)
    blk = TransformerBlock(c.d, c.H, c.F, c.S, BR.THETA, num_kv_heads=c.Hkv, remove_rope=not spec.rope, eps=BR.EPS,
                           device=dev, dtype=torch.bfloat16)
    _load(blk, p)
    if spec.rope:
        assert torch.equal(blk.attn.rope.cos.cpu(), p["cos"]) and torch.equal(blk.attn.rope.sin.cpu(), p["sin"])
    else:
        assert blk.attn.rope is None
    return blk


def _assert_routes(dev, c, prerotate: bool = True) -> None:
    """The shape predicates the case is in the matrix for (an edit to the routing rules must not turn it into a
    duplicate of another case)."""
    T, W = c.B * c.S, (c.H + 2 * c.Hkv) * c.D
    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.bfloat16)  # noqa: E731
    assert fused_block._fuse_qkv_rope(e(T, c.d), e(W, c.d), c.S) is c.qkv, c.name
    assert fused_block._fuse_swiglu_fwd(e(T, c.d), e(2 * c.F, c.d)) is c.fwd, c.name
    assert fused_block._fuse_swiglu_bwd(e(T, c.d), e(c.d, c.F), e(T, 2 * c.F)) is c.bwd, c.name
    tn = tuple(fused_block._dx_tn(w) for w in (e(W, c.d), e(c.d, c.H * c.D), e(2 * c.F, c.d), e(c.d, c.F)))
    assert tn == c.tn, (c.name, tn)
    assert fused_block.prerotate_default(c.D) is prerotate


def _attach(blk, store: str, counts: dict) -> None:
    """Gradient buffers of the main_grad modes, pre-filled with G0; a ready-callback counter on every parameter."""
    gdt = torch.float32 if store.endswith("fp32") else torch.bfloat16
    if store.startswith("flat"):
        flat = FlatParameters.from_module(blk, grad_dtype=gdt)
        order = [s.name for s in flat.slots]
        assert order == [PARAMS[n] for n in ("wq", "wk", "wv", "wo", "ln1", "ln2", "w1", "w3", "w2")], order
        for s in flat.slots:
            s.param.main_grad = flat.grad_view(s).view_as(s.param)
        assert fused_block._adjacent_view([_param(blk, n).main_grad for n in ("wq", "wk", "wv")]) is not None
        assert fused_block._adjacent_view([_param(blk, n).main_grad for n in ("w1", "w3")]) is not None
        blk._flat = flat
    else:
        for n in BR.WEIGHTS:
            p = _param(blk, n)
            p.main_grad = torch.empty(p.shape, device=p.device, dtype=gdt)
        assert fused_block._adjacent_view([_param(blk, n).main_grad for n in ("wq", "wk", "wv")]) is None
        assert fused_block._adjacent_view([_param(blk, n).main_grad for n in ("w1", "w3")]) is None
    for n in BR.WEIGHTS:
        p = _param(blk, n)
        p.grad = None
        p.main_grad.copy_(BR.g0(*p.shape))

        def ready(q, n=n):
            counts[n] = counts.get(n, 0) + 1

        p._bpe_grad_ready = ready


def _run(dev, spec, store: str = "autograd", xr_cpu=None, backward: bool = True) -> dict:
    """One forward (+ backward) of ``fused_block_pair`` on the case's block -> CPU outputs by ``block_refs`` name."""
    c, p = BR.BY_NAME[spec.case], BR.inputs(spec)
    blk = _block(dev, spec)
    counts: dict[str, int] = {}
    if store != "autograd":
        _attach(blk, store, counts)
    xr = (p["xr"] if xr_cpu is None else xr_cpu).to(dev).requires_grad_(True)
    xd = None if p["xd"] is None else p["xd"].to(dev).requires_grad_(True)
    doc = None if p["doc_start"] is None else (p["doc_start"].to(dev), p["doc_end"].to(dev))
    xm, g2 = fused_block.fused_block_pair(blk, xr, xd, c.B, c.S, doc)
    out = {"xm": xm.detach().cpu(), "g2": g2.detach().cpu()}
    if not backward:
        return out
    torch.autograd.backward([xm, g2], [p["dxm_out"].to(dev), p["dg2"].to(dev)])
    torch.cuda.synchronize()
    out["dxr"] = xr.grad.cpu()
    out["dxd"] = None if xd is None else xd.grad.cpu()
    for n in BR.WEIGHTS:
        q = _param(blk, n)
        if store == "autograd":
            assert q.grad is not None and q.grad.dtype == torch.bfloat16, n
            out["d" + n] = q.grad.cpu()
        else:
            assert q.grad is None, f"{n}: the function must return None with main_grad"
            out["d" + n] = q.main_grad.cpu()
    if store != "autograd":
        assert counts == {n: 1 for n in BR.WEIGHTS}, counts
    return out


def _check(label: str, got: dict, spec, store: str = "autograd", group: str | None = None) -> dict:
    """Print the run's needs, fold them into its group's row of the module-end table, assert the bound."""
    ms = BR.measures(got, spec, MODE_OF[store])
    _note(group or label, ms)
    print(f"\n  {label}: " + " ".join(f"{n} {v:.1e}" for n, v in ms.items()), end="")
    BR.check(ms, label)
    return got


def _same(a: dict, b: dict, names) -> None:
    for n in names:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
        else:
            assert a[n].dtype == b[n].dtype and torch.equal(a[n], b[n]), n


# ------------------------------------------------------------------ the shape matrix and the variants, autograd
@pytest.mark.parametrize("spec", BR.matrix(), ids=lambda s: "-".join(str(v) for v in s))
def test_matrix_against_float64(gpu_device, spec):
    """Every row of the shape matrix, and ``xd=None`` / no RoPE / document mask on ``fused64`` and ``fallback``."""
    _assert_routes(gpu_device, BR.BY_NAME[spec.case])
    got = _check("-".join(str(v) for v in spec), _run(gpu_device, spec), spec)
    if spec.xd:
        assert torch.equal(got["dxd"], got["dxr"])
    else:
        assert got["dxd"] is None


@pytest.mark.parametrize("name", ["fused64", "d128odd"])
def test_in_kernel_rope(gpu_device, monkeypatch, name):
    """``BPE_ROPE_PREROTATE=0``: Q / K stay unrotated in the QKV activation and the attention kernels rotate."""
    monkeypatch.setenv("BPE_ROPE_PREROTATE", "0")
    c = BR.BY_NAME[name]
    assert fused_block.prerotate_default(c.D) is False
    spec = BR.Spec(name)
    _check(f"{name}/in-kernel-rope", _run(gpu_device, spec), spec)


@pytest.mark.parametrize("name", ["fallback", "d128odd"])
def test_fused_atomics_backward_with_forward_zeroed_dq_acc(gpu_device, name):
    """``fa_bwd_config(1)``: the forward zeroes the backward's fp32 dQ accumulator (``B * ceil(S / 64) * 64`` rows:
    padded at S 100)."""
    c, spec = BR.BY_NAME[name], BR.Spec(name)
    prev = hip().fa_bwd_config(1)
    try:
        assert hip().fa_bwd_needs_dq_acc(c.D)
        _check(f"{name}/fused-atomics", _run(gpu_device, spec), spec)
    finally:
        hip().fa_bwd_config(prev)
    assert hip().fa_bwd_config(-1) == prev


def test_second_backward_through_dq_acc_raises(gpu_device):
    spec = BR.Spec("fallback")
    c, p = BR.BY_NAME[spec.case], BR.inputs(spec)
    blk = _block(gpu_device, spec)
    prev = hip().fa_bwd_config(1)
    try:
        xr = p["xr"].to(gpu_device).requires_grad_(True)
        xm, g2 = fused_block.fused_block_pair(blk, xr, p["xd"].to(gpu_device), c.B, c.S)
        loss = (xm.float() * p["dxm_out"].to(gpu_device).float()).sum() + (g2.float() * p["dg2"].to(gpu_device).float()).sum()
        loss.backward(retain_graph=True)
        with pytest.raises(RuntimeError, match="backward ran twice"):
            loss.backward()
    finally:
        hip().fa_bwd_config(prev)


# ------------------------------------------------------------------ gradient storage
@pytest.mark.parametrize("name", ["fused64", "fallback", "d128"])
def test_gradient_storage_modes(gpu_device, monkeypatch, name):
    """(a) autograd, (b) adjacent bf16 main_grad, (c) separately allocated main_grad (column-sliced ``dy``), (d) fp32
    main_grad -- each main_grad mode with the norm dW added by the kernel and by the caller: ``G0 + dW`` against
    float64, the ready callback once per parameter, None returned for the parameters; and the dX chain
    (``xm g2 dxr dxd``) bit-identical in every mode."""
    spec = BR.Spec(name)
    _assert_routes(gpu_device, BR.BY_NAME[name])
    base = _run(gpu_device, spec)
    assert torch.equal(base["dxd"], base["dxr"])
    for store in STORES[1:] + ("split-fp32",):
        for nacc in (True, False):
            monkeypatch.setattr(fused_block, "_NORM_DW_ACC", nacc)
            got = _check(f"{name}/{store}/nacc={int(nacc)}", _run(gpu_device, spec, store), spec, store,
                         group=f"{name}/{store}")
            _same(got, base, BR.ACTS)
    monkeypatch.setattr(fused_block, "_NORM_DW_ACC", True)


@pytest.mark.parametrize("store", ["autograd", "flat-fp32"])
@pytest.mark.parametrize("name", ["fused64", "fallback", "d128"])
def test_two_runs_are_bitwise_equal(gpu_device, name, store):
    spec = BR.Spec(name)
    a, b = _run(gpu_device, spec, store), _run(gpu_device, spec, store)
    _same(a, b, BR.NAMES)


@pytest.mark.parametrize("name", ["fallback", "fused64"])
def test_forward_rows_are_independent(gpu_device, name):
    """Other values in batch row 1 leave batch row 0's ``xm`` and ``g2`` rows bit for bit as they were."""
    spec = BR.Spec(name)
    c, p = BR.BY_NAME[name], BR.inputs(spec)
    xr = p["xr"].clone()
    xr[c.S:2 * c.S] = BR.randn(c.S, c.d, seed=(77,), scale=3.0)
    a, b = _run(gpu_device, spec, backward=False), _run(gpu_device, spec, xr_cpu=xr, backward=False)
    for n in ("xm", "g2"):
        assert torch.equal(a[n][:c.S], b[n][:c.S]), n
        assert not torch.equal(a[n][c.S:2 * c.S], b[n][c.S:2 * c.S]), n


# ------------------------------------------------------------------ every dW route, pinned
@pytest.mark.parametrize("store", ["flat-bf16", "flat-fp32"])
@pytest.mark.parametrize("name", ["fused64", "d128", "d128odd"])
def test_every_dw_route(gpu_device, monkeypatch, name, store):
    """``_tune`` picks by timing, so each candidate of each of the case's four dW shapes is pinned in turn (run i pins
    every shape to its i-th candidate, the last one once the list is exhausted) and checked against float64."""
    c, spec = BR.BY_NAME[name], BR.Spec(name)
    shapes = BR.dw_shapes(c)
    cands = [gemm._candidates(*s) for s in shapes]
    assert all(cs[-1] == "blas" for cs in cands) and any(len(cs) > 2 for cs in cands), cands
    seen = set()
    ran: list[tuple] = []
    real_run = gemm._run

    def recording_run(route, g, dy, x, x_scale=None):
        ran.append(((*g.shape, dy.shape[0]), route))
        real_run(route, g, dy, x, x_scale)

    monkeypatch.setattr(gemm, "_run", recording_run)
    for i in range(max(len(cs) for cs in cands)):
        pins = []
        ran.clear()
        for s, cs in zip(shapes, cands):
            r = cs[min(i, len(cs) - 1)]
            monkeypatch.setitem(gemm._route, s if store == "flat-bf16" else (*s, 32), r)
            pins.append(r)
            seen.add((s, r))
        _check(f"{name}/{store}/" + "+".join(pins), _run(gpu_device, spec, store), spec, store,
               group=f"{name}/routes/{store}")
        assert ran == [(shapes[j], pins[j]) for j in (3, 2, 1, 0)], ran  # W2, [W1;W3], Wo, [Wq;Wk;Wv]: each as pinned
    assert seen == {(s, r) for s, cs in zip(shapes, cands) for r in cs}


# ------------------------------------------------------------------ the stack: two blocks and AddRMSNormFn
def test_stack_against_float64(gpu_device):
    """``model.hidden_states`` on two fused blocks and the final ``AddRMSNormFn`` (its ``dx`` reaches both the
    residual and the delta of the last block); the embedding rows are the block-0 input, so their gradient is ``dx``."""
    c, p = BR.BY_NAME[BR.STACK.case], BR.stack_inputs()
    T = c.B * c.S
    model = TransformerLM(T, c.S, c.d, 2, c.H, c.F, BR.THETA, num_kv_heads=c.Hkv, eps=BR.EPS, device=gpu_device,
                          dtype=torch.bfloat16)
    for blk, w in zip(model.layers, p["layers"]):
        _load(blk, w)
    with torch.no_grad():
        model.token_embeddings.weight.copy_(p["xr"])
        model.ln_final.weight.copy_(p["lnf"])
    ids = torch.arange(T, device=gpu_device).view(c.B, c.S)
    assert all(layer._fused_ok(model.token_embeddings(ids)) for layer in model.layers)
    y = model.hidden_states(ids)
    y.backward(p["dy"].to(gpu_device).view(c.B, c.S, c.d))
    got = {"y": y.detach().reshape(T, c.d).cpu(), "dx": model.token_embeddings.weight.grad.cpu(),
           "dlnf": model.ln_final.weight.grad.cpu(),
           "layers": [{"d" + n: _param(blk, n).grad.cpu() for n in BR.WEIGHTS} for blk in model.layers]}
    ms = BR.stack_measures(got)
    _note("stack", ms)
    print("\n  stack: " + " ".join(f"{n} {v:.1e}" for n, v in ms.items()), end="")
    BR.check(ms, "stack")
