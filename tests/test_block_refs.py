"""CPU checks of ``tests/block_refs.py``: the float64 block reference against an independently written float64
composition (``TransformerBlock.forward`` through ``_forward_reference``, its norms in float64), the emulation of the
fused block's rounding points on every spec of the GPU matrix against the recorded ``NEED`` (so ``C = 2 * NEED`` is
satisfiable before a GPU sees it), and the negative cases: the emulation broken the way the block could be must exceed
``C``."""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models.layers import RMSNorm, TransformerBlock

from . import block_refs as BR
from .decode_refs import f64

MEASURED: dict[str, float] = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nblock emulation, worst need per name (NEED recorded / C):")
        for n, v in MEASURED.items():
            print(f"  {n:8s} {v:.4f}  ({BR.NEED[n]:g} / {BR.C[n]:g})")


class _Norm64(torch.nn.Module):
    """RMSNorm without the module's fp32 statistics (``ops.rmsnorm`` computes in fp32 whatever the input dtype, which
    would cap the agreement at 1e-7)."""

    def __init__(self, d: int, eps: float):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(d, dtype=torch.float64))

    def forward(self, x):
        return x / torch.sqrt((x * x).sum(-1, keepdim=True) / x.shape[-1] + self.eps) * self.weight


def _block64(c, w, rope: bool) -> TransformerBlock:
    blk = TransformerBlock(c.d, c.H, c.F, c.S, BR.THETA, num_kv_heads=c.Hkv, remove_rope=not rope, eps=BR.EPS,
                           dtype=torch.float64)
    assert isinstance(blk.ln1, RMSNorm) and isinstance(blk.ln2, RMSNorm)
    blk.ln1, blk.ln2 = _Norm64(c.d, BR.EPS), _Norm64(c.d, BR.EPS)
    names = {"ln1": blk.ln1.weight, "wq": blk.attn.q_proj.weight, "wk": blk.attn.k_proj.weight,
             "wv": blk.attn.v_proj.weight, "wo": blk.attn.output_proj.weight, "ln2": blk.ln2.weight,
             "w1": blk.ffn.w1.weight, "w3": blk.ffn.w3.weight, "w2": blk.ffn.w2.weight}
    with torch.no_grad():
        for n, p in names.items():
            assert p.shape == w[n].shape, n
            p.copy_(f64(w[n]))
    blk.params = names
    return blk


def test_table_is_consistent():
    assert len({c.name for c in BR.CASES}) == len(BR.CASES) == 7
    for c in BR.CASES:
        assert c.d == c.H * c.D and c.H % c.Hkv == 0 and c.B * c.S <= 512
    for name, rows in BR.DOCS.items():
        c = BR.BY_NAME[name]
        assert len(rows) == c.B and all(sum(r) == c.S for r in rows)
        starts = {sum(r[:i]) for r in rows for i in range(1, len(r))}
        assert {32, 64} <= starts and any(s % 32 for s in starts) and any(1 in r for r in rows)
    for n, v in BR.NEED.items():
        assert BR.C[n] == pytest.approx(2 * v, rel=1e-12), n
    assert set(BR.C) == set(BR.NEED)
    g = BR.g0(5, 7)
    assert torch.equal(g.to(torch.bfloat16).float(), g) and bool((g != 0).all())


@pytest.mark.parametrize("spec", BR.matrix(), ids=lambda s: "-".join(str(v) for v in s))
def test_reference_matches_transformer_block(spec):
    """``block_ref64`` against ``TransformerBlock.forward`` in float64 on the CPU (the per-op composition with
    ``_forward_reference`` attention: doc mask and GQA included) and its autograd."""
    c, p, ref = BR.BY_NAME[spec.case], BR.inputs(spec), BR.block_ref64(spec)
    blk = _block64(c, p, spec.rope)
    xr = f64(p["xr"]).requires_grad_(True)
    xd = None if p["xd"] is None else f64(p["xd"]).requires_grad_(True)
    x = (xr if xd is None else xr + xd).view(c.B, c.S, c.d)
    doc = None if p["doc_start"] is None else (p["doc_start"], p["doc_end"])
    xm = x + blk.attn(blk.ln1(x), None, doc)
    g2 = blk.ffn(blk.ln2(xm))
    xm, g2 = xm.reshape(-1, c.d), g2.reshape(-1, c.d)
    torch.autograd.backward([xm, g2], [f64(p["dxm_out"]), f64(p["dg2"])])
    got = {"xm": xm.detach(), "g2": g2.detach(), "dxr": xr.grad, "dxd": None if xd is None else xd.grad}
    got.update({"d" + n: q.grad for n, q in blk.params.items()})
    for n in BR.NAMES:
        if ref[n] is None:
            assert got[n] is None
            continue
        e = float((got[n] - ref[n]).abs().max() / ref[n].abs().max())
        assert e < 1e-11, (n, e)
    # the block's own forward is the same composition
    y = blk(f64(p["xr"]).view(c.B, c.S, c.d) if xd is None else (f64(p["xr"]) + f64(p["xd"])).view(c.B, c.S, c.d),
            doc_bounds=doc)
    assert float((y.detach().reshape(-1, c.d) - (ref["xm"] + ref["g2"])).abs().max()) < 1e-11


def test_stack_reference_matches_transformer_blocks():
    c, p, ref = BR.BY_NAME[BR.STACK.case], BR.stack_inputs(), BR.stack_ref64()
    blks = [_block64(c, w, True) for w in p["layers"]]
    lnf = _Norm64(c.d, BR.EPS)
    with torch.no_grad():
        lnf.weight.copy_(f64(p["lnf"]))
    x0 = f64(p["xr"]).requires_grad_(True)
    x = x0.view(c.B, c.S, c.d)
    for b in blks:
        x = b(x)
    y = lnf(x).reshape(-1, c.d)
    y.backward(f64(p["dy"]))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    assert rel(y.detach(), ref["y"]) < 1e-11 and rel(x0.grad, ref["dx"]) < 1e-11
    assert rel(lnf.weight.grad, ref["dlnf"]) < 1e-11
    for b, r in zip(blks, ref["layers"]):
        for n, q in b.params.items():
            assert rel(q.grad, r["d" + n]) < 1e-11, n


def _note(ms):
    for n, v in ms.items():
        MEASURED[n] = max(MEASURED.get(n, -math.inf), v)


@pytest.mark.parametrize("spec", BR.matrix(), ids=lambda s: "-".join(str(v) for v in s))
def test_emulation_within_need(spec):
    """Every spec and gradient mode: the emulation stays within ``NEED`` as recorded (guards the table against edits
    to the inputs), hence within half of ``C``."""
    for mode in BR.MODES:
        ms = BR.measures(BR.emulate(spec, mode), spec, mode)
        _note(ms)
        for n, v in ms.items():
            assert v <= BR.NEED[n], (mode, n, v, BR.NEED[n])
        BR.check(ms, mode)
    got = BR.emulate(spec)
    if spec.xd:
        assert torch.equal(got["dxd"], got["dxr"])
    else:
        assert got["dxd"] is None


def test_stack_emulation_within_need():
    ms = BR.stack_measures(BR.emulate_stack())
    _note(ms)
    for n, v in ms.items():
        assert v <= BR.NEED[n], (n, v, BR.NEED[n])


def test_need_is_attained():
    """``NEED`` is the emulation's own worst case, not a number above it: some spec reaches 90 % of every entry."""
    worst: dict[str, float] = {}
    for spec in BR.matrix():
        for mode in BR.MODES:
            for n, v in BR.measures(BR.emulate(spec, mode), spec, mode).items():
                worst[n] = max(worst.get(n, -math.inf), v)
    worst.update(BR.stack_measures(BR.emulate_stack()))
    assert set(worst) == set(BR.NEED)
    for n, v in worst.items():
        assert 0.9 * BR.NEED[n] <= v <= BR.NEED[n], (n, v, BR.NEED[n])


# defect -> (spec, gradient modes, the outputs it must push past C)
NEGATIVE = {
    "gqa-mod": (BR.Spec("d128"), ("autograd",), ("xm", "g2", "dxr", "dwk", "dwv")),
    "no-resid-grad-1": (BR.Spec("fused64"), ("autograd",), ("dxr", "dxd")),
    "no-resid-grad-2": (BR.Spec("fallback"), ("autograd",), ("dxr", "dxd", "dwo", "dwq")),
    "dw-overwrite": (BR.Spec("fused64"), ("bf16", "fp32"), ("dwq", "dwk", "dwv", "dwo", "dw1", "dw3", "dw2")),
    "rope-k-missing": (BR.Spec("fallback"), ("autograd",), ("xm", "g2", "dxr", "dwq", "dwk")),
    "dxd-missing": (BR.Spec("fallback"), ("autograd",), ("dxd",)),
    "norm-dw-twice": (BR.Spec("d128"), ("bf16", "fp32"), ("dln1", "dln2")),
}


@pytest.mark.parametrize("defect", BR.DEFECTS)
def test_defects_exceed_c(defect):
    """The bound can fail: each defect exceeds ``C`` on the tensors it touches, and ``check`` raises."""
    spec, modes, names = NEGATIVE[defect]
    for mode in modes:
        ms = BR.measures(BR.emulate(spec, mode, defect=defect), spec, mode)
        for n in names:
            n = n + "32" if mode == "fp32" else n
            assert ms[n] > BR.C[n], (defect, mode, n, ms[n], BR.C[n])
        with pytest.raises(AssertionError):
            BR.check(ms, defect)


def test_gqa_defect_is_invisible_without_a_real_group():
    """``h % Hkv`` equals ``h // G`` at Hkv = 1 and at H = Hkv: only a case with 1 < Hkv < H can see the defect, which
    is why the matrix has ``d128`` / ``d128odd`` (4:2)."""
    for name in ("fallback", "fused64"):
        spec = BR.Spec(name)
        a, b = BR.emulate(spec), BR.emulate(spec, defect="gqa-mod")
        assert all(torch.equal(a[n], b[n]) for n in BR.NAMES)


def test_nan_fails_the_bound():
    spec = BR.Spec("short")
    got = dict(BR.emulate(spec))
    got["xm"] = got["xm"].clone()
    got["xm"][3, 5] = float("nan")
    assert BR.measures(got, spec)["xm"] == math.inf
