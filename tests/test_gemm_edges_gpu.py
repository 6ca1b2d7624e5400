"""The bf16 GEMMs (``csrc/gemm.hip`` tiles 128 / 256, ``csrc/gemm_pp.hip``) and the ping-pong kernel's fused epilogues
(QKV + RoPE, SwiGLU forward / backward) against the float64 references of ``tests/gemm_refs.py``, where a GEMM can
go wrong without a random-operand ``rel < 1e-2`` test noticing: the single fp32 -> bf16 rounding, ``beta``, views of
wider buffers, non-finite values, the range ends, and the epilogues' geometry and edge values.

Inputs are built on the CPU with fixed seeds and copied to the GPU.  Bounds:

* the plain GEMMs are exact: integer operands make every partial sum exact in fp32 in any order, so every output bit
  equals ``round_bf16(beta * C + A B^T)`` computed in float64 (``tests/test_gemm_refs.py`` asserts, on these very
  inputs, that 39 % or more of the outputs need rounding, 20 % are ties and double rounding would change 15 %);
* the fused epilogues evaluate fp32 formulas on the bf16-rounded exact product, so each output must lie in the
  reference's accept set (``gemm_refs.Accept16``: a single bf16 value for all but ~0.03 % of the RoPE elements) and
  the SwiGLU ones must equal the unfused kernels bit for bit.  There is no mismatch budget.
"""

from __future__ import annotations

import contextlib
import math

import pytest
import torch

from . import fp8_refs as FR
from . import gemm_refs as GR
from .rowwise_refs import f64

pytestmark = pytest.mark.gpu

CDT = [torch.bfloat16, torch.float32]
MODES = {"tile": 0, "persist": 1, "persist3": 3}
SHAPES = {"g128": GR.G128_SHAPE, "g256": GR.G256_SHAPE, "pp": GR.PP_SHAPE}


@contextlib.contextmanager
def persist(mode: int):
    """gemm_pp kernel form: 0 one tile per workgroup, 1 persistent (one workgroup per CU), 3 persistent with three
    workgroups (two tiles each on the 2 x 3 tile shapes here)."""
    h = torch.ops.bpe_hip
    prev = h.gpp_persist_config(mode)
    try:
        yield
    finally:
        h.gpp_persist_config(prev)


@pytest.fixture(params=list(MODES.values()), ids=list(MODES))
def gpp_mode(request, gpu_device):
    with persist(request.param):
        yield request.param


def _lay(lay) -> str:
    return ("K" if lay[0] else "M") + ("K" if lay[1] else "M")


def _cases(one_mode: bool = False):
    """(kernel, layout pair, R, splits, persist mode) of every plain-GEMM case.  The persist mode only exists for
    gemm_pp; ``one_mode`` keeps the default form only."""
    out = []
    for R, s in GR.G128_CASES:
        out += [pytest.param("g128", lay, R, s, 1, id=f"g128-{_lay(lay)}-R{R}-s{s}") for lay in GR.LAYOUTS]
    for R, s in GR.G256_CASES:
        out.append(pytest.param("g256", (False, False), R, s, 1, id=f"g256-MM-R{R}-s{s}"))
    for R, s in GR.PP_CASES:
        for lay in GR.LAYOUTS:
            for name, mode in MODES.items():
                if one_mode and mode != 1:
                    continue
                out.append(pytest.param("pp", lay, R, s, mode, id=f"pp-{_lay(lay)}-R{R}-s{s}-{name}"))
    return out


def run_gemm(dev, kern, a, ak, b, bk, c, beta, splits):
    """One GEMM call on device tensors; c is written in place."""
    h = torch.ops.bpe_hip
    if kern == "pp":
        h.gemm_pp(a, ak, b, bk, c, beta, splits)
    else:
        h.gemm(a, ak, b, bk, c, beta, splits, 128 if kern == "g128" else 256)
    return c


def as_dtype(v64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> the C dtype with one rounding."""
    return GR.to_bf16(v64) if dtype == torch.bfloat16 else v64.to(torch.float32)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_bits(got: torch.Tensor, ref64: torch.Tensor, what: str, rows=None):
    """Every bit of ``got`` (CPU) equals the float64 reference rounded once to got's dtype."""
    ref = as_dtype(ref64, got.dtype)
    bad = bits(got) != bits(ref)
    if rows is not None:
        bad = bad & rows.unsqueeze(1)
    n = int(bad.sum())
    print(f"{what}: {n} of {bad.numel()} outputs differ")
    if n:
        idx = bad.nonzero()[:6]
        show = [(int(i), int(j), float(got[i, j]), float(ref[i, j]), float(ref64[i, j])) for i, j in idx]
        raise AssertionError((what, n, "row, col, got, ref, exact", show))


def dev_operands(dev, M, N, R, lay, seed=0):
    A, B = GR.int_operands(M, N, R, seed)
    return GR.store(A, lay[0]).to(dev), GR.store(B, lay[1]).to(dev)


# ------------------------------------------------------------------ A. exact accumulation, one rounding
@pytest.mark.parametrize("cdt", CDT, ids=["c16", "c32"])
@pytest.mark.parametrize("kern,lay,R,splits,mode", _cases())
def test_gemm_exact_rounding(gpu_device, kern, lay, R, splits, mode, cdt):
    """beta in {0, 1, -0.5, 2} over integer C: bitwise ``round_bf16(beta C + A B^T)`` (the fp32 sum for an fp32 C) --
    one rounding, round-to-nearest-even, whatever the tile schedule or split.  (Before the fix of the ping-pong
    kernel's one-pass epilogue, which added C to the already rounded product, exactly the ``pp`` cases with
    ``splits = 1``, a bf16 C and beta != 0 failed here, in 15 % of their outputs.)"""
    M, N = SHAPES[kern]
    a, b = dev_operands(gpu_device, M, N, R, lay)
    c0 = as_dtype(GR.int_c(M, N), cdt)
    with persist(mode):
        for beta in GR.BETAS:
            c = run_gemm(gpu_device, kern, a, lay[0], b, lay[1], c0.to(gpu_device, copy=True), beta, splits)
            assert_bits(c.cpu(), GR.gemm_ref(M, N, R, beta, cdt == torch.float32), f"beta={beta}")


# ------------------------------------------------------------------ B. beta = 0 never reads C
@pytest.mark.parametrize("cdt", CDT, ids=["c16", "c32"])
@pytest.mark.parametrize("kern,lay,R,splits,mode", _cases())
def test_gemm_beta0_over_poisoned_c(gpu_device, kern, lay, R, splits, mode, cdt):
    """C pre-filled with NaN (both signs, with payloads), +inf and -inf: beta = 0 must not read it (0 * NaN = NaN)."""
    M, N = SHAPES[kern]
    a, b = dev_operands(gpu_device, M, N, R, lay)
    with persist(mode):
        c = run_gemm(gpu_device, kern, a, lay[0], b, lay[1], GR.poison(M, N, cdt).to(gpu_device), 0.0, splits).cpu()
    assert not torch.isnan(c).any() and torch.isfinite(c).all()
    assert_bits(c, GR.gemm_ref(M, N, R, 0.0, cdt == torch.float32), "poisoned C")


# ------------------------------------------------------------------ C. views of wider buffers
VIEW_CASES = [("g128", (True, True), 192, 1), ("g128", (False, False), 192, 3), ("g128", (True, False), 64, 1),
              ("g128", (False, True), 448, 3), ("g256", (False, False), 96, 1), ("g256", (False, False), 288, 3)]
VIEW_CASES += [("pp", lay, R, s) for lay in GR.LAYOUTS for R, s in ((192, 1), (192, 3))]


@pytest.mark.parametrize("cdt", CDT, ids=["c16", "c32"])
@pytest.mark.parametrize("kern,lay,R,splits", VIEW_CASES, ids=[f"{k}-{_lay(l)}-R{r}-s{s}" for k, l, r, s in VIEW_CASES])
def test_gemm_views(gpu_device, kern, lay, R, splits, cdt):
    """A, B and C are column slices (offsets 8 / 16 / 8 elements, 24 columns of padding) of wider parents: outputs
    bitwise as in the contiguous case (beta = 1), every element of C's parent outside the view keeps its sentinel.
    The operands' parents hold NaN outside the views, so a read outside would show."""
    M, N = SHAPES[kern]
    A, B = GR.int_operands(M, N, R)
    sent = GR.SENTINEL16 if cdt == torch.bfloat16 else GR.SENTINEL32
    cp, _ = GR.widen(as_dtype(GR.int_c(M, N), cdt), 8, 24, sent)
    # the whole parents go to the device; the views are taken there
    av, bv = _view(gpu_device, GR.store(A, lay[0]), 8), _view(gpu_device, GR.store(B, lay[1]), 16)
    cpd = cp.to(gpu_device)
    cv = cpd[:, 8:8 + N]
    assert not av.is_contiguous() and not cv.is_contiguous() and av.stride(0) % 8 == 0 and cv.stride(0) % 8 == 0
    run_gemm(gpu_device, kern, av, lay[0], bv, lay[1], cv, 1.0, splits)
    out = cpd.cpu()
    assert_bits(out[:, 8:8 + N].contiguous(), GR.gemm_ref(M, N, R, 1.0, cdt == torch.float32), "view")
    outside = torch.ones(out.shape, dtype=torch.bool)
    outside[:, 8:8 + N] = False
    assert bool((bits(out)[outside] == bits(cp)[outside]).all()), "bytes outside C's view were written"


# ------------------------------------------------------------------ D. non-finite values and range
NF_CASES = [("g128", (True, True), 192, 1, 1), ("g128", (False, False), 192, 3, 1), ("g256", (False, False), 96, 1, 1),
            ("g256", (False, False), 288, 3, 1), ("pp", (True, True), 192, 1, 0), ("pp", (True, True), 192, 1, 1),
            ("pp", (False, False), 192, 1, 3), ("pp", (True, False), 192, 3, 1), ("pp", (False, True), 192, 3, 1)]
NF_IDS = [f"{k}-{_lay(l)}-R{r}-s{s}-m{m}" for k, l, r, s, m in NF_CASES]


@pytest.mark.parametrize("cdt", CDT, ids=["c16", "c32"])
@pytest.mark.parametrize("kern,lay,R,splits,mode", NF_CASES, ids=NF_IDS)
def test_gemm_nan_and_inf_rows(gpu_device, kern, lay, R, splits, mode, cdt):
    """One NaN in one row of A makes exactly that output row NaN; one +inf in a row of A against strictly positive B
    makes that row +inf.  Every other row keeps its exact bits (beta = 1)."""
    M, N = SHAPES[kern]
    A, B = GR.int_operands(M, N, R)
    C = GR.int_c(M, N)
    i0, k0 = 137, R - 3
    others = torch.arange(M) != i0
    with persist(mode):
        for val in (math.nan, math.inf):
            A2, B2 = A.clone(), (B if math.isnan(val) else B.abs() + 1.0)
            A2[i0, k0] = val
            a, b = GR.store(A2, lay[0]).to(gpu_device), GR.store(B2, lay[1]).to(gpu_device)
            c = run_gemm(gpu_device, kern, a, lay[0], b, lay[1], as_dtype(C, cdt).to(gpu_device), 1.0, splits).cpu()
            A2[i0, k0] = 0.0
            ref = C + A2 @ B2.t()
            assert_bits(c, ref if cdt == torch.float32 else FR.round_bf16(ref), f"rows beside the {val} row", others)
            row = c[i0].double()
            assert bool(torch.isnan(row).all() if math.isnan(val) else (row == math.inf).all()), (val, row[:8])


@pytest.mark.parametrize("cdt", CDT, ids=["c16", "c32"])
@pytest.mark.parametrize("kern,lay,R,splits,mode", NF_CASES, ids=NF_IDS)
def test_gemm_overflow_boundary(gpu_device, kern, lay, R, splits, mode, cdt):
    """Same-sign rows whose exact sums straddle the bf16 overflow boundary 255.5 * 2^120 (below fp32's): the largest
    sum that rounds down gives the last finite bf16, the tie and everything above +inf, the mirrored rows -inf; an
    fp32 C gets the exact finite sums."""
    M, N = SHAPES[kern]
    A, B, S = GR.overflow_operands(M, N, R)
    a, b = GR.store(A, lay[0]).to(gpu_device), GR.store(B, lay[1]).to(gpu_device)
    with persist(mode):
        c = run_gemm(gpu_device, kern, a, lay[0], b, lay[1], GR.poison(M, N, cdt).to(gpu_device), 0.0, splits).cpu()
    v = (S * 2.0 ** 114).unsqueeze(1).expand(M, N)
    assert_bits(c, v if cdt == torch.float32 else FR.round_bf16(v), "overflow boundary")
    if cdt == torch.bfloat16:
        col = c[:, N - 1].double()
        assert col[0] == GR.BF16_MAX and col[1] == -GR.BF16_MAX and col[2] == math.inf and col[3] == -math.inf


@pytest.mark.parametrize("kind", ["out", "in"])
@pytest.mark.parametrize("cdt", CDT, ids=["c16", "c32"])
@pytest.mark.parametrize("kern,lay,R,splits,mode", NF_CASES, ids=NF_IDS)
def test_gemm_subnormals(gpu_device, kern, lay, R, splits, mode, cdt, kind):
    """``out``: results (and every accumulator) below the fp32 normal range from normal bf16 inputs; ``in``:
    bf16-subnormal A entries with normal results.  The reference is IEEE, nothing flushed -- and that is what the
    MI355X does in all three kernels, one-pass and split: the bf16 MFMAs take subnormal inputs at their value and
    keep subnormal fp32 accumulators, the slab reduce and the fp32 -> bf16 conversion keep subnormal results (every
    case equal bit for bit when this test was written; no flush-to-zero form of the assertion was needed)."""
    M, N = SHAPES[kern]
    A, B = GR.subnormal_operands(M, N, R, kind)
    a, b = GR.store(A, lay[0]).to(gpu_device), GR.store(B, lay[1]).to(gpu_device)
    with persist(mode):
        c = run_gemm(gpu_device, kern, a, lay[0], b, lay[1], GR.poison(M, N, cdt).to(gpu_device), 0.0, splits).cpu()
    v = A @ B.t()
    flushed = float((c == 0).double().mean()), float((v == 0).double().mean())
    print(f"{kind}: zeros in the output {flushed[0]:.3f}, in the reference {flushed[1]:.3f}")
    assert_bits(c, v if cdt == torch.float32 else FR.round_bf16(v), f"subnormal {kind}")


# ------------------------------------------------------------------ E. RoPE epilogue geometry
@pytest.mark.parametrize("D", sorted(GR.ROPE_HEADS))
@pytest.mark.parametrize("S,M", GR.ROPE_SM)
def test_qkv_rope_geometry(gpu_device, gpp_mode, S, M, D):
    """Sequences shorter than a tile (S = 64), sequence boundaries inside tiles (S = 192), tables longer than S,
    head sizes 32 / 64 / 96 / 128 (D = 96: heads straddle tiles, rotation ends inside one).  Rotated outputs lie in
    the accept set of the fp64 rotation of the bf16-rounded exact product (table row ``m % S``); V columns are that
    product bit for bit."""
    H, Hkv = GR.ROPE_HEADS[D]
    N, rot_cols = (H + 2 * Hkv) * D, (H + Hkv) * D
    A, B = GR.int_operands(M, N, GR.ROPE_R, seed=2)
    P = FR.round_bf16(A @ B.t())
    cos, sin = GR.rope_tables(S, D)
    x, w = GR.store(A, True).to(gpu_device), GR.store(B, True).to(gpu_device)
    out = torch.ops.bpe_hip.gemm_qkv_rope(x, w, cos.to(gpu_device), sin.to(gpu_device), S, D, rot_cols).cpu()
    rot, acc = GR.rope_epilogue(P, cos, sin, S, D, rot_cols)
    ok = GR.in_accept16(out, acc)
    print(f"S={S} D={D}: {int((~ok).sum())} of {ok.numel()} outside the accept set")
    assert bool(ok.all()), [(int(i), int(j), float(out[i, j]), float(acc.lo[i, j]), float(acc.hi[i, j]))
                            for i, j in (~ok).nonzero()[:6]]
    assert_bits(out[:, rot_cols:].contiguous(), P[:, rot_cols:], "V columns")


# ------------------------------------------------------------------ F. SwiGLU epilogues at edge values
def same_bits_or_nan(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))


def test_swiglu_fwd_edge_values(gpu_device, gpp_mode):
    """gu planted exactly (one-hot power-of-two rows of x against the edge values in w13): gu bitwise, +-inf from
    overflow included; a in the accept set of ``rowwise_refs.swiglu`` wherever g and u are finite, and bitwise the
    unfused ``swiglu_fwd`` of the same gu everywhere.  The row-wise edge tests pin no class for non-finite g or u
    (their inputs are finite), so there the unfused kernel is the reference."""
    h = torch.ops.bpe_hip
    x, w13, gu_ref = GR.swiglu_fwd_inputs()
    F = GR.SWF_SHAPE[1]
    gu, a = h.gemm_swiglu_fwd(x.to(gpu_device), w13.to(gpu_device))
    a_unfused = h.swiglu_fwd(gu).cpu()
    gu, a = gu.cpu(), a.cpu()
    assert_bits(gu, gu_ref, "gu")
    finite = torch.isfinite(gu_ref[:, :F]) & torch.isfinite(gu_ref[:, F:])
    ok = GR.in_accept16(a, GR.swiglu_fwd_accept(gu_ref)) | ~finite
    print(f"a: {int((~ok).sum())} of {int(finite.sum())} finite-input elements outside the accept set")
    assert bool(ok.all()), [(float(gu_ref[i, j]), float(gu_ref[i, F + j]), float(a[i, j])) for i, j in (~ok).nonzero()[:6]]
    same = same_bits_or_nan(a, a_unfused)
    assert bool(same.all()), [(float(gu_ref[i, j]), float(gu_ref[i, F + j]), float(a[i, j]), float(a_unfused[i, j]))
                              for i, j in (~same).nonzero()[:6]]


def test_swiglu_bwd_edge_values(gpu_device, gpp_mode):
    """gu holds the edge pairs (both flips, subnormals, the largest finite g), dy and w2 are integers, so
    da = round_bf16(dy w2) exactly: dgu in the accept set of ``rowwise_refs.swiglu_bwd`` and bitwise the unfused
    ``swiglu_bwd`` of the same da and gu."""
    h = torch.ops.bpe_hip
    dy, w2, gu, da = GR.swiglu_bwd_inputs()
    gud = gu.to(gpu_device)
    dgu = h.gemm_swiglu_bwd(dy.to(gpu_device), w2.to(gpu_device), gud).cpu()
    unfused = h.swiglu_bwd(GR.to_bf16(da).to(gpu_device), gud).cpu()
    ok = GR.in_accept16(dgu, GR.swiglu_bwd_accept(f64(gu), da))
    print(f"dgu: {int((~ok).sum())} of {ok.numel()} outside the accept set")
    F = GR.SWB_SHAPE[1]
    assert bool(ok.all()), [(int(i), int(j), float(gu[i, j % F]), float(gu[i, F + j % F]), float(da[i, j % F]),
                             float(dgu[i, j])) for i, j in (~ok).nonzero()[:6]]
    same = same_bits_or_nan(dgu, unfused)
    assert bool(same.all()), [(int(i), int(j), float(dgu[i, j]), float(unfused[i, j])) for i, j in (~same).nonzero()[:6]]


# ------------------------------------------------------------------ C. (continued) strided inputs of the epilogue forms
def _view(dev, t: torch.Tensor, off: int) -> torch.Tensor:
    parent, _ = GR.widen(t, off, 24)
    return parent.to(dev)[:, off:off + t.shape[1]]


def test_epilogue_forms_on_views(gpu_device, gpp_mode):
    """The row-strided inputs the fused forms accept (x / w13, dy / w2, x / w of QKV + RoPE) as column slices of
    wider, NaN-padded parents: outputs bitwise those of the contiguous inputs."""
    h, dev = torch.ops.bpe_hip, gpu_device
    x, w13, _ = GR.swiglu_fwd_inputs()
    gu0, a0 = h.gemm_swiglu_fwd(x.to(dev), w13.to(dev))
    gu1, a1 = h.gemm_swiglu_fwd(_view(dev, x, 8), _view(dev, w13, 16))
    assert bool(same_bits_or_nan(gu0, gu1).all()) and bool(same_bits_or_nan(a0, a1).all())
    dy, w2, gu, _ = GR.swiglu_bwd_inputs()
    d0 = h.gemm_swiglu_bwd(dy.to(dev), w2.to(dev), gu.to(dev))
    d1 = h.gemm_swiglu_bwd(_view(dev, dy, 16), _view(dev, w2, 8), gu.to(dev))
    assert bool(same_bits_or_nan(d0, d1).all())
    S, M, D = 192, 768, 96
    H, Hkv = GR.ROPE_HEADS[D]
    N, rot_cols = (H + 2 * Hkv) * D, (H + Hkv) * D
    A, B = GR.int_operands(M, N, GR.ROPE_R, seed=2)
    cos, sin = (t.to(dev) for t in GR.rope_tables(S, D))
    xa, wb = GR.store(A, True), GR.store(B, True)
    q0 = h.gemm_qkv_rope(xa.to(dev), wb.to(dev), cos, sin, S, D, rot_cols)
    q1 = h.gemm_qkv_rope(_view(dev, xa, 8), _view(dev, wb, 24), cos, sin, S, D, rot_cols)
    assert torch.equal(bits(q0), bits(q1))
