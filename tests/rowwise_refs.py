"""Plain float64 references and shared input builders for the row-wise kernels.

The HIP kernels in ``csrc/softmax.hip``, ``rope.hip``, ``embedding.hip``, ``activations.hip``,
``cross_entropy.hip`` and ``add_rmsnorm_fwd`` (``rmsnorm.hip``) compute in fp32 from inputs that are already
rounded to the test dtype.  Every function here takes those rounded inputs upcast to float64 (``f64``) and
returns the forward result or the gradient in float64, written as the textbook formula with no tricks.
``tests/test_rowwise_refs.py`` checks each against torch's own float64 op / autograd (CPU);
``tests/test_rowwise_kernels_gpu.py`` checks the kernels against them.

The builders make the inputs of the GPU tests (CPU tensors, fixed seed, rounded to the dtype), so the CPU tests
can guard their invariants: a ``-inf`` pattern never masks a whole row it was not meant to, a cross-entropy
target is never a ``-inf`` column.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

NEG_INF = float("-inf")
IGNORE = -100


def f64(t: Tensor) -> Tensor:
    return t.detach().to("cpu", torch.float64)


def vec_elems(dtype: torch.dtype) -> int:
    """Elements of one 16-byte vector."""
    return 8 if dtype == torch.bfloat16 else 4


# ------------------------------------------------------------------ softmax
def softmax(x: Tensor, dim: int = -1) -> Tensor:
    """exp(x - max) / sum: a ``-inf`` entry gives exactly 0, a row of only ``-inf`` gives NaN (-inf - -inf), which
    is what ``torch.softmax`` returns too."""
    e = torch.exp(x - x.amax(dim=dim, keepdim=True))
    return e / e.sum(dim=dim, keepdim=True)


def softmax_bwd(y: Tensor, dy: Tensor, dim: int = -1) -> Tensor:
    return y * (dy - (dy * y).sum(dim=dim, keepdim=True))


SOFTMAX_NS = (1, 5, 63, 64, 65, 255, 256, 257, 600, 1000, 4099)
SOFTMAX_MS = (1, 3, 37)
# name -> the row widths it is built at
SOFTMAX_INF_PATTERNS = {
    "col0": (600, 5),
    "first256": (600,),       # every thread's first element
    "wave2": (600,),          # exactly the columns owned by wave 2 of the 256-thread block
    "every_other": (600, 5),
    "all_but_last": (600, 5),
    "causal65": (65,),
}


def softmax_input(M: int, N: int, dtype: torch.dtype, seed: int = 0) -> Tensor:
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + N)
    return (2.0 * torch.randn(M, N, generator=g)).to(dtype)


def softmax_inf_mask(pattern: str, N: int, M: int = 3) -> Tensor:
    """Boolean [M, N], True = ``-inf``."""
    cols = torch.arange(N)
    if pattern == "col0":
        m = cols == 0
    elif pattern == "first256":
        m = cols < 256
    elif pattern == "wave2":
        m = (cols % 256) // 64 == 2
    elif pattern == "every_other":
        m = cols % 2 == 0
    elif pattern == "all_but_last":
        m = cols < N - 1
    elif pattern == "causal65":
        assert N == 65
        return ~torch.ones(N, N, dtype=torch.bool).tril()
    else:
        raise KeyError(pattern)
    return m.expand(M, N).clone()


def softmax_inf_input(pattern: str, N: int, dtype: torch.dtype) -> Tensor:
    mask = softmax_inf_mask(pattern, N)
    x = softmax_input(mask.shape[0], N, dtype, seed=3)
    return x.masked_fill(mask, NEG_INF)


def softmax_masked_row_input(N: int, dtype: torch.dtype) -> tuple[Tensor, int]:
    """Three rows, the middle one (the returned index) fully ``-inf``."""
    x = softmax_input(3, N, dtype, seed=4)
    x[1] = NEG_INF
    return x, 1


def softmax_spread_input(N: int, dtype: torch.dtype) -> Tensor:
    """Rows spanning 200: exp(x - max) underflows to exact zeros in fp32 for the low end."""
    x = torch.linspace(-200.0, 0.0, N).repeat(3, 1)
    x[1] = x[1].flip(0)
    x[2] = x[2][torch.randperm(N, generator=torch.Generator().manual_seed(5))]
    return x.to(dtype)


# ------------------------------------------------------------------ RoPE
def rope(x: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, inverse: bool = False) -> Tensor:
    """Interleaved pairs (x[2i], x[2i+1]) rotated by the table angle at ``pos`` (broadcast against
    ``x.shape[:-1]``); ``cos`` / ``sin`` are the fp32 tables upcast.  ``inverse`` rotates back (the backward)."""
    c = cos[pos]
    s = -sin[pos] if inverse else sin[pos]
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).flatten(-2)


ROPE_DS = (8, 16, 64, 96, 128, 256)
ROPE_MAX_SEQ = 64
ROPE_SHAPE = (2, 3, 37)  # B, H, S


def rope_positions(kind: str) -> Tensor | None:
    """``None`` (arange), ``[S]`` or ``[B, 1, S]`` positions, all inside the table; the explicit ones contain both
    0 and ``ROPE_MAX_SEQ - 1``."""
    B, _, S = ROPE_SHAPE
    g = torch.Generator().manual_seed(11)
    if kind == "none":
        return None
    if kind == "s":
        p = torch.randint(0, ROPE_MAX_SEQ, (S,), generator=g)
        p[3], p[S - 1] = 0, ROPE_MAX_SEQ - 1
        return p
    if kind == "b1s":
        p = torch.randint(0, ROPE_MAX_SEQ, (B, 1, S), generator=g)
        p[0, 0, 0], p[1, 0, 5] = ROPE_MAX_SEQ - 1, 0
        p[1, 0, S - 1], p[0, 0, 9] = ROPE_MAX_SEQ - 1, 0
        return p
    raise KeyError(kind)


# ------------------------------------------------------------------ embedding
def embedding(weight: Tensor, ids: Tensor) -> Tensor:
    return weight[ids]


def embedding_bwd(dout: Tensor, ids: Tensor, vocab: int) -> Tensor:
    D = dout.shape[-1]
    return torch.zeros(vocab, D, dtype=dout.dtype).index_add_(0, ids.reshape(-1), dout.reshape(-1, D))


EMBED_VOCAB = 311
# one width per embed_bwd_kernel<T, C> instantiation, C = 1, 2, 4, 8, 16, plus the narrowest legal row
EMBED_DS = {torch.bfloat16: (8, 520, 1032, 2056, 4104, 8192), torch.float32: (4, 260, 516, 1028, 2052, 4096)}
EMBED_ID_CASES = ("one", "seven", "all_equal", "all_distinct", "last_run")


def embedding_ids(case: str, vocab: int = EMBED_VOCAB) -> Tensor:
    g = torch.Generator().manual_seed(13)
    if case == "one":
        return torch.tensor([vocab - 1])
    if case == "seven":
        return torch.tensor([0, vocab - 1, 3, 3, 0, 5, vocab - 1])
    if case == "all_equal":
        return torch.full((301,), 17)
    if case == "all_distinct":
        return torch.randperm(vocab, generator=g)[:301]
    if case == "last_run":  # the largest id once: its run starts at the last sorted position
        ids = torch.randint(0, 20, (301,), generator=g)
        ids[0], ids[150] = 0, vocab - 1
        return ids
    raise KeyError(case)


# ------------------------------------------------------------------ activations
def silu(x: Tensor) -> Tensor:
    return x / (1.0 + torch.exp(-x))


def silu_bwd(x: Tensor, dy: Tensor) -> Tensor:
    s = 1.0 / (1.0 + torch.exp(-x))
    return dy * s * (1.0 + x * (1.0 - s))


_GELU_C = math.sqrt(2.0 / math.pi)


def gelu(x: Tensor) -> Tensor:
    return 0.5 * x * (1.0 + torch.tanh(_GELU_C * (x + 0.044715 * x ** 3)))


def gelu_bwd(x: Tensor, dy: Tensor) -> Tensor:
    t = torch.tanh(_GELU_C * (x + 0.044715 * x ** 3))
    return dy * (0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _GELU_C * (1.0 + 3 * 0.044715 * x * x))


def swiglu(gu: Tensor) -> Tensor:
    F = gu.shape[-1] // 2
    return silu(gu[..., :F]) * gu[..., F:]


def swiglu_bwd(gu: Tensor, dout: Tensor) -> Tensor:
    F = gu.shape[-1] // 2
    g, u = gu[..., :F], gu[..., F:]
    return torch.cat((silu_bwd(g, dout * u), dout * silu(g)), dim=-1)


ACT_EDGE_VALUES = (0.0, 1e-30, 1.0, 20.0, 88.0, 1e4)


def act_edge_input(dtype: torch.dtype) -> Tensor:
    """One row per magnitude (0 / -0, then +-v alternating), one 16-byte vector wide twice over, so that a
    per-row error bound is meaningful for the small magnitudes next to 1e4."""
    w = 2 * vec_elems(dtype)
    sign = torch.tensor([1.0, -1.0]).repeat(w // 2)
    return torch.stack([v * sign for v in ACT_EDGE_VALUES]).to(dtype)


def swiglu_edge_input(dtype: torch.dtype, flip: bool) -> Tensor:
    """[g | u] with g the edge rows and u the same rows (``flip``: mirrored, so g = +-v meets u = -+v).  In the
    1e-30 row u is +-1.5 instead: silu(1e-30) * 1e-30 = 5e-61 is below the smallest fp32 denormal, no kernel
    that computes in fp32 can return it."""
    g = act_edge_input(dtype)
    u = g.flip(1).clone() if flip else g.clone()
    amax = g.float().abs().amax(dim=1)
    tiny = (amax > 0) & (amax < 2.0 ** -63)
    u[tiny] = (1.5 * torch.sign(u[tiny].float())).to(dtype)
    return torch.cat((g, u), dim=1)


def act_input(shape: tuple[int, ...], dtype: torch.dtype, seed: int = 0, scale: float = 3.0) -> Tensor:
    g = torch.Generator().manual_seed(17 + seed)
    return (scale * torch.randn(*shape, generator=g)).to(dtype)


# ------------------------------------------------------------------ add + RMSNorm
def add_rmsnorm(x: Tensor, d: Tensor, w: Tensor, eps: float, dtype: torch.dtype) -> tuple[Tensor, Tensor, Tensor]:
    """``sum = round_dtype(x + d)`` (the stored residual stream), ``rstd`` and ``y`` from the ROUNDED sum.
    x + d of two fp32-representable values is exact in float64, so one rounding to ``dtype`` through fp32 equals
    the kernel's single rounding for bf16 and fp32 alike."""
    s = (x + d).to(torch.float32).to(dtype).to(torch.float64)
    rstd = torch.rsqrt((s * s).mean(dim=-1) + eps)
    return s, s * rstd.unsqueeze(-1) * w, rstd


ADD_RMS_NS = {torch.bfloat16: (8, 512, 520, 1024, 2048, 2056, 4096), torch.float32: (4, 768, 4100)}
ADD_RMS_MS = (1, 4, 7)


def add_rmsnorm_input(M: int, N: int, dtype: torch.dtype) -> tuple[Tensor, Tensor, Tensor]:
    g = torch.Generator().manual_seed(19 + M + N)
    x = torch.randn(M, N, generator=g).to(dtype)
    d = (0.5 * torch.randn(M, N, generator=g)).to(dtype)
    w = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype)
    return x, d, w


# ------------------------------------------------------------------ cross-entropy
def cross_entropy(logits: Tensor, targets: Tensor, ignore_index: int = IGNORE):
    """-> (mean loss over the non-ignored rows, per-row loss, per-row logsumexp, d mean-loss / d logits).
    ``-inf`` logits have probability and gradient exactly 0; ignored rows have loss and gradient 0; with no valid
    row the mean's denominator is 1 (loss 0)."""
    m = logits.amax(dim=-1, keepdim=True)
    e = torch.exp(logits - m)
    ssum = e.sum(dim=-1, keepdim=True)
    lse = (m + torch.log(ssum)).squeeze(-1)
    valid = targets != ignore_index
    t = torch.where(valid, targets, torch.zeros_like(targets))
    rows = torch.where(valid, lse - logits.gather(-1, t.unsqueeze(-1)).squeeze(-1), torch.zeros_like(lse))
    n = max(int(valid.sum()), 1)
    onehot = torch.zeros_like(logits).scatter_(-1, t.unsqueeze(-1), 1.0)
    grad = (e / ssum - onehot) * (valid.to(logits.dtype) / n).unsqueeze(-1)
    return rows.sum() / n, rows, lse, grad


CE_M = 6
CE_REG_ROWS = 512 * 16  # launch_ce_fwd_bwd: register kernel iff (V + vn) / vn <= 512 * MAXV


def ce_uses_register_kernel(V: int, dtype: torch.dtype) -> bool:
    vn = vec_elems(dtype)
    return (V + vn) // vn <= CE_REG_ROWS


def ce_boundary_vocabs(dtype: torch.dtype) -> tuple[int, int]:
    """The odd vocabularies nearest the register / two-pass switch on either side: (V + vn) // vn <= 8192 holds
    up to V = 8192 vn - 1, which is odd; the next odd size above is 8192 vn + 1."""
    vn = vec_elems(dtype)
    return CE_REG_ROWS * vn - 1, CE_REG_ROWS * vn + 1


def ce_row_split(r: int, V: int, dtype: torch.dtype, ld: int | None = None) -> tuple[int, int]:
    """(head, body_end) of row ``r`` of a 16-byte-aligned [M, V] buffer with row stride ``ld``: columns
    [0, head) are the unaligned scalar head, [head, body_end) whole 16-byte vectors, [body_end, V) the tail."""
    vn = vec_elems(dtype)
    head = min((-(r * (V if ld is None else ld))) % vn, V)
    return head, head + (V - head) // vn * vn


def ce_logits(V: int, dtype: torch.dtype, M: int = CE_M) -> Tensor:
    g = torch.Generator().manual_seed(23 + V)
    return (1.5 * torch.randn(M, V, generator=g)).to(dtype)


def ce_position_targets(V: int, dtype: torch.dtype) -> tuple[Tensor, dict[str, int]]:
    """Targets in the unaligned head, the vector body, the scalar tail and at V - 1 (rows 1-4, chosen by each
    row's own alignment), a body target in the aligned row 0, row 5 ignored.  -> (targets, {class: row})."""
    t = [0] * CE_M
    where: dict[str, int] = {}
    for r in range(1, 5):
        head, body_end = ce_row_split(r, V, dtype)
        if "head" not in where and head >= 1:
            where["head"], t[r] = r, head - 1
        elif "tail" not in where and V - body_end >= 2:
            where["tail"], t[r] = r, body_end
        elif "last" not in where:
            where["last"], t[r] = r, V - 1
        else:
            where["body"], t[r] = r, head + 5 * vec_elems(dtype) + 3
    t[0] = ce_row_split(0, V, dtype)[0] + 1234 * vec_elems(dtype) + 1
    t[5] = IGNORE
    return torch.tensor(t), where


CE_INF_PATTERNS = ("aligned_run16", "scattered5", "head")


def ce_inf_case(pattern: str, V: int, dtype: torch.dtype) -> tuple[Tensor, Tensor, Tensor]:
    """-> (logits with ``-inf`` columns, targets, mask).  Targets are finite body columns; row 5 is ignored."""
    x = ce_logits(V, dtype)
    mask = torch.zeros(CE_M, V, dtype=torch.bool)
    vn = vec_elems(dtype)
    for r in range(CE_M):
        head, _ = ce_row_split(r, V, dtype)
        if pattern == "aligned_run16":
            # whole 16-byte vectors of the row's body, in the SECOND sweep of the two-pass kernel's 256 threads:
            # a thread's first vector meets (m, s) = (-inf, 0), which online_merge leaves alone either way
            c0 = head + (256 + 16) * vn
            mask[r, c0:c0 + 16] = True
        elif pattern == "scattered5":   # never a whole vector
            mask[r, [1, 100, 1001, 20002, V - 3]] = True
        elif pattern == "head":
            mask[r, :head] = True
        else:
            raise KeyError(pattern)
    t = torch.tensor([30000 + 9 * r for r in range(CE_M)])
    t[5] = IGNORE
    return x.masked_fill(mask, NEG_INF), t, mask
