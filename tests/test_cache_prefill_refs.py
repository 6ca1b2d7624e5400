"""CPU side of the flash prefill over the KV cache: the op wrapper's oracle path, the session's chunk plan, chunked
prefill on the reference path, and -- with the rounding emulation of ``tests/cache_prefill_refs.py`` -- that every
input and bound of ``tests/test_cache_prefill_gpu.py`` is satisfiable by a kernel with the documented rounding
points (bf16 ``q * scale * log2 e``, bf16 ``P``, fp32 accumulation) before a GPU sees them.
"""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.models import generation as gen
from bpe_transformer.ops import decode as OD

from . import cache_prefill_refs as CR
from . import decode_refs as DR
from . import ragged_refs as RR
from .decode_refs import f64

DOMINANT = CR.DOMINANT


# ------------------------------------------------------------------ the op wrapper on the CPU
@pytest.mark.parametrize("T,p0", [(9, 0), (33, 65)])
def test_prefill_attention_cpu_shared_pos(T, p0):
    B, Hkv, G, D, Lmax = 2, 2, 2, 64, 128
    q = DR.queries(B, T, Hkv * G, D, seed=3).float()
    k, v = (t.float() for t in DR.caches(B, Hkv, Lmax, D, p0 + T, seed=3))
    ref, A = DR.decode_attention(f64(q), f64(k), f64(v), p0, Hkv * G, T)
    got = OD.prefill_attention(q, k, v, torch.tensor([p0], dtype=torch.int32), Hkv * G, n_new=T)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert bool(((f64(got) - ref).abs() <= CR.TOL32 * A).all())


def test_prefill_attention_cpu_per_sequence_pos():
    pos, T, Hkv, G, D, Lmax = [0, 5, 40], 12, 2, 3, 64, 64
    q, k, v, H = RR.attention_case(Hkv, G, D, Lmax, pos, T)
    ref, A = RR.decode_attention(q, k, v, pos, H, T)
    got = OD.prefill_attention(q.float(), k.float(), v.float(), torch.tensor(pos, dtype=torch.int32), H, n_new=T)
    assert bool(((f64(got) - ref).abs() <= CR.TOL32 * A).all())


# ------------------------------------------------------------------ the chunk plan
def test_plan_small_window_is_one_decode_step():
    for G in (1, 2, 4, 8):
        for T in range(1, 8 // G + 1):
            assert gen._append_plan(T, G, True) == [(0, T, "decode")]


def test_plan_large_window_is_one_cache_chunk():
    assert gen._append_plan(9, 1, True) == [(0, 9, "cache")]
    assert gen._append_plan(512, 1, True) == [(0, 512, "cache")]
    assert gen._append_plan(2, 8, True) == [(0, 2, "cache")]
    assert gen._append_plan(3, 4, True) == [(0, 3, "cache")]


@pytest.mark.parametrize("T,c", [(50, 16), (64, 16), (17, 16), (512, 128)])
def test_plan_prefill_chunk(T, c):
    plan = gen._append_plan(T, 1, True, c)
    assert len(plan) == math.ceil(T / c)
    assert [t0 for t0, _, _ in plan] == list(range(0, T, c)) and sum(w for _, w, _ in plan) == T
    assert all(w <= c for _, w, _ in plan)
    assert all(kind == ("cache" if w > 8 else "decode") for _, w, kind in plan)


def test_plan_empty_cache_starts_with_flash():
    assert gen._append_plan(40, 1, False) == [(0, 40, "flash")]
    assert gen._append_plan(50, 1, False, 16) == [(0, 16, "flash"), (16, 16, "cache"), (32, 16, "cache"),
                                                   (48, 2, "decode")]
    assert gen._append_plan(50, 8, False, 16)[-1] == (48, 2, "cache")
    assert gen._append_plan(1, 1, False) == [(0, 1, "decode")]  # a single token never took the flash path


# ------------------------------------------------------------------ chunked prefill on the reference path
def _model(**kw):
    torch.manual_seed(0)
    cfg = dict(vocab_size=97, context_length=48, d_model=64, num_layers=2, num_heads=4, d_ff=96)
    cfg.update(kw)
    return TransformerLM(**cfg).eval()


@pytest.mark.parametrize("ragged", [False, True])
def test_cpu_session_prefill_chunk_matches_whole_window(ragged):
    model = _model(num_kv_heads=2)
    ids = torch.randint(0, 97, (3, 23), generator=torch.Generator().manual_seed(1))
    lengths = [23, 7, 12] if ragged else None
    a = DecodeSession(model, 3, ragged=ragged)
    b = DecodeSession(model, 3, ragged=ragged, prefill_chunk=5)
    with torch.no_grad():
        la, lb = a.prefill(ids, lengths), b.prefill(ids, lengths)
        assert (la - lb).abs().max() < 1e-5
        assert a.cache._len == b.cache._len and torch.equal(a.cache.pos, b.cache.pos)
        for s, n in enumerate(lengths or [23] * 3):
            # fp32 on the CPU: the same rows through GEMMs of another height, equal to the last bits or nearly
            assert torch.allclose(a.cache.k[:, s, :, :n], b.cache.k[:, s, :, :n], rtol=0, atol=1e-6)
            assert torch.allclose(a.cache.v[:, s, :, :n], b.cache.v[:, s, :, :n], rtol=0, atol=1e-6)
        nxt = torch.randint(0, 97, (3,), generator=torch.Generator().manual_seed(2))
        assert (a.decode(nxt) - b.decode(nxt)).abs().max() < 1e-5


# ------------------------------------------------------------------ the GPU tests' inputs and bounds, emulated
@pytest.mark.parametrize("D", [64, 128])
def test_emulation_meets_bounds_lengths(D):
    for T, p0 in CR.LENGTHS:
        q, k, v, H, ref, A = CR.length_case(D, T, p0)
        assert torch.isfinite(k[:, :, :p0 + T]).all() and not torch.isfinite(k[:, :, p0 + T:]).any()
        assert not torch.isfinite(v[:, :, p0 + T:]).any()
        emu = CR.emulate(q, k, v, p0, H, T)
        assert CR.global_rel(emu, ref) < CR.TOL_GLOBAL, (T, p0, CR.global_rel(emu, ref))


def test_emulation_meets_bounds_not_a_tile_multiple():
    q, k, v, H, ref, A = CR.length_case(64, 64, 136, Lmax=200)
    assert CR.global_rel(CR.emulate(q, k, v, 136, H, 64), ref) < CR.TOL_GLOBAL


@pytest.mark.parametrize("G", CR.GROUPS)
def test_emulation_meets_bounds_groups(G):
    q, k, v, H, ref, A = CR.length_case(64, 40, 70, G=G)
    assert CR.global_rel(CR.emulate(q, k, v, 70, H, 40), ref) < CR.TOL_GLOBAL


def test_emulation_meets_bounds_ragged():
    q, k, v, H, ref, A = CR.ragged_case()
    assert RR.visible_is_finite(k, v, CR.RAGGED_POS, CR.RAGGED_T) and RR.poison_is_there(k, v, CR.RAGGED_POS, CR.RAGGED_T)
    assert CR.global_rel(CR.emulate(q, k, v, CR.RAGGED_POS, H, CR.RAGGED_T), ref) < CR.TOL_GLOBAL


def test_emulation_meets_bounds_full_cache():
    q, k, v, H, p0, n, ref, A = CR.full_case()
    B, T = k.shape[0], q.shape[0] // k.shape[0]
    emu = CR.emulate(q, k, v, p0, H, T).view(B, T, -1)[:, :n].reshape(B * n, -1)
    assert CR.global_rel(emu, ref) < CR.TOL_GLOBAL


@pytest.mark.parametrize("D,T,p0", DOMINANT)
def test_dominant_key_inputs_and_bound(D, T, p0):
    q, k, v, ref, A, rows = CR.dominant_case(D, T, p0, 0)
    # the key really dominates: the reference itself is V[p0 + t] to within 1e-4 (|V| ~ 1, one bf16 ulp ~ 8e-3)
    assert float((ref - rows).abs().max()) < 1e-4
    extra = CR.dominant_extra(q, k, v, p0, T)
    assert float(extra.max()) < 2.0 ** -10  # the derived bf16 term is small beside the ulp, as it must be here
    emu = f64(CR.emulate(q, k, v, p0, k.shape[1], T))
    assert bool(((emu - rows).abs() <= CR.dominant_bound(rows, ref, A, extra)).all())


@pytest.mark.parametrize("D,T,p0", DOMINANT)
def test_look_ahead_inputs_are_sharp(D, T, p0):
    q, k, v, ref, A, nxt = CR.dominant_case(D, T, p0, 1)
    assert torch.isfinite(k[:, :, :p0 + T]).all() and torch.isfinite(v[:, :, :p0 + T]).all()
    emu = CR.emulate(q, k, v, p0, k.shape[1], T)
    assert CR.global_rel(emu, ref) < CR.TOL_GLOBAL
    # a kernel that lets token t see key p0 + t + 1 returns that key's V row: far outside the tolerance
    have = ~torch.isnan(nxt)
    wrong = torch.where(have, nxt, ref)
    assert float((wrong - ref).abs().max() / ref.abs().max()) > 10 * CR.TOL_GLOBAL
