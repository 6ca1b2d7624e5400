"""Document-masked attention on the CPU: the bounds, the fp32 oracle, the model and the trainer plumbing."""

from __future__ import annotations

import pytest
import torch

from bpe_transformer import ops
from bpe_transformer.models import TransformerLM, get_preset
from bpe_transformer.ops import reference as R
from bpe_transformer.train.config import TrainConfig, apply_overrides
from bpe_transformer.train.trainer import Trainer
from bpe_transformer.utils.checkpoint import read_checkpoint

E = 9  # the separator id of the hand-written rows


def test_doc_bounds_hand_written_rows():
    rows = {
        "no separator": ([1, 2, 3, 4, 5], [0, 0, 0, 0, 0], [5, 5, 5, 5, 5]),
        "separator first": ([E, 1, 2, 3, 4], [0, 1, 1, 1, 1], [1, 5, 5, 5, 5]),
        "separator last": ([1, 2, 3, 4, E], [0, 0, 0, 0, 0], [5, 5, 5, 5, 5]),
        "adjacent separators": ([1, E, E, 2, 3], [0, 0, 2, 3, 3], [2, 2, 3, 5, 5]),
        "two documents": ([1, 2, E, 3, 4], [0, 0, 0, 3, 3], [3, 3, 3, 5, 5]),
    }
    for name, (ids, start, end) in rows.items():
        s, e = ops.doc_bounds(torch.tensor([ids]), E)
        assert s.tolist() == [start] and e.tolist() == [end], name
    # a different layout in every batch row, all at once
    ids = torch.tensor([r[0] for r in rows.values()])
    s, e = ops.doc_bounds(ids, E)
    assert s.tolist() == [r[1] for r in rows.values()]
    assert e.tolist() == [r[2] for r in rows.values()]
    for t in (s, e):
        assert t.dtype == torch.int32 and t.shape == ids.shape and t.is_contiguous() and t.device == ids.device
        assert bool((t[:, 1:] >= t[:, :-1]).all())  # non-decreasing along a row
    with pytest.raises(ValueError):
        ops.doc_bounds(torch.tensor([1, 2, 3]), E)


def _bounds_from_lengths(rows: list[list[int]]) -> tuple[torch.Tensor, torch.Tensor]:
    S = sum(rows[0])
    start = torch.empty(len(rows), S, dtype=torch.int32)
    end = torch.empty(len(rows), S, dtype=torch.int32)
    for b, lens in enumerate(rows):
        assert sum(lens) == S
        p = 0
        for n in lens:
            start[b, p : p + n] = p
            end[b, p : p + n] = p + n
            p += n
    return start, end


@pytest.mark.parametrize("rope", [False, True])
def test_reference_with_bounds_equals_per_document_runs(rope):
    """The masked oracle equals the unmasked oracle run on every document alone; with RoPE each document gets the
    table rows of its own positions 0..len-1 while the masked run keeps 0..S-1 -- the relative-position claim."""
    torch.manual_seed(0)
    H, Hkv, D = 4, 2, 16
    rows = [[5, 1, 11, 7], [24], [1, 1, 22]]
    B, S = len(rows), 24
    qkv = torch.randn(B * S, (H + 2 * Hkv) * D)
    cos = sin = None
    if rope:
        cos, sin = R.rope_tables(D, S, 10000.0)
    start, _ = _bounds_from_lengths(rows)
    got = ops.attention_qkv_reference(qkv, B, S, H, Hkv, D, cos, sin, True, doc_start=start).view(B, S, H * D)
    x = qkv.view(B, S, -1)
    for b, lens in enumerate(rows):
        p = 0
        for n in lens:
            alone = ops.attention_qkv_reference(x[b, p : p + n].reshape(n, -1), 1, n, H, Hkv, D,
                                                None if cos is None else cos[:n], None if sin is None else sin[:n],
                                                True)
            # fp32 rounding of the rotations at shifted positions: a few ulp of O(1) values
            torch.testing.assert_close(got[b, p : p + n], alone, rtol=0, atol=2e-5 if rope else 1e-6)
            p += n
    # the CPU branch of flash_attention_qkv takes the same path
    same = ops.flash_attention_qkv(qkv, B, S, H, Hkv, D, cos, sin, True, doc_bounds=_bounds_from_lengths(rows))
    assert torch.equal(same.view(B, S, H * D), got)
    with pytest.raises(ValueError, match="causal"):
        ops.flash_attention_qkv(qkv, B, S, H, Hkv, D, cos, sin, False, doc_bounds=_bounds_from_lengths(rows))
    with pytest.raises(ValueError, match="causal"):
        ops.attention_qkv_reference(qkv, B, S, H, Hkv, D, cos, sin, False, doc_start=start)


def test_model_logits_equal_per_document_runs():
    """A packed row of three documents through a small fp32 model (2 layers, RoPE, GQA 4:2): with doc_mask_token set
    the logits of every document equal those of the document run alone; with masking off they do not."""
    torch.manual_seed(0)
    eot = 7
    model = TransformerLM(vocab_size=64, context_length=32, d_model=32, num_layers=2, num_heads=4, d_ff=64,
                          num_kv_heads=2)
    g = torch.Generator().manual_seed(1)
    docs = []
    for n in (9, 6, 13):  # every document ends with its separator
        d = torch.randint(8, 64, (n,), generator=g)
        d[-1] = eot
        docs.append(d)
    ids = torch.cat(docs)[None]

    def worst(logits: torch.Tensor) -> float:
        p, w = 0, 0.0
        for d in docs:
            alone = model(d[None])[0]
            w = max(w, float((logits[0, p : p + len(d)] - alone).abs().max()))
            p += len(d)
        return w

    with torch.no_grad():
        plain = model(ids)
        model.doc_mask_token = eot
        masked = model(ids)
        explicit = model(ids, doc_bounds=ops.doc_bounds(ids, eot))
        model.doc_mask_token = None
        err, leak = worst(masked), worst(plain)
    assert torch.equal(masked, explicit)
    bound = 7.7e-6  # 10 x the measured max abs difference, 7.7e-7 (CPU fp32, logits of magnitude ~1, this seed)
    print(f"masked vs alone {err:.3e}, unmasked vs alone {leak:.3e}")
    assert err < bound, err
    assert leak > 100 * bound, leak  # negative control: without the mask the comparison sees the leak


def _cfg(tmp_path, **kw) -> TrainConfig:
    cfg = TrainConfig(model=get_preset("ts-tests", vocab_size=256, context_length=16), batch_size=4, max_iters=1,
                      device="cpu", log_every=1, ckpt_dir=str(tmp_path / "ck"))
    cfg.optim.warmup_iters = 1
    cfg.data.synthetic_tokens = 20_000
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_train_config_doc_mask_token(tmp_path):
    tok = 3
    assert TrainConfig().doc_mask_token is None
    assert apply_overrides(TrainConfig(), ["doc_mask_token=50256"]).doc_mask_token == 50256
    tr = Trainer(_cfg(tmp_path, doc_mask_token=tok))
    assert tr.model.doc_mask_token == tok
    x = torch.randint(0, 256, (4, 16), generator=torch.Generator().manual_seed(2))
    x[0, 5] = x[2, 0] = x[3, 15] = tok
    y = torch.roll(x, -1, 1)
    with torch.no_grad():
        want = tr.model.loss(x, y, doc_bounds=ops.doc_bounds(x, tok))
        tr.model.doc_mask_token = None
        plain = tr.model.loss(x, y)
        tr.model.doc_mask_token = tok
    got = tr.engine.train_step([(x, y)], lr=0.0)
    assert float(got) == pytest.approx(float(want), abs=1e-6)
    assert abs(float(plain) - float(want)) > 1e-5  # the mask changes this batch's loss
    # the field travels through a checkpoint's config and back; a config written before the field existed loads
    tr.save(1)
    obj = read_checkpoint(tmp_path / "ck" / "ckpt_00000001.pt")
    assert obj["config"]["doc_mask_token"] == tok
    assert TrainConfig.from_dict(obj["config"]).doc_mask_token == tok
    old = dict(obj["config"])
    del old["doc_mask_token"]
    assert TrainConfig.from_dict(old).doc_mask_token is None
    resumed = Trainer(_cfg(tmp_path, resume=str(tmp_path / "ck" / "ckpt_00000001.pt")))
    assert resumed.start_iter == 1 and resumed.model.doc_mask_token is None
    with pytest.raises(ValueError, match="doc_mask_token"):
        Trainer(_cfg(tmp_path, doc_mask_token=256))
