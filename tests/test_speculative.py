"""Speculative decoding (``SpeculativeSession``, ``generate(..., draft_model=...)``) and the session primitives under
it (``DecodeSession.score`` / ``truncate``): on the CPU oracle path and -- the ``gpu`` twins -- on the captured-graph
fast path, with the tiny models of ``test_device_sampler.py``."""

from __future__ import annotations

import copy

import pytest
import torch

from bpe_transformer.models import DecodeSession, SpeculativeSession, TransformerLM
from bpe_transformer.ops import sampling as S

CFG = {"cpu": dict(vocab_size=97, context_length=64, d_model=64, num_layers=2, num_heads=4, d_ff=96),
       "gpu": dict(vocab_size=1000, context_length=256, d_model=256, num_layers=2, num_heads=4, d_ff=512)}


def _model(kind, dev, seed=0, **over):
    torch.manual_seed(seed)
    m = TransformerLM(**{**CFG[kind], **over}).eval()
    return m if kind == "cpu" else m.to(dev, torch.bfloat16)


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu), pytest.param("gpu-gqa", marks=pytest.mark.gpu)])
def setup(request):
    """(target, unrelated random draft, device, vocabulary, fast path?, session-vs-full-forward bound)"""
    if request.param == "cpu":
        dev = torch.device("cpu")
        return _model("cpu", dev), _model("cpu", dev, 5, num_layers=1), dev, 97, False, 1e-4
    dev = request.getfixturevalue("gpu_device")
    over = {"num_kv_heads": 2} if request.param == "gpu-gqa" else {}
    return _model("gpu", dev, 0, **over), _model("gpu", dev, 5, num_layers=1), dev, 1000, True, 3e-2


def _prompt(dev, V, B=2, S_=6, seed=1):
    return torch.randint(0, V, (B, S_), generator=torch.Generator().manual_seed(seed)).to(dev)


def _rel(a, b):
    return float((a.float() - b.float()).abs().max()) / float(b.float().abs().max())


# ---------------------------------------------------------------- score / truncate
@pytest.mark.parametrize("T", [3, 9])
def test_score_equals_prefill_plus_decode(setup, T):
    """Every position's logits of a scored window are those of feeding the window one token at a time (T = 9 takes
    the cache_attn route on the GPU, T = 3 decode_attn)."""
    model, _, dev, V, fast, tol = setup
    ids = _prompt(dev, V, B=2, S_=5 + T)
    a = DecodeSession(model, 2, max_len=32, ragged=True)
    b = DecodeSession(model, 2, max_len=32, ragged=True)
    assert a.fast == fast
    a.prefill(ids[:, :5])
    got = a.score(ids[:, 5:])
    assert got.shape == (2, T, V) and a.cache.lengths == [5 + T] * 2 == a.cache.pos.tolist()
    b.prefill(ids[:, :5])
    want = torch.stack([b.decode(ids[:, 5 + i]) for i in range(T)], 1)
    assert _rel(got, want) < tol
    # a non-ragged session scores too
    c = DecodeSession(model, 2, max_len=32)
    c.prefill(ids[:, :5])
    assert _rel(c.score(ids[:, 5:]), want) < tol


def test_truncate_then_decode_equals_fresh_session(setup):
    model, _, dev, V, _, tol = setup
    ids = _prompt(dev, V, B=2, S_=12)
    a = DecodeSession(model, 2, max_len=32, ragged=True)
    a.prefill(ids[:, :6])
    a.score(ids[:, 6:11])
    a.truncate([7, 9])
    assert a.cache.lengths == [7, 9] == a.cache.pos.tolist()
    b = DecodeSession(model, 2, max_len=32, ragged=True)
    b.prefill(ids[:, :9], [7, 9])
    tok = ids[:, 11]
    assert _rel(a.decode(tok), b.decode(tok)) < tol
    with pytest.raises(AssertionError):
        a.truncate([20, 3])
    with pytest.raises(AssertionError):
        DecodeSession(model, 2, max_len=32).truncate([1, 1])


# ---------------------------------------------------------------- the hand loop
def _hand_loop(target, draft, prompts, lens, n_new, K, T, seed, eos=-1):
    """Speculative decoding over the public pieces: two ragged sessions, decode, sample_logits with
    philox_uniform(..., stream), score, spec_verify, truncate.  Returns (emitted tokens per row, the sessions)."""
    dev = prompts.device
    B = prompts.shape[0]
    ts = DecodeSession(target, B, max_len=max(lens) + n_new + K + 1, ragged=True)
    ds = DecodeSession(draft, B, max_len=max(lens) + n_new + K + 1, ragged=True)
    logits = ts.prefill(prompts, lens)
    ds.prefill(prompts, lens)
    last = S.sample_logits(logits, T, 0, 1.0, S.philox_uniform(seed, 0, B, dev, stream=2))
    out = [[int(v)] for v in last.tolist()]
    active = [not (len(o) >= n_new or o[-1] == eos) for o in out]
    c = 1
    while any(active):
        base = list(ts.cache.lengths)
        tok, drafts, dl = last, [], []
        for j in range(K):
            lg = ds.decode(tok, active)
            tok = torch.where(torch.tensor(active, device=dev),
                              S.sample_logits(lg, T, 0, 1.0, S.philox_uniform(seed, c + j, B, dev, stream=0)), tok)
            drafts.append(tok)
            dl.append(lg)
        ds.decode(tok, active)
        win = torch.stack([last, *drafts], 1)
        tl = ts.score(win)
        ua = torch.stack([S.philox_uniform(seed, c + j, B, dev, stream=1) for j in range(K)], 1)
        n, y = S.spec_verify(tl, win[:, 1:], torch.stack(dl, 1).to(tl.dtype) if T > 0 else None, T, ua,
                             S.philox_uniform(seed, c, B, dev, stream=2))
        new_len, nxt = list(base), last.clone()
        for b in range(B):
            if not active[b]:
                continue
            m = 0
            for t_ in win[b, 1 : 1 + int(n[b])].tolist() + [int(y[b])]:
                out[b].append(t_)
                m += 1
                if t_ == eos or len(out[b]) >= n_new:
                    active[b] = False
                    break
            new_len[b], nxt[b] = base[b] + m, out[b][-1]
        ts.truncate(new_len)
        ds.truncate(new_len)
        last = nxt
        c += K + 1
    return out, ts, ds


@pytest.mark.parametrize("T", [0.0, 0.8])
@pytest.mark.parametrize("sync_every", [1, 3])
def test_generate_equals_hand_loop(setup, T, sync_every):
    target, draft, dev, V, fast, _ = setup
    K, n_new, seed = 3, 10, 77
    prompt = _prompt(dev, V, B=2)
    sess = SpeculativeSession(target, draft, 2, K, max_len=6 + n_new + K + 1)
    assert sess.fast == fast and sess.use_graph == fast
    got = sess.generate(prompt, n_new, temperature=T, seed=seed, sync_every=sync_every)
    want, ts, ds = _hand_loop(target, draft, prompt, [6, 6], n_new, K, T, seed)
    assert torch.equal(got, torch.cat([prompt, torch.tensor(want, device=dev)], 1))
    for mine, ref in ((sess.target, ts), (sess.draft, ds)):
        assert mine.cache.lengths == mine.cache.pos.tolist() == ref.cache.lengths == [6 + n_new - 1] * 2
    # the sessions serve on: one more plain decode agrees with the hand loop's
    nxt = got[:, -1]
    assert torch.equal(sess.target.decode(nxt).float().argmax(-1), ts.decode(nxt).float().argmax(-1))
    # a ragged list of prompts, through the same session (same graph: other prompts, other seed)
    lens = [3, 6]
    lst = [prompt[0, :3], prompt[1]]
    got = sess.generate(lst, n_new, temperature=T, seed=seed + 1, sync_every=sync_every)
    padded = torch.zeros_like(prompt)
    padded[0, :3], padded[1] = lst[0], lst[1]
    want, ts, ds = _hand_loop(target, draft, padded, lens, n_new, K, T, seed + 1)
    assert [g.tolist() for g in got] == [p.tolist() + w for p, w in zip(lst, want)]
    for mine, ref in ((sess.target, ts), (sess.draft, ds)):
        assert mine.cache.lengths == mine.cache.pos.tolist() == ref.cache.lengths


# ---------------------------------------------------------------- greedy exactness
def _near_argmax(model, ids, n_prompt, bound):
    """Every emitted token's logit in the fp32 full forward of the emitted sequence is within ``bound * max|row|``
    of that row's maximum."""
    full = copy.deepcopy(model).float()(ids)[:, n_prompt - 1 : -1].float()
    chosen = full.gather(-1, ids[:, n_prompt:, None])[..., 0]
    gap = full.amax(-1) - chosen
    assert bool((gap <= bound * full.abs().amax(-1)).all()), float((gap / full.abs().amax(-1)).max())


@pytest.mark.parametrize("K", [4, 9])
def test_greedy_is_the_targets_own_output(setup, K):
    """K = 9: the window takes the cache_attn route.  The bound: the project's session-vs-full-forward bound, once for
    each of the two logits compared (CPU fp32: 1e-4)."""
    target, draft, dev, V, fast, tol = setup
    bound = 2 * tol if fast else tol
    prompt, n_new = _prompt(dev, V, B=3, S_=5), 14
    for d in (target, target.truncated(1), draft):
        sess = SpeculativeSession(target, d, 3, K, max_len=5 + n_new + K + 1)
        got = sess.generate(prompt, n_new, temperature=0.0)
        assert got.shape == (3, 5 + n_new) and torch.equal(got[:, :5], prompt)
        _near_argmax(target, got, 5, bound)
    # the draft is the target: at least 90 % of the drafts stand.  One sequence, a host sync per round: the round
    # counter says how many ran, each proposed K drafts and emitted its accepted ones plus one token
    n_new = 1 + 3 * (K + 1)
    sess = SpeculativeSession(target, target, 1, K, max_len=5 + n_new + K + 1)
    got = sess.generate(prompt[:1], n_new, temperature=0.0, sync_every=1)
    _near_argmax(target, got, 5, bound)
    rounds = (int(sess._st["rngs"][0, 1]) - 1) // (K + 1)
    accepted = (n_new - 1) - rounds
    print(f"K={K}: {rounds} rounds, {accepted} of {K * rounds} drafts accepted")
    assert accepted >= 0.9 * K * rounds
    # through TransformerLM.generate, 1-D prompt included
    one = target.generate(prompt[0], 6, temperature=0.0, draft_model=draft, num_draft_tokens=2)
    assert one.shape == (11,)
    _near_argmax(target, one[None], 5, bound)


def test_truncated_shares_the_weights(setup):
    target = setup[0]
    d = target.truncated(1)
    assert len(d.layers) == 1 and d.config.num_layers == 1 and len(target.layers) == 2
    assert d.lm_head.weight.data_ptr() == target.lm_head.weight.data_ptr()
    assert d.layers[0] is target.layers[0] and d.token_embeddings is target.token_embeddings


# ---------------------------------------------------------------- EOS
def _eos_case(target, draft, dev, V, K, n):
    """Three prompts and an EOS id such that (greedy, draft = the target, so every draft stands) sequence 0 emits it as
    an accepted draft, sequence 1 as the correction / bonus token of a round, and sequence 2 never."""
    for seed in range(200):
        g = torch.Generator().manual_seed(seed)
        prompts = [torch.randint(0, V, (m,), generator=g).to(dev) for m in (3, 7, 5)]
        free = [f[len(p):].tolist() for f, p in zip(target.generate(prompts, n, temperature=0.0), prompts)]
        for eos in set(free[0]):
            i0 = free[0].index(eos)
            if eos in free[2] or eos not in free[1]:
                continue
            i1 = free[1].index(eos)
            # token i >= 1 of the continuation is draft (i - 1) % (K + 1) + 1 of its round, or the round's last token
            if i0 >= 1 and (i0 - 1) % (K + 1) < K and i1 >= 1 and (i1 - 1) % (K + 1) == K:
                return prompts, eos, free
    raise AssertionError("no seed gives the wanted EOS pattern")


def test_eos_stops_each_sequence(setup):
    target, _, dev, V, fast, _ = setup
    K, n = 2, 12
    prompts, eos, free = _eos_case(target, target, dev, V, K, n)
    sess = SpeculativeSession(target, target, 3, K, max_len=7 + n + K + 1)
    got = sess.generate(prompts, n, temperature=0.0, eos_token_id=eos, sync_every=2)
    host = target.generate(prompts, n, temperature=0.0, eos_token_id=eos)
    new = [g[len(p):].tolist() for g, p in zip(got, prompts)]
    assert new[0][-1] == eos and new[1][-1] == eos and eos not in new[2] and len(new[2]) == n
    assert all(eos not in x[:-1] for x in new)
    if not fast:  # fp32 oracle path: the very tokens of the plain session
        assert new == [h[len(p):].tolist() for h, p in zip(host, prompts)]
    # a finished row's cache position stopped while the others went on: all but the last emitted token are cached
    want = [len(p) + len(x) - 1 for p, x in zip(prompts, new)]
    for s in (sess.target, sess.draft):
        assert s.cache.pos.tolist() == want == s.cache.lengths
    # tensor form: rows keep generating until every row has emitted EOS, as with the host sampler
    two = torch.stack([prompts[1][:5], prompts[2]])
    a = target.generate(two, n, temperature=0.0, eos_token_id=eos, draft_model=target, num_draft_tokens=K)
    b = target.generate(two, n, temperature=0.0, eos_token_id=eos)
    assert a.shape == b.shape
    if not fast:
        assert torch.equal(a, b)


# ---------------------------------------------------------------- errors
def test_errors(setup):
    target, draft, dev, V, _, _ = setup
    prompt = _prompt(dev, V)
    with pytest.raises(ValueError, match="top_k"):
        target.generate(prompt, 4, top_k=5, draft_model=draft)
    with pytest.raises(ValueError, match="top_k"):
        target.generate(prompt, 4, top_p=0.9, draft_model=draft)
    other = TransformerLM(**{**CFG["cpu"], "vocab_size": 50}).eval()
    with pytest.raises(ValueError, match="vocabulary"):
        SpeculativeSession(target, other, 2)
    with pytest.raises(ValueError, match="at least 1"):
        SpeculativeSession(target, draft, 2, num_draft_tokens=0)
    sess = SpeculativeSession(target, draft, 2, 3, max_len=6 + 4 + 3)  # one short of prompt + new + K + 1
    with pytest.raises(ValueError, match="KV cache full"):
        sess.generate(prompt, 4, temperature=0.0)
    assert sess.generate(prompt, 3, temperature=0.0).shape == (2, 9)
    with pytest.raises(ValueError, match="context length"):
        target.generate(prompt, CFG["cpu"]["context_length"] * 8, temperature=0.0, draft_model=draft)
