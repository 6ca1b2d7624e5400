"""Prompt-lookup speculative decoding (``PromptLookupSession``, ``generate(..., prompt_lookup=...)``) on the CPU oracle
path and -- the ``gpu`` twins -- on the captured-graph fast path, with the tiny models and the three setups of
``test_speculative.py``."""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.models import DecodeSession, PromptLookupSession, SpeculativeSession
from bpe_transformer.ops import sampling as S

from .lookup_refs import lookup
from .test_speculative import _model, _near_argmax, _prompt


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu), pytest.param("gpu-gqa", marks=pytest.mark.gpu)])
def setup(request):
    """(kind, model overrides, device, vocabulary, fast path?, session-vs-full-forward bound)"""
    if request.param == "cpu":
        return "cpu", {}, torch.device("cpu"), 97, False, 1e-4
    over = {"num_kv_heads": 2} if request.param == "gpu-gqa" else {}
    return "gpu", over, request.getfixturevalue("gpu_device"), 1000, True, 3e-2


def _target(setup, seed=0, **over):
    kind, base, dev = setup[:3]
    return _model(kind, dev, seed, **base, **over)


def _cycling_target(setup, seed=0, **over):
    """A target whose ``attn.output_proj`` and ``ffn.w2`` are zero in every layer: its hidden state is the current
    token's embedding, so its greedy output iterates a map ``token -> token`` on 64 tokens and enters a cycle."""
    target = _target(setup, seed, vocab_size=64, **over)
    for layer in target.layers:
        layer.attn.output_proj.weight.data.zero_()
        layer.ffn.w2.weight.data.zero_()
    return target


# ---------------------------------------------------------------- the hand loop
def _hand_loop(target, prompts, lens, n_new, K, T, seed, n_hi, n_lo, eos=-1):
    """Prompt-lookup decoding over the public pieces: one ragged session (prefill, score, truncate), the oracle
    lookup, spec_verify(point_mass=True) and philox_uniform.  Returns (emitted tokens per row, the session, rounds)."""
    dev = prompts.device
    B = prompts.shape[0]
    ts = DecodeSession(target, B, max_len=max(lens) + n_new + K + 1, ragged=True)
    logits = ts.prefill(prompts, lens)
    last = S.sample_logits(logits, T, 0, 1.0, S.philox_uniform(seed, 0, B, dev, stream=2))
    out = [[int(v)] for v in last.tolist()]
    active = [not (len(o) >= n_new or o[-1] == eos) for o in out]
    c = 1
    while any(active):
        base = list(ts.cache.lengths)
        drafts = [lookup(prompts[b, : lens[b]].tolist() + out[b], K, n_hi, n_lo) for b in range(B)]
        win = torch.cat([last[:, None], torch.tensor(drafts, device=dev)], 1)
        tl = ts.score(win)
        ua = torch.stack([S.philox_uniform(seed, c + j, B, dev, stream=1) for j in range(K)], 1)
        n, y = S.spec_verify(tl, win[:, 1:], None, T, ua, S.philox_uniform(seed, c, B, dev, stream=2), point_mass=True)
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
        last = nxt
        c += K + 1
    return out, ts, (c - 1) // (K + 1)


def _rounds(sess) -> int:
    return (int(sess._st["rngs"][0, 1]) - 1) // (sess.K + 1)


@pytest.mark.parametrize("T", [0.0, 0.8])
@pytest.mark.parametrize("sync_every", [1, 3])
def test_generate_equals_hand_loop(setup, T, sync_every):
    """A tensor prompt, then a ragged list through the same session (the same graph: other prompts, another seed).
    The first prompt is the longer one, 8 tokens against a padded width of 6, and built to match: row 0 repeats the
    second call's first emitted token of row 0, each time followed by another token.  Its last two columns stay
    behind in the session's static prompt buffer, past the second call's ``n_prompt[0] = 3`` and its padding: a
    lookup that read them would draft that other token instead of finding no match."""
    _, _, dev, V, fast, _ = setup
    target = _target(setup)
    K, n_new, seed, n_hi, n_lo = 3, 10, 77, 3, 1
    base = _prompt(dev, V, B=2, S_=8)
    lens = [3, 6]
    lst = [base[0, :3], base[1, :6]]
    padded = torch.zeros(2, 6, dtype=base.dtype, device=dev)
    padded[0, :3], padded[1] = lst[0], lst[1]
    want2, ts2, rounds2 = _hand_loop(target, padded, lens, n_new, K, T, seed + 1, n_hi, n_lo)
    f0 = want2[0][0]
    first = base.clone()
    first[0, 3:] = torch.tensor([(f0 + 1) % V, f0, (f0 + 2) % V, f0, (f0 + 3) % V])  # (what stays behind, stale)

    sess = PromptLookupSession(target, 2, K, (n_hi, n_lo), max_len=8 + n_new + K + 1)
    assert sess.fast == fast and sess.use_graph == fast and sess.draft is None
    got = sess.generate(first, n_new, temperature=T, seed=seed, sync_every=sync_every)
    want, ts, rounds = _hand_loop(target, first, [8, 8], n_new, K, T, seed, n_hi, n_lo)
    assert torch.equal(got, torch.cat([first, torch.tensor(want, device=dev)], 1))
    assert sess.target.cache.lengths == sess.target.cache.pos.tolist() == ts.cache.lengths == [8 + n_new - 1] * 2
    if sync_every == 1:  # a host look per round: no round runs after the last token
        assert _rounds(sess) == rounds
    # the session serves on: one more plain decode agrees with the hand loop's
    nxt = got[:, -1]
    assert torch.equal(sess.target.decode(nxt).float().argmax(-1), ts.decode(nxt).float().argmax(-1))

    got = sess.generate(lst, n_new, temperature=T, seed=seed + 1, sync_every=sync_every)
    assert sess._st["prompt"][0, 6:8].tolist() == first[0, 6:].tolist() == [f0, (f0 + 3) % V]  # stale, still there
    assert [g.tolist() for g in got] == [p.tolist() + w for p, w in zip(lst, want2)]
    assert sess.target.cache.lengths == sess.target.cache.pos.tolist() == ts2.cache.lengths
    if sync_every == 1:
        assert _rounds(sess) == rounds2


# ---------------------------------------------------------------- greedy exactness
@pytest.mark.parametrize("K", [4, 9])
def test_greedy_is_the_targets_own_output(setup, K):
    """K = 9: the window takes the cache_attn route.  The criterion and bounds are those of ``test_speculative.py``."""
    _, _, dev, V, fast, tol = setup
    target = _target(setup)
    bound = 2 * tol if fast else tol
    prompt, n_new = _prompt(dev, V, B=3, S_=5), 14
    prompt[1, 3:] = prompt[1, :2]  # one row whose prompt repeats: its lookups match from the first round on
    sess = PromptLookupSession(target, 3, K, 3, max_len=5 + n_new + K + 1)
    got = sess.generate(prompt, n_new, temperature=0.0)
    assert got.shape == (3, 5 + n_new) and torch.equal(got[:, :5], prompt)
    _near_argmax(target, got, 5, bound)
    # through TransformerLM.generate, 1-D prompt included
    one = target.generate(prompt[0], 6, temperature=0.0, prompt_lookup=3, num_draft_tokens=2)
    assert one.shape == (11,)
    _near_argmax(target, one[None], 5, bound)
    two = target.generate(prompt, 6, temperature=0.0, prompt_lookup=(3, 2), num_draft_tokens=K)
    assert two.shape == (3, 11)
    _near_argmax(target, two, 5, bound)


# ---------------------------------------------------------------- drafts really stand
CYCLE_SEED = 44


def test_drafts_stand_on_a_cycling_target(setup):
    """From the first repeated token on, the lookup's drafts on the cycling target are the target's own tokens: at
    least half of the rounds emit more than one token.

    The rounds are counted from ``rngs`` (one sequence, a host look per round).  How many tokens each emitted follows
    from the output alone: greedy draft ``j`` stands iff it is the token the target emitted at its position, so
    replaying the oracle lookup over the emitted sequence gives every round's count, and the replay must take
    exactly the counted number of rounds.

    CYCLE_SEED = 44 for the weights: of the seeds 0..59 it is one of six at which, on the token map alone (fp32, on
    the CPU), at least 60 % of the rounds emit more than one token under all three configurations -- here 11 of 15,
    11 of 16 and 11 of 16, where half are asked for -- and among those the one whose bf16 configurations keep the
    widest top-two logit gap on every visited row (4.6 % of the row's largest logit, a dozen bf16 roundings), so the
    fast path takes the same walk."""
    _, _, dev, _, fast, _ = setup
    K, n_new = 4, 60
    target = _cycling_target(setup, CYCLE_SEED, context_length=128)
    prompt = _prompt(dev, 64, B=1, S_=4)
    sess = PromptLookupSession(target, 1, K, (2, 1), max_len=4 + n_new + K + 1)
    assert sess.fast == fast
    got = sess.generate(prompt, n_new, temperature=0.0, sync_every=1)
    assert got.shape == (1, 4 + n_new)
    seq = got[0].tolist()
    at, counts = 5, []  # (the first new token is the prefill's)
    while at < len(seq):
        d, n = lookup(seq[:at], K, 2, 1), 0
        while n < K and at + n < len(seq) and d[n] == seq[at + n]:
            n += 1
        m = min(n + 1, len(seq) - at)
        counts.append(m)
        at += m
    multi = sum(c > 1 for c in counts)
    print(f"{len(counts)} rounds, {multi} of them emitted more than one token: {counts}")
    assert _rounds(sess) == len(counts)
    assert 2 * multi >= len(counts)


# ---------------------------------------------------------------- EOS and the output limit
def test_eos_and_the_output_limit(setup):
    """Row 0's prompt is six distinct tokens ``w[0..5]`` of a greedy walk of the cycling target followed by ``w[0..2]``
    again: the first emitted token is ``w[3]``, the first round's lookup drafts ``w[4], w[5], w[0], ...`` of which
    the first two stand, so ``eos = w[5]`` arrives as an accepted draft in the middle of a window.  Each sequence
    stops inclusive at its first EOS; ``max_new_tokens`` cuts a window."""
    _, _, dev, _, fast, _ = setup
    K, n = 4, 20
    target = _cycling_target(setup)
    walks = (target.generate(torch.tensor([s0], device=dev), 5, temperature=0.0).tolist() for s0 in range(64))
    w = next(w for w in walks if len(set(w)) == 6)
    g = torch.Generator().manual_seed(4)
    prompts = [torch.tensor(w + w[:3], device=dev), *(torch.randint(0, 64, (m,), generator=g).to(dev) for m in (7, 5))]
    sess = PromptLookupSession(target, 3, K, 2, max_len=9 + n + K + 1)
    free = [f[len(p):].tolist() for f, p in zip(sess.generate(prompts, n, temperature=0.0), prompts)]
    assert all(len(f) == n for f in free) and free[0][:3] == w[3:]
    plain = target.generate(prompts, n, temperature=0.0)
    if not fast:  # fp32 oracle path: the very tokens of the plain session
        assert free == [h[len(p):].tolist() for h, p in zip(plain, prompts)]
    eos = w[5]
    got = sess.generate(prompts, n, temperature=0.0, eos_token_id=eos, sync_every=2)
    new = [x[len(p):].tolist() for x, p in zip(got, prompts)]
    for b in range(3):
        stop = free[b].index(eos) + 1 if eos in free[b] else n
        assert new[b] == free[b][:stop], (b, new[b], free[b])
    assert new[0] == w[3:]
    want = [len(p) + len(x) - 1 for p, x in zip(prompts, new)]
    assert sess.target.cache.pos.tolist() == want == sess.target.cache.lengths
    # the EOS stood as a draft: one row, a host look per round -- three tokens, the first the prefill's, in one round
    one = PromptLookupSession(target, 1, K, 2, max_len=9 + n + K + 1)
    x = one.generate([prompts[0]], n, temperature=0.0, eos_token_id=eos, sync_every=1)[0]
    assert x[9:].tolist() == w[3:] and _rounds(one) == 1
    # max_new_tokens cuts a window: the second round of row 0 would emit past it
    for cut in (2, 1 + (K + 1) + 2):
        short = sess.generate(prompts, cut, temperature=0.0)
        assert [s[len(p):].tolist() for s, p in zip(short, prompts)] == [f[:cut] for f in free]
    # tensor form: rows keep generating until every row has emitted EOS, as with the host sampler
    two = torch.stack([prompts[1][:5], prompts[2]])
    a = target.generate(two, n, temperature=0.0, eos_token_id=eos, prompt_lookup=2, num_draft_tokens=K)
    b = target.generate(two, n, temperature=0.0, eos_token_id=eos)
    assert a.shape == b.shape
    if not fast:
        assert torch.equal(a, b)


# ---------------------------------------------------------------- errors
def test_errors(setup):
    _, _, dev, V, _, _ = setup
    target = _target(setup)
    prompt = _prompt(dev, V)
    with pytest.raises(ValueError, match="draft_model"):
        target.generate(prompt, 4, prompt_lookup=3, draft_model=target)
    with pytest.raises(ValueError, match="top_k"):
        target.generate(prompt, 4, top_k=5, prompt_lookup=3)
    with pytest.raises(ValueError, match="top_k"):
        target.generate(prompt, 4, top_p=0.9, prompt_lookup=3)
    for bad in (0, (3, 0), (2, 3)):
        with pytest.raises(ValueError, match="n_lo"):
            target.generate(prompt, 4, prompt_lookup=bad)
        with pytest.raises(ValueError, match="n_lo"):
            PromptLookupSession(target, 2, 3, bad)
    with pytest.raises(ValueError, match="at least 1"):
        target.generate(prompt, 4, prompt_lookup=3, num_draft_tokens=0)
    with pytest.raises(ValueError, match="at least 1"):
        PromptLookupSession(target, 2, num_draft_tokens=0)
    with pytest.raises(ValueError, match="not supported yet"):
        target.generate(prompt, 4, prompt_lookup=3, kv_dtype="fp8")
    with pytest.raises(ValueError, match="not supported yet"):
        target.generate(prompt, 4, prompt_lookup=3, weight_dtype="fp8")
    with pytest.raises(ValueError, match="not supported yet"):
        PromptLookupSession(target, 2, kv_dtype="fp8")
    sess = PromptLookupSession(target, 2, 3, 3, max_len=6 + 4 + 3)  # one short of prompt + new + K + 1
    with pytest.raises(ValueError, match="KV cache full"):
        sess.generate(prompt, 4, temperature=0.0)
    assert sess.generate(prompt, 3, temperature=0.0).shape == (2, 9)
    with pytest.raises(ValueError, match="context length"):
        target.generate(prompt, 64 * 8, temperature=0.0, prompt_lookup=3)
    assert isinstance(sess, SpeculativeSession)  # one round engine, two proposers
