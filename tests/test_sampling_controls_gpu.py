"""``generate(sampler="device", ...)`` with sampling controls on the MI355X: the captured step decode ->
``logit_process_rows`` -> ``sample_rows`` -> ``token_commit_rows``, every value read from the sampling table, must give
exactly the tokens and log-probs of a hand loop over the public scalar pieces on the same device (``prefill`` /
``decode`` without a graph, then ``logit_process`` -> ``sample_step`` -> ``token_commit``).  The graphs are keyed by
the three structural switches alone: values never capture, and a call leaves nothing behind for the next."""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer import ops
from bpe_transformer.models import DecodeSession, TransformerLM

pytestmark = pytest.mark.gpu

T, K, P, SEED = 0.8, 50, 0.95, 2**33 + 17
CTL = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2)
_MODELS: dict = {}


def _model(dev, V=1025):
    if V not in _MODELS:
        torch.manual_seed(0)
        cfg = dict(vocab_size=V, context_length=64, d_model=128, num_layers=2, num_heads=2, d_ff=256)
        _MODELS[V] = TransformerLM(**cfg).to(dev, torch.bfloat16).eval()
    return _MODELS[V]


def _prompts(dev, V, as_list, B=3):
    g = torch.Generator().manual_seed(5)
    if as_list:
        return [torch.randint(0, V, (m,), generator=g).to(dev) for m in (3, 7, 5)[:B]]
    return torch.randint(0, V, (B, 6), generator=g).to(dev)


def _bias(dev, V):
    b = torch.zeros(V)
    b[torch.arange(0, V, 7)] = torch.linspace(-3, 3, len(range(0, V, 7)))
    b[11] = -math.inf
    return b.to(dev)


def hand_loop(sess, prompt, n, eos, bias, ctl=CTL):
    """The public pieces, one launch at a time on ``sess`` (no graph): what ``generate`` must reproduce."""
    dev, B = sess.device, sess.batch
    as_list = isinstance(prompt, list)
    if as_list:
        lengths = [len(p) for p in prompt]
        ids = torch.zeros(B, max(lengths), dtype=torch.long, device=dev)
        for b, p in enumerate(prompt):
            ids[b, : len(p)] = p
    else:
        ids, lengths = prompt, None
    sess.reset()
    logits = sess.prefill(ids, lengths)
    V = logits.shape[1]
    hist = ops.prompt_hist(ids, lengths, V)
    rng = torch.tensor([SEED, 0], device=dev)
    tok = torch.zeros(B, 1, dtype=torch.long, device=dev)
    out = torch.full((B, n), -1, dtype=torch.long, device=dev)
    done = torch.zeros(B, dtype=torch.int32, device=dev)
    step = torch.ones(B, dtype=torch.int32, device=dev) if as_list else None
    lse = torch.empty(B, device=dev)
    logprob = torch.full((B, n), math.nan, device=dev)
    keos = eos if as_list and eos is not None else -1  # (a tensor prompt's rows all run on: generate's docstring)
    for i in range(n):
        proc = torch.empty_like(logits)
        ops.logit_process(logits, hist, bias, ctl["repetition_penalty"], ctl["presence_penalty"],
                          ctl["frequency_penalty"], proc, lse)
        ops.sample_step(proc, T, K, P, rng, tok, out, step, done, keos)
        ops.token_commit(out, rng, hist, logits, lse, logprob)
        rng[1] += 1
        active = (done == 0).tolist()
        if not any(active):
            break
        if i + 1 < n:
            logits = sess.decode(tok[:, 0], active=active) if as_list else sess.decode(tok[:, 0])
    out, logprob = out.cpu(), logprob.cpu()
    hit = out == eos if eos is not None else torch.zeros_like(out, dtype=torch.bool)
    first = torch.where(hit.any(1), hit.int().argmax(1), torch.full((B,), n)).tolist()
    if as_list:
        return ([torch.cat([p.cpu(), out[b, : min(first[b] + 1, n)]]) for b, p in enumerate(prompt)],
                [logprob[b, : min(first[b] + 1, n)] for b in range(B)])
    keep = min(max(first) + 1, n)
    return torch.cat([ids.cpu(), out[:, :keep]], 1), logprob[:, :keep]


def _same(got, want, as_list) -> None:
    (gt, gl), (wt, wl) = got, want
    if not as_list:
        gt, gl, wt, wl = [gt], [gl], [wt], [wl]
    assert len(gt) == len(wt)
    for a, b, c, d in zip(gt, gl, wt, wl):
        assert torch.equal(a.cpu(), c) and c.shape[-1] > 0
        assert b.dtype == torch.float32 and torch.equal(b.cpu(), d) and not torch.isnan(d).any()


def _eos(sess, prompt, n, bias):
    """An EOS id that row 0 emits as its fourth token (so rows stop at different times)."""
    toks, _ = hand_loop(sess, prompt, n, None, bias)
    t = toks[0] if isinstance(prompt, list) else toks[0]
    return int(t[-n + 3])


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("as_list", [False, True], ids=["tensor", "ragged"])
def test_generate_equals_hand_loop(gpu_device, as_list, sync_every):
    model = _model(gpu_device)
    prompt, bias, n = _prompts(gpu_device, 1025, as_list), _bias(gpu_device, 1025), 14
    ref = DecodeSession(model, 3, max_len=32, ragged=as_list, use_graph=False)
    eos = _eos(ref, prompt, n, bias)
    want = hand_loop(ref, prompt, n, eos, bias)
    sess = DecodeSession(model, 3, max_len=32, ragged=as_list)
    assert sess.fast and sess.use_graph
    got = sess.generate(prompt, n, T, P, eos, None, K, "device", SEED, sync_every, logit_bias=bias,
                        return_logprobs=True, **CTL)
    _same(got, want, as_list)
    assert len({len(t) for t in want[0]}) > 1 or not as_list, "the rows should stop at different times"
    # the controls do change what is sampled
    plain = sess.generate(prompt, n, T, P, eos, None, K, "device", SEED, sync_every)
    assert not all(torch.equal(a.cpu(), b) for a, b in zip(plain, want[0]))


@pytest.mark.parametrize("as_list", [False, True], ids=["tensor", "ragged"])
def test_graph_equals_no_graph(gpu_device, as_list):
    model = _model(gpu_device)
    prompt, bias, n = _prompts(gpu_device, 1025, as_list), _bias(gpu_device, 1025), 12
    runs = []
    for use_graph in (True, False):
        sess = DecodeSession(model, 3, max_len=32, ragged=as_list, use_graph=use_graph)
        runs.append(sess.generate(prompt, n, T, P, None, None, K, "device", SEED, 4, logit_bias=bias,
                                  return_logprobs=True, **CTL))
    (at, al), (bt, bl) = runs
    if not as_list:
        at, al, bt, bl = [at], [al], [bt], [bl]
    assert all(torch.equal(x, y) for x, y in zip(at, bt)) and all(torch.equal(x, y) for x, y in zip(al, bl))


@pytest.mark.parametrize("kw", [dict(kv_dtype="fp8"), dict(weight_dtype="fp8"), dict(kv_layout="paged")],
                         ids=["kv-fp8", "w-fp8", "paged"])
def test_composes_with_session_options(gpu_device, kw):
    model = _model(gpu_device)
    prompt, bias, n = _prompts(gpu_device, 1025, True), _bias(gpu_device, 1025), 10
    ref = DecodeSession(model, 3, max_len=32, ragged=True, use_graph=False, **kw)
    eos = _eos(ref, prompt, n, bias)
    want = hand_loop(ref, prompt, n, eos, bias)
    sess = DecodeSession(model, 3, max_len=32, ragged=True, **kw)
    got = sess.generate(prompt, n, T, P, eos, None, K, "device", SEED, 4, logit_bias=bias, return_logprobs=True, **CTL)
    _same(got, want, True)


def test_changing_a_penalty_recaptures(gpu_device):
    model = _model(gpu_device)
    prompt, bias, n = _prompts(gpu_device, 1025, False), _bias(gpu_device, 1025), 10
    run = lambda s, **c: s.generate(prompt, n, T, P, None, None, K, "device", SEED, 4, logit_bias=bias,  # noqa: E731
                                    return_logprobs=True, **c)
    sess = DecodeSession(model, 3, max_len=32)
    first = run(sess, **CTL)
    other = dict(CTL, frequency_penalty=0.9)
    second = run(sess, **other)
    # the values live in the sampling table: another value replays the graph of the same three switches
    assert sess._samp["captures"] == 1 and sess._samp["key"] == (True, True, True)
    fresh = run(DecodeSession(model, 3, max_len=32), **other)
    _same(second, (fresh[0].cpu(), fresh[1].cpu()), False)
    assert not torch.equal(first[0], second[0])
    # and back: the history and the log-probs of the earlier call leave nothing behind
    _same(run(sess, **CTL), (first[0].cpu(), first[1].cpu()), False)
    # no controls at all: the key and the graph of a session that never had any
    plain = sess.generate(prompt, n, T, P, None, None, K, "device", SEED, 4)
    assert sess._samp["key"] == (False, False, False) and sess._samp["captures"] == 2
    assert torch.equal(plain, DecodeSession(model, 3, max_len=32).generate(prompt, n, T, P, None, None, K, "device",
                                                                           SEED, 4))


def test_gpt2_vocabulary_once(gpu_device):
    V = 50257
    model = _model(gpu_device, V)
    prompt, n = _prompts(gpu_device, V, False, B=2), 6
    bias = {11: -math.inf, 300: 2.5}
    bt = torch.zeros(V)
    bt[11], bt[300] = -math.inf, 2.5
    want = hand_loop(DecodeSession(model, 2, max_len=16, use_graph=False), prompt, n, None, bt.to(gpu_device))
    got = model.generate(prompt, n, T, P, None, None, True, K, "device", SEED, logit_bias=bias, return_logprobs=True,
                         **CTL)
    _same(got, want, False)
    assert not torch.isin(got[0][:, 6:], torch.tensor([11], device=gpu_device)).any()


def _cpu(r):
    """A ``generate`` result (a tensor, a list, or a ``(tokens, logprobs)`` pair of either) as a flat list on the CPU."""
    parts = r if isinstance(r, tuple) else (r,)
    return [x.cpu() for part in parts for x in (part if isinstance(part, list) else [part])]


def _equal(a, b) -> bool:
    a, b = _cpu(a), _cpu(b)
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_captures_once_per_set_of_switches_never_per_value(gpu_device):
    model = _model(gpu_device)
    prompt, n = _prompts(gpu_device, 1025, True), 10
    bias = _bias(gpu_device, 1025)
    sess = DecodeSession(model, 3, max_len=32, ragged=True)
    gen = lambda t=T, k=K, p=P, eos=None, s=sess, **c: s.generate(prompt, n, t, p, eos, None, k, "device", SEED, 4, **c)  # noqa: E731
    state = lambda s=sess: (s._samp["captures"], s._samp["key"])  # noqa: E731
    first = gen()
    assert state() == (1, (False, False, False))
    for t, k, p, eos in ((0.0, None, None, None), (1.3, 5, None, 7), (0.7, None, 0.5, 300), (T, K, P, int(first[0][-2]))):
        gen(t, k, p, eos)
        assert state() == (1, (False, False, False)), (t, k, p, eos)
    for c in (CTL, dict(CTL, frequency_penalty=0.9), dict(repetition_penalty=0.7), dict(presence_penalty=-0.5)):
        gen(**c)
        assert state() == (2, (True, False, False)), c
    gen(return_logprobs=True)
    assert state() == (3, (False, True, False))
    gen(logit_bias=bias, return_logprobs=True, **CTL)
    gen(0.5, 7, 0.8, 11, logit_bias={3: 1.5}, return_logprobs=True, **dict(CTL, presence_penalty=0.0))
    assert state() == (4, (True, True, True))
    gen(**CTL)  # a graph captured earlier is replayed, not captured again
    assert state() == (4, (True, False, False))
    # a plain call after controlled ones: the tokens and the key of a session that never had any
    fresh = DecodeSession(model, 3, max_len=32, ragged=True)
    assert _equal(gen(), gen(s=fresh)) and _equal(gen(), first)
    assert state() == (4, (False, False, False)) and state(fresh) == (1, (False, False, False))


@pytest.mark.parametrize("as_list", [False, True], ids=["tensor", "ragged"])
def test_no_bias_leak(gpu_device, as_list):
    model = _model(gpu_device)
    prompt, n = _prompts(gpu_device, 1025, as_list), 10
    gen = lambda s, **c: s.generate(prompt, n, T, P, None, None, K, "device", SEED, 4, **c)  # noqa: E731
    want = gen(DecodeSession(model, 3, max_len=32, ragged=as_list))
    # the bias bans every token the plain call emits: values left in the shared buffer would show
    new = lambda r: torch.cat([x[-n:] for x in r]) if as_list else r[:, -n:].reshape(-1)  # noqa: E731
    emitted = new(want)
    sess = DecodeSession(model, 3, max_len=32, ragged=as_list)
    banned = gen(sess, logit_bias={int(v): -math.inf for v in emitted.unique()})
    assert not torch.isin(new(banned), emitted).any()
    assert _equal(gen(sess), want) and sess._samp["key"] == (False, False, False)


@pytest.mark.parametrize("as_list", [False, True], ids=["tensor-shared-pos", "ragged"])
def test_generate_leaves_nothing_behind(gpu_device, as_list):
    """After a ``generate`` without EOS every row is still active: one more ``decode`` of all rows advances every
    length by one and returns the logits of a session without a graph that was driven the same way."""
    model = _model(gpu_device)
    prompt, n = _prompts(gpu_device, 1025, as_list), 9
    got = []
    for use_graph in (True, False):
        sess = DecodeSession(model, 3, max_len=32, ragged=as_list, use_graph=use_graph)
        toks = sess.generate(prompt, n, T, P, None, None, K, "device", SEED, 4)
        t = sess._samp["table"]
        assert t.done.tolist() == [0] * 3 and t.step.tolist() == [1] * 3 and t.count.tolist() == [n] * 3
        before = list(sess.cache._len)
        assert before == [len(p) + n - 1 for p in prompt]
        last = torch.stack([x[-1] for x in toks]) if as_list else toks[:, -1]
        logits = sess.decode(last)
        assert sess.cache._len == [x + 1 for x in before]
        assert sess.cache.pos.tolist() == (sess.cache._len if as_list else sess.cache._len[:1])
        got.append((toks, logits))
    assert _equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
