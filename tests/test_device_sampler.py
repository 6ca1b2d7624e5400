"""``generate(..., sampler="device")``: sampling inside the decode loop on the device (``ops.sample_step``), on the
CPU oracle path and -- the ``gpu`` twins -- on the captured-graph fast path with the tiny model of
``test_generation_gpu.py``; plus ``top_k`` on the host sampler."""

from __future__ import annotations

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.models.generation import _sample
from bpe_transformer.ops import sampling as S


def _cpu_model():
    torch.manual_seed(0)
    return TransformerLM(vocab_size=97, context_length=48, d_model=64, num_layers=2, num_heads=4, d_ff=96).eval()


def _gpu_model(dev):
    torch.manual_seed(0)
    cfg = dict(vocab_size=1000, context_length=256, d_model=256, num_layers=2, num_heads=4, d_ff=512)
    return TransformerLM(**cfg).to(dev, torch.bfloat16).eval()


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def setup(request):
    """(model, device, vocabulary, whether the session runs the captured-graph fast path)"""
    if request.param == "cpu":
        return _cpu_model(), torch.device("cpu"), 97, False
    dev = request.getfixturevalue("gpu_device")
    return _gpu_model(dev), dev, 1000, True


def _prompt(dev, V, B=2, S=6, seed=1):
    return torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(seed)).to(dev)


def _ragged_case(model, dev, V, n):
    """Prompts of 3, 7 and 5 tokens and an EOS id such that, decoding greedily, sequence 0 emits it as its first
    token and sequence 1 never does (the first seed at which the model at hand behaves so)."""
    for seed in range(64):
        g = torch.Generator().manual_seed(seed)
        prompts = [torch.randint(0, V, (m,), generator=g).to(dev) for m in (3, 7, 5)]
        free = model.generate(prompts, n, temperature=0.0)
        eos = int(free[0][3])
        if eos not in free[1][7:].tolist():
            return prompts, eos
    raise AssertionError("no seed gives the wanted EOS pattern")


def test_device_generate_equals_hand_loop(setup):
    model, dev, V, fast = setup
    prompt, seed, n = _prompt(dev, V), 1234, 9
    T, k, p = 0.8, 20, 0.9
    sess = DecodeSession(model, 2, max_len=6 + n)
    assert sess.fast == fast and sess.use_graph == fast
    got = sess.generate(prompt, n, temperature=T, top_k=k, top_p=p, sampler="device", seed=seed, sync_every=4)
    assert sess.length == 6 + n - 1
    ref = DecodeSession(model, 2, max_len=6 + n)
    logits, toks = ref.prefill(prompt), []
    for i in range(n):
        toks.append(S.sample_logits(logits, T, k, p, S.philox_uniform(seed, i, 2, dev)))
        if i + 1 < n:
            logits = ref.decode(toks[-1])
    assert torch.equal(got, torch.cat([prompt, torch.stack(toks, 1)], 1))
    # the session goes on as the host loop's would: one more decode agrees with the hand-driven session
    nxt = toks[-1]
    assert torch.equal(sess.decode(nxt).float().argmax(-1), ref.decode(nxt).float().argmax(-1))


def test_device_generate_seeds(setup):
    model, dev, V, _ = setup
    prompt = _prompt(dev, V)
    run = lambda **kw: model.generate(prompt, 12, temperature=1.0, top_p=0.95, sampler="device", **kw)  # noqa: E731
    a, b, c = run(seed=5), run(seed=5), run(seed=6)
    assert a.shape == (2, 18) and torch.equal(a[:, :6], prompt)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # seed=None draws the seed from the generator, and only that
    d = run(generator=torch.Generator().manual_seed(9))
    e = run(generator=torch.Generator().manual_seed(9))
    assert torch.equal(d, e) and not torch.equal(d, a)
    one = model.generate(prompt[0], 5, temperature=1.0, sampler="device", seed=5)
    assert one.shape == (11,)


def test_device_greedy_equals_host_greedy(setup):
    model, dev, V, _ = setup
    prompt = _prompt(dev, V, B=3)
    host = model.generate(prompt, 10, temperature=0.0)
    assert torch.equal(model.generate(prompt, 10, temperature=0.0, sampler="device"), host)
    assert torch.equal(model.generate(prompt, 10, temperature=0.7, top_k=1, sampler="device", seed=1), host)


@pytest.mark.parametrize("sync_every", [1, 3, 16])
def test_device_eos_tensor_form(setup, sync_every):
    model, dev, V, _ = setup
    prompt = _prompt(dev, V, B=1)
    free = model.generate(prompt, 12, temperature=0.0)
    eos = int(free[0, 6 + 4])  # greedy emits it at step 4 (or earlier, if it repeats)
    host = model.generate(prompt, 12, temperature=0.0, eos_token_id=eos)
    assert host.shape[1] < 18
    sess = DecodeSession(model, 1, max_len=18)
    got = sess.generate(prompt, 12, temperature=0.0, eos_token_id=eos, sampler="device", sync_every=sync_every)
    assert torch.equal(got, host)
    assert sess.length == host.shape[1] - 1 and sess.cache.pos.tolist() == [sess.length]
    # two rows: the first to finish keeps generating until the other has, as on the host
    two = _prompt(dev, V, B=2, seed=4)
    free = model.generate(two, 12, temperature=0.0)
    eos = int(free[1, 6 + 2])
    host = model.generate(two, 12, temperature=0.0, eos_token_id=eos)
    assert torch.equal(model.generate(two, 12, temperature=0.0, eos_token_id=eos, sampler="device"), host)


def test_device_eos_ragged_form(setup):
    model, dev, V, fast = setup
    n = 11  # not a multiple of sync_every
    prompts, eos0 = _ragged_case(model, dev, V, n)
    host = model.generate(prompts, n, temperature=0.0, eos_token_id=eos0)
    sess = DecodeSession(model, 3, max_len=7 + n, ragged=True)
    assert sess.fast == fast
    got = sess.generate(prompts, n, temperature=0.0, eos_token_id=eos0, sampler="device", sync_every=4)
    assert [t.tolist() for t in got] == [t.tolist() for t in host]
    assert len(got[0]) == 4 and len(got[1]) == 7 + n
    assert sess.cache.lengths == sess.cache.pos.tolist()
    assert sess.cache.lengths[0] == 3 and sess.cache.lengths[1] == 7 + n - 1
    # the session serves on: refill slot 0, decode it with slot 1, against a fresh session fed the same tokens
    new = _prompt(dev, V, B=1, S=4, seed=8)[0]
    fresh = DecodeSession(model, 3, max_len=7 + n + 2, ragged=True)
    ids = torch.zeros(3, 7 + n - 1, dtype=torch.long, device=dev)
    ids[0, :4] = new
    ids[1] = got[1][:-1]
    ids[2, : sess.cache.lengths[2]] = got[2][: sess.cache.lengths[2]]
    fresh.prefill(ids, [4, 7 + n - 1, sess.cache.lengths[2]])
    sess.reset_slot(0)
    l0 = sess.prefill_slot(0, new)
    assert sess.cache.lengths == fresh.cache.lengths
    tok = torch.stack([l0[0].float().argmax(), got[1][-1], got[2][-1]]).to(dev)
    active = [True, True, False]
    a, b = sess.decode(tok, active), fresh.decode(tok, active)
    tol = 3e-2 if fast else 1e-4
    assert float((a[:2].float() - b[:2].float()).abs().max()) <= tol * float(b[:2].float().abs().max())
    assert sess.cache.lengths == sess.cache.pos.tolist()


def test_device_sampler_checks_capacity_up_front(setup):
    model, dev, V, _ = setup
    sess = DecodeSession(model, 2, max_len=10)
    with pytest.raises(AssertionError, match="KV cache full"):
        sess.generate(_prompt(dev, V), 5, sampler="device", seed=0)
    assert sess.generate(_prompt(dev, V), 4, sampler="device", seed=0).shape == (2, 10)


def test_host_top_k_restricts_draws():
    model = _cpu_model()
    prompt = _prompt(torch.device("cpu"), 97)
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(4, 97, generator=g)
    top = logits.topk(3, -1).indices
    for _ in range(20):
        t = _sample(logits, 1.5, None, g, top_k=3)
        assert all(int(t[b]) in top[b].tolist() for b in range(4))
        t = _sample(logits, 1.5, 0.99, g, top_k=3)
        assert all(int(t[b]) in top[b].tolist() for b in range(4))
    assert torch.equal(_sample(logits, 1.5, None, g, top_k=1), logits.argmax(-1))
    # through generate, with and without the cache: top_k = 1 is greedy whatever the temperature
    greedy = model.generate(prompt, 6, temperature=0.0)
    for use_cache in (True, False):
        assert torch.equal(model.generate(prompt, 6, temperature=2.0, top_k=1, use_cache=use_cache), greedy)


def test_top_k_none_leaves_the_host_stream_unchanged():
    """test_generation.py's reproducibility case, and bit-for-bit the sampler of before: same generator draws."""
    model = _cpu_model()
    prompt = _prompt(torch.device("cpu"), 97, S=4)
    outs = []
    for kw in ({}, {"top_k": None}, {"top_k": None, "sampler": "host"}):
        g = torch.Generator().manual_seed(7)
        outs.append(model.generate(prompt, 8, temperature=0.8, top_p=0.9, generator=g, **kw))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # the sampler itself against the formula it had before top_k existed
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    logits = torch.randn(3, 97, generator=torch.Generator().manual_seed(1))
    probs = torch.softmax(logits.float() / 0.8, dim=-1)
    sp, si = probs.sort(dim=-1, descending=True)
    sp = sp * (sp.cumsum(-1) - sp < 0.9)
    probs = torch.zeros_like(probs).scatter_(-1, si, sp)
    want = torch.multinomial(probs / probs.sum(-1, keepdim=True), 1, generator=g1).squeeze(-1)
    assert torch.equal(_sample(logits, 0.8, 0.9, g2), want)
