"""``generate(..., repetition_penalty / presence_penalty / frequency_penalty / logit_bias / return_logprobs)`` on the
CPU: a tiny model, the host sampler and ``sampler="device"`` (which runs the torch references of
``ops/sampling.py`` there).  ``test_sampling_controls_gpu.py`` has the captured-graph twins."""

from __future__ import annotations

import math

import pytest
import torch

from bpe_transformer.models import DecodeSession, TransformerLM
from bpe_transformer.ops import sampling as S

from . import logit_refs as LR

V = 97
SAMPLERS = ["host", "device"]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return TransformerLM(vocab_size=V, context_length=64, d_model=64, num_layers=2, num_heads=4, d_ff=96).eval()


def _prompt(B=2, n=6, seed=1):
    return torch.randint(0, V, (B, n), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_presence_penalty_never_repeats(model, sampler):
    prompt, n = _prompt(), 40
    free = model.generate(prompt, n, temperature=0.0, sampler=sampler)[:, 6:]
    assert any(len(set(r.tolist())) < n for r in free), "the unpenalised model should loop, or this shows nothing"
    out = model.generate(prompt, n, temperature=0.0, sampler=sampler, presence_penalty=1e4)[:, 6:]
    assert out.shape == (2, n) and all(len(set(r.tolist())) == n for r in out)
    # the repetition penalty also sees the prompt; with frequency alone a token may come back, but later
    rep = model.generate(prompt, n, temperature=0.0, sampler=sampler, repetition_penalty=1e4, frequency_penalty=1e4)
    assert all(len(set(r.tolist())) == n for r in rep[:, 6:])


def test_greedy_host_and_device_agree(model):
    prompt = _prompt(seed=3)
    kw = dict(temperature=0.0, repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25,
              logit_bias={5: 2.0, 7: -math.inf}, return_logprobs=True)
    (a, la), (b, lb) = model.generate(prompt, 20, sampler="host", **kw), model.generate(prompt, 20, sampler="device", **kw)
    assert torch.equal(a, b) and torch.equal(la, lb) and la.shape == (2, 20) and la.dtype == torch.float32
    assert not torch.equal(a, model.generate(prompt, 20, temperature=0.0))


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("temperature", [0.0, 1.0])
def test_minus_inf_bias_bans_the_argmax(model, sampler, temperature):
    prompt = _prompt(seed=2)
    first = DecodeSession(model, 2).prefill(prompt).float().argmax(-1)
    kw = dict(temperature=temperature, sampler=sampler, seed=11, generator=torch.Generator().manual_seed(11))
    free = model.generate(prompt, 24, **kw)
    if temperature == 0.0:
        assert torch.equal(free[:, 6], first)
    bias = torch.zeros(V)
    bias[first] = -math.inf
    kw["generator"] = torch.Generator().manual_seed(11)
    for b in (bias, {int(t): -math.inf for t in first}):
        out = model.generate(prompt, 24, logit_bias=b, **kw)
        assert not torch.isin(out[:, 6:], first).any()
        if temperature == 0.0:
            assert bool((out[:, 6] != free[:, 6]).all())


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("as_list", [False, True])
def test_defaults_change_nothing_and_launch_nothing(model, monkeypatch, sampler, as_list):
    calls = []
    # (the host sampler runs the scalar ops, the device sampler their per-row forms: neither may run by default)
    for name in ("logit_process", "token_commit", "prompt_hist", "logit_process_rows", "token_commit_rows"):
        real = getattr(S, name)
        monkeypatch.setattr(S, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    prompt = [_prompt(1, m, seed=m)[0] for m in (3, 7)] if as_list else _prompt()
    run = lambda **kw: model.generate(prompt, 12, temperature=0.9, top_k=20, top_p=0.9, sampler=sampler, seed=4,  # noqa: E731
                                      generator=torch.Generator().manual_seed(4), **kw)
    a = run()
    b = run(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, return_logprobs=False)
    same = all(torch.equal(x, y) for x, y in zip(a, b)) if as_list else torch.equal(a, b)
    assert same and calls == []
    sess = DecodeSession(model, len(prompt), ragged=as_list)
    c = sess.generate(prompt, 12, 0.9, 0.9, None, torch.Generator().manual_seed(4), 20, sampler, 4,
                      repetition_penalty=1.0, logit_bias={})
    assert (all(torch.equal(x, y) for x, y in zip(a, c)) if as_list else torch.equal(a, c)) and calls == []
    run(repetition_penalty=1.1, return_logprobs=True)
    ran = {c.removesuffix("_rows") for c in calls}
    assert {"logit_process", "token_commit", "prompt_hist"} <= ran  # (the spy does see them when they run)


def _model_logprobs(model, seq: torch.Tensor, n_prompt: int) -> tuple[torch.Tensor, torch.Tensor]:
    """log_softmax of ``score``'s fp32 logits at the tokens ``seq[n_prompt:]`` of one sequence, and those rows' max."""
    logits = DecodeSession(model, 1).score(seq[None, :-1]).float()[0, n_prompt - 1 :]
    lp = torch.log_softmax(logits.double(), -1).gather(-1, seq[n_prompt:, None])[:, 0]
    return lp, logits.amax(-1)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_logprobs_are_the_models_own_tensor_prompt(model, sampler):
    prompt, n = _prompt(seed=5), 14
    plain = model.generate(prompt, n, temperature=0.8, top_k=30, sampler=sampler, seed=7,
                           generator=torch.Generator().manual_seed(7))
    eos = int(plain[0, 6 + 4])  # row 0 emits it at step 4; generation goes on until row 1 has, or to the end
    kw = dict(temperature=0.8, top_k=30, sampler=sampler, seed=7, eos_token_id=eos)
    ref = model.generate(prompt, n, generator=torch.Generator().manual_seed(7), **kw)
    out, lp = model.generate(prompt, n, generator=torch.Generator().manual_seed(7), return_logprobs=True, **kw)
    assert torch.equal(out, ref), "log-probs alone do not change what is sampled"
    assert lp.dtype == torch.float32 and lp.shape == (2, out.shape[1] - 6) and not torch.isnan(lp).any()
    for b in range(2):
        want, xmax = _model_logprobs(model, out[b], 6)
        err = (lp[b].double() - want).abs()
        print(f"row {b}: worst |logprob - ref| = {float(err.max()):.3e}")
        assert bool((err <= LR.lse_bound(xmax)).all()), float(err.max())
    # penalties and a bias change the tokens, never what a log-prob means
    out, lp = model.generate(prompt, n, generator=torch.Generator().manual_seed(7), return_logprobs=True,
                             repetition_penalty=1.5, frequency_penalty=0.3, logit_bias={3: 1.0}, **kw)
    for b in range(2):
        want, xmax = _model_logprobs(model, out[b], 6)
        assert bool(((lp[b].double() - want).abs() <= LR.lse_bound(xmax)).all())


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_logprobs_are_the_models_own_list_prompts(model, sampler):
    prompts = [_prompt(1, m, seed=10 + m)[0] for m in (3, 7, 5)]
    n = 12
    plain = model.generate(prompts, n, temperature=0.0, sampler=sampler, presence_penalty=0.7)
    eos = int(plain[0][3 + 2])  # sequence 0 stops after three tokens at the latest
    out, lps = model.generate(prompts, n, temperature=0.0, sampler=sampler, presence_penalty=0.7, eos_token_id=eos,
                              return_logprobs=True)
    assert len(out[0]) <= 3 + 3 and int(out[0][-1]) == eos
    assert max(len(o) - len(p) for o, p in zip(out, prompts)) > 3
    for o, p, lp in zip(out, prompts, lps):
        assert lp.dim() == 1 and lp.dtype == torch.float32 and len(lp) == len(o) - len(p)  # the EOS has its log-prob
        assert torch.equal(o[: len(p)], p) and not torch.isnan(lp).any()
        want, xmax = _model_logprobs(model, o, len(p))
        assert bool(((lp.double() - want).abs() <= LR.lse_bound(xmax)).all())


def test_controls_with_speculative_decoding_are_refused(model):
    prompt = _prompt()
    draft = model.truncated(1)
    for kw in (dict(repetition_penalty=1.2), dict(presence_penalty=0.1), dict(frequency_penalty=0.1),
               dict(logit_bias={1: -1.0}), dict(return_logprobs=True)):
        with pytest.raises(ValueError, match="not supported yet"):
            model.generate(prompt, 8, temperature=0.0, draft_model=draft, **kw)
        with pytest.raises(ValueError, match="not supported yet"):
            model.generate(prompt, 8, temperature=0.0, prompt_lookup=3, **kw)


def test_bad_arguments(model):
    prompt = _prompt()
    with pytest.raises(ValueError):
        model.generate(prompt, 4, repetition_penalty=0.0)
    with pytest.raises(ValueError):
        model.generate(prompt, 4, logit_bias={V: 1.0})
    with pytest.raises(ValueError):
        model.generate(prompt, 4, logit_bias=torch.zeros(V + 1))
