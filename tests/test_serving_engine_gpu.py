"""The continuous-batching engine on the MI355X: the 2-layer d 256 vocab 1000 bf16 model of the ragged tests (context
1024), paged cache, ``sync_every=4``, batch 3 (skinny-GEMM step) and batch 9 (library-GEMM step), with a pool small
enough that a request has to wait.  One prompt of 250 tokens plus 12 new ones crosses a page boundary.

Every check is exact: (a) a request's tokens and log-probs do not depend on its co-tenants' prompts and parameters;
(b) at batch 1 it equals ``model.generate(..., sampler="device")``; (c) one capture for six parameter sets; (d) no
page in use after ``run()``; (e) the fp8 cache and fp8 weights pass (a); (f) ``use_graph=False`` gives the same
tokens."""

from __future__ import annotations

import dataclasses
import functools

import pytest
import torch

from bpe_transformer.models import ServingEngine, SamplingParams, TransformerLM

pytestmark = pytest.mark.gpu

V = 1000
LENS = [(250, 12), (17, 9), (40, 14), (5, 6), (300, 5), (33, 11), (9, 13), (120, 7), (64, 10), (21, 8), (7, 12)]
CHOSEN = 0  # the request that crosses a page boundary


@functools.lru_cache(maxsize=None)
def model(dev):
    torch.manual_seed(0)
    cfg = dict(vocab_size=V, context_length=1024, d_model=256, num_layers=2, num_heads=4, d_ff=512)
    return TransformerLM(**cfg).to(dev, torch.bfloat16).eval()


def prompt(n, seed):
    return torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(seed))


def chosen_params(sampled: bool, n: int) -> SamplingParams:
    if not sampled:
        return SamplingParams(temperature=0.0, max_new_tokens=n, logprobs=True)
    return SamplingParams(temperature=0.9, top_k=50, top_p=0.95, min_p=0.02, seed=1234, max_new_tokens=n,
                          repetition_penalty=1.2, presence_penalty=0.1, frequency_penalty=0.05, logprobs=True)


def tenant_params(i: int, variant: int, n: int) -> SamplingParams:
    """Six parameter sets, rotated by ``variant``: same limits, different everything else."""
    sets = [
        dict(temperature=0.0),
        dict(temperature=0.7, top_k=20, seed=3 + variant),
        dict(temperature=1.2, top_p=0.8, seed=5 + variant, repetition_penalty=1.3),
        dict(temperature=1.0, min_p=0.1, seed=7 + variant, presence_penalty=0.4),
        dict(temperature=0.5, top_k=100, top_p=0.9, min_p=0.01, seed=9 + variant, frequency_penalty=0.3),
        dict(temperature=2.0, seed=11 + variant, logprobs=True),
    ]
    return SamplingParams(max_new_tokens=n, **sets[(i + variant) % len(sets)])


def schedule(eng, variant: int, sampled: bool, count: int):
    """The same arrival schedule for every ``variant``: all requests up front; request ``CHOSEN`` identical, the
    others with other prompt tokens and other sampling parameters but the same lengths and limits."""
    rids = []
    for i, (n, new) in enumerate(LENS[:count]):
        if i == CHOSEN:
            rids.append(eng.submit(prompt(n, 1), chosen_params(sampled, new)))
        else:
            rids.append(eng.submit(prompt(n, 100 * variant + i), tenant_params(i, variant, new)))
    waited = eng.num_waiting
    outs = {o.rid: o for o in eng.step()}
    waited_after = eng.num_waiting
    outs.update(eng.run())
    return rids, outs, waited_after, waited


def engine(dev, batch, **kw):
    # the pool: less than the budgets of `batch` requests of LENS, so somebody waits for pages or a slot
    kw.setdefault("num_pages", 4 if batch == 3 else 10)
    return ServingEngine(model(dev), batch=batch, max_len=1024, kv_layout="paged", sync_every=4, penalties=True,
                         logprobs=True, **kw)


def co_tenant_check(dev, batch, sampled, **kw):
    res = []
    for variant in (0, 1):
        eng = engine(dev, batch, **kw)
        rids, outs, waiting, _ = schedule(eng, variant, sampled, len(LENS))
        assert waiting > 0, "the schedule must make a request wait"
        assert len(outs) == len(LENS) and eng.pages_in_use == 0  # (d)
        assert eng.captures == 1  # (c): six parameter sets, the chosen one's besides
        for i, r in enumerate(rids):
            assert len(outs[r].tokens) == LENS[i][1] and outs[r].finish_reason == "length"
        res.append(outs[rids[CHOSEN]])
    a, b = res
    assert torch.equal(a.tokens, b.tokens), (a.tokens, b.tokens)
    assert torch.equal(a.logprobs, b.logprobs) and torch.isfinite(a.logprobs).all()
    return a


@pytest.mark.parametrize("sampled", (False, True), ids=("greedy", "sampled"))
@pytest.mark.parametrize("batch", (3, 9))
def test_co_tenants_do_not_change_a_request(gpu_device, batch, sampled):
    co_tenant_check(gpu_device, batch, sampled)


@pytest.mark.parametrize("fmt", ("kv_fp8", "w_fp8"))
def test_formats(gpu_device, fmt):
    kw = dict(kv_dtype="fp8") if fmt == "kv_fp8" else dict(weight_dtype="fp8")
    co_tenant_check(gpu_device, 3, True, **kw)


@pytest.mark.parametrize("sampled", (False, True), ids=("greedy", "sampled"))
def test_batch_1_equals_generate(gpu_device, sampled):
    dev = gpu_device
    n, new = LENS[CHOSEN]
    p = prompt(n, 1)
    sp = dataclasses.replace(chosen_params(sampled, new), min_p=0.0)  # (generate has no min_p)
    eng = ServingEngine(model(dev), batch=1, max_len=n + new, kv_layout="paged", sync_every=4)
    rid = eng.submit(p, sp)
    o = eng.run()[rid]
    ref, lp = model(dev).generate([p.to(dev)], new, sp.temperature, sp.top_p, None, top_k=sp.top_k, sampler="device",
                                  seed=sp.seed, repetition_penalty=sp.repetition_penalty,
                                  presence_penalty=sp.presence_penalty, frequency_penalty=sp.frequency_penalty,
                                  return_logprobs=True, kv_layout="paged")
    assert torch.equal(o.tokens, ref[0][n:].cpu()), (o.tokens, ref[0][n:])
    assert torch.equal(o.logprobs, lp[0].cpu())
    assert eng.pages_in_use == 0


def test_eos_ends_a_request_in_the_graph(gpu_device):
    dev = gpu_device
    n, new = LENS[1]
    p = prompt(n, 2)
    eng = engine(dev, 3)
    rid = eng.submit(p, SamplingParams(temperature=0.8, seed=5, max_new_tokens=new))
    full = eng.run()[rid].tokens.tolist()
    eos = full[5]
    rids = [eng.submit(prompt(m, 50 + i), tenant_params(i, 0, k)) for i, (m, k) in enumerate(LENS[2:5])]
    rid = eng.submit(p, SamplingParams(temperature=0.8, seed=5, max_new_tokens=new, eos_token_id=eos))
    outs = eng.run()
    assert outs[rid].tokens.tolist() == full[: full.index(eos) + 1] and outs[rid].finish_reason == "eos"
    assert all(outs[r].finish_reason == "length" for r in rids) and eng.pages_in_use == 0 and eng.captures == 1


def test_no_graph_gives_the_same_tokens(gpu_device):
    res = []
    for use_graph in (True, False):
        eng = engine(gpu_device, 3, use_graph=use_graph)
        rids, outs, _, _ = schedule(eng, 0, True, 6)
        assert eng.captures == int(use_graph) and eng.pages_in_use == 0
        res.append([outs[r] for r in rids])
    for a, b in zip(*res):
        assert torch.equal(a.tokens, b.tokens)
        assert (a.logprobs is None) == (b.logprobs is None)
        if a.logprobs is not None:
            assert torch.equal(a.logprobs, b.logprobs)


def test_a_switch_turned_on_later_captures_once_more(gpu_device):
    eng = ServingEngine(model(gpu_device), batch=3, max_len=1024, kv_layout="paged", num_pages=6, sync_every=4)
    for i in range(4):  # parameter values never capture
        eng.submit(prompt(9 + i, i), SamplingParams(temperature=0.5 * i, top_k=5 * i, seed=i, max_new_tokens=5))
    eng.run()
    assert eng.captures == 1
    rid = eng.submit(prompt(9, 9), SamplingParams(temperature=0.0, max_new_tokens=5, repetition_penalty=1.5))
    plain = eng.submit(prompt(9, 9), SamplingParams(temperature=0.0, max_new_tokens=5))
    outs = eng.run()
    assert eng.captures == 2 and len(outs[rid].tokens) == 5 and len(outs[plain].tokens) == 5
    eng.submit(prompt(9, 9), SamplingParams(temperature=0.0, max_new_tokens=5, repetition_penalty=1.1))
    eng.run()
    assert eng.captures == 2
