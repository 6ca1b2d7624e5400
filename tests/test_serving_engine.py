"""The continuous-batching engine (``bpe_transformer/models/serving.py``) on the CPU: a tiny fp32 model on the
reference ops.  Scheduling (FIFO into the lowest free slot, page-budget admission, the budget returning on an early
EOS), the ``ValueError`` cases of ``submit``, ``finish_reason``, ``run()``, and a request's tokens against a
hand-driven ragged ``DecodeSession`` of the same batch on the scalar reference path."""

from __future__ import annotations

import functools

import pytest
import torch

from bpe_transformer.models import DecodeSession, ServingEngine, SamplingParams, TransformerLM
from bpe_transformer.ops import sampling as S

V = 64


@functools.lru_cache(maxsize=None)
def model():
    torch.manual_seed(0)
    return TransformerLM(vocab_size=V, context_length=600, d_model=32, num_layers=2, num_heads=2, d_ff=64).eval()


def prompt(n, seed=0):
    return torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(seed))


def one(eng, p, sp):
    """Submit one request and run the engine dry: its output."""
    rid = eng.submit(p, sp)
    return eng.run()[rid]


def test_fifo_into_lowest_free_slot():
    eng = ServingEngine(model(), batch=3, max_len=64, sync_every=2)
    r = [eng.submit(prompt(4 + i, i), SamplingParams(temperature=0.0, max_new_tokens=n))
         for i, n in enumerate((9, 2, 9, 5, 3))]
    done = eng.step()
    assert [eng.slot_of(x) for x in r] == [0, None, 2, None, None]  # r1 ran in slot 1 and is finished
    assert [o.rid for o in done] == [r[1]] and eng.num_waiting == 2
    eng.step()
    assert eng.slot_of(r[3]) == 1 and eng.slot_of(r[4]) is None  # first come first served, the lowest free slot
    outs = eng.run()
    assert sorted(outs) == sorted(set(r) - {r[1]}) and eng.num_running == 0 and eng.num_waiting == 0
    assert [len(outs[x].tokens) for x in (r[0], r[2], r[3], r[4])] == [9, 9, 5, 3]
    assert all(o.finish_reason == "length" and o.logprobs is None for o in outs.values())


def test_page_budget_makes_a_request_wait():
    eng = ServingEngine(model(), batch=3, max_len=600, kv_layout="paged", num_pages=3, sync_every=4)
    a = eng.submit(prompt(250, 1), SamplingParams(temperature=0.0, max_new_tokens=40))  # 290 tokens: 2 pages
    b = eng.submit(prompt(5, 2), SamplingParams(temperature=0.0, max_new_tokens=6))  # 1 page
    c = eng.submit(prompt(5, 3), SamplingParams(temperature=0.0, max_new_tokens=9))  # 1 page: over the budget of 3
    eng.step()
    assert eng.slot_of(a) == 0 and eng.slot_of(b) == 1 and eng.slot_of(c) is None and eng.num_waiting == 1
    assert eng.pages_in_use <= 3
    outs = {}
    while eng.slot_of(c) is None and eng.num_waiting:
        outs.update({o.rid: o for o in eng.step()})
    assert b in outs and eng.slot_of(c) == 1  # admitted when b's page came back, a still running
    assert eng.slot_of(a) == 0
    outs.update(eng.run())
    assert len(outs[a].tokens) == 40 and len(outs[c].tokens) == 9 and eng.pages_in_use == 0


def test_budget_returns_on_early_eos():
    p = prompt(200, 4)
    probe = ServingEngine(model(), batch=1, max_len=600)
    first = one(probe, p, SamplingParams(temperature=0.0, max_new_tokens=3)).tokens.tolist()
    eos = first[1] if first[1] != first[0] else first[0]
    eng = ServingEngine(model(), batch=2, max_len=600, kv_layout="paged", num_pages=2, sync_every=4)
    a = eng.submit(p, SamplingParams(temperature=0.0, max_new_tokens=100, eos_token_id=eos))  # 300 tokens: 2 pages
    b = eng.submit(prompt(7, 5), SamplingParams(temperature=0.0, max_new_tokens=4))
    done = eng.step()
    assert [o.rid for o in done] == [a] and done[0].finish_reason == "eos"
    assert done[0].tokens.tolist() == first[: first.index(eos) + 1]
    assert eng.slot_of(b) is None and eng.pages_in_use == 0  # b waited for the budget; a's pages are back
    outs = eng.run()
    assert outs[b].finish_reason == "length" and len(outs[b].tokens) == 4 and eng.pages_in_use == 0


def test_submit_rejects_what_can_never_run():
    eng = ServingEngine(model(), batch=2, max_len=600, kv_layout="paged", num_pages=1)
    ok = SamplingParams(max_new_tokens=4)
    with pytest.raises(ValueError, match="max_len"):
        eng.submit(prompt(598), ok)
    with pytest.raises(ValueError, match="pages"):
        eng.submit(prompt(255), ok)  # 259 tokens: 2 pages, the pool has 1
    with pytest.raises(ValueError, match="speculative"):
        eng.submit(prompt(4), ok, draft_model=model())
    with pytest.raises(ValueError, match="speculative"):
        eng.submit(prompt(4), ok, prompt_lookup=3)
    with pytest.raises(ValueError, match="logit_bias"):
        eng.submit(prompt(4), SamplingParams(max_new_tokens=4, logit_bias={1: 2.0}))
    with pytest.raises(ValueError, match="empty"):
        eng.submit(torch.zeros(0, dtype=torch.long), ok)
    assert eng.num_waiting == 0 and eng.run() == {}


def test_a_request_can_end_on_its_first_token():
    p = prompt(6, 6)
    probe = ServingEngine(model(), batch=1, max_len=64)
    first = int(one(probe, p, SamplingParams(temperature=0.0, max_new_tokens=1)).tokens[0])
    eng = ServingEngine(model(), batch=2, max_len=64)
    a = eng.submit(p, SamplingParams(temperature=0.0, max_new_tokens=5, eos_token_id=first))
    b = eng.submit(p, SamplingParams(temperature=0.0, max_new_tokens=1))
    outs = eng.run()
    assert outs[a].tokens.tolist() == [first] and outs[a].finish_reason == "eos"
    assert outs[b].tokens.tolist() == [first] and outs[b].finish_reason == "length"


PARAMS = [
    SamplingParams(temperature=0.0, max_new_tokens=9),
    SamplingParams(temperature=0.8, top_k=10, top_p=0.9, seed=5, max_new_tokens=11),
    SamplingParams(temperature=1.1, seed=2**40 + 3, max_new_tokens=7, repetition_penalty=1.3, presence_penalty=0.2,
                   frequency_penalty=0.1, logprobs=True),
]


def hand_driven(p, sp: SamplingParams, batch: int, slot: int):
    """A ragged session of ``batch`` slots, ``slot`` alone in use: ``prefill_slot``, then the scalar reference path
    (``logit_process`` -> ``sample_step`` -> ``token_commit`` -> decode) with the request's own parameters."""
    m = model()
    sess = DecodeSession(m, batch, max_len=64, ragged=True)
    hist = S.prompt_hist(p[None], None, V)
    rng = torch.tensor([sp.seed, 0])
    ids, out = torch.zeros(1, 1, dtype=torch.long), torch.full((1, sp.max_new_tokens), -1)
    done, lse = torch.zeros(1, dtype=torch.int32), torch.zeros(1)
    lp = torch.full((1, sp.max_new_tokens), float("nan"))
    logits = sess.prefill_slot(slot, p)
    active = [b == slot for b in range(batch)]
    for i in range(sp.max_new_tokens):
        proc = torch.empty_like(logits)
        S.logit_process_reference(logits, hist, None, sp.repetition_penalty, sp.presence_penalty,
                                  sp.frequency_penalty, proc, lse)
        S.sample_step_reference(proc, sp.temperature, int(sp.top_k or 0), 1.0 if sp.top_p is None else sp.top_p, rng,
                                ids, out, None, done, -1 if sp.eos_token_id is None else sp.eos_token_id)
        S.token_commit_reference(out, rng, hist, logits, lse, lp)
        rng[1] += 1
        if int(done[0]) or i + 1 == sp.max_new_tokens:
            break
        feed = torch.zeros(batch, dtype=torch.long)
        feed[slot] = ids[0, 0]
        logits = sess.decode(feed, active=active)[slot : slot + 1]
    n = int(rng[1])
    return out[0, :n], lp[0, :n]


@pytest.mark.parametrize("which", range(len(PARAMS)))
def test_tokens_equal_hand_driven_session(which):
    sp = PARAMS[which]
    eng = ServingEngine(model(), batch=3, max_len=64, sync_every=4)
    rids = [eng.submit(prompt(5 + 3 * i, 10 + i), q) for i, q in enumerate(PARAMS)]  # slots 0, 1, 2 with co-tenants
    outs = eng.run()
    toks, lp = hand_driven(prompt(5 + 3 * which, 10 + which), sp, 3, which)
    o = outs[rids[which]]
    assert o.tokens.tolist() == toks.tolist()
    if sp.logprobs:
        torch.testing.assert_close(o.logprobs, lp, rtol=0, atol=1e-5)  # (other rows' lengths change the fp32 sums)
    else:
        assert o.logprobs is None
    assert eng.captures == 0  # no graph off the fast path


def test_eos_equals_hand_driven_session():
    p = prompt(8, 20)
    base = SamplingParams(temperature=0.9, top_k=12, seed=9, max_new_tokens=12)
    eng = ServingEngine(model(), batch=2, max_len=64, sync_every=3)
    full = one(eng, p, base).tokens.tolist()
    eos = full[4]
    sp = SamplingParams(temperature=0.9, top_k=12, seed=9, max_new_tokens=12, eos_token_id=eos)
    eng.submit(prompt(3, 21), SamplingParams(temperature=0.0, max_new_tokens=6))
    rid = eng.submit(p, sp)
    o = eng.run()[rid]
    toks, _ = hand_driven(p, sp, 2, 1)
    assert o.tokens.tolist() == toks.tolist() == full[: full.index(eos) + 1] and o.finish_reason == "eos"
