"""Speculative decoding against the plain device-sampler decode loop, same process, same box.

GPT-2-small target (random init), batch 1 and 8, prompt 128, K in {2, 4, 7}, greedy; drafts: (a) ``truncated(2)``,
(b) the target itself (acceptance ~ 1: the ceiling of the accept path), (c) an unrelated random 2-layer model
(acceptance ~ 0: the floor).  Reports ms per round, mean tokens emitted per round and sequence, and the plain
``sampler="device"`` ms per token; from them the break-even tokens per round and acceptance rate per K (a round of
cost ``r`` pays once it emits more than ``r / plain`` tokens; with per-draft acceptance ``a`` a round emits
``(1 - a^(K+1)) / (1 - a)`` tokens).  The weights are random, so acceptance here says nothing about real text.

    python benchmarks/spec_bench.py [--new 96] [--reps 3]

``--lookup N`` measures prompt-lookup drafting (``PromptLookupSession``, n-grams of up to ``N`` tokens, no draft
model) instead, against the same plain loop, the two alternated rep by rep, in two regimes:

* ``repeat``: a history that repeats, so most drafts stand.  The target's ``attn.output_proj`` and ``ffn.w2`` are
  zeroed (the same launches and bytes as any GPT-2-small), which makes its greedy output a walk ``w`` of a token map;
  the prompt is ``w[:prompt - 16]`` followed by ``w[:16]`` again, so the continuation is in the history.
* ``random``: a random prompt on the random-init target, so almost no draft stands: the feature's cost, the ratio
  of a lookup round to a plain decode step.

    python benchmarks/spec_bench.py --lookup 3 [--K 4] [--new 96] [--reps 5]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bpe_transformer.models import (  # noqa: E402
    DecodeSession,
    PromptLookupSession,
    SpeculativeSession,
    TransformerLM,
    get_preset,
)


def _timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def _break_even(K: int, tokens: float) -> float | None:
    """Per-draft acceptance a at which a round emits ``tokens``: (1 - a^(K+1)) / (1 - a) = tokens (bisection)."""
    if tokens <= 1:
        return 0.0
    if tokens >= K + 1:
        return None
    lo, hi = 0.0, 1.0
    for _ in range(60):
        a = 0.5 * (lo + hi)
        lo, hi = (a, hi) if (1 - a ** (K + 1)) / (1 - a) < tokens else (lo, a)
    return round(0.5 * (lo + hi), 3)


def _lookup_main(a) -> None:
    dev = torch.device("cuda")
    cfg = get_preset("gpt2-small")
    torch.manual_seed(0)
    target = TransformerLM.from_config(cfg, device=dev, dtype=torch.bfloat16).eval()
    cyc = TransformerLM.from_config(cfg, device=dev, dtype=torch.bfloat16).eval()
    cyc.load_state_dict(target.state_dict())
    for layer in cyc.layers:
        layer.attn.output_proj.weight.data.zero_()
        layer.ffn.w2.weight.data.zero_()
    rows = []
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        walk = cyc.generate(torch.randint(0, cfg.vocab_size, (B, 1), generator=g).to(dev), a.prompt - 17,
                            temperature=0.0)
        regimes = {"repeat": (cyc, torch.cat([walk, walk[:, :16]], 1)),
                   "random": (target, torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=g).to(dev))}
        for regime, (model, prompt) in regimes.items():
            plain = DecodeSession(model, B, max_len=a.prompt + a.new + 8)
            for K in a.K:
                sess = PromptLookupSession(model, B, K, a.lookup, max_len=a.prompt + a.new + K + 1)
                runs = {
                    "plain": lambda: plain.generate(prompt, a.new, temperature=0.0, sampler="device", seed=1),
                    "plain1": lambda: plain.generate(prompt, 1, temperature=0.0, sampler="device", seed=1),
                    "look1": lambda: sess.generate(prompt, 1, temperature=0.0, seed=1),
                    "look": lambda: sess.generate(prompt, a.new, temperature=0.0, seed=1, sync_every=4),
                }
                for fn in runs.values():  # capture, warm-up
                    fn()
                best = {k: float("inf") for k in runs}
                for _ in range(a.reps):  # alternated: every rep times all four, the long lookup run last
                    for k, fn in runs.items():
                        best[k] = min(best[k], _timed(fn, 1))
                rounds = (int(sess._st["rngs"][0, 1]) - 1) // (K + 1)  # replays, the idle ones before a sync included
                # the prefill and the first token are in both runs of a pair: their difference is the loop alone
                ms_tok = (best["plain"] - best["plain1"]) * 1e3 / (a.new - 1)
                ms_round = (best["look"] - best["look1"]) * 1e3 / rounds
                sess.generate(prompt, a.new, temperature=0.0, seed=1, sync_every=1)
                live = (int(sess._st["rngs"][0, 1]) - 1) // (K + 1)
                tokens = (a.new - 1) / live  # (the slowest sequence's: a lower bound for the others)
                rows.append(dict(regime=regime, batch=B, K=K, n_hi=a.lookup, ms_round=round(ms_round, 4),
                                 tokens_per_round=round(tokens, 3), plain_ms_per_token=round(ms_tok, 4),
                                 lookup_ms_per_token=round(ms_round / tokens, 4),
                                 plain_tokens_per_s=round(B * 1e3 / ms_tok, 1),
                                 lookup_tokens_per_s=round(B * 1e3 * tokens / ms_round, 1),
                                 round_over_plain_step=round(ms_round / ms_tok, 3),
                                 speedup=round(ms_tok * tokens / ms_round, 3)))
                print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"bench": "spec-lookup", "prompt": a.prompt, "new": a.new, "rows": rows}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=96)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--lookup", type=int, default=0, metavar="N",
                    help="measure prompt-lookup drafting with n-grams of up to N tokens instead of draft models")
    ap.add_argument("--K", type=int, nargs="+", default=[4], help="draft tokens per round (--lookup)")
    a = ap.parse_args()
    if a.lookup:
        return _lookup_main(a)
    dev = torch.device("cuda")
    cfg = get_preset("gpt2-small")
    torch.manual_seed(0)
    target = TransformerLM.from_config(cfg, device=dev, dtype=torch.bfloat16).eval()
    torch.manual_seed(1)
    rand_cfg = get_preset("gpt2-small")
    rand_cfg.num_layers = 2
    drafts = {"truncated(2)": target.truncated(2), "target": target,
              "random-2-layer": TransformerLM.from_config(rand_cfg, device=dev, dtype=torch.bfloat16).eval()}
    rows = []
    for B in (1, 8):
        prompt = torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=torch.Generator().manual_seed(B)).to(dev)
        plain = DecodeSession(target, B, max_len=a.prompt + a.new + 8)
        run = lambda: plain.generate(prompt, a.new, temperature=0.0, sampler="device", seed=1)  # noqa: E731
        run()  # capture
        short = lambda: plain.generate(prompt, 1, temperature=0.0, sampler="device", seed=1)  # noqa: E731
        short()
        # the prefill and the first token are in both runs: their difference is the decode loop alone
        ms_tok = (_timed(run, a.reps) - _timed(short, a.reps)) * 1e3 / (a.new - 1)
        for K in (2, 4, 7):
            for name, d in drafts.items():
                sess = SpeculativeSession(target, d, B, K, max_len=a.prompt + a.new + K + 1)
                run = lambda: sess.generate(prompt, a.new, temperature=0.0, seed=1, sync_every=4)  # noqa: E731
                short = lambda: sess.generate(prompt, 1, temperature=0.0, seed=1)  # noqa: E731
                run()
                short()
                t = -_timed(short, a.reps) + _timed(run, a.reps)  # (the long run last: its round counter is read)
                rounds = (int(sess._st["rngs"][0, 1]) - 1) // (K + 1)  # replays, the idle ones before a sync included
                ms_round = t * 1e3 / rounds
                # tokens per round and sequence over the rounds a sequence was active in: sync_every = 1 counts them
                sess.generate(prompt, a.new, temperature=0.0, seed=1, sync_every=1)
                live = (int(sess._st["rngs"][0, 1]) - 1) // (K + 1)
                tokens = (a.new - 1) / live  # (the slowest sequence's: a lower bound for the others)
                need = ms_round / ms_tok
                rows.append(dict(batch=B, K=K, draft=name, ms_round=round(ms_round, 4), tokens_per_round=round(tokens, 3),
                                 plain_ms_per_token=round(ms_tok, 4), spec_ms_per_token=round(ms_round / tokens, 4),
                                 break_even_tokens=round(need, 3), break_even_acceptance=_break_even(K, need)))
                print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"bench": "spec", "prompt": a.prompt, "new": a.new, "rows": rows}))


if __name__ == "__main__":
    main()
