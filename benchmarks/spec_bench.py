"""Speculative decoding against the plain device-sampler decode loop, same process, same box.

GPT-2-small target (random init), batch 1 and 8, prompt 128, K in {2, 4, 7}, greedy; drafts: (a) ``truncated(2)``,
(b) the target itself (acceptance ~ 1: the ceiling of the accept path), (c) an unrelated random 2-layer model
(acceptance ~ 0: the floor).  Reports ms per round, mean tokens emitted per round and sequence, and the plain
``sampler="device"`` ms per token; from them the break-even tokens per round and acceptance rate per K (a round of
cost ``r`` pays once it emits more than ``r / plain`` tokens; with per-draft acceptance ``a`` a round emits
``(1 - a^(K+1)) / (1 - a)`` tokens).  The weights are random, so acceptance here says nothing about real text.

    python benchmarks/spec_bench.py [--new 96] [--reps 3]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bpe_transformer.models import DecodeSession, SpeculativeSession, TransformerLM, get_preset  # noqa: E402


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=96)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    a = ap.parse_args()
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
