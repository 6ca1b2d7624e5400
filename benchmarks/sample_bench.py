"""Sampling benchmark: the device sampler (``ops/csrc/sample.hip``, ``sampler="device"``) against the host one.

Two arms, one process, the host arm of the same run being the baseline:

(a) the sampler alone: microseconds per call of ``ops.sample_logits`` against ``generation._sample`` on
    ``[B, 50257]`` bf16 logits (N(0, 4^2)), timed with device events after a warm-up;
(b) end to end: ``DecodeSession.generate`` tokens per second, ``sampler="host"`` against ``"device"`` (one graph
    replay per token, no per-token sync), no EOS.

Grid: batch 1 / 8 / 64 x {greedy, T 0.8, T 0.8 + top-p 0.95, T 0.8 + top-k 50}.  Every cell is timed ``--rounds``
times with the two sides alternating; the figures are the medians, all rounds are printed.  One JSON line per cell.

    python benchmarks/sample_bench.py --model gpt2-small --batch 1 8 64 --prompt 128 --tokens 256
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bpe_transformer.models import DecodeSession, TransformerLM, get_preset  # noqa: E402
from bpe_transformer.models.generation import _sample  # noqa: E402
from bpe_transformer.ops import sampling  # noqa: E402

GRID = [  # (name, temperature, top_k, top_p)
    ("greedy", 0.0, None, None),
    ("T0.8", 0.8, None, None),
    ("T0.8+top_p0.95", 0.8, None, 0.95),
    ("T0.8+top_k50", 0.8, 50, None),
]


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def sampler_arm(B, V, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = (torch.randn(B, V, device="cuda", generator=g) * 4).bfloat16()
    u = torch.rand(B, device="cuda", generator=g)
    for name, T, k, p in GRID:
        dev = lambda: sampling.sample_logits(logits, T, k or 0, 1.0 if p is None else p, u)  # noqa: E731
        host = lambda: _sample(logits, T, p, g, k)  # noqa: E731
        for fn in (dev, host):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        d, h = [], []
        for _ in range(rounds):
            h.append(event_us(host, iters))
            d.append(event_us(dev, iters))
        print(json.dumps({"arm": "sampler", "batch": B, "vocab": V, "case": name,
                          "host_us": round(statistics.median(h), 2), "device_us": round(statistics.median(d), 2),
                          "host_us_rounds": [round(x, 2) for x in h], "device_us_rounds": [round(x, 2) for x in d],
                          "speedup": round(statistics.median(h) / statistics.median(d), 2)}), flush=True)


def generate_s(sess, prompt, tokens, T, k, p, sampler):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = sess.generate(prompt, tokens, temperature=T, top_k=k, top_p=p, sampler=sampler, seed=1,
                        generator=torch.Generator(device="cuda").manual_seed(1) if sampler == "host" else None)
    torch.cuda.synchronize()
    assert out.shape[1] == prompt.shape[1] + tokens
    return time.perf_counter() - t0


def generate_arm(model, cfg, B, prompt_len, tokens, rounds):
    prompt = torch.randint(0, cfg.vocab_size, (B, prompt_len), device="cuda")
    sess = DecodeSession(model, B, max_len=prompt_len + tokens)
    for name, T, k, p in GRID:
        for s in ("host", "device"):  # graph capture and first-use costs outside the timed runs
            generate_s(sess, prompt, 8, T, k, p, s)
        h, d = [], []
        for _ in range(rounds):
            h.append(generate_s(sess, prompt, tokens, T, k, p, "host"))
            d.append(generate_s(sess, prompt, tokens, T, k, p, "device"))
        mh, md = statistics.median(h), statistics.median(d)
        print(json.dumps({"arm": "generate", "batch": B, "prompt": prompt_len, "new_tokens": tokens, "case": name,
                          "host_tok_s": round(B * tokens / mh, 1), "device_tok_s": round(B * tokens / md, 1),
                          "host_ms_per_token": round(mh / tokens * 1e3, 4),
                          "device_ms_per_token": round(md / tokens * 1e3, 4),
                          "host_s_rounds": [round(x, 4) for x in h], "device_s_rounds": [round(x, 4) for x in d],
                          "speedup": round(mh / md, 3)}), flush=True)
    del sess
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window of the sampler arm")
    ap.add_argument("--arms", nargs="+", default=["sampler", "generate"], choices=["sampler", "generate"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sample_bench needs a GPU"
    cfg = get_preset(a.model)
    torch.manual_seed(0)
    with torch.no_grad():
        if "sampler" in a.arms:
            for B in a.batch:
                sampler_arm(B, cfg.vocab_size, a.rounds, a.iters)
        if "generate" in a.arms:
            model = TransformerLM.from_config(cfg, device="cuda", dtype=torch.bfloat16).eval()
            for B in a.batch:
                generate_arm(model, cfg, B, a.prompt, a.tokens, a.rounds)


if __name__ == "__main__":
    main()
