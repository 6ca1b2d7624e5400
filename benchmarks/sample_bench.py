"""Sampling benchmark: the device sampler (``ops/csrc/sample.hip``, ``sampler="device"``) against the host one.

Two arms, one process, the host arm of the same run being the baseline:

(a) the sampler alone: microseconds per call of ``ops.sample_logits`` against ``generation._sample`` on
    ``[B, 50257]`` bf16 logits (N(0, 4^2)), timed with device events after a warm-up;
(b) end to end: ``DecodeSession.generate`` tokens per second, ``sampler="host"`` against ``"device"`` (one graph
    replay per token, no per-token sync), no EOS.

Grid: batch 1 / 8 / 64 x {greedy, T 0.8, T 0.8 + top-p 0.95, T 0.8 + top-k 50}.  Every cell is timed ``--rounds``
times with the two sides alternating; the figures are the medians, all rounds are printed.  One JSON line per cell.

    python benchmarks/sample_bench.py --model gpt2-small --batch 1 8 64 --prompt 128 --tokens 256

``--repetition-penalty`` / ``--presence-penalty`` / ``--frequency-penalty`` / ``--logprobs`` add a third side to arm
(b): the device sampler with those sampling controls (``ops/csrc/logit_process.hip``: two more launches per captured
step), alternating with the other two; ``controls_added_us`` is its step time minus the plain device sampler's.
``--cases`` picks rows of the grid by name.

    python benchmarks/sample_bench.py --arms generate --cases T0.8 --repetition-penalty 1.2 --logprobs
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


def generate_s(sess, prompt, tokens, T, k, p, sampler, controls=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = sess.generate(prompt, tokens, temperature=T, top_k=k, top_p=p, sampler=sampler, seed=1,
                        generator=torch.Generator(device="cuda").manual_seed(1) if sampler == "host" else None,
                        **(controls or {}))
    torch.cuda.synchronize()
    if controls and controls.get("return_logprobs"):
        out = out[0]
    assert out.shape[1] == prompt.shape[1] + tokens
    return time.perf_counter() - t0


def generate_arm(model, cfg, B, prompt_len, tokens, rounds, grid=GRID, controls=None):
    prompt = torch.randint(0, cfg.vocab_size, (B, prompt_len), device="cuda")
    sess = DecodeSession(model, B, max_len=prompt_len + tokens)
    # the controls side has a session of its own (one session would hold both graphs, one per set of switches; two keep
    # the sides' caches and buffers apart, as in the figures recorded so far)
    csess = DecodeSession(model, B, max_len=prompt_len + tokens) if controls else None
    for name, T, k, p in grid:
        for s in ("host", "device"):  # graph capture and first-use costs outside the timed runs
            generate_s(sess, prompt, 8, T, k, p, s)
        if controls:
            generate_s(csess, prompt, 8, T, k, p, "device", controls)
        h, d, c = [], [], []
        for _ in range(rounds):
            h.append(generate_s(sess, prompt, tokens, T, k, p, "host"))
            d.append(generate_s(sess, prompt, tokens, T, k, p, "device"))
            if controls:
                c.append(generate_s(csess, prompt, tokens, T, k, p, "device", controls))
        mh, md = statistics.median(h), statistics.median(d)
        row = {"arm": "generate", "batch": B, "prompt": prompt_len, "new_tokens": tokens, "case": name,
               "host_tok_s": round(B * tokens / mh, 1), "device_tok_s": round(B * tokens / md, 1),
               "host_ms_per_token": round(mh / tokens * 1e3, 4),
               "device_ms_per_token": round(md / tokens * 1e3, 4),
               "host_s_rounds": [round(x, 4) for x in h], "device_s_rounds": [round(x, 4) for x in d],
               "speedup": round(mh / md, 3)}
        if controls:
            mc = statistics.median(c)
            row.update({"controls": {k_: v for k_, v in controls.items()},
                        "controls_ms_per_token": round(mc / tokens * 1e3, 4),
                        "controls_added_us": round((mc - md) / tokens * 1e6, 2),
                        "controls_s_rounds": [round(x, 4) for x in c]})
        print(json.dumps(row), flush=True)
    del sess, csess
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
    ap.add_argument("--cases", nargs="+", default=None, choices=[g[0] for g in GRID], help="rows of the grid (all)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--presence-penalty", type=float, default=0.0)
    ap.add_argument("--frequency-penalty", type=float, default=0.0)
    ap.add_argument("--logprobs", action="store_true", help="return_logprobs=True on the controls side")
    a = ap.parse_args()
    controls = dict(repetition_penalty=a.repetition_penalty, presence_penalty=a.presence_penalty,
                    frequency_penalty=a.frequency_penalty, return_logprobs=a.logprobs)
    if controls == dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, return_logprobs=False):
        controls = None
    grid = [g for g in GRID if a.cases is None or g[0] in a.cases]
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
                generate_arm(model, cfg, B, a.prompt, a.tokens, a.rounds, grid, controls)


if __name__ == "__main__":
    main()
