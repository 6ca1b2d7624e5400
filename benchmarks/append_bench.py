"""Serving benchmark: appending ``T`` tokens to a KV cache that already holds some (``models/generation.py``).

A second turn of a conversation, a chunk of a long prompt, a slot that keeps a shared prefix: ``prefill`` on a
filled cache.  Two routes are timed on the same session, alternating, after a warm-up of each:

* ``cache``  -- this tree's route: one pass over the layers, ``kv_append`` + ``cache_attn``
  (``csrc/flash_attn_cache.hip``);
* ``decode`` -- the route before ``cache_attn`` existed: steps of ``8 // G`` tokens, each a pass over the layers
  ending in ``decode_attn``.  It is still in the tree for short windows; raising the routing threshold
  (``generation._CACHE_ATTN_MIN_ROWS``) past ``G * T`` selects it for any window, with the same kernels and host
  loop the parent commit ran.

Every timed call starts from the same cache state (the position is put back, the rows are overwritten with the same
values).  Times are medians of ``--reps`` host-synchronised calls; one JSON line per (configuration, T).

    python benchmarks/append_bench.py --filled 512 --tokens 9 16 64 256 512
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
from bpe_transformer.models import generation as gen  # noqa: E402

CONFIGS = {
    "gpt2-small": lambda: get_preset("gpt2-small"),
    # Llama-shaped, two layers: d 2048, 32 query / 4 KV heads (G = 8, D = 64)
    "llama-2l": lambda: dict(vocab_size=32000, context_length=2048, d_model=2048, num_layers=2, num_heads=32,
                             num_kv_heads=4, d_ff=5632),
}


def build(name):
    cfg = CONFIGS[name]()
    torch.manual_seed(0)
    if isinstance(cfg, dict):
        return TransformerLM(**cfg).to("cuda", torch.bfloat16).eval(), cfg["vocab_size"]
    return TransformerLM.from_config(cfg, device="cuda", dtype=torch.bfloat16).eval(), cfg.vocab_size


def timed_append(sess, ids, filled, route):
    """One append of ``ids`` at position ``filled`` on ``route``; -> seconds."""
    sess.cache.pos.fill_(filled)
    sess.cache._len = [filled] * sess.batch
    keep = gen._CACHE_ATTN_MIN_ROWS
    gen._CACHE_ATTN_MIN_ROWS = keep if route == "cache" else 1 << 30
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.prefill(ids)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    finally:
        gen._CACHE_ATTN_MIN_ROWS = keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["gpt2-small:1", "gpt2-small:8", "llama-2l:1"],
                    help="model:batch pairs")
    ap.add_argument("--filled", type=int, default=512, help="tokens already in the cache")
    ap.add_argument("--tokens", type=int, nargs="+", default=[9, 16, 64, 256, 512])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    models = {}
    for spec in a.configs:
        name, B = spec.split(":")
        B = int(B)
        if name not in models:
            models[name] = build(name)
        model, vocab = models[name]
        sess = DecodeSession(model, B, max_len=a.filled + max(a.tokens))
        G = sess.H // sess.Hkv
        ids = torch.randint(0, vocab, (B, a.filled + max(a.tokens)), device="cuda")
        with torch.no_grad():
            sess.prefill(ids[:, : a.filled])
            for T in a.tokens:
                new = ids[:, a.filled : a.filled + T]
                routes = ["cache", "decode"] if G * T >= gen._CACHE_ATTN_MIN_ROWS else ["decode"]
                for r in routes:  # warm-up: first-use costs of both routes
                    timed_append(sess, new, a.filled, r)
                t = {r: [] for r in routes}
                for _ in range(a.reps):  # alternating
                    for r in routes:
                        t[r].append(timed_append(sess, new, a.filled, r))
                med = {r: statistics.median(v) for r, v in t.items()}
                out = {"config": name, "batch": B, "G": G, "filled": a.filled, "T": T,
                       "decode_route_passes": -(-T // max(1, 8 // G)),
                       "decode_route_ms": round(med["decode"] * 1e3, 3)}
                if "cache" in med:
                    out["cache_route_ms"] = round(med["cache"] * 1e3, 3)
                    out["cache_route_min_ms"] = round(min(t["cache"]) * 1e3, 3)
                    out["decode_route_min_ms"] = round(min(t["decode"]) * 1e3, 3)
                    out["speedup"] = round(med["decode"] / med["cache"], 2)
                print(json.dumps(out), flush=True)
        del sess
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
