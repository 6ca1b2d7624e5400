"""Serving benchmark: appending ``T`` tokens to a KV cache that already holds some (``models/generation.py``).

A second turn of a conversation, a chunk of a long prompt, a slot that keeps a shared prefix: ``prefill`` on a
filled cache.  Two routes are timed on the same session, alternating, after a warm-up of each:

* ``cache``  -- this tree's route: one pass over the layers, ``kv_append`` + ``cache_attn``
  (``csrc/flash_attn_cache.hip``);
* ``decode`` -- the route before ``cache_attn`` existed: steps of ``8 // G`` tokens, each a pass over the layers
  ending in ``decode_attn``.  It is still in the tree for short windows; raising the routing threshold
  (``generation._CACHE_ATTN_MIN_ROWS``) past ``G * T`` selects it for any window, with the same kernels and host
  loop the parent commit ran.

``--kv-dtype fp8`` times the fp8-cache session instead (``DecodeSession(kv_dtype="fp8")``), whose long windows run on
``cache_attn_fp8`` (the same kernel reading the e4m3 rows and their scales as stored), against the route it replaced:

* ``dequant`` -- ``kv_dequant`` of the layer's valid rows into a one-layer bf16 scratch + the bf16 ``cache_attn``, called
  through the ops on the same cache (``KVView.attend`` is swapped for the timed call), two launches per layer.

``--kv-layout paged`` times the paged session (``DecodeSession(kv_layout="paged")``, of ``--kv-dtype``) against the
slab one on this tree's route, two sessions alternating: the same launches, the cache rows behind a block table.

``--long-cache`` adds the 4-layer Llama-shaped model with 4030 tokens cached (max_len 4096) and windows of 64 and 512.

Every timed call starts from the same cache state (the position is put back, the rows are overwritten with the same
values).  Times are medians of ``--reps`` host-synchronised calls; one JSON line per (configuration, T).

    python benchmarks/append_bench.py --filled 512 --tokens 9 16 64 256 512
    python benchmarks/append_bench.py --kv-dtype fp8 --long-cache
    python benchmarks/append_bench.py --kv-layout paged
"""
import argparse
import json
import math
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
    # the long-cache arm: the Llama-1.1B shape cut to four layers, max_len 4096 (decode_bench.py --long-context)
    "llama-4l": lambda: get_preset("llama-1.1b", num_layers=4, context_length=4096),
}


def build(name):
    cfg = CONFIGS[name]()
    torch.manual_seed(0)
    if isinstance(cfg, dict):
        return TransformerLM(**cfg).to("cuda", torch.bfloat16).eval(), cfg["vocab_size"]
    return TransformerLM.from_config(cfg, device="cuda", dtype=torch.bfloat16).eval(), cfg.vocab_size


_ATTEND = gen.KVView.attend
_SCRATCH = {}


def dequant_attend(self, h, q, li, T, H, kind, combine=True):
    """``KVView.attend`` before ``cache_attn_fp8``: a long window over an fp8 cache is ``kv_dequant`` into a zero-filled
    one-layer bf16 scratch (allocated once per cache) followed by the bf16 ``cache_attn``."""
    if self.scales is None or kind != "cache":
        return _ATTEND(self, h, q, li, T, H, kind, combine)
    k, v, pos = self.k[li], self.v[li], self.pos
    key = id(self.cache)
    if key not in _SCRATCH:
        _SCRATCH.clear()
        _SCRATCH[key] = tuple(torch.zeros(self.cache.k.shape[1:], device=k.device, dtype=torch.bfloat16)
                              for _ in range(2))
    kd, vd = (t[: k.shape[0]] for t in _SCRATCH[key])
    h.kv_dequant(k, v, self.scales[0][li], self.scales[1][li], pos, T, kd, vd)
    return h.cache_attn(q, kd, vd, pos, H, 1.0 / math.sqrt(k.shape[-1]), T)


def timed_append(sess, ids, filled, route):
    """One append of ``ids`` at position ``filled`` on ``route``; -> seconds."""
    sess.cache.pos.fill_(filled)
    sess.cache._len = [filled] * sess.batch
    keep = gen._CACHE_ATTN_MIN_ROWS
    gen._CACHE_ATTN_MIN_ROWS = 1 << 30 if route == "decode" else keep
    gen.KVView.attend = dequant_attend if route == "dequant" else _ATTEND
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.prefill(ids)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    finally:
        gen._CACHE_ATTN_MIN_ROWS = keep
        gen.KVView.attend = _ATTEND


def run_fp8(a, name, B, model, vocab, filled, tokens):
    """fp8 cache: ``cache_attn_fp8`` against ``kv_dequant`` + ``cache_attn``, alternating, ``--reps`` rounds."""
    max_len = 4096 if name == "llama-4l" else filled + max(tokens)
    sess = DecodeSession(model, B, max_len=max_len, kv_dtype="fp8", prefill_chunk=512)
    G = sess.H // sess.Hkv
    ids = torch.randint(0, vocab, (B, filled + max(tokens)), device="cuda")
    routes = ["cache", "dequant"]
    with torch.no_grad():
        sess.prefill(ids[:, :filled])
        sess.prefill_chunk = None
        for T in tokens:
            if G * T < gen._CACHE_ATTN_MIN_ROWS:
                continue
            new = ids[:, filled : filled + T]
            for r in routes:
                timed_append(sess, new, filled, r)
            t = {r: [] for r in routes}
            for _ in range(a.reps):
                for r in routes:
                    t[r].append(timed_append(sess, new, filled, r))
            med = {r: statistics.median(v) for r, v in t.items()}
            print(json.dumps({"config": name, "kv_dtype": "fp8", "batch": B, "G": G, "filled": filled, "T": T,
                              "rounds": a.reps,
                              "cache_attn_fp8_ms": round(med["cache"] * 1e3, 3),
                              "cache_attn_fp8_min_ms": round(min(t["cache"]) * 1e3, 3),
                              "cache_attn_fp8_max_ms": round(max(t["cache"]) * 1e3, 3),
                              "dequant_route_ms": round(med["dequant"] * 1e3, 3),
                              "dequant_route_min_ms": round(min(t["dequant"]) * 1e3, 3),
                              "dequant_route_max_ms": round(max(t["dequant"]) * 1e3, 3),
                              "speedup": round(med["dequant"] / med["cache"], 3)}), flush=True)
    del sess
    _SCRATCH.clear()
    torch.cuda.empty_cache()


def run_paged(a, name, B, model, vocab, filled, tokens):
    """Slab against paged sessions of ``--kv-dtype`` on the session's own route, alternating, ``--reps`` rounds."""
    max_len = 4096 if name == "llama-4l" else filled + max(tokens)
    kw = dict(max_len=max_len, kv_dtype=a.kv_dtype, prefill_chunk=512)
    sess = {"slab": DecodeSession(model, B, **kw), "paged": DecodeSession(model, B, kv_layout="paged", **kw)}
    G = sess["slab"].H // sess["slab"].Hkv
    ids = torch.randint(0, vocab, (B, filled + max(tokens)), device="cuda")
    with torch.no_grad():
        for s in sess.values():
            s.prefill(ids[:, :filled])
            s.prefill_chunk = None
        for T in tokens:
            new = ids[:, filled : filled + T]
            for s in sess.values():
                timed_append(s, new, filled, "cache")
            t = {k: [] for k in sess}
            for _ in range(a.reps):
                for k, s in sess.items():
                    t[k].append(timed_append(s, new, filled, "cache"))
            med = {k: statistics.median(v) for k, v in t.items()}
            print(json.dumps({"config": name, "kv_dtype": a.kv_dtype, "batch": B, "G": G, "filled": filled, "T": T,
                              "rounds": a.reps,
                              "slab_ms_median_min_max": [round(x * 1e3, 3) for x in (med["slab"], min(t["slab"]),
                                                                                     max(t["slab"]))],
                              "paged_ms_median_min_max": [round(x * 1e3, 3) for x in (med["paged"], min(t["paged"]),
                                                                                      max(t["paged"]))],
                              "paged_over_slab": round(med["paged"] / med["slab"], 4),
                              "pages_in_use": sess["paged"].cache.pages_in_use}), flush=True)
    del sess
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["gpt2-small:1", "gpt2-small:8", "llama-2l:1"],
                    help="model:batch pairs")
    ap.add_argument("--filled", type=int, default=512, help="tokens already in the cache")
    ap.add_argument("--tokens", type=int, nargs="+", default=[9, 16, 64, 256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: the fp8-cache session, cache_attn_fp8 against kv_dequant + cache_attn")
    ap.add_argument("--kv-layout", choices=["slab", "paged"], default="slab",
                    help="paged: the paged session against the slab one (of --kv-dtype), alternating")
    ap.add_argument("--long-cache", action="store_true",
                    help="add llama-4l (max_len 4096) with 4030 tokens cached, windows of 64 and 512")
    ap.add_argument("--long-batch", type=int, nargs="+", default=[1, 16], help="batch sizes of the --long-cache arm")
    a = ap.parse_args()
    models = {}
    arms = [(spec, a.filled, a.tokens) for spec in a.configs]
    if a.long_cache:
        arms += [(f"llama-4l:{b}", 4030, [64]) for b in a.long_batch]
        arms += [(f"llama-4l:{b}", 4096 - 512 - 2, [512]) for b in a.long_batch]
    for spec, filled, tokens in arms:
        name, B = spec.split(":")
        B = int(B)
        if name not in models:
            models[name] = build(name)
        model, vocab = models[name]
        if a.kv_layout == "paged":
            run_paged(a, name, B, model, vocab, filled, tokens)
            continue
        if a.kv_dtype == "fp8":
            run_fp8(a, name, B, model, vocab, filled, tokens)
            continue
        a_filled, a_tokens = a.filled, a.tokens
        a.filled, a.tokens = filled, tokens
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
        a.filled, a.tokens = a_filled, a_tokens


if __name__ == "__main__":
    main()
