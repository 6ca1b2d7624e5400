"""Serving benchmark: KV-cache decode throughput / latency (``models/generation.py``).

For each batch size: prefill a prompt, then time ``--tokens`` decode steps (HIP-graph replay by default,
``--no-graph`` for eager launches), and the decode-attention kernel alone at the final cache length (HBM
bandwidth of the K/V read).  ``--recompute`` also times the cache-less baseline (full prefix re-run per token).
``--ragged`` adds the same loop on a ragged session (one cache position per sequence) whose prompt lengths are
spread over ``[prompt / 4, prompt]`` with a fixed seed: ms/step and tok/s beside the uniform figures.
``--kv-dtype fp8`` adds, to every line, the fp8-cache session (``DecodeSession(kv_dtype="fp8")``) against the bf16
one in the same process, alternating over ``--rounds`` rounds (median and min of each), both caches' bytes and the
fp8 attention kernel alone.  ``--long-context`` replaces the model by the regime the fp8 cache is for: a Llama-shaped
model cut to ``--layers`` layers (d 2048, 32 query / 4 KV heads, D 64), ``max_len`` 4096 and a prompt that nearly
fills it (``4096 - tokens - 2``), batch 64 by default.
``--weight-dtype fp8`` adds, in the same alternating way, the fp8-weight session (``DecodeSession(weight_dtype="fp8")``)
against the bf16 one: median, min and max of each over the rounds, the ratio of the medians and both sessions'
projection-weight bytes.
``--kv-layout paged`` adds, in the same alternating way, the paged session (``DecodeSession(kv_layout="paged")``)
against the slab one -- with ``--kv-dtype fp8`` both on the fp8 cache: median, min and max of each, the ratio of the
medians, the pages in use and the paged attention kernel alone through the session's block table.
Random-init weights, synthetic prompts; one JSON line per configuration.

    python benchmarks/decode_bench.py --model gpt2-small --batch 1 8 64 --prompt 128 --tokens 256
    python benchmarks/decode_bench.py --kv-dtype fp8 --long-context --batch 64 --tokens 64
    python benchmarks/decode_bench.py --weight-dtype fp8 --model llama-1.1b --batch 1 8 64
    python benchmarks/decode_bench.py --kv-layout paged --model gpt2-small --batch 1 8 64
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bpe_transformer.models import DecodeSession, TransformerLM, get_preset  # noqa: E402
from bpe_transformer.ops import decode as dec  # noqa: E402


def time_decode(sess, ids, prompt_len, tokens):
    sess.reset()
    sess.prefill(ids[:, :prompt_len])
    nxt = ids[:, prompt_len]
    sess.decode(nxt)  # graph capture / first-use costs outside the timed loop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(tokens):
        sess.decode(nxt)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / tokens


def time_attn(fn, n=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n / 1e3


def fp8_arm(model, sess, ids, prompt, tokens, rounds, graph, chunk):
    """bf16 and fp8 sessions alternating in this process -> the extra fields of the JSON line."""
    B = ids.shape[0]
    f8 = DecodeSession(model, B, max_len=sess.max_len, use_graph=graph, kv_dtype="fp8", prefill_chunk=chunk)
    t = {"bf16": [], "fp8": []}
    for _ in range(rounds):
        t["bf16"].append(time_decode(sess, ids, prompt, tokens))
        t["fp8"].append(time_decode(f8, ids, prompt, tokens))
    L = f8.length
    q = torch.randn(B, f8.H * f8.D, device="cuda", dtype=torch.bfloat16)
    pos = torch.tensor([L - 1], dtype=torch.int32, device="cuda")
    c = f8.cache
    t_attn = time_attn(lambda: dec.decode_attention_fp8(q, c.k[0], c.v[0], c.k_scale[0], c.v_scale[0], pos, f8.H))
    kv_bytes = 2 * B * f8.Hkv * L * (f8.D + 4)
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    return {
        "kv_rounds": rounds,
        "bf16_decode_ms_per_step_median_min": [round(med(t["bf16"]) * 1e3, 4), round(min(t["bf16"]) * 1e3, 4)],
        "fp8_decode_ms_per_step_median_min": [round(med(t["fp8"]) * 1e3, 4), round(min(t["fp8"]) * 1e3, 4)],
        "fp8_over_bf16": round(med(t["fp8"]) / med(t["bf16"]), 4),
        "bf16_cache_bytes": sess.cache.nbytes(), "fp8_cache_bytes": c.nbytes(),
        "fp8_attn_us_per_layer": round(t_attn * 1e6, 2), "fp8_attn_kv_GBps": round(kv_bytes / t_attn / 1e9, 1),
    }


def w8_arm(model, sess, ids, prompt, tokens, rounds, graph, chunk):
    """bf16- and fp8-weight sessions alternating in this process -> the extra fields of the JSON line."""
    B = ids.shape[0]
    w8 = DecodeSession(model, B, max_len=sess.max_len, use_graph=graph, weight_dtype="fp8", prefill_chunk=chunk)
    t = {"bf16": [], "fp8": []}
    for _ in range(rounds):
        t["bf16"].append(time_decode(sess, ids, prompt, tokens))
        t["fp8"].append(time_decode(w8, ids, prompt, tokens))
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    mmm = lambda x: [round(med(x) * 1e3, 4), round(min(x) * 1e3, 4), round(max(x) * 1e3, 4)]  # noqa: E731
    return {
        "w_rounds": rounds,
        "bf16w_decode_ms_per_step_median_min_max": mmm(t["bf16"]),
        "fp8w_decode_ms_per_step_median_min_max": mmm(t["fp8"]),
        "fp8w_over_bf16w": round(med(t["fp8"]) / med(t["bf16"]), 4),
        "bf16_weight_bytes": sess.weight_nbytes(), "fp8_weight_bytes": w8.weight_nbytes(),
    }


def paged_arm(model, sess, ids, prompt, tokens, rounds, graph, chunk, kv_dtype):
    """Slab and paged sessions (of ``kv_dtype``) alternating in this process -> the extra fields of the JSON line."""
    B = ids.shape[0]
    kw = dict(max_len=sess.max_len, use_graph=graph, prefill_chunk=chunk, kv_dtype=kv_dtype)
    slab = sess if kv_dtype == "bf16" else DecodeSession(model, B, **kw)
    pg = DecodeSession(model, B, kv_layout="paged", **kw)
    t = {"slab": [], "paged": []}
    for _ in range(rounds):
        t["slab"].append(time_decode(slab, ids, prompt, tokens))
        t["paged"].append(time_decode(pg, ids, prompt, tokens))
    L, c = pg.length, pg.cache
    q = torch.randn(B, pg.H * pg.D, device="cuda", dtype=torch.bfloat16)
    pos = torch.tensor([L - 1], dtype=torch.int32, device="cuda")
    tail = dict(block_table=c.block_table, max_len=c.max_len)
    if kv_dtype == "fp8":
        fn = lambda: dec.decode_attention_fp8(q, c.k[0], c.v[0], c.k_scale[0], c.v_scale[0], pos, pg.H, **tail)  # noqa: E731
    else:
        fn = lambda: dec.decode_attention(q, c.k[0], c.v[0], pos, pg.H, **tail)  # noqa: E731
    t_attn = time_attn(fn)
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    mmm = lambda x: [round(med(x) * 1e3, 4), round(min(x) * 1e3, 4), round(max(x) * 1e3, 4)]  # noqa: E731
    return {
        "layout_rounds": rounds, "layout_kv_dtype": kv_dtype,
        "slab_decode_ms_per_step_median_min_max": mmm(t["slab"]),
        "paged_decode_ms_per_step_median_min_max": mmm(t["paged"]),
        "paged_over_slab": round(med(t["paged"]) / med(t["slab"]), 4),
        "pages_in_use": c.pages_in_use, "pages": c.num_pages,
        "slab_cache_bytes": slab.cache.nbytes(), "paged_pool_bytes": c.nbytes(),
        "paged_attn_us_per_layer": round(t_attn * 1e6, 2),
    }


def ragged_lengths(batch, prompt):
    """Prompt lengths over [prompt / 4, prompt], fixed seed; the longest is ``prompt`` itself."""
    g = torch.Generator().manual_seed(1234)
    n = torch.randint(max(1, prompt // 4), prompt + 1, (batch,), generator=g).tolist()
    n[0] = prompt
    return n


def time_decode_ragged(sess, ids, lengths, tokens):
    sess.reset()
    sess.prefill(ids[:, : max(lengths)], lengths)
    nxt = ids[:, -1]
    sess.decode(nxt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(tokens):
        sess.decode(nxt)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--recompute", action="store_true")
    ap.add_argument("--ragged", action="store_true",
                    help="also time a ragged session: prompt lengths spread over [prompt/4, prompt]")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: also time the fp8-cache session against the bf16 one, alternating in this process")
    ap.add_argument("--weight-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: also time the fp8-weight session against the bf16 one, alternating in this process")
    ap.add_argument("--kv-layout", choices=["slab", "paged"], default="slab",
                    help="paged: also time the paged session against the slab one, alternating in this process")
    ap.add_argument("--rounds", type=int, default=5,
                    help="alternating rounds of the --kv-dtype fp8 / --weight-dtype fp8 / --kv-layout paged comparisons")
    ap.add_argument("--long-context", action="store_true",
                    help="Llama-shaped model cut to --layers layers, max_len 4096, a prompt that nearly fills it")
    ap.add_argument("--layers", type=int, default=4)
    a = ap.parse_args()
    chunk = None
    if a.long_context:
        a.model, max_len, chunk = f"llama-1.1b[{a.layers} layers]", 4096, 512
        a.prompt = max_len - a.tokens - 2
        cfg = get_preset("llama-1.1b", num_layers=a.layers, context_length=max_len)
    else:
        cfg = get_preset(a.model)
        max_len = a.prompt + a.tokens + 2
    torch.manual_seed(0)
    model = TransformerLM.from_config(cfg, device="cuda", dtype=torch.bfloat16).eval()
    for B in a.batch:
        ids = torch.randint(0, cfg.vocab_size, (B, a.prompt + 1), device="cuda")
        sess = DecodeSession(model, B, max_len=max_len, use_graph=not a.no_graph, prefill_chunk=chunk)
        with torch.no_grad():
            # prefill throughput
            sess.reset()
            sess.prefill(ids[:, : a.prompt])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                sess.reset()
                sess.prefill(ids[:, : a.prompt])
            torch.cuda.synchronize()
            t_pre = (time.perf_counter() - t0) / 3
            t_tok = time_decode(sess, ids, a.prompt, a.tokens)
            # the attention kernel alone at the final length (all layers' worth of K/V bytes per call)
            L = sess.length
            q = torch.randn(B, sess.H * sess.D, device="cuda", dtype=torch.bfloat16)
            pos = torch.tensor([L - 1], dtype=torch.int32, device="cuda")
            kc, vc = sess.cache.k[0], sess.cache.v[0]
            for _ in range(3):
                dec.decode_attention(q, kc, vc, pos, sess.H)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                dec.decode_attention(q, kc, vc, pos, sess.H)
            e1.record()
            torch.cuda.synchronize()
            t_attn = e0.elapsed_time(e1) / 50 / 1e3
            kv_bytes = 2 * B * sess.Hkv * L * sess.D * 2
            out = {
                "model": a.model, "batch": B, "prompt": a.prompt, "decode_tokens": a.tokens,
                "graph": not a.no_graph,
                "prefill_ms": round(t_pre * 1e3, 3),
                "prefill_tok_s": round(B * a.prompt / t_pre, 1),
                "decode_ms_per_step": round(t_tok * 1e3, 4),
                "decode_tok_s": round(B / t_tok, 1),
                "attn_us_per_layer": round(t_attn * 1e6, 2),
                "attn_kv_GBps": round(kv_bytes / t_attn / 1e9, 1),
                "cache_len": L,
            }
            if a.kv_dtype == "fp8":
                out.update(fp8_arm(model, sess, ids, a.prompt, a.tokens, a.rounds, not a.no_graph, chunk))
            if a.weight_dtype == "fp8":
                out.update(w8_arm(model, sess, ids, a.prompt, a.tokens, a.rounds, not a.no_graph, chunk))
            if a.kv_layout == "paged":
                out.update(paged_arm(model, sess, ids, a.prompt, a.tokens, a.rounds, not a.no_graph, chunk, a.kv_dtype))
            if a.ragged:
                lengths = ragged_lengths(B, a.prompt)
                rs = DecodeSession(model, B, max_len=max_len, use_graph=not a.no_graph, ragged=True)
                t_rag = time_decode_ragged(rs, ids, lengths, a.tokens)
                out["ragged_prompt_min_mean_max"] = [min(lengths), round(sum(lengths) / B, 1), max(lengths)]
                out["ragged_decode_ms_per_step"] = round(t_rag * 1e3, 4)
                out["ragged_decode_tok_s"] = round(B / t_rag, 1)
                del rs
            if a.recompute:
                n = 16
                ctx = ids[:, : a.prompt]
                model(ctx)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    model(ctx)[:, -1].argmax(-1)
                torch.cuda.synchronize()
                out["recompute_ms_per_token"] = round((time.perf_counter() - t0) / n * 1e3, 3)
        print(json.dumps(out), flush=True)
        del sess
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
