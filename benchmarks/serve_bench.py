"""Continuous batching benchmark: the request engine (``models/serving.py``) against static batching.

A fixed seeded trace of ``--requests`` requests (prompts of 16-512 tokens, ``max_new_tokens`` of 16-256, all present
at time 0, one sampling parameter set, no EOS) is served two ways on the same model in one process, alternating:

(a) ``engine``: ``ServingEngine(batch=B)``, slab cache, ``run()`` until the trace is drained;
(b) ``static``: the same requests through ``DecodeSession.generate(sampler="device")`` in arrival-order groups of
    ``B`` -- every group starts together and runs until its longest ``max_new_tokens``.

Tokens per second count each request's own ``max_new_tokens`` on both sides (what a static group generates past a
request's limit is waste).  One JSON line per batch with the medians and every round.

With ``--prefill-tokens N`` a third arm runs beside them, alternating in the same rounds:

(c) ``packed``: the engine with ``prefill_tokens=N`` -- a window's admissions prefilled together, one pass over the
    layers per group of at most ``N`` packed prompt tokens (``DecodeSession.prefill_slots``).

``--attn-micro`` times, with device events, ``cache_attn_packed`` on the trace's first admission group (the first
``--batch`` prompts, cut at ``--prefill-tokens``) against the sum of the per-slot ``cache_attn`` calls on the same
cache, at the model's head geometry.

Both sides replay the same captured step (decode -> ``sample_rows``); ``sample_bench.py`` times it per token.

    python benchmarks/serve_bench.py --model gpt2-small --batch 8 64
    python benchmarks/serve_bench.py --model gpt2-small --batch 8 64 --prefill-tokens 2048 --attn-micro
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bpe_transformer.models import DecodeSession, SamplingParams, ServingEngine, TransformerLM, get_preset  # noqa: E402

T, TOP_K = 0.8, 50


def trace(n, vocab, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(16, 513, (n,), generator=g).tolist()
    news = torch.randint(16, 257, (n,), generator=g).tolist()
    return [(torch.randint(0, vocab, (ln,), generator=g), nw) for ln, nw in zip(lens, news)]


def run_engine(eng, reqs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, (p, new) in enumerate(reqs):
        eng.submit(p, SamplingParams(temperature=T, top_k=TOP_K, seed=i, max_new_tokens=new))
    outs = eng.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert sum(len(o.tokens) for o in outs.values()) == sum(n for _, n in reqs)
    return dt


def run_static(sess, reqs, B):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g0 in range(0, len(reqs), B):
        group = reqs[g0 : g0 + B]
        pad = [group[-1]] * (B - len(group))  # (a short last group: the session has B rows)
        sess.generate([p for p, _ in group + pad], max(n for _, n in group), temperature=T, top_k=TOP_K,
                      sampler="device", seed=g0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def attn_micro(cfg, B, reqs, budget, iters=20):
    """``cache_attn_packed`` on the first admission group against the per-slot ``cache_attn`` calls it replaces: empty
    slots (pos 0), the K / V rows already written, median of ``iters`` device-event timings each."""
    from bpe_transformer.ops import decode as OD

    H, D = cfg.num_heads, cfg.d_model // cfg.num_heads
    Hkv = getattr(cfg, "num_kv_heads", None) or H
    lens, tot = [], 0
    for p, _ in reqs[:B]:
        if lens and tot + p.numel() > budget:
            break
        lens.append(int(p.numel()))
        tot += lens[-1]
    S, Lmax = len(lens), max(lens)
    g = torch.Generator(device="cuda").manual_seed(0)
    k = torch.randn(S, Hkv, Lmax, D, device="cuda", generator=g).bfloat16()
    v = torch.randn(S, Hkv, Lmax, D, device="cuda", generator=g).bfloat16()
    q = torch.randn(tot, H * D, device="cuda", generator=g).bfloat16()
    pos = torch.zeros(S, dtype=torch.int32, device="cuda")
    pk = OD.PackedPrompts(range(S), lens, "cuda")
    parts = [(q[o : o + n], k[i : i + 1], v[i : i + 1], pos[i : i + 1], n) for i, (o, n) in enumerate(zip(pk.offs, lens))]

    def packed():
        return OD.prefill_attention_packed(q, k, v, pos, pk, H)

    def per_slot():
        return [OD.prefill_attention(x, kk, vv, pp, H, n_new=n) for x, kk, vv, pp, n in parts]

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)

    assert torch.equal(packed(), torch.cat(per_slot()))
    print(json.dumps({"arm": "attn_micro", "batch": B, "sequences": S, "packed_tokens": tot, "H": H, "Hkv": Hkv, "D": D,
                      "cache_attn_packed_us": round(timed(packed), 1),
                      "cache_attn_per_slot_sum_us": round(timed(per_slot), 1)}), flush=True)


def serve_arm(model, cfg, B, reqs, rounds, sync_every, prefill_tokens=None):
    max_len = max(p.numel() + n for p, n in reqs)
    eng = ServingEngine(model, batch=B, max_len=max_len, sync_every=sync_every)
    pack = None
    if prefill_tokens is not None:
        pack = ServingEngine(model, batch=B, max_len=max_len, sync_every=sync_every, prefill_tokens=prefill_tokens)
        run_engine(pack, reqs[:B])
    # (a static group needs room for its longest prompt plus its longest continuation, on every row)
    sess = DecodeSession(model, B, max_len=max(p.numel() for p, _ in reqs) + max(n for _, n in reqs), ragged=True)
    run_engine(eng, reqs[:B])  # capture and first-use costs outside the timed runs
    run_static(sess, reqs[:B], B)
    e, s, k = [], [], []
    for _ in range(rounds):
        s.append(run_static(sess, reqs, B))
        e.append(run_engine(eng, reqs))
        if pack is not None:
            k.append(run_engine(pack, reqs))
    useful = sum(n for _, n in reqs)
    me, ms = statistics.median(e), statistics.median(s)
    res = {"arm": "serve", "batch": B, "requests": len(reqs), "useful_tokens": useful,
           "sync_every": sync_every, "engine_tok_s": round(useful / me, 1),
           "static_tok_s": round(useful / ms, 1), "engine_s_rounds": [round(x, 4) for x in e],
           "static_s_rounds": [round(x, 4) for x in s], "speedup": round(ms / me, 3),
           "captures": eng.captures}
    if pack is not None:
        mk = statistics.median(k)
        res.update({"prefill_tokens": prefill_tokens, "packed_tok_s": round(useful / mk, 1),
                    "packed_s_rounds": [round(x, 4) for x in k], "packed_speedup": round(ms / mk, 3),
                    "packed_vs_engine": round(me / mk, 3), "packed_captures": pack.captures})
    print(json.dumps(res), flush=True)
    del eng, sess, pack
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sync-every", type=int, default=8)
    ap.add_argument("--prefill-tokens", type=int, default=None,
                    help="add an engine arm with packed admission (ServingEngine(prefill_tokens=N))")
    ap.add_argument("--attn-micro", action="store_true",
                    help="time cache_attn_packed on the first admission group against the per-slot cache_attn calls")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "serve_bench needs a GPU"
    cfg = get_preset(a.model)
    torch.manual_seed(0)
    reqs = trace(a.requests, cfg.vocab_size)
    with torch.no_grad():
        model = TransformerLM.from_config(cfg, device="cuda", dtype=torch.bfloat16).eval()
        for B in a.batch:
            serve_arm(model, cfg, B, reqs, a.rounds, a.sync_every, a.prefill_tokens)
            if a.attn_micro:
                attn_micro(cfg, B, reqs, a.prefill_tokens or sum(p.numel() for p, _ in reqs))


if __name__ == "__main__":
    main()
