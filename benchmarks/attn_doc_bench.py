"""Document-masked flash attention microbenchmark: forward + backward of ``ops.flash_attention_qkv`` on random data
at the GPT-2 (B 128, S 1024, 12 heads, D 64) and Llama (B 16, S 4096, 32:4, D 64) training shapes, three arms:

  plain    plain causal attention (the default kernels: v8 forward, dq16 / split backward);
  doc1     the document path with one document per row (doc_start = 0, doc_end = S): the general forward and the
           32-row split backward doing the plain causal work -- their cost against v8 / dq16;
  doc4     the document path with every row cut into four equal documents of S / 4: about a quarter of the score
           work of the plain arm, so it must come out faster than ``plain`` if tile skipping works.

Every arm goes through the public op with RoPE tables, so each pays the same rotated copy of the QKV activation
(``rope_qk_``).  The arms alternate inside every round; each round times ``--iters`` forward+backward calls per arm
between two device events after one untimed call; the table reports the median and the minimum over ``--rounds``.

    python benchmarks/attn_doc_bench.py                      # both shapes -> profiles/bench/attn_doc_mask.log
    python benchmarks/attn_doc_bench.py --shapes gpt2 --log ''
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bpe_transformer import ops  # noqa: E402
from bpe_transformer.ops import reference as R  # noqa: E402

SHAPES = {"gpt2": (128, 1024, 12, 12, 64), "llama": (16, 4096, 32, 4, 64)}  # B, S, H, Hkv, D
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def equal_docs(B: int, S: int, n: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """Bounds of rows cut into ``n`` equal documents, through ``ops.doc_bounds`` (a separator ends each one)."""
    ids = torch.ones(B, S, dtype=torch.long, device=device)
    ids[:, S // n - 1 :: S // n] = 0
    return ops.doc_bounds(ids, 0)


def score_work(start: torch.Tensor) -> float:
    """(query, key) pairs the mask keeps, summed over the batch."""
    idx = torch.arange(start.shape[1], device=start.device)
    return float((idx[None] - start + 1).sum())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["gpt2", "llama"], choices=sorted(SHAPES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "bench", "attn_doc_mask.log"),
                    help="also append the result lines to this file ('' = stdout only)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("attn_doc_bench: no GPU (a timing needs the device; nothing measured)", file=sys.stderr)
        return 1
    dev = torch.device("cuda")
    lines = []
    for name in a.shapes:
        B, S, H, Hkv, D = SHAPES[name]
        torch.manual_seed(0)
        qkv = torch.randn(B * S, (H + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, requires_grad=True)
        do = torch.randn(B * S, H * D, device=dev, dtype=torch.bfloat16)
        cos, sin = R.rope_tables(D, S, 10000.0, device=dev)
        arms = {"plain": None, "doc1": equal_docs(B, S, 1, dev), "doc4": equal_docs(B, S, 4, dev)}
        full = float(B) * S * (S + 1) / 2
        work = {k: (full if v is None else score_work(v[0])) / full for k, v in arms.items()}

        def step(doc):
            qkv.grad = None
            o = ops.flash_attention_qkv(qkv, B, S, H, Hkv, D, cos, sin, True, doc_bounds=doc)
            o.backward(do)

        for _ in range(a.warmup):
            for doc in arms.values():
                step(doc)
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(a.rounds):
            for k, doc in arms.items():  # the arms alternate inside a round
                step(doc)
                ev[0].record()
                for _ in range(a.iters):
                    step(doc)
                ev[1].record()
                torch.cuda.synchronize()
                times[k].append(ev[0].elapsed_time(ev[1]) / a.iters)
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        for k, t in times.items():
            lines.append(json.dumps({"shape": name, "B_S_H_Hkv_D": [B, S, H, Hkv, D], "arm": k,
                                     "score_work_vs_plain": round(work[k], 4),
                                     "fwd_bwd_ms_median": round(med[k], 4), "fwd_bwd_ms_min": round(min(t), 4),
                                     "fwd_bwd_ms_max": round(max(t), 4),
                                     "time_vs_plain": round(med[k] / med["plain"], 4)}))
            print(lines[-1], flush=True)
        ok = med["doc4"] < med["plain"]
        lines.append(json.dumps({"shape": name, "doc4_faster_than_plain": ok}))
        print(lines[-1], flush=True)
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(f"# benchmarks/attn_doc_bench.py --iters {a.iters} --rounds {a.rounds} --warmup {a.warmup}: forward"
                    f" + backward of flash_attention_qkv, {torch.cuda.get_device_name(0)}\n")
            f.write("\n".join(lines) + "\n")
    return 0 if all('"doc4_faster_than_plain": false' not in ln for ln in lines) else 2


if __name__ == "__main__":
    sys.exit(main())
