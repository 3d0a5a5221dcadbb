#!/usr/bin/env python3
"""Time to first token of a prompt on top of a cached prefix at the GritLM-7B shape (random weights): the decoder's "rows" prefill (the
decode kernels over the prompt's rows; the token-by-token loop above 512 rows) against "gemm" (the encoder's MFMA GEMMs +
grit_attn_prefill_cached_*).  A 64-token cache is the reference's query caching (rag/eval.py:200-238: passage + prompt behind the query's
K/V), a 2048-token cache its doc caching.  Both paths alternate in one process after a warm-up; per shape: the median device-event time of
generate(max_new_tokens=1) (cache copy into the decode state + prompt + first logits), the GEMM and prefill-attention kernel time of one
"gemm" run, and 1 - cos of the first logits between the two paths.
python tools/prefill_bench.py [--prompts 16,64,200,512,2048 --caches 64,2048 --reps 3 --out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gritlm_amd import ops  # noqa: E402
from gritlm_amd.decoder import MistralDecoder  # noqa: E402
from gritlm_amd.encoder import EncoderConfig, MistralEncoderEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prompts", default="16,64,200,512,2048")
ap.add_argument("--caches", default="64,2048")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--precision", default="bf16")
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg = EncoderConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.layers, num_attention_heads=32, num_key_value_heads=8, vocab_size=32000)
eng = MistralEncoderEngine.random_init(cfg, dev, seed=0)
eng.set_precision(a.precision)
lm_head = (torch.randn((32000, 4096), device=dev) * 0.02).to(torch.bfloat16)
dec = MistralDecoder(eng, lm_head)
g = torch.Generator(device=dev).manual_seed(3)


def ttft(prompt, kv):
    """(ms, first logits) of one generate(max_new_tokens=1) under the decoder's current prefill"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    _, lg = dec.generate(prompt, 1, past_key_values=kv, return_logits=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), lg[:, 0].double()


rows = []
for S0 in [int(x) for x in a.caches.split(",")]:
    doc = torch.randint(3, 32000, (1, S0), generator=g, device=dev)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True, kv_dtype=None)
    for P in [int(x) for x in a.prompts.split(",")]:
        prompt = torch.randint(3, 32000, (1, P), generator=g, device=dev)
        times, first, path = {"rows": [], "gemm": []}, {}, {}
        for mode in ("rows", "gemm"):                       # warm-up (allocations, fp16 copies, graph-free first launch)
            dec.prefill = mode
            ttft(prompt, kv)
        for _ in range(a.reps):
            for mode in ("rows", "gemm"):
                dec.prefill = mode
                ms, lg = ttft(prompt, kv)
                times[mode].append(ms)
                first[mode], path[mode] = lg, dec.last_prefill
        timer = ops.KernelTimer()                           # kernel classes of one "gemm" run
        ops.set_timer(timer)
        dec.prefill = "gemm"
        ttft(prompt, kv)
        ops.set_timer(None)
        ks = timer.summary()
        gemm_ms = sum(v["total_ms"] for k, v in ks.items() if k.startswith("gemm_"))
        attn_ms = ks.get("attn_prefill_cached", {}).get("total_ms", 0.0)
        a_, b_ = first["rows"], first["gemm"]
        omc = float((1.0 - (a_ * b_).sum(-1) / (a_.norm(dim=-1) * b_.norm(dim=-1))).max())
        med = {m: sorted(t)[len(t) // 2] for m, t in times.items()}
        row = dict(cache=S0, prompt=P, rows_path=path["rows"], rows_ms=med["rows"], gemm_ms=med["gemm"], speedup=med["rows"] / med["gemm"],
                   rows_ms_runs=times["rows"], gemm_ms_runs=times["gemm"], gemm_kernels_ms=gemm_ms, attn_prefill_ms=attn_ms,
                   attn_frac_of_gemm_ttft=attn_ms / med["gemm"], first_logits_1_minus_cos=omc)
        rows.append(row)
        print(json.dumps(row), flush=True)
cross = {}
for S0 in sorted({r["cache"] for r in rows}):
    faster = [r["prompt"] for r in rows if r["cache"] == S0 and r["gemm_ms"] < r["rows_ms"]]
    cross[str(S0)] = min(faster) if faster else None
res = {"metric": "time to first token, prompt on a cached prefix, 7B shape (random weights, 1 sequence)", "precision": a.precision,
       "layers": a.layers, "reps": a.reps, "smallest_measured_prompt_where_gemm_is_faster": cross, "shapes": rows}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
