#!/usr/bin/env python3
"""Batched greedy decode at the GritLM-7B shape (random weights, 32 layers, random [32000, 4096] lm_head): ms per decode step and tokens/s
in graph replay for B sequences on top of a cached prefix, against the status quo in the same process -- B/8 consecutive generate() calls
of 8 rows, alternating with the batched call.  ms per step = the slope between a run of n and a run of 3n new tokens (prompt, cache copy
and launch set-up cancel); the median over the repetitions.  Bytes per step from the shapes: weights + the K/V every row reads (its mean
cached length over the 3n run) + the step's activation rows; / 8 TB/s = the roofline convention of README / DESIGN.
python tools/batched_decode_bench.py [--policies bf16,f16_operands --prefixes 256,2048 --batches 1,8,16,32,64 --new 16 --reps 3 --out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gritlm_amd.decoder import MistralDecoder  # noqa: E402
from gritlm_amd.encoder import EncoderConfig, MistralEncoderEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--policies", default="bf16,f16_operands")
ap.add_argument("--prefixes", default="256,2048")
ap.add_argument("--batches", default="1,8,16,32,64")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--new", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--prompt", type=int, default=4)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
H, I, V, L, nkv, d = 4096, 14336, 32000, a.layers, 8, 128
cfg = EncoderConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=32, num_key_value_heads=nkv, vocab_size=V)
eng = MistralEncoderEngine.random_init(cfg, dev, seed=0)
lm_head = (torch.randn((V, H), device=dev) * 0.02).to(torch.bfloat16)
dec = MistralDecoder(eng, lm_head)
g = torch.Generator(device=dev).manual_seed(3)
wbytes = (sum(sum(getattr(Lr, k).numel() for k in ("wqkv", "wo", "wgu", "wdown")) for Lr in eng.layers) + lm_head.numel()) * 2


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


rows = []
Bmax = max(int(b) for b in a.batches.split(","))
for pol in a.policies.split(","):
    eng.set_precision(pol)
    for S0 in [int(x) for x in a.prefixes.split(",")]:
        doc = torch.randint(3, V, (Bmax, S0), generator=g, device=dev)
        kv_all = []
        for c0 in range(0, Bmax, 8):                          # the prefix pass in chunks of 8 sequences (activation memory)
            _, kv = eng.forward(doc[c0:c0 + 8], torch.ones_like(doc[c0:c0 + 8]), return_kv=True, kv_dtype=None)
            kv_all.append(kv)
        kv_full = [(torch.cat([k[li][0] for k in kv_all]), torch.cat([k[li][1] for k in kv_all])) for li in range(L)]
        del kv_all
        q_all = torch.randint(3, V, (Bmax, a.prompt), generator=g, device=dev)
        for B in [int(b) for b in a.batches.split(",")]:
            kv = [(k[:B], v[:B]) for k, v in kv_full]
            q = q_all[:B]
            chunks = [(c0, min(c0 + 8, B)) for c0 in range(0, B, 8)] if B > 8 else None
            kv8 = [[(k[c0:c1], v[c0:c1]) for k, v in kv] for c0, c1 in chunks] if chunks else None
            new_run = lambda n: dec.generate(q, n, past_key_values=kv)
            base_run = lambda n: [dec.generate(q[c0:c1], n, past_key_values=kv8[i]) for i, (c0, c1) in enumerate(chunks)]
            new_run(4)                                         # warm-up: fp16 copies, graph-free first launches
            if chunks:
                base_run(4)
            slopes, bslopes = [], []
            for _ in range(a.reps):                            # the two paths alternate
                t = {n: timed(lambda: new_run(n)) for n in (a.new, 3 * a.new)}
                slopes.append((t[3 * a.new] - t[a.new]) / (2 * a.new) * 1e3)
                if chunks:
                    tb = {n: timed(lambda: base_run(n)) for n in (a.new, 3 * a.new)}
                    bslopes.append((tb[3 * a.new] - tb[a.new]) / (2 * a.new) * 1e3)
            ms = sorted(slopes)[len(slopes) // 2]
            Lmean = S0 + a.prompt + 2 * a.new                  # mean cached length over the 3n run
            kvbytes = B * L * 2 * nkv * d * 2 * Lmean
            actbytes = B * L * (2 * H * 2 + (32 + 2 * nkv) * d * 4 + 2 * I * 2 + H * 4) + B * V * 4
            step_bytes = wbytes + kvbytes + actbytes
            row = dict(policy=pol, decode_arithmetic=dec.last_precision, prefix=S0, batch=B, ms_per_step=ms, tokens_per_s=B * 1e3 / ms,
                       ms_per_step_runs=slopes, bytes_per_step=step_bytes, weight_bytes=wbytes, kv_bytes=kvbytes,
                       roofline_ms=step_bytes / 8e12 * 1e3, frac_of_roofline=step_bytes / 8e12 * 1e3 / ms,
                       projections="gemv" if B <= 8 else "decode_gemm")
            if chunks:
                bms = sorted(bslopes)[len(bslopes) // 2]
                row.update(baseline_calls_of_8=len(chunks), baseline_ms_per_step=bms, baseline_tokens_per_s=B * 1e3 / bms,
                           baseline_ms_per_step_runs=bslopes, speedup_tokens_per_s=bms / ms)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del kv_full
        torch.cuda.empty_cache()
res = {"metric": "batched native decode, ms per step and tokens/s at the 7B shape (random weights, graph replay)", "layers": L, "new": a.new,
       "reps": a.reps, "prompt": a.prompt, "hbm_bytes_per_s": 8e12, "configs": rows}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
