#!/usr/bin/env python3
"""Sampled against greedy native decode at the GritLM-7B shape (random weights, 32 layers, random [32000, 4096] lm_head, a cached prefix of
256 tokens, graph replay): ms per decode step for B sequences with the device argmax (greedy), with the reference's HumanEval setting
(scripts/generative_eval.sh: temperature 0.2; top_p 0.95, top_k 0 as its sampling runs are usually paired) and with Hugging Face's
GenerationConfig defaults (temperature 1, top_k 50, top_p 1).  The three modes alternate in one process; ms per step = the slope between
a run of n and a run of 3n new tokens (prompt, cache copy and launch set-up cancel), the median over the repetitions.  bf16 policy: bf16
logits (grit_sample_advance); f16_operands: fp32 logits (grit_sample_advance_f32).  The kernel time of the sampling launch comes from a
separate `rocprofv3 --kernel-trace --stats` run of this script (--modes picks one sampled mode per run).
python tools/sampled_decode_bench.py [--policies bf16,f16_operands --batches 1,20,64 --modes greedy,t02_p095,hf_default --new 16 --reps 3
                                      --out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gritlm_amd.decoder import MistralDecoder  # noqa: E402
from gritlm_amd.encoder import EncoderConfig, MistralEncoderEngine  # noqa: E402

MODES = {"greedy": dict(), "t02_p095": dict(do_sample=True, temperature=0.2, top_k=0, top_p=0.95),
         "hf_default": dict(do_sample=True, temperature=1.0, top_k=50, top_p=1.0)}

ap = argparse.ArgumentParser()
ap.add_argument("--policies", default="bf16,f16_operands")
ap.add_argument("--batches", default="1,20,64")
ap.add_argument("--modes", default=",".join(MODES))
ap.add_argument("--prefix", type=int, default=256)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--new", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--prompt", type=int, default=4)
ap.add_argument("--out", default="")
a = ap.parse_args()
modes = a.modes.split(",")
dev = torch.device("cuda:0")
H, I, V, L = 4096, 14336, 32000, a.layers
cfg = EncoderConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=32, num_key_value_heads=8, vocab_size=V)
eng = MistralEncoderEngine.random_init(cfg, dev, seed=0)
lm_head = (torch.randn((V, H), device=dev) * 0.02).to(torch.bfloat16)
dec = MistralDecoder(eng, lm_head)
g = torch.Generator(device=dev).manual_seed(3)


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
    doc = torch.randint(3, V, (Bmax, a.prefix), generator=g, device=dev)
    kv_all = []
    for c0 in range(0, Bmax, 8):                              # the prefix pass in chunks of 8 sequences (activation memory)
        _, kv = eng.forward(doc[c0:c0 + 8], torch.ones_like(doc[c0:c0 + 8]), return_kv=True, kv_dtype=None)
        kv_all.append(kv)
    kv_full = [(torch.cat([k[li][0] for k in kv_all]), torch.cat([k[li][1] for k in kv_all])) for li in range(L)]
    del kv_all
    q_all = torch.randint(3, V, (Bmax, a.prompt), generator=g, device=dev)
    for B in [int(b) for b in a.batches.split(",")]:
        kv = [(k[:B], v[:B]) for k, v in kv_full]
        q = q_all[:B]
        run = lambda mode, n: dec.generate(q, n, past_key_values=kv, seed=7, **MODES[mode])
        for mode in modes:
            run(mode, 4)                                      # warm-up: fp16 copies, graph-free first launches
        slopes = {m: [] for m in modes}
        for _ in range(a.reps):                               # the modes alternate
            for mode in modes:
                t = {n: timed(lambda: run(mode, n)) for n in (a.new, 3 * a.new)}
                slopes[mode].append((t[3 * a.new] - t[a.new]) / (2 * a.new) * 1e3)
        ms = {m: sorted(s)[len(s) // 2] for m, s in slopes.items()}
        row = dict(policy=pol, logits="fp32" if dec.last_precision == "f16" else "bf16", prefix=a.prefix, batch=B,
                   ms_per_step=ms, ms_per_step_runs=slopes, tokens_per_s={m: B * 1e3 / v for m, v in ms.items()})
        if "greedy" in ms:
            row["sampled_over_greedy"] = {m: ms[m] / ms["greedy"] for m in ms if m != "greedy"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    del kv_full
    torch.cuda.empty_cache()
res = {"metric": "native decode ms per step, sampled against greedy, 7B shape (random weights, graph replay)", "layers": L, "new": a.new,
       "reps": a.reps, "prompt": a.prompt, "modes": {m: MODES[m] for m in modes}, "configs": rows}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
