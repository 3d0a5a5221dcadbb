#!/usr/bin/env python3
"""Sampled decode of n continuations of ONE cached passage at the GritLM-7B shape (random weights, 32 layers, random [32000, 4096]
lm_head), graph replay: generate(do_sample=True, num_return_sequences=n) with share_prefix (one copy of the prefix K/V, the MFMA prefix
attention) against the expanded route (n copies of the cache: what the call does without the flag) in the same process, alternating.
The protocol of tools/batched_decode_bench.py: ms per step = the slope between a run of `new` and a run of 3 `new` tokens (prompt,
cache copies and launch set-up cancel), the median over the repetitions after a warm-up of both routes; peak allocated bytes over one
call of 3 `new` tokens.  Prints ONE JSON line (progress goes to stderr); --out writes it to a file as well.
python tools/shared_prefix_bench.py [--policies bf16,f16_operands --prefixes 256,2048 --ns 20,64 --new 16 --reps 3 --out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gritlm_amd import prefix_ops  # noqa: E402
from gritlm_amd.decoder import MistralDecoder  # noqa: E402
from gritlm_amd.encoder import EncoderConfig, MistralEncoderEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--policies", default="bf16,f16_operands")
ap.add_argument("--prefixes", default="256,2048")
ap.add_argument("--ns", default="20,64")
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
SAMPLING = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.9, seed=7)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


rows = []
for pol in a.policies.split(","):
    eng.set_precision(pol)
    for S0 in [int(x) for x in a.prefixes.split(",")]:
        doc = torch.randint(3, V, (1, S0), generator=g, device=dev)
        _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True, kv_dtype=None)
        kv = [(k.clone(), v.clone()) for k, v in kv]
        q = torch.randint(3, V, (1, a.prompt), generator=g, device=dev)
        for n in [int(x) for x in a.ns.split(",")]:
            run = {share: (lambda m, share=share: dec.generate(q, m, past_key_values=kv, num_return_sequences=n, share_prefix=share, **SAMPLING))
                   for share in (False, True)}
            for share in (False, True):                        # warm-up: fp16 copies, first launches, LDS opt-ins
                run[share](4)
            slopes = {False: [], True: []}
            for _ in range(a.reps):                            # the two routes alternate
                for share in (False, True):
                    t = {m: timed(lambda: run[share](m)) for m in (a.new, 3 * a.new)}
                    slopes[share].append((t[3 * a.new] - t[a.new]) / (2 * a.new) * 1e3)
            ms = {share: sorted(s)[len(s) // 2] for share, s in slopes.items()}
            peaks = {share: peak(lambda: run[share](3 * a.new)) for share in (False, True)}
            row = dict(policy=pol, decode_arithmetic=dec.last_precision, prefix=S0, n=n,
                       expanded_ms_per_step=ms[False], expanded_tokens_per_s=n * 1e3 / ms[False], expanded_ms_per_step_runs=slopes[False],
                       expanded_peak_bytes=peaks[False],
                       shared_ms_per_step=ms[True], shared_tokens_per_s=n * 1e3 / ms[True], shared_ms_per_step_runs=slopes[True],
                       shared_peak_bytes=peaks[True], speedup_tokens_per_s=ms[False] / ms[True])
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del kv
        torch.cuda.empty_cache()
res = {"metric": "sampled decode of n continuations of one cached passage, shared prefix against n expanded copies, ms per step and "
                 "tokens/s at the 7B shape (random weights, graph replay)", "kc": prefix_ops.kc(), "layers": L, "new": a.new, "reps": a.reps,
       "prompt": a.prompt, "configs": rows}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
