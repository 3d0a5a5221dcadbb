#!/usr/bin/env python3
"""The launch sequence of MistralDecoder.generate(), recorded on the CPU: every function of gritlm_amd.ops is replaced by a recorder and
the engine by a stand-in that holds small CPU tensors, so generate() (use_graph = False) runs to the end without a device and leaves the
exact list of launches -- op name, and for every argument of the op (by name, defaults filled in) the scalar or (buffer by order of first appearance, storage offset, shape,
strides, dtype).  Identical traces on untouched kernels are identical device work: the guard of a decoder refactor.

    python tools/decode_launch_trace.py                 # per case: launch count, prompt path, SHA-256 of the canonical JSON trace
    python tools/decode_launch_trace.py --json          # the same table as JSON (tests/golden/decode_launch_trace.json)
    python tools/decode_launch_trace.py --dump CASE     # the whole trace of one case, to diff two checkouts

Uses only the decoder's public surface (MistralDecoder, generate, its documented attributes), so one copy of this file runs on any commit.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), os.path.dirname(os.path.abspath(__file__))]
from gritlm_amd.decoder import MistralDecoder  # noqa: E402
from launch_recorder import Recorder, canonical  # noqa: E402

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
FUSE = ("deferred", "deferred_mlp", "all", "qkv", "none")
S0, P, NEW = 5, 3, 3            # cached prefix tokens, prompt tokens on top of them, generated tokens


class _Cfg:
    num_attention_heads, num_key_value_heads, head_dim = 4, 2, 128
    hidden_size, intermediate_size, num_hidden_layers = 512, 1024, 2
    rms_norm_eps, rope_theta, vocab = 1e-5, 1e4, 64


class _Layer:
    pass


class _Engine:
    """What MistralDecoder reads of a MistralEncoderEngine: config, zero weights, the fp16 copies, and forward / forward_on_cache that
    record the policy (precision, causal) they were called under."""

    def __init__(self, experts, precision, log):
        c = _Cfg()
        c.num_local_experts = experts
        self.cfg, self.device, self.precision, self.log = c, torch.device("cpu"), precision, log
        self.window_keys, self.rope_bf16, self.causal = 0, True, False
        z = lambda *s: torch.zeros(s, dtype=BF16)
        H, I, qkv = c.hidden_size, c.intermediate_size, (c.num_attention_heads + 2 * c.num_key_value_heads) * c.head_dim
        self.embed, self.norm = z(c.vocab, H), z(H)
        self.layers = []
        for _ in range(c.num_hidden_layers):
            l = _Layer()
            l.wqkv, l.wo, l.wgu, l.wdown = z(qkv, H), z(H, c.num_attention_heads * c.head_dim), z(2 * I, H), z(H, I)
            l.ln1, l.ln2 = z(H), z(H)
            if experts:
                l.wgate, l.w13, l.w2 = z(experts, H), z(experts, 2 * I, H), z(experts, H, I)
            self.layers.append(l)

    def _f16_weights(self, l):
        if not hasattr(l, "_h16"):
            src = (l.wqkv, l.wo, l.w13, l.w2) if self.cfg.num_local_experts else (l.wqkv, l.wo, l.wgu, l.wdown)
            l._h16 = tuple(w.to(F16) for w in src)
        return l._h16

    def _wide(self):
        return F32 if self.precision.startswith("f16") else BF16

    def forward(self, ids, mask, **kw):
        c = self.cfg
        self.log("engine.forward", [ids, mask], dict(kw, precision=self.precision, causal=self.causal))
        B, T = ids.shape
        kdt = kw.get("kv_dtype") or F16
        kv = [(torch.zeros((B, c.num_key_value_heads, T, c.head_dim), dtype=kdt), torch.zeros((B, c.num_key_value_heads, T, c.head_dim), dtype=kdt))
              for _ in range(c.num_hidden_layers)]
        return torch.zeros((B, T, c.hidden_size), dtype=self._wide()), kv

    def forward_on_cache(self, ids, cache, lens, plen, pos, last, **kw):
        flat = [t for kv in cache for t in kv]
        self.log("engine.forward_on_cache", [ids, *flat, lens, plen, pos, last], dict(kw, precision=self.precision, causal=self.causal))
        return torch.zeros((ids.shape[0], self.cfg.hidden_size), dtype=self._wide())


def trace(fuse="deferred", B=1, f16=False, experts=0, engine="bf16", cached=True, prefill="rows", attrs=None, gen=None):
    """(launch list, last_prefill) of one generate() call.  ``engine``: the stand-in engine's policy (the decoder is pinned to bf16 / f16 by
    ``f16``); ``cached``: the prompt rides on a cached prefix of S0 tokens; ``attrs``: decoder attributes to set; ``gen``: generate() keywords."""
    with Recorder({"attn_decode_workspace": lambda *a, **k: torch.zeros(8), "f16_overflow_flag": lambda *a, **k: False}) as r:
        out, log = r.out, r.log
        eng = _Engine(experts, engine, log)
        c = eng.cfg
        dec = MistralDecoder(eng, torch.zeros((c.vocab, c.hidden_size), dtype=BF16))
        dec.use_graph, dec.fuse_norm, dec.precision, dec.prefill = False, fuse, "f16" if f16 else "bf16", prefill
        dec.prompt_chunk, dec.prompt_chunk_max_rows, dec.on_overflow = not experts, 512, "raise"       # (whatever the environment says)
        for k, v in (attrs or {}).items():
            setattr(dec, k, v)
        kdt = F16 if f16 else BF16
        kv = lambda: torch.zeros((B, c.num_key_value_heads, S0, c.head_dim), dtype=kdt)
        past = [(kv(), kv()) for _ in range(c.num_hidden_layers)] if cached else None
        dec.generate(torch.zeros((B, P), dtype=torch.int64), NEW, past_key_values=past, **(gen or {}))
        log("engine.after", [], dict(precision=eng.precision, causal=eng.causal))          # (the policy generate() leaves behind)
        return out, dec.last_prefill


def cases():
    """name -> trace() keywords: the fixed case matrix."""
    m = {}
    for fuse in FUSE:
        for B in (1, 2, 3, 8, 9, 64):
            for f16 in (False, True):
                m[f"dense/{fuse}/B{B}/{'f16' if f16 else 'bf16'}"] = dict(fuse=fuse, B=B, f16=f16)
    for B in (1, 8):
        for f16 in (False, True):
            m[f"moe/B{B}/{'f16' if f16 else 'bf16'}"] = dict(B=B, f16=f16, experts=4)
    for f16 in (False, True):
        p = "f16" if f16 else "bf16"
        other = "bf16" if f16 else "f16_operands"          # the engine on the other arithmetic than its decoder
        for B in (3, 9):
            m[f"no_chunk/B{B}/{p}"] = dict(B=B, f16=f16, attrs={"prompt_chunk": False})
            m[f"chunk_too_large/B{B}/{p}"] = dict(B=B, f16=f16, attrs={"prompt_chunk_max_rows": B * P - 1})
            m[f"sample/B{B}/{p}"] = dict(B=B, f16=f16, gen=dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=11))
            m[f"return_logits/B{B}/{p}"] = dict(B=B, f16=f16, gen=dict(return_logits=True))
            m[f"no_past/B{B}/{p}/engine_{other}"] = dict(B=B, f16=f16, engine=other, cached=False)
            m[f"prefill_gemm/B{B}/{p}/engine_{other}"] = dict(B=B, f16=f16, engine=other, prefill="gemm")
        m[f"sample_return_logits_n2/B2/{p}"] = dict(B=2, f16=f16, gen=dict(do_sample=True, seed=3, num_return_sequences=2, return_logits=True))
        m[f"no_past/B3/{p}/engine_same"] = dict(B=3, f16=f16, engine="f16_operands" if f16 else "bf16", cached=False)
        m[f"prefill_gemm/B3/{p}/engine_same"] = dict(B=3, f16=f16, engine="f16_operands" if f16 else "bf16", prefill="gemm")
    m["moe/sample/B2/bf16"] = dict(B=2, experts=4, gen=dict(do_sample=True, seed=5))
    return m


def launches(tr) -> int:
    return sum(not l[0].startswith("engine.") for l in tr)           # (the stand-in engine's own records are not launches)


def table():
    """name -> {"launches", "prefill", "sha256"} over the case matrix."""
    t = {}
    for name, kw in cases().items():
        tr, prefill = trace(**kw)
        t[name] = {"launches": launches(tr), "prefill": prefill, "sha256": hashlib.sha256(canonical(tr).encode()).hexdigest()}
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", action="store_true", help="print the table as JSON")
    ap.add_argument("--dump", metavar="CASE", help="print the whole trace of one case, one launch per line")
    a = ap.parse_args()
    if a.dump:
        tr, prefill = trace(**cases()[a.dump])
        print(f"# {a.dump}: {launches(tr)} launches, prompt path {prefill}")
        for launch in tr:
            print(canonical(launch))
        return
    t = table()
    if a.json:
        print(json.dumps(t, indent=1, sort_keys=True))
        return
    for name, r in t.items():
        print(f"{name:48s} {r['launches']:4d}  {r['prefill']:8s} {r['sha256'][:16]}")


if __name__ == "__main__":
    main()
