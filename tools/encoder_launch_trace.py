#!/usr/bin/env python3
"""The launch sequences of the encoder engine and the training engines, recorded on the CPU: every function of gritlm_amd.ops is replaced
by a recorder (tools/launch_recorder.py) and the REAL MistralEncoderEngine (random weights), MistralTrainEngine (on SyntheticBackbone) and
MixtralTrainEngine (on the installed transformers.MixtralModel) run on small CPU tensors.  Per launch: op name and, per argument by name,
the scalar or (buffer by first appearance, offset, shape, strides, dtype) plus the VALUES of small integer tensors (ids, positions,
cu_seqlens, lens: the batch geometry is computed by real torch code); per call a closing record of what it returned (buffer, offset,
shape, dtype: aliasing) or of the exception it raised.  Identical traces on untouched kernels are identical device work.

    python tools/encoder_launch_trace.py                 # per case: launch count, SHA-256 of the canonical JSON trace
    python tools/encoder_launch_trace.py --json          # the same table as JSON (tests/golden/encoder_launch_trace.json)
    python tools/encoder_launch_trace.py --dump CASE     # the whole trace of one case, to diff two checkouts

Uses only the engines' entry points and documented attributes, so one copy of this file runs on any commit.
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), os.path.dirname(os.path.abspath(__file__))]
from gritlm_amd import _lib  # noqa: E402
from gritlm_amd.encoder import EncoderConfig, MistralEncoderEngine  # noqa: E402
from gritlm_amd.training.engine import MistralTrainEngine, MixtralTrainEngine, SyntheticBackbone  # noqa: E402
from launch_recorder import Recorder, canonical  # noqa: E402

BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
POLICIES = ("bf16", "fp32_residual", "f16_operands", "f16_stream")
NOGRAD = ("bf16", "f16_operands", "f16_stream")
S, VOCAB = 8, 64
HALF = (_lib.EPI_SWIGLU, _lib.EPI_SWIGLU_STACKED, _lib.EPI_SWIGLU_STACKED_SAVE)


def cfg(experts=0):
    return EncoderConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                         vocab_size=VOCAB, num_local_experts=experts)


def batch(kind):
    """(ids, mask) int64 [B,S]: a ragged right-padded batch, an all-valid one, one that is NOT right-padded (left padding and a hole)."""
    mask = {"ragged": [[1] * 8, [1] * 5 + [0] * 3, [1] * 3 + [0] * 5], "full": [[1] * 8, [1] * 8],
            "holes": [[0, 0, 1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 0, 0, 0]]}[kind]
    mask = torch.tensor(mask, dtype=I64)
    ids = (torch.arange(mask.numel(), dtype=I64).view(mask.shape) * 7 + 3) % VOCAB
    return ids * mask, mask


# ---- what the recorder hands back for ops the engines call without ``out``
def _n_out(N, epi):
    return N // 2 if epi in HALF else (2 * N if epi == _lib.EPI_SWIGLU_BWD else N)


def _gemm_nt(a, w, out=None, epilogue=_lib.EPI_STORE, residual=None):
    if out is not None:
        return out
    return torch.zeros((a.shape[0], _n_out(w.shape[0], epilogue)), dtype=F32 if epilogue == _lib.EPI_RESIDUAL_F32 else a.dtype)


def _grouped(a, w, counts, m_total, epilogue=_lib.EPI_STORE, out=None, residual=None, a_rows=None):
    return out if out is not None else torch.zeros((m_total, _n_out(w.shape[1], epilogue)), dtype=a.dtype)


def _route(x, *rest):
    """a valid routing: token t takes experts t % E and (t + 1) % E; rows sorted by expert, stable"""
    T, E = x.shape[0], rest[-1].shape[0]
    t = torch.arange(T)
    experts = torch.stack([t % E, (t + 1) % E], dim=1)
    order = torch.argsort(experts.reshape(-1), stable=True)
    rows = torch.empty((2 * T,), dtype=I64)
    rows[order] = torch.arange(2 * T)
    return (experts.to(I32), torch.full((T, 2), 0.5, dtype=F32), torch.bincount(experts.reshape(-1), minlength=E).to(I32),
            (order // 2).to(I32), rows.view(T, 2).to(I32))


def _transpose(x, out=None):
    if out is not None:
        return out
    R, C = x.shape
    return torch.zeros((C, (R + 7) // 8 * 8), dtype=BF16)[:, :R]


RETURNS = {
    "embed_gather": lambda table, ids, out=None: out if out is not None else torch.zeros((ids.numel(), table.shape[1]), dtype=BF16),
    "rmsnorm": lambda x, w, eps, out=None: out if out is not None else torch.zeros(x.shape, dtype=BF16),
    "gemm_nt": _gemm_nt,
    "gemm_nt_grouped": lambda a, w, counts, m_total, out=None, epilogue=_lib.EPI_STORE, a_rows=None: _grouped(a, w, counts, m_total, epilogue, out),
    "gemm_nt_grouped_epi": _grouped,
    "moe_route": _route,
    "moe_route_f32": _route,
    "moe_combine": lambda y, rows, weights, residual, out=None: out if out is not None else torch.zeros((rows.shape[0], y.shape[1]), dtype=F32 if y.dtype == F16 else BF16),
    "moe_combine_bwd": lambda dout, y, *a: (torch.zeros((2 * dout.shape[0], dout.shape[1]), dtype=BF16), torch.zeros((dout.shape[0], 2), dtype=F32)),
    "moe_router_bwd": lambda x, *a, **k: torch.zeros(x.shape, dtype=BF16),
    "mask_pack": lambda mask: torch.zeros((mask.shape[0], (mask.shape[1] + 63) // 64), dtype=I64),
    "pool_norm": lambda hidden, *a, **k: torch.zeros((hidden.shape[0], hidden.shape[2]), dtype=F32),
    "pool_norm_varlen": lambda hidden, cu, *a, **k: torch.zeros((cu.numel() - 1, hidden.shape[1]), dtype=F32),
    "pool_norm_bwd": lambda y, dy, inv, mask, method, normalize, S, instr_len=None: torch.zeros((y.shape[0], S, y.shape[1]), dtype=BF16),
    "pool_norm_varlen_bwd": lambda y, dy, inv, cu, T, *a, **k: torch.zeros((T, y.shape[1]), dtype=BF16),
    "transpose": _transpose,
    "rmsnorm_bwd": lambda dy, x, w, eps, dw, dres=None, out=None: out if out is not None else torch.zeros_like(x),
    "attn_bidir_bwd": lambda qkv, *a, **k: torch.zeros_like(qkv),
    "attn_bidir_varlen_bwd": lambda qkv, *a, **k: torch.zeros_like(qkv),
    "rope_qk_": lambda qkv, *a, **k: qkv,
    "rope_qk_pos_": lambda qkv, *a, **k: qkv,
    "embed_scatter_add": lambda dh, ids, grad: grad,
    "accum_bf16_from_f32": lambda acc, x: acc,
    "f16_overflow_flag": lambda *a, **k: False,
}


class Trace:
    """One case: a Recorder, and ``call(name, fn)`` that runs an engine entry point and closes it with a record of its result."""

    def __init__(self):
        self.rec = Recorder(RETURNS, values=True)

    def launches(self):
        return sum(not l[0].startswith("call.") for l in self.rec.out)

    def call(self, name, fn, show=lambda r: r):
        n0 = self.launches()
        try:
            r = fn()
        except Exception as e:  # noqa: BLE001  -- a refused combination is a case: its type, and how many launches preceded it
            self.rec.log("call.raised", [name, type(e).__name__, self.launches() - n0], {})
            return None
        self.rec.log("call.returned", [name, show(r)], {})
        return r


def _kv(r):
    return [r[0], [(k, v) for k, v in r[1]]]


def _saved(r):
    """forward() of a training engine: the hidden state and the geometry it hands back"""
    g = r[1].geom
    return [r[0], bool(g.packed), g.T, g.cu, g.pos, g.max_len, bool(g.causal), g.window, r[1].ids]


def encoder(experts=0, seed=0):
    return MistralEncoderEngine.random_init(cfg(experts), "cpu", seed=seed)


def attn_mode(eng, mode):
    eng.causal, eng.window_keys = mode != "bidir", 5 if mode == "window" else 0


# ---- the cases: name -> function(Trace)
def cases():
    m = {}

    def enc_forward(pol, mode, variant, experts=0, direct=False):
        def run(t):
            eng = encoder(experts)
            attn_mode(eng, mode)
            if direct:
                eng.precision = pol
            elif t.call("set_precision", lambda: eng.set_precision(pol), lambda r: None) is None:
                return
            ids, mask = batch("ragged")
            kw, show = {}, (lambda r: r)
            if variant.startswith("return_kv"):
                kw, show = dict(return_kv=True, kv_dtype=BF16 if variant.endswith("bf16") else None), _kv
            elif variant == "inputs_embeds":
                ids, kw = None, dict(inputs_embeds=torch.zeros((3, S, 512), dtype=BF16))
            elif variant == "layer_range":
                kw = dict(layer_range=(1, 2), final_norm=False)
            elif variant == "borrow":
                kw = dict(borrow=True)
            t.call("forward", lambda: eng.forward(ids, mask, **kw), show)
        return run

    for pol in POLICIES:
        for mode in ("bidir", "causal", "window"):
            for variant in ("plain", "borrow", "return_kv_bf16", "return_kv_none", "inputs_embeds", "layer_range"):
                m[f"encoder/forward/{pol}/{mode}/{variant}"] = enc_forward(pol, mode, variant)

    def enc_pooled(pol, packed, kind, mode="bidir", experts=0):
        def run(t):
            eng = encoder(experts).set_precision(pol)
            attn_mode(eng, mode)
            ids, mask = batch(kind)
            t.call("encode_pooled", lambda: eng.encode_pooled(ids, mask, "mean", True, packed=packed))
            t.call("encode_pooled", lambda: eng.encode_pooled(ids, mask, "lasttoken", False, instr_len=torch.ones(ids.shape[0], dtype=I32), packed=packed))
        return run

    for pol in POLICIES:
        for packed in (None, True, False):
            for kind in ("ragged", "full", "holes"):
                m[f"encoder/encode_pooled/{pol}/packed_{packed}/{kind}"] = enc_pooled(pol, packed, kind)
        m[f"encoder/encode_pooled/{pol}/packed_None/ragged/window"] = enc_pooled(pol, None, "ragged", "window")

    def on_cache(pol, final_norm, experts=0, window=0, cache_dtype=None):
        def run(t):
            eng = encoder(experts)
            eng.precision = pol
            eng.causal, eng.window_keys = True, window
            B, P, Lmax = 2, 3, 16
            kdt = cache_dtype or (F16 if pol.startswith("f16") else BF16)
            cache = [(torch.zeros((B, 2, Lmax, 128), dtype=kdt), torch.zeros((B, 2, Lmax, 128), dtype=kdt)) for _ in range(2)]
            lens, plen = torch.tensor([5, 4], dtype=I32), torch.tensor([3, 2], dtype=I32)
            positions = (lens.view(B, 1) + torch.arange(P, dtype=I32)).reshape(-1).contiguous()
            last = torch.arange(B, dtype=I64) * P + plen.to(I64) - 1
            ids = (torch.arange(B * P, dtype=I64).view(B, P) * 5 + 3) % VOCAB
            t.call("forward_on_cache", lambda: eng.forward_on_cache(ids, cache, lens, plen, positions, last, final_norm=final_norm))
        return run

    for pol in POLICIES:
        for fn in (True, False):
            m[f"encoder/forward_on_cache/{pol}/final_norm_{fn}"] = on_cache(pol, fn)
    m["refused/forward_on_cache/window"] = on_cache("bf16", True, window=5)
    m["refused/forward_on_cache/cache_dtype"] = on_cache("bf16", True, cache_dtype=F16)
    m["refused/forward_on_cache/moe"] = on_cache("bf16", True, experts=4)

    def enc_switch(t):
        """two calls with different T, then a policy switch: the workspace is re-allocated"""
        eng = encoder()
        for kind in ("full", "ragged", "full"):
            ids, mask = batch(kind)
            t.call("forward", lambda: eng.forward(ids, mask, borrow=True))
            t.call("encode_pooled", lambda: eng.encode_pooled(ids, mask, "mean", True))
        for pol in ("f16_operands", "f16_stream", "f16_operands", "bf16"):
            eng.set_precision(pol)
            ids, mask = batch("ragged")
            t.call("forward", lambda: eng.forward(ids, mask, borrow=True))
            t.call("encode_pooled", lambda: eng.encode_pooled(ids, mask, "mean", True))
    m["encoder/successive_calls_and_policy_switch"] = enc_switch

    for pol in ("bf16", "f16_operands"):
        m[f"moe/forward/{pol}"] = enc_forward(pol, "bidir", "plain", experts=4)
        m[f"moe/forward/{pol}/return_kv"] = enc_forward(pol, "causal", "return_kv_bf16", experts=4)
        for packed in (None, False):
            m[f"moe/encode_pooled/{pol}/packed_{packed}"] = enc_pooled(pol, packed, "ragged", experts=4)
    for pol in ("fp32_residual", "f16_stream"):
        m[f"refused/moe/set_precision/{pol}"] = enc_forward(pol, "bidir", "plain", experts=4)
        m[f"refused/moe/precision_assigned/{pol}"] = enc_forward(pol, "bidir", "plain", experts=4, direct=True)

    # ---- training engines
    def dense_train():
        c = cfg()
        return MistralTrainEngine(SyntheticBackbone(c, "cpu", seed=1), c, "cpu")

    def mixtral_train():
        from transformers import MixtralConfig, MixtralModel
        torch.manual_seed(0)
        hc = MixtralConfig(vocab_size=VOCAB, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                           num_key_value_heads=2, num_local_experts=4, num_experts_per_tok=2, rms_norm_eps=1e-5, sliding_window=None,
                           max_position_embeddings=64, pad_token_id=0, bos_token_id=1, eos_token_id=2)
        return MixtralTrainEngine(MixtralModel(hc).to(BF16), hc, "cpu")

    def train_forward(make, pol, packed, save, causal, kind="ragged"):
        def run(t):
            eng = make().set_nograd_precision(pol)
            ids, mask = batch(kind)
            t.call("forward", lambda: eng.forward(ids, mask, save=save, packed=packed, causal=causal), _saved)
        return run

    def train_step(make, recompute, packed, pooled=True):
        def run(t):
            eng = make()
            eng.recompute = recompute
            ids, mask = batch("ragged")
            for _ in range(2):                      # (the second chunk of a step accumulates into the same gradient buffers)
                if pooled:
                    r = t.call("forward_pooled", lambda: eng.forward_pooled(ids, mask, "mean", True, save=True, packed=packed), lambda r: r[0])
                    t.call("backward_pooled", lambda: eng.backward_pooled(r[1], torch.zeros((3, 512), dtype=F32)))
                else:
                    r = t.call("forward", lambda: eng.forward(ids, mask, save=True, packed=packed), _saved)
                    t.call("backward", lambda: eng.backward(r[1], torch.zeros(r[0].shape, dtype=BF16)))
        return run

    for name, make in (("train", dense_train), ("mixtral", mixtral_train)):
        for pol in (NOGRAD if name == "train" else ("bf16", "f16_operands")):
            for packed in (False, True):
                for save in (False, True):
                    for causal in ((False, True) if name == "train" else (False,)):
                        m[f"{name}/forward/{pol}/{'packed' if packed else 'padded'}/save_{save}/causal_{causal}"] = \
                            train_forward(make, pol, packed, save, causal)
            m[f"{name}/forward/{pol}/packed_requested_on_holes"] = train_forward(make, pol, True, False, False, kind="holes")
        for recompute in (False, True):
            for packed in (False, True):
                m[f"{name}/forward_backward/recompute_{recompute}/{'packed' if packed else 'padded'}"] = train_step(make, recompute, packed, pooled=False)
            m[f"{name}/forward_backward_pooled/recompute_{recompute}"] = train_step(make, recompute, True)

    def train_pooled(make, pol):
        def run(t):
            eng = make().set_nograd_precision(pol)
            for kind, packed in (("ragged", True), ("ragged", False), ("full", True)):
                ids, mask = batch(kind)
                t.call("forward_pooled", lambda: eng.forward_pooled(ids, mask, "mean", True, packed=packed), lambda r: r[0])
        return run

    def train_update(make, pol, owner):
        def run(t):
            """an in-place parameter update between two fp16 no-grad calls: the weight-copy cache re-converts (new buffers)"""
            eng = make().set_nograd_precision(pol)
            ids, mask = batch("ragged")
            t.call("forward_pooled", lambda: eng.forward_pooled(ids, mask, "mean", True), lambda r: r[0])
            t.call("forward_pooled", lambda: eng.forward_pooled(ids, mask, "mean", True), lambda r: r[0])
            with torch.no_grad():
                owner(eng).mul_(0.5)
                eng.embed.mul_(0.5)
            t.call("forward_pooled", lambda: eng.forward_pooled(ids, mask, "mean", True), lambda r: r[0])
            eng.weights_updated()
            t.call("forward_pooled", lambda: eng.forward_pooled(ids, mask, "mean", True), lambda r: r[0])
        return run

    for pol in NOGRAD:
        m[f"train/forward_pooled/{pol}"] = train_pooled(dense_train, pol)
    for pol in ("f16_operands", "f16_stream"):
        m[f"train/param_update_between_calls/{pol}"] = train_update(dense_train, pol, lambda e: e.backbone.layers[0].mlp.down_proj.weight)
    m["mixtral/forward_pooled/f16_operands"] = train_pooled(mixtral_train, "f16_operands")
    m["mixtral/param_update_between_calls/f16_operands"] = train_update(mixtral_train, "f16_operands", lambda e: e.layers[1].wdown)
    m["refused/mixtral/set_nograd_precision/f16_stream"] = lambda t: t.call("set_nograd_precision", lambda: mixtral_train().set_nograd_precision("f16_stream"))
    return m


def trace(fn):
    t = Trace()
    with t.rec, torch.no_grad():
        torch.cuda.device = lambda d: contextlib.nullcontext()          # (encode_pooled makes its device current: there is none here)
        try:
            fn(t)
        finally:
            torch.cuda.device = _cuda_device
    return t.rec.out, t.launches()


_cuda_device = torch.cuda.device


def table():
    """name -> {"launches", "sha256"} over the case matrix."""
    out = {}
    for name, fn in cases().items():
        tr, n = trace(fn)
        out[name] = {"launches": n, "sha256": hashlib.sha256(canonical(tr).encode()).hexdigest()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", action="store_true", help="print the table as JSON")
    ap.add_argument("--dump", metavar="CASE", help="print the whole trace of one case, one launch per line")
    a = ap.parse_args()
    if a.dump:
        tr, n = trace(cases()[a.dump])
        print(f"# {a.dump}: {n} launches")
        for launch in tr:
            print(canonical(launch))
        return
    t = table()
    if a.json:
        print(json.dumps(t, indent=1, sort_keys=True))
        return
    for name, r in t.items():
        print(f"{name:72s} {r['launches']:4d}  {r['sha256'][:16]}")


if __name__ == "__main__":
    main()
