"""Native greedy generation on the encoder engine's weights: prompt prefill + token-by-token decode on HIP kernels.

Replaces, for the RAG doc-caching flow of the reference (rag/eval.py:237-302: ``model.generate(inputs, past_key_values=kv_cache)`` where
``kv_cache`` came from ``encode(..., get_cache=True)``, gritlm/gritlm.py:131-140), the Hugging Face decode loop: every projection of a
decode step is an HBM-bound GEMV (``grit_gemv_bf16``), attention reads the sequence's KV once (``grit_attn_decode``), the new token's
K/V are appended in place, sampling is a device-side argmax -- and the whole step (5 launches per layer) is captured in ONE HIP
graph, so the host only replays it.  Greedy by default; ``do_sample=True`` draws each token with temperature / top-k / top-p on the device
(``grit_sample_advance``: one launch in place of the argmax, the step is still one graph).  head_dim 128.

Batch: 1 to 64 sequences (sparse-MoE engines: 1 to 8).  At 1..8 rows every projection of a step is the GEMV above; at 9..64 rows it is
the MFMA decode GEMM (``grit_decode_gemm_*`` / ``grit_rmsnorm_decode_gemm_*_deferred``: every weight element read once per step whatever
the row count), the other kernels of the step are the same, and the step is still one graph.  The seam at 8 | 9: a row decoded in a batch
of 8 and the same row in a batch of 9 differ in the last bits (GEMV against MFMA summation order, and the deferred norm's operand
x * ln_w is rounded once to the 16-bit operand format on the MFMA); within 9..64 a row's bits do not depend on the batch.

Precision (round 6): the decoder follows its engine's policy.  Under ``"bf16"`` / ``"fp32_residual"`` the step is the reference's bf16
arithmetic (teacher-forced logits within ~1e-3 (1 - cos) of the fp32 module: the bf16 level).  Under ``"f16_operands"`` / ``"f16_stream"`` it
runs on the engine's fp16 weight copies around an fp32 residual stream (``grit_gemv_f16`` ...; formats in include/gritlm_hip.h): the
continuation of ``encode(get_cache=True)`` at the north-star's own level (fp16 K/V: same bytes per token as bf16).
"""
from __future__ import annotations

import collections
import contextlib
import math
import numbers

import torch

from . import ops, prefix_ops
from ._lib import EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU
from ._lib import GritHipError
from .encoder import F16_POLICIES, MistralEncoderEngine, rope_tables

BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64


PREFILL_MODES = ("rows", "gemm")
GEMV_ROWS = 8           # up to this many rows a step's projections are GEMVs (grit_gemv_*); above, the MFMA decode GEMMs
MAX_ROWS = 64           # the batch limit of the dense decoder (grit_decode_gemm_*: 1..64 rows)


def check_sampling(temperature, top_k, top_p, num_return_sequences, do_sample: bool = True):
    """The sampling parameters of generate(), refused before anything runs: T > 0 and finite, integer top_k >= 0, 0 <= top_p <= 1, integer
    num_return_sequences >= 1 (above 1 only when sampling: greedy copies of a prompt would be identical, and Hugging Face refuses them)."""
    if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, numbers.Integral) or num_return_sequences < 1:
        raise ValueError(f"num_return_sequences={num_return_sequences!r}: an integer >= 1")
    if not do_sample:
        if num_return_sequences != 1:
            raise ValueError("num_return_sequences > 1 needs do_sample=True")
        return
    if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or top_k < 0:
        raise ValueError(f"top_k={top_k!r}: an integer >= 0 (0: no top-k filter)")
    if not (isinstance(temperature, numbers.Real) and math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature={temperature!r}: a finite number > 0")
    if not (isinstance(top_p, numbers.Real) and 0.0 <= top_p <= 1.0):
        raise ValueError(f"top_p={top_p!r}: a number in [0, 1]")


def row_keys(seed: int, rows: int, device) -> torch.Tensor:
    """The RNG keys of a call's rows: key_r = seed + r (mod 2^64), as the int64 bit patterns grit_sample_advance reads as uint64."""
    ks = [(int(seed) + r) % 2 ** 64 for r in range(rows)]
    return torch.tensor([k - 2 ** 64 if k >= 2 ** 63 else k for k in ks], dtype=I64, device=device)


def draw_seed() -> int:
    """A 64-bit seed from torch's default CPU generator (torch.manual_seed / transformers.set_seed reproduce it)."""
    lo, hi = (int(x) for x in torch.randint(0, 2 ** 32, (2,), dtype=torch.int64))
    return (hi << 32) | lo


# What a pass over the layers launches is a small table, resolved once per call by MistralDecoder._plan.
# The three forms of a norm site (input_layernorm -> q|k|v; post_attention_layernorm -> gate|up; final norm -> lm_head), _norm_proj:
DEFERRED = "deferred"           # the row scale multiplies the finished dot products: x_n is not rounded (one rounding fewer than the reference)
EXACT = "exact fused"           # the reference's two roundings inside the GEMV; above 8 rows the norm's own launch in front of the MFMA GEMM
OWN = "own launch"              # rmsnorm, then the plain projection
# The forms of a bf16 dense step by fuse_norm (any other value: as "qkv"); fp16 operands and sparse-MoE steps: DEFERRED, DEFERRED always.
NORM_FORMS = {                  # q|k|v site, MLP and final sites
    "deferred":     (DEFERRED, DEFERRED),
    "deferred_mlp": (EXACT,    DEFERRED),
    "all":          (EXACT,    EXACT),        # 3+ rows: OWN, OWN (_plan)
    "qkv":          (EXACT,    OWN),          # 3+ rows: OWN, OWN
    "none":         (OWN,      OWN),
}
# attn: "rope" (grit_attn_decode_rope: RoPE + K/V append + attention in one launch, behind every fused q|k|v site), "append"
# (grit_rope_kv_append + grit_attn_decode, behind a q|k|v norm with its own launch), for a prompt chunk "rows" (grit_rope_kv_append_rows +
# grit_attn_decode_rows over all rows) or, for the n rows per sequence of share_prefix, "prefix" (the four launches of prefix_ops: every row
# attends to its sequence's one prefix copy and to its own tail).  groups: the row ranges (a, b) a projection runs over, [None] for the whole batch.
Plan = collections.namedtuple("Plan", "qkv_norm mlp_norm attn groups")


def _proj(x: torch.Tensor, w: torch.Tensor, **kw):
    """x @ w^T of a decode step (epilogues of ops.gemv): the GEMV at 1..8 rows, the MFMA decode GEMM at 9..64."""
    return (ops.gemv if x.shape[0] <= GEMV_ROWS else ops.decode_gemm)(x, w, **kw)


def _norm_proj(form: str, x: torch.Tensor, ln_w: torch.Tensor, eps: float, w: torch.Tensor, out: torch.Tensor, xn: torch.Tensor | None,
               epilogue: int = EPI_STORE):
    """One norm site: RMSNorm + projection in the given form, at 1..8 rows on the GEMVs and at 9..64 on the MFMA decode GEMMs (``xn``: where
    a norm with its own launch writes its rows)."""
    gemv = x.shape[0] <= GEMV_ROWS
    if form == OWN or (form == EXACT and not gemv):
        ops.rmsnorm(x, ln_w, eps, out=xn)
        return _proj(xn, w, out=out, epilogue=epilogue)
    if gemv:
        return ops.rmsnorm_gemv(x, ln_w, eps, w, out=out, epilogue=epilogue, deferred=form == DEFERRED)
    return ops.rmsnorm_decode_gemm(x, ln_w, eps, w, out=out, epilogue=epilogue)


def _cut(t, g):
    """rows g = (a, b) of a buffer; the whole of it for g = None (a step), None for no buffer"""
    return t if g is None or t is None else t[g[0]:g[1]]


def prefill_layout(attention_mask: torch.Tensor, lens: torch.Tensor, Lmax: int | None = None):
    """The geometry of a right-padded prompt chunk on top of cached prefixes (pure tensor arithmetic, any device): ``attention_mask`` [B,P]
    over the chunk's tokens, ``lens`` [B] the cached prefix length of every row.  Returns (plen int32 [B]: valid tokens per row;
    positions int32 [B*P]: lens[b] + i of every chunk row, padding rows included, clamped below ``Lmax``; last int64 [B]: the flattened row
    b*P + plen[b] - 1 of every row's last valid token).  A mask that is not right-padded (left padding, holes) or a row without a token
    raises NotImplementedError."""
    m = attention_mask != 0
    B, P = m.shape
    plen = m.sum(dim=1)
    ar = torch.arange(P, device=m.device).view(1, P)
    if not bool(((ar < plen.view(B, 1)) == m).all()):
        raise NotImplementedError("native decode: prompt rows on top of past_key_values must be right-padded (a mask of 1 ... 1 0 ... 0 per row)")
    if not bool((plen > 0).all()):
        raise NotImplementedError("native decode: every prompt row on top of past_key_values needs at least one token")
    lens = lens.to(device=m.device, dtype=torch.int64).view(B, 1)
    positions = lens + ar
    if Lmax is not None:
        positions = positions.clamp(max=Lmax - 1)
    last = torch.arange(B, device=m.device, dtype=torch.int64) * P + plen.to(torch.int64) - 1
    return plen.to(I32), positions.reshape(B * P).to(I32), last


def _layers_of(cache):
    """per-layer (k, v) [B, nkv, S, d] from the installed transformers' cache object or a legacy tuple of tuples."""
    if hasattr(cache, "layers"):
        return [(l.keys, l.values) for l in cache.layers]
    return [(l[0], l[1]) for l in cache]


class MistralDecoder:
    def __init__(self, engine: MistralEncoderEngine, lm_head: torch.Tensor):
        self.eng, self.cfg, self.device = engine, engine.cfg, engine.device
        self.moe = bool(engine.cfg.num_local_experts)      # sparse-MoE (Mixtral) layers: router + the two chosen experts per row (_layers_moe)
        self.lm_head = lm_head.detach().to(device=self.device, dtype=BF16).contiguous()
        self.use_graph = True
        # which RMSNorms ride inside the following GEMV (grit_rmsnorm_gemv_bf16): "all" (input_layernorm -> q|k|v, post_attention_layernorm
        # -> gate|up, final norm -> lm_head), "qkv" (the MLP's and the final norm get their own launches) or "none"; GRIT_DECODE_FUSE_NORM for A/B runs
        # (profiles/r05_decode_variants.log).  Same bits in these three forms: the fused kernel applies the reference's two roundings.
        # "deferred" / "deferred_mlp": all three norms / the MLP's and the final one ride in the DEFERRED form (grit_rmsnorm_gemv_bf16_deferred:
        # the row scale multiplies the finished dot products, no second pass over the row; x_n is not rounded to bf16 -- one rounding fewer
        # than the reference's arithmetic).
        import os
        # The exact forms (round 5, profiles/r05_decode_variants.log, one box: all 3.49, qkv 3.25, none 3.32 ms per token): the 7168 workgroups of
        # the gate|up GEMV -- and the 8000 of lm_head -- each re-derive the row's RMS when the norm is fused, which costs more than the
        # one-row launch it saves; the q|k|v GEMV is a single workgroup wave deep and keeps the fusion.
        # Default "deferred" (tools/decode_norm_ab.sh, one box: qkv 3.149, deferred_mlp 3.014, deferred 2.904, all 3.410 ms per token).
        # It is NOT the reference's bf16 arithmetic bit for bit (one rounding fewer per norm; parity is held where it is bounded: greedy
        # tokens of the reference fixtures, teacher-forced logits vs fp32) -- GRIT_DECODE_FUSE_NORM=qkv restores the exact bits; both are
        # the same arithmetic at every batch size 1..8.
        self.fuse_norm = os.environ.get("GRIT_DECODE_FUSE_NORM", "deferred")
        # None: follow the engine's policy (fp16 operands under its fp16 policies); "bf16" / "f16" pin the decode arithmetic
        self.precision = os.environ.get("GRIT_DECODE_PRECISION") or None
        self.on_overflow = "raise"                # fp16 operands, a value beyond the range: "raise" | "bf16" (repeat the call in bf16)
        # prompt tokens on top of past_key_values: all at once through the step's kernels (same bits as one token per step; False or
        # GRIT_DECODE_PROMPT_CHUNK=0: the token-by-token loop).  Above `prompt_chunk_max_rows` rows (the attention workspace grows with
        # rows x splits) the loop is used.
        self.prompt_chunk = os.environ.get("GRIT_DECODE_PROMPT_CHUNK", "1") != "0" and not self.moe
        self.prompt_chunk_max_rows = 512
        # prompt tokens on top of past_key_values, the path: "rows" (the default: the decode step's kernels above, or the token loop) or
        # "gemm" (the encoder engine's MFMA GEMMs over the whole chunk, grit_attn_prefill_cached_*: MistralEncoderEngine.forward_on_cache;
        # right-padded rows supported).  GRIT_DECODE_PREFILL sets it.
        self.prefill = os.environ.get("GRIT_DECODE_PREFILL", "rows")
        if self.prefill not in PREFILL_MODES:
            raise ValueError(f"GRIT_DECODE_PREFILL={self.prefill!r}: one of {PREFILL_MODES}")
        self.last_prefill = None                  # the prompt path of the last generate() call: "encoder" | "rows" | "tokens" | "gemm"
        self._lm_head16 = None
        self.last_precision = None                # what the last generate() call ran in ("bf16" | "f16"; "bf16 (f16 overflow)" after a fallback)

    def _f16(self) -> bool:
        if self.precision not in (None, "bf16", "f16"):
            raise ValueError(f"MistralDecoder.precision={self.precision!r}: None (follow the engine), 'bf16' or 'f16'")
        return self.precision == "f16" or (self.precision is None and self.eng.precision in F16_POLICIES)

    def _lm_head_f16(self):
        key = (self.lm_head.data_ptr(), self.lm_head._version)
        if self._lm_head16 is None or self._lm_head16[0] != key:
            w = self.lm_head.to(F16)
            if bool(torch.isinf(w).any()):
                raise GritHipError("native decode on fp16 operands: lm_head weights exceed the fp16 range")
            self._lm_head16 = (key, w)
        return self._lm_head16[1]

    def _plan(self, rows: int, f16: bool, chunk: bool = False) -> Plan:
        """The launches of a pass over ``rows`` rows (a step's batch, or all B P rows of a prompt chunk), resolved once per call."""
        if chunk:
            # the projections in groups of 8 rows, so a chunk stays on the GEMV at any row count: its bits are the token-by-token path's at
            # 1..8 sequences (generate() takes it for the DEFERRED, DEFERRED plans only)
            return Plan(DEFERRED, DEFERRED, "rows", [(a, min(a + GEMV_ROWS, rows)) for a in range(0, rows, GEMV_ROWS)])
        qkv_norm, mlp_norm = (DEFERRED, DEFERRED) if f16 or self.moe else NORM_FORMS.get(self.fuse_norm, NORM_FORMS["qkv"])
        # beyond 2 rows the EXACT fused forms give the norm its own launch (they re-derive every row's RMS in every workgroup; same bits
        # either way).  The DEFERRED forms keep their arithmetic at every batch size (round 6): x_n is not rounded to bf16 there,
        # so switching to the un-fused norm at 3+ rows would make a row's logits -- and near-tie argmaxes -- depend on how many rows share
        # the step; the price is the deferred form's per-row work in the GEMV at 3..8 rows (batch 4: 4.93 against 4.69 ms per step, one box).
        # ("deferred_mlp" keeps its exact q|k|v norm fused at 3..8 rows as well.)
        if rows > 2 and DEFERRED not in (qkv_norm, mlp_norm):
            qkv_norm, mlp_norm = OWN, OWN
        return Plan(qkv_norm, mlp_norm, "append" if qkv_norm == OWN else "rope", [None])

    def _weights(self, L, f16: bool):
        """(q|k|v, o, gate|up, down) of a layer in the operand format; a sparse-MoE layer: (q|k|v, o, w13 stack, w2 stack)"""
        if f16:
            return self.eng._f16_weights(L)
        return (L.wqkv, L.wo, L.w13, L.w2) if self.moe else (L.wqkv, L.wo, L.wgu, L.wdown)

    def _embed(self, r, ids: torch.Tensor):
        ops.embed_gather(self.eng.embed, ids, out=r["h"])
        if r["f16"]:
            r["h16"].copy_(r["h"])                     # (bf16 embedding rows: exact in fp16 inside its range)

    def _attention(self, plan: Plan, r, li: int, L, wqkv, wo, out16):
        """The attention half of a layer, for every kind of pass: input_layernorm + q|k|v, RoPE + K/V append + attention, o_proj + residual.
        ``r``: the rows' buffers (a step: the state itself); ``out16``: where the residual epilogue writes the stream's fp16 rounding."""
        c = self.cfg
        nq, nkv, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        h, qkv, ctx, cos, sin, lens, ws = r["h"], r["qkv"], r["ctx"], r["cos"], r["sin"], r["lens"], r["ws"]
        ck, cv = r["cache"][li]
        for g in plan.groups:
            _norm_proj(plan.qkv_norm, _cut(r["xin"], g), L.ln1, c.rms_norm_eps, wqkv, _cut(qkv, g), r["x"])
        if plan.attn == "rope":
            ops.attn_decode_rope(qkv, cos, sin, ck, cv, lens, ctx, ws, nq, nkv, d)
        elif plan.attn == "append":
            ops.rope_kv_append(qkv, cos, sin, ck, cv, lens, nq, nkv, d)
            ops.attn_decode(qkv, ck, cv, lens, ctx, ws, nq, nkv, d)
        elif plan.attn == "prefix":                    # row v: prefix rows 0 .. plen[v // n] - 1 of its sequence, then its own tail (ck, cv)
            n, plen, (pk, pv) = r["n"], r["plen"], r["prefix"][li]
            Lpre, Ltail = pk.shape[2], ck.shape[2]
            prefix_ops.rope_kv_append_tail(qkv, cos, sin, ck, cv, lens, plen, n, nq, nkv, d, q16=r["q16"])
            prefix_ops.attn_decode_prefix(r["q16"] if r["f16"] else qkv, pk, pv, plen, ws, n, nq, nkv, d, Ltail)
            prefix_ops.attn_decode_tail(qkv, ck, cv, lens, plen, ws, n, nq, nkv, d, Lpre)
            prefix_ops.attn_decode_prefix_combine(ws, ctx, nq, nkv, d, Lpre, Ltail)
        else:                                          # "rows": row v is the token at position lens[v] of sequence rows[v]
            ops.rope_kv_append_rows(qkv, cos, sin, ck, cv, lens, r["rows"], nq, nkv, d)
            ops.attn_decode_rows(qkv, ck, cv, lens, r["rows"], ctx, ws, nq, nkv, d)
        for g in plan.groups:
            hg = _cut(h, g)
            _proj(_cut(ctx, g), wo, out=hg, epilogue=EPI_RESIDUAL, residual=hg, out16=_cut(out16, g))

    def _layers(self, plan: Plan, r):
        """Every dense layer over the rows of ``r`` (all sizes static, lengths on the device).  bf16: the stream h is its own operand; fp16
        operands: fp32 stream / q|k|v row / logits, fp16 weights, K/V and operand rows (xin = h16 = the stream's rounding, written by the
        residual epilogues; ctx; act).  The four projections of a layer run site by site, each over all row groups."""
        eps = self.cfg.rms_norm_eps
        for li, L in enumerate(self.eng.layers):
            wqkv, wo, wgu, wdown = self._weights(L, r["f16"])
            self._attention(plan, r, li, L, wqkv, wo, r["h16"])
            for g in plan.groups:                      # post_attention_layernorm + gate|up + SwiGLU
                _norm_proj(plan.mlp_norm, _cut(r["xin"], g), L.ln2, eps, wgu, _cut(r["act"], g), r["x"], epilogue=EPI_SWIGLU)
            for g in plan.groups:
                hg = _cut(r["h"], g)
                _proj(_cut(r["act"], g), wdown, out=hg, epilogue=EPI_RESIDUAL, residual=hg, out16=_cut(r["h16"], g))

    def _layers_moe(self, plan: Plan, st):
        """The layers of a sparse-MoE (Mixtral) model, MixtralSparseMoeBlock.forward (scripts/modeling_mixtral_gritlm.py:839-882) at 1..8
        rows: the attention half as in the dense step; then the router's top-2 decision ON THE DEVICE (experts [B,2], weights [B,2]) and,
        per row and choice, the two GEMVs of the chosen expert -- ``grit_gemv_*_expert`` reads the expert index from device memory, so the
        step is still one HIP graph and streams 2 of the 8 experts' weights per row -- and the weighted combine.
        bf16: the reference's arithmetic (exact RMSNorm for the block input, router on those bf16 rows, ``grit_moe_combine`` rounding
        points).  fp16 operands: the router reads the fp32 stream (norm folded in, nothing rounded), the experts run on fp16 copies, the
        combine adds fp32 expert outputs into the fp32 stream."""
        eps, f16 = self.cfg.rms_norm_eps, st["f16"]
        h, h16, x, act2, y2 = st["h"], st["h16"], st["x"], st["act2"], st["y2"]
        experts, weights = st["experts"], st["weights"]
        for li, L in enumerate(self.eng.layers):
            wqkv, wo, w13, w2 = self._weights(L, f16)
            self._attention(plan, st, li, L, wqkv, wo, None)       # (no out16: the combine below rewrites h16)
            if f16:
                ops.moe_router_top2(h, L.wgate, experts, weights, ln_w=L.ln2, eps=eps)
            ops.rmsnorm(h, L.ln2, eps, out=x)              # (bf16 rows: the reference's x_n; fp16 rows under fp16 operands)
            if not f16:
                ops.moe_router_top2(x, L.wgate, experts, weights)
            for b in range(h.shape[0]):
                for k in (0, 1):
                    r = 2 * b + k
                    ops.gemv_expert(x[b:b + 1], w13, experts[b, k:k + 1], out=act2[r:r + 1], epilogue=EPI_SWIGLU)
                    ops.gemv_expert(act2[r:r + 1], w2, experts[b, k:k + 1], out=y2[r:r + 1])
            if f16:
                ops.moe_decode_combine_f32(h, h16, y2, weights)
            else:
                ops.moe_combine(y2, st["rows_c"], weights, h, out=h)

    def _logits(self, form: str, st, x: torch.Tensor):
        """final norm + lm_head of the rows ``x`` into st["logits"]"""
        _norm_proj(form, x, self.eng.norm, self.cfg.rms_norm_eps, self._lm_head_f16() if st["f16"] else self.lm_head, st["logits"], st["x"])

    def _logits_after_engine(self, st, hidden: torch.Tensor):
        """The first logits after a prompt pass of the encoder engine, from each row's last valid token.  bf16: ``hidden`` is the final-norm
        output.  fp16 operands: the un-normalised stream, rounded to fp16, through the deferred final norm + lm_head launch of the steps."""
        if st["f16"]:
            self._logits(DEFERRED, st, hidden.to(F16))
        else:
            _proj(hidden, self.lm_head, out=st["logits"])

    # ------------------------------------------------------------------ one decode step
    def _step(self, st):
        plan = st["plan"]
        self._embed(st, st["next"])
        (self._layers_moe if self.moe else self._layers)(plan, st)
        self._logits(plan.mlp_norm, st, st["xin"])

    # ------------------------------------------------------------------ a prompt chunk on top of the cache, all its tokens at once
    def _prompt_rows(self, st, ids: torch.Tensor):
        """The P prompt tokens of every sequence in ONE pass over the weights per 8 rows instead of P decode steps (round 6): the V = B P
        rows go through the decode step's own kernels -- the GEMVs in groups of 8 rows, then every row's k / v appended at position
        lens + i (grit_rope_kv_append_rows), then every row attending to keys 0 .. lens + i of its sequence (grit_attn_decode_rows) --
        so the arithmetic per row is the token-by-token path's, bit for bit (tests: native_generate_prompt_chunk).  Leaves the logits after
        the last prompt token in st["logits"] and advances lens by P.  Built for the default (deferred-norm) step and the fp16 one."""
        c, dev = self.cfg, self.device
        nq, nkv, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        f16 = st["f16"]
        B, P = ids.shape
        V = B * P
        op, wide = (F16, F32) if f16 else (BF16, BF16)
        mk = lambda n, dt: torch.empty((V, n), dtype=dt, device=dev)
        h, h16 = mk(c.hidden_size, wide), mk(c.hidden_size, F16) if f16 else None
        r = dict(st, h=h, h16=h16, xin=h16 if f16 else h, x=None, qkv=mk((nq + 2 * nkv) * d, wide), ctx=mk(nq * d, op), act=mk(c.intermediate_size, op),
                 lens=(st["lens"].view(B, 1) + torch.arange(P, dtype=I32, device=dev).view(1, P)).reshape(V).contiguous(),
                 rows=torch.arange(B, dtype=I32, device=dev).repeat_interleave(P).contiguous(),
                 ws=ops.attn_decode_workspace(V, nq, nkv, st["cache"][0][0].shape[2], dev))
        plan = self._plan(V, f16, chunk=True)
        self._embed(r, ids.reshape(-1).contiguous())
        self._layers(plan, r)
        last = r["xin"].view(B, P, -1)[:, P - 1].contiguous()              # the stream of every sequence's last prompt token
        self._logits(plan.mlp_norm, st, last)                               # (B rows: 9..64 on the MFMA)
        st["lens"] += P

    @contextlib.contextmanager
    def _engine_pass(self, f16: bool, causal: bool | None = None):
        """A pass of the encoder engine under the decoder's arithmetic: a decoder on "f16" over a bf16 engine (or the reverse) switches the
        engine's policy -- and, with ``causal``, its attention -- for the pass and restores both."""
        e = self.eng
        was = e.causal, e.precision
        if f16 != (e.precision in F16_POLICIES):
            e.precision = "f16_operands" if f16 else "bf16"
        if causal is not None:
            e.causal = causal
        try:
            yield e
        finally:
            e.causal, e.precision = was

    def _prompt_gemm(self, st, ids: torch.Tensor, mask: torch.Tensor):
        """The prompt chunk through the encoder engine's GEMMs on top of the cache (MistralEncoderEngine.forward_on_cache; the engine's
        policy switched for the pass as in the past=None prefill), the first logits from each row's last valid token through the same
        launch the past=None prefill uses; advances lens by each row's valid length."""
        dev, f16 = self.device, st["f16"]
        plen, pos, last = (t.to(dev) for t in prefill_layout(mask, st["lens"], st["cache"][0][0].shape[2]))
        with self._engine_pass(f16) as e:
            hl = e.forward_on_cache(ids, st["cache"], st["lens"], plen, pos, last, final_norm=not f16)
        self._logits_after_engine(st, hl)
        st["lens"] += plen

    def _load_past(self, st, past, past_lens):
        """The cached prefix into the step's cache: K/V, every row's valid length, and -- K/V narrowed to fp16 on their way in (a bf16 /
        fp32 cache: values beyond 65504 became inf) -- a flag for non-finite values: they would surface as nan logits without touching
        the device's overflow flag (the fp32 outputs are not range-checked)."""
        dev, B, S0 = self.device, st["lens"].shape[0], past[0][0].shape[2]
        for (ck, cv), (k, v) in zip(st["cache"], past):
            ck[:, :, :S0].copy_(k.to(dev)); cv[:, :, :S0].copy_(v.to(dev))
        if st["f16"] and any(k.dtype != F16 or v.dtype != F16 for k, v in past):
            bad = torch.zeros((), dtype=torch.bool, device=dev)
            for ck, cv in st["cache"]:
                bad |= ~torch.isfinite(ck[:, :, :S0]).all()
                bad |= ~torch.isfinite(cv[:, :, :S0]).all()
            st["cache_bad"] = bad
        st["lens"].copy_(torch.full((B,), S0, dtype=I32, device=dev) if past_lens is None else past_lens.to(device=dev, dtype=I32))

    def _sample(self, st, lens: bool = True):
        """the token of the step: the device argmax, or with st["sampling"] = (T, top_k, top_p) the sampled draw on the rows' keys"""
        ln = st["lens"] if lens else None
        if st.get("sampling") is not None:
            T, k, p = st["sampling"]
            ops.sample_advance(st["logits"], st["next"], st["keys"], T, k, p, ln, st["history"], st["step"])
        else:
            ops.argmax_advance(st["logits"], st["next"], ln, st["history"], st["step"])

    def _shared_state(self, st0, n: int, max_new_tokens: int):
        """The decode state of share_prefix: B = B0 n rows on top of the B0-row state ``st0`` the prompt phase ran on.  Its cache stays
        where it is -- rows 0 .. lens0[s] - 1 are sequence s's prefix, ONE copy -- and every row gets a tail cache [nkv, Ltail, d] for its
        own tokens (Ltail: max_new_tokens rounded up to 64); lens [B] (global positions) start at lens0 repeated, plen [B0] = lens0 stays.
        The first-step logits are st0's rows repeated n times consecutively (Hugging Face's order: row r = s n + j)."""
        c, dev, f16 = self.cfg, self.device, st0["f16"]
        nq, nkv, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        B0, Lpre = st0["lens"].shape[0], st0["cache"][0][0].shape[2]
        B, Ltail = B0 * n, (max(max_new_tokens, 1) + 63) // 64 * 64
        st = self._rows(B, f16)
        cos, sin = rope_tables(Lpre + Ltail, d, c.rope_theta, self.eng.rope_bf16 and not f16, dev)
        st.update(plan=st["plan"]._replace(attn="prefix"), n=n, prefix=st0["cache"], plen=st0["lens"].clone(), cos=cos, sin=sin,
                  ws=prefix_ops.workspace(B, nq, nkv, Lpre, Ltail, dev), q16=torch.empty((B, nq * d), dtype=F16, device=dev) if f16 else None,
                  cache=self._caches(B, Ltail, f16))
        st["lens"].copy_(st0["lens"].repeat_interleave(n))
        st["logits"].copy_(st0["logits"].repeat_interleave(n, dim=0))
        if "cache_bad" in st0:
            st["cache_bad"] = st0["cache_bad"]
        return st

    def _caches(self, B: int, L: int, f16: bool):
        """per-layer (k, v) [B, nkv, L, d] in the operand format, zeroed"""
        c, op = self.cfg, F16 if f16 else BF16
        shape = (B, c.num_key_value_heads, L, c.head_dim)
        return [(torch.zeros(shape, dtype=op, device=self.device), torch.zeros(shape, dtype=op, device=self.device)) for _ in range(c.num_hidden_layers)]

    def _rows(self, B: int, f16: bool):
        """The per-row buffers of a pass over B rows and its plan -- everything of a state that does not depend on a cache length."""
        c, dev = self.cfg, self.device
        nq, nkv, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        op = F16 if f16 else BF16                      # operand rows and the K/V cache
        wide = F32 if f16 else BF16                    # the stream, the q|k|v row, the logits
        mk = lambda n, dt: torch.empty((B, n), dtype=dt, device=dev)
        moe = {}
        if self.moe:
            moe = dict(act2=torch.empty((2 * B, c.intermediate_size), dtype=op, device=dev), y2=torch.empty((2 * B, c.hidden_size), dtype=wide, device=dev),
                       experts=torch.zeros((B, 2), dtype=I32, device=dev), weights=torch.zeros((B, 2), dtype=F32, device=dev),
                       rows_c=torch.arange(2 * B, dtype=I32, device=dev).view(B, 2).contiguous())
        h, h16 = mk(c.hidden_size, wide), mk(c.hidden_size, F16) if f16 else None
        # (xin: what a norm + projection launch reads of the stream -- its fp16 rounding under fp16 operands)
        return dict(**moe, f16=f16, plan=self._plan(B, f16), h=h, h16=h16, xin=h16 if f16 else h, x=mk(c.hidden_size, op), qkv=mk((nq + 2 * nkv) * d, wide), ctx=mk(nq * d, op),
                    act=mk(c.intermediate_size, op), logits=mk(self.lm_head.shape[0], wide), next=torch.zeros((B,), dtype=I64, device=dev),
                    lens=torch.zeros((B,), dtype=I32, device=dev), step=torch.zeros((1,), dtype=I32, device=dev))

    def _state(self, B: int, Lmax: int, f16: bool = False):
        c, dev = self.cfg, self.device
        # (the fp16 policies rotate with the unrounded fp32 tables, like the encoder's fp16 forward)
        cos, sin = rope_tables(Lmax, c.head_dim, c.rope_theta, self.eng.rope_bf16 and not f16, dev)
        return dict(**self._rows(B, f16), cos=cos, sin=sin, ws=ops.attn_decode_workspace(B, c.num_attention_heads, c.num_key_value_heads, Lmax, dev),
                    cache=self._caches(B, Lmax, f16))

    # ------------------------------------------------------------------ API
    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int, attention_mask: torch.Tensor | None = None, past_key_values=None,
                 past_lens: torch.Tensor | None = None, eos_token_id: int | None = None, return_logits: bool = False,
                 on_overflow: str | None = None, do_sample: bool = False, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                 seed: int | None = None, num_return_sequences: int = 1, share_prefix: bool = False, _force_bf16: bool = False):
        """Greedy (or, with ``do_sample``, sampled) continuation.  ``input_ids`` [B,P]: the NEW prompt tokens (right-padded rows need
        ``attention_mask``; with ``past_key_values`` all rows must be full length under ``prefill="rows"``, right-padded under ``"gemm"``).
        ``past_key_values``: per-layer K/V [B,nkv,S,d] of an already encoded prefix, e.g. the bidirectional document pass of ``encode(get_cache=True)``; ``past_lens`` [B] = valid prefix tokens per row
        (default S).  Returns the generated ids [B, max_new_tokens] (int64; positions after ``eos_token_id`` keep that id) and, with
        ``return_logits``, the logits of every generated position [B, max_new_tokens, V] (bf16; fp32 on fp16 operands).

        On fp16 operands (module docstring) a value beyond the fp16 range invalidates the call: ``on_overflow="raise"`` raises
        ``GritHipError``, ``"bf16"`` repeats the whole call in the bf16 arithmetic; default ``self.on_overflow`` ("raise";
        ``GritLM(precision="auto").native_decoder()`` sets "bf16": the ladder's last rung).

        ``do_sample``: each token is drawn as Hugging Face's multinomial sampling draws it -- ``temperature``, then ``top_k`` (0: off), then
        ``top_p`` (1: off); defaults are GenerationConfig's -- by grit_sample_advance (semantics and RNG contract in include/gritlm_hip.h).
        Row r of the call draws with key ``seed + r`` (mod 2^64); ``seed=None`` takes one from torch's default CPU generator.
        ``num_return_sequences`` = n repeats every input row n times first (rows of one prompt consecutive, as ``repeat_interleave``), so
        the call decodes B n rows and returns [B n, max_new_tokens].  The bf16 repeat of an fp16 overflow reuses the call's seed.

        ``share_prefix`` (with n > 1; a no-op at n = 1; dense engines only): everything before the first sampled token -- cached document
        and prompt -- is computed once per input row and its K/V kept ONCE; the n rows of an input row attend to that shared prefix on the
        MFMA (grit_attn_decode_prefix) and to a short tail of their own tokens, instead of to n copies of the cache.  Same row order, keys
        and sampling; the prefix products round P (and, on fp16 operands, q) to the 16-bit operand format like the encoder's attention,
        so the logits are not bit-identical to the expanded call's (both within the same bounds of the fp32 module).  Measured at the 7B shape
        (tools/shared_prefix_bench.py, one box, B0 = 1): the shared step was the faster one at every measured point, prefix 256 included
        (n = 20: 5.25 against 5.50 ms, n = 64: 8.10 against 9.56 ms) and 1.8x at prefix 2048, n = 64; shorter prefixes and smaller n
        were not measured -- there the four attention launches per layer in place of two are the cost to weigh."""
        dev, c = self.device, self.cfg
        if self.prefill not in PREFILL_MODES:
            raise ValueError(f"MistralDecoder.prefill={self.prefill!r}: one of {PREFILL_MODES}")
        check_sampling(temperature, top_k, top_p, num_return_sequences, do_sample)
        n = int(num_return_sequences)
        if share_prefix and self.moe:
            raise NotImplementedError("native decode of a sparse-MoE (Mixtral) engine: share_prefix is built for dense engines")
        shared = bool(share_prefix) and n > 1             # (n = 1: nothing to share, the plain path)
        attention_mask0, past_key_values0, past_lens0 = attention_mask, past_key_values, past_lens      # (the bf16 repeat expands again)
        B = input_ids.shape[0] * n
        if B > MAX_ROWS:
            raise NotImplementedError(f"native decode: batch <= {MAX_ROWS} (got {B}); split the batch")
        if self.moe and B > GEMV_ROWS:
            raise NotImplementedError(f"native decode of a sparse-MoE (Mixtral) engine: batch <= {GEMV_ROWS} (got {B})")
        f16 = self._f16() and not _force_bf16
        on_overflow = self.on_overflow if on_overflow is None else on_overflow
        if on_overflow not in ("raise", "bf16"):
            raise ValueError(f"on_overflow={on_overflow!r}: 'raise' or 'bf16'")
        if do_sample and seed is None:
            seed = draw_seed()
        if f16:
            ops.f16_overflow_flag(dev, clear=True)        # a stale flag of an earlier call is not this call's
            self.eng._f16_weights(self.eng.layers[0])     # (refuses weights beyond the fp16 range before anything runs)
        ids = input_ids.to(device=dev, dtype=I64)
        if n > 1 and not shared:                          # Hugging Face's expansion: the n copies of a row are consecutive
            ids = ids.repeat_interleave(n, dim=0)
            attention_mask = None if attention_mask is None else attention_mask.repeat_interleave(n, dim=0)
            past_lens = None if past_lens is None else past_lens.repeat_interleave(n, dim=0)
            if past_key_values is not None:
                past_key_values = [(k.repeat_interleave(n, dim=0), v.repeat_interleave(n, dim=0)) for k, v in _layers_of(past_key_values)]
        B, P = ids.shape
        nq, nkv, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        past = _layers_of(past_key_values) if past_key_values is not None else None
        S0 = past[0][0].shape[2] if past is not None else 0
        if 0 < self.eng.window_keys < S0 + P + max_new_tokens:
            # the reference's sdpa path (window_keys = 0) attends to the whole cache; its eager / flash paths window the cache (and the
            # flash path slices it, modeling_mistral_gritlm.py:394-415) -- the decode kernels attend to the whole cache only
            raise NotImplementedError(f"native decode past the sliding window ({self.eng.window_keys} keys) is built for the sdpa semantics "
                                      "only (window_keys = 0: full causal attention over the cache)")
        # (share_prefix: the prompt phase runs on the B0 un-expanded rows, on a state whose cache ends with the prompt)
        Lmax = (S0 + P + (0 if shared else max_new_tokens) + 255) // 256 * 256
        st = self._state(B, Lmax, f16)
        if past is None:
            # prefill: one causal pass over the prompt that also emits the post-RoPE K/V (the encoder engine's forward)
            mask = torch.ones((B, P), dtype=I64, device=dev) if attention_mask is None else attention_mask.to(device=dev, dtype=I64)
            # fp16 operands: the prompt pass runs under the engine's fp16 policy as well (causal fp16 attention, grit_attn_causal_f16_fwd); its
            # fp16 K/V go into the cache as they are and the first token's logits come from the un-normalised stream of the last prompt
            # token through the same deferred norm + lm_head launch the decode steps use.  A decoder pinned to "f16" on a bf16 engine
            # (or the reverse) switches the engine's policy for the pass and restores it.
            with self._engine_pass(f16, causal=True) as e:
                hidden, kv = e.forward(ids, mask, borrow=True, return_kv=True, final_norm=not f16, kv_dtype=None if f16 else BF16)
            for li, (k, v) in enumerate(kv):
                st["cache"][li][0][:, :, :P].copy_(k); st["cache"][li][1][:, :, :P].copy_(v)
            plen = mask.sum(dim=1).to(I32)
            st["lens"].copy_(plen)
            self.last_prefill = "encoder"
            last = hidden[torch.arange(B, device=dev), (plen - 1).long()].contiguous()              # [B,H] of the last prompt token
            self._logits_after_engine(st, last)
        elif self.prefill == "gemm" and P > 0:
            mask = torch.ones((B, P), dtype=I64, device=dev) if attention_mask is None else attention_mask.to(device=dev, dtype=I64)
            prefill_layout(mask, torch.zeros((B,), dtype=I32, device=dev))        # (refuses a mask that is not right-padded before anything runs)
            self._load_past(st, past, past_lens)
            self._prompt_gemm(st, ids, mask)
            self.last_prefill = "gemm"
        else:
            if attention_mask is not None and not bool((attention_mask != 0).all()):
                raise NotImplementedError("native decode: padded prompt rows on top of past_key_values")
            self._load_past(st, past, past_lens)
            # the prompt rides on the decode path: all its tokens at once (_prompt_rows: the step's own kernels over B P rows), or, for the
            # exact-norm forms and very long prompts, one token per step (teacher forced); its K/V land behind the cached prefix
            if P > 0 and self.prompt_chunk and (f16 or self.fuse_norm == "deferred") and B * P <= self.prompt_chunk_max_rows:
                self._prompt_rows(st, ids)
                self.last_prefill = "rows"
            else:
                for t in range(P):
                    st["next"].copy_(ids[:, t])
                    self._step(st)
                    st["lens"] += 1
                self.last_prefill = "tokens"
        if shared:                                        # the decode phase: B0 n rows on the one prefix copy and their own tails
            st = self._shared_state(st, n, max_new_tokens)
            B *= n
        st["history"] = torch.zeros((B, max_new_tokens), dtype=I64, device=dev)
        if do_sample:
            st["sampling"], st["keys"] = (float(temperature), int(top_k), float(top_p)), row_keys(seed, B, dev)
        logits_all = torch.empty((B, max_new_tokens, self.lm_head.shape[0]), dtype=st["logits"].dtype, device=dev) if return_logits else None
        # first generated token from the prefill logits, then decode steps (graph replay)
        if return_logits:
            logits_all[:, 0].copy_(st["logits"])
        self._sample(st, lens=False)
        graph = None
        for t in range(1, max_new_tokens):
            # Hugging Face's generate() stops once every row has emitted EOS; here the host only replays a graph, so it looks every 16
            # tokens (one small D2H) instead of after each one: at most 15 tokens of wasted steps, none of them returned
            if eos_token_id is not None and t % 16 == 0 and bool((st["history"][:, :t] == eos_token_id).any(dim=1).all()):
                break
            if graph is not None:
                graph.replay()
            else:
                self._step(st)
                if logits_all is not None:
                    logits_all[:, t].copy_(st["logits"])
                self._sample(st)
                if self.use_graph and logits_all is None and t + 1 < max_new_tokens:
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self._step(st)
                        self._sample(st)
        out = st["history"]
        self.last_precision = "f16" if f16 else ("bf16 (f16 overflow)" if _force_bf16 else "bf16")
        if f16 and (ops.f16_overflow_flag(dev, clear=True) or bool(st.get("cache_bad", False))):
            if on_overflow == "bf16":
                return self.generate(input_ids, max_new_tokens, attention_mask=attention_mask0, past_key_values=past_key_values0,
                                     past_lens=past_lens0, eos_token_id=eos_token_id, return_logits=return_logits, do_sample=do_sample,
                                     temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, num_return_sequences=n, share_prefix=share_prefix,
                                     _force_bf16=True)
            raise GritHipError("native decode on fp16 operands: a value exceeded the fp16 range (activation, K/V or a cached K/V that was "
                               "already inf); the tokens of this call are invalid -- decode with precision 'bf16' (MistralDecoder.precision, "
                               "or on_overflow='bf16')")
        if eos_token_id is not None:
            hit = (out == eos_token_id).long().cumsum(dim=1) > 0
            out = torch.where(hit, torch.full_like(out, eos_token_id), out)
        return (out, logits_all) if return_logits else out
