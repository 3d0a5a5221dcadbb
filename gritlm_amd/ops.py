"""Thin torch-tensor -> C-ABI adapters.  PyTorch is plumbing here: it owns device memory and streams;
all arithmetic happens in libgritlm_hip.so.  Every function launches on torch's current HIP stream.

How an op is written: allocate what it returns, then make one ``_call(entry, *C arguments)`` -- the entry point is named once, the
stream is ``_stream()`` where the header has it, a refusal raises with the entry's name.  Every pointer comes from ``_chk`` (``_opt``
for an optional operand), which refuses a CPU tensor, another dtype or another layout.  An op with one entry point per operand format
takes it from a table that ``_entries`` makes from the name rule; an output's width under an epilogue is ``_epi_cols``; a timed op
puts ``ev = _timer and _begin(...)`` in front of the call and ``if ev: ev.record()`` behind it."""
from __future__ import annotations

import ctypes
import functools
import os

import torch

from . import _lib
from ._lib import (EPI_RESIDUAL, EPI_RESIDUAL_F32, EPI_STORE, EPI_SWIGLU, EPI_SWIGLU_BWD, EPI_SWIGLU_STACKED, EPI_SWIGLU_STACKED_SAVE,
                   POOL_MODES, check)

BF16, F16, F32, I64, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int64, torch.int32


def _stream():
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional per-kernel-class HIP-event timing (bench.py's live roofline measurement).

    Events are recorded on torch's current stream -- the stream every kernel here is launched on."""

    def __init__(self):
        self.pairs: dict[str, list] = {}
        self.work: dict[str, float] = {}
        self.tags: dict[str, list] = {}
        self.deferred: dict[str, list] = {}

    def span(self, name: str, work=0.0, tag: str | None = None):
        """``work``: FLOPs (or bytes) of the launch -- a float, or a 0-dim DEVICE tensor when the amount depends on device data (the packed
        attention's sum of len^2): it is read at summary(), after the timed region, never inside it."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.setdefault(name, []).append((a, b))
        if torch.is_tensor(work):
            self.deferred.setdefault(name, []).append(work)
            work = 0.0
        self.tags.setdefault(name, []).append((tag, work))
        self.work[name] = self.work.get(name, 0.0) + work
        return a, b

    def summary(self) -> dict:
        torch.cuda.synchronize()
        for name, ws in self.deferred.items():
            self.work[name] = self.work.get(name, 0.0) + float(sum(float(w) for w in ws))
        self.deferred = {}
        out = {}
        for name, pairs in self.pairs.items():
            ms = [a.elapsed_time(b) for a, b in pairs]
            out[name] = dict(launches=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / len(ms), work=self.work[name])
            by_tag = {}
            for t, (tag, work) in zip(ms, self.tags[name]):
                if tag is not None:
                    d = by_tag.setdefault(tag, dict(launches=0, total_ms=0.0, work=0.0))
                    d["launches"] += 1; d["total_ms"] += t; d["work"] += work
            if by_tag:
                out[name]["by_tag"] = by_tag
        return out


_timer: KernelTimer | None = None
_TAG_M = bool(os.environ.get("GRIT_TIMER_TAG_M"))          # tools/contrastive_shapes.py: the GEMM tags carry M as well (forward / dgrad / wgrad shapes apart)


def set_timer(t: KernelTimer | None):
    global _timer
    _timer = t


def _call(name: str, *args):
    """The one way into the library: entry point ``name`` on its C arguments (the stream among them, where the header has it, taken from
    ``_stream()`` by the op); a refusal raises, naming that entry."""
    rc = getattr(_lib.load(), name)(*args)
    if rc:
        check(rc, name)


def _begin(name: str, work, tag: str | None = None):
    """The timer bracket of a timed op, which costs one None test when no timer is set: ``ev = _timer and _begin(name, work, tag)`` in
    front of the launch (the arguments of KernelTimer.span), ``if ev: ev.record()`` behind it."""
    ev = _timer.span(name, work, tag)
    ev[0].record()
    return ev[1]


def _chk(t: torch.Tensor, dtype, name: str, rank: int = 0):
    """Pointer of a checked operand.  ``rank`` 0: contiguous; 2: row-strided matrix (unit column stride, leading dimension stride(0): what
    the GEMM entry points take); 3: [E,N,K] stack of such matrices (leading dimension stride(1), matrix stride stride(0))."""
    if not t.is_cuda:
        raise _lib.GritHipError(f"{name}: tensor must live on the GPU (got {t.device}); the native path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if (t.dim() != rank or t.stride(-1) != 1) if rank else not t.is_contiguous():
        raise ValueError(f"{name}: {rank}-D tensor with unit column stride expected" if rank else f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _opt(t: torch.Tensor | None, dtype, name: str, ld: bool = False):
    """Pointer of an optional contiguous operand, 0 without it; ``ld``: (pointer, row stride) of an optional matrix, (0, 0) without it."""
    if t is None:
        return (0, 0) if ld else 0
    return (_chk(t, dtype, name, 2), t.stride(0)) if ld else _chk(t, dtype, name)


def _entries(pattern: str) -> dict:
    """operand format -> entry point, for the ops that have one per format: ``{fmt}`` is the format's name (grit_gemv_{fmt}: bf16, f16);
    ``{_fmt}`` is for the pairs whose bf16 entry carries no name (grit_argmax_advance{_fmt}: nothing, _f32; grit_attn_decode_rope{_fmt}: _f16)."""
    return {dt: pattern.format(fmt=fmt, _fmt="" if dt == BF16 else "_" + fmt) for dt, fmt in ((BF16, "bf16"), (F16, "f16"), (F32, "f32"))}


# the output's columns under an epilogue, in halves of the weight's N rows: the SWIGLU forms halve them, SWIGLU_BWD gives [d_gate | d_up]
_EPI_HALVES = {EPI_SWIGLU: 1, EPI_SWIGLU_STACKED: 1, EPI_SWIGLU_STACKED_SAVE: 1, EPI_SWIGLU_BWD: 4}


def _epi_cols(N: int, epilogue: int) -> int:
    return N * _EPI_HALVES.get(epilogue, 2) // 2


# (table or input rows, out) formats -> entry point (and, for the fp16-rows RMSNorm, its "out is fp16" argument); a pair that is not
# built is refused as the first format's default out
_EMBED_GATHER = {(BF16, F32): "grit_embed_gather_f32", **dict.fromkeys(((BF16, BF16), (F16, F16)), "grit_embed_gather")}     # (16-bit words copied)
_RMSNORM_FWD = {(BF16, BF16): ("grit_rmsnorm_fwd", ()), (F32, BF16): ("grit_rmsnorm_fwd_f32in", ()), (F32, F16): ("grit_rmsnorm_fwd_f32in_f16", ()),
                **{(F16, odt): ("grit_rmsnorm_fwd_f16in", (int(odt == F16),)) for odt in (F16, BF16)}}


def embed_gather(table: torch.Tensor, ids: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 table: rows copied, or widened (exact) into an fp32 ``out`` (the fp32 residual stream).  fp16 table (the fp16 residual stream's
    copy of it): rows copied into an fp16 ``out`` (the gather moves 16-bit words)."""
    V, H = table.shape
    T = ids.numel()
    if out is None:
        out = torch.empty((T, H), dtype=BF16, device=table.device)
    pair = (table.dtype, out.dtype)
    if pair not in _EMBED_GATHER:
        pair = (F16, F16) if table.dtype == F16 else (BF16, BF16)
    _call(_EMBED_GATHER[pair], _chk(table, pair[0], "table"), _chk(ids, I64, "ids"), _chk(out, pair[1], "out"), T, H, V, _stream())
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 rows: the reference's bf16 arithmetic.  fp32 rows (the encoder's fp32 residual stream): one rounding, bf16 out -- or fp16 out
    when ``out`` is an fp16 tensor (the f16_operands policy; w stays bf16).  fp16 rows (the fp16 residual stream): one rounding, to fp16
    (the next operand) or to bf16 (last_hidden_state)."""
    H = x.shape[-1]
    T = x.numel() // H
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    pair = (x.dtype, out.dtype)
    if pair not in _RMSNORM_FWD:
        pair = (F16, F16) if x.dtype == F16 else (F32 if x.dtype == F32 else BF16, BF16)
    name, out_is_f16 = _RMSNORM_FWD[pair]
    _call(name, _chk(x, pair[0], "x"), _chk(w, BF16, "w"), _chk(out, pair[1], "out"), *out_is_f16, T, H, float(eps), _stream())
    return out


def rope_qk_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, S: int, nq: int, nkv: int, d: int, inverse: bool = False):
    T, stride = qkv.shape
    _call("grit_rope_qk_inplace", _chk(qkv, BF16, "qkv"), _chk(cos, F32, "cos"), _chk(sin, F32, "sin"), T, S, nq, nkv, d, stride, int(inverse), _stream())
    return qkv


def rope_qk_pos_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, positions: torch.Tensor, nq: int, nkv: int, d: int,
                 inverse: bool = False):
    """RoPE for packed rows: positions[t] (int32) = index of token t inside its own sequence."""
    T, stride = qkv.shape
    _call("grit_rope_qk_inplace_pos", _chk(qkv, BF16, "qkv"), _chk(cos, F32, "cos"), _chk(sin, F32, "sin"), _chk(positions, I32, "positions"),
          T, cos.shape[0], nq, nkv, d, stride, int(inverse), _stream())
    return qkv


def _attn_entry(kind: str, varlen: bool, causal: bool, window: int, dtype=BF16):
    """(entry point's name, extra arguments) of an attention call (``kind``: fwd or bwd; padded or packed rows): bidirectional, causal, or
    causal with a sliding window of ``window`` keys.  fp16 (forward only): the fp16-operand entry points, whose causal form takes the
    window (0: none) as an argument."""
    window = int(window or 0)
    if window > 0 and not causal:
        raise ValueError("a sliding window applies to causal attention only (the bidirectional embedding path ignores it, as the reference)")
    extra = (window,) if (causal if dtype == F16 else window > 0) else ()
    mode = ("causal_window" if window > 0 and dtype != F16 else "causal") if causal else "bidir"
    return "grit_attn_" + mode + ("_varlen" if varlen else "") + ("_f16_" if dtype == F16 else "_") + kind, extra


def _attn_fwd(varlen: bool, qkv, layout, layout_name: str, sizes: tuple, flops, nq: int, nkv: int, d: int, out, scale, lse, causal: bool, window: int):
    """What the padded and the packed forward share: ``layout`` is key_bits or cu_seqlens, ``sizes`` the (B, S) or (B, max_len) in front of
    nq; ``flops`` (a number, or a callable for a count that costs device work) feeds the timer span."""
    T, stride = qkv.shape
    if out is None:
        out = torch.empty((T, nq * d), dtype=qkv.dtype, device=qkv.device)
    if scale is None:
        scale = d ** -0.5
    odt = F16 if qkv.dtype == F16 else BF16            # fp16: the fp16-operand policies
    name, wa = _attn_entry("fwd", varlen, causal, window, odt)
    ev = _timer and _begin("attn_bidir_fwd", flops() if callable(flops) else flops)
    _call(name, _chk(qkv, odt, "qkv"), _chk(layout, I32 if varlen else I64, layout_name), _chk(out, odt, "out"), _opt(lse, F32, "lse"), *sizes,
          nq, nkv, d, stride, out.stride(0), float(scale), *wa, _stream())
    if ev:
        ev.record()
    return out


def attn_bidir_varlen(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, nq: int, nkv: int, d: int,
                      out: torch.Tensor | None = None, scale: float | None = None, lse: torch.Tensor | None = None,
                      causal: bool = False, window: int = 0) -> torch.Tensor:
    """lse (optional, fp32 [T, nq]) receives the log-sum-exp rows for grit_attn_bidir_varlen_bwd.  ``window`` > 0 (causal only): sliding
    window, a query sees keys q - window + 1 .. q."""
    def flops():         # algorithmic FLOPs of the packed launch: 4 d nq sum(len^2) (half of it when causal), summed on the device
        lens = (cu_seqlens[1:] - cu_seqlens[:-1]).double()
        return (lens * lens).sum() * (4.0 * nq * d * (0.5 if causal else 1.0))
    return _attn_fwd(True, qkv, cu_seqlens, "cu_seqlens", (cu_seqlens.numel() - 1, int(max_len)), flops, nq, nkv, d, out, scale, lse, causal, window)


def _pool_fwd(varlen: bool, hidden, layout, sizes: tuple, method: str, normalize: bool, instr_len, inv_norm):
    """What the padded and the packed pooling share: ``layout`` is the int64 mask or the int32 cu_seqlens, ``sizes`` (B, S, H) or (B, H)."""
    if method not in POOL_MODES:
        raise NotImplementedError(f"Unknown pooling method: {method}")     # gritlm/gritlm.py:215
    out = torch.empty((sizes[0], sizes[-1]), dtype=F32, device=hidden.device)
    _call("grit_pool_norm_varlen_fwd" if varlen else "grit_pool_norm_fwd", _chk(hidden, BF16, "hidden"),
          _chk(layout, I32, "cu_seqlens") if varlen else _chk(layout, I64, "mask"), _opt(instr_len, I32, "instr_len"), _chk(out, F32, "out"),
          _opt(inv_norm, F32, "inv_norm"), *sizes, POOL_MODES[method], int(normalize), _stream())
    return out


def _pool_bwd(varlen: bool, y, dy, inv_norm, layout, dh_shape: tuple, sizes: tuple, method: str, normalize: bool, instr_len):
    dh = torch.empty(dh_shape, dtype=BF16, device=y.device)
    _call("grit_pool_norm_varlen_bwd" if varlen else "grit_pool_norm_bwd", _chk(y, F32, "y"), _chk(dy, F32, "dy"), _opt(inv_norm, F32, "inv_norm"),
          _chk(layout, I32, "cu_seqlens") if varlen else _chk(layout, I64, "mask"), _opt(instr_len, I32, "instr_len"), _chk(dh, BF16, "dhidden"),
          *sizes, POOL_MODES[method], int(normalize), _stream())
    return dh


def pool_norm_varlen(hidden: torch.Tensor, cu_seqlens: torch.Tensor, method: str, normalize: bool,
                     instr_len: torch.Tensor | None = None, inv_norm: torch.Tensor | None = None) -> torch.Tensor:
    return _pool_fwd(True, hidden, cu_seqlens, (cu_seqlens.numel() - 1, hidden.shape[-1]), method, normalize, instr_len, inv_norm)


def pool_norm_varlen_bwd(y: torch.Tensor, dy: torch.Tensor, inv_norm: torch.Tensor | None, cu_seqlens: torch.Tensor, T: int, method: str,
                         normalize: bool, instr_len: torch.Tensor | None = None) -> torch.Tensor:
    B, H = y.shape
    return _pool_bwd(True, y, dy, inv_norm, cu_seqlens, (T, H), (B, H), method, normalize, instr_len)


_GEMM_NT = _entries("gemm_{fmt}_nt")          # (the timer's span names; the entry points with grit_ in front)


def gemm_nt(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None, epilogue: int = EPI_STORE,
            residual: torch.Tensor | None = None) -> torch.Tensor:
    """out[M,N] = a[M,K] @ w[N,K]^T (+ epilogue).  SWIGLU: w holds interleaved gate/up rows (SWIGLU_STACKED: [gate; up]), out is [M, N/2].
    SWIGLU_STACKED_SAVE: additionally writes the bf16 [gate | up] pre-activations into `residual` ([M, N]).
    SWIGLU_BWD: a @ w^T is d_act [M, N]; `residual` holds the saved [gate | up] ([M, 2N]); out = [d_gate | d_up] ([M, 2N])."""
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K, (a.shape, w.shape)
    n_out = _epi_cols(N, epilogue)
    opd = a.dtype if a.dtype == F16 else BF16                 # fp16 operands: the f16_operands policy (STORE, SWIGLU, RESIDUAL_F32)
    odt = F32 if epilogue == EPI_RESIDUAL_F32 else opd        # RESIDUAL_F32: out and residual are the fp32 residual stream
    if opd == F16 and epilogue not in (EPI_STORE, EPI_SWIGLU, EPI_SWIGLU_STACKED, EPI_RESIDUAL, EPI_RESIDUAL_F32):
        raise _lib.GritHipError(f"gemm_nt: epilogue {epilogue} is not built for fp16 operands (STORE, SWIGLU, SWIGLU_STACKED, RESIDUAL, RESIDUAL_F32)")
    if out is None:
        out = torch.empty((M, n_out), dtype=odt, device=a.device)
    assert out.shape == (M, n_out)
    rp, ldr = 0, 0
    if epilogue in (EPI_RESIDUAL, EPI_RESIDUAL_F32, EPI_SWIGLU_STACKED_SAVE, EPI_SWIGLU_BWD):
        assert residual is not None and residual.shape == (M, 2 * N if epilogue == EPI_SWIGLU_BWD else N)
        rp, ldr = _opt(residual, odt, "residual", True)
    name = _GEMM_NT[opd]
    ev = _timer and _begin(name, 2.0 * M * N * K, (f"M={M}," if _TAG_M else "") + f"N={N},K={K},epi={epilogue}")
    _call("grit_" + name, _chk(a, opd, "a", 2), _chk(w, opd, "w", 2), _chk(out, odt, "out", 2), M, N, K, a.stride(0), w.stride(0), out.stride(0),
          epilogue, rp, ldr, _stream())
    if ev:
        ev.record()
    return out


def gemm_nt_pair(a1: torch.Tensor, w1: torch.Tensor, out1: torch.Tensor, a2: torch.Tensor, w2: torch.Tensor, out2: torch.Tensor,
                 accumulate: bool = True) -> None:
    """Two dense GEMMs with the same K in ONE launch: out_i (+)= a_i[M_i,K] @ w_i[N_i,K]^T, bit-identical to two gemm_nt calls.  Used for
    weight-gradient pairs whose tile counts do not fill whole waves of CUs on their own (``accumulate``: RESIDUAL epilogue onto out_i)."""
    (M1, K), (M2, K2) = a1.shape, a2.shape
    N1, N2 = w1.shape[0], w2.shape[0]
    assert K == K2 == w1.shape[1] == w2.shape[1] and out1.shape == (M1, N1) and out2.shape == (M2, N2)
    epi = EPI_RESIDUAL if accumulate else EPI_STORE
    ev = _timer and _begin("gemm_bf16_nt", 2.0 * (M1 * N1 + M2 * N2) * K, (f"M={M1}+{M2}," if _TAG_M else "") + f"pair N={N1}+{N2},K={K},epi={epi}")
    o1, o2 = _chk(out1, BF16, "out1", 2), _chk(out2, BF16, "out2", 2)
    _call("grit_gemm_bf16_nt_pair",
          _chk(a1, BF16, "a1", 2), _chk(w1, BF16, "w1", 2), o1, o1 if accumulate else 0, M1, N1, a1.stride(0), w1.stride(0), out1.stride(0),
          out1.stride(0) if accumulate else 0,
          _chk(a2, BF16, "a2", 2), _chk(w2, BF16, "w2", 2), o2, o2 if accumulate else 0, M2, N2, a2.stride(0), w2.stride(0), out2.stride(0),
          out2.stride(0) if accumulate else 0, K, epi, _stream())
    if ev:
        ev.record()


def gemm_nt_rope(a: torch.Tensor, w: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, rope_cols: int, S: int = 0,
                 positions: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Fused QKV projection + RoPE on the leading ``rope_cols`` columns (q, k heads; head_dim 128): gemm_nt followed by rope_qk_[pos_],
    in one launch.  Positions: ``positions`` int32 [M] (packed rows) or row % S."""
    M, K = a.shape
    N = w.shape[0]
    opd = a.dtype if a.dtype == F16 else BF16                 # fp16 operands: rotation on the fp32 accumulators, one rounding
    if out is None:
        out = torch.empty((M, N), dtype=opd, device=a.device)
    name = _GEMM_NT[opd]
    ev = _timer and _begin(name, 2.0 * M * N * K, (f"M={M}," if _TAG_M else "") + f"N={N},K={K},epi=3")
    _call("grit_" + name + "_rope", _chk(a, opd, "a", 2), _chk(w, opd, "w", 2), _chk(out, opd, "out", 2), M, N, K, a.stride(0), w.stride(0),
          out.stride(0), _chk(cos, F32, "cos"), _chk(sin, F32, "sin"), _opt(positions, I32, "positions"), int(S), cos.shape[0], int(rope_cols), _stream())
    if ev:
        ev.record()
    return out


def _grouped_out(a, w, m_total: int, epilogue: int, out, dtype):
    """(out [m_total, columns under ``epilogue``], allocated when absent; E, N, K) of a grouped GEMM over ``w [E,N,K]``."""
    E, N, K = w.shape
    assert a.shape[1] == K
    n_out = _epi_cols(N, epilogue)
    if out is None:
        out = torch.empty((m_total, n_out), dtype=dtype, device=a.device)
    assert out.shape == (m_total, n_out)
    return out, E, N, K


def gemm_nt_grouped(a: torch.Tensor, w: torch.Tensor, counts: torch.Tensor, m_total: int, out: torch.Tensor | None = None,
                    epilogue: int = EPI_STORE, a_rows: torch.Tensor | None = None) -> torch.Tensor:
    """Grouped GEMM over ``w [E,N,K]``: sorted row r (group by group, ``counts`` int32 [E] on the device) is
    a[a_rows[r]] @ w[g]^T.  ``m_total`` = number of sorted rows (2T for top-2 routing).  fp16 ``a`` / ``w`` / ``out``: the fp16
    instantiation (the "f16_operands" policy of the MoE engine; STORE, SWIGLU, SWIGLU_STACKED)."""
    opd = F16 if a.dtype == F16 else BF16
    out, E, N, K = _grouped_out(a, w, m_total, epilogue, out, opd)
    name = _GEMM_NT[opd] + "_grouped"
    ev = _timer and _begin(name, 2.0 * m_total * N * K)
    _call("grit_" + name, _chk(a, opd, "a", 2), _opt(a_rows, I32, "a_rows"), _chk(w, opd, "w", 3), _chk(out, opd, "out", 2), _chk(counts, I32, "counts"),
          E, m_total, N, K, a.stride(0), w.stride(1), w.stride(0), out.stride(0), epilogue, _stream())
    if ev:
        ev.record()
    return out


def gemm_nt_grouped_epi(a: torch.Tensor, w: torch.Tensor, counts: torch.Tensor, m_total: int, epilogue: int, out: torch.Tensor | None = None,
                        residual: torch.Tensor | None = None, a_rows: torch.Tensor | None = None) -> torch.Tensor:
    """Grouped GEMM over ``w [E,N,K]`` with the training epilogues (see grit_gemm_bf16_nt_grouped_epi): STORE / SWIGLU* give
    ``out [m_total, N or N/2]``; SWIGLU_STACKED_SAVE also fills ``residual [m_total, N]`` with [gate | up]; SWIGLU_BWD reads the saved
    ``residual [m_total, 2N]`` and gives ``out [m_total, 2N]`` = [d_gate | d_up]."""
    out, E, N, K = _grouped_out(a, w, m_total, epilogue, out, BF16)
    if epilogue in (EPI_SWIGLU_STACKED_SAVE, EPI_SWIGLU_BWD):
        need = 2 * N if epilogue == EPI_SWIGLU_BWD else N
        assert residual is not None and tuple(residual.shape) == (m_total, need), "residual: [m_total, N] (SAVE) / [m_total, 2N] (BWD)"
    ev = _timer and _begin("gemm_bf16_nt_grouped", 2.0 * m_total * N * K)
    pa, par, pw, po = _chk(a, BF16, "a", 2), _opt(a_rows, I32, "a_rows"), _chk(w, BF16, "w", 3), _chk(out, BF16, "out", 2)
    rp, ldr = _opt(residual, BF16, "residual", True)
    _call("grit_gemm_bf16_nt_grouped_epi", pa, par, pw, po, rp, _chk(counts, I32, "counts"), E, m_total, N, K, a.stride(0), w.stride(1), w.stride(0),
          out.stride(0), ldr, epilogue, _stream())
    if ev:
        ev.record()
    return out


def moe_combine_bwd(dout: torch.Tensor, y: torch.Tensor, row_token: torch.Tensor, rows: torch.Tensor, weights: torch.Tensor):
    """Backward of moe_combine: (dy [2T,H] bf16 = w * dout[token], dw [T,2] fp32 = <y, dout[token]>)."""
    T, H = dout.shape
    dy = torch.empty((2 * T, H), dtype=BF16, device=dout.device)
    dw = torch.empty((T, 2), dtype=F32, device=dout.device)
    _call("grit_moe_combine_bwd", _chk(dout, BF16, "dout"), _chk(y, BF16, "y"), _chk(row_token, I32, "row_token"), _chk(rows, I32, "rows"),
          _chk(weights, F32, "weights"), dy.data_ptr(), dw.data_ptr(), T, H, _stream())
    return dy, dw


def moe_router_bwd(x: torch.Tensor, gate_w: torch.Tensor, experts: torch.Tensor, dw: torch.Tensor, dx_in: torch.Tensor | None,
                   gate_grad: torch.Tensor, aux_dlogits: torch.Tensor | None = None, return_dlogits: bool = False):
    """Backward of the router (softmax -> top-2 -> renormalise through the gate Linear): returns dx [T,H] bf16 = dx_in + dlogits @ gate_w and
    accumulates gate_grad [E,H] bf16 += bf16(dlogits^T @ x).  dw [T,2] fp32 comes from moe_combine_bwd; aux_dlogits [T,E] fp32 optional."""
    T, H = x.shape
    E = gate_w.shape[0]
    dlogits = torch.empty((T, E), dtype=F32, device=x.device)
    dx = torch.empty((T, H), dtype=BF16, device=x.device)
    _call("grit_moe_router_bwd", _chk(x, BF16, "x"), _chk(gate_w, BF16, "gate_w"), _chk(experts, I32, "experts"), _chk(dw, F32, "dw"),
          _opt(aux_dlogits, F32, "aux_dlogits"), _opt(dx_in, BF16, "dx_in"), dx.data_ptr(), dlogits.data_ptr(), T, H, E, _stream())
    ws = torch.empty((int(_lib.load().grit_moe_router_wgrad_workspace_floats(T, H, E)),), dtype=F32, device=x.device)
    _call("grit_moe_router_wgrad", _chk(x, BF16, "x"), dlogits.data_ptr(), _chk(gate_grad, BF16, "gate_grad"), ws.data_ptr(), T, H, E, _stream())
    return (dx, dlogits) if return_dlogits else dx


def _router_top2(f32: bool, x, gate_w, experts, weights, ln_w=None, eps: float = 0.0):
    """The two routers: the reference's on normalised bf16 rows, or (``f32``) the fp16-operand policy's on the fp32 residual stream
    itself, with the RMSNorm (``ln_w``, ``eps``) folded in.  The caller says which: moe_router_top2 goes by x's format, moe_route and
    moe_route_f32 each by their own, so that either still refuses rows of the other format."""
    T, H = x.shape
    E = gate_w.shape[0]
    if f32:
        _call("grit_moe_router_top2_f32", _chk(x, F32, "h"), _chk(ln_w, BF16, "ln_w"), float(eps), _chk(gate_w, BF16, "gate_w"),
              _chk(experts, I32, "experts"), _chk(weights, F32, "weights"), T, H, E, _stream())
    else:
        _call("grit_moe_router_top2", _chk(x, BF16, "x"), _chk(gate_w, BF16, "gate_w"), _chk(experts, I32, "experts"), _chk(weights, F32, "weights"),
              T, H, E, _stream())


def _route(f32: bool, x, gate_w, ln_w=None, eps: float = 0.0):
    """Routing with the index built: the five buffers, the router, grit_moe_index."""
    T, E, dev = x.shape[0], gate_w.shape[0], x.device
    experts = torch.empty((T, 2), dtype=I32, device=dev)
    weights = torch.empty((T, 2), dtype=F32, device=dev)
    counts = torch.empty((E,), dtype=I32, device=dev)
    row_token = torch.empty((2 * T,), dtype=I32, device=dev)
    rows = torch.empty((T, 2), dtype=I32, device=dev)
    _router_top2(f32, x, gate_w, experts, weights, ln_w, eps)
    ws = torch.empty((int(_lib.load().grit_moe_index_workspace_ints(T, E)),), dtype=I32, device=dev)
    _call("grit_moe_index", experts.data_ptr(), T, E, counts.data_ptr(), row_token.data_ptr(), rows.data_ptr(), ws.data_ptr(), _stream())
    return experts, weights, counts, row_token, rows


def moe_route(x: torch.Tensor, gate_w: torch.Tensor):
    """Top-2 routing of x [T,H] -> (experts [T,2] i32, weights [T,2] f32, counts [E] i32, row_token [2T] i32, rows [T,2] i32)."""
    return _route(False, x, gate_w)


_MOE_COMBINE = _entries("grit_moe_combine{_fmt}")


def moe_combine(y: torch.Tensor, rows: torch.Tensor, weights: torch.Tensor, residual: torch.Tensor | None, out: torch.Tensor | None = None):
    """out[t] = residual[t] + w[t,0] y[rows[t,0]] + w[t,1] y[rows[t,1]].  bf16 y / residual / out: the reference's bf16 rounding points;
    fp16 y with an fp32 residual / out: the "f16_operands" policy (fp32 arithmetic, nothing rounded)."""
    T = rows.shape[0]
    H = y.shape[1]
    ydt, odt = (F16, F32) if y.dtype == F16 else (BF16, BF16)
    if out is None:
        out = torch.empty((T, H), dtype=odt, device=y.device)
    _call(_MOE_COMBINE[odt], _chk(y, ydt, "y"), _chk(rows, I32, "rows"), _chk(weights, F32, "weights"),
          _opt(residual, odt, "residual"), _chk(out, odt, "out"), T, H, _stream())
    return out


def moe_route_f32(h: torch.Tensor, ln_w: torch.Tensor, eps: float, gate_w: torch.Tensor):
    """moe_route for the "f16_operands" policy: the routing decision is taken in fp32 on the residual stream h [T,H] itself (the
    post-attention RMSNorm folded in, nothing rounded: grit_moe_router_top2_f32).  Same return tuple as moe_route."""
    return _route(True, h, gate_w, ln_w, eps)


def f16_overflow_flag(device, clear: bool = True) -> bool:
    """True when a kernel of the f16_operands policy stored an inf / nan on ``device`` since the last clear.  Waits for the device's
    current stream (one 4-byte D2H copy): call it once per encode, next to the copy of the embeddings."""
    flag = ctypes.c_int(0)
    with torch.cuda.device(device):
        _call("grit_f16_overflow_flag", ctypes.byref(flag), int(clear), _stream())
    return bool(flag.value)


def mask_pack(mask: torch.Tensor) -> torch.Tensor:
    B, S = mask.shape
    bits = torch.empty((B, (S + 63) // 64), dtype=I64, device=mask.device)   # uint64 payload in int64 storage
    _call("grit_mask_pack", _chk(mask, I64, "mask"), _chk(bits, I64, "bits"), B, S, _stream())
    return bits


def attn_bidir(qkv: torch.Tensor, key_bits: torch.Tensor, B: int, S: int, nq: int, nkv: int, d: int,
               out: torch.Tensor | None = None, lse: torch.Tensor | None = None, scale: float | None = None,
               causal: bool = False, window: int = 0) -> torch.Tensor:
    assert qkv.shape[0] == B * S
    return _attn_fwd(False, qkv, key_bits, "key_bits", (B, S), 4.0 * B * nq * S * S * d, nq, nkv, d, out, scale, lse, causal, window)


def pool_norm(hidden: torch.Tensor, mask: torch.Tensor, method: str, normalize: bool, instr_len: torch.Tensor | None = None,
              inv_norm: torch.Tensor | None = None) -> torch.Tensor:
    return _pool_fwd(False, hidden, mask, tuple(hidden.shape), method, normalize, instr_len, inv_norm)


def pool_norm_bwd(y: torch.Tensor, dy: torch.Tensor, inv_norm: torch.Tensor | None, mask: torch.Tensor, method: str, normalize: bool,
                  S: int, instr_len: torch.Tensor | None = None) -> torch.Tensor:
    B, H = y.shape
    return _pool_bwd(False, y, dy, inv_norm, mask, (B, S, H), (B, S, H), method, normalize, instr_len)


def infonce(q: torch.Tensor, p: torch.Tensor, temperature: float, q_off: int = 0, nq_loc: int | None = None, p_off: int = 0,
            np_loc: int | None = None, want_grad: bool = True):
    """Returns (loss[1] fp32, dq [nq_loc,H] | None, dp [np_loc,H] | None)."""
    Nq, H = q.shape
    Np = p.shape[0]
    nq_loc = Nq if nq_loc is None else nq_loc
    np_loc = Np if np_loc is None else np_loc
    scores = torch.empty((Nq, Np), dtype=F32, device=q.device)
    loss_buf = torch.empty((1 + Nq,), dtype=F32, device=q.device)        # [0] mean loss, [1 + i] the term of row i
    loss, loss_rows = loss_buf[:1], loss_buf[1:]
    dq = torch.empty((nq_loc, H), dtype=F32, device=q.device) if want_grad else None
    dp = torch.empty((np_loc, H), dtype=F32, device=q.device) if want_grad else None
    _call("grit_infonce_rows_fwd_bwd", _chk(q, F32, "q"), _chk(p, F32, "p"), 1.0 / float(temperature), _chk(scores, F32, "scores"),
          _chk(loss, F32, "loss"), _chk(loss_rows, F32, "loss_rows"), 0 if dq is None else dq.data_ptr(), 0 if dp is None else dp.data_ptr(),
          Nq, Np, H, q_off, nq_loc, p_off, np_loc, _stream())
    return loss, dq, dp


def transpose(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """[R,C] -> [C,R]; ``out`` may be a wider buffer [C, >=R] (zero-padded K for the wgrad GEMM)."""
    R, Cc = x.shape
    ret_view = None
    if out is None:
        out = torch.empty((Cc, (R + 7) // 8 * 8), dtype=BF16, device=x.device)
        ret_view = out if out.shape[1] == R else out[:, :R]
    assert out.shape[0] == Cc and out.shape[1] >= R and x.stride(1) == 1 and out.stride(1) == 1
    if x.dtype != BF16 or out.dtype != BF16 or not x.is_cuda:
        raise TypeError("transpose: bf16 CUDA tensors expected")
    _call("grit_transpose_bf16", x.data_ptr(), out.data_ptr(), R, Cc, x.stride(0), out.stride(0), _stream())
    return out if ret_view is None else ret_view


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float, dw: torch.Tensor, dres: torch.Tensor | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """dx (+ dres) -> out; dw [H] fp32 += sum_t dy * xhat."""
    H = x.shape[-1]
    T = x.numel() // H
    if out is None:
        out = torch.empty_like(x)
    part = torch.empty((_lib.load().grit_rmsnorm_bwd_workspace_rows(T), H), dtype=F32, device=x.device)
    _call("grit_rmsnorm_bwd", _chk(dy, BF16, "dy"), _chk(x, BF16, "x"), _chk(w, BF16, "w"), _opt(dres, BF16, "dres"), _chk(out, BF16, "dx"),
          part.data_ptr(), _chk(dw, F32, "dw"), T, H, float(eps), _stream())
    return out


def swiglu(gu: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    T, I2 = gu.shape
    I = I2 // 2
    if out is None:
        out = torch.empty((T, I), dtype=BF16, device=gu.device)
    _call("grit_swiglu_fwd", _chk(gu, BF16, "gu"), _chk(out, BF16, "act"), T, I, _stream())
    return out


def swiglu_bwd(gu: torch.Tensor, dact: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    T, I2 = gu.shape
    if out is None:
        out = torch.empty_like(gu)
    _call("grit_swiglu_bwd", _chk(gu, BF16, "gu"), _chk(dact, BF16, "dact"), _chk(out, BF16, "dgu"), T, I2 // 2, _stream())
    return out


def _attn_bwd(varlen: bool, qkv, layout, layout_name: str, sizes: tuple, delta_shape: tuple, out, dout, lse, nq: int, nkv: int, d: int, dqkv, scale,
              causal: bool, window: int):
    """What the padded and the packed backward share: ``sizes`` is (B, S) or (B, max_len, T); delta is the kernels' scratch."""
    stride = qkv.shape[1]
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    if scale is None:
        scale = d ** -0.5
    delta = torch.empty(delta_shape, dtype=F32, device=qkv.device)
    name, wa = _attn_entry("bwd", varlen, causal, window)
    _call(name, _chk(qkv, BF16, "qkv"), _chk(layout, I32 if varlen else I64, layout_name), _chk(out, BF16, "out"), _chk(dout, BF16, "dout"),
          _chk(lse, F32, "lse"), delta.data_ptr(), _chk(dqkv, BF16, "dqkv"), *sizes, nq, nkv, d, stride, out.stride(0), float(scale), *wa, _stream())
    return dqkv


def attn_bidir_bwd(qkv: torch.Tensor, key_bits: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, B: int, S: int,
                   nq: int, nkv: int, d: int, dqkv: torch.Tensor | None = None, scale: float | None = None,
                   causal: bool = False, window: int = 0) -> torch.Tensor:
    return _attn_bwd(False, qkv, key_bits, "key_bits", (B, S), (B, nq, S), out, dout, lse, nq, nkv, d, dqkv, scale, causal, window)


def attn_bidir_varlen_bwd(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, out: torch.Tensor, dout: torch.Tensor,
                          lse: torch.Tensor, nq: int, nkv: int, d: int, dqkv: torch.Tensor | None = None,
                          scale: float | None = None, causal: bool = False, window: int = 0) -> torch.Tensor:
    T = qkv.shape[0]
    return _attn_bwd(True, qkv, cu_seqlens, "cu_seqlens", (cu_seqlens.numel() - 1, int(max_len), T), (T, nq), out, dout, lse, nq, nkv, d, dqkv,
                     scale, causal, window)


def _proj_args(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None, epilogue: int, ln_w: torch.Tensor | None = None, eps: float = 0.0):
    """What the decode projections (gemv, decode_gemm and their rmsnorm forms) share: out [B, N] (N // 2 under SWIGLU) in the format the
    weights and the epilogue give (bf16 weights: bf16; fp16 weights: fp32, under SWIGLU the fp16 activation), allocated when absent, and
    the checked head of the C argument list: x, [ln_w, eps,] w, out, B, N, K, ldx, ldw, ldo, epilogue.  Returns (out, operand format, head)."""
    B, K = x.shape
    N = w.shape[0]
    op, odt = (F16, F16 if epilogue == EPI_SWIGLU else F32) if w.dtype == F16 else (BF16, BF16)
    if out is None:
        out = torch.empty((B, _epi_cols(N, epilogue)), dtype=odt, device=x.device)
    norm = [] if ln_w is None else [_chk(ln_w, BF16, "ln_w"), float(eps)]
    return out, op, [_chk(x, op, "x", 2), *norm, _chk(w, op, "w", 2), _chk(out, odt, "out", 2), B, N, K, x.stride(0), w.stride(0), out.stride(0), epilogue]


def _proj(entries: dict, x, w, out, epilogue: int, residual, out16):
    """gemv and decode_gemm: the bf16 entry takes (residual, ldr) behind the head, the fp16 entry (out16, ldo16) as well."""
    out, op, args = _proj_args(x, w, out, epilogue)
    if op == F16:
        _call(entries[op], *args, *_opt(residual, F32, "residual", True), *_opt(out16, F16, "out16", True), _stream())
    else:
        _call(entries[op], *args, *_opt(residual, BF16, "residual", True), _stream())
    return out


_GEMV, _GEMV_EXPERT, _DECODE_GEMM = _entries("grit_gemv_{fmt}"), _entries("grit_gemv_{fmt}_expert"), _entries("grit_decode_gemm_{fmt}")
_RMSNORM_GEMV, _RMSNORM_GEMV_DEFERRED = _entries("grit_rmsnorm_gemv_{fmt}"), _entries("grit_rmsnorm_gemv_{fmt}_deferred")
_RMSNORM_DECODE_GEMM = _entries("grit_rmsnorm_decode_gemm_{fmt}_deferred")


def gemv(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None, epilogue: int = EPI_STORE,
         residual: torch.Tensor | None = None, out16: torch.Tensor | None = None) -> torch.Tensor:
    """out[B,N] = x[B,K] @ w[N,K]^T for B <= 8 rows (decode); same epilogues as gemm_nt.  fp16 ``w`` (and ``x``): the fp16-operand form --
    STORE / RESIDUAL write fp32 (``residual`` is the fp32 stream; ``out16``: additionally its fp16 rounding, the next GEMV's operand),
    SWIGLU writes the fp16 activation."""
    return _proj(_GEMV, x, w, out, epilogue, residual, out16)


def gemv_expert(x: torch.Tensor, w_stack: torch.Tensor, expert: torch.Tensor, out: torch.Tensor | None = None, epilogue: int = EPI_STORE) -> torch.Tensor:
    """x [B,K] @ w_stack[expert[0]]^T for a stack [E,N,K]: the expert index is read on the DEVICE (``expert``: an int32 tensor or view whose
    first element is the index), so a sparse-MoE decode step can be captured in a graph; the kernel clamps the index to [0, E).  STORE / SWIGLU;
    fp16 stack: the fp16 formats."""
    B, K = x.shape
    E, N, _ = w_stack.shape
    op, odt = (F16, F16 if epilogue == EPI_SWIGLU else F32) if w_stack.dtype == F16 else (BF16, BF16)
    if out is None:
        out = torch.empty((B, _epi_cols(N, epilogue)), dtype=odt, device=x.device)
    if expert.dtype != I32 or not expert.is_cuda:
        raise TypeError("gemv_expert: expert must be an int32 CUDA tensor")
    _call(_GEMV_EXPERT[op], _chk(x, op, "x", 2), _chk(w_stack, op, "w_stack", 3), _chk(out, odt, "out", 2), expert.data_ptr(),
          w_stack.stride(0), E, B, N, K, x.stride(0), w_stack.stride(1), out.stride(0), epilogue, _stream())
    return out


def moe_decode_combine_f32(h: torch.Tensor, h16: torch.Tensor, y: torch.Tensor, weights: torch.Tensor):
    """h[b] += weights[b,0] y[2b] + weights[b,1] y[2b+1] (fp32, in place) and h16 = fp16(h): the sparse-MoE decode step on fp16 operands."""
    B, H = h.shape
    _call("grit_moe_decode_combine_f32", _chk(h, F32, "h"), _chk(h16, F16, "h16"), _chk(y, F32, "y"), _chk(weights, F32, "weights"), B, H, _stream())


def moe_router_top2(x: torch.Tensor, gate_w: torch.Tensor, experts: torch.Tensor, weights: torch.Tensor, ln_w: torch.Tensor | None = None,
                    eps: float = 0.0):
    """The routing decision alone into caller-owned buffers (experts [T,2] int32, weights [T,2] fp32) -- no index building, no host
    round trip: the sparse-MoE decode step.  bf16 x: the reference's router on the normalised bf16 rows; fp32 x with ``ln_w``: the
    fp16-operand policy's router on the residual stream itself (norm folded in, nothing rounded)."""
    _router_top2(x.dtype == F32, x, gate_w, experts, weights, ln_w, eps)


def rmsnorm_gemv(x: torch.Tensor, ln_w: torch.Tensor, eps: float, w: torch.Tensor, out: torch.Tensor | None = None,
                 epilogue: int = EPI_STORE, deferred: bool = False) -> torch.Tensor:
    """gemv(rmsnorm(x, ln_w, eps), w) in one launch (decode step).  ``deferred``: the row scale multiplies the finished dot products
    (no pass over x in front of the weight stream; x_n is not rounded to bf16: not the bits of the two launches).  fp16 ``w``: x is the
    fp16 copy of the residual stream, the deferred form only; STORE writes fp32, SWIGLU the fp16 activation."""
    if w.dtype == F16 and not deferred:
        raise ValueError("rmsnorm_gemv on fp16 weights: the deferred form only")
    out, op, args = _proj_args(x, w, out, epilogue, ln_w, eps)
    _call((_RMSNORM_GEMV_DEFERRED if deferred else _RMSNORM_GEMV)[op], *args, _stream())
    return out


def decode_gemm(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None, epilogue: int = EPI_STORE,
                residual: torch.Tensor | None = None, out16: torch.Tensor | None = None) -> torch.Tensor:
    """out[B,N] = x[B,K] @ w[N,K]^T for 1..64 rows on the MFMA (batched decode: the step's projections above 8 rows); the epilogues and
    formats of ``gemv`` (fp16 ``w``: STORE / RESIDUAL write fp32, ``out16`` the fp16 copy, SWIGLU the fp16 activation).  A row's output
    does not depend on B or on the other rows, bit for bit; it differs from ``gemv``'s in the last bits (another summation order)."""
    return _proj(_DECODE_GEMM, x, w, out, epilogue, residual, out16)


def rmsnorm_decode_gemm(x: torch.Tensor, ln_w: torch.Tensor, eps: float, w: torch.Tensor, out: torch.Tensor | None = None,
                        epilogue: int = EPI_STORE) -> torch.Tensor:
    """decode_gemm with the DEFERRED RMSNorm of x folded in (the row scale multiplies the finished fp32 sums; x * ln_w is rounded once to
    the operand format for the MFMA).  1..64 rows; STORE or SWIGLU; fp16 ``w``: x is the fp16 copy of the stream, STORE writes fp32."""
    out, op, args = _proj_args(x, w, out, epilogue, ln_w, eps)
    _call(_RMSNORM_DECODE_GEMM[op], *args, _stream())
    return out


def rope_kv_append(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor,
                   nq: int, nkv: int, d: int):
    B, _, Lmax, _ = cache_k.shape
    assert cos.shape[0] >= Lmax
    _call("grit_rope_kv_append", _chk(qkv, BF16, "qkv", 2), _chk(cos, F32, "cos"), _chk(sin, F32, "sin"), _chk(cache_k, BF16, "cache_k"),
          _chk(cache_v, BF16, "cache_v"), _chk(lens, I32, "lens"), B, nq, nkv, d, Lmax, qkv.stride(0), _stream())


def kv_append(qkv: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor, nq: int, nkv: int, d: int):
    B, _, Lmax, _ = cache_k.shape
    _call("grit_kv_append", _chk(qkv, BF16, "qkv", 2), _chk(cache_k, BF16, "cache_k"), _chk(cache_v, BF16, "cache_v"), _chk(lens, I32, "lens"),
          B, nq, nkv, d, Lmax, qkv.stride(0), _stream())


def attn_decode_workspace(B: int, nq: int, nkv: int, Lmax: int, device) -> torch.Tensor:
    return torch.empty((int(_lib.load().grit_attn_decode_workspace_floats(B, nq, nkv, Lmax)),), dtype=F32, device=device)


def attn_decode(q: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor, out: torch.Tensor, workspace: torch.Tensor,
                nq: int, nkv: int, d: int, scale: float | None = None):
    B, _, Lmax, _ = cache_k.shape
    _call("grit_attn_decode", _chk(q, BF16, "q", 2), _chk(cache_k, BF16, "cache_k"), _chk(cache_v, BF16, "cache_v"), _chk(lens, I32, "lens"),
          _chk(out, BF16, "out", 2), _chk(workspace, F32, "workspace"), B, nq, nkv, d, Lmax, q.stride(0), out.stride(0),
          float(d ** -0.5 if scale is None else scale), _stream())
    return out


_ATTN_DECODE_ROPE, _ATTN_PREFILL_CACHED = _entries("grit_attn_decode_rope{_fmt}"), _entries("grit_attn_prefill_cached{_fmt}_fwd")


def attn_decode_rope(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor,
                     out: torch.Tensor, workspace: torch.Tensor, nq: int, nkv: int, d: int, scale: float | None = None):
    """rope_kv_append + attn_decode in one launch (qkv: the raw fused projection of the new token; the caches are appended to)."""
    B, _, Lmax, _ = cache_k.shape
    assert cos.shape[0] >= Lmax
    dt, qdt = (F16, F32) if cache_k.dtype == F16 else (BF16, BF16)  # fp16-operand form: fp32 q|k|v row, fp16 caches and ctx
    _call(_ATTN_DECODE_ROPE[dt], _chk(qkv, qdt, "qkv", 2), _chk(cos, F32, "cos"), _chk(sin, F32, "sin"), _chk(cache_k, dt, "cache_k"),
          _chk(cache_v, dt, "cache_v"), _chk(lens, I32, "lens"), _chk(out, dt, "out", 2), _chk(workspace, F32, "workspace"), B, nq, nkv, d, Lmax,
          qkv.stride(0), out.stride(0), float(d ** -0.5 if scale is None else scale), _stream())
    return out


def rope_kv_append_rows(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor,
                        cache_row: torch.Tensor, nq: int, nkv: int, d: int):
    """rope_kv_append for V rows that are tokens of the caches' B <= V sequences (row v: sequence cache_row[v], position lens[v]); fp16
    caches: the fp16-operand formats (fp32 rows)."""
    V = qkv.shape[0]
    _, _, Lmax, _ = cache_k.shape
    f16 = cache_k.dtype == F16
    assert cos.shape[0] >= Lmax and lens.numel() == V and cache_row.numel() == V
    _call("grit_rope_kv_append_rows", _chk(qkv, F32 if f16 else BF16, "qkv", 2), _chk(cos, F32, "cos"), _chk(sin, F32, "sin"),
          _chk(cache_k, cache_k.dtype, "cache_k"), _chk(cache_v, cache_k.dtype, "cache_v"), _chk(lens, I32, "lens"), _chk(cache_row, I32, "cache_row"),
          V, nq, nkv, d, Lmax, qkv.stride(0), int(f16), _stream())


def attn_decode_rows(q: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor, cache_row: torch.Tensor, out: torch.Tensor,
                     workspace: torch.Tensor, nq: int, nkv: int, d: int, scale: float | None = None):
    """attn_decode for V rows that are tokens of the caches' sequences: row v attends to keys 0 .. lens[v] of sequence cache_row[v]."""
    V = q.shape[0]
    _, _, Lmax, _ = cache_k.shape
    f16 = cache_k.dtype == F16
    _call("grit_attn_decode_rows", _chk(q, F32 if f16 else BF16, "q", 2), _chk(cache_k, cache_k.dtype, "cache_k"), _chk(cache_v, cache_k.dtype, "cache_v"),
          _chk(lens, I32, "lens"), _chk(cache_row, I32, "cache_row"), _chk(out, F16 if f16 else BF16, "out", 2), _chk(workspace, F32, "workspace"),
          V, nq, nkv, d, Lmax, q.stride(0), out.stride(0), float(d ** -0.5 if scale is None else scale), int(f16), _stream())
    return out


def kv_append_chunk(qkv: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor, plen: torch.Tensor, nq: int, nkv: int,
                    d: int):
    """The k / v heads of a prompt chunk's fused q|k|v rows [B*P, stride] (post-RoPE) -> cache rows lens[b] + i, i < plen[b]; the rows
    and the caches [B,nkv,Lmax,d] share one 16-bit format (bf16, or fp16 under the fp16 policies)."""
    B, _, Lmax, _ = cache_k.shape
    T = qkv.shape[0]
    dt = cache_k.dtype
    assert T % B == 0 and lens.numel() == B and plen.numel() == B
    _call("grit_kv_append_chunk", _chk(qkv, dt, "qkv", 2), _chk(cache_k, dt, "cache_k"), _chk(cache_v, dt, "cache_v"), _chk(lens, I32, "lens"),
          _chk(plen, I32, "plen"), B, T // B, nq, nkv, d, Lmax, qkv.stride(0), _stream())


def attn_prefill_cached(q: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor, plen: torch.Tensor, nq: int, nkv: int,
                        d: int, out: torch.Tensor | None = None, scale: float | None = None) -> torch.Tensor:
    """Attention of a prompt chunk over the cache: ``q`` [B*P, stride] (the fused q|k|v rows: the q heads are read), query (b, i) attends to
    keys 0 .. lens[b] + i of sequence b; rows i >= plen[b] come back as zeros.  bf16 or fp16 (the caches' format)."""
    B, _, Lmax, _ = cache_k.shape
    T = q.shape[0]
    dt = cache_k.dtype
    assert T % B == 0 and lens.numel() == B and plen.numel() == B
    if out is None:
        out = torch.empty((T, nq * d), dtype=dt, device=q.device)
    # (work: the keys each valid query sees, lens[b] + i + 1 -- device data, read after the timed region)
    ev = _timer and _begin("attn_prefill_cached", (4.0 * nq * d * plen.double() * (lens.double() + (plen.double() + 1) / 2)).sum())
    _call(_ATTN_PREFILL_CACHED[F16 if dt == F16 else BF16], _chk(q, dt, "q", 2), _chk(cache_k, dt, "cache_k"),
          _chk(cache_v, dt, "cache_v"), _chk(lens, I32, "lens"), _chk(plen, I32, "plen"), _chk(out, dt, "out", 2), B, T // B, nq, nkv, d, Lmax,
          q.stride(0), out.stride(0), float(d ** -0.5 if scale is None else scale), _stream())
    if ev:
        ev.record()
    return out


_ARGMAX_ADVANCE, _SAMPLE_ADVANCE = _entries("grit_argmax_advance{_fmt}"), _entries("grit_sample_advance{_fmt}")


def _advance_head(logits, dt, next_ids, lens, history, step) -> list:
    """The ten leading arguments of grit_argmax_advance and grit_sample_advance: logits, ld, V, next, lens, history, its stride, step, B, stream."""
    B, V = logits.shape
    return [_chk(logits, dt, "logits", 2), logits.stride(0), V, _chk(next_ids, I64, "next"), _opt(lens, I32, "lens"), _opt(history, I64, "history"),
            0 if history is None else history.stride(0), _opt(step, I32, "step"), B, _stream()]


def argmax_advance(logits: torch.Tensor, next_ids: torch.Tensor, lens: torch.Tensor | None = None, history: torch.Tensor | None = None,
                   step: torch.Tensor | None = None):
    dt = F32 if logits.dtype == F32 else BF16
    _call(_ARGMAX_ADVANCE[dt], *_advance_head(logits, dt, next_ids, lens, history, step))
    return next_ids


def sample_advance(logits: torch.Tensor, next_ids: torch.Tensor, keys: torch.Tensor, temperature: float, top_k: int, top_p: float,
                   lens: torch.Tensor | None = None, history: torch.Tensor | None = None, step: torch.Tensor | None = None):
    """argmax_advance with a sampled token (grit_sample_advance[_f32]: temperature, top-k, top-p, Gumbel-max on Philox noise; semantics
    and RNG contract in include/gritlm_hip.h).  ``keys``: int64 [B] row keys on the device (the bits of the uint64 keys); bf16 or fp32 logits."""
    B = logits.shape[0]
    dt = F32 if logits.dtype == F32 else BF16
    if keys.numel() != B or next_ids.numel() < B or (lens is not None and lens.numel() < B) or (history is not None and history.shape[0] < B):
        raise ValueError(f"sample_advance: {B} rows need B keys, next ids, lens and history rows")
    _call(_SAMPLE_ADVANCE[dt], *_advance_head(logits, dt, next_ids, lens, history, step),
          float(temperature), min(int(top_k), 2 ** 31 - 1), float(top_p), _chk(keys, I64, "keys"))      # (top_k >= V keeps every token)
    return next_ids


def knn_topk(queries: torch.Tensor, embeddings: torch.Tensor, k: int, transposed: bool = False):
    """Brute-force inner-product search: (scores [Q,k] fp32 descending, indices [Q,k] int64).  ``embeddings`` is [N,H], or with
    ``transposed=True`` the reference index layout [H,N] (rag/index.py:141); any strides."""
    if queries.dtype != F32 or embeddings.dtype != F32:
        raise TypeError("knn_topk: fp32 tensors expected")
    Q, H = queries.shape
    N = embeddings.shape[1] if transposed else embeddings.shape[0]
    assert (embeddings.shape[0] if transposed else embeddings.shape[1]) == H
    sn, sh = (embeddings.stride(1), embeddings.stride(0)) if transposed else (embeddings.stride(0), embeddings.stride(1))
    ws = torch.empty((int(_lib.load().grit_knn_workspace_bytes(Q, N, k)),), dtype=torch.uint8, device=queries.device)
    scores = torch.empty((Q, k), dtype=F32, device=queries.device)
    index = torch.empty((Q, k), dtype=I64, device=queries.device)
    if not embeddings.is_cuda:
        raise _lib.GritHipError("knn_topk: tensors must live on the GPU; the native path has no CPU fallback")
    _call("grit_knn_topk", _chk(queries, F32, "queries"), embeddings.data_ptr(), Q, N, H, sn, sh, int(k), ws.data_ptr(), scores.data_ptr(),
          index.data_ptr(), _stream())
    return scores, index


def ce_fwd(logits: torch.Tensor, labels: torch.Tensor):
    """(lse [T], loss_row [T]) fp32 of bf16 logits [T,V] against int64 labels (-100 ignored)."""
    T, V = logits.shape
    lse = torch.empty((T,), dtype=F32, device=logits.device)
    loss_row = torch.empty((T,), dtype=F32, device=logits.device)
    _call("grit_ce_fwd", _chk(logits, BF16, "logits", 2), logits.stride(0), _chk(labels, I64, "labels"), lse.data_ptr(), loss_row.data_ptr(), T, V, _stream())
    return lse, loss_row


def ce_bwd_(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, scale: float, dev_scale: torch.Tensor | None = None):
    """In place: logits <- (softmax - onehot) * scale * dev_scale (bf16)."""
    T, V = logits.shape
    _call("grit_ce_bwd", _chk(logits, BF16, "logits", 2), logits.stride(0), _chk(labels, I64, "labels"), _chk(lse, F32, "lse"),
          _opt(dev_scale, F32, "dev_scale"), float(scale), T, V, _stream())
    return logits


def embed_scatter_add(dh: torch.Tensor, ids: torch.Tensor, grad: torch.Tensor):
    """Embedding weight gradient: grad[ids[t]] += dh[t] (bf16 table, fp32 sums in token order; deterministic, no atomics).  The stable
    sort of the ids is index plumbing and stays in torch."""
    V, H = grad.shape
    T = ids.numel()
    sorted_ids, order = torch.sort(ids.reshape(-1).clamp(0, V - 1), stable=True)
    _call("grit_embed_scatter_add_sorted", _chk(dh, BF16, "dh"), _chk(sorted_ids, I64, "sorted_ids"), _chk(order, I64, "order"),
          _chk(grad, BF16, "grad"), T, H, V, _stream())
    return grad


def accum_bf16_from_f32(acc: torch.Tensor, x: torch.Tensor):
    assert acc.numel() == x.numel()
    _call("grit_accum_bf16_from_f32", _chk(acc, BF16, "acc"), _chk(x, F32, "x"), acc.numel(), _stream())
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# Device guard.  A HIP launch goes to the calling thread's CURRENT device and `_stream()` is that device's current stream, while the
# reference API lets the caller put the model anywhere (GritLM(..., device="cuda:1"), gritlm/gritlm.py:24,57): every public op therefore
# runs with the device of its first tensor argument made current, so kernels, the stream they are ordered on and torch's own ops on
# that tensor all agree.  (One `current_device()` read per call when the devices already match.)
def _on_tensor_device(fn):
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        for a in (*args, *kwargs.values()):          # first tensor, positional or keyword
            if torch.is_tensor(a):
                if a.is_cuda and a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return guarded


# Every public function of this module that launches kernels is wrapped; host-only helpers are listed, so a new op is guarded by default
# and tests/test_abi.py::test_every_public_op_is_device_guarded fails if a launcher slips through.
_HOST_ONLY = ("set_timer", "check", "attn_decode_workspace", "f16_overflow_flag")
for _name, _fn in list(globals().items()):
    if callable(_fn) and getattr(_fn, "__module__", None) == __name__ and not _name.startswith("_") and not isinstance(_fn, type) \
            and _name not in _HOST_ONLY:
        globals()[_name] = _on_tensor_device(_fn)
        globals()[_name]._device_guarded = True
del _name, _fn
