"""Launchers of include/gritlm_hip_prefix.h: decode attention of B = B0 n rows over ONE copy of each sequence's prefix K/V plus a short
per-row tail (``MistralDecoder.generate(num_return_sequences=n, share_prefix=True)``).  Beside ``ops.py`` rather than in it, as
``index_ops.py`` is: the set of public launchers there is pinned by a recorded call trace.

Formats: bf16 caches go with bf16 q|k|v rows; fp16 caches with fp32 q|k|v rows plus a fp16 copy ``q16`` of the rotated q heads (the
decode step's fp16-operand conventions).  Every launcher refuses operands that do not fit with ``ValueError`` before anything runs."""
from __future__ import annotations

import torch

from . import _lib
from .ops import _on_tensor_device

BF16, F16, F32, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name: str, tensors, *args):
    """entry point ``name`` on its C arguments and the current stream (the last argument of every launch), once every operand -- checked
    by then -- is known to live on the GPU"""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.GritHipError(f"{name}: tensors must live on the GPU (got {t.device}); the native path has no CPU fallback")
    rc = getattr(_lib.load(), name)(*args, _stream())
    if rc:
        _lib.check(rc, name)


def _ptr(t: torch.Tensor, dtype, name: str, rows: bool = False):
    """Pointer of a checked operand: contiguous, or with ``rows`` a matrix of contiguous rows (any row stride)."""
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if (t.dim() != 2 or t.stride(1) != 1) if rows else not t.is_contiguous():
        raise ValueError(f"{name}: a matrix of contiguous rows expected" if rows else f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _formats(cache: torch.Tensor, name: str):
    """(16-bit operand format, format of the q|k|v rows, f16 flag) of a cache"""
    if cache.dtype not in (BF16, F16):
        raise ValueError(f"{name}: bf16 or fp16 expected, got {cache.dtype}")
    return (F16, F32, 1) if cache.dtype == F16 else (BF16, BF16, 0)


def _geometry(cache: torch.Tensor, name: str, d: int, nkv: int):
    if cache.dim() != 4 or cache.shape[1] != nkv or cache.shape[3] != d:
        raise ValueError(f"{name}: [rows, {nkv}, L, {d}] expected, got {tuple(cache.shape)}")
    return cache.shape[0], cache.shape[2]


def _rows_of(B: int, n: int, plen: torch.Tensor):
    if n < 1 or plen.numel() * n != B:
        raise ValueError(f"n * B0 != B: {n} rows per sequence, {plen.numel()} sequences (plen), {B} rows")


def _ws_fits(ws: torch.Tensor, B: int, nq: int, nkv: int, Lpre: int, Ltail: int, name: str):
    """the workspace holds the records of B rows at these lengths (launches 2 and 3 write all of them, launch 4 reads all of them)"""
    floats = int(_lib.load().grit_attn_decode_prefix_workspace_floats(B, nq, nkv, Lpre, Ltail))
    if floats <= 0 or ws.numel() < floats:
        raise ValueError(f"{name}: workspace of {ws.numel()} floats, {floats} needed (B={B}, nq={nq}, nkv={nkv}, Lpre={Lpre}, Ltail={Ltail}; "
                         "0: sizes not built)")


def kc() -> int:
    """keys per prefix chunk: a compile-time constant of the library"""
    return int(_lib.load().grit_attn_decode_prefix_kc())


def workspace(B: int, nq: int, nkv: int, Lpre: int, Ltail: int, device) -> torch.Tensor:
    floats = int(_lib.load().grit_attn_decode_prefix_workspace_floats(B, nq, nkv, Lpre, Ltail))
    if floats <= 0:
        raise ValueError(f"attn_decode_prefix workspace: sizes not built (B={B}, nq={nq}, nkv={nkv}, Lpre={Lpre}, Ltail={Ltail})")
    return torch.empty((floats,), dtype=F32, device=device)


@_on_tensor_device
def rope_kv_append_tail(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, tail_k: torch.Tensor, tail_v: torch.Tensor, lens: torch.Tensor,
                        plen: torch.Tensor, n: int, nq: int, nkv: int, d: int, q16: torch.Tensor | None = None):
    """Launch 1: q and k of every row's new token rotated at position lens[r] (q in place; fp16 form: ``q16`` [B, >= nq d] receives
    its fp16 rounding), k / v appended at tail slot lens[r] - plen[r // n]."""
    dt, qdt, f16 = _formats(tail_k, "tail_k")
    B, Ltail = _geometry(tail_k, "tail_k", d, nkv)
    _rows_of(B, n, plen)
    if qkv.shape[0] != B or lens.numel() != B or tail_v.shape != tail_k.shape or cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != d // 2:
        raise ValueError(f"rope_kv_append_tail: {B} rows of q|k|v and lens, v like k, [positions, {d // 2}] tables expected")
    if f16 and (q16 is None or q16.shape[0] != B):
        raise ValueError("rope_kv_append_tail: the fp16 form needs q16 [B, nq d]")
    p16, ld16 = (_ptr(q16, F16, "q16", True), q16.stride(0)) if f16 else (0, 0)
    _call("grit_rope_kv_append_tail", (qkv, cos, sin, tail_k, tail_v, lens, plen, q16), _ptr(qkv, qdt, "qkv", True), _ptr(cos, F32, "cos"),
          _ptr(sin, F32, "sin"), _ptr(tail_k, dt, "tail_k"),
          _ptr(tail_v, dt, "tail_v"), _ptr(lens, I32, "lens"), _ptr(plen, I32, "plen"), p16, B, n, nq, nkv, d, Ltail, cos.shape[0],
          qkv.stride(0), ld16, f16)


@_on_tensor_device
def attn_decode_prefix(q: torch.Tensor, prefix_k: torch.Tensor, prefix_v: torch.Tensor, plen: torch.Tensor, ws: torch.Tensor, n: int, nq: int,
                       nkv: int, d: int, Ltail: int, scale: float | None = None):
    """Launch 2: the prefix records of every (row, head).  ``q`` [B0 n, >= nq d] in the caches' 16-bit format: the rotated q|k|v rows
    (bf16) or ``q16`` (fp16)."""
    dt, _, f16 = _formats(prefix_k, "prefix_k")
    B0, Lpre = _geometry(prefix_k, "prefix_k", d, nkv)
    _rows_of(q.shape[0], n, plen)
    if plen.numel() != B0 or prefix_v.shape != prefix_k.shape:
        raise ValueError(f"attn_decode_prefix: {B0} prefixes, {plen.numel()} lengths; v like k expected")
    _ws_fits(ws, q.shape[0], nq, nkv, Lpre, Ltail, "attn_decode_prefix")
    _call("grit_attn_decode_prefix", (q, prefix_k, prefix_v, plen, ws), _ptr(q, dt, "q", True), _ptr(prefix_k, dt, "prefix_k"),
          _ptr(prefix_v, dt, "prefix_v"), _ptr(plen, I32, "plen"),
          _ptr(ws, F32, "workspace"), B0, n, nq, nkv, d, Lpre, Ltail, q.stride(0), float(d ** -0.5 if scale is None else scale), f16)


@_on_tensor_device
def attn_decode_tail(q: torch.Tensor, tail_k: torch.Tensor, tail_v: torch.Tensor, lens: torch.Tensor, plen: torch.Tensor, ws: torch.Tensor, n: int,
                     nq: int, nkv: int, d: int, Lpre: int, scale: float | None = None):
    """Launch 3: the tail records of every (row, head).  ``q``: the rotated q|k|v rows (bf16; fp32 beside fp16 tails)."""
    dt, qdt, f16 = _formats(tail_k, "tail_k")
    B, Ltail = _geometry(tail_k, "tail_k", d, nkv)
    _rows_of(B, n, plen)
    if q.shape[0] != B or lens.numel() != B or tail_v.shape != tail_k.shape:
        raise ValueError(f"attn_decode_tail: {B} rows of q and lens, v like k expected")
    _ws_fits(ws, B, nq, nkv, Lpre, Ltail, "attn_decode_tail")
    _call("grit_attn_decode_tail", (q, tail_k, tail_v, lens, plen, ws), _ptr(q, qdt, "q", True), _ptr(tail_k, dt, "tail_k"),
          _ptr(tail_v, dt, "tail_v"), _ptr(lens, I32, "lens"),
          _ptr(plen, I32, "plen"), _ptr(ws, F32, "workspace"), B, n, nq, nkv, d, Lpre, Ltail, q.stride(0),
          float(d ** -0.5 if scale is None else scale), f16)


@_on_tensor_device
def attn_decode_prefix_combine(ws: torch.Tensor, out: torch.Tensor, nq: int, nkv: int, d: int, Lpre: int, Ltail: int) -> torch.Tensor:
    """Launch 4: the records of every (row, head) merged into ``out`` [B, >= nq d] (bf16 or fp16: the caches' format)."""
    _, _, f16 = _formats(out, "out")
    if out.dim() == 2:
        _ws_fits(ws, out.shape[0], nq, nkv, Lpre, Ltail, "attn_decode_prefix_combine")
    _call("grit_attn_decode_prefix_combine", (ws, out), _ptr(ws, F32, "workspace"), _ptr(out, out.dtype, "out", True), out.shape[0], nq, nkv, d,
          Lpre, Ltail, out.stride(0), f16)
    return out
