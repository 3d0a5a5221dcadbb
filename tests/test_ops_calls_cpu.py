"""CPU: what gritlm_amd/ops.py hands to the library is pinned, call by call.
tests/golden/ops_abi_calls.json holds, for a deterministic table of calls that drives every public launcher of ``ops`` through every
branch its wrapper has (each dtype form, each optional argument absent and present, ``out`` given or not, each epilogue the wrapper
treats differently, padded and packed layouts, causal and window, ``deferred`` and ``transposed`` on and off), what the revision the
table was recorded from did: every C call (entry point and arguments in order), the scratch it allocated, what it returned and, with
a timer set, every span.  A second table of bad calls holds the exception type and message of every Python-side refusal.  The
revision under test must reproduce both, byte for byte.

Nothing is launched and no device is needed (a device that is present is not touched): for the duration of a call, through pytest's
MonkeyPatch, ``torch.Tensor.is_cuda`` answers True, ``torch.cuda.current_device`` answers None, ``ops._stream`` answers a constant and
``ops._lib.load`` answers a stand-in that serves every name of ``_lib._SIGNATURES``, records the call and returns 0 (the host-only
``*_workspace_*`` size functions are forwarded to the real library, so the built library must be there).

How a C call is recorded: integers as they are, floats by repr, a pointer as the tensor it points into (an argument of the op by
name, ``r<i>`` the i-th returned tensor, ``s<i>`` the i-th scratch allocation) plus ``+<byte offset>``, 0 for null, ``S`` for the
stream.  Scratch is what the op allocates while it runs (torch.empty / zeros / empty_like / full / ones, and the results of
torch.sort) and does not return; its dtype and shape are recorded, so an undersized workspace shows.  A returned tensor is recorded
as ``dtype[shape;strides]``, or ``=<argument>`` when it is that argument itself.  A span is (name, repr(work), tag); work that is a
device tensor is recorded by value.  Every case runs with no timer and with one: the C calls must not depend on it.

A third pass makes the stand-in answer GRIT_E_BADARG once for each entry point: the GritHipError must name the entry that was
called.  ``reported`` in the fixture holds what the recorded revision named instead, where it named another; MISNAMED_BEFORE lists
the entries for which that is allowed.

Recording (from the revision whose behaviour is to be pinned, e.g. a ``git worktree`` of it with its library built; this file uses
only public signatures and the hooks above, so the same file runs against both revisions):
    PYTHONPATH=<that revision's root> python tests/test_ops_calls_cpu.py --record"""
import contextlib
import ctypes
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)            # (appended: a recording puts the recorded revision in front)
from gritlm_amd import _lib, ops  # noqa: E402
from gritlm_amd._lib import (EPI_RESIDUAL, EPI_RESIDUAL_F32, EPI_STORE, EPI_SWIGLU, EPI_SWIGLU_BWD, EPI_SWIGLU_STACKED,  # noqa: E402
                             EPI_SWIGLU_STACKED_SAVE)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ops_abi_calls.json")
STREAM = 0x57AE40
LAST_ERROR = b"stand-in"
BF16, F16, F32, I64, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int64, torch.int32

# entry points of the binding that ops.py never calls (comm.py, distributed.py and the engines do); nothing else may be missing from the trace
NEVER_CALLED = ("grit_version", "grit_last_error_string", "grit_swiglu_block", "grit_comm_unique_id", "grit_comm_init",
                "grit_comm_allgather_packed", "grit_comm_destroy", "grit_stream_create_cu_mask", "grit_stream_destroy")
# the four refusals that named an entry which was not called (op: the entries it concerns) at the recorded revision
MISNAMED_BEFORE = {"gemv_expert": ("grit_gemv_bf16_expert", "grit_gemv_f16_expert"),
                   "rmsnorm_decode_gemm": ("grit_rmsnorm_decode_gemm_bf16_deferred", "grit_rmsnorm_decode_gemm_f16_deferred"),
                   "rmsnorm_gemv, deferred bf16": ("grit_rmsnorm_gemv_bf16_deferred",),
                   "attn_prefill_cached, fp16": ("grit_attn_prefill_cached_f16_fwd",)}

T, H, N, K, E = 4, 64, 32, 64, 4
B, NQ, NKV, D, S = 2, 4, 2, 128, 8
V, TOPK = 1001, 2
QS, TS, L = (NQ + 2 * NKV) * D, B * S, 8          # fused q|k|v row, padded rows, cache length


class _StandInLib:
    """serves every name of the signature table: records (name, arguments), returns 0 -- or GRIT_E_BADARG, once, for ``fail``"""

    def __init__(self, real, fail=None):
        self.real, self.fail, self.calls = real, fail, []

    def __getattr__(self, name):
        if name not in _lib._SIGNATURES:
            raise AttributeError(name)

        def entry(*args):
            assert len(args) == len(_lib._SIGNATURES[name][1]), (name, len(args))
            self.calls.append((name, args))
            if name == "grit_last_error_string":
                return LAST_ERROR
            if "_workspace_" in name:
                return getattr(self.real, name)(*args)
            if name == self.fail:
                self.fail = None
                return _lib.GRIT_E_BADARG
            return 0
        return entry


class _Event:
    def record(self):
        pass


class _StandInTimer:
    """ops' side of KernelTimer (which creates device events): span() hands back two things with a no-op record()"""

    def __init__(self):
        self.spans = []

    def span(self, name, work=0.0, tag=None):
        self.spans.append([name, repr(float(work)), tag])
        return _Event(), _Event()


@contextlib.contextmanager
def patched(real, cpu=False, timer=None, fail=None, tag_m=False):
    """the hooks of the module docstring; ``cpu``: tensors stay what they are (the refusal of a CPU tensor).  Yields (stand-in, allocations)."""
    lib, allocs = _StandInLib(real, fail), []
    with pytest.MonkeyPatch.context() as mp:
        if not cpu:
            mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        mp.setattr(torch.cuda, "current_device", lambda: None)
        mp.setattr(ops, "_stream", lambda: STREAM)
        mp.setattr(ops._lib, "load", lambda: lib)
        mp.setattr(ops, "_timer", timer)
        if tag_m:
            mp.setattr(ops, "_TAG_M", True)

        def watch(fn):
            def watched(*a, **k):
                r = fn(*a, **k)
                allocs.extend(r if isinstance(r, tuple) else [r])
                return r
            return watched
        for name in ("empty", "zeros", "empty_like", "full", "ones", "sort"):
            mp.setattr(torch, name, watch(getattr(torch, name)))
        yield lib, allocs


def Z(*shape, dt=BF16):
    return torch.zeros(shape, dtype=dt)


def ints(*v, dt=I32):
    return torch.tensor(v, dtype=dt)


def wide(rows, cols, dt=BF16, pad=8):
    """row-strided view: leading dimension cols + pad"""
    return Z(rows, cols + pad, dt=dt)[:, :cols]


def _attn(dt=BF16, **kw):
    return dict(dict(qkv=Z(TS, QS, dt=dt), key_bits=Z(B, 1, dt=I64), B=B, S=S, nq=NQ, nkv=NKV, d=D), **kw)


def _attn_varlen(dt=BF16, **kw):
    return dict(dict(qkv=Z(TS, QS, dt=dt), cu_seqlens=ints(0, 7, TS), max_len=9, nq=NQ, nkv=NKV, d=D), **kw)


def _attn_bwd(**kw):
    return dict(dict(qkv=Z(TS, QS), key_bits=Z(B, 1, dt=I64), out=Z(TS, NQ * D), dout=Z(TS, NQ * D), lse=Z(TS, NQ, dt=F32), B=B, S=S, nq=NQ, nkv=NKV,
                     d=D), **kw)


def _attn_varlen_bwd(**kw):
    return dict(dict(qkv=Z(TS, QS), cu_seqlens=ints(0, 7, TS), max_len=9, out=Z(TS, NQ * D), dout=Z(TS, NQ * D), lse=Z(TS, NQ, dt=F32), nq=NQ,
                     nkv=NKV, d=D), **kw)


def _gemm(epilogue=EPI_STORE, dt=BF16, **kw):
    return dict(dict(a=Z(T, K, dt=dt), w=Z(N, K, dt=dt), epilogue=epilogue), **kw)


def _grouped(dt=BF16, **kw):
    return dict(dict(a=Z(T, K, dt=dt), w=Z(E, N, K, dt=dt), counts=Z(E, dt=I32), m_total=2 * T), **kw)


def _proj(dt=BF16, **kw):
    return dict(dict(x=Z(B, K, dt=dt), w=Z(N, K, dt=dt)), **kw)


def _norm_proj(dt=BF16, **kw):
    return dict(dict(x=Z(B, K, dt=dt), ln_w=Z(K), eps=1e-5, w=Z(N, K, dt=dt)), **kw)


def _cache(dt=BF16, rows=B, row_dt=None, **kw):
    """the decode ops' common operands; ``rows``: rows of the fused projection"""
    return dict(dict(qkv=Z(rows, QS, dt=row_dt or dt), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), cache_k=Z(B, NKV, L, D, dt=dt),
                     cache_v=Z(B, NKV, L, D, dt=dt), lens=Z(rows, dt=I32), nq=NQ, nkv=NKV, d=D), **kw)


def _without(d, *names):
    return {k: v for k, v in d.items() if k not in names}


def _q(d):
    """the same operands for an op that calls the rows ``q``"""
    return {("q" if k == "qkv" else k): v for k, v in _without(d, "cos", "sin").items()}


def _token(dt=BF16, full=False, **kw):
    opt = dict(lens=Z(B, dt=I32), history=Z(B, 16, dt=I64), step=Z(1, dt=I32)) if full else {}
    return dict(dict(logits=wide(B, V, dt, pad=7), next_ids=Z(B, dt=I64)), **opt, **kw)


_SAMPLE = dict(temperature=0.7, top_k=40, top_p=0.9)

# (case, op, its arguments by name, flags of patched()) -- the arguments are built anew for every run
CASES = [
    ("embed_gather bf16", "embed_gather", lambda: dict(table=Z(V, H), ids=Z(T, dt=I64)), {}),
    ("embed_gather bf16 out", "embed_gather", lambda: dict(table=Z(V, H), ids=Z(T, dt=I64), out=Z(T, H)), {}),
    ("embed_gather f32 out", "embed_gather", lambda: dict(table=Z(V, H), ids=Z(T, dt=I64), out=Z(T, H, dt=F32)), {}),
    ("embed_gather f16", "embed_gather", lambda: dict(table=Z(V, H, dt=F16), ids=Z(T, dt=I64), out=Z(T, H, dt=F16)), {}),
    ("rmsnorm bf16", "rmsnorm", lambda: dict(x=Z(T, H), w=Z(H), eps=1e-5), {}),
    ("rmsnorm bf16 3-d out", "rmsnorm", lambda: dict(x=Z(2, 2, H), w=Z(H), eps=1e-6, out=Z(2, 2, H)), {}),
    ("rmsnorm f32", "rmsnorm", lambda: dict(x=Z(T, H, dt=F32), w=Z(H), eps=1e-5), {}),
    ("rmsnorm f32 out bf16", "rmsnorm", lambda: dict(x=Z(T, H, dt=F32), w=Z(H), eps=1e-5, out=Z(T, H)), {}),
    ("rmsnorm f32 out f16", "rmsnorm", lambda: dict(x=Z(T, H, dt=F32), w=Z(H), eps=1e-5, out=Z(T, H, dt=F16)), {}),
    ("rmsnorm f16", "rmsnorm", lambda: dict(x=Z(T, H, dt=F16), w=Z(H), eps=1e-5), {}),
    ("rmsnorm f16 out f16", "rmsnorm", lambda: dict(x=Z(T, H, dt=F16), w=Z(H), eps=1e-5, out=Z(T, H, dt=F16)), {}),
    ("rmsnorm f16 out bf16", "rmsnorm", lambda: dict(x=Z(T, H, dt=F16), w=Z(H), eps=1e-5, out=Z(T, H)), {}),
    ("rope_qk_", "rope_qk_", lambda: dict(qkv=Z(TS, QS), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), S=S, nq=NQ, nkv=NKV, d=D), {}),
    ("rope_qk_ inverse", "rope_qk_", lambda: dict(qkv=Z(TS, QS), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), S=S, nq=NQ, nkv=NKV, d=D, inverse=True), {}),
    ("rope_qk_pos_", "rope_qk_pos_",
     lambda: dict(qkv=Z(TS, QS), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), positions=Z(TS, dt=I32), nq=NQ, nkv=NKV, d=D), {}),
    ("rope_qk_pos_ inverse", "rope_qk_pos_",
     lambda: dict(qkv=Z(TS, QS), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), positions=Z(TS, dt=I32), nq=NQ, nkv=NKV, d=D, inverse=True), {}),
    ("attn_bidir", "attn_bidir", lambda: _attn(), {}),
    ("attn_bidir out lse scale", "attn_bidir", lambda: _attn(out=Z(TS, NQ * D), lse=Z(TS, NQ, dt=F32), scale=0.125), {}),
    ("attn_bidir causal", "attn_bidir", lambda: _attn(causal=True), {}),
    ("attn_bidir causal window lse", "attn_bidir", lambda: _attn(causal=True, window=3, lse=Z(TS, NQ, dt=F32)), {}),
    ("attn_bidir f16", "attn_bidir", lambda: _attn(F16), {}),
    ("attn_bidir f16 out lse", "attn_bidir", lambda: _attn(F16, out=Z(TS, NQ * D, dt=F16), lse=Z(TS, NQ, dt=F32)), {}),
    ("attn_bidir f16 causal", "attn_bidir", lambda: _attn(F16, causal=True), {}),
    ("attn_bidir f16 causal window", "attn_bidir", lambda: _attn(F16, causal=True, window=3, scale=0.125), {}),
    ("attn_bidir_varlen", "attn_bidir_varlen", lambda: _attn_varlen(), {}),
    ("attn_bidir_varlen out lse scale", "attn_bidir_varlen", lambda: _attn_varlen(out=Z(TS, NQ * D), lse=Z(TS, NQ, dt=F32), scale=0.125), {}),
    ("attn_bidir_varlen causal", "attn_bidir_varlen", lambda: _attn_varlen(causal=True), {}),
    ("attn_bidir_varlen causal window lse", "attn_bidir_varlen", lambda: _attn_varlen(causal=True, window=3, lse=Z(TS, NQ, dt=F32)), {}),
    ("attn_bidir_varlen f16", "attn_bidir_varlen", lambda: _attn_varlen(F16), {}),
    ("attn_bidir_varlen f16 out lse", "attn_bidir_varlen", lambda: _attn_varlen(F16, out=Z(TS, NQ * D, dt=F16), lse=Z(TS, NQ, dt=F32)), {}),
    ("attn_bidir_varlen f16 causal", "attn_bidir_varlen", lambda: _attn_varlen(F16, causal=True), {}),
    ("attn_bidir_varlen f16 causal window", "attn_bidir_varlen", lambda: _attn_varlen(F16, causal=True, window=3, scale=0.125), {}),
    ("attn_bidir_bwd", "attn_bidir_bwd", lambda: _attn_bwd(), {}),
    ("attn_bidir_bwd dqkv scale", "attn_bidir_bwd", lambda: _attn_bwd(dqkv=Z(TS, QS), scale=0.125), {}),
    ("attn_bidir_bwd causal", "attn_bidir_bwd", lambda: _attn_bwd(causal=True), {}),
    ("attn_bidir_bwd causal window", "attn_bidir_bwd", lambda: _attn_bwd(causal=True, window=3), {}),
    ("attn_bidir_varlen_bwd", "attn_bidir_varlen_bwd", lambda: _attn_varlen_bwd(), {}),
    ("attn_bidir_varlen_bwd dqkv scale", "attn_bidir_varlen_bwd", lambda: _attn_varlen_bwd(dqkv=Z(TS, QS), scale=0.125), {}),
    ("attn_bidir_varlen_bwd causal", "attn_bidir_varlen_bwd", lambda: _attn_varlen_bwd(causal=True), {}),
    ("attn_bidir_varlen_bwd causal window", "attn_bidir_varlen_bwd", lambda: _attn_varlen_bwd(causal=True, window=3), {}),
    ("pool_norm mean", "pool_norm", lambda: dict(hidden=Z(B, S, H), mask=Z(B, S, dt=I64), method="mean", normalize=True), {}),
    ("pool_norm weightedmean", "pool_norm", lambda: dict(hidden=Z(B, S, H), mask=Z(B, S, dt=I64), method="weightedmean", normalize=False), {}),
    ("pool_norm cls", "pool_norm", lambda: dict(hidden=Z(B, S, H), mask=Z(B, S, dt=I64), method="cls", normalize=True), {}),
    ("pool_norm lasttoken instr inv_norm", "pool_norm",
     lambda: dict(hidden=Z(B, S, H), mask=Z(B, S, dt=I64), method="lasttoken", normalize=True, instr_len=Z(B, dt=I32), inv_norm=Z(B, dt=F32)), {}),
    ("pool_norm_bwd", "pool_norm_bwd",
     lambda: dict(y=Z(B, H, dt=F32), dy=Z(B, H, dt=F32), inv_norm=None, mask=Z(B, S, dt=I64), method="mean", normalize=False, S=S), {}),
    ("pool_norm_bwd inv_norm instr", "pool_norm_bwd",
     lambda: dict(y=Z(B, H, dt=F32), dy=Z(B, H, dt=F32), inv_norm=Z(B, dt=F32), mask=Z(B, S, dt=I64), method="lasttoken", normalize=True, S=S,
                  instr_len=Z(B, dt=I32)), {}),
    ("pool_norm_varlen mean", "pool_norm_varlen", lambda: dict(hidden=Z(TS, H), cu_seqlens=ints(0, 7, TS), method="mean", normalize=True), {}),
    ("pool_norm_varlen cls", "pool_norm_varlen", lambda: dict(hidden=Z(TS, H), cu_seqlens=ints(0, 7, TS), method="cls", normalize=False), {}),
    ("pool_norm_varlen weightedmean instr inv_norm", "pool_norm_varlen",
     lambda: dict(hidden=Z(TS, H), cu_seqlens=ints(0, 7, TS), method="weightedmean", normalize=True, instr_len=Z(B, dt=I32), inv_norm=Z(B, dt=F32)), {}),
    ("pool_norm_varlen_bwd", "pool_norm_varlen_bwd",
     lambda: dict(y=Z(B, H, dt=F32), dy=Z(B, H, dt=F32), inv_norm=None, cu_seqlens=ints(0, 7, TS), T=TS, method="mean", normalize=False), {}),
    ("pool_norm_varlen_bwd inv_norm instr", "pool_norm_varlen_bwd",
     lambda: dict(y=Z(B, H, dt=F32), dy=Z(B, H, dt=F32), inv_norm=Z(B, dt=F32), cu_seqlens=ints(0, 7, TS), T=TS, method="lasttoken", normalize=True,
                  instr_len=Z(B, dt=I32)), {}),
    ("gemm_nt store", "gemm_nt", lambda: dict(a=Z(T, K), w=Z(N, K)), {}),
    ("gemm_nt store strided out tag_m", "gemm_nt", lambda: dict(a=wide(T, K), w=wide(N, K, pad=16), out=wide(T, N)), dict(tag_m=True)),
    ("gemm_nt residual", "gemm_nt", lambda: _gemm(EPI_RESIDUAL, residual=wide(T, N)), {}),
    ("gemm_nt swiglu", "gemm_nt", lambda: _gemm(EPI_SWIGLU), {}),
    ("gemm_nt swiglu_stacked", "gemm_nt", lambda: _gemm(EPI_SWIGLU_STACKED), {}),
    ("gemm_nt swiglu_stacked_save", "gemm_nt", lambda: _gemm(EPI_SWIGLU_STACKED_SAVE, residual=Z(T, N)), {}),
    ("gemm_nt swiglu_bwd", "gemm_nt", lambda: _gemm(EPI_SWIGLU_BWD, residual=Z(T, 2 * N)), {}),
    ("gemm_nt residual_f32", "gemm_nt", lambda: _gemm(EPI_RESIDUAL_F32, residual=Z(T, N, dt=F32)), {}),
    ("gemm_nt f16 store", "gemm_nt", lambda: _gemm(EPI_STORE, F16), {}),
    ("gemm_nt f16 swiglu out", "gemm_nt", lambda: _gemm(EPI_SWIGLU, F16, out=Z(T, N // 2, dt=F16)), {}),
    ("gemm_nt f16 swiglu_stacked", "gemm_nt", lambda: _gemm(EPI_SWIGLU_STACKED, F16), {}),
    ("gemm_nt f16 residual", "gemm_nt", lambda: _gemm(EPI_RESIDUAL, F16, residual=Z(T, N, dt=F16)), {}),
    ("gemm_nt f16 residual_f32", "gemm_nt", lambda: _gemm(EPI_RESIDUAL_F32, F16, residual=Z(T, N, dt=F32)), {}),
    ("gemm_nt_pair", "gemm_nt_pair",
     lambda: dict(a1=Z(T, K), w1=Z(N, K), out1=Z(T, N), a2=wide(6, K), w2=Z(16, K), out2=wide(6, 16)), {}),
    ("gemm_nt_pair store tag_m", "gemm_nt_pair",
     lambda: dict(a1=Z(T, K), w1=Z(N, K), out1=Z(T, N), a2=wide(6, K), w2=Z(16, K), out2=wide(6, 16), accumulate=False), dict(tag_m=True)),
    ("gemm_nt_rope", "gemm_nt_rope", lambda: dict(a=Z(TS, K), w=Z(3 * D, K), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), rope_cols=2 * D, S=S), {}),
    ("gemm_nt_rope positions out tag_m", "gemm_nt_rope",
     lambda: dict(a=Z(TS, K), w=Z(3 * D, K), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), rope_cols=2 * D, positions=Z(TS, dt=I32), out=wide(TS, 3 * D)),
     dict(tag_m=True)),
    ("gemm_nt_rope f16", "gemm_nt_rope",
     lambda: dict(a=Z(TS, K, dt=F16), w=Z(3 * D, K, dt=F16), cos=Z(16, D, dt=F32), sin=Z(16, D, dt=F32), rope_cols=2 * D, S=S), {}),
    ("gemm_nt_grouped store", "gemm_nt_grouped", lambda: _grouped(), {}),
    ("gemm_nt_grouped swiglu a_rows", "gemm_nt_grouped", lambda: _grouped(epilogue=EPI_SWIGLU, a_rows=Z(2 * T, dt=I32)), {}),
    ("gemm_nt_grouped swiglu_stacked out", "gemm_nt_grouped", lambda: _grouped(epilogue=EPI_SWIGLU_STACKED, out=wide(2 * T, N // 2)), {}),
    ("gemm_nt_grouped f16 store", "gemm_nt_grouped", lambda: _grouped(F16), {}),
    ("gemm_nt_grouped f16 swiglu a_rows", "gemm_nt_grouped", lambda: _grouped(F16, epilogue=EPI_SWIGLU, a_rows=Z(2 * T, dt=I32)), {}),
    ("gemm_nt_grouped_epi store", "gemm_nt_grouped_epi", lambda: _grouped(epilogue=EPI_STORE), {}),
    ("gemm_nt_grouped_epi swiglu a_rows", "gemm_nt_grouped_epi", lambda: _grouped(epilogue=EPI_SWIGLU, a_rows=Z(2 * T, dt=I32)), {}),
    ("gemm_nt_grouped_epi swiglu_stacked out", "gemm_nt_grouped_epi", lambda: _grouped(epilogue=EPI_SWIGLU_STACKED, out=wide(2 * T, N // 2)), {}),
    ("gemm_nt_grouped_epi swiglu_stacked_save", "gemm_nt_grouped_epi",
     lambda: _grouped(epilogue=EPI_SWIGLU_STACKED_SAVE, residual=wide(2 * T, N)), {}),
    ("gemm_nt_grouped_epi swiglu_bwd", "gemm_nt_grouped_epi", lambda: _grouped(epilogue=EPI_SWIGLU_BWD, residual=Z(2 * T, 2 * N)), {}),
    ("moe_combine_bwd", "moe_combine_bwd",
     lambda: dict(dout=Z(T, H), y=Z(2 * T, H), row_token=Z(2 * T, dt=I32), rows=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32)), {}),
    ("moe_router_bwd", "moe_router_bwd",
     lambda: dict(x=Z(T, H), gate_w=Z(E, H), experts=Z(T, 2, dt=I32), dw=Z(T, 2, dt=F32), dx_in=None, gate_grad=Z(E, H)), {}),
    ("moe_router_bwd dx_in aux dlogits", "moe_router_bwd",
     lambda: dict(x=Z(T, H), gate_w=Z(E, H), experts=Z(T, 2, dt=I32), dw=Z(T, 2, dt=F32), dx_in=Z(T, H), gate_grad=Z(E, H),
                  aux_dlogits=Z(T, E, dt=F32), return_dlogits=True), {}),
    ("moe_route", "moe_route", lambda: dict(x=Z(T, H), gate_w=Z(E, H)), {}),
    ("moe_route_f32", "moe_route_f32", lambda: dict(h=Z(T, H, dt=F32), ln_w=Z(H), eps=1e-5, gate_w=Z(E, H)), {}),
    ("moe_combine", "moe_combine", lambda: dict(y=Z(2 * T, H), rows=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32), residual=None), {}),
    ("moe_combine residual out", "moe_combine",
     lambda: dict(y=Z(2 * T, H), rows=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32), residual=Z(T, H), out=Z(T, H)), {}),
    ("moe_combine f16", "moe_combine", lambda: dict(y=Z(2 * T, H, dt=F16), rows=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32), residual=None), {}),
    ("moe_combine f16 residual out", "moe_combine",
     lambda: dict(y=Z(2 * T, H, dt=F16), rows=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32), residual=Z(T, H, dt=F32), out=Z(T, H, dt=F32)), {}),
    ("f16_overflow_flag", "f16_overflow_flag", lambda: dict(device=-1), {}),
    ("f16_overflow_flag keep", "f16_overflow_flag", lambda: dict(device=-1, clear=False), {}),
    ("mask_pack", "mask_pack", lambda: dict(mask=Z(B, 70, dt=I64)), {}),
    ("infonce", "infonce", lambda: dict(q=Z(3, H, dt=F32), p=Z(5, H, dt=F32), temperature=0.02), {}),
    ("infonce local rows", "infonce", lambda: dict(q=Z(3, H, dt=F32), p=Z(5, H, dt=F32), temperature=0.05, q_off=1, nq_loc=2, p_off=2, np_loc=3), {}),
    ("infonce no grad", "infonce", lambda: dict(q=Z(3, H, dt=F32), p=Z(5, H, dt=F32), temperature=0.02, want_grad=False), {}),
    ("transpose", "transpose", lambda: dict(x=Z(8, 6)), {}),
    ("transpose padded", "transpose", lambda: dict(x=wide(4, 6)), {}),
    ("transpose out", "transpose", lambda: dict(x=Z(4, 6), out=Z(6, 16)), {}),
    ("rmsnorm_bwd", "rmsnorm_bwd", lambda: dict(dy=Z(T, H), x=Z(T, H), w=Z(H), eps=1e-5, dw=Z(H, dt=F32)), {}),
    ("rmsnorm_bwd dres out", "rmsnorm_bwd", lambda: dict(dy=Z(2, 2, H), x=Z(2, 2, H), w=Z(H), eps=1e-5, dw=Z(H, dt=F32), dres=Z(2, 2, H), out=Z(2, 2, H)), {}),
    ("swiglu", "swiglu", lambda: dict(gu=Z(T, 2 * N)), {}),
    ("swiglu out", "swiglu", lambda: dict(gu=Z(T, 2 * N), out=Z(T, N)), {}),
    ("swiglu_bwd", "swiglu_bwd", lambda: dict(gu=Z(T, 2 * N), dact=Z(T, N)), {}),
    ("swiglu_bwd out", "swiglu_bwd", lambda: dict(gu=Z(T, 2 * N), dact=Z(T, N), out=Z(T, 2 * N)), {}),
    ("gemv", "gemv", lambda: _proj(), {}),
    ("gemv residual out", "gemv", lambda: _proj(x=wide(B, K), out=wide(B, N), epilogue=EPI_RESIDUAL, residual=wide(B, N, pad=16)), {}),
    ("gemv swiglu", "gemv", lambda: _proj(epilogue=EPI_SWIGLU), {}),
    ("gemv f16", "gemv", lambda: _proj(F16), {}),
    ("gemv f16 residual out16", "gemv", lambda: _proj(F16, epilogue=EPI_RESIDUAL, residual=Z(B, N, dt=F32), out16=wide(B, N, F16)), {}),
    ("gemv f16 swiglu", "gemv", lambda: _proj(F16, epilogue=EPI_SWIGLU), {}),
    ("gemv_expert", "gemv_expert", lambda: dict(x=Z(B, K), w_stack=Z(E, N, K), expert=Z(1, dt=I32)), {}),
    ("gemv_expert swiglu expert view", "gemv_expert", lambda: dict(x=Z(B, K), w_stack=Z(E, N, K), expert=Z(T, 2, dt=I32)[1], epilogue=EPI_SWIGLU), {}),
    ("gemv_expert f16 out", "gemv_expert",
     lambda: dict(x=Z(B, K, dt=F16), w_stack=Z(E, N, K, dt=F16), expert=Z(1, dt=I32), out=Z(B, N, dt=F32)), {}),
    ("gemv_expert f16 swiglu", "gemv_expert", lambda: dict(x=Z(B, K, dt=F16), w_stack=Z(E, N, K, dt=F16), expert=Z(1, dt=I32), epilogue=EPI_SWIGLU), {}),
    ("moe_decode_combine_f32", "moe_decode_combine_f32",
     lambda: dict(h=Z(B, H, dt=F32), h16=Z(B, H, dt=F16), y=Z(2 * B, H, dt=F32), weights=Z(B, 2, dt=F32)), {}),
    ("moe_router_top2", "moe_router_top2", lambda: dict(x=Z(T, H), gate_w=Z(E, H), experts=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32)), {}),
    ("moe_router_top2 f32", "moe_router_top2",
     lambda: dict(x=Z(T, H, dt=F32), gate_w=Z(E, H), experts=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32), ln_w=Z(H), eps=1e-5), {}),
    ("rmsnorm_gemv", "rmsnorm_gemv", lambda: _norm_proj(), {}),
    ("rmsnorm_gemv deferred swiglu", "rmsnorm_gemv", lambda: _norm_proj(epilogue=EPI_SWIGLU, deferred=True), {}),
    ("rmsnorm_gemv f16 deferred out", "rmsnorm_gemv", lambda: _norm_proj(F16, deferred=True, out=wide(B, N, F32)), {}),
    ("rmsnorm_gemv f16 deferred swiglu", "rmsnorm_gemv", lambda: _norm_proj(F16, deferred=True, epilogue=EPI_SWIGLU), {}),
    ("decode_gemm", "decode_gemm", lambda: _proj(), {}),
    ("decode_gemm residual out", "decode_gemm", lambda: _proj(x=wide(B, K), out=wide(B, N), epilogue=EPI_RESIDUAL, residual=wide(B, N, pad=16)), {}),
    ("decode_gemm swiglu", "decode_gemm", lambda: _proj(epilogue=EPI_SWIGLU), {}),
    ("decode_gemm f16", "decode_gemm", lambda: _proj(F16), {}),
    ("decode_gemm f16 residual out16", "decode_gemm", lambda: _proj(F16, epilogue=EPI_RESIDUAL, residual=Z(B, N, dt=F32), out16=wide(B, N, F16)), {}),
    ("decode_gemm f16 swiglu", "decode_gemm", lambda: _proj(F16, epilogue=EPI_SWIGLU), {}),
    ("rmsnorm_decode_gemm", "rmsnorm_decode_gemm", lambda: _norm_proj(), {}),
    ("rmsnorm_decode_gemm swiglu out", "rmsnorm_decode_gemm", lambda: _norm_proj(epilogue=EPI_SWIGLU, out=wide(B, N // 2)), {}),
    ("rmsnorm_decode_gemm f16", "rmsnorm_decode_gemm", lambda: _norm_proj(F16), {}),
    ("rmsnorm_decode_gemm f16 swiglu", "rmsnorm_decode_gemm", lambda: _norm_proj(F16, epilogue=EPI_SWIGLU), {}),
    ("rope_kv_append", "rope_kv_append", lambda: _cache(), {}),
    ("kv_append", "kv_append", lambda: _without(_cache(), "cos", "sin"), {}),
    ("attn_decode_workspace", "attn_decode_workspace", lambda: dict(B=B, nq=NQ, nkv=NKV, Lmax=L, device="cpu"), {}),
    ("attn_decode", "attn_decode", lambda: _q(_cache(out=Z(B, NQ * D), workspace=Z(4096, dt=F32))), {}),
    ("attn_decode scale", "attn_decode", lambda: _q(_cache(out=wide(B, NQ * D), workspace=Z(4096, dt=F32), scale=0.125)), {}),
    ("attn_decode_rope", "attn_decode_rope", lambda: _cache(out=Z(B, NQ * D), workspace=Z(4096, dt=F32)), {}),
    ("attn_decode_rope f16 scale", "attn_decode_rope", lambda: _cache(F16, row_dt=F32, out=Z(B, NQ * D, dt=F16), workspace=Z(4096, dt=F32), scale=0.125), {}),
    ("rope_kv_append_rows", "rope_kv_append_rows", lambda: _cache(rows=3, cache_row=Z(3, dt=I32)), {}),
    ("rope_kv_append_rows f16", "rope_kv_append_rows", lambda: _cache(F16, rows=3, row_dt=F32, cache_row=Z(3, dt=I32)), {}),
    ("attn_decode_rows", "attn_decode_rows", lambda: _q(_cache(rows=3, cache_row=Z(3, dt=I32), out=Z(3, NQ * D), workspace=Z(4096, dt=F32))), {}),
    ("attn_decode_rows f16 scale", "attn_decode_rows",
     lambda: _q(_cache(F16, rows=3, row_dt=F32, cache_row=Z(3, dt=I32), out=Z(3, NQ * D, dt=F16), workspace=Z(4096, dt=F32), scale=0.125)), {}),
    ("kv_append_chunk", "kv_append_chunk", lambda: _without(_cache(rows=B * 4, lens=ints(1, 2), plen=ints(3, 4)), "cos", "sin"), {}),
    ("kv_append_chunk f16", "kv_append_chunk", lambda: _without(_cache(F16, rows=B * 4, lens=ints(1, 2), plen=ints(3, 4)), "cos", "sin"), {}),
    ("attn_prefill_cached", "attn_prefill_cached", lambda: _q(_cache(rows=B * 4, lens=ints(1, 2), plen=ints(3, 4))), {}),
    ("attn_prefill_cached out scale", "attn_prefill_cached",
     lambda: _q(_cache(rows=B * 4, lens=ints(1, 2), plen=ints(3, 4), out=Z(B * 4, NQ * D), scale=0.125)), {}),
    ("attn_prefill_cached f16", "attn_prefill_cached", lambda: _q(_cache(F16, rows=B * 4, lens=ints(1, 2), plen=ints(3, 4))), {}),
    ("argmax_advance", "argmax_advance", lambda: _token(), {}),
    ("argmax_advance lens history step", "argmax_advance", lambda: _token(full=True), {}),
    ("argmax_advance f32", "argmax_advance", lambda: _token(F32), {}),
    ("argmax_advance f32 lens history step", "argmax_advance", lambda: _token(F32, full=True), {}),
    ("sample_advance", "sample_advance", lambda: _token(keys=Z(B, dt=I64), **_SAMPLE), {}),
    ("sample_advance lens history step", "sample_advance", lambda: _token(full=True, keys=Z(B, dt=I64), **_SAMPLE), {}),
    ("sample_advance f32 top_k beyond int32", "sample_advance", lambda: _token(F32, keys=Z(B, dt=I64), temperature=1.0, top_k=2 ** 40, top_p=1.0), {}),
    ("sample_advance f32 lens history step", "sample_advance", lambda: _token(F32, full=True, keys=Z(B, dt=I64), **_SAMPLE), {}),
    ("knn_topk", "knn_topk", lambda: dict(queries=Z(3, H, dt=F32), embeddings=wide(10, H, F32), k=TOPK), {}),
    ("knn_topk transposed", "knn_topk", lambda: dict(queries=Z(3, H, dt=F32), embeddings=wide(H, 10, F32), k=TOPK, transposed=True), {}),
    ("ce_fwd", "ce_fwd", lambda: dict(logits=wide(T, V, pad=7), labels=Z(T, dt=I64)), {}),
    ("ce_bwd_", "ce_bwd_", lambda: dict(logits=wide(T, V, pad=7), labels=Z(T, dt=I64), lse=Z(T, dt=F32), scale=0.25), {}),
    ("ce_bwd_ dev_scale", "ce_bwd_", lambda: dict(logits=wide(T, V, pad=7), labels=Z(T, dt=I64), lse=Z(T, dt=F32), scale=0.25, dev_scale=Z(1, dt=F32)), {}),
    ("embed_scatter_add", "embed_scatter_add", lambda: dict(dh=Z(T, H), ids=ints(3, 1, 3, 0, dt=I64), grad=Z(V, H)), {}),
    ("accum_bf16_from_f32", "accum_bf16_from_f32", lambda: dict(acc=Z(T, H), x=Z(T, H, dt=F32)), {}),
]

# every Python-side refusal of the file: (case, op, arguments, flags); cpu: is_cuda is left alone
REFUSALS = [
    ("contiguous operand: cpu tensor", "rmsnorm", lambda: dict(x=Z(T, H), w=Z(H), eps=1e-5), dict(cpu=True)),
    ("contiguous operand: wrong dtype", "rmsnorm", lambda: dict(x=Z(T, H), w=Z(H, dt=F32), eps=1e-5), {}),
    ("contiguous operand: not contiguous", "rmsnorm", lambda: dict(x=wide(T, H), w=Z(H), eps=1e-5), {}),
    ("2-d operand: cpu tensor", "gemm_nt", lambda: dict(a=Z(T, K), w=Z(N, K)), dict(cpu=True)),
    ("2-d operand: wrong dtype", "gemm_nt", lambda: dict(a=Z(T, K), w=Z(N, K, dt=F16)), {}),
    ("2-d operand: column stride", "gemm_nt", lambda: dict(a=Z(K, T).t(), w=Z(N, K)), {}),
    ("2-d operand: wrong rank", "attn_decode", lambda: _q(_cache(qkv=Z(B, 1, QS), out=Z(B, NQ * D), workspace=Z(4096, dt=F32))), {}),
    ("2-d optional operand: wrong dtype", "gemv", lambda: _proj(epilogue=EPI_RESIDUAL, residual=Z(B, N, dt=F32)), {}),
    ("3-d operand: wrong dtype", "gemm_nt_grouped", lambda: _grouped(w=Z(E, N, K, dt=F16)), {}),
    ("3-d operand: column stride", "gemm_nt_grouped", lambda: _grouped(w=Z(E, K, N).transpose(1, 2)), {}),
    ("optional operand: wrong dtype", "pool_norm", lambda: dict(hidden=Z(B, S, H), mask=Z(B, S, dt=I64), method="mean", normalize=True,
                                                                instr_len=Z(B, dt=I64)), {}),
    ("moe_route: fp32 rows", "moe_route", lambda: dict(x=Z(T, H, dt=F32), gate_w=Z(E, H)), {}),
    ("moe_route_f32: bf16 rows", "moe_route_f32", lambda: dict(h=Z(T, H), ln_w=Z(H), eps=1e-5, gate_w=Z(E, H)), {}),
    ("moe_router_top2: fp32 rows without ln_w", "moe_router_top2",
     lambda: dict(x=Z(T, H, dt=F32), gate_w=Z(E, H), experts=Z(T, 2, dt=I32), weights=Z(T, 2, dt=F32)), {}),
    ("embed_gather: fp16 table needs an fp16 out", "embed_gather", lambda: dict(table=Z(V, H, dt=F16), ids=Z(T, dt=I64)), {}),
    ("rmsnorm: fp16 rows, fp32 out", "rmsnorm", lambda: dict(x=Z(T, H, dt=F16), w=Z(H), eps=1e-5, out=Z(T, H, dt=F32)), {}),
    ("pool_norm: unknown method", "pool_norm", lambda: dict(hidden=Z(B, S, H), mask=Z(B, S, dt=I64), method="weighted_mean", normalize=True), {}),
    ("pool_norm_varlen: unknown method", "pool_norm_varlen", lambda: dict(hidden=Z(TS, H), cu_seqlens=ints(0, 7, TS), method="max", normalize=True), {}),
    ("attn_bidir: window without causal", "attn_bidir", lambda: _attn(window=3), {}),
    ("attn_bidir f16: window without causal", "attn_bidir", lambda: _attn(F16, window=3), {}),
    ("attn_bidir_varlen: window without causal", "attn_bidir_varlen", lambda: _attn_varlen(window=3), {}),
    ("attn_bidir_bwd: window without causal", "attn_bidir_bwd", lambda: _attn_bwd(window=3), {}),
    ("attn_bidir_varlen_bwd: window without causal", "attn_bidir_varlen_bwd", lambda: _attn_varlen_bwd(window=3), {}),
    ("attn_bidir: rows", "attn_bidir", lambda: _attn(S=S + 1), {}),
    ("gemm_nt: fp16 swiglu_stacked_save", "gemm_nt", lambda: _gemm(EPI_SWIGLU_STACKED_SAVE, F16, residual=Z(T, N, dt=F16)), {}),
    ("gemm_nt: fp16 swiglu_bwd", "gemm_nt", lambda: _gemm(EPI_SWIGLU_BWD, F16, residual=Z(T, 2 * N, dt=F16)), {}),
    ("gemm_nt: K mismatch", "gemm_nt", lambda: dict(a=Z(T, K), w=Z(N, K + 8)), {}),
    ("gemm_nt: out shape under swiglu", "gemm_nt", lambda: _gemm(EPI_SWIGLU, out=Z(T, N)), {}),
    ("gemm_nt: residual missing", "gemm_nt", lambda: _gemm(EPI_RESIDUAL), {}),
    ("gemm_nt: residual shape under swiglu_bwd", "gemm_nt", lambda: _gemm(EPI_SWIGLU_BWD, residual=Z(T, N)), {}),
    ("gemm_nt_pair: shapes", "gemm_nt_pair", lambda: dict(a1=Z(T, K), w1=Z(N, K), out1=Z(T, N), a2=Z(6, K), w2=Z(16, K), out2=Z(6, N)), {}),
    ("gemm_nt_grouped: K mismatch", "gemm_nt_grouped", lambda: _grouped(a=Z(T, K + 8)), {}),
    ("gemm_nt_grouped: out shape under swiglu", "gemm_nt_grouped", lambda: _grouped(epilogue=EPI_SWIGLU, out=Z(2 * T, N)), {}),
    ("gemm_nt_grouped_epi: out shape under swiglu_bwd", "gemm_nt_grouped_epi", lambda: _grouped(epilogue=EPI_SWIGLU_BWD, out=Z(2 * T, N),
                                                                                             residual=Z(2 * T, 2 * N)), {}),
    ("gemm_nt_grouped_epi: residual shape", "gemm_nt_grouped_epi", lambda: _grouped(epilogue=EPI_SWIGLU_STACKED_SAVE, residual=Z(2 * T, 2 * N)), {}),
    ("gemm_nt_grouped_epi: residual missing", "gemm_nt_grouped_epi", lambda: _grouped(epilogue=EPI_SWIGLU_BWD), {}),
    ("transpose: wrong dtype", "transpose", lambda: dict(x=Z(4, 6, dt=F32)), {}),
    ("transpose: cpu tensor", "transpose", lambda: dict(x=Z(4, 6)), dict(cpu=True)),
    ("transpose: out too narrow", "transpose", lambda: dict(x=Z(4, 6), out=Z(6, 2)), {}),
    ("gemv_expert: expert int64", "gemv_expert", lambda: dict(x=Z(B, K), w_stack=Z(E, N, K), expert=Z(1, dt=I64)), {}),
    ("gemv_expert: cpu tensor", "gemv_expert", lambda: dict(x=Z(B, K), w_stack=Z(E, N, K), expert=Z(1, dt=I32)), dict(cpu=True)),
    ("rmsnorm_gemv: fp16 without deferred", "rmsnorm_gemv", lambda: _norm_proj(F16), {}),
    ("rope_kv_append: table shorter than the cache", "rope_kv_append", lambda: _cache(cos=Z(4, D, dt=F32)), {}),
    ("attn_decode_rope: table shorter than the cache", "attn_decode_rope", lambda: _cache(cos=Z(4, D, dt=F32), out=Z(B, NQ * D), workspace=Z(4096, dt=F32)), {}),
    ("rope_kv_append_rows: one lens per row", "rope_kv_append_rows", lambda: _cache(rows=3, lens=Z(B, dt=I32), cache_row=Z(3, dt=I32)), {}),
    ("kv_append_chunk: rows per sequence", "kv_append_chunk", lambda: _without(_cache(rows=B * 4 + 1, lens=ints(1, 2), plen=ints(3, 4)), "cos", "sin"), {}),
    ("attn_prefill_cached: one plen per sequence", "attn_prefill_cached", lambda: _q(_cache(rows=B * 4, lens=ints(1, 2), plen=ints(3, 4, 1))), {}),
    ("sample_advance: keys", "sample_advance", lambda: _token(keys=Z(B + 1, dt=I64), **_SAMPLE), {}),
    ("sample_advance: next ids", "sample_advance", lambda: _token(next_ids=Z(1, dt=I64), keys=Z(B, dt=I64), **_SAMPLE), {}),
    ("sample_advance: lens", "sample_advance", lambda: _token(lens=Z(1, dt=I32), keys=Z(B, dt=I64), **_SAMPLE), {}),
    ("sample_advance: history rows", "sample_advance", lambda: _token(history=Z(1, 16, dt=I64), step=Z(1, dt=I32), keys=Z(B, dt=I64), **_SAMPLE), {}),
    ("knn_topk: wrong dtype", "knn_topk", lambda: dict(queries=Z(3, H), embeddings=Z(10, H, dt=F32), k=TOPK), {}),
    ("knn_topk: H mismatch", "knn_topk", lambda: dict(queries=Z(3, H, dt=F32), embeddings=Z(10, H, dt=F32), k=TOPK, transposed=True), {}),
    ("knn_topk: cpu tensor", "knn_topk", lambda: dict(queries=Z(3, H, dt=F32), embeddings=Z(10, H, dt=F32), k=TOPK), dict(cpu=True)),
    ("accum_bf16_from_f32: sizes", "accum_bf16_from_f32", lambda: dict(acc=Z(T, H), x=Z(T, H + 1, dt=F32)), {}),
]


def _extent(t):
    return ((sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()) if t.numel() else 0


def _describe(t):
    return f"{str(t.dtype)[6:]}[{','.join(map(str, t.shape))};{','.join(map(str, t.stride()))}]"


def _tensors(ret):
    return [r for r in (ret if isinstance(ret, tuple) else (ret,)) if torch.is_tensor(r)]


def _recorded(kwargs, ret, lib, allocs, timer):
    """[C calls, returned, scratch, spans] of one finished op call, in the fixture's form"""
    named = [(n, a) for n, a in kwargs.items() if torch.is_tensor(a)]
    rets = _tensors(ret)
    known = [a for _, a in named] + rets
    scratch = [a for a in allocs if not any(a is k for k in known)]
    named += [(f"r{i}", r) for i, r in enumerate(rets)] + [(f"s{i}", s) for i, s in enumerate(scratch)]

    def pointer(p):
        if not isinstance(p, (int, type(None))):
            return type(p).__name__
        if not p:
            return 0
        if p == STREAM:
            return "S"
        for label, t in named:
            off = p - t.data_ptr()
            if 0 <= off < _extent(t):
                return label if off == 0 else f"{label}+{off}"
        return "?"

    calls = []
    for name, args in lib.calls:
        row = [name]
        for a, ty in zip(args, _lib._SIGNATURES[name][1]):
            row.append(pointer(a) if ty is _lib._p or not isinstance(a, (int, float)) else repr(float(a)) if ty is _lib._f else int(a))
        calls.append(row)

    def returned(r):
        if torch.is_tensor(r):
            arg = [n for n, a in kwargs.items() if a is r]
            return "=" + arg[0] if arg else _describe(r)
        return r if r is None or isinstance(r, (bool, int)) else repr(r)
    out = [returned(r) for r in ret] if isinstance(ret, tuple) else returned(ret)
    return [calls, out, [_describe(s) for s in scratch], timer.spans if timer is not None else []]


def run_case(real, op, make, flags, timed):
    kwargs = make()
    timer = _StandInTimer() if timed else None
    with patched(real, timer=timer, **flags) as (lib, allocs):
        ret = getattr(ops, op)(**kwargs)
    return _recorded(kwargs, ret, lib, allocs, timer)


def run_refusal(real, op, make, flags):
    kwargs = make()
    with patched(real, **flags):
        try:
            getattr(ops, op)(**kwargs)
        except Exception as e:      # noqa: BLE001
            return [type(e).__name__, str(e)]
    return None


def run_failing(real, entry, op, make, flags):
    """the message of the GritHipError when ``entry`` answers GRIT_E_BADARG"""
    kwargs = make()
    with patched(real, fail=entry, **flags) as (lib, _):
        with pytest.raises(_lib.GritHipError) as e:
            getattr(ops, op)(**kwargs)
    assert lib.calls[-1][0] == "grit_last_error_string" and lib.calls[-2][0] == entry, (entry, [c[0] for c in lib.calls])
    return str(e.value)


def _failing_message(entry):
    return f"{entry} failed (GRIT_E_BADARG): {LAST_ERROR.decode()}"


def first_case_of_every_entry(trace):
    """entry point with a return code -> the first case of the table that calls it"""
    first = {}
    for case in CASES:
        for call in trace[case[0]][0]:
            if "_workspace_" not in call[0]:
                first.setdefault(call[0], case)
    return first


def live():
    """(trace, refusals, reported) of the revision on the path"""
    real = _lib.load()
    trace = {}
    for cid, op, make, flags in CASES:
        assert cid not in trace, cid
        trace[cid] = run_case(real, op, make, flags, timed=True)
        untimed = run_case(real, op, make, flags, timed=False)
        assert untimed == trace[cid][:3] + [[]], (cid, "the timer changes what is called")
    refusals = {cid: run_refusal(real, op, make, flags) for cid, op, make, flags in REFUSALS}
    reported = {}
    for entry, (_, op, make, flags) in first_case_of_every_entry(trace).items():
        msg = run_failing(real, entry, op, make, flags)
        if msg != _failing_message(entry):
            assert msg.endswith(_failing_message("")), msg
            reported[entry] = msg[:-len(_failing_message(""))]
    return trace, refusals, reported


def record():
    trace, refusals, reported = live()
    assert all(r is not None for r in refusals.values()), [k for k, r in refusals.items() if r is None]
    assert "?" not in json.dumps(trace), "a pointer that belongs to no tensor the recorder knows"
    dumps = lambda v: json.dumps(v, separators=(",", ":"))      # noqa: E731
    with open(GOLDEN, "w") as f:
        f.write('{"cases":{\n' + ",\n".join(f"{dumps(k)}:{dumps(v)}" for k, v in trace.items()) + '\n},"refusals":{\n')
        f.write(",\n".join(f"{dumps(k)}:{dumps(v)}" for k, v in refusals.items()) + '\n},"reported":' + dumps(reported) + "}\n")
    print(f"{len(trace)} cases, {sum(len(v[0]) for v in trace.values())} C calls, {len(refusals)} refusals, misnamed: {reported}")
    print(f"{os.path.getsize(GOLDEN)} bytes -> {GOLDEN} (recorded from {os.path.dirname(os.path.abspath(ops.__file__))})")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def real():
    return _lib.load()


def test_the_table_drives_every_guarded_op_and_reaches_every_entry_point(golden):
    assert list(golden["cases"]) == [c[0] for c in CASES] and list(golden["refusals"]) == [c[0] for c in REFUSALS]
    guarded = {n for n, fn in vars(ops).items() if getattr(fn, "_device_guarded", False)}
    launchers = {n for n, fn in vars(ops).items() if not n.startswith("_") and inspect.isfunction(fn) and fn.__module__ == ops.__name__} - {"set_timer"}
    driven = {c[1] for c in CASES}
    assert guarded and guarded <= launchers and driven == launchers, sorted(launchers ^ driven)
    reached = {call[0] for v in golden["cases"].values() for call in v[0]}
    assert not reached & set(NEVER_CALLED), sorted(reached & set(NEVER_CALLED))
    assert reached | set(NEVER_CALLED) == set(_lib._SIGNATURES), sorted(set(_lib._SIGNATURES) - reached - set(NEVER_CALLED))
    assert "?" not in json.dumps(golden["cases"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_calls_match_the_recording(golden, real, case):
    cid, op, make, flags = case
    want = golden["cases"][cid]
    assert run_case(real, op, make, flags, timed=True) == want
    assert run_case(real, op, make, flags, timed=False) == want[:3] + [[]]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_match_the_recording(golden, real, case):
    cid, op, make, flags = case
    assert run_refusal(real, op, make, flags) == golden["refusals"][cid]


def test_the_recording_misnamed_only_the_four_listed(golden):
    allowed = {e for entries in MISNAMED_BEFORE.values() for e in entries}
    assert set(golden["reported"]) <= allowed, sorted(set(golden["reported"]) - allowed)


def test_a_refused_call_names_the_entry_that_was_called(golden, real):
    first = first_case_of_every_entry(golden["cases"])
    assert set(first) == {n for n in _lib._SIGNATURES if "_workspace_" not in n} - set(NEVER_CALLED)
    wrong = {}
    for entry, (_, op, make, flags) in first.items():
        msg = run_failing(real, entry, op, make, flags)
        if msg != _failing_message(entry):
            wrong[entry] = msg
    assert not wrong, wrong


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    record()
