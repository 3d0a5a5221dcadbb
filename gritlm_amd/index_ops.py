"""Launchers of include/gritlm_hip_index.h: the search of a bf16 / fp16 RAG index as it lies (``grit_knn16_topk``).  Beside ``ops.py``
rather than in it: the set of public launchers there is pinned by a recorded call trace, like the main header's symbol table."""
from __future__ import annotations

import torch

from . import _lib

_INDEX_DTYPES = (torch.bfloat16, torch.float16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(queries, embeddings_hn, Q, N, H, ld, k):
    lib = _lib.load()
    ws = torch.empty((max(int(lib.grit_knn16_workspace_bytes(Q, N, H, k)), 1),), dtype=torch.uint8, device=queries.device)
    scores = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    index = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    rc = lib.grit_knn16_topk(queries.data_ptr(), embeddings_hn.data_ptr(), int(embeddings_hn.dtype == torch.float16), Q, N, H, ld, k,
                             ws.data_ptr(), scores.data_ptr(), index.data_ptr(), _stream())
    _lib.check(rc, "grit_knn16_topk")
    return scores, index


def knn16_topk(queries: torch.Tensor, embeddings_hn: torch.Tensor, k: int):
    """Exhaustive inner-product search of fp32 ``queries`` [Q,H] against a bf16 / fp16 index in the reference's layout [H,N]
    (rag/index.py:141; unit column stride, any row stride): (scores [Q,k] fp32 descending, indices [Q,k] int64, equal scores lower
    column first).  The queries are not rounded to the index format; no fp32 copy of the index and no [Q,N] score matrix is made."""
    if queries.dtype != torch.float32:
        raise TypeError(f"knn16_topk: fp32 queries expected, got {queries.dtype}")
    if embeddings_hn.dtype not in _INDEX_DTYPES:
        raise TypeError(f"knn16_topk: bf16 or fp16 index expected, got {embeddings_hn.dtype}")
    if queries.dim() != 2 or not queries.is_contiguous():
        raise ValueError("knn16_topk: queries must be a contiguous [Q,H] matrix")
    if embeddings_hn.dim() != 2 or (embeddings_hn.shape[1] > 1 and embeddings_hn.stride(1) != 1):
        raise ValueError("knn16_topk: [H,N] index with unit column stride expected")
    Q, H = queries.shape
    N = embeddings_hn.shape[1]
    if embeddings_hn.shape[0] != H:
        raise ValueError(f"knn16_topk: the queries are {H} wide, the index {embeddings_hn.shape[0]}")
    if not (queries.is_cuda and embeddings_hn.is_cuda):
        raise _lib.GritHipError("knn16_topk: tensors must live on the GPU; the native path has no CPU fallback")
    if embeddings_hn.device != queries.device:
        raise ValueError("knn16_topk: queries and index on different devices")
    ld = embeddings_hn.stride(0) if H > 1 else max(N, 1)
    # the launch goes to the calling thread's current device and stream: make the tensors' device current (as every op of ops.py does)
    if queries.device.index != torch.cuda.current_device():
        with torch.cuda.device(queries.device):
            return _launch(queries, embeddings_hn, Q, N, H, ld, int(k))
    return _launch(queries, embeddings_hn, Q, N, H, ld, int(k))
