"""CPU: the 16-bit index search's boundary (include/gritlm_hip_index.h, _lib._INDEX_SIGNATURES, index_ops.knn16_topk) without a device:
exported symbols, every documented refusal, the workspace cap, the Python-side checks, the C argument order, and the kernels' resources."""
import ctypes
import os

import pytest
import torch

from gritlm_amd import _lib, index_ops

U, B = _lib.GRIT_E_UNSUPPORTED, _lib.GRIT_E_BADARG


def _cap(Q, N, H, k):
    return 2 * 1024 * Q * k * 12 + 8 * Q * (H + 64) + 4096


def test_index_header_table_and_library_agree():
    lib = _lib.load()
    syms = _lib.header_symbols(_lib.INDEX_HEADER_PATH)
    assert set(syms) == set(_lib._INDEX_SIGNATURES) == {"grit_knn16_workspace_bytes", "grit_knn16_topk"}
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/gritlm_hip_index.h but not exported"
    assert "rag/index.py:97-104" in open(_lib.INDEX_HEADER_PATH).read()
    assert not set(_lib._INDEX_SIGNATURES) & set(_lib._SIGNATURES)


def test_refusals_come_before_the_device_is_touched():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    call = lambda q=p, e=p, f16=0, Q=2, N=100, H=64, ld=100, k=5, ws=p, os_=p, oi=p: lib.grit_knn16_topk(q, e, f16, Q, N, H, ld, k, ws, os_, oi, None)
    for null in ("q", "e", "ws", "os_", "oi"):
        assert call(**{null: None}) == B, null
        assert b"null pointer" in lib.grit_last_error_string()
    assert call(ld=99) == B and b"ld" in lib.grit_last_error_string()
    assert call(e=p + 1) == B and b"odd" in lib.grit_last_error_string()
    assert call(e=p + 1, f16=1) == B
    assert call(Q=-1) == B and call(N=0) == B and call(N=-5, ld=100) == B and call(H=0) == B and call(H=-64) == B
    assert call(k=0) == U and call(k=-1) == U and call(k=101) == U                    # k outside 1 .. min(N, 1024)
    assert call(N=5000, ld=5000, k=1025) == U and b"1024" in lib.grit_last_error_string()
    assert call(Q=65536) == U and b"65535" in lib.grit_last_error_string()
    assert call(N=2 ** 31, ld=2 ** 31) == U and b"2^31" in lib.grit_last_error_string()
    assert call(Q=0) == _lib.GRIT_OK and call(Q=0, q=None, e=None, ws=None) == _lib.GRIT_OK


@pytest.mark.parametrize("Q,N,H,k", [(16, 2 ** 30, 4096, 100), (512, 21 * 10 ** 6, 4096, 100), (1, 37, 64, 37),
                                      (1, 2 ** 31 - 1, 4096, 1), (65535, 2 ** 31 - 1, 1, 1024), (3, 300, 5, 300)])
def test_workspace_stays_under_the_cap(Q, N, H, k):
    """(the first three are the sizes the cap was stated for; then the corners: one query of width 4096 with k = 1 on the longest index --
    where a query tile padded to 32 rows would break the cap --, the largest Q and k, a width that is no multiple of the K-tile)"""
    ws = _lib.load().grit_knn16_workspace_bytes(Q, N, H, k)
    assert 0 < ws <= _cap(Q, N, H, k), (ws, _cap(Q, N, H, k))


def test_workspace_is_zero_for_refused_sizes():
    ws = _lib.load().grit_knn16_workspace_bytes
    for Q, N, H, k in [(0, 100, 64, 5), (-1, 100, 64, 5), (2, 0, 64, 5), (2, 100, 0, 5), (2, 100, 64, 0), (2, 100, 64, 101), (2, 5000, 64, 1025),
                       (65536, 100, 64, 5), (2, 2 ** 31, 64, 5)]:
        assert ws(Q, N, H, k) == 0, (Q, N, H, k)


def test_python_side_refusals():
    q, e = torch.zeros((3, 64)), torch.zeros((64, 10), dtype=torch.bfloat16)
    with pytest.raises(_lib.GritHipError, match="no CPU fallback"):
        index_ops.knn16_topk(q, e, 2)
    with pytest.raises(TypeError, match="bf16 or fp16"):
        index_ops.knn16_topk(q, e.float(), 2)
    with pytest.raises(TypeError, match="fp32 queries"):
        index_ops.knn16_topk(q.to(torch.bfloat16), e, 2)
    with pytest.raises(ValueError, match="wide"):
        index_ops.knn16_topk(torch.zeros((3, 32)), e, 2)
    with pytest.raises(ValueError, match="unit column stride"):
        index_ops.knn16_topk(q, torch.zeros((10, 64), dtype=torch.float16).t(), 2)
    with pytest.raises(ValueError, match="contiguous"):
        index_ops.knn16_topk(torch.zeros((3, 128))[:, ::2], e, 2)


class _StandIn:
    def __init__(self, real):
        self.real, self.calls = real, []

    def grit_knn16_workspace_bytes(self, *a):
        self.calls.append(("grit_knn16_workspace_bytes", a))
        return self.real.grit_knn16_workspace_bytes(*a)

    def grit_knn16_topk(self, *a):
        self.calls.append(("grit_knn16_topk", a))
        return 0


@pytest.mark.parametrize("dt,is_f16", [(torch.bfloat16, 0), (torch.float16, 1)])
def test_c_arguments_are_passed_in_header_order(monkeypatch, dt, is_f16):
    """nothing is launched: for the call, Tensor.is_cuda answers True and the library is a stand-in that records"""
    real = _lib.load()
    lib = _StandIn(real)
    made = []
    empty = torch.empty
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)
    monkeypatch.setattr(index_ops, "_stream", lambda: 0x57AE40)
    monkeypatch.setattr(index_ops._lib, "load", lambda: lib)
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(empty(*a, **k)) or made[-1])
    q = torch.zeros((3, 64))
    e = torch.zeros((64, 16), dtype=dt)[:, :10]                      # row stride 16
    scores, index = index_ops.knn16_topk(q, e, 2)
    ws = made[0]
    assert scores.shape == (3, 2) and scores.dtype == torch.float32 and index.shape == (3, 2) and index.dtype == torch.int64
    assert ws.dtype == torch.uint8 and ws.numel() == real.grit_knn16_workspace_bytes(3, 10, 64, 2)
    assert lib.calls == [("grit_knn16_workspace_bytes", (3, 10, 64, 2)),
                         ("grit_knn16_topk", (q.data_ptr(), e.data_ptr(), is_f16, 3, 10, 64, 16, 2, ws.data_ptr(), scores.data_ptr(),
                                              index.data_ptr(), 0x57AE40))]
    assert len(_lib._INDEX_SIGNATURES["grit_knn16_topk"][1]) == 12 and len(_lib._INDEX_SIGNATURES["grit_knn16_workspace_bytes"][1]) == 4


def test_a_refusal_of_the_library_raises(monkeypatch):
    class Refusing(_StandIn):
        def grit_knn16_topk(self, *a):
            return B

        def grit_last_error_string(self):
            return b"stand-in"
    lib = Refusing(_lib.load())
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)
    monkeypatch.setattr(index_ops, "_stream", lambda: 0)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    with pytest.raises(_lib.GritHipError, match="grit_knn16_topk"):
        index_ops.knn16_topk(torch.zeros((3, 64)), torch.zeros((64, 10), dtype=torch.bfloat16), 2)


def test_host_half_index_keeps_the_widened_route_and_gpu_route_is_selected_by_placement(monkeypatch):
    """rag.DistributedIndex: a 16-bit index on the host is widened for ops.knn_topk; one that reports itself on the GPU goes to
    index_ops.knn16_topk as it lies -- the very tensor, no fp32 copy kept."""
    from gritlm_amd import rag
    seen = []
    monkeypatch.setattr(rag.ops, "knn_topk", lambda q, emb, k, transposed=False: seen.append(("widened", emb.dtype)) or
                        (torch.zeros((q.shape[0], k)), torch.zeros((q.shape[0], k), dtype=torch.int64)))
    monkeypatch.setattr(rag.index_ops, "knn16_topk", lambda q, emb, k: seen.append(("in place", emb)) or
                        (torch.zeros((q.shape[0], k)), torch.zeros((q.shape[0], k), dtype=torch.int64)))
    idx = rag.DistributedIndex(dtype=torch.float16)
    idx.is_in_gpu = False
    idx.init_embeddings([{"id": i} for i in range(5)], 8)
    idx.search_knn(torch.zeros((2, 8)), 3)
    assert seen == [("widened", torch.float32)]
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    idx.search_knn(torch.zeros((2, 8)), 3)
    assert seen[1][0] == "in place" and seen[1][1] is idx.embeddings


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_knn16_kernels_do_not_spill():
    """compiled the way test_kernel_resources.py compiles its sources: the query split per format and the scan per (format, staging
    path) -- zero VGPR spills, zero scratch, and the two waves per SIMD the scan's launch bound asks for"""
    from test_kernel_resources import _resources
    ks = _resources("knn16.hip")
    names = [k["name"] for k in ks]
    assert sum("knn16_split_k" in n for n in names) == 2 and sum("knn16_scan_k" in n for n in names) == 4 and len(ks) == 6, names
    for k in ks:
        assert int(k["VGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        if "knn16_scan_k" in k["name"]:
            assert int(k["Occupancy [waves/SIMD]"]) >= 2, k
