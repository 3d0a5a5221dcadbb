"""CPU: the batched-decode GEMM entry points (csrc/decode_gemm.hip) -- exported and in the ctypes table, argument validation without
touching the device, hipcc's resource usage of every instantiation -- and the decoder's batch limits, which refuse before any launch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from gritlm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ("grit_decode_gemm_bf16", "grit_decode_gemm_f16", "grit_rmsnorm_decode_gemm_bf16_deferred", "grit_rmsnorm_decode_gemm_f16_deferred")


def test_decode_gemm_symbols_are_declared_and_exported():
    lib = _lib.load()
    syms = _lib.header_symbols()
    for s in NEW:
        assert s in syms and s in _lib._SIGNATURES and hasattr(lib, s), s
    # additive: the GEMV's signatures are the templates of the new ones
    assert _lib._SIGNATURES["grit_decode_gemm_bf16"] == _lib._SIGNATURES["grit_gemv_bf16"]
    assert _lib._SIGNATURES["grit_decode_gemm_f16"] == _lib._SIGNATURES["grit_gemv_f16"]
    assert _lib._SIGNATURES["grit_rmsnorm_decode_gemm_bf16_deferred"] == _lib._SIGNATURES["grit_rmsnorm_gemv_bf16_deferred"]
    assert _lib._SIGNATURES["grit_rmsnorm_decode_gemm_f16_deferred"] == _lib._SIGNATURES["grit_rmsnorm_gemv_f16_deferred"]


def _buf():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


@pytest.mark.parametrize("name", ["grit_decode_gemm_bf16", "grit_decode_gemm_f16"])
def test_decode_gemm_rejects_bad_arguments(name):
    lib = _lib.load()
    _keep, p = _buf()
    f = getattr(lib, name)
    f16 = name == "grit_decode_gemm_f16"
    U, Bd = _lib.GRIT_E_UNSUPPORTED, _lib.GRIT_E_BADARG
    #       x  W  out B  N   K   ldx ldw ldo epi residual ldr
    good = [p, p, p, 9, 64, 64, 64, 64, 64, 0, None, 0]
    tail = [None, 0, None] if f16 else [None]
    call = lambda kw: f(*[kw.get(i, good[i]) for i in range(len(good))], *tail)
    assert call({0: None}) == Bd and b"null pointer" in lib.grit_last_error_string()
    assert call({1: None}) == Bd and call({2: None}) == Bd
    assert call({3: 0}) == U and b"1..64" in lib.grit_last_error_string()
    assert call({3: 65}) == U and b"1..64" in lib.grit_last_error_string()
    assert call({5: 96, 6: 96, 7: 96}) == U and b"multiple of 64" in lib.grit_last_error_string()      # K % 64
    assert call({4: 24, 8: 24}) == U and b"multiple of 16" in lib.grit_last_error_string()            # N % 16
    assert call({4: 48, 8: 48, 9: 2}) == U and b"SWIGLU" in lib.grit_last_error_string()              # SWIGLU N % 32
    assert call({4: 0}) == Bd and call({5: -64}) == Bd                                                 # sizes
    assert call({6: 32}) == Bd and call({7: 68}) == Bd                                                 # ldx < K, ldw % 8
    assert call({8: 32}) == Bd and b"ldo" in lib.grit_last_error_string()                             # ldo < N
    assert call({0: p + 2}) == Bd and b"aligned" in lib.grit_last_error_string()
    assert call({1: p + 8}) == Bd
    assert call({9: 7}) == Bd and b"unknown epilogue" in lib.grit_last_error_string()
    assert call({9: 1}) == Bd and b"RESIDUAL" in lib.grit_last_error_string()                         # RESIDUAL without residual
    assert call({9: 1, 10: p, 11: 32}) == Bd                                                           # ldr < N
    if f16:
        assert f(*good, p, 64, None) == Bd and b"out16" in lib.grit_last_error_string()               # out16 without RESIDUAL
        assert f(*good[:9], 1, p, 64, p, 32, None) == Bd and b"ldo16" in lib.grit_last_error_string()


@pytest.mark.parametrize("name", ["grit_rmsnorm_decode_gemm_bf16_deferred", "grit_rmsnorm_decode_gemm_f16_deferred"])
def test_rmsnorm_decode_gemm_rejects_bad_arguments(name):
    lib = _lib.load()
    _keep, p = _buf()
    f = getattr(lib, name)
    U, Bd = _lib.GRIT_E_UNSUPPORTED, _lib.GRIT_E_BADARG
    #       x  ln eps  W  out B   N   K   ldx ldw ldo epi
    good = [p, p, 1e-5, p, p, 16, 64, 64, 64, 64, 64, 0, None]
    call = lambda kw: f(*[kw.get(i, good[i]) for i in range(len(good))])
    assert call({1: None}) == Bd and b"null pointer" in lib.grit_last_error_string()
    assert call({0: None}) == Bd
    assert call({11: 1}) == Bd and b"STORE or SWIGLU" in lib.grit_last_error_string()
    assert call({11: 9}) == Bd
    assert call({5: 0}) == U and call({5: 65}) == U
    assert call({7: 32, 8: 32, 9: 32}) == U
    assert call({6: 40, 10: 40}) == U
    assert call({1: p + 4}) == Bd and b"aligned" in lib.grit_last_error_string()


def _resources(src):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(ROOT, "gritlm_amd", "csrc", src),
                        "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)(?: \[-Rpass|$)", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            out.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_decode_gemm_kernels_do_not_spill():
    """14 instantiations: {bf16, fp16} x {STORE, deferred STORE} x {16 rows / 8 waves, 32 rows / 4 waves per workgroup} + {bf16, fp16} x
    RESIDUAL (16 rows / 8 waves) + {bf16, fp16} x {SWIGLU, deferred SWIGLU} (32 rows / 4 waves).  No spill, no scratch; at least two
    waves per SIMD: the 8-wave workgroups are one per CU at N = 4096, and two 4-wave workgroups per CU fit even the deferred-norm forms."""
    ks = [k for k in _resources("decode_gemm.hip") if "decode_gemm_k" in k["name"]]
    assert len(ks) == 14, [k["name"] for k in ks]
    for k in ks:
        assert int(k["VGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs"]) + int(k["AGPRs"]) <= 256 and int(k["Occupancy [waves/SIMD]"]) >= 2, k
        assert int(k["LDS Size [bytes/block]"]) <= 64 * 1024, k


class _Eng:                      # the attributes MistralDecoder.__init__ / generate read before any launch
    def __init__(self, experts=0):
        self.cfg = type("C", (), {"num_local_experts": experts})()
        self.device = torch.device("cpu")
        self.precision = "bf16"


def test_decoder_batch_limits_refuse_before_any_launch(monkeypatch):
    from gritlm_amd import decoder as D
    from gritlm_amd import ops

    def boom(*a, **k):
        raise AssertionError("a kernel was launched")

    for n in ("gemv", "decode_gemm", "rmsnorm_gemv", "rmsnorm_decode_gemm", "embed_gather", "f16_overflow_flag"):
        monkeypatch.setattr(ops, n, boom)
    assert D.MAX_ROWS == 64 and D.GEMV_ROWS == 8
    dec = D.MistralDecoder(_Eng(), torch.zeros((4, 4), dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="64"):
        dec.generate(torch.zeros((65, 3), dtype=torch.int64), 4)
    moe = D.MistralDecoder(_Eng(experts=4), torch.zeros((4, 4), dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        moe.generate(torch.zeros((9, 3), dtype=torch.int64), 4)
