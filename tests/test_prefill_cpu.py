"""CPU: the prompt-prefill-on-cache entry points (csrc/prefill.hip) -- exported, argument validation without touching the device, hipcc's
resource usage of the attention kernel -- and the decoder's mask -> (plen, positions, last row) helper."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from gritlm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ("grit_kv_append_chunk", "grit_attn_prefill_cached_fwd", "grit_attn_prefill_cached_f16_fwd")


def test_prefill_symbols_are_declared_and_exported():
    lib = _lib.load()
    syms = _lib.header_symbols()
    for s in NEW:
        assert s in syms and s in _lib._SIGNATURES and hasattr(lib, s), s
    assert lib.grit_version() == _lib.ABI_VERSION == 6


def test_prefill_entry_points_reject_bad_arguments():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    for name in ("grit_attn_prefill_cached_fwd", "grit_attn_prefill_cached_f16_fwd"):
        f = getattr(lib, name)
        #       q  k  v  lens plen out  B  P  nq nkv d  Lmax q_stride out_stride
        good = [p, p, p, p, p, p, 2, 5, 4, 2, 128, 256, 1024, 512, 0.088, None]
        call = lambda kw: f(*[kw.get(i, good[i]) for i in range(len(good))])
        assert call({0: None}) == _lib.GRIT_E_BADARG and b"null pointer" in lib.grit_last_error_string()
        assert call({4: None}) == _lib.GRIT_E_BADARG
        assert call({10: 64}) == _lib.GRIT_E_UNSUPPORTED and b"head_dim" in lib.grit_last_error_string()
        assert call({8: 6, 9: 4}) == _lib.GRIT_E_BADARG and b"multiple" in lib.grit_last_error_string()      # nq % nkv
        assert call({7: 0}) == _lib.GRIT_E_BADARG                                                            # P < 1
        assert call({11: 0}) == _lib.GRIT_E_BADARG                                                           # Lmax
        assert call({6: 0}) == _lib.GRIT_E_BADARG                                                            # B
        assert call({12: 256}) == _lib.GRIT_E_BADARG                                                         # q_stride < nq * d
        assert call({0: p + 2}) == _lib.GRIT_E_BADARG and b"aligned" in lib.grit_last_error_string()
        assert call({1: p + 8}) == _lib.GRIT_E_BADARG
    f = lib.grit_kv_append_chunk
    #       qkv k  v  lens plen B  P  nq nkv d  Lmax stride
    good = [p, p, p, p, p, 2, 5, 4, 2, 128, 256, 1024, None]
    call = lambda kw: f(*[kw.get(i, good[i]) for i in range(len(good))])
    assert call({2: None}) == _lib.GRIT_E_BADARG and b"null pointer" in lib.grit_last_error_string()
    assert call({9: 96}) == _lib.GRIT_E_UNSUPPORTED
    assert call({7: 5, 8: 2}) == _lib.GRIT_E_BADARG
    assert call({6: 0}) == _lib.GRIT_E_BADARG
    assert call({10: -1}) == _lib.GRIT_E_BADARG
    assert call({11: 512}) == _lib.GRIT_E_BADARG                                                             # stride < (nq + 2 nkv) d
    assert call({0: p + 4}) == _lib.GRIT_E_BADARG


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
def test_prefill_attention_does_not_spill():
    """exactly the bf16 and the fp16 instantiation; no spill, no scratch; two workgroups (8 waves) per CU = two waves per SIMD, which the
    80 KiB of LDS per workgroup is sized for"""
    ks = _resources("prefill.hip")
    att = [k for k in ks if "attn_prefill_cached_k" in k["name"]]
    assert sorted(k["name"] for k in att) == ["_ZN4grit21attn_prefill_cached_kILb0EEEvPKtS2_S2_PKiS4_Ptiiiillfii",
                                              "_ZN4grit21attn_prefill_cached_kILb1EEEvPKtS2_S2_PKiS4_Ptiiiillfii"], [k["name"] for k in att]
    assert not any("attn_bidir_fwd_k" in k["name"] for k in ks)
    for k in att:
        assert int(k["VGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs"]) + int(k["AGPRs"]) <= 256 and int(k["Occupancy [waves/SIMD]"]) >= 2, k
    for k in ks:
        assert int(k["VGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k


def test_prefill_layout_right_padded():
    from gritlm_amd.decoder import prefill_layout
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0], [1, 0, 0, 0]])
    lens = torch.tensor([0, 37, 700], dtype=torch.int32)
    plen, pos, last = prefill_layout(mask, lens)
    assert plen.dtype == torch.int32 and plen.tolist() == [4, 2, 1]
    assert pos.dtype == torch.int32 and pos.tolist() == [0, 1, 2, 3, 37, 38, 39, 40, 700, 701, 702, 703]
    assert last.dtype == torch.int64 and last.tolist() == [3, 5, 8]
    _, pos_c, _ = prefill_layout(mask, lens, Lmax=702)
    assert pos_c.tolist()[-4:] == [700, 701, 701, 701]
    plen1, pos1, last1 = prefill_layout(torch.ones((1, 3), dtype=torch.int64), torch.tensor([5]))
    assert plen1.tolist() == [3] and pos1.tolist() == [5, 6, 7] and last1.tolist() == [2]


@pytest.mark.parametrize("mask", [[[0, 1, 1], [1, 1, 1]],          # left padding
                                  [[1, 0, 1], [1, 1, 1]],          # a hole
                                  [[1, 1, 1], [0, 0, 0]]])         # a row without a token
def test_prefill_layout_refuses_other_masks(mask):
    from gritlm_amd.decoder import prefill_layout
    with pytest.raises(NotImplementedError):
        prefill_layout(torch.tensor(mask), torch.zeros(2, dtype=torch.int32))


def test_decoder_prefill_mode_is_validated(monkeypatch):
    from gritlm_amd.decoder import PREFILL_MODES, MistralDecoder
    assert PREFILL_MODES == ("rows", "gemm")

    class _Eng:                      # the attributes MistralDecoder.__init__ reads; nothing touches a device before generate()
        cfg = type("C", (), {"num_local_experts": 0})()
        device = torch.device("cpu")
        precision = "bf16"

    monkeypatch.setenv("GRIT_DECODE_PREFILL", "tokens")
    with pytest.raises(ValueError):
        MistralDecoder(_Eng(), torch.zeros((4, 4), dtype=torch.bfloat16))
    monkeypatch.setenv("GRIT_DECODE_PREFILL", "gemm")
    dec = MistralDecoder(_Eng(), torch.zeros((4, 4), dtype=torch.bfloat16))
    assert dec.prefill == "gemm" and dec.last_prefill is None
    monkeypatch.delenv("GRIT_DECODE_PREFILL")
    dec = MistralDecoder(_Eng(), torch.zeros((4, 4), dtype=torch.bfloat16))
    assert dec.prefill == "rows"
    dec.prefill = "bogus"
    with pytest.raises(ValueError):
        dec.generate(torch.zeros((1, 2), dtype=torch.int64), 1)
