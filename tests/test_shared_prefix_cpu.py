"""CPU: the boundary of share_prefix without a device (include/gritlm_hip_prefix.h, _lib._PREFIX_SIGNATURES, prefix_ops, the host-side
branch of MistralDecoder.generate): exported symbols, the library's refusals, the workspace size, the C argument order of the four
launchers, their Python-side refusals, the arguments' defaults and the kernels' resources."""
import ctypes
import inspect
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gritlm_amd import _lib, prefix_ops
from gritlm_amd.decoder import MistralDecoder, check_sampling

U, BAD = _lib.GRIT_E_UNSUPPORTED, _lib.GRIT_E_BADARG
BF16, F16, F32, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int32
NAMES = {"grit_attn_decode_prefix_kc", "grit_attn_decode_prefix_workspace_floats", "grit_rope_kv_append_tail", "grit_attn_decode_prefix",
         "grit_attn_decode_tail", "grit_attn_decode_prefix_combine"}


def test_prefix_header_table_and_library_agree():
    lib = _lib.load()
    syms = _lib.header_symbols(_lib.PREFIX_HEADER_PATH)
    assert set(syms) == set(_lib._PREFIX_SIGNATURES) == NAMES
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/gritlm_hip_prefix.h but not exported"
    assert not set(_lib._PREFIX_SIGNATURES) & set(_lib._SIGNATURES) and not set(_lib._PREFIX_SIGNATURES) & set(_lib._INDEX_SIGNATURES)
    assert "NATURAL exponent" in open(_lib.PREFIX_HEADER_PATH).read()          # the header states the workspace's convention
    kc = lib.grit_attn_decode_prefix_kc()
    assert kc in (128, 256, 512) and prefix_ops.kc() == kc


def test_workspace_size_and_refused_sizes():
    lib = _lib.load()
    ws, kc = lib.grit_attn_decode_prefix_workspace_floats, lib.grit_attn_decode_prefix_kc()
    assert ws(64, 32, 8, 2048, 64) == 64 * 32 * (2048 // kc + 1) * 130
    assert ws(3, 4, 2, kc + 1, 128) == 3 * 4 * (2 + 2) * 130                    # a started chunk counts
    for B, nq, nkv, Lpre, Ltail in [(0, 4, 2, 256, 64), (3, 0, 2, 256, 64), (3, 4, 0, 256, 64), (3, 4, 3, 256, 64), (3, 4, 2, 0, 64),
                                    (3, 4, 2, 256, 0), (3, 4, 2, 256, 70), (3, 4, 2, 512 * kc, 64), (65536, 4, 2, 256, 64)]:
        assert ws(B, nq, nkv, Lpre, Ltail) == 0, (B, nq, nkv, Lpre, Ltail)
    with pytest.raises(ValueError, match="workspace"):
        prefix_ops.workspace(3, 4, 2, 256, 70, "cpu")


def test_refusals_come_before_the_device_is_touched():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    append = lambda qkv=p, tk=p, lens=p, q16=p, B=6, n=3, nq=4, nkv=2, d=128, Ltail=64, Lpos=512, ld=1024, ld16=512, f16=0: \
        lib.grit_rope_kv_append_tail(qkv, p, p, tk, p, lens, p, q16, B, n, nq, nkv, d, Ltail, Lpos, ld, ld16, f16, None)
    prefix = lambda q=p, ws=p, B0=2, n=3, nq=4, nkv=2, d=128, Lpre=256, Ltail=64, ld=1024: \
        lib.grit_attn_decode_prefix(q, p, p, p, ws, B0, n, nq, nkv, d, Lpre, Ltail, ld, 0.088, 0, None)
    tail = lambda q=p, ws=p, B=6, n=3, nq=4, nkv=2, d=128, Lpre=256, Ltail=64, ld=1024: \
        lib.grit_attn_decode_tail(q, p, p, p, p, ws, B, n, nq, nkv, d, Lpre, Ltail, ld, 0.088, 0, None)
    combine = lambda ws=p, out=p, B=6, nq=4, nkv=2, d=128, Lpre=256, Ltail=64, ld=512: \
        lib.grit_attn_decode_prefix_combine(ws, out, B, nq, nkv, d, Lpre, Ltail, ld, 0, None)
    for call, nulls in ((append, ("qkv", "tk", "lens")), (prefix, ("q", "ws")), (tail, ("q", "ws")), (combine, ("ws", "out"))):
        for null in nulls:
            assert call(**{null: None}) == BAD, null
            assert b"null pointer" in lib.grit_last_error_string()
    assert append(q16=None, f16=1) == BAD                                                  # (q16 belongs to the fp16 form)
    for call in (append, prefix, tail, combine):
        assert call(d=64) == U and b"128" in lib.grit_last_error_string()
    assert append(B=7) == BAD and tail(B=7) == BAD                                         # rows that are no multiple of n
    assert append(ld=1016) == BAD and append(ld16=500, f16=1) == BAD and prefix(ld=500) == BAD and combine(ld=500) == BAD
    assert append(qkv=p + 2) == BAD and prefix(q=p + 2) == BAD and prefix(ws=p + 4) == BAD and tail(ws=p + 4) == BAD
    assert prefix(nq=4, nkv=3) == U and prefix(nq=32, nkv=2) == U                          # whole groups of at most 8 heads
    assert prefix(Ltail=70) == BAD and tail(Lpre=0) == BAD and combine(Ltail=0) == BAD
    kc = lib.grit_attn_decode_prefix_kc()
    assert prefix(Lpre=512 * kc) == U and b"records" in lib.grit_last_error_string()


def test_python_side_refusals():
    """wrong dtypes, non-contiguous rows and n * B0 != B: ValueError, before the device question is asked"""
    nq, nkv, d, n, B0 = 4, 2, 128, 3, 2
    B = n * B0
    qkv, cos = torch.zeros((B, (nq + 2 * nkv) * d), dtype=BF16), torch.zeros((256, 64))
    tk, pk = torch.zeros((B, nkv, 64, d), dtype=BF16), torch.zeros((B0, nkv, 256, d), dtype=BF16)
    lens, plen = torch.zeros((B,), dtype=I32), torch.zeros((B0,), dtype=I32)
    ws, ctx = torch.zeros((B * nq * 2 * 130,)), torch.zeros((B, nq * d), dtype=BF16)            # 1 prefix chunk + 1 tail split per row-head
    ok_append = lambda **k: prefix_ops.rope_kv_append_tail(**{**dict(qkv=qkv, cos=cos, sin=cos, tail_k=tk, tail_v=tk, lens=lens, plen=plen, n=n,
                                                                   nq=nq, nkv=nkv, d=d), **k})
    ok_prefix = lambda **k: prefix_ops.attn_decode_prefix(**{**dict(q=qkv, prefix_k=pk, prefix_v=pk, plen=plen, ws=ws, n=n, nq=nq, nkv=nkv, d=d,
                                                                  Ltail=64), **k})
    ok_tail = lambda **k: prefix_ops.attn_decode_tail(**{**dict(q=qkv, tail_k=tk, tail_v=tk, lens=lens, plen=plen, ws=ws, n=n, nq=nq, nkv=nkv, d=d,
                                                              Lpre=256), **k})
    with pytest.raises(_lib.GritHipError, match="no CPU fallback"):                          # every check passed: the device question
        ok_append()
    with pytest.raises(ValueError, match="n \\* B0 != B"):
        ok_append(n=4)
    with pytest.raises(ValueError, match="n \\* B0 != B"):
        ok_prefix(plen=torch.zeros((3,), dtype=I32))
    with pytest.raises(ValueError, match="n \\* B0 != B"):
        ok_tail(n=2)
    with pytest.raises(ValueError, match="qkv: expected"):
        ok_append(qkv=qkv.float())                                                           # fp32 rows go with fp16 tails only
    with pytest.raises(ValueError, match="q: expected"):
        ok_prefix(q=qkv.to(F16))
    with pytest.raises(ValueError, match="lens: expected"):
        ok_tail(lens=lens.long())
    with pytest.raises(ValueError, match="bf16 or fp16"):
        ok_tail(tail_k=tk.float(), tail_v=tk.float())
    with pytest.raises(ValueError, match="q16"):
        ok_append(qkv=qkv.float(), tail_k=tk.to(F16), tail_v=tk.to(F16))
    with pytest.raises(ValueError, match="contiguous rows"):
        ok_append(qkv=torch.zeros((B, 2 * (nq + 2 * nkv) * d), dtype=BF16)[:, ::2])
    with pytest.raises(ValueError, match="contiguous rows"):
        prefix_ops.attn_decode_prefix_combine(ws, torch.zeros((B, 2 * nq * d), dtype=BF16)[:, ::2], nq, nkv, d, 256, 64)
    with pytest.raises(ValueError, match="must be contiguous"):
        ok_prefix(prefix_k=pk[:, :, ::2], prefix_v=pk[:, :, ::2])
    with pytest.raises(ValueError, match="workspace: expected"):
        prefix_ops.attn_decode_prefix_combine(ws.double(), ctx, nq, nkv, d, 256, 64)
    # a workspace sized for other lengths would be written past its end: refused by all three launches that touch it
    with pytest.raises(ValueError, match="workspace of .* floats"):
        ok_prefix(Ltail=128)
    with pytest.raises(ValueError, match="workspace of .* floats"):
        ok_tail(Lpre=256 + prefix_ops.kc())
    with pytest.raises(ValueError, match="workspace of .* floats"):
        prefix_ops.attn_decode_prefix_combine(ws[:-1], ctx, nq, nkv, d, 256, 64)
    with pytest.raises(ValueError, match="sizes not built"):
        ok_prefix(Ltail=70)


_REAL = _lib.load()


class _StandIn:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in NAMES:
            raise AttributeError(name)
        if name == "grit_attn_decode_prefix_workspace_floats":          # (the launchers' size check: answered by the library, not recorded)
            return _REAL.grit_attn_decode_prefix_workspace_floats
        return lambda *a: self.calls.append((name, a)) or 0


@pytest.mark.parametrize("dt,f16", [(BF16, 0), (F16, 1)])
def test_c_arguments_are_passed_in_header_order(monkeypatch, dt, f16):
    """nothing is launched: for the calls, Tensor.is_cuda answers True and the library is a stand-in that records"""
    lib = _StandIn()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)
    monkeypatch.setattr(prefix_ops, "_stream", lambda: 0x57AE40)
    monkeypatch.setattr(prefix_ops._lib, "load", lambda: lib)
    nq, nkv, d, n, B0, Lpre, Ltail, Lpos = 4, 2, 128, 3, 2, 512, 128, 640
    B, qdt = n * B0, F32 if f16 else BF16
    qkv = torch.zeros((B, (nq + 2 * nkv) * d + 64), dtype=qdt)[:, :(nq + 2 * nkv) * d]      # row stride 1088
    q16 = torch.zeros((B, nq * d + 8), dtype=F16)[:, :nq * d] if f16 else None              # row stride 520
    cos, sin = torch.zeros((Lpos, 64)), torch.zeros((Lpos, 64))
    tk, tv = torch.zeros((B, nkv, Ltail, d), dtype=dt), torch.zeros((B, nkv, Ltail, d), dtype=dt)
    pk, pv = torch.zeros((B0, nkv, Lpre, d), dtype=dt), torch.zeros((B0, nkv, Lpre, d), dtype=dt)
    lens, plen, ws = torch.zeros((B,), dtype=I32), torch.zeros((B0,), dtype=I32), torch.zeros((B * nq * (Lpre // _REAL.grit_attn_decode_prefix_kc() + Ltail // 64) * 130,))
    ctx = torch.zeros((B, nq * d + 16), dtype=dt)[:, :nq * d]                               # row stride 528
    prefix_ops.rope_kv_append_tail(qkv, cos, sin, tk, tv, lens, plen, n, nq, nkv, d, q16=q16)
    q = q16 if f16 else qkv
    prefix_ops.attn_decode_prefix(q, pk, pv, plen, ws, n, nq, nkv, d, Ltail, scale=0.25)
    prefix_ops.attn_decode_tail(qkv, tk, tv, lens, plen, ws, n, nq, nkv, d, Lpre)
    assert prefix_ops.attn_decode_prefix_combine(ws, ctx, nq, nkv, d, Lpre, Ltail) is ctx
    S = 0x57AE40
    assert lib.calls == [
        ("grit_rope_kv_append_tail", (qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), tk.data_ptr(), tv.data_ptr(), lens.data_ptr(), plen.data_ptr(),
                                      q16.data_ptr() if f16 else 0, B, n, nq, nkv, d, Ltail, Lpos, 1088, 520 if f16 else 0, f16, S)),
        ("grit_attn_decode_prefix", (q.data_ptr(), pk.data_ptr(), pv.data_ptr(), plen.data_ptr(), ws.data_ptr(), B0, n, nq, nkv, d, Lpre, Ltail,
                                     520 if f16 else 1088, 0.25, f16, S)),
        ("grit_attn_decode_tail", (qkv.data_ptr(), tk.data_ptr(), tv.data_ptr(), lens.data_ptr(), plen.data_ptr(), ws.data_ptr(), B, n, nq, nkv, d,
                                   Lpre, Ltail, 1088, d ** -0.5, f16, S)),
        ("grit_attn_decode_prefix_combine", (ws.data_ptr(), ctx.data_ptr(), B, nq, nkv, d, Lpre, Ltail, 528, f16, S))]
    for (name, args) in lib.calls:
        assert len(args) == len(_lib._PREFIX_SIGNATURES[name][1]), name


def test_a_refusal_of_the_library_raises(monkeypatch):
    class Refusing:
        grit_attn_decode_prefix_workspace_floats = _REAL.grit_attn_decode_prefix_workspace_floats

        def grit_attn_decode_prefix_combine(self, *a):
            return BAD

        def grit_last_error_string(self):
            return b"stand-in"
    lib = Refusing()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)
    monkeypatch.setattr(prefix_ops, "_stream", lambda: 0)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    with pytest.raises(_lib.GritHipError, match="grit_attn_decode_prefix_combine"):
        prefix_ops.attn_decode_prefix_combine(torch.zeros((2 * 4 * 2 * 130,)), torch.zeros((2, 512), dtype=BF16), 4, 2, 128, 256, 64)


# ------------------------------------------------------------------------------------------------------------------ the host-side branch
class _Reached(Exception):
    pass


def _host_decoder(moe=False):
    """a decoder without an engine behind it: generate() up to the first allocation, which reports (rows, cache length) and ends the call"""
    dec = object.__new__(MistralDecoder)
    cfg = types.SimpleNamespace(num_attention_heads=4, num_key_value_heads=2, head_dim=128)
    dec.eng = types.SimpleNamespace(precision="bf16", window_keys=0, cfg=cfg)
    dec.cfg, dec.device, dec.moe, dec.prefill, dec.precision, dec.on_overflow = cfg, "cpu", moe, "rows", None, "raise"

    def _state(B, Lmax, f16=False):
        raise _Reached(B, Lmax)
    dec._state = _state
    return dec


def test_share_prefix_defaults_and_the_host_side_branch():
    from gritlm_amd import GritLM
    assert inspect.signature(MistralDecoder.generate).parameters["share_prefix"].default is False
    assert inspect.signature(GritLM.sample_native).parameters["share_prefix"].default is False
    check_sampling(1.0, 50, 1.0, 1, do_sample=False)                    # greedy, n = 1: what share_prefix=True is a no-op on
    with pytest.raises(ValueError, match="do_sample"):
        check_sampling(1.0, 50, 1.0, 2, do_sample=False)
    dec, ids = _host_decoder(), torch.zeros((3, 5), dtype=torch.int64)
    past = [(torch.zeros((3, 2, 300, 128)), torch.zeros((3, 2, 300, 128)))]
    for kw in (dict(), dict(share_prefix=True), dict(do_sample=True, seed=1, share_prefix=True)):
        with pytest.raises(_Reached) as e:                               # n = 1: the plain state -- 3 rows, the cache holds the new tokens
            dec.generate(ids, 40, past_key_values=past, **kw)
        assert e.value.args == (3, 512), kw
    with pytest.raises(_Reached) as e:                                   # n = 4 expanded: 12 rows
        dec.generate(ids, 40, past_key_values=past, do_sample=True, seed=1, num_return_sequences=4)
    assert e.value.args == (12, 512)
    with pytest.raises(_Reached) as e:                                   # n = 4 shared: the prompt phase on the 3 input rows, the cache ends with the prompt
        dec.generate(ids, 40, past_key_values=past, do_sample=True, seed=1, num_return_sequences=4, share_prefix=True)
    assert e.value.args == (3, 512) and (300 + 5 + 255) // 256 * 256 == 512
    with pytest.raises(_Reached) as e:
        dec.generate(ids, 300, past_key_values=past, do_sample=True, seed=1, num_return_sequences=4, share_prefix=True)
    assert e.value.args == (3, 512)                                      # ... whatever max_new_tokens is (the expanded call: 768)
    with pytest.raises(ValueError, match="do_sample"):
        dec.generate(ids, 4, num_return_sequences=2, share_prefix=True)
    with pytest.raises(NotImplementedError, match="batch <= 64"):        # the refusals stay: B0 n <= 64
        dec.generate(ids, 4, do_sample=True, num_return_sequences=22, share_prefix=True)
    dec.eng.window_keys = 128
    with pytest.raises(NotImplementedError, match="sliding window"):
        dec.generate(ids, 4, past_key_values=past, do_sample=True, num_return_sequences=4, share_prefix=True)
    moe = _host_decoder(moe=True)
    with pytest.raises(NotImplementedError, match="share_prefix"):
        moe.generate(ids[:1], 4, do_sample=True, num_return_sequences=2, share_prefix=True)
    with pytest.raises(_Reached):                                        # (without the flag a sparse-MoE engine samples as before)
        moe.generate(ids[:1], 4, do_sample=True, num_return_sequences=2, seed=1)


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_prefix_kernels_do_not_spill():
    """compiled the way test_kernel_resources.py compiles its sources: four kernels x two operand formats, zero VGPR spills and zero
    scratch, and the MFMA kernel keeps the two waves per SIMD of attn_prefill_cached_k"""
    from test_kernel_resources import _resources
    ks = _resources("decode_prefix.hip")
    names = [k["name"] for k in ks]
    for needle in ("rope_kv_append_tail_k", "attn_decode_prefix_k", "attn_decode_tail_k", "attn_decode_prefix_combine_k"):
        assert sum(needle in n for n in names) == 2, (needle, names)
    assert len(ks) == 8, names
    for k in ks:
        assert int(k["VGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        if "attn_decode_prefix_k" in k["name"]:
            assert int(k["Occupancy [waves/SIMD]"]) >= 2, k
