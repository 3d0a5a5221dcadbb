"""Sampled decoding (grit_sample_advance, MistralDecoder.generate(do_sample=True), GritLM.sample_native) without a GPU: the entry points
are declared and exported, bad arguments are refused before any launch, and the numpy restatement the GPU tests compare the kernel
against -- Philox4x32-10, the Gumbel noise, the kept set of include/gritlm_hip.h -- reproduces the Random123 known answers and
transformers' own warpers.  The kernels compile without spills or scratch."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gritlm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMS = ("grit_sample_advance", "grit_sample_advance_f32")


# ---------------------------------------------------------------------------------------------------- the restatement (numpy)
def philox4x32_10(ctr, key):
    """Philox4x32-10 with the Random123 constants: ctr uint32 [..., 4], key (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(ctr[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M, p1 >> np.uint64(32), p1 & M
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(key64: int, t: int, V: int):
    """u_v = ((x >> 8) + 1/2) 2^-24 of the header's contract, fp64 [V]: counter (v >> 2, t, 0, 0), word v & 3"""
    key64 %= 2 ** 64
    q = np.arange((V + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q, np.full_like(q, t), np.zeros_like(q), np.zeros_like(q)], axis=-1)
    x = philox4x32_10(ctr, (key64 & 0xFFFFFFFF, key64 >> 32)).reshape(-1)[:V]
    return ((x >> 8).astype(np.float64) + 0.5) * 2.0 ** -24


def scores(logits, T):
    """s = fp32(logit / T); NaN -> -inf (excluded); +inf -> FLT_MAX"""
    s = (np.asarray(logits, np.float32) / np.float32(T)).astype(np.float32)
    s = np.where(np.isnan(s), np.float32(-np.inf), s)
    return np.where(s == np.inf, np.finfo(np.float32).max, s).astype(np.float32)


def kept(logits, T, top_k, top_p, with_margin=False):
    """the kept set of include/gritlm_hip.h (bool [V]); with_margin: also min_v |A_v / Z - top_p| over the top-k set (the distance of
    the top-p boundary from a decision; 1.0 when top-p is off)"""
    s = scores(logits, T)
    V = s.shape[0]
    keep = np.isfinite(s)
    if not keep.any():
        return (keep, 1.0) if with_margin else keep
    if 0 < top_k < V and keep.sum() > top_k:
        kth = np.sort(s[keep])[::-1][top_k - 1]
        keep &= s >= kth
    margin = 1.0
    if top_p < 1.0:
        M = s[keep].max()
        m = np.where(keep, np.floor(np.exp((s - M).astype(np.float32)).astype(np.float64) * 2.0 ** 32), 0.0)
        Z = m.sum()
        order = np.argsort(s[keep], kind="stable")
        sv, cm = s[keep][order], np.cumsum(m[keep][order])
        le = np.searchsorted(sv, s, side="right")                       # kept tokens with a score <= s_v
        A = Z - np.where(le > 0, cm[np.maximum(le - 1, 0)], 0.0)          # kept mass strictly above s_v
        thr = max(math.ceil(float(np.float32(top_p)) * Z), 1)
        d = np.abs(A[keep & (A > 0)] / Z - float(np.float32(top_p)))          # (the maxima, A = 0, are kept whatever top_p is)
        margin = float(d.min()) if d.size else 1.0
        keep &= (A < thr) & (m > 0)
    return (keep, margin) if with_margin else keep


def draw(logits, T, top_k, top_p, key64, t):
    """(token, best - second perturbed score) of the Gumbel-max draw in fp64 (token 0 for a row with nothing kept)"""
    keep = kept(logits, T, top_k, top_p)
    if not keep.any():
        return 0, np.inf
    u = uniforms(key64, t, keep.shape[0])
    z = np.where(keep, scores(logits, T).astype(np.float64) - np.log(-np.log(u)), -np.inf)
    tok = int(np.argmax(z))
    two = np.sort(z)[-2:]
    return tok, float(two[1] - two[0])


def probs(logits, T, top_k, top_p, mode="header"):
    """fp64 probabilities of the kept set.  mode "header": the kernel's rule; "no_temperature": the same filters on T = 1; "p_first":
    top-p applied before the temperature (the two orderings the distribution test must tell apart)."""
    if mode == "no_temperature":
        T = 1.0
    x = scores(logits, T).astype(np.float64)
    if mode == "p_first":
        keep = kept(logits, 1.0, top_k, top_p)
    else:
        keep = kept(logits, T, top_k, top_p)
    w = np.where(keep, np.exp(x - x[keep].max()), 0.0)
    return w / w.sum()


def hf_kept(logits, T, top_k, top_p):
    """transformers' TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, as _get_logits_processor builds them"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    sc = torch.from_numpy(np.asarray(logits, np.float32)).view(1, -1)
    ids = torch.zeros((1, 1), dtype=torch.long)
    if T != 1.0:
        sc = TemperatureLogitsWarper(T)(ids, sc)
    if top_k != 0:
        sc = TopKLogitsWarper(top_k=top_k)(ids, sc)
    if top_p < 1.0:
        sc = TopPLogitsWarper(top_p=top_p)(ids, sc)
    return torch.isfinite(sc[0]).numpy()


# ---------------------------------------------------------------------------------------------------- tests
def test_symbols_declared_exported_and_typed():
    lib = _lib.load()
    syms = _lib.header_symbols()
    for s in SYMS:
        assert s in syms and s in _lib._SIGNATURES and hasattr(lib, s), s
    assert _lib.ABI_VERSION == 6 and lib.grit_version() == 6
    src = open(_lib.HEADER_PATH).read()
    assert "generative_eval.sh" in src and "Philox4x32-10" in src


def test_bad_arguments_return_badarg_without_a_launch():
    lib = _lib.load()
    buf = (ctypes.c_char * 8192)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    B = _lib.GRIT_E_BADARG
    for fn in (lib.grit_sample_advance, lib.grit_sample_advance_f32):
        call = lambda T=1.0, k=50, p=1.0, keys=p16, ld=16, V=16: fn(p16, ld, V, p16, None, None, 0, None, 1, None, T, k, p, keys)
        for T in (0.0, -1.0, float("nan"), float("inf")):
            assert call(T=T) == B and b"temperature" in lib.grit_last_error_string(), T
        for p in (-0.1, 1.5, float("nan")):
            assert call(p=p) == B and b"top_p" in lib.grit_last_error_string(), p
        assert call(k=-1) == B and b"top_k" in lib.grit_last_error_string()
        assert call(keys=None) == B and b"null" in lib.grit_last_error_string()
        assert call(ld=12) == B                                                        # ld < V
        assert call(ld=20, V=20) == B                                                  # ld % 8
        assert fn(p16 + 2, 16, 16, p16, None, None, 0, None, 1, None, 1.0, 50, 1.0, p16) == B    # alignment


def test_philox_restatement_known_answers():
    f = lambda c, k: [f"{x:08x}" for x in philox4x32_10(np.array([c], np.uint64), k)[0]]
    assert f([0, 0, 0, 0], (0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    m = 0xFFFFFFFF
    assert f([m, m, m, m], (m, m)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert f([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0)) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    u = uniforms(2 ** 64 + 5, 3, 1001)                              # keys are taken mod 2^64
    assert u.shape == (1001,) and (u > 0).all() and (u < 1).all() and np.array_equal(u, uniforms(5, 3, 1001))


@pytest.mark.parametrize("top_k", [0, 1, 50, 700])
@pytest.mark.parametrize("top_p", [0.0, 0.5, 0.95, 1.0])
def test_kept_set_restatement_equals_transformers_warpers(top_k, top_p):
    """tie-free rows (V = 600): the header's kept set is TopKLogitsWarper o TopPLogitsWarper o TemperatureLogitsWarper's; rows whose top-p
    boundary lies within 1e-5 of a decision are set aside (the 2^-32 mass quantum and HF's fp32 cumulative sum may split them); 40 rows
    per setting, 640 over the 16 settings"""
    rng = np.random.default_rng(100 + top_k + int(top_p * 100))
    V, compared = 600, 0
    for i in range(40):
        T = (0.2, 0.7, 1.0, 1.6)[i % 4]
        lg = (rng.standard_normal(V) * (1 + i % 5)).astype(np.float32)
        while len(np.unique(scores(lg, T))) != V:                      # (the division by T can round two logits together)
            lg = (rng.standard_normal(V) * (1 + i % 5)).astype(np.float32)
        mine, margin = kept(lg, T, top_k, top_p, with_margin=True)
        if margin < 1e-5:
            continue
        assert np.array_equal(mine, hf_kept(lg, T, top_k, top_p)), (i, T)
        compared += 1
    assert compared >= 30


def test_kept_set_on_planted_boundary_ties():
    """ties straddling the boundaries follow the header's rule: top-k keeps every tie of the k-th score, top-p keeps a token iff the
    mass strictly above it is < p Z, and p = 0 keeps the tied maxima"""
    lg = np.array([3.0, 1.0, 2.0, 2.0, 2.0, 0.0, 3.0, -1.0], np.float32)
    assert kept(lg, 1.0, 3, 1.0).tolist() == [True, False, True, True, True, False, True, False]     # 3rd largest = 2.0: all three 2.0s
    assert kept(lg, 1.0, 0, 0.0).tolist() == [True, False, False, False, False, False, True, False]  # the two maxima
    e3, e2 = math.exp(0.0), math.exp(-1.0)
    Z = 2 * e3 + 3 * e2 + math.exp(-2.0) + math.exp(-3.0) + math.exp(-4.0)
    p = (2 * e3 + 0.5 * e2) / Z                                     # the boundary inside the tie at 2.0: mass above it is 2 e^0 < p Z
    got = kept(lg, 1.0, 0, p)
    assert got.tolist() == [True, False, True, True, True, False, True, False]
    p_low = (2 * e3) / Z * 0.999                                    # mass above the 2.0 tie (2 e^0) >= p Z: only the maxima
    assert kept(lg, 1.0, 0, p_low).tolist() == [True, False, False, False, False, False, True, False]
    nf = np.array([np.nan, -np.inf, 1.0, np.inf], np.float32)       # NaN / -inf excluded, +inf read as FLT_MAX
    assert kept(nf, 1.0, 0, 1.0).tolist() == [False, False, True, True]
    assert kept(np.array([np.nan, -np.inf], np.float32), 1.0, 50, 0.9).tolist() == [False, False]


def _engine(moe=False):
    from types import SimpleNamespace
    cfg = SimpleNamespace(num_local_experts=8 if moe else 0, num_attention_heads=2, num_key_value_heads=1, head_dim=128, hidden_size=256,
                          intermediate_size=512, num_hidden_layers=1, rms_norm_eps=1e-5, rope_theta=1e4)
    return SimpleNamespace(cfg=cfg, device=torch.device("cpu"), precision="bf16", window_keys=0)


def test_decoder_refuses_bad_sampling_parameters_before_any_launch(monkeypatch):
    from gritlm_amd import ops
    from gritlm_amd.decoder import MistralDecoder

    def boom(*a, **k):
        raise AssertionError("a kernel was launched")

    for name in ("sample_advance", "argmax_advance", "embed_gather", "f16_overflow_flag"):
        monkeypatch.setattr(ops, name, boom)
    ids = torch.zeros((2, 3), dtype=torch.long)
    dec = MistralDecoder(_engine(), torch.zeros((8, 256)))
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
           dict(top_p=-0.01), dict(top_p=1.01), dict(top_p=float("nan")), dict(top_k=-1), dict(top_k=2.5), dict(num_return_sequences=0),
           dict(num_return_sequences=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            dec.generate(ids, 2, do_sample=True, **kw)
    with pytest.raises(ValueError):                                  # greedy copies of a prompt would be identical
        dec.generate(ids, 2, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="64"):
        dec.generate(torch.zeros((13, 3), dtype=torch.long), 2, do_sample=True, num_return_sequences=5)         # 65 rows
    moe = MistralDecoder(_engine(moe=True), torch.zeros((8, 256)))
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        moe.generate(torch.zeros((3, 3), dtype=torch.long), 2, do_sample=True, num_return_sequences=3)          # 9 rows


def test_sample_native_refuses_bad_parameters_and_generate_native_still_refuses_sampling(monkeypatch):
    from types import SimpleNamespace
    from gritlm_amd import GritLM, ops
    monkeypatch.setattr(ops, "sample_advance", lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
    m = GritLM.__new__(GritLM)
    torch.nn.Module.__init__(m)
    m.engine, m._precision, m._decoder = _engine(), "bf16", None
    m.model, m.tokenizer = SimpleNamespace(lm_head=SimpleNamespace(weight=torch.zeros((8, 256)))), SimpleNamespace(eos_token_id=2)
    ids = torch.zeros((4, 3), dtype=torch.long)
    for kw in (dict(temperature=0.0), dict(top_p=2.0), dict(top_k=-3), dict(num_return_sequences=0)):
        with pytest.raises(ValueError):
            m.sample_native(ids, max_new_tokens=2, **kw)
    with pytest.raises(NotImplementedError, match="64"):
        m.sample_native(ids, max_new_tokens=2, num_return_sequences=17)
    with pytest.raises(NotImplementedError, match="sample_native"):
        m.generate_native(ids, max_new_tokens=2, do_sample=True)


def test_row_keys_and_seed_draw():
    from gritlm_amd.decoder import draw_seed, row_keys
    k = row_keys(2 ** 64 - 2, 4, "cpu")
    assert k.dtype == torch.int64 and [int(x) % 2 ** 64 for x in k] == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]
    torch.manual_seed(7)
    a = draw_seed()
    torch.manual_seed(7)
    assert draw_seed() == a and 0 <= a < 2 ** 64


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sampling_kernels_do_not_spill():
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(ROOT, "gritlm_amd", "csrc", "sample.hip"),
                        "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    ks, cur = [], None
    for line in r.stderr.splitlines():
        mt = re.search(r"remark:\s+(.*?)(?: \[-Rpass|$)", line)
        if not mt:
            continue
        t = mt.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            ks.append(cur)
        elif cur is not None and ":" in t:
            a, b = t.split(":", 1)
            cur[a.strip()] = b.strip()
    ks = [k for k in ks if "sample_advance_k" in k["name"]]
    assert len(ks) == 2, [k["name"] for k in ks]
    for k in ks:
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["Occupancy [waves/SIMD]"]) >= 4, k                 # one 1024-thread workgroup per CU
