#!/usr/bin/env python3
"""Bit-level record of the token-by-token decode kernels (csrc/decode.hip, decode_gemm.hip, sample.hip): a fixed seeded table of calls
through gritlm_amd.ops, one line per case with the sha-256 of every output's raw bytes (NaN payloads included) and the fp16 overflow
flag, read and cleared.  Two builds of the library compute the same thing iff their outputs of this tool are identical:
    GRIT_HIP_LIB=<other build> python tools/decode_kernels_ab.py > a.txt;  python tools/decode_kernels_ab.py > b.txt;  diff a.txt b.txt
(one fresh process per library: GRIT_HIP_LIB is read at import).  The shapes are the smallest at which these kernels take another path:
every rows-per-launch instantiation of the GEMV and fewer rows than it holds, K with idle lanes / one / one and a one-lane tail / two
iterations, N off the rows per workgroup; one chunk, one chunk per wave and a lone last chunk in the row GEMM's K split, both of its
launch forms; MHA and groups of 3, 4 and 8 heads in the attention, empty splits and more splits than the combine holds in registers."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gritlm_amd import ops  # noqa: E402
from gritlm_amd.ops import EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU  # noqa: E402

DEV = "cuda"
BF, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
EPS = 1e-5


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(INT_VIEW[t.element_size()]).cpu().numpy().tobytes()).hexdigest()[:32]


def emit(name: str, *outs: torch.Tensor):
    flag = int(ops.f16_overflow_flag(torch.cuda.current_device(), clear=True))
    print(name, " ".join(sha(o) for o in outs), f"flag={flag}", flush=True)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed)) * scale


_cache = {}


def weights(N, K, dt):
    """[N, K] in the operand format, from one seeded fp32 matrix per shape"""
    if (N, K) not in _cache:
        _cache[(N, K)] = randn((N, K), 7 * N + K, K ** -0.5)
    return _cache[(N, K)].to(dt).to(DEV)


def ln_weight(K):
    return (1 + 0.1 * randn((K,), K + 1)).to(BF).to(DEV)


def projection_cases(tag, proj, proj_norm, rows, Ks, shapes, exact):
    """STORE / RESIDUAL / SWIGLU x the norm forms x both operand formats; proj(x, w, epilogue=, residual=, out16=), proj_norm(x, ln, w, epilogue, form)"""
    for dt, fmt in ((BF, "bf16"), (F16, "f16")):
        rdt = F32 if dt == F16 else BF                        # the stream's format: what RESIDUAL reads and writes
        for K in Ks:
            ln = ln_weight(K)
            for B in rows:
                x = randn((B, K), 100 * K + B).to(dt).to(DEV)
                for epi, name, N in shapes:
                    w = weights(N, K, dt)
                    case = f"{tag} {fmt} {name} B={B} N={N} K={K}"
                    if epi == EPI_RESIDUAL:
                        res = randn((B, N), N + B).to(rdt).to(DEV)
                        emit(case, proj(x, w, epilogue=epi, residual=res))
                        if dt == F16:
                            o16 = torch.zeros((B, N), dtype=F16, device=DEV)
                            emit(case + " out16", proj(x, w, epilogue=epi, residual=res, out16=o16), o16)
                        continue
                    emit(case, proj(x, w, epilogue=epi))
                    emit(case + " deferred norm", proj_norm(x, ln, w, epi, True))
                    if exact and dt == BF:
                        emit(case + " exact norm", proj_norm(x, ln, w, epi, False))


def projection_edges(tag, proj, proj_norm, B, K, N):
    """an fp16 row whose output leaves the fp16 range (flag = 1) and a row with a NaN"""
    for dt, fmt in ((BF, "bf16"), (F16, "f16")):
        rdt = F32 if dt == F16 else BF
        x = randn((B, K), 5).to(dt)
        x[B - 1] = 16000.0                                    # 16000 * sqrt(K) * E|w_hat| >> 65504 in the RESIDUAL copy and the SWIGLU activation
        big = x.to(DEV)
        x = randn((B, K), 6).to(dt)
        x[0, 3] = float("nan")
        nan = x.to(DEV)
        w = weights(N, K, dt).abs()
        res = randn((B, N), 8).to(rdt).to(DEV)
        for what, xx in (("overflow row", big), ("NaN row", nan)):
            o16 = torch.zeros((B, N), dtype=F16, device=DEV) if dt == F16 else None
            outs = [proj(xx, w, epilogue=EPI_RESIDUAL, residual=res, out16=o16)] + ([o16] if dt == F16 else [])
            emit(f"{tag} {fmt} RESIDUAL {what} B={B} N={N} K={K}", *outs)
            emit(f"{tag} {fmt} SWIGLU {what} B={B} N={N} K={K}", proj(xx, w, epilogue=EPI_SWIGLU))
            emit(f"{tag} {fmt} SWIGLU deferred norm {what} B={B} N={N} K={K}", proj_norm(xx, ln_weight(K), w, EPI_SWIGLU, True))


def gemv_cases():
    norm = lambda x, ln, w, epi, deferred: ops.rmsnorm_gemv(x, ln, EPS, w, epilogue=epi, deferred=deferred)
    shapes = [(EPI_STORE, "STORE", 64), (EPI_STORE, "STORE", 1030), (EPI_RESIDUAL, "RESIDUAL", 64), (EPI_RESIDUAL, "RESIDUAL", 1030),
              (EPI_SWIGLU, "SWIGLU", 96), (EPI_SWIGLU, "SWIGLU", 1024)]
    projection_cases("gemv", ops.gemv, norm, (1, 2, 3, 4, 5, 8), (256, 2048, 2056, 4096), shapes, exact=True)
    projection_edges("gemv", ops.gemv, norm, 3, 2048, 64)
    E, N, K, B = 5, 64, 256, 2                                # the expert stack: the kernel clamps the device index to [0, E)
    for dt, fmt in ((BF, "bf16"), (F16, "f16")):
        stack = randn((E, N, K), 11, K ** -0.5).to(dt).to(DEV)
        x = randn((B, K), 12).to(dt).to(DEV)
        for idx in (0, 4, -3, 9):
            e = torch.tensor([idx], dtype=I32, device=DEV)
            emit(f"gemv_expert {fmt} E={E} index={idx}", ops.gemv_expert(x, stack, e), ops.gemv_expert(x, stack, e, epilogue=EPI_SWIGLU))


def decode_gemm_cases():
    norm = lambda x, ln, w, epi, deferred: ops.rmsnorm_decode_gemm(x, ln, EPS, w, epilogue=epi)
    shapes = [(EPI_STORE, "STORE", 64), (EPI_STORE, "STORE", 16384), (EPI_RESIDUAL, "RESIDUAL", 64), (EPI_SWIGLU, "SWIGLU", 64)]
    projection_cases("decode_gemm", ops.decode_gemm, norm, (9, 16, 17, 64), (64, 512, 1088), shapes, exact=False)
    projection_edges("decode_gemm", ops.decode_gemm, norm, 17, 512, 64)


def rope_tables(Lmax, d):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
    ang = torch.arange(Lmax, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(F32).to(DEV), ang.sin().to(F32).to(DEV)


def attn_decode_cases():
    d = 128
    # (Lmax, lens of the sequences, rows form: (sequence, position) of every row -- two rows are consecutive tokens of sequence 0)
    shapes = ((256, (0, 63, 64, 255), ((0, 62), (0, 63), (1, 0), (2, 64), (3, 255))), (8192, (8000,), ((0, 7999), (0, 8000))))
    for nq, nkv in ((4, 4), (8, 2), (6, 2), (16, 2)):
        for Lmax, lens_l, rows in shapes:
            B = len(lens_l)
            cos, sin = rope_tables(Lmax, d)
            seed = 1000 * nq + Lmax
            k32, v32 = randn((B, nkv, Lmax, d), seed), randn((B, nkv, Lmax, d), seed + 1)
            qkv32 = randn((B, (nq + 2 * nkv) * d), seed + 2)
            lens = torch.tensor(lens_l, dtype=I32, device=DEV)
            ws = ops.attn_decode_workspace(B, nq, nkv, Lmax, DEV)
            for cdt, fmt in ((BF, "bf16"), (F16, "f16")):
                qdt = F32 if cdt == F16 else BF               # fp16 caches: the q (q|k|v) row is fp32
                case = f"{fmt} nq={nq} nkv={nkv} Lmax={Lmax} lens={lens_l}"
                ck, cv = k32.to(cdt).to(DEV), v32.to(cdt).to(DEV)
                ctx = torch.zeros((B, nq * d), dtype=cdt, device=DEV)
                if cdt == BF:
                    emit("attn_decode " + case, ops.attn_decode(qkv32.to(BF).to(DEV), ck, cv, lens, ctx, ws, nq, nkv, d))
                ctx = torch.zeros((B, nq * d), dtype=cdt, device=DEV)
                ops.attn_decode_rope(qkv32.to(qdt).to(DEV), cos, sin, ck, cv, lens, ctx, ws, nq, nkv, d)
                emit("attn_decode_rope " + case, ctx, ck, cv)
                V = len(rows)
                crow = torch.tensor([r[0] for r in rows], dtype=I32, device=DEV)
                rlens = torch.tensor([r[1] for r in rows], dtype=I32, device=DEV)
                rq = randn((V, (nq + 2 * nkv) * d), seed + 3).to(qdt).to(DEV)
                ck, cv = k32.to(cdt).to(DEV), v32.to(cdt).to(DEV)
                ops.rope_kv_append_rows(rq, cos, sin, ck, cv, rlens, crow, nq, nkv, d)
                ctx = torch.zeros((V, nq * d), dtype=cdt, device=DEV)
                ops.attn_decode_rows(rq, ck, cv, rlens, crow, ctx, ops.attn_decode_workspace(V, nq, nkv, Lmax, DEV), nq, nkv, d)
                emit(f"attn_decode_rows {fmt} nq={nq} nkv={nkv} Lmax={Lmax} rows={rows}", ctx, ck, cv)


def logits_rows(V, seed):
    """random rows; a tie between columns that fall to different waves; a row of -inf; a row with NaNs, one in the maximum's place"""
    x = randn((5, V), seed, 4.0).to(BF).to(F32)               # (bf16-exact values: both formats see the same numbers)
    x[1, 100] = x[1, 700] = 64.0
    x[2] = float("-inf")
    x[3, int(x[3].argmax())] = float("nan"); x[3, 5] = float("nan"); x[3, V - 1] = float("nan")
    x[4, V - 1] = 80.0                                        # the maximum in the last chunk (partial where V % 8 != 0)
    return x


def padded(x, dt):
    """[B, V] rows inside a buffer whose leading dimension is a multiple of 8"""
    B, V = x.shape
    buf = torch.zeros((B, (V + 7) // 8 * 8), dtype=dt, device=DEV)
    buf[:, :V] = x.to(dt).to(DEV)
    return buf[:, :V]


def token_state(B, with_state):
    nxt = torch.full((B,), -1, dtype=I64, device=DEV)
    if not with_state:
        return nxt, None, None, None
    lens = torch.arange(10, 10 + B, dtype=I32, device=DEV)
    return nxt, lens, torch.full((B, 8), -1, dtype=I64, device=DEV), torch.tensor([3], dtype=I32, device=DEV)


def argmax_cases():
    for V in (1001, 32003):
        x = logits_rows(V, V)
        for dt, fmt in ((BF, "bf16"), (F32, "f32")):
            for with_state in (True, False):
                nxt, lens, hist, step = token_state(x.shape[0], with_state)
                ops.argmax_advance(padded(x, dt), nxt, lens, hist, step)
                emit(f"argmax {fmt} V={V} state={int(with_state)}", *[t for t in (nxt, hist, lens, step) if t is not None])


def sample_cases():
    for V in (1001, 40000):                                   # 40000: beyond the 32768 columns staged in LDS
        x = logits_rows(V, V + 1)
        keys = torch.tensor([11, 2 ** 40 + 7, -5, 123456789, 2 ** 62], dtype=I64, device=DEV)
        for dt, fmt in ((BF, "bf16"), (F32, "f32")):
            for T, top_k, top_p in ((1.0, 0, 1.0), (0.2, 50, 1.0), (0.7, 0, 0.9), (1.0, 1, 1.0)):
                nxt, lens, hist, step = token_state(x.shape[0], True)
                ops.sample_advance(padded(x, dt), nxt, keys, T, top_k, top_p, lens, hist, step)
                emit(f"sample {fmt} V={V} T={T} top_k={top_k} top_p={top_p}", nxt, hist, lens, step)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "decode_kernels_ab.py needs a GPU"
    ops.f16_overflow_flag(torch.cuda.current_device(), clear=True)
    for cases in (gemv_cases, decode_gemm_cases, attn_decode_cases, argmax_cases, sample_cases):
        cases()
