#!/usr/bin/env python3
"""Bit-level record of the HBM-bound row kernels (csrc/elementwise.hip, pool.hip, moe.hip, backward.hip): a fixed seeded table of calls
through gritlm_amd.ops, one line per case with the sha-256 of every output's raw bytes (NaN payloads included) and the fp16 overflow
flag, read and cleared.  Two builds of the library compute the same thing iff their outputs of this tool are identical:
    GRIT_HIP_LIB=<other build> python tools/row_kernels_ab.py > a.txt;  python tools/row_kernels_ab.py > b.txt;  diff a.txt b.txt
(one fresh process per library: GRIT_HIP_LIB is read at import).  The table reaches every instantiation and both sides of every
dispatch of the RMSNorm forward, the embedding gathers, pooling forward / backward in both layouts and both routers."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gritlm_amd import ops  # noqa: E402

DEV = "cuda"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(INT_VIEW[t.element_size()]).cpu().numpy().tobytes()).hexdigest()[:32]


def emit(name: str, *outs: torch.Tensor):
    flag = int(ops.f16_overflow_flag(torch.cuda.current_device(), clear=True))
    print(name, " ".join(sha(o) for o in outs), f"flag={flag}", flush=True)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def rmsnorm_cases():
    pairs = (("bf16_bf16", BF, BF), ("f32_bf16", F32, BF), ("f32_f16", F32, F16), ("f16_f16", F16, F16), ("f16_bf16", F16, BF))
    for H in (264, 512, 768, 1024, 2048, 4096, 8192, 8200, 16384):
        w = 1 + 0.1 * torch.randn((H,), generator=gen(H))
        w[5] = 2048.0                                          # a spike row times this weight leaves the fp16 range
        w = w.to(BF).to(DEV)
        for T in (1, 3, 16, 17, 37, 1031):
            x = torch.randn((T, H), generator=gen(1000 * H + T)) * 2.0
            if T >= 3:
                x[0] *= 1e-3; x[0, 5] = 3.0e4                  # overflows an fp16 output
                x[1, 7] = float("nan")
                x[2, 9] = float("inf"); x[2, 11] = float("-inf")
            for tag, din, dout in pairs:
                y = torch.empty((T, H), dtype=dout, device=DEV)
                ops.rmsnorm(x.to(din).to(DEV), w, 1e-5, out=y)
                emit(f"rmsnorm {tag} T={T} H={H}", y)


def embed_cases():
    V, H, T = 97, 4096, 300
    tab = torch.randn((V, H), generator=gen(7))
    ids = torch.randint(0, V, (T,), generator=gen(8))
    ids[3], ids[4], ids[5], ids[6] = -1, -2 ** 40, V, V + 12345
    ids = ids.to(DEV)
    for tag, dt, do in (("bf16", BF, BF), ("bf16_to_f32", BF, F32), ("f16", F16, F16)):
        out = torch.empty((T, H), dtype=do, device=DEV)
        ops.embed_gather(tab.to(dt).to(DEV), ids, out=out)
        emit(f"embed_gather {tag} T={T} H={H}", out)


MODES = ("mean", "weightedmean", "cls", "lasttoken")


def pool_cases():
    B = 5
    for H in (256, 4096):
        for S in (1, 7, 70, 512, 1031):
            hid = torch.randn((B, S, H), generator=gen(10 * S + H)).to(BF).to(DEV)
            dy = torch.randn((B, H), generator=gen(10 * S + H + 1)).to(DEV)
            mask = torch.ones((B, S), dtype=torch.int64)
            mask[1, (S + 1) // 2:] = 0                          # ragged right padding
            mask[2] = 0                                        # all-zero row: denominator 0
            mask[3, : S // 3] = 0                              # left-padded
            mask[4] = torch.randint(0, 4, (S,), generator=gen(S))   # non-binary
            mask = mask.to(DEV)
            instr_t = torch.tensor([0, 1, 2, S // 2, S + 3], dtype=torch.int32).to(DEV)     # the last one >= the row length
            for mode in MODES:
                for norm in (True, False):
                    for instr in (None, instr_t):
                        inv = torch.empty((B,), dtype=F32, device=DEV)
                        y = ops.pool_norm(hid, mask, mode, norm, instr, inv_norm=inv)
                        dh = ops.pool_norm_bwd(y, dy, inv, mask, mode, norm, S, instr)
                        emit(f"pool padded {mode} norm={int(norm)} instr={int(instr is not None)} S={S} H={H}", y, inv, dh)
        for lens in ((40, 25, 33, 1), (200, 71, 128, 1, 300)):
            T, n = sum(lens), len(lens)
            hid = torch.randn((T, H), generator=gen(T + H)).to(BF).to(DEV)
            dy = torch.randn((n, H), generator=gen(T + H + 1)).to(DEV)
            cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32).to(DEV)
            instr_t = torch.tensor([3, 0, 40, 1, 17][:n], dtype=torch.int32).to(DEV)        # 40 >= the third document's 33 rows
            for mode in MODES:
                for norm in (True, False):
                    for instr in (None, instr_t):
                        inv = torch.empty((n,), dtype=F32, device=DEV)
                        y = ops.pool_norm_varlen(hid, cu, mode, norm, instr, inv_norm=inv)
                        dh = ops.pool_norm_varlen_bwd(y, dy, inv, cu, T, mode, norm, instr)
                        emit(f"pool packed {mode} norm={int(norm)} instr={int(instr is not None)} lens={lens} H={H}", y, inv, dh)


def router_cases():
    for E in (4, 8, 16):
        for H in (256, 4096):
            gw = (torch.randn((E, H), generator=gen(E + H)) * 0.5).to(BF).to(DEV)
            ln = (1 + 0.1 * torch.randn((H,), generator=gen(E + H + 1))).to(BF).to(DEV)
            for T in (1, 130, 777):
                x = torch.randn((T, H), generator=gen(E * H + T))
                emit(f"router bf16 E={E} H={H} T={T}", *ops.moe_route(x.to(BF).to(DEV), gw))
                emit(f"router f32 E={E} H={H} T={T}", *ops.moe_route_f32(x.to(DEV), ln, 1e-5, gw))
    # constructed rows (what check_moe_router_edges builds): one-hot gate rows so that logit e = x[:, e], column E shared by every expert
    E, H = 8, 256
    gate = torch.zeros((E, H)); gate[torch.arange(E), torch.arange(E)] = 1.0; gate[:, E] = 1.0
    rows = []
    for hot in ((0, 1), (0, E - 1), (E - 2, E - 1), (1, 2, 3), tuple(range(E))):              # exact ties, all-equal
        r = -torch.arange(E, dtype=F32) - 2.0; r[list(hot)] = 3.0; rows.append(r)
    X = torch.zeros((len(rows) + 4, H)); X[: len(rows), :E] = torch.stack(rows)
    X[-4, E - 1] = 120.0                                       # softmax underflow: the 2nd pick is decided by index
    X[-3, 2] = float("inf"); X[-2, E - 1] = float("nan"); X[-1, E] = float("-inf")          # +inf, NaN, every logit -inf
    ones = torch.ones((H,)).to(BF).to(DEV)
    emit("router bf16 edges", *ops.moe_route(X.to(BF).to(DEV), gate.to(BF).to(DEV)))
    emit("router f32 edges", *ops.moe_route_f32(X.to(DEV), ones, 1e-5, (gate * 16.0).to(BF).to(DEV)))
    emit("router f32 finite rows only", *ops.moe_route_f32(X[:-3].to(DEV), ones, 1e-5, (gate * 16.0).to(BF).to(DEV)))


def unchanged_cases():
    """kernels that only lost a launch helper: one line each"""
    T, H, E = 50, 4096, 8
    x = torch.randn((T, H), generator=gen(1)).to(BF).to(DEV)
    dy = torch.randn((T, H), generator=gen(2)).to(BF).to(DEV)
    w = (1 + 0.1 * torch.randn((H,), generator=gen(3))).to(BF).to(DEV)
    dw = torch.zeros((H,), dtype=F32, device=DEV)
    emit("rmsnorm_bwd T=50 H=4096", ops.rmsnorm_bwd(dy, x, w, 1e-5, dw, dres=x), dw)
    gu = torch.randn((T, 2 * 1024), generator=gen(4)).to(BF).to(DEV)
    act = ops.swiglu(gu)
    emit("swiglu fwd+bwd T=50 I=1024", act, ops.swiglu_bwd(gu, torch.randn((T, 1024), generator=gen(5)).to(BF).to(DEV)))
    gw = (torch.randn((E, H), generator=gen(6)) * 0.5).to(BF).to(DEV)
    experts, _, _, _, _ = ops.moe_route(x, gw)
    gg = torch.zeros((E, H), dtype=BF, device=DEV)
    dx, dl = ops.moe_router_bwd(x, gw, experts, torch.randn((T, 2), generator=gen(7)).to(DEV), dy, gg, return_dlogits=True)
    emit("moe_router_bwd T=50 H=4096 E=8", dx, dl, gg)
    emit("transpose 300x264", ops.transpose(torch.randn((300, 264), generator=gen(8)).to(BF).to(DEV)).contiguous())


if __name__ == "__main__":
    assert torch.cuda.is_available(), "row_kernels_ab.py needs a GPU"
    ops.f16_overflow_flag(torch.cuda.current_device(), clear=True)
    for cases in (rmsnorm_cases, embed_cases, pool_cases, router_cases, unchanged_cases):
        cases()
