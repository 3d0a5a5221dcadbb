#!/usr/bin/env python3
"""Bit-level record of the attention backward (csrc/attention_bwd.hip): a fixed seeded table of calls through gritlm_amd.ops, one line per
case with the sha-256 of dq | dk | dv (the raw bytes of dqkv).  Two builds of the library compute the same thing iff their outputs of this
tool are identical:
    GRIT_HIP_LIB=<other build> python tools/attn_bwd_bits.py > a.txt;  python tools/attn_bwd_bits.py > b.txt;  diff a.txt b.txt
(one fresh process per library: GRIT_HIP_LIB is read at import).  The table reaches all six entry points and both sides of every dispatch
(padded / packed, bidirectional / causal / window) at the tile and block edges: sequence lengths around 64 and 128, ragged last blocks,
ragged and holed key masks, a mask whose last words are empty, GQA groups 1, 2 and 4, windows below a tile, across tiles and >= S."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gritlm_amd import ops  # noqa: E402

DEV, BF, D = "cuda", torch.bfloat16, 128
LENGTHS = (1, 63, 64, 65, 127, 128, 129, 200, 330)
HEADS = ((2, 2), (4, 2), (8, 2))                          # (nq, nkv): GQA groups 1, 2, 4
WINDOWS = (2, 16, 64, 100, 129, 1000)                     # the last one >= every S here
PACKED = (200, 71, 128, 1, 300, 513, 64, 40)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def operands(T: int, nq: int, nkv: int, seed: int):
    qkv = torch.randn((T, (nq + 2 * nkv) * D), generator=gen(seed)).to(BF).to(DEV)
    dout = torch.randn((T, nq * D), generator=gen(seed + 1)).to(BF).to(DEV)
    return qkv, dout


def emit(name: str, dqkv: torch.Tensor):
    print(name, hashlib.sha256(dqkv.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:32], flush=True)


def masks(S: int) -> torch.Tensor:
    """row 0: every key; row 1: ragged (right padding; at S = 330 the last three mask words are empty); row 2: holes"""
    m = torch.ones((3, S), dtype=torch.int64)
    m[1, max(1, (S * 2) // 5):] = 0
    m[2, 1::3] = 0
    m[2, S // 2: S // 2 + 9] = 0
    m[2, 0] = 1
    return m


def padded(S: int, nq: int, nkv: int, causal: bool, window: int):
    B = 3
    qkv, dout = operands(B * S, nq, nkv, 100 * S + nq)
    bits = ops.mask_pack(masks(S).to(DEV))
    lse = torch.empty((B, nq, S), dtype=torch.float32, device=DEV)
    out = ops.attn_bidir(qkv, bits, B, S, nq, nkv, D, lse=lse, causal=causal, window=window)
    dqkv = torch.zeros_like(qkv)
    ops.attn_bidir_bwd(qkv, bits, out, dout, lse, B, S, nq, nkv, D, dqkv=dqkv, causal=causal, window=window)
    emit(f"padded S={S} nq={nq} nkv={nkv} causal={int(causal)} window={window}", dqkv)


def packed(lens, nq: int, nkv: int, causal: bool, window: int):
    T = sum(lens)
    qkv, dout = operands(T, nq, nkv, 7 * T + nq + len(lens))
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32).to(DEV)
    lse = torch.empty((T, nq), dtype=torch.float32, device=DEV)
    out = ops.attn_bidir_varlen(qkv, cu, max(lens), nq, nkv, D, lse=lse, causal=causal, window=window)
    dqkv = torch.zeros_like(qkv)
    ops.attn_bidir_varlen_bwd(qkv, cu, max(lens), out, dout, lse, nq, nkv, D, dqkv=dqkv, causal=causal, window=window)
    emit(f"packed lens={','.join(map(str, lens))} nq={nq} nkv={nkv} causal={int(causal)} window={window}", dqkv)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "attn_bwd_bits.py needs a GPU"
    for nq, nkv in HEADS:
        for causal in (False, True):
            for S in LENGTHS:
                padded(S, nq, nkv, causal, 0)
                packed((S,), nq, nkv, causal, 0)
            packed(PACKED, nq, nkv, causal, 0)
    for window in WINDOWS:
        for S in (65, 129, 330):
            padded(S, 4, 2, True, window)
        packed(PACKED, 4, 2, True, window)
        packed(PACKED, 8, 2, True, window)
