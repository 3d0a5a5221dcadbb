"""Batched greedy decode (9..64 rows) on the MFMA decode GEMMs (csrc/decode_gemm.hip): the kernels against fp64 at the 7B projection
shapes (every epilogue, both operand formats, strided operands, NaN sentinels that must survive), batch invariance and reproducibility bit for
bit, the fp16 overflow flag; the decoder against the fp32 oracle at 16 and 64 rows with per-row cached lengths, without a cache on ragged
prompts, GritLM.generate_native on 32 prompts, graph replay against eager launches, the fp16 overflow fallback, the untouched 1..8-row path
and the limits."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU = 0, 1, 2
SHAPES = {"qkv": (6144, 4096), "o_proj": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336), "lm_head": (32000, 4096),
          "wide_residual": (32000, 4096)}       # (RESIDUAL at N >= 16384: the 16-row launch form as well)


def _omc(a, b):
    """max over rows of 1 - cos(a_row, b_row), fp64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(1.0 - np.sum(a * b, axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))))


def _swiglu_ref(y):
    """the interleaved gate/up layout (blocks of 16 rows): y [B, N] fp64 -> silu(g) * u [B, N/2]"""
    B, N = y.shape
    blk = y.reshape(B, N // 32, 2, 16)
    g, u = blk[:, :, 0].reshape(B, N // 2), blk[:, :, 1].reshape(B, N // 2)
    return g / (1.0 + np.exp(-g)) * u


def _operands(N, K, dt, seed, rows=64, wscale=0.02):
    """W [N, K] and x [rows, K] in a buffer of leading dimension K + 64 whose padding columns are NaN (never read)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = (torch.randn((N, K), generator=g, device=DEV) * wscale).to(dt)
    xb = torch.full((rows, K + 64), float("nan"), device=DEV).to(dt)
    xb[:, :K] = torch.randn((rows, K), generator=g, device=DEV).to(dt)
    return w, xb[:, :K], g


def _run(kind, dt, B, x, w, deferred, g):
    """one launch with NaN sentinels in rows >= B and columns n_out .. ldo-1; returns (got fp64 [B, n_out], ref fp64, tolerance)"""
    from gritlm_amd import ops
    N, K = w.shape
    epi = {"o_proj": EPI_RESIDUAL, "down": EPI_RESIDUAL, "wide_residual": EPI_RESIDUAL, "gate_up": EPI_SWIGLU}.get(kind, EPI_STORE)
    n_out = N // 2 if epi == EPI_SWIGLU else N
    f16 = dt == F16
    odt = (F16 if epi == EPI_SWIGLU else F32) if f16 else BF16
    outb = torch.full((64, n_out + 16), float("nan"), device=DEV).to(odt)
    out = outb[:, :n_out]
    xs = x[:B]
    X = xs.double()
    ln = None
    if deferred:
        ln = (1.0 + 0.2 * torch.randn((K,), generator=g, device=DEV)).to(BF16)
        X = X * ln.double() * torch.rsqrt(X.pow(2).mean(dim=1, keepdim=True) + 1e-5)
    Y = (X @ w.double().T)
    res = res16 = None
    if epi == EPI_RESIDUAL:
        resb = torch.full((64, N + 8), float("nan"), device=DEV).to(F32 if f16 else BF16)
        resb[:B, :N] = torch.randn((B, N), generator=g, device=DEV).to(resb.dtype)
        res = resb[:, :N]
        if f16:
            res16 = torch.full((64, N + 24), float("nan"), device=DEV).to(F16)
        ref = Y + res[:B].double()
        out = res                                                   # in place, as the decoder calls it
    elif epi == EPI_SWIGLU:
        ref = _swiglu_ref(Y.cpu().numpy())
    else:
        ref = Y
    ref = np.asarray(ref.cpu() if torch.is_tensor(ref) else ref, np.float64)
    if deferred:
        ops.rmsnorm_decode_gemm(xs, ln, 1e-5, w, out=out[:B], epilogue=epi)
    else:
        ops.decode_gemm(xs, w, out=out[:B], epilogue=epi, residual=None if res is None else res[:B],
                        out16=None if res16 is None else res16[:B, :N])
    torch.cuda.synchronize()
    base = res if epi == EPI_RESIDUAL else outb
    assert torch.isnan(base[B:].float()).all(), "rows >= B were written"
    if epi != EPI_RESIDUAL:
        assert torch.isnan(outb[:, n_out:].float()).all(), "columns >= N were written"
    else:
        assert torch.isnan(resb[:, N:].float()).all(), "columns >= N were written"
        if res16 is not None:
            assert torch.isnan(res16[:, N:].float()).all() and torch.isnan(res16[B:].float()).all()
            assert torch.equal(res16[:B, :N], res[:B].to(F16)), "out16 is the fp16 rounding of the fp32 output"
    got = out[:B].double().cpu().numpy()
    scale = float(np.max(np.abs(ref)))
    # output rounding: bf16 2^-8, fp16 2^-11 relative; deferred forms also round x * ln_w once to the operand format
    tol = (1.2e-2 if not f16 else 2e-3) if (odt != F32 or deferred) else 2e-4
    return got, ref, tol * scale


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_decode_gemm_vs_fp64(kind, dtype):
    dt = BF16 if dtype == "bf16" else F16
    N, K = SHAPES[kind]
    w, x, g = _operands(N, K, dt, seed=11 + len(kind))
    for B in (1, 9, 16, 33, 64):
        for deferred in ((False, True) if kind in ("qkv", "gate_up", "lm_head") else (False,)):
            got, ref, tol = _run(kind, dt, B, x, w, deferred, g)
            assert np.isfinite(got).all(), (kind, B, deferred)
            err = float(np.max(np.abs(got - ref)))
            assert err < tol, (kind, dtype, B, deferred, err, tol)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_decode_gemm_batch_invariant_and_reproducible(dtype):
    """64 rows, then subsets of 9 and 16 rows in a permuted order: every row's output is the same bits; two identical launches too"""
    from gritlm_amd import ops
    dt = BF16 if dtype == "bf16" else F16
    for kind in ("qkv", "gate_up", "down", "lm_head"):
        N, K = SHAPES[kind]
        w, x, g = _operands(N, K, dt, seed=5)
        x = x.contiguous()
        ln = (1.0 + 0.2 * torch.randn((K,), generator=g, device=DEV)).to(BF16)
        if kind == "down":
            res = torch.randn((64, N), generator=g, device=DEV).to(F32 if dt == F16 else dt)
            f = lambda rows: ops.decode_gemm(x[rows], w, epilogue=EPI_RESIDUAL, residual=res[rows].contiguous(),
                                             out16=torch.empty((len(rows), N), dtype=F16, device=DEV) if dt == F16 else None)
        elif kind == "gate_up":
            f = lambda rows: ops.rmsnorm_decode_gemm(x[rows], ln, 1e-5, w, epilogue=EPI_SWIGLU)
        elif kind == "lm_head":
            f = lambda rows: ops.rmsnorm_decode_gemm(x[rows], ln, 1e-5, w)
        else:
            f = lambda rows: ops.decode_gemm(x[rows], w)
        all_rows = torch.arange(64, device=DEV)
        full = f(all_rows)
        assert torch.equal(full.view(torch.int16) if full.element_size() == 2 else full.view(torch.int32),
                           (lambda o: o.view(torch.int16) if o.element_size() == 2 else o.view(torch.int32))(f(all_rows))), kind
        perm = torch.randperm(64, generator=torch.Generator().manual_seed(3)).to(DEV)
        for n in (9, 16):
            rows = perm[:n]
            part = f(rows)
            a = full[rows]
            assert torch.equal(a.view(torch.int16) if a.element_size() == 2 else a.view(torch.int32),
                               part.view(torch.int16) if part.element_size() == 2 else part.view(torch.int32)), (kind, n)


def test_decode_gemm_f16_overflow_flag():
    from gritlm_amd import ops
    N, K = 1024, 512
    g = torch.Generator(device=DEV).manual_seed(9)
    w = (torch.randn((N, K), generator=g, device=DEV) * 0.05).to(F16)
    x = torch.randn((16, K), generator=g, device=DEV).to(F16)
    ln = torch.ones((K,), dtype=BF16, device=DEV)
    ops.f16_overflow_flag(DEV, clear=True)
    ops.decode_gemm(x, w, epilogue=EPI_SWIGLU)
    ops.rmsnorm_decode_gemm(x, ln, 1e-5, w, epilogue=EPI_SWIGLU)
    res = torch.randn((16, N), generator=g, device=DEV)
    ops.decode_gemm(x, w, out=res, epilogue=EPI_RESIDUAL, residual=res, out16=torch.empty((16, N), dtype=F16, device=DEV))
    assert not ops.f16_overflow_flag(DEV, clear=True), "in-range values must leave the flag clear"
    ops.decode_gemm(x, (w.float() * 400).to(F16), epilogue=EPI_SWIGLU)                   # silu(g) u beyond 65504
    assert ops.f16_overflow_flag(DEV, clear=True)
    res[3, 7] = 7e4                                                                        # the fp16 copy of the stream overflows
    ops.decode_gemm(x, w, out=res, epilogue=EPI_RESIDUAL, residual=res, out16=torch.empty((16, N), dtype=F16, device=DEV))
    assert ops.f16_overflow_flag(DEV, clear=True)
    # the deferred form's own rounding: x * ln_w to the fp16 MFMA operand (a STORE writes fp32, which is not range-checked)
    big_ln = torch.full((K,), 300.0, dtype=BF16, device=DEV)
    xs = torch.full((16, K), 1.0, dtype=F16, device=DEV)
    ops.rmsnorm_decode_gemm(xs, big_ln, 1e-5, w)
    assert not ops.f16_overflow_flag(DEV, clear=True), "300 fits fp16"
    xs[5, 100] = 300.0                                                                     # 300 * 300 = 9e4 > 65504
    ops.rmsnorm_decode_gemm(xs, big_ln, 1e-5, w)
    assert ops.f16_overflow_flag(DEV, clear=True)


# ------------------------------------------------------------------------------------------------------------------- the decoder
def _setup(cfg_name, seed=6, lm_seed=131):
    import gritlm_oracle as O
    from gpu_checks import build_engine
    from gritlm_amd.decoder import MistralDecoder
    eng, cfg, w = build_engine(cfg_name, seed)
    rng = np.random.default_rng(lm_seed)
    lm = O.bf16_round((rng.standard_normal((cfg["vocab_size"], cfg["hidden_size"])) * 0.05).astype(np.float32))
    return eng, cfg, w, lm, MistralDecoder(eng, torch.from_numpy(lm)), rng


@pytest.mark.parametrize("policy", ["bf16", "f16_operands", "f16_stream"])
@pytest.mark.parametrize("cfg_name,B", [("gqa", 16), ("gqa", 64), ("7b-l2s", 16), ("7b-l2s", 64)])
def test_batched_decoder_vs_oracle(cfg_name, B, policy):
    """per-row cached lengths; teacher-forced logits of every generated position against the fp32 oracle (every row on gqa; on the 7B
    layer shape the oracle is slow, so four rows spread over the batch)"""
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup(cfg_name)
    eng.set_precision(policy)
    S0, P, new = 48, 3, 5
    doc = rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)
    plens = (S0 - (np.arange(B) * 7) % 29).astype(np.int32)
    dmask = (np.arange(S0)[None] < plens[:, None]).astype(np.int64)
    _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.from_numpy(dmask).to(DEV), return_kv=True, kv_dtype=None)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)).to(DEV)
    toks, lg = dec.generate(prompt, new, past_key_values=kv, past_lens=torch.from_numpy(plens).to(DEV), return_logits=True)
    assert dec.last_precision == ("bf16" if policy == "bf16" else "f16")
    bound = 2e-4 if policy == "bf16" else 1e-5
    rows = range(B) if cfg_name == "gqa" else sorted({0, 9, B // 2 + 1, B - 1})
    for b in rows:
        _, kv_ref = O.mistral_encode(w, cfg, doc[b:b + 1], dmask[b:b + 1], return_layers="kv")
        seq = np.concatenate([prompt[b].cpu().numpy(), toks[b].cpu().numpy()])
        ref = O.mistral_continue(w, cfg, kv_ref, int(plens[b]), seq, lm)[P - 1:P - 1 + new].astype(np.float64)
        omc = _omc(lg[b].float().cpu().numpy(), ref)
        assert omc < bound, (b, omc)


def test_batched_decoder_no_cache_ragged_prompts():
    """B = 24 right-padded prompts of different lengths: the encoder's causal prefill, then decode at 24 rows; teacher-forced logits
    against the oracle's causal forward of each row's prompt + generated tokens"""
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    B, P, new = 24, 19, 6
    plen = 19 - (np.arange(B) * 5) % 17
    ids = rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)
    mask = (np.arange(P)[None] < plen[:, None]).astype(np.int64)
    toks, lg = dec.generate(torch.from_numpy(ids).to(DEV), new, attention_mask=torch.from_numpy(mask).to(DEV), return_logits=True)
    assert dec.last_prefill == "encoder"
    for b in range(B):
        seq = np.concatenate([ids[b, :plen[b]], toks[b].cpu().numpy()])
        hid = O.mistral_encode(w, cfg, seq[None], None, causal=True)[0]
        ref = (hid.astype(np.float64) @ lm.astype(np.float64).T)[plen[b] - 1:plen[b] - 1 + new]
        assert _omc(lg[b].float().cpu().numpy(), ref) < 2e-4, b


def test_generate_native_32_prompts():
    import synth
    from gritlm_amd import GritLM
    with tempfile.TemporaryDirectory() as td:
        d16 = synth.build_mistral_dir(os.path.join(td, "m16"), "tiny", 0, "bfloat16")
        m = GritLM(d16, pooling_method="mean", attn="bbcc", device="cuda", torch_dtype=torch.bfloat16, mode="unified")
        texts = [" ".join(synth.WORDS[(3 * i) % 40:(3 * i) % 40 + 4 + i % 9]) for i in range(32)]
        enc = m.tokenizer(texts, return_tensors="pt", padding=True, add_special_tokens=False)
        ids, mask = enc["input_ids"].to(DEV), enc["attention_mask"].to(DEV)
        assert bool((mask[:, 0] == 1).all()) and int(mask.sum(1).min()) < mask.shape[1]     # right-padded prompts of different lengths
        P, new = ids.shape[1], 8
        plain = m.generate_native(input_ids=ids, attention_mask=mask, max_new_tokens=new, min_new_tokens=new, pad_token_id=0)
        assert tuple(plain.shape) == (32, P + new) and torch.equal(plain[:, :P], ids)
        gen = plain[:, P:]
        eos = int(gen[0, 2])                                     # a token some rows emit: Hugging Face's padding after each row's EOS
        out = m.generate_native(input_ids=ids, attention_mask=mask, max_new_tokens=new, pad_token_id=0, eos_token_id=eos)
        assert out.shape[0] == 32 and torch.equal(out[:, :P], ids)
        got = out[:, P:]
        for b in range(32):
            hits = (gen[b] == eos).nonzero()
            stop = int(hits[0]) + 1 if len(hits) else new
            n = min(stop, got.shape[1])
            assert torch.equal(got[b, :n], gen[b, :n]), b
            assert bool((got[b, n:] == 0).all()), b


def test_graph_replay_matches_eager_at_64_rows():
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    B, S0, P, new = 64, 40, 2, 24
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)).to(DEV)
    for policy in ("bf16", "f16_operands"):
        eng.set_precision(policy)
        dec.use_graph = True
        t_graph = dec.generate(prompt, new, past_key_values=kv)
        dec.use_graph = False
        t_eager = dec.generate(prompt, new, past_key_values=kv)
        t_l1, l1 = dec.generate(prompt, new, past_key_values=kv, return_logits=True)
        t_l2, l2 = dec.generate(prompt, new, past_key_values=kv, return_logits=True)
        dec.use_graph = True
        assert torch.equal(t_graph, t_eager) and torch.equal(t_eager, t_l1), policy
        assert torch.equal(t_l1, t_l2) and torch.equal(l1, l2), policy


def test_batched_f16_overflow_falls_back_to_bf16():
    eng, cfg, w, lm, dec, rng = _setup("tiny")
    from gritlm_amd._lib import GritHipError
    B, S0, P, new = 16, 40, 5, 4
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)).to(DEV)
    eng.layers[0].wgu.mul_(400.0)
    eng.set_precision("f16_operands")
    with pytest.raises(GritHipError):
        dec.generate(prompt, new, past_key_values=kv, on_overflow="raise")
    t_fb = dec.generate(prompt, new, past_key_values=kv, on_overflow="bf16")
    assert dec.last_precision == "bf16 (f16 overflow)"
    eng.set_precision("bf16")
    t_bf = dec.generate(prompt, new, past_key_values=kv)
    assert dec.last_precision == "bf16" and torch.equal(t_fb, t_bf)


def test_no_decode_gemm_at_8_rows_or_fewer(monkeypatch):
    from gritlm_amd import ops
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(8, 30)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)

    def boom(*a, **k):
        raise AssertionError("decode_gemm launched at <= 8 rows")

    monkeypatch.setattr(ops, "decode_gemm", boom)
    monkeypatch.setattr(ops, "rmsnorm_decode_gemm", boom)
    for policy in ("bf16", "f16_operands"):
        eng.set_precision(policy)
        for B in (1, 3, 8):
            prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, 4)).astype(np.int64)).to(DEV)
            dec.generate(prompt, 3)
            dec.generate(prompt, 3, past_key_values=[(k[:B], v[:B]) for k, v in kv])
    for fn in ("qkv", "none", "deferred_mlp"):
        dec.fuse_norm = fn
        eng.set_precision("bf16")
        dec.generate(torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(8, 4)).astype(np.int64)).to(DEV), 3)


@pytest.mark.parametrize("fuse_norm", ["qkv", "deferred_mlp"])
def test_batched_exact_norm_forms_vs_oracle(fuse_norm):
    """above 8 rows the exact q|k|v norm is an RMSNorm launch followed by a STORE decode_gemm ("qkv": every norm; "deferred_mlp": the
    q|k|v one): teacher-forced logits against the fp32 oracle at 16 rows with per-row cached lengths"""
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    dec.fuse_norm = fuse_norm
    B, S0, P, new = 16, 40, 3, 5
    doc = rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)
    plens = (S0 - (np.arange(B) * 5) % 23).astype(np.int32)
    dmask = (np.arange(S0)[None] < plens[:, None]).astype(np.int64)
    _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.from_numpy(dmask).to(DEV), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)).to(DEV)
    toks, lg = dec.generate(prompt, new, past_key_values=kv, past_lens=torch.from_numpy(plens).to(DEV), return_logits=True)
    for b in range(B):
        _, kv_ref = O.mistral_encode(w, cfg, doc[b:b + 1], dmask[b:b + 1], return_layers="kv")
        seq = np.concatenate([prompt[b].cpu().numpy(), toks[b].cpu().numpy()])
        ref = O.mistral_continue(w, cfg, kv_ref, int(plens[b]), seq, lm)[P - 1:P - 1 + new].astype(np.float64)
        assert _omc(lg[b].float().cpu().numpy(), ref) < 2e-4, b


@pytest.mark.parametrize("fuse_norm", ["qkv", "none", "deferred_mlp"])
def test_batched_exact_norm_forms(fuse_norm):
    """the exact-norm forms above 8 rows: an RMSNorm launch, then a STORE decode_gemm; each row as it runs within another batch of 9..64"""
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    dec.fuse_norm = fuse_norm
    B, S0, P, new = 20, 30, 3, 5
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)).to(DEV)
    t20, l20 = dec.generate(prompt, new, past_key_values=kv, return_logits=True)
    t10, l10 = dec.generate(prompt[5:15], new, past_key_values=[(k[5:15], v[5:15]) for k, v in kv], return_logits=True)
    assert torch.equal(t20[5:15], t10) and torch.equal(l20[5:15], l10)


def test_limits_with_real_engines():
    from gpu_checks import build_engine
    from gritlm_amd.decoder import MistralDecoder
    eng, cfg, w, lm, dec, rng = _setup("tiny")
    with pytest.raises(NotImplementedError, match="64"):
        dec.generate(torch.zeros((65, 4), dtype=I64, device=DEV) + 3, 2)
    meng, mcfg, _ = build_engine("moe-tiny", 0)
    mdec = MistralDecoder(meng, torch.from_numpy(lm[:, :mcfg["hidden_size"]].copy()) if lm.shape[1] >= mcfg["hidden_size"] else
                          torch.zeros((mcfg["vocab_size"], mcfg["hidden_size"])))
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        mdec.generate(torch.zeros((9, 4), dtype=I64, device=DEV) + 3, 2)
