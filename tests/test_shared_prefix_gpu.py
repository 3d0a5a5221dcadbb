"""share_prefix: n sampled continuations over ONE copy of the prefix K/V (csrc/decode_prefix.hip, prefix_ops.py, MistralDecoder.generate).
The four launches against fp64 with NaN everywhere they must not read or write, row independence and reproducibility bit for bit, the
decoder against the fp32 oracle (cached documents with per-row lengths, and prompt-only ragged rows), tails across a 64-key split with
graph replay against eager launches, the memory the flag saves, the fallbacks, and GritLM.sample_native."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_sampling_cpu import hf_kept, kept  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
D = 128
TAILS = (0, 1, 63, 64, 70)          # tokens a row's tail holds before the new one
LTAIL = 128


def _omc(a, b):
    """max over rows of 1 - cos(a_row, b_row), fp64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(1.0 - np.sum(a * b, axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))))


def _setup(cfg_name, seed=6, lm_seed=131):
    import gritlm_oracle as O
    from gpu_checks import build_engine
    from gritlm_amd.decoder import MistralDecoder
    eng, cfg, w = build_engine(cfg_name, seed)
    rng = np.random.default_rng(lm_seed)
    lm = O.bf16_round((rng.standard_normal((cfg["vocab_size"], cfg["hidden_size"])) * 0.05).astype(np.float32))
    return eng, cfg, w, lm, MistralDecoder(eng, torch.from_numpy(lm)), rng


# ------------------------------------------------------------------------------------------------------------------ 1. the four launches
def _operands(dtype, nq, nkv, n, plen, seed):
    """B0 = len(plen) sequences x n rows.  q and K at 0.7, V at 1.0 (the scales of test_attn_prefill_cached_vs_fp64); every prefix slot
    >= plen[s], every tail slot from the row's new one on, the ctx buffer (two rows and 64 columns larger than the output) and the
    workspace are NaN."""
    from gritlm_amd import prefix_ops
    from gritlm_amd.encoder import rope_tables
    dt, qdt = (F16, F32) if dtype == "f16" else (BF16, BF16)
    B0, B, KC = len(plen), len(plen) * n, prefix_ops.kc()
    Lpre = 2 * KC + 64                                  # (a last chunk at or past every plen: the neutral element)
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda shape, s: torch.randn(shape, generator=g, device=DEV) * s
    width = (nq + 2 * nkv) * D
    qkv = torch.full((B, width + 64), float("nan"), device=DEV).to(qdt)
    qkv[:, :width] = rnd((B, width), 0.7).to(qdt)
    qkv[:, (nq + nkv) * D:width] = rnd((B, nkv * D), 1.0).to(qdt)
    pk, pv = rnd((B0, nkv, Lpre, D), 0.7).to(dt), rnd((B0, nkv, Lpre, D), 1.0).to(dt)
    tk, tv = rnd((B, nkv, LTAIL, D), 0.7).to(dt), rnd((B, nkv, LTAIL, D), 1.0).to(dt)
    tails = [TAILS[(3 * r + r // n) % len(TAILS)] for r in range(B)]
    for s in range(B0):
        pk[s, :, plen[s]:] = float("nan"); pv[s, :, plen[s]:] = float("nan")
    for r in range(B):
        tk[r, :, tails[r]:] = float("nan"); tv[r, :, tails[r]:] = float("nan")
    tplen = torch.tensor(plen, dtype=I32, device=DEV)
    lens = (tplen.repeat_interleave(n) + torch.tensor(tails, dtype=I32, device=DEV)).contiguous()
    cos, sin = rope_tables(Lpre + LTAIL, D, 10000.0, dtype != "f16", DEV)
    return dict(dt=dt, qdt=qdt, f16=dtype == "f16", n=n, nq=nq, nkv=nkv, B0=B0, B=B, Lpre=Lpre, qkv=qkv[:, :width], pk=pk, pv=pv, tk=tk, tv=tv,
                tails=tails, plen=plen, tplen=tplen, lens=lens, cos=cos, sin=sin)


def _launch(o):
    """launches 1 to 4 on clones of the operands; returns (ctx buffer, its output view, rotated qkv, q16, tails after the append)"""
    from gritlm_amd import prefix_ops
    n, nq, nkv, B = o["n"], o["nq"], o["nkv"], o["B"]
    qkvb = torch.full((B, o["qkv"].shape[1] + 64), float("nan"), device=DEV).to(o["qdt"])
    qkv = qkvb[:, :o["qkv"].shape[1]]
    qkv.copy_(o["qkv"])
    tk, tv = o["tk"].clone(), o["tv"].clone()
    q16 = torch.full((B, nq * D + 8), float("nan"), dtype=F16, device=DEV)[:, :nq * D] if o["f16"] else None
    ws = prefix_ops.workspace(B, nq, nkv, o["Lpre"], LTAIL, DEV)
    ws.fill_(float("nan"))
    buf = torch.full((B + 2, nq * D + 64), float("nan"), dtype=o["dt"], device=DEV)
    ctx = buf[:B, :nq * D]
    prefix_ops.rope_kv_append_tail(qkv, o["cos"], o["sin"], tk, tv, o["lens"], o["tplen"], n, nq, nkv, D, q16=q16)
    prefix_ops.attn_decode_prefix(q16 if o["f16"] else qkv, o["pk"], o["pv"], o["tplen"], ws, n, nq, nkv, D, LTAIL)
    prefix_ops.attn_decode_tail(qkv, tk, tv, o["lens"], o["tplen"], ws, n, nq, nkv, D, o["Lpre"])
    prefix_ops.attn_decode_prefix_combine(ws, ctx, nq, nkv, D, o["Lpre"], LTAIL)
    torch.cuda.synchronize()
    return buf, ctx, qkv, q16, tk, tv


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n", [9, 33, 64])
@pytest.mark.parametrize("case", ["1-64-kc+1", "63-65-2kc"])
@pytest.mark.parametrize("nq,nkv", [(32, 8), (4, 4), (4, 2)])
def test_prefix_kernels_vs_fp64(nq, nkv, case, n, dtype):
    """max |error| of ctx against the fp64 softmax over prefix[:plen[s]] || tail[:t_b + 1]: < 2e-2 bf16, < 2.5e-3 fp16 (the bounds of
    test_attn_prefill_cached_vs_fp64); the appended tail rows and the rotated q are the bits of grit_rope_kv_append_rows; no NaN comes
    through and nothing outside [B, nq 128] of ctx is written"""
    from gritlm_amd import ops, prefix_ops
    KC = prefix_ops.kc()
    plen = (1, 64, KC + 1) if case == "1-64-kc+1" else (63, 65, 2 * KC)
    o = _operands(dtype, nq, nkv, n, plen, seed=100 + nq + n)
    B, gq = o["B"], nq // nkv
    ops.f16_overflow_flag(DEV, clear=True)
    buf, ctx, qkv, q16, tk, tv = _launch(o)
    if o["f16"]:
        assert not ops.f16_overflow_flag(DEV, clear=True), "in-range values must leave the flag clear"
    # ---- the append, bit for bit: the existing kernel rotates the same rows at the same positions into a cache indexed by POSITION
    ref_qkv = o["qkv"].clone()
    rk = torch.zeros((B, nkv, o["Lpre"] + LTAIL, D), dtype=o["dt"], device=DEV)
    rv = torch.zeros_like(rk)
    ops.rope_kv_append_rows(ref_qkv, o["cos"], o["sin"], rk, rv, o["lens"], torch.arange(B, dtype=I32, device=DEV), nq, nkv, D)
    bits = lambda t: t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    assert torch.equal(bits(qkv[:, :nq * D]), bits(ref_qkv[:, :nq * D])), "q rotated in place"
    if o["f16"]:
        assert torch.equal(bits(q16), bits(ref_qkv[:, :nq * D].to(F16))), "q16 is the fp16 rounding of the rotated q"
    lens = o["lens"].tolist()
    for r in range(B):
        t = o["tails"][r]
        assert torch.equal(bits(tk[r, :, t]), bits(rk[r, :, lens[r]])) and torch.equal(bits(tv[r, :, t]), bits(rv[r, :, lens[r]])), r
        assert torch.equal(bits(tk[r, :, :t]), bits(o["tk"][r, :, :t])) and torch.isnan(tk[r, :, t + 1:].float()).all(), r
        assert torch.isnan(tv[r, :, t + 1:].float()).all(), r
    # ---- the attention against fp64
    got = ctx.double().reshape(B, nkv, gq, D)
    assert not torch.isnan(got).any()
    assert torch.isnan(buf[B:].float()).all() and torch.isnan(buf[:, nq * D:].float()).all(), "written outside [B, nq 128]"
    worst = 0.0
    for r in range(B):
        s, t = r // n, o["tails"][r]
        K = torch.cat([o["pk"][s, :, :plen[s]], tk[r, :, :t + 1]], dim=1).double()             # [nkv, keys, d]
        V = torch.cat([o["pv"][s, :, :plen[s]], tv[r, :, :t + 1]], dim=1).double()
        q = qkv[r, :nq * D].double().reshape(nkv, gq, D)
        p = torch.softmax(q @ K.transpose(1, 2) / np.sqrt(D), dim=-1)
        worst = max(worst, float((got[r] - p @ V).abs().max()))
    print(f"prefix kernels vs fp64 {dtype} nq={nq} nkv={nkv} n={n} {case}: max |error| {worst:.3e}")
    assert worst < (2e-2 if dtype == "bf16" else 2.5e-3), worst


def test_append_tail_f16_overflow_flag():
    from gritlm_amd import ops
    o = _operands("f16", 4, 2, 9, (1, 64, 70), seed=4)
    o["qkv"][5, (4 + 1) * D + 3] = 2e5                     # a k value beyond 65504 (whatever the rotation's angle: one of the pair >= 1.4e5)
    ops.f16_overflow_flag(DEV, clear=True)
    _launch(o)
    assert ops.f16_overflow_flag(DEV, clear=True)


# ------------------------------------------------------------------------------------------------------------------ 2. row independence
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_rows_do_not_depend_on_n_and_launches_reproduce(dtype):
    """rows 0..8 of every sequence at n = 20 against a launch at n = 9 over the same rows: the same bits; two identical launches too"""
    from gritlm_amd import prefix_ops
    nq, nkv = 32, 8
    o = _operands(dtype, nq, nkv, 20, (prefix_ops.kc() + 37, 65), seed=9)
    _, ctx20, *_ = _launch(o)
    _, again, *_ = _launch(o)
    assert torch.equal(ctx20, again)
    idx = torch.tensor([s * 20 + j for s in range(2) for j in range(9)], device=DEV)
    o9 = dict(o, n=9, B=18, qkv=o["qkv"][idx].contiguous(), tk=o["tk"][idx].contiguous(), tv=o["tv"][idx].contiguous(),
              lens=o["lens"][idx].contiguous(), tails=[o["tails"][i] for i in idx.tolist()])
    _, ctx9, *_ = _launch(o9)
    assert not torch.isnan(ctx9.float()).any() and torch.equal(ctx20[idx], ctx9)


# ------------------------------------------------------------------------------------------------------------------ 3. the decoder
T, TOPK, TOPP = 0.8, 40, 0.9


def _check_kept(lgf, toks):
    for b in range(toks.shape[0]):
        for t in range(toks.shape[1]):
            mine, margin = kept(lgf[b, t], T, TOPK, TOPP, with_margin=True)
            assert mine[toks[b, t]] or margin < 1e-6, (b, t)            # (fp32 exp one ulp apart on a boundary token)
            if margin >= 1e-5:
                assert hf_kept(lgf[b, t], T, TOPK, TOPP)[toks[b, t]], (b, t)


@pytest.mark.parametrize("cfg_name,policy", [("gqa", "bf16"), ("gqa", "f16_operands"), ("gqa", "f16_stream"), ("7b-l2s", "bf16"),
                                             ("7b-l2s", "f16_operands")])
def test_shared_prefix_decoder_vs_oracle(cfg_name, policy):
    """cached documents of per-row lengths (70, 41), 3 prompt tokens, 12 samples each: teacher-forced logits of the checked rows within
    the bounds of test_batched_decoder_vs_oracle (1 - cos: 2e-4 bf16, 1e-5 fp16 policies); every token in the warpers' kept set"""
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup(cfg_name)
    eng.set_precision(policy)
    B0, S0, P, n, new = 2, 70, 3, 12, 5
    doc = rng.integers(3, cfg["vocab_size"], size=(B0, S0)).astype(np.int64)
    plens = np.array([70, 41], dtype=np.int32)
    dmask = (np.arange(S0)[None] < plens[:, None]).astype(np.int64)
    _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.from_numpy(dmask).to(DEV), return_kv=True, kv_dtype=None)
    prompt = rng.integers(3, cfg["vocab_size"], size=(B0, P)).astype(np.int64)
    toks, lg = dec.generate(torch.from_numpy(prompt).to(DEV), new, past_key_values=kv, past_lens=torch.from_numpy(plens).to(DEV),
                            do_sample=True, temperature=T, top_k=TOPK, top_p=TOPP, seed=77, num_return_sequences=n, share_prefix=True,
                            return_logits=True)
    assert dec.last_precision == ("bf16" if policy == "bf16" else "f16") and tuple(toks.shape) == (B0 * n, new)
    toks_np, lgf = toks.cpu().numpy(), lg.float().cpu().numpy()
    _check_kept(lgf, toks_np)
    for s in range(B0):                                  # the n copies share their first-step logits bit for bit and then part
        assert all(torch.equal(lg[s * n + j, 0], lg[s * n, 0]) for j in range(n)), s
        assert len({tuple(r) for r in toks_np[s * n:s * n + n]}) > 1, s
    bound = 2e-4 if policy == "bf16" else 1e-5
    kv_ref = [O.mistral_encode(w, cfg, doc[s:s + 1], dmask[s:s + 1], return_layers="kv")[1] for s in range(B0)]
    for r in (range(B0 * n) if cfg_name == "gqa" else (0, 11, 12, 23)):
        s = r // n
        seq = np.concatenate([prompt[s], toks_np[r]])
        ref = O.mistral_continue(w, cfg, kv_ref[s], int(plens[s]), seq, lm)[P - 1:P - 1 + new].astype(np.float64)
        omc = _omc(lgf[r], ref)
        assert omc < bound, (r, omc)


@pytest.mark.parametrize("policy", ["bf16", "f16_operands"])
def test_shared_prefix_without_a_cache_on_ragged_prompts(policy):
    """prompt-only: 2 right-padded prompts of different lengths x 10 samples; the prefix is the encoder prefill's K/V of each prompt"""
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    eng.set_precision(policy)
    B0, P, n, new = 2, 19, 10, 5
    plen = np.array([19, 8])
    ids = rng.integers(3, cfg["vocab_size"], size=(B0, P)).astype(np.int64)
    mask = (np.arange(P)[None] < plen[:, None]).astype(np.int64)
    toks, lg = dec.generate(torch.from_numpy(ids).to(DEV), new, attention_mask=torch.from_numpy(mask).to(DEV), do_sample=True, temperature=T,
                            top_k=TOPK, top_p=TOPP, seed=77, num_return_sequences=n, share_prefix=True, return_logits=True)
    assert dec.last_prefill == "encoder" and tuple(toks.shape) == (B0 * n, new)
    toks_np, lgf = toks.cpu().numpy(), lg.float().cpu().numpy()
    _check_kept(lgf, toks_np)
    for r in range(B0 * n):
        s = r // n
        seq = np.concatenate([ids[s, :plen[s]], toks_np[r]])
        hid = O.mistral_encode(w, cfg, seq[None], None, causal=True)[0]
        ref = (hid.astype(np.float64) @ lm.astype(np.float64).T)[plen[s] - 1:plen[s] - 1 + new]
        assert _omc(lgf[r], ref) < (2e-4 if policy == "bf16" else 1e-5), r


# ------------------------------------------------------------------------------------------------------------------ 4. tails past a split
def test_tails_cross_a_split_graph_equals_eager():
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup("tiny")
    S0, P, n, new = 100, 2, 20, 70
    doc = rng.integers(3, cfg["vocab_size"], size=(1, S0)).astype(np.int64)
    _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.ones((1, S0), dtype=I64, device=DEV), return_kv=True)
    prompt = rng.integers(3, cfg["vocab_size"], size=(1, P)).astype(np.int64)
    kw = dict(past_key_values=kv, do_sample=True, temperature=T, top_k=TOPK, top_p=TOPP, num_return_sequences=n, share_prefix=True)
    tp = torch.from_numpy(prompt).to(DEV)
    dec.use_graph = True
    g1 = dec.generate(tp, new, seed=5, **kw)
    g2 = dec.generate(tp, new, seed=5, **kw)
    other = dec.generate(tp, new, seed=6, **kw)
    dec.use_graph = False
    e1 = dec.generate(tp, new, seed=5, **kw)
    dec.use_graph = True
    assert tuple(g1.shape) == (n, new) and torch.equal(g1, g2) and torch.equal(g1, e1) and not torch.equal(g1, other)
    toks, lg = dec.generate(tp, new, seed=5, return_logits=True, **kw)
    assert torch.equal(toks, g1)
    _, kv_ref = O.mistral_encode(w, cfg, doc, np.ones((1, S0), np.int64), return_layers="kv")
    for r in (0, 19):
        seq = np.concatenate([prompt[0], toks[r].cpu().numpy()])
        ref = O.mistral_continue(w, cfg, kv_ref, S0, seq, lm)[P - 1 + new - 1].astype(np.float64)
        assert _omc(lg[r, -1].float().cpu().numpy()[None], ref[None]) < 2e-4, r


# ------------------------------------------------------------------------------------------------------------------ 5. memory
def test_shared_prefix_saves_the_copies_of_the_cache():
    """peak allocated bytes over the call: the expanded call holds at least 2 n copies of past_key_values (the repeat of every layer, and
    the state), the shared one a single copy plus 64 rows x 64 tail slots -- so the peaks differ by at least (n - 1) copies"""
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    S0, n, new = 1024, 64, 4
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(1, S0)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    kv = [(k.clone(), v.clone()) for k, v in kv]
    past_bytes = sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in kv)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(1, 3)).astype(np.int64)).to(DEV)

    def peak(share):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        out = dec.generate(prompt, new, past_key_values=kv, do_sample=True, seed=3, num_return_sequences=n, share_prefix=share)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (n, new)
        return torch.cuda.max_memory_allocated()
    peak_expanded, peak_shared = peak(False), peak(True)
    print(f"peak allocated: expanded {peak_expanded}, shared {peak_shared}, past_key_values {past_bytes}")
    assert peak_shared <= peak_expanded - (n - 1) * past_bytes, (peak_shared, peak_expanded, past_bytes)


# ------------------------------------------------------------------------------------------------------------------ 6. fallbacks
def test_share_prefix_with_one_sequence_is_the_plain_call():
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(3, 30)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(3, 4)).astype(np.int64)).to(DEV)
    kw = dict(past_key_values=kv, do_sample=True, seed=8, return_logits=True)
    t0, l0 = dec.generate(prompt, 6, **kw)
    t1, l1 = dec.generate(prompt, 6, share_prefix=True, **kw)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    g0 = dec.generate(prompt, 6, past_key_values=kv)
    assert torch.equal(g0, dec.generate(prompt, 6, past_key_values=kv, share_prefix=True))          # greedy, n = 1: a no-op as well


def test_shared_f16_overflow_raises_or_falls_back_to_bf16():
    from gritlm_amd._lib import GritHipError
    eng, cfg, w, lm, dec, rng = _setup("tiny")
    B0, S0, P, new, n = 2, 40, 5, 4, 6
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B0, S0)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B0, P)).astype(np.int64)).to(DEV)
    eng.layers[0].wgu.mul_(400.0)
    eng.set_precision("f16_operands")
    kw = dict(past_key_values=kv, do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=99, num_return_sequences=n, share_prefix=True)
    with pytest.raises(GritHipError):
        dec.generate(prompt, new, on_overflow="raise", **kw)
    fb = dec.generate(prompt, new, on_overflow="bf16", **kw)
    assert dec.last_precision == "bf16 (f16 overflow)" and tuple(fb.shape) == (B0 * n, new)
    eng.set_precision("bf16")
    bf = dec.generate(prompt, new, **kw)
    assert dec.last_precision == "bf16" and torch.equal(fb, bf)


def test_sparse_moe_refuses_share_prefix():
    from gpu_checks import build_engine
    from gritlm_amd.decoder import MistralDecoder
    meng, mcfg, _ = build_engine("moe-tiny", 0)
    lm = (torch.randn((mcfg["vocab_size"], mcfg["hidden_size"]), generator=torch.Generator().manual_seed(2)) * 0.05)
    mdec = MistralDecoder(meng, lm)
    ids = torch.randint(3, mcfg["vocab_size"], (2, 5), generator=torch.Generator().manual_seed(3)).to(DEV)
    with pytest.raises(NotImplementedError, match="share_prefix"):
        mdec.generate(ids, 4, do_sample=True, num_return_sequences=2, seed=1, share_prefix=True)


# ------------------------------------------------------------------------------------------------------------------ 7. GritLM
def test_sample_native_share_prefix_on_a_checkpoint():
    """the rules of test_sample_native_on_a_checkpoint under share_prefix: [B 5, P + new], input rows in repeat_interleave order, pad
    after each row's EOS on the same draws"""
    import synth
    from gritlm_amd import GritLM
    with tempfile.TemporaryDirectory() as td:
        d16 = synth.build_mistral_dir(os.path.join(td, "m16"), "tiny", 0, "bfloat16")
        m = GritLM(d16, pooling_method="mean", attn="bbcc", device="cuda", torch_dtype=torch.bfloat16, mode="unified")
        texts = [" ".join(synth.WORDS[(3 * i) % 40:(3 * i) % 40 + 4 + i]) for i in range(4)]
        enc = m.tokenizer(texts, return_tensors="pt", padding=True, add_special_tokens=False)
        ids, mask = enc["input_ids"].to(DEV), enc["attention_mask"].to(DEV)
        P, new = ids.shape[1], 8
        kw = dict(num_return_sequences=5, seed=21, temperature=0.9, top_k=50, top_p=0.95, share_prefix=True)
        out = m.sample_native(ids, attention_mask=mask, max_new_tokens=new, min_new_tokens=new, **kw)
        assert tuple(out.shape) == (20, P + new) and torch.equal(out[:, :P], ids.repeat_interleave(5, dim=0))
        raw = m.native_decoder().generate(ids, new, attention_mask=mask, do_sample=True, **kw)
        assert torch.equal(out[:, P:], raw)
        eos = int(raw[0, 2])
        cut = m.sample_native(ids, attention_mask=mask, max_new_tokens=new, eos_token_id=eos, pad_token_id=0, **kw)
        got = cut[:, P:]
        for r in range(20):
            hits = (raw[r] == eos).nonzero()
            stop = int(hits[0]) + 1 if len(hits) else new
            k = min(stop, got.shape[1])
            assert torch.equal(got[r, :k], raw[r, :k]) and bool((got[r, k:] == 0).all()), r
        if bool((raw == eos).any(dim=1).all()):
            assert got.shape[1] == max(int((raw[r] == eos).nonzero()[0]) + 1 for r in range(20))
