"""Prompt prefill on cached K/V through the MFMA GEMMs (MistralDecoder.prefill = "gemm"): the two kernels of csrc/prefill.hip against fp64
numpy, the decoder against the fp32 oracle (O.mistral_continue) and the "rows" path, ragged right-padded prompts, fp16 overflow, and the
GritLM.generate_native flow on top of a query cache (the reference's query caching, rag/eval.py:200-238)."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, I32, I64 = torch.bfloat16, torch.float16, torch.int32, torch.int64


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


# ---------------------------------------------------------------------------------------------------------------- 1. attention kernel
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("P", [1, 7, 200])
@pytest.mark.parametrize("nq,nkv", [(32, 8), (4, 4)])
def test_attn_prefill_cached_vs_fp64(dtype, P, nq, nkv):
    from gritlm_amd import ops
    d, B, Lmax = 128, 3, 1024
    dt = BF16 if dtype == "bf16" else F16
    lens = (0, 37, 700)
    plen = (P, min(5, P), max(P - 3, 1))
    rng = np.random.default_rng(1000 + P + nq)
    G = nq // nkv
    stride = (nq + 2 * nkv) * d
    qkv = torch.from_numpy(rng.standard_normal((B * P, stride)).astype(np.float32) * 0.7).to(DEV).to(dt)
    ck = torch.from_numpy(rng.standard_normal((B, nkv, Lmax, d)).astype(np.float32) * 0.7).to(DEV).to(dt)
    cv = torch.from_numpy(rng.standard_normal((B, nkv, Lmax, d)).astype(np.float32)).to(DEV).to(dt)
    for b in range(B):                             # slots behind the last key any query sees: NaN -- none of it may leak
        ck[b, :, lens[b] + plen[b]:] = float("nan")
        cv[b, :, lens[b] + plen[b]:] = float("nan")
    tl, tp = torch.tensor(lens, dtype=I32, device=DEV), torch.tensor(plen, dtype=I32, device=DEV)
    out = torch.full((B * P, nq * d), float("nan"), dtype=dt, device=DEV)
    ops.attn_prefill_cached(qkv, ck, cv, tl, tp, nq, nkv, d, out=out)
    got = out.double().cpu().numpy().reshape(B, P, nq, d)
    Q = qkv.double().cpu().numpy().reshape(B, P, -1)[:, :, :nq * d].reshape(B, P, nq, d)
    K, V = ck.double().cpu().numpy(), cv.double().cpu().numpy()
    worst = 0.0
    for b in range(B):
        n = lens[b] + plen[b]
        for h in range(nq):
            sc = Q[b, :plen[b], h] @ K[b, h // G, :n].T / np.sqrt(d)                    # [plen, n]
            allowed = np.arange(n)[None, :] <= lens[b] + np.arange(plen[b])[:, None]
            sc = np.where(allowed, sc, -np.inf)
            p = np.exp(sc - sc.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
            worst = max(worst, float(np.max(np.abs(got[b, :plen[b], h] - p @ V[b, h // G, :n]))))
        assert np.all(got[b, plen[b]:] == 0.0), "padded rows must come back as exact zeros"
    assert not np.isnan(got).any()
    assert worst < (2e-2 if dtype == "bf16" else 2.5e-3), worst      # the bounds of the existing attention checks


# ---------------------------------------------------------------------------------------------------------------- 2. append kernel
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_kv_append_chunk_bitwise(dtype):
    from gritlm_amd import ops
    d, B, P, nq, nkv, Lmax = 128, 3, 9, 8, 2, 256
    dt = BF16 if dtype == "bf16" else F16
    lens, plen = (0, 37, 200), (9, 5, 1)
    rng = np.random.default_rng(7)
    qkv = torch.from_numpy(rng.standard_normal((B * P, (nq + 2 * nkv) * d + 64)).astype(np.float32)).to(DEV).to(dt)[:, :(nq + 2 * nkv) * d]
    ck = torch.from_numpy(rng.standard_normal((B, nkv, Lmax, d)).astype(np.float32)).to(DEV).to(dt)
    cv = torch.from_numpy(rng.standard_normal((B, nkv, Lmax, d)).astype(np.float32)).to(DEV).to(dt)
    ck0, cv0 = ck.clone(), cv.clone()
    ops.kv_append_chunk(qkv, ck, cv, torch.tensor(lens, dtype=I32, device=DEV), torch.tensor(plen, dtype=I32, device=DEV), nq, nkv, d)
    want_k, want_v = ck0.clone(), cv0.clone()
    rows = qkv.reshape(B, P, -1)
    for b in range(B):
        for i in range(plen[b]):
            want_k[b, :, lens[b] + i] = rows[b, i, nq * d:(nq + nkv) * d].view(nkv, d)
            want_v[b, :, lens[b] + i] = rows[b, i, (nq + nkv) * d:].view(nkv, d)
    assert torch.equal(ck.view(torch.int16), want_k.view(torch.int16))
    assert torch.equal(cv.view(torch.int16), want_v.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- 3. decoder vs fp32 oracle
@pytest.mark.parametrize("cfg_name,B,S0,P,new,policy", [
    ("gqa", 2, 70, 11, 5, "bf16"), ("gqa", 2, 70, 37, 5, "bf16"), ("gqa", 2, 70, 11, 5, "f16_operands"), ("gqa", 2, 70, 37, 5, "f16_stream"),
    ("7b-l2s", 1, 1500, 600, 4, "bf16"), ("7b-l2s", 1, 1500, 600, 4, "f16_operands")])
def test_decoder_gemm_prefill_vs_oracle(cfg_name, B, S0, P, new, policy):
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup(cfg_name)
    eng.set_precision(policy)
    doc = rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)
    plens = np.array([S0, S0 - 29][:B], dtype=np.int32)
    dmask = (np.arange(S0)[None] < plens[:, None]).astype(np.int64)
    _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.from_numpy(dmask).to(DEV), return_kv=True, kv_dtype=None)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)).to(DEV)
    pl = torch.from_numpy(plens).to(DEV)
    res = {}
    for mode in ("gemm", "rows"):
        dec.prefill = mode
        res[mode] = dec.generate(prompt, new, past_key_values=kv, past_lens=pl, return_logits=True)
        res[mode + "_path"] = dec.last_prefill
    assert res["gemm_path"] == "gemm"
    assert res["rows_path"] == ("rows" if B * P <= 512 else "tokens")
    toks, lg = res["gemm"]
    bound = 2e-4 if policy == "bf16" else 1e-5
    for b in range(B):
        _, kv_ref = O.mistral_encode(w, cfg, doc[b:b + 1], dmask[b:b + 1], return_layers="kv")
        seq = np.concatenate([prompt[b].cpu().numpy(), toks[b].cpu().numpy()])
        ref = O.mistral_continue(w, cfg, kv_ref, int(plens[b]), seq, lm)[P - 1:P - 1 + new].astype(np.float64)
        got = lg[b].float().cpu().numpy().astype(np.float64)
        omc = _omc(got, ref)
        assert omc < bound, (b, omc)
        # greedy tokens == the "rows" path wherever the fp32 margin is clear (up to the first position the two paths disagree on)
        srt = np.sort(ref, axis=-1)
        clear = (srt[:, -1] - srt[:, -2]) > 4 * float(np.max(np.abs(got - ref))) + 1e-4
        rt = res["rows"][0][b].cpu().numpy()
        gt = toks[b].cpu().numpy()
        for t in range(new):
            if not clear[t]:
                break
            assert gt[t] == rt[t], (b, t)


# ---------------------------------------------------------------------------------------------------------------- 4. ragged prompts
def test_ragged_prompts_match_rows_alone():
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    B, S0, P, new = 3, 80, 23, 6
    doc = rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)
    _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.ones((B, S0), dtype=I64, device=DEV), return_kv=True)
    past_lens = torch.tensor([80, 51, 17], dtype=I32, device=DEV)
    plen = [23, 9, 1]
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)).to(DEV)
    mask = (torch.arange(P, device=DEV)[None] < torch.tensor(plen, device=DEV)[:, None]).to(I64)
    dec.prefill = "gemm"
    toks, lg = dec.generate(prompt, new, attention_mask=mask, past_key_values=kv, past_lens=past_lens, return_logits=True)
    assert dec.last_prefill == "gemm"
    for b in range(B):
        kv1 = [(k[b:b + 1], v[b:b + 1]) for k, v in kv]
        t1, l1 = dec.generate(prompt[b:b + 1], new, attention_mask=mask[b:b + 1], past_key_values=kv1, past_lens=past_lens[b:b + 1],
                              return_logits=True)
        # the GEMMs and the attention compute each row independently of how many rows share the launch: bit for bit
        assert torch.equal(t1[0], toks[b]), b
        assert torch.equal(l1[0], lg[b]), b
    dec.prefill = "rows"
    with pytest.raises(NotImplementedError):
        dec.generate(prompt, new, attention_mask=mask, past_key_values=kv, past_lens=past_lens)
    left = torch.flip(mask, dims=[1])
    for mode in ("rows", "gemm"):
        dec.prefill = mode
        with pytest.raises(NotImplementedError):
            dec.generate(prompt, new, attention_mask=left, past_key_values=kv, past_lens=past_lens)


# ---------------------------------------------------------------------------------------------------------------- 5. fp16 overflow
def test_gemm_prefill_f16_overflow():
    from gritlm_amd._lib import GritHipError
    eng, cfg, w, lm, dec, rng = _setup("tiny")
    S0, P, new = 70, 21, 3
    doc = rng.integers(3, cfg["vocab_size"], size=(1, S0)).astype(np.int64)
    _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.ones((1, S0), dtype=I64, device=DEV), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(1, P)).astype(np.int64)).to(DEV)
    eng.layers[0].wgu.mul_(400.0)                  # |gate|, |up| x 400: silu(g) u beyond 65504 for some elements (a massive-activation model)
    eng.set_precision("f16_operands")
    dec.prefill = "gemm"
    with pytest.raises(GritHipError):
        dec.generate(prompt, new, past_key_values=kv, on_overflow="raise")
    assert dec.last_prefill == "gemm"
    t_fb = dec.generate(prompt, new, past_key_values=kv, on_overflow="bf16")
    assert dec.last_precision == "bf16 (f16 overflow)" and dec.last_prefill == "gemm"
    eng.set_precision("bf16")
    t_bf = dec.generate(prompt, new, past_key_values=kv)
    assert dec.last_precision == "bf16" and dec.last_prefill == "gemm"
    assert torch.equal(t_fb, t_bf)


# ---------------------------------------------------------------------------------------------------------------- 6. GritLM.generate_native
def test_generate_native_query_cache_gemm_prefill():
    import synth
    from transformers import DynamicCache
    from gritlm_amd import GritLM
    with tempfile.TemporaryDirectory() as td:
        d16 = synth.build_mistral_dir(os.path.join(td, "m16"), "tiny", 0, "bfloat16")
        m = GritLM(d16, pooling_method="mean", attn="bbcc", device="cuda", torch_dtype=torch.bfloat16, mode="unified")
        # query caching: the cache is the QUERY's bidirectional K/V, the input is the passage plus the prompt
        _, cache = m.encode([" ".join(synth.WORDS[3:9])], max_length=48, get_cache=True)
        get = lambda c, li: (c.layers[li].keys, c.layers[li].values) if hasattr(c, "layers") else (c[li][0], c[li][1])
        n_layers = len(cache.layers) if hasattr(cache, "layers") else len(cache)
        kv = [(get(cache, li)[0].clone(), get(cache, li)[1].clone()) for li in range(n_layers)]
        S0 = kv[0][0].shape[2]
        words = synth.WORDS * 8
        passage = m.tokenizer([" ".join(words[10:70])], return_tensors="pt", add_special_tokens=False)["input_ids"].to(DEV)
        P = passage.shape[1]
        mask = torch.ones((1, S0 + P), dtype=torch.long, device=DEV)
        dec = m.native_decoder()
        dec.prefill = "gemm"
        full = m.generate_native(input_ids=passage, attention_mask=mask, past_key_values=kv, max_new_tokens=6, min_new_tokens=6, pad_token_id=0)
        assert dec.last_prefill == "gemm"
        assert tuple(full.shape) == (1, P + 6) and torch.equal(full[:, :P], passage)
        pc = DynamicCache()
        for li, (k_, v_) in enumerate(kv):
            pc.update(k_.clone(), v_.clone(), li)
        hf = m.generate(input_ids=torch.cat([torch.zeros((1, S0), dtype=torch.long, device=DEV), passage], dim=1), attention_mask=mask,
                        past_key_values=pc, max_new_tokens=6, min_new_tokens=6, do_sample=False, pad_token_id=0)[0, S0 + P:]
        assert int((hf == full[0, P:]).sum()) >= 4          # as check_generate_native_api counts (bf16 near-ties on a random tiny model)
        # batched, right-padded passages on the same query cache: each row as it runs alone
        short = m.tokenizer([" ".join(words[20:41])], return_tensors="pt", add_special_tokens=False)["input_ids"].to(DEV)
        n1 = short.shape[1]
        assert n1 < P
        ids2 = torch.zeros((2, P), dtype=passage.dtype, device=DEV)
        ids2[0], ids2[1, :n1] = passage[0], short[0]
        m2 = (torch.arange(P, device=DEV)[None] < torch.tensor([P, n1], device=DEV)[:, None]).to(torch.long)
        kv2 = [(k.expand(2, -1, -1, -1).contiguous(), v.expand(2, -1, -1, -1).contiguous()) for k, v in kv]
        mask2 = torch.cat([torch.ones((2, S0), dtype=m2.dtype, device=DEV), m2], dim=1)
        both = m.generate_native(input_ids=ids2, attention_mask=mask2, past_key_values=kv2, max_new_tokens=6, min_new_tokens=6, pad_token_id=0)
        assert dec.last_prefill == "gemm"
        assert torch.equal(both[0, ids2.shape[1]:], full[0, P:])
        one = m.generate_native(input_ids=ids2[1:, :n1], attention_mask=torch.ones((1, S0 + n1), dtype=torch.long, device=DEV),
                                past_key_values=kv, max_new_tokens=6, min_new_tokens=6, pad_token_id=0)
        assert torch.equal(both[1, ids2.shape[1]:], one[0, n1:])
