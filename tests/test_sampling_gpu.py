"""Sampled decoding on the MI355X: grit_sample_advance[_f32] against the numpy restatement of include/gritlm_hip.h (test_sampling_cpu.py:
Philox4x32-10, fp64 Gumbel, the kept set), padding and non-finite logits, greedy equivalence, the draw distribution (chi-square with power
against the wrong orderings), reproducibility and row independence; then MistralDecoder.generate(do_sample=True) and GritLM.sample_native:
the kept set of every step, teacher-forced logits against the fp32 oracle, graph against eager, seeds, num_return_sequences, top_k = 1
against greedy, EOS padding, the fp16 overflow fallback and the sparse-MoE row limit."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_sampling_cpu import draw, hf_kept, kept, probs  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
LD = 32008


def _buf(x: np.ndarray, fmt: str, ld: int = LD, pad=float("inf")):
    """logits [B, V] in a [B, ld] buffer of the format whose columns V .. ld-1 hold ``pad``; returns (view [B, V], fp32 numpy of the view)"""
    B, V = x.shape
    dt = BF16 if fmt == "bf16" else F32
    b = torch.full((B, ld), pad, dtype=dt, device=DEV)
    b[:, :V] = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV).to(dt)
    v = b[:, :V]
    return v, v.float().cpu().numpy()


def _run(lg, keys, T, k, p, launches=1, step0=0):
    """``launches`` draws per row (t = step0, step0 + 1, ...): history [B, launches] int64, next, lens, step"""
    from gritlm_amd import ops
    B = lg.shape[0]
    nxt = torch.zeros((B,), dtype=I64, device=DEV)
    lens = torch.zeros((B,), dtype=I32, device=DEV)
    hist = torch.full((B, step0 + launches), -1, dtype=I64, device=DEV)
    step = torch.tensor([step0], dtype=I32, device=DEV)
    kt = torch.tensor([(int(x) % 2 ** 64) - (2 ** 64 if int(x) % 2 ** 64 >= 2 ** 63 else 0) for x in keys], dtype=I64, device=DEV)
    for _ in range(launches):
        ops.sample_advance(lg, nxt, kt, T, k, p, lens, hist, step)
    torch.cuda.synchronize()
    return hist[:, step0:].cpu().numpy(), nxt.cpu().numpy(), lens.cpu().numpy(), int(step.item())


SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 0.9), (0.2, 0, 0.95), (1.3, 200, 0.5), (1.0, 50, 1.0)]


# ------------------------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("fmt", ["bf16", "f32"])
@pytest.mark.parametrize("V", [32000, 32003])
def test_padding_and_nonfinite_logits(fmt, V):
    """+inf padding columns are never read; -inf and NaN tokens are never drawn; a row with no finite logit draws token 0"""
    rng = np.random.default_rng(V)
    B = 8
    x = rng.standard_normal((B, V)).astype(np.float32) * 3
    bad = np.zeros((B, V), bool)
    for b in range(B - 1):
        i = rng.choice(V, 200, replace=False)
        x[b, i[:100]], x[b, i[100:]] = np.nan, -np.inf
        bad[b, i] = True
    x[B - 1, ::2], x[B - 1, 1::2] = -np.inf, np.nan
    lg, _ = _buf(x, fmt)
    for T, k, p in SETTINGS:
        hist, nxt, lens, step = _run(lg, [11 + b for b in range(B)], T, k, p, launches=16)
        assert step == 16 and (lens == 16).all() and (hist[:, -1] == nxt).all()
        assert ((hist >= 0) & (hist < V)).all(), (T, k, p)
        for b in range(B - 1):
            assert not bad[b, hist[b]].any(), (T, k, p, b)
        assert (hist[B - 1] == 0).all()


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
def test_top_k_1_and_top_p_0_are_greedy(fmt):
    from gritlm_amd import ops
    rng = np.random.default_rng(4)
    B, V = 64, 32003
    lg, xf = _buf(rng.standard_normal((B, V)).astype(np.float32) * 2, fmt)
    srt = np.sort(xf, axis=1)
    unique = srt[:, -1] > srt[:, -2]
    want = torch.zeros((B,), dtype=I64, device=DEV)
    ops.argmax_advance(lg, want)
    want = want.cpu().numpy()
    for T, k, p in ((0.7, 1, 1.0), (1.0, 0, 0.0), (1.9, 50, 0.0)):
        hist, *_ = _run(lg, range(100, 100 + B), T, k, p, launches=3)
        assert unique.sum() > 50 and (hist[unique] == want[unique, None]).all(), (T, k, p)


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
def test_draws_equal_the_numpy_restatement(fmt):
    """512 draws (64 rows x 8 launches over the settings): numpy's Philox with fp64 Gumbel gives the kernel's token; a mismatch is allowed
    only where the two best perturbed scores lie within 1e-4 (fp32 against fp64 noise)"""
    rng = np.random.default_rng(7)
    B, V = 64, 32003
    x = (rng.standard_normal((B, V)) * rng.uniform(0.5, 4, (B, 1))).astype(np.float32)
    lg, xf = _buf(x, fmt)
    mism = 0
    for i, (T, k, p) in enumerate(SETTINGS[:4]):
        keys = [(2 ** 63 + 977 * i + 31 * b) for b in range(B)]
        hist, *_ = _run(lg, keys, T, k, p, launches=2, step0=5 * i)
        for b in range(B):
            for j in range(2):
                tok, gap = draw(xf[b], T, k, p, keys[b], 5 * i + j)
                if hist[b, j] != tok:
                    mism += 1
                    assert gap < 1e-4, (fmt, T, k, p, b, j, int(hist[b, j]), tok, gap)
    assert mism <= 2


def _distribution_logits(fmt):
    """V = 32000: 60 head tokens (4 .. 0, spread over the vocabulary) over a tail at -5, rounded to the format: top-k 50 cuts the tail and
    the last head tokens, top-p 0.9 / 0.95 cut inside the top-k set"""
    V = 32000
    x = np.full((V,), -5.0, np.float32)
    head = (np.arange(60) * 523 + 17) % V
    x[head] = np.linspace(4.0, 0.0, 60)
    _, xf = _buf(x[None], fmt)
    return xf[0]


def _chi2_p(counts, pr, n):
    """chi-square p-value of counts against probabilities pr (bins with expected < 5 merged); 0 when a token outside pr's support was drawn"""
    from scipy.stats import chi2
    if counts[pr == 0].sum() > 0:
        return 0.0
    exp = pr * n
    big = exp >= 5
    obs_b, exp_b = list(counts[big]), list(exp[big])
    if (~big).any() and exp[~big].sum() > 0:
        obs_b.append(counts[~big].sum()); exp_b.append(exp[~big].sum())
    obs_b, exp_b = np.array(obs_b, np.float64), np.array(exp_b)
    stat = float(((obs_b - exp_b) ** 2 / exp_b).sum())
    return float(chi2.sf(stat, len(obs_b) - 1))


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
@pytest.mark.parametrize("T,k,p", [(0.7, 50, 0.9), (0.2, 0, 0.95), (1.0, 50, 1.0)])
def test_draw_distribution(fmt, T, k, p):
    """64 identical rows with distinct keys x 256 launches = 16384 draws against the fp64 kept-set probabilities (p >= 1e-6, fixed keys:
    deterministic); with T != 1 and top_p < 1 the same counts must fail (p < 1e-6) against the distribution without the temperature and
    against top-p applied before the temperature"""
    xf = _distribution_logits(fmt)
    V = xf.shape[0]
    assert kept(xf, T, k, p).sum() < kept(xf, T, 0, 1.0).sum()        # the filters bind
    if k and p < 1:
        assert kept(xf, T, k, p).sum() < kept(xf, T, k, 1.0).sum() and kept(xf, T, k, 1.0).sum() < kept(xf, T, 0, 1.0).sum()
    lg, _ = _buf(np.repeat(xf[None], 64, axis=0), fmt)
    hist, *_ = _run(lg, [12345 + r for r in range(64)], T, k, p, launches=256)
    counts = np.bincount(hist.reshape(-1), minlength=V).astype(np.float64)
    n = counts.sum()
    assert n == 16384
    assert _chi2_p(counts, probs(xf, T, k, p), n) >= 1e-6
    if T != 1.0 and p < 1.0:
        assert _chi2_p(counts, probs(xf, T, k, p, mode="no_temperature"), n) < 1e-6
        assert _chi2_p(counts, probs(xf, T, k, p, mode="p_first"), n) < 1e-6


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
def test_reproducible_and_independent_of_other_rows(fmt):
    rng = np.random.default_rng(9)
    V = 32003
    x = rng.standard_normal((64, V)).astype(np.float32)
    lg, _ = _buf(x, fmt)
    keys = [2 ** 64 - 3 + r for r in range(64)]
    for T, k, p in SETTINGS:
        a, *_ = _run(lg, keys, T, k, p, launches=4, step0=2)
        b, *_ = _run(lg, keys, T, k, p, launches=4, step0=2)
        assert np.array_equal(a, b)
        y = x.copy()
        y[1:] = rng.standard_normal((63, V))
        lg2, _ = _buf(y, fmt)
        c, *_ = _run(lg2, [keys[0]] + [7 * r for r in range(1, 64)], T, k, p, launches=4, step0=2)
        one, *_ = _run(lg[:1], keys[:1], T, k, p, launches=4, step0=2)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[0], one[0]), (T, k, p)


# ------------------------------------------------------------------------------------------------------------------ the decoder
def _setup(cfg_name, seed=6, lm_seed=131):
    import gritlm_oracle as O
    from gpu_checks import build_engine
    from gritlm_amd.decoder import MistralDecoder
    eng, cfg, w = build_engine(cfg_name, seed)
    rng = np.random.default_rng(lm_seed)
    lm = O.bf16_round((rng.standard_normal((cfg["vocab_size"], cfg["hidden_size"])) * 0.05).astype(np.float32))
    return eng, cfg, w, lm, MistralDecoder(eng, torch.from_numpy(lm)), rng


def _omc(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(1.0 - np.sum(a * b, axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))))


@pytest.mark.parametrize("policy", ["bf16", "f16_operands"])
@pytest.mark.parametrize("B", [4, 24])
@pytest.mark.parametrize("cached", [True, False])
def test_sampled_steps_keep_the_warpers_set_and_match_the_oracle(policy, B, cached):
    """every sampled token lies in the set transformers' warpers keep on that step's returned logits (and in the header's set), and the
    teacher-forced logits along the sampled sequences agree with the fp32 oracle (2e-4 bf16 / 1e-5 fp16 operands)"""
    import gritlm_oracle as O
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    eng.set_precision(policy)
    T, k, p, new = 0.8, 40, 0.9, 6
    if cached:
        S0, P = 40, 3
        doc = rng.integers(3, cfg["vocab_size"], size=(B, S0)).astype(np.int64)
        plens = (S0 - (np.arange(B) * 7) % 23).astype(np.int32)
        dmask = (np.arange(S0)[None] < plens[:, None]).astype(np.int64)
        _, kv = eng.forward(torch.from_numpy(doc).to(DEV), torch.from_numpy(dmask).to(DEV), return_kv=True, kv_dtype=None)
        prompt = rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)
        toks, lg = dec.generate(torch.from_numpy(prompt).to(DEV), new, past_key_values=kv, past_lens=torch.from_numpy(plens).to(DEV),
                                return_logits=True, do_sample=True, temperature=T, top_k=k, top_p=p, seed=77)
    else:
        P = 11
        prompt = rng.integers(3, cfg["vocab_size"], size=(B, P)).astype(np.int64)
        toks, lg = dec.generate(torch.from_numpy(prompt).to(DEV), new, return_logits=True, do_sample=True, temperature=T, top_k=k, top_p=p,
                                seed=77)
    toks, lgf = toks.cpu().numpy(), lg.float().cpu().numpy()
    bound = 2e-4 if policy == "bf16" else 1e-5
    for b in range(B):
        for t in range(new):
            mine, margin = kept(lgf[b, t], T, k, p, with_margin=True)
            assert mine[toks[b, t]] or margin < 1e-6, (b, t)            # (fp32 exp one ulp apart on a boundary token)
            if margin >= 1e-5:
                assert hf_kept(lgf[b, t], T, k, p)[toks[b, t]], (b, t)
        seq = np.concatenate([prompt[b], toks[b]])
        if cached:
            _, kv_ref = O.mistral_encode(w, cfg, doc[b:b + 1], dmask[b:b + 1], return_layers="kv")
            ref = O.mistral_continue(w, cfg, kv_ref, int(plens[b]), seq, lm)[P - 1:P - 1 + new]
        else:
            hid = O.mistral_encode(w, cfg, seq[None], None, causal=True)[0]
            ref = (hid.astype(np.float64) @ lm.astype(np.float64).T)[P - 1:P - 1 + new]
        assert _omc(lgf[b], ref) < bound, (b, _omc(lgf[b], ref))
    assert len({tuple(r) for r in toks}) > 1


@pytest.mark.parametrize("policy", ["bf16", "f16_operands"])
@pytest.mark.parametrize("B", [4, 24])
def test_graph_equals_eager_and_seeds_reproduce(policy, B):
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    eng.set_precision(policy)
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, 30)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, 2)).astype(np.int64)).to(DEV)
    kw = dict(past_key_values=kv, do_sample=True, temperature=1.0, top_k=0, top_p=0.95)
    dec.use_graph = True
    g1 = dec.generate(prompt, 20, seed=5, **kw)
    g2 = dec.generate(prompt, 20, seed=5, **kw)
    dec.use_graph = False
    e1 = dec.generate(prompt, 20, seed=5, **kw)
    dec.use_graph = True
    assert torch.equal(g1, g2) and torch.equal(g1, e1)
    assert not torch.equal(g1, dec.generate(prompt, 20, seed=6, **kw))
    torch.manual_seed(1234)
    m1 = dec.generate(prompt, 20, **kw)
    torch.manual_seed(1234)
    m2 = dec.generate(prompt, 20, **kw)
    assert torch.equal(m1, m2)


def test_num_return_sequences_five_copies():
    """4 prompts x 5: [20, new]; the copies of a prompt share their first-step logits and their continuations differ"""
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(4, 7)).astype(np.int64)).to(DEV)
    toks, lg = dec.generate(prompt, 8, return_logits=True, do_sample=True, num_return_sequences=5, seed=3)
    assert tuple(toks.shape) == (20, 8)
    first = lg[:, 0].float().cpu().numpy()
    for i in range(4):
        for j in range(5):
            assert _omc(first[5 * i + j][None], first[5 * i][None]) < 1e-6
        assert len({tuple(r) for r in toks[5 * i:5 * i + 5].tolist()}) > 1, i
    # the same rows as a call on the repeated prompts
    again = dec.generate(prompt.repeat_interleave(5, dim=0), 8, do_sample=True, seed=3)
    assert torch.equal(again, toks)


@pytest.mark.parametrize("B", [4, 24])
def test_top_k_1_equals_greedy_on_f16_operands(B):
    eng, cfg, w, lm, dec, rng = _setup("gqa")
    eng.set_precision("f16_operands")
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, 30)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, 3)).astype(np.int64)).to(DEV)
    greedy, lg = dec.generate(prompt, 12, past_key_values=kv, return_logits=True)
    sampled = dec.generate(prompt, 12, past_key_values=kv, do_sample=True, top_k=1, temperature=0.6, seed=11)
    top2 = lg.float().topk(2, dim=-1).values
    tied = (top2[..., 0] == top2[..., 1]).cpu().numpy()
    for b in range(B):
        stop = int(np.argmax(tied[b])) + 1 if tied[b].any() else 12
        assert torch.equal(greedy[b, :stop], sampled[b, :stop]), b


def test_f16_overflow_falls_back_with_the_same_seed():
    eng, cfg, w, lm, dec, rng = _setup("tiny")
    B = 6
    doc = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, 40)).astype(np.int64)).to(DEV)
    _, kv = eng.forward(doc, torch.ones_like(doc), return_kv=True)
    prompt = torch.from_numpy(rng.integers(3, cfg["vocab_size"], size=(B, 4)).astype(np.int64)).to(DEV)
    eng.layers[0].wgu.mul_(400.0)
    eng.set_precision("f16_operands")
    kw = dict(past_key_values=kv, do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=99, num_return_sequences=2)
    fb = dec.generate(prompt, 5, on_overflow="bf16", **kw)
    assert dec.last_precision == "bf16 (f16 overflow)" and tuple(fb.shape) == (12, 5)
    eng.set_precision("bf16")
    bf = dec.generate(prompt, 5, **kw)
    assert dec.last_precision == "bf16" and torch.equal(fb, bf)


def test_sparse_moe_sampling_row_limit():
    from gpu_checks import build_engine
    from gritlm_amd.decoder import MistralDecoder
    meng, mcfg, _ = build_engine("moe-tiny", 0)
    lm = (torch.randn((mcfg["vocab_size"], mcfg["hidden_size"]), generator=torch.Generator().manual_seed(2)) * 0.05)
    mdec = MistralDecoder(meng, lm)
    ids = torch.randint(3, mcfg["vocab_size"], (4, 5), generator=torch.Generator().manual_seed(3)).to(DEV)
    out = mdec.generate(ids, 4, do_sample=True, num_return_sequences=2, seed=1)
    assert tuple(out.shape) == (8, 4) and bool(((out >= 0) & (out < mcfg["vocab_size"])).all())
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        mdec.generate(ids[:3], 4, do_sample=True, num_return_sequences=3, seed=1)


def test_sample_native_on_a_checkpoint():
    """GritLM.sample_native (mode 'unified', synth tiny checkpoint): Hugging Face's return shape with the input rows repeated in
    repeat_interleave order; EOS padding and trimming follow generate_native's rules on the same draws"""
    import synth
    from gritlm_amd import GritLM
    with tempfile.TemporaryDirectory() as td:
        d16 = synth.build_mistral_dir(os.path.join(td, "m16"), "tiny", 0, "bfloat16")
        m = GritLM(d16, pooling_method="mean", attn="bbcc", device="cuda", torch_dtype=torch.bfloat16, mode="unified")
        texts = [" ".join(synth.WORDS[(3 * i) % 40:(3 * i) % 40 + 4 + i]) for i in range(4)]
        enc = m.tokenizer(texts, return_tensors="pt", padding=True, add_special_tokens=False)
        ids, mask = enc["input_ids"].to(DEV), enc["attention_mask"].to(DEV)
        P, new = ids.shape[1], 8
        out = m.sample_native(ids, attention_mask=mask, max_new_tokens=new, min_new_tokens=new, num_return_sequences=5, seed=21,
                              temperature=0.9, top_k=50, top_p=0.95)
        assert tuple(out.shape) == (20, P + new) and torch.equal(out[:, :P], ids.repeat_interleave(5, dim=0))
        raw = m.native_decoder().generate(ids, new, attention_mask=mask, do_sample=True, num_return_sequences=5, seed=21, temperature=0.9,
                                          top_k=50, top_p=0.95)
        assert torch.equal(out[:, P:], raw)
        eos = int(raw[0, 2])
        cut = m.sample_native(ids, attention_mask=mask, max_new_tokens=new, eos_token_id=eos, pad_token_id=0, num_return_sequences=5,
                              seed=21, temperature=0.9, top_k=50, top_p=0.95)
        got = cut[:, P:]
        for r in range(20):
            hits = (raw[r] == eos).nonzero()
            stop = int(hits[0]) + 1 if len(hits) else new
            n = min(stop, got.shape[1])
            assert torch.equal(got[r, :n], raw[r, :n]) and bool((got[r, n:] == 0).all()), r
        if bool((raw == eos).any(dim=1).all()):
            assert got.shape[1] == max(int((raw[r] == eos).nonzero()[0]) + 1 for r in range(20))
        torch.manual_seed(8)
        a = m.sample_native(ids, attention_mask=mask, max_new_tokens=4, min_new_tokens=4)
        torch.manual_seed(8)
        assert torch.equal(a, m.sample_native(ids, attention_mask=mask, max_new_tokens=4, min_new_tokens=4))
