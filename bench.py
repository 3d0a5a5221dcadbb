#!/usr/bin/env python3
"""bench.py -- headline benchmark of the GritLM embedding-encode hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]   (N > 1 without a launcher: bench.py starts its own N ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch: GritLM-7B (Mistral-7B shape, 32 layers, bf16,
random-init weights) bidirectional encode of 256 docs x 512 tokens, masked mean pooling, L2-normalise
(BASELINE.json configs[1]).  Token ids are synthetic and already resident in HBM when the timed region
starts.  N > 1: one replica per GPU, every rank encodes its own 256-doc batch (documents are independent:
no data-path collective, weak scaling); value = docs of all ranks / max-over-ranks time.

Prints ONE JSON line (rank 0) with the driver's contract fields plus
  roofline:     dominant kernel (gemm_bf16_nt, bf16 MFMA bound) measured live with HIP events during the timed steps.
A plain run stops there: set up, warm up, time K steps, write the outputs (--dump-outputs), print the line.
--dump-outputs DIR: the pooled, normalised embeddings of the last timed step as DIR/embeddings.npy (float32, DOCS x hidden; rank r > 0
                writes DIR/embeddings_rank<r>.npy).  Weights and token ids are seeded, so the same arguments give the same inputs every run.
--full adds everything else (each leg can still be dropped with its --no-* flag):
  gemm_over_vendor_*: hipBLASLt on the same GEMM shapes in the same process,
  ragged_batch: padded vs packed path on a ragged batch,
  parity_full_depth: the engine's embeddings of the timed batch vs the reference-equivalent module in FP32 on this GPU on the engine's own
                weights (numeric bounds, both precision policies), + the fixture model against the fp32 numpy oracle,
  cpu_baseline: the reference's CPU encode (stock transformers.MistralModel + bidirectional mask + pooling, bit-equal to the reference
                on the reference-generated fixtures; oracle/torch_reference.py) timed on this host's cores on a bounded sample (N = 1 only),
  rocm_torch_baseline: the same Python on this GPU through stock PyTorch-ROCm (bf16, sdpa) at the full config -- what a user gets today,
  contrastive:  BASELINE configs[2] as stated (256 pairs x (1 + 8) x 512 tokens per GPU, GradCache chunk 32), 1 timed step (--contrastive-steps),
  mixtral_8x7b_seq2048 / rag_doc_caching: BASELINE configs[3] / configs[4] as time-boxed child processes (N = 1 only; --no-mixtral / --no-rag).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0   # dense, /opt/skills/guides/MI355X_MICROARCH.md


def measured_traffic():
    """HBM-side bytes per GEMM launch from the committed rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction +
    WRITE_SIZE, each collected in its own --pmc run: profiles/rNN_gemm_pmc.json).  bench.py cannot run PMC
    collection itself, so the figure is only as fresh as that profile: the profile stores the sha256 of the kernel
    source it was collected on and a mismatch with the shipped gritlm_amd/csrc/gemm_bf16.hip is flagged ``traffic_stale``.
    Returns (bytes or None, {provenance fields})."""
    import glob
    import hashlib
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_pmc.json")))
    if not files:
        return None, {}
    try:
        d = json.load(open(files[-1]))
        sha = hashlib.sha256(open(os.path.join(ROOT, "gritlm_amd", "csrc", "gemm_bf16.hip"), "rb").read()).hexdigest()[:16]
        note = {"traffic_source": os.path.relpath(files[-1], ROOT), "traffic_stale": d.get("gemm_bf16_hip_sha16") != sha}
        return d["avg_traffic_bytes_per_gemm_launch_in_forward"], note
    except Exception:  # noqa: BLE001
        return None, {}
DOCS, SEQ = 256, 512


def cpu_baseline():
    """The reference's CPU path on this host's cores: stock transformers.MistralModel + 4-D bidirectional mask + pooling (bit-equal to
    the reference's GritLM.encode core on the reference-generated fixtures: oracle/torch_reference.py), fp32, bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch_reference as TR
    return TR.time_cpu(layers=2, docs=8, seq=SEQ)


def vendor_gemm_comparator(dev, M=DOCS * SEQ):
    """hipBLASLt (`torch.matmul`, plain GEMM without the fused RoPE / residual / SwiGLU epilogues) on the model's four GEMM shapes, same
    GPU, same run, random bf16 operands: context for `roofline.achieved` (the chip is power-limited on random data)."""
    out, tot_f, tot_t = {}, 0.0, 0.0
    for name, (N, K) in {"qkv": (6144, 4096), "o_proj": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}.items():
        a = torch.randn((M, K), device=dev, dtype=torch.float32).to(torch.bfloat16)
        w = (torch.randn((N, K), device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16)
        wt = w.t()
        for _ in range(2):
            c = a @ wt
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            c = a @ wt
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 5
        fl = 2.0 * M * N * K
        out[name] = fl / (ms * 1e-3) / 1e12
        tot_f += fl; tot_t += ms * 1e-3
        del a, w, wt, c
    torch.cuda.empty_cache()
    out["flop_weighted"] = tot_f / tot_t / 1e12
    return out


def vendor_gemm_sustained(dev, layers=8, passes=2, M=DOCS * SEQ):
    """The like-for-like form of the comparator (tools/gemm_sustained_ab.py): the four GEMMs of a layer walked over `layers`
    DISTINCT weight sets (nothing stays in the 256 MB Infinity Cache between uses), passes alternating between this repository's kernel
    with its fused RoPE / residual / SwiGLU epilogues and torch.matmul (hipBLASLt, plain store) on the SAME operands, HIP events per launch."""
    from gritlm_amd import ops
    from gritlm_amd._lib import EPI_RESIDUAL, EPI_SWIGLU
    from gritlm_amd.encoder import rope_tables
    BF, H, I, NQKV = torch.bfloat16, 4096, 14336, 6144
    g = torch.Generator(device=dev).manual_seed(0)
    mk = lambda *s: (torch.randn(s, generator=g, device=dev, dtype=torch.float32) * (0.02 if s[0] != M else 1.0)).to(BF)
    Ls = [dict(qkv=mk(NQKV, H), o=mk(H, H), gu=mk(2 * I, H), down=mk(H, I)) for _ in range(layers)]
    x, ctx, act, res = mk(M, H), mk(M, H), mk(M, I), mk(M, H)
    o_qkv, o_h = torch.empty((M, NQKV), device=dev, dtype=BF), torch.empty((M, H), device=dev, dtype=BF)
    o_act, o_gu = torch.empty((M, I), device=dev, dtype=BF), torch.empty((M, 2 * I), device=dev, dtype=BF)
    cos, sin = rope_tables(SEQ, 128, 10000.0, True, dev)
    flops = {"qkv": 2.0 * M * NQKV * H, "o_proj": 2.0 * M * H * H, "gate_up": 2.0 * M * 2 * I * H, "down": 2.0 * M * H * I}
    ev = {k: {n: [] for n in flops} for k in ("ours", "vendor")}

    def timed(kind, name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        ev[kind][name].append((e0, e1))

    def one_pass(kind):
        for L in Ls:
            if kind == "ours":
                timed(kind, "qkv", lambda: ops.gemm_nt_rope(x, L["qkv"], cos, sin, 40 * 128, S=SEQ, out=o_qkv))
                timed(kind, "o_proj", lambda: ops.gemm_nt(ctx, L["o"], out=o_h, epilogue=EPI_RESIDUAL, residual=res))
                timed(kind, "gate_up", lambda: ops.gemm_nt(x, L["gu"], out=o_act, epilogue=EPI_SWIGLU))
                timed(kind, "down", lambda: ops.gemm_nt(act, L["down"], out=o_h, epilogue=EPI_RESIDUAL, residual=res))
            else:
                timed(kind, "qkv", lambda: torch.matmul(x, L["qkv"].t(), out=o_qkv))
                timed(kind, "o_proj", lambda: torch.matmul(ctx, L["o"].t(), out=o_h))
                timed(kind, "gate_up", lambda: torch.matmul(x, L["gu"].t(), out=o_gu))
                timed(kind, "down", lambda: torch.matmul(act, L["down"].t(), out=o_h))

    one_pass("ours"); one_pass("vendor")                    # warm-up: also brings the chip to its sustained clock
    for k in ev:
        for n in ev[k]:
            ev[k][n].clear()
    for _ in range(passes):
        one_pass("ours"); one_pass("vendor")
    torch.cuda.synchronize()
    out, tot = {"layers_of_distinct_weights": layers, "passes": passes}, {}
    for k in ev:
        tf = tt = 0.0
        for n, fl in flops.items():
            ms = [p.elapsed_time(q) for p, q in ev[k][n]]
            out[f"{k}_{n}_tflops"] = fl * len(ms) / (sum(ms) * 1e-3) / 1e12
            tf += fl * len(ms); tt += sum(ms) * 1e-3
        tot[k] = out[f"{k}_flop_weighted_tflops"] = tf / tt / 1e12
    out["ours_over_vendor"] = tot["ours"] / tot["vendor"]
    del Ls, x, ctx, act, res, o_qkv, o_h, o_act, o_gu
    torch.cuda.empty_cache()
    return out


def contrastive_leg(cfg, dev, world, rank, dist, pairs=256, group=8, chunk=32, steps=1, warmup=1, ragged_pairs=32, pass1_precision="f16_stream",
                    parity_pairs=16, parity_loss_pairs=256):
    """Second headline metric: contrastive pairs/s on BASELINE configs[2] as stated -- per rank 256 queries + 2048 passages
    (1 positive + 7 negatives each) @ seq512, GradCache chunk 32 (scripts/training/train_gritlm_7b.sh:60-67; gritlm/training/run.py:93-104).
    One step = pass 1 (no grad) -> chunk-wise all-gather of the reps (N > 1) -> fused InfoNCE (similarity [W*256, W*2048] + CE + rep
    grads) -> pass 2 forward+backward per chunk -> gradient all-reduce under the last chunk's backward (N > 1) -> AdamW."""
    from gritlm_amd.training.engine import MistralTrainEngine, SyntheticBackbone
    from gritlm_amd.training.gradcache import GradCacheStep
    from gritlm_amd.training.model import DistributedContrastiveLoss, GritLMTrainModel
    bb = SyntheticBackbone(cfg, dev, seed=1)
    m = GritLMTrainModel.__new__(GritLMTrainModel)
    torch.nn.Module.__init__(m)
    m.model, m.embedding_attr, m.projection, m.normalized, m.pooling_method, m.attn = bb, None, None, True, "mean", "bbcc"
    m.emb_loss_fn = DistributedContrastiveLoss(0.02, dist is not None)
    m.train_engine = MistralTrainEngine(bb, cfg, dev)
    m.train_engine.cache_transposed_weights = True      # W^T reused by every GradCache chunk of a step (invalidated after AdamW)
    opt = torch.optim.AdamW(bb.parameters(), lr=1e-5, fused=True)
    # pass 1 (the no-grad forward that defines the representations and the loss) under the policy that meets the north-star's loss tolerance
    # at depth 32 (fp16 MFMA operands, fp16 residual stream; `parity` below holds it -- and the all-bf16 step -- against the fp32 reference)
    gc = GradCacheStep(m, chunk, precision=pass1_precision)
    gen = torch.Generator(device=dev).manual_seed(4321 + rank)
    mk = lambda n: {"input_ids": torch.randint(3, cfg.vocab_size, (n, SEQ), generator=gen, device=dev, dtype=torch.int64),
                    "attention_mask": torch.ones((n, SEQ), dtype=torch.int64, device=dev)}
    q, p = mk(pairs), mk(pairs * group)

    def step(g_=gc, q_=q, p_=p):
        loss = g_(q_, p_)
        opt.step(); opt.zero_grad(set_to_none=True)
        m.train_engine.weights_updated()
        return loss

    # PARITY first, on the leg's INITIAL weights (random init, no optimizer step yet): the timed steps below train on ONE synthetic batch,
    # which the 7B model memorises within four updates (loss 7.6 -> 0.15: a saturated softmax whose loss no longer moves with the scores),
    # so a loss comparison taken AFTER them would pass for any arithmetic; at initialisation the softmax over the 2048 passages is wide
    # open and every score counts
    parity = None
    if parity_pairs:
        try:
            pols = ("bf16",) + tuple(x for x in ("f16_stream", "f16_operands") if x == pass1_precision or (pass1_precision == "bf16" and x == "f16_stream"))
            parity = contrastive_parity(m, bb, cfg, opt, q, p, dev, chunk, group, pairs=min(parity_pairs, pairs), policies=pols,
                                        loss_pairs=min(parity_loss_pairs, pairs))
        except Exception as e:  # noqa: BLE001
            parity = {"error": repr(e)[:300]}
        gc = GradCacheStep(m, chunk, precision=pass1_precision)          # (the parity leg left the engine on its last policy)
        opt.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    for _ in range(warmup):
        step(gc)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    gc.profile = {}
    marks = [torch.cuda.Event(enable_timing=True)]
    t0 = time.perf_counter()
    marks[0].record()
    for _ in range(steps):
        loss = step(gc)
        marks.append(torch.cuda.Event(enable_timing=True)); marks[-1].record()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    step_ms = sorted(a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:]))
    if dist is not None:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    prof = {k: (v / steps if k.endswith("_ms") else v) for k, v in gc.profile_summary().items()}
    gc.profile = None
    if dist is not None and prof.get("gather_bytes_received") is not None:
        # the exchange step against xGMI (7 links x ~153 GB/s per GPU, /opt/skills/guides): bytes a rank receives per step and the time its
        # compute stream was BLOCKED on them (the rest of the transfer ran under the document tower); a lower bound of the achieved rate
        prof["xgmi_peak_gbps_per_gpu"] = 7 * 153
        ex = prof.get("exposed_gather_ms", 0.0)
        prof["exposed_gather_us"] = ex * 1e3
        prof["gather_gbps_over_exposed_time"] = (prof["gather_bytes_received"] / (ex * 1e-3) / 1e9) if ex > 0 else None
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30
    pairs_per_s = world * pairs * steps / dt
    pass1_overflow = None
    if pass1_precision != "bf16":
        from gritlm_amd import ops as _ops
        pass1_overflow = bool(_ops.f16_overflow_flag(dev))

    # ragged training batch (rank-local, outside the timed region above, smaller batch): lengths U{64..512} right-padded to 512 --
    # padded rows through every kernel (what the reference's SDPA path does) vs the packed (un-padded) training path
    ragged = None
    if ragged_pairs:
        def rag(n):
            b = mk(n)
            lens = torch.randint(64, SEQ + 1, (n,), generator=gen, device=dev)
            b["attention_mask"] = (torch.arange(SEQ, device=dev).unsqueeze(0) < lens.unsqueeze(1)).to(torch.int64)
            return b, float(lens.float().mean().item())
        (rq, lq), (rp, lp) = rag(ragged_pairs), rag(ragged_pairs * group)
        rates, losses = {}, {}
        for packed in (False, True):
            m.native_packed = packed
            loss_r = gc(rq, rp); opt.zero_grad(set_to_none=True)          # warm-up (buffers sized for this layout)
            torch.cuda.synchronize()
            t0r = time.perf_counter()
            loss_r = step(gc, rq, rp)
            torch.cuda.synchronize()
            rates[packed], losses[packed] = ragged_pairs / (time.perf_counter() - t0r), float(loss_r)
        m.native_packed = True
        ragged = {"lengths": "U{64..512} right-padded to 512", "pairs_per_step": ragged_pairs, "mean_len": (lq + group * lp) / (1 + group),
                  "pairs_per_s_per_gpu_padded_path": rates[False], "pairs_per_s_per_gpu_packed_path": rates[True],
                  "loss_padded": losses[False], "loss_packed_after_one_more_update": losses[True]}
    eng_flops = 2.0 * cfg.num_hidden_layers * (cfg.hidden_size * (6144) + 4096 * cfg.hidden_size + 3 * cfg.hidden_size * cfg.intermediate_size) \
        + 4.0 * cfg.num_hidden_layers * SEQ * 4096
    alg_flops_per_pair = 3.0 * eng_flops * SEQ * (1 + group)          # fwd + bwd = 3 x forward; recompute passes are overhead
    return {"metric": "contrastive pairs/sec @ seq512", "value": pairs_per_s, "unit": "pairs/s", "n_gpus": world, "steps": steps,
            "warmup": warmup, "ms_per_step": dt / steps * 1e3, "ms_per_step_median": step_ms[len(step_ms) // 2], "ms_per_step_min": step_ms[0],
            "pairs_per_s_per_gpu_best_step": pairs / step_ms[0] * 1e3,
            "pairs_per_gpu_per_step": pairs, "group_size": group, "gradcache_chunk": chunk,
            "gradcache_pass1_rows_per_call": gc.pass1_chunk_size,      # pass 1 keeps nothing: several chunks per call, same bits
            "global_batch": world * pairs, "loss": float(loss), "peak_hbm_gib": peak_gb,
            "pass1_precision": pass1_precision, "pass1_fp16_overflow_flag": pass1_overflow, "parity": parity,
            "includes": "GradCache pass 1 + rep all-gather + InfoNCE + pass 2 fwd/bwd + grad all-reduce + AdamW",
            "config": f"BASELINE configs[2]: {pairs} (q, pos, 7 neg) per GPU @ seq512, chunk {chunk}, tau 0.02, mean pooling, cross-device negatives"
                      + ("" if pairs == 256 and chunk == 32 else "  [REDUCED from 256 pairs / chunk 32]"),
            "mfma_roofline_frac": pairs_per_s / world * alg_flops_per_pair / (MFMA_BF16_PEAK_TFLOPS * 1e12),
            "per_step_ms": prof,
            **({"ragged_batch": ragged} if ragged is not None else {})}


def contrastive_parity(m, bb, cfg, opt, q, p, dev, chunk, group, pairs=16, tau=0.02, policies=("bf16", "f16_stream"), loss_pairs=64):
    """Full-depth parity datum of BASELINE configs[2] (VERDICT r05 #1a): a sub-batch of `pairs` (query, 1 + 7 passages) units of the timed
    batch -- on the leg's OWN 32-layer weights, as initialised (the caller runs this BEFORE the training steps) -- through (1) the engine's GradCache step (pass 1 under each
    pass-1 policy, InfoNCE on HIP, pass 2 forward + backward in bf16; no optimizer step) and (2) the reference's training forward
    (gritlm/training/model.py:134-222: encode -> pool -> normalise -> scores / tau -> CrossEntropy(arange * group)) + backward in FP32 on the
    stock transformers module loaded from the same weights (oracle/torch_reference.py::encode_with_grad, gradient checkpointing as the
    reference trains).  Reported per policy: max 1 - cos of the pass-1 representations, |loss - fp32 loss| against the north-star's 1e-3, and
    the parameter gradients against the fp32 gradients (relative l2 and cosine per weight matrix: median / worst over the 7 x 32 matrices).
    `loss_pairs` (> pairs): the LOSS datum again on a larger sub-batch, forward only on both sides (engine: pass-1 representations + the
    HIP InfoNCE kernel; reference: fp32 module + torch cross entropy) -- with 1 / tau = 50 one score moves the loss of n queries by
    ~50 sqrt(2 (1 - cos)) / (64 sqrt(n)), so the number of queries the loss averages over matters for the 1e-3 (configs[2] has 256 per GPU)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch_reference as TR
    from gritlm_amd.training.gradcache import GradCacheStep
    from gritlm_amd.training.model import DistributedContrastiveLoss
    n_q, n_p = pairs, pairs * group
    qs = {k: v[:n_q].contiguous() for k, v in q.items()}
    ps = {k: v[:n_p].contiguous() for k, v in p.items()}
    names = [n for n, t in bb.named_parameters() if t.dim() == 2 and "embed" not in n]
    out = {"what": f"{pairs} (query, 1 + {group - 1} passages) units of the timed batch x {SEQ} tokens, the leg's own {cfg.num_hidden_layers}-layer weights as "
                   "initialised (before any optimizer step: the softmax over the passages is wide open): engine GradCache step (pass 1 under the named policy, pass 2 + backward in bf16, no optimizer step) vs the reference's "
                   "training forward + backward in FP32 on the stock module (gradient checkpointing), same weights, same rows",
           "pairs": pairs, "tokens": (n_q + n_p) * SEQ, "temperature": tau}
    # ---- engine side, per pass-1 policy (local loss: the sub-batch is this rank's own rows)
    keep_loss, eng_side = m.emb_loss_fn, {}
    m.emb_loss_fn = DistributedContrastiveLoss(tau, False)
    try:
        for pol in policies:
            opt.zero_grad(set_to_none=True)
            gcp = GradCacheStep(m, chunk, precision=pol)
            loss = gcp(dict(qs), dict(ps), sync=False)
            torch.cuda.synchronize()
            flag = False
            if pol != "bf16":
                from gritlm_amd import ops
                flag = bool(ops.f16_overflow_flag(dev))
            eng_side[pol] = {"loss": float(loss.item()), "q": gcp.last_reps[0].double().clone(), "p": gcp.last_reps[1].double().clone(),
                             "grads": {n: dict(bb.named_parameters())[n].grad.detach().clone() for n in names}, "fp16_overflow_flag": flag}
        opt.zero_grad(set_to_none=True)
    finally:
        m.emb_loss_fn = keep_loss
    m.train_engine._tbuf.clear(); m.train_engine._wT.clear(); m.train_engine._w16.clear(); m.train_engine._ws16.clear()
    torch.cuda.empty_cache()
    # ---- reference side: fp32, autograd
    t0 = time.perf_counter()
    cfgd = dict(TR.SHAPE_7B, num_hidden_layers=cfg.num_hidden_layers)
    ref = TR.build_model(cfgd, torch.float32, dev, state_dict={k: v.detach() for k, v in bb.state_dict().items()})
    ref.train()
    doc_chunk = 16
    enc = lambda b: torch.cat([TR.encode_with_grad(ref, b["input_ids"][i:i + doc_chunk], b["attention_mask"][i:i + doc_chunk])
                               for i in range(0, b["input_ids"].shape[0], doc_chunk)])
    rq, rp = enc(qs), enc(ps)
    ref_loss = TR.contrastive_loss(rq, rp, tau)
    ref_loss.backward()
    torch.cuda.synchronize()
    rgrads = dict(ref.named_parameters())
    out["reference_fp32"] = {"loss": float(ref_loss.item()), "seconds": time.perf_counter() - t0}
    omc = lambda a, b: float((1.0 - torch.nn.functional.cosine_similarity(a, b.double(), dim=1)).max())
    for pol, d in eng_side.items():
        rel, cosg = [], []
        for n in names:
            g, r = d["grads"][n].double(), rgrads[n].grad.double()
            rel.append(float((g - r).norm() / (r.norm() + 1e-30)))
            cosg.append(float((g * r).sum() / (g.norm() * r.norm() + 1e-30)))
        rel_t, cos_t = torch.tensor(rel), torch.tensor(cosg)
        err = abs(d["loss"] - out["reference_fp32"]["loss"])
        out[pol] = {"pass1_precision": pol, "loss": d["loss"], "loss_abs_err": err, "loss_within_1e-3": bool(err < 1e-3),
                    "reps_max_one_minus_cos": max(omc(d["q"], rq.detach()), omc(d["p"], rp.detach())),
                    "grad_rel_l2_median": float(rel_t.median()), "grad_rel_l2_worst": float(rel_t.max()),
                    "grad_cos_median": float(cos_t.median()), "grad_cos_min": float(cos_t.min()), "weight_matrices_compared": len(names),
                    "fp16_overflow_flag": d["fp16_overflow_flag"]}
    del rgrads, rq, rp
    ref.zero_grad(set_to_none=True)
    torch.cuda.empty_cache()
    # ---- the loss datum on `loss_pairs` pairs, forward only
    if loss_pairs and loss_pairs > pairs:
        from gritlm_amd import ops
        t1 = time.perf_counter()
        nq2, np2 = min(loss_pairs, q["input_ids"].shape[0]), min(loss_pairs, q["input_ids"].shape[0]) * group
        ql = {k: v[:nq2].contiguous() for k, v in q.items()}
        pl = {k: v[:np2].contiguous() for k, v in p.items()}
        ref.eval()
        with torch.no_grad():
            renc = lambda b: torch.cat([TR.encode(ref, b["input_ids"][i:i + 32], b["attention_mask"][i:i + 32]) for i in range(0, b["input_ids"].shape[0], 32)])
            rq2, rp2 = renc(ql), renc(pl)
            l_ref = float(TR.contrastive_loss(rq2.double(), rp2.double(), tau))
            big = {"pairs": nq2, "tokens": (nq2 + np2) * SEQ, "reference_fp32_loss": l_ref}
            for pol in policies:
                m.train_engine.set_nograd_precision(pol)
                eenc = lambda b: torch.cat([m.encode({k: v[i:i + 128] for k, v in b.items()}) for i in range(0, b["input_ids"].shape[0], 128)])
                eq, ep = eenc(ql), eenc(pl)
                l_eng = float(ops.infonce(eq.float().contiguous(), ep.float().contiguous(), tau, want_grad=False)[0].item())
                big[pol] = {"loss": l_eng, "loss_abs_err": abs(l_eng - l_ref), "loss_within_1e-3": bool(abs(l_eng - l_ref) < 1e-3),
                            "reps_max_one_minus_cos": max(omc(eq.double(), rq2), omc(ep.double(), rp2)),
                            "fp16_overflow_flag": bool(ops.f16_overflow_flag(dev)) if pol != "bf16" else False}
                del eq, ep
        big["seconds"] = time.perf_counter() - t1
        out["loss_on_larger_sub_batch"] = big
        del rq2, rp2
    lsrc = out.get("loss_on_larger_sub_batch") or out
    best = next((pol for pol in policies if pol != "bf16" and lsrc[pol]["loss_within_1e-3"] and out[pol]["loss_abs_err"] < 2e-3
                 and max(out[pol]["reps_max_one_minus_cos"], lsrc[pol]["reps_max_one_minus_cos"]) < 1e-4
                 and not out[pol]["fp16_overflow_flag"] and not lsrc[pol]["fp16_overflow_flag"]), None)
    out["north_star_policy"] = best
    out["north_star_met"] = best is not None
    # the leg's headline parity number: |loss - fp32 loss| of the north-star policy on the largest sub-batch measured
    out["loss_abs_err"] = lsrc[best]["loss_abs_err"] if best else lsrc[policies[-1]]["loss_abs_err"]
    out["loss_abs_err_pairs"] = lsrc.get("pairs", pairs)
    del ref, eng_side
    torch.cuda.empty_cache()
    return out


def compact_summary(line: dict) -> dict:
    """<= 1500 characters, appended as the LAST key of the JSON line (VERDICT r05 #2b: the driver keeps the last 2000 characters): every
    headline number of the round -- both metrics, the roofline fractions, the parity data per leg, the same-run comparators."""
    def g(d, *ks):
        for k in ks:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return d

    def r(x, n=4):
        if isinstance(x, float):
            return float(f"{x:.{n}g}")
        return x
    ns, c, mx, rag = line.get("north_star_policy") or {}, line.get("contrastive") or {}, line.get("mixtral_8x7b_seq2048") or {}, line.get("rag_doc_caching") or {}
    cp = c.get("parity") or {}
    cpb = cp.get(cp.get("north_star_policy") or "") or {}
    mp = mx.get("parity") or {}
    s = {"encode_docs_per_s": r(line.get("value")), "n_gpus": line.get("n_gpus"), "gemm_frac": r(g(line, "roofline", "frac")), "mfu": r(line.get("model_flops_utilisation")),
         "default_bf16_1mcos": r(g(line, "parity_full_depth", "vs_reference_fp32_same_weights", "engine_bf16_residual_default", "max_one_minus_cos")),
         "ns_policy": ns.get("precision"), "ns_docs_per_s": r(ns.get("docs_per_s")), "ns_1mcos": r(ns.get("max_one_minus_cos_timed_batch")),
         "ns_timed_steps": ns.get("timed_steps"), "north_star_met": line.get("north_star_met"),
         "gemm_over_vendor": [r(line.get("gemm_over_vendor_in_model")), r(line.get("gemm_over_vendor_sustained"))],
         "vs_rocm_torch": r(line.get("speedup_vs_rocm_torch")),
         "contrastive": {"pairs_per_s": r(c.get("value")), "frac": r(c.get("mfma_roofline_frac")), "steps": c.get("steps"), "pass1": c.get("pass1_precision"),
                         "loss_abs_err": r(cp.get("loss_abs_err")), "loss_err_pairs": cp.get("loss_abs_err_pairs"),
                         "loss_abs_err_bf16": r(g(cp, "loss_on_larger_sub_batch", "bf16", "loss_abs_err") or g(cp, "bf16", "loss_abs_err")),
                         "reps_1mcos": r(cpb.get("reps_max_one_minus_cos")), "grad_cos_min": r(cpb.get("grad_cos_min")),
                         "grad_rel_l2_median": r(cpb.get("grad_rel_l2_median")), "north_star_met": cp.get("north_star_met"), "err": (c.get("error") or cp.get("error"))},
         "mixtral": {"docs_per_s": r(mx.get("value")), "grouped_gemm_frac": r(g(mx, "roofline", "frac")), "f16_docs_per_s": r(g(mx, "north_star_policy", "docs_per_s")),
                     "f16_e2e_1mcos": r(g(mp, "policies", "f16_operands", "end_to_end", "max_one_minus_cos")),
                     "f16_routing_agree_min": r(min([v["routing_agree"] for v in (g(mp, "policies", "f16_operands", "teacher_forced_per_layer") or {}).values()] or [0.0])),
                     "bf16_e2e_1mcos": r(g(mp, "policies", "bf16", "end_to_end", "max_one_minus_cos")),
                     "ref_bf16_dataflow_e2e_1mcos": r(g(mp, "reference_dataflow_in_bf16_end_to_end", "max_one_minus_cos")),
                     "decode_frac": r(g(mx, "native_decode", "frac_of_weight_streaming_roofline")),
                     "north_star_met": mp.get("north_star_met"), "err": mx.get("error")},
         "rag": {"decode_frac": r(rag.get("decode_frac_of_weight_streaming_roofline")), "encode_frac": r(rag.get("encode_mfma_roofline_frac")),
                 "decode_logits_1mcos_bf16_level": r(g(rag, "parity", "max_one_minus_cos")),
                 "f16_decode_logits_1mcos": r(g(rag, "parity", "f16_flow", "f16_stream", "max_one_minus_cos")),
                 "f16_decode_frac": r(g(rag, "parity", "f16_flow", "f16_stream", "decode_frac_of_weight_streaming_roofline")),
                 "f16_flow_north_star_met": g(rag, "parity", "f16_flow", "north_star_met"),
                 "latency16_native_s": r(g(rag, "native_decode", "latency_16_new_tokens", "native_s")),
                 "latency16_hf_s": r(g(rag, "native_decode", "latency_16_new_tokens", "hugging_face_generate_s")),
                 "encode_get_cache_1mcos": {k: r(g(rag, "parity", "encode_get_cache_by_policy", k, "max_one_minus_cos")) for k in ("bf16", "f16_stream", "f16_operands")},
                 "err": rag.get("error")}}

    def prune(d):
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                v = prune(v)
            if v is None or v == {} or (isinstance(v, list) and all(x is None for x in v)) or (k.endswith("routing_agree_min") and v == 0.0):
                continue
            out[k] = v
        return out
    s = prune(s)
    while len(json.dumps(s)) > 1500 and s:                 # never longer than the window: drop the least important tail entries
        s.pop(next(reversed(s)))
    return s


def secondary_leg(script: str, argv: list, timeout_s: float, keep: tuple) -> dict:
    """BASELINE configs[3] / configs[4] as time-boxed secondary legs (VERDICT r03 #2c): the tool runs in a CHILD process (its own HIP context
    and allocator: 108 / 174 GB of weights + KV never meet the parent's caches; a hang or an out-of-memory there cannot cost the primary
    line), one JSON line back, the fields in `keep` copied into the bench line."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "tools", script)] + [str(x) for x in argv]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return {"error": f"{script} exceeded its {timeout_s:.0f} s box", "cmd": " ".join(cmd[1:])}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": f"{script} rc={r.returncode}: {r.stderr[-300:]}", "cmd": " ".join(cmd[1:])}
    d = json.loads(lines[-1])
    out = {k: d[k] for k in keep if k in d}
    out["cmd"] = "python " + " ".join(os.path.relpath(c, ROOT) if c.startswith(ROOT) else c for c in cmd[1:])
    out["leg_wall_s"] = time.perf_counter() - t0
    return out


def self_launch(n: int) -> int:
    """``python bench.py --gpus N`` with N > 1 and no launcher environment: start the N ranks ourselves, exactly as the driver's
    documented command does (``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P
    bench.py <same flags>``), pass their output through (rank 0 prints the one JSON line) and return their exit code."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, len(os.sched_getaffinity(0)) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"bench.py: --gpus {n} without a launcher environment -> starting {n} ranks: {' '.join(cmd[1:8])} ...", file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


class DryEncoder:
    """--dry-cpu ONLY (no GPU in the build container): a tiny stock ``transformers.MistralModel`` on the host stands in for the HIP
    engine so that everything AROUND the kernels -- self-launch, process group, barriers, max-over-ranks timing, the cross-rank
    GradCache step, the deadline guard, the one JSON line -- can be executed with 2 gloo ranks by tests/test_bench_cli.py.  The line
    it produces carries "INVALID"; no number in it is a measurement."""

    def __init__(self, layers: int, seed: int = 0):
        from transformers import MistralConfig, MistralModel
        hc = MistralConfig(vocab_size=512, hidden_size=64, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=2,
                           num_key_value_heads=1, head_dim=32, max_position_embeddings=512, sliding_window=None, pad_token_id=0,
                           bos_token_id=1, eos_token_id=2, tie_word_embeddings=False)
        hc.use_cache = False
        hc._attn_implementation = "sdpa"
        torch.manual_seed(seed)
        self.model = MistralModel(hc).eval()
        self.config = hc

    @torch.no_grad()
    def encode(self, ids, mask):
        h = self.model(input_ids=ids, attention_mask=mask, is_causal=False)[0]
        m = mask.unsqueeze(-1).float()
        return torch.nn.functional.normalize((h.float() * m).sum(1) / m.sum(1), dim=-1)


def dry_contrastive_leg(enc: "DryEncoder", world, rank, dist, pairs, group, chunk, seq):
    """--dry-cpu: the cross-rank GradCache step (chunk-wise rep gathers, loss on the gathered batch with local-shard-only gradients,
    gradient averaging) on the Hugging Face CPU path of GritLMTrainModel, gloo collectives."""
    from gritlm_amd.training.gradcache import GradCacheStep
    from gritlm_amd.training.model import DistributedContrastiveLoss, GritLMTrainModel
    m = GritLMTrainModel.__new__(GritLMTrainModel)
    torch.nn.Module.__init__(m)
    m.model, m.embedding_attr, m.projection, m.normalized, m.pooling_method, m.attn = enc.model.train(), None, None, True, "mean", "bbcc"
    m.emb_loss_fn = DistributedContrastiveLoss(0.02, dist is not None)
    m.train_engine = None
    gc = GradCacheStep(m, chunk)
    gc.profile = {}
    gen = torch.Generator().manual_seed(4321 + rank)
    mk = lambda n: {"input_ids": torch.randint(3, enc.config.vocab_size, (n, seq), generator=gen),
                    "attention_mask": torch.ones((n, seq), dtype=torch.int64)}
    q, p = mk(pairs), mk(pairs * group)
    t0 = time.perf_counter()
    loss = gc(q, p)
    if dist is not None:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    gnorm = torch.stack([x.grad.float().norm() for x in enc.model.parameters() if x.grad is not None]).norm().reshape(1).double()
    spread = gnorm.clone()
    if dist is not None:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        lo, hi = gnorm.clone(), gnorm.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        spread = hi - lo
    prof = gc.profile_summary()
    return {"metric": "contrastive pairs/sec (DRY RUN)", "value": world * pairs / float(t.item()), "unit": "pairs/s", "n_gpus": world,
            "pairs_per_gpu_per_step": pairs, "group_size": group, "gradcache_chunk": chunk, "global_batch": world * pairs,
            "loss": float(loss), "grad_norm_after_averaging": float(gnorm.item()),
            "grad_norm_spread_over_ranks": float(spread.item()) if dist is not None else 0.0,
            "per_step_ms": {k: v for k, v in prof.items() if not k.startswith("_")}}


def claim_stdout():
    """The contract is ONE JSON line on stdout.  Libraries write there too -- RCCL prints a five-line version banner through C stdio when
    its first communicator comes up, and it reaches the pipe at exit, i.e. AFTER the JSON line (the round-2 forced-distributed run shows
    it: profiles/r02_bench_forced_one_rank_rccl.json) -- so the process's fd 1 is pointed at stderr for everybody else and the line is
    written to the saved descriptor.  Returns emit(str)."""
    sys.stdout.flush()
    real = os.dup(1)
    os.dup2(2, 1)

    def emit(text: str):
        os.write(real, (text + "\n").encode())
    return emit


def deadline_guard(budget_s: float, late_line, emit=None):
    """Arms a daemon thread: unless the returned Event is set within ``budget_s`` seconds the thread prints ``late_line()`` (if it
    returns a string) and ends the PROCESS with exit code 0 (``os._exit``: the main thread may be parked inside a collective that will
    never complete).  tests/test_bench_guard.py exercises it in a subprocess."""
    import threading
    done = threading.Event()

    def _watch():
        if not done.wait(budget_s):
            out = late_line()
            if out is not None:
                (emit or (lambda t: print(t, flush=True)))(out)
            os._exit(0)
    threading.Thread(target=_watch, daemon=True).start()
    return done


# Numeric bounds on 1 - cos of the pooled embeddings against the reference's arithmetic in FP32 after all 32 layers (VERDICT r03 #1c: constants,
# not ratios to a yardstick).  Anchors: profiles/r04_depth_parity.json and tests/golden/encoder_7b-depth32.npz (DESIGN section 2 "depth").
#   fixture model (the same layer 32 times, uniform +-0.035 weights; the reference's OWN bf16 run of it is 4.6e-4 .. 6.0e-4 from its fp32 run):
FULL_DEPTH_BOUND_BF16_RESIDUAL = 7.0e-4          # measured 4.3e-4 .. 5.4e-4 (default precision policy: the reference's bf16 rounding points)
FULL_DEPTH_BOUND_FP32_RESIDUAL = 4.5e-4          # measured 2.9e-4 .. 3.4e-4 (opt-in fp32 residual stream)
#   bench model (32 DISTINCT N(0, 0.02) layers, the first 32 documents of the timed 256 x 512 batch):
BENCH_BOUND_BF16_RESIDUAL = 1.0e-3               # measured max 7.1e-4 / mean 6.4e-4 over 32 documents
BENCH_BOUND_FP32_RESIDUAL = 6.5e-4               # measured max 4.5e-4 / mean 4.1e-4
#   precision="f16_operands" (round 5: fp32 residual stream + fp16 MFMA operands) is held to the NORTH-STAR's own tolerance on both models;
#   the CPU emulation of the policy predicts 4e-6 at depth 32 (profiles/r05_precision_budget.json)
FULL_DEPTH_BOUND_F16_OPERANDS = 1.0e-4
BENCH_BOUND_F16_OPERANDS = 1.0e-4
NORTH_STAR_NOTE = ("north_star asks 1 - cos < 1e-4 against the reference's fp32 encode().  With bf16 MFMA operands no implementation reaches it at depth "
                   "32 on these synthetic models (the error grows linearly with depth: independent 8-bit-mantissa roundings of x, q|k|v, P, ctx, act "
                   "in every layer; the reference's own bf16 run is further from its fp32 run than the engine is, profiles/r04_depth_parity.json). "
                   "precision='f16_operands' (fp32 residual stream, every MFMA operand in fp16 -- same MFMA rate, 3 more mantissa bits, overflow "
                   "flagged) is the policy held to 1e-4 here; the per-operand error budget it was derived from is profiles/r05_precision_budget.json")


def parity_same_weights(eng, hf_sd, ids, mask, emb_default, dev, layers, docs=32, chunk=8, time_steps=3, north_star_steps=None):
    """`encode()` at configs[1], not a synthetic side case (VERDICT r03 #1a): the engine's embeddings of the first `docs` documents of the TIMED
    batch against the reference-equivalent module (oracle/torch_reference.py: the stock transformers module driven with the reference's mask
    rule -- no mask for an all-valid batch, modeling_mistral_gritlm.py:1017-1020 --, pinned bit for bit on reference-generated fixtures) in
    FP32 on this GPU, loaded from the ENGINE'S OWN weights (gritlm/gritlm.py:129-158, scripts/modeling_mistral_gritlm.py:936-1096).  Both
    precision policies of the engine are held to numeric bounds; the stock module in bf16 on this GPU is reported, it bounds nothing."""
    import torch_reference as TR
    from gritlm_amd import ops
    cfgd = dict(TR.SHAPE_7B, num_hidden_layers=layers)
    n = min(docs, ids.shape[0])
    si, sm = ids[:n].contiguous(), mask[:n].contiguous()

    def omc(a, b):
        d = 1.0 - torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1)
        return {"max_one_minus_cos": float(d.max()), "mean_one_minus_cos": float(d.mean())}

    def stock(dtype, rule):
        m = TR.build_model(cfgd, dtype, dev, state_dict=hf_sd)
        e = torch.cat([TR.encode(m, si[i:i + chunk], sm[i:i + chunk], mask_rule=rule) for i in range(0, n, chunk)]).float()
        del m
        torch.cuda.empty_cache()
        return e

    ref = stock(torch.float32, "reference")
    e_stock = stock(torch.bfloat16, "reference")
    out = {"what": f"the first {n} documents of the timed batch ({ids.shape[0]} x {ids.shape[1]}, the bench's own {layers}-layer weights): HIP engine vs "
                   "the reference-equivalent module in FP32 on this GPU loaded from the engine's weights (oracle/torch_reference.py, reference "
                   "mask rule); 1 - cos per document",
           "docs": n, "layers": layers}
    d = omc(emb_default[:n], ref)
    out["engine_bf16_residual_default"] = {**d, "bound": BENCH_BOUND_BF16_RESIDUAL, "within_bound": d["max_one_minus_cos"] < BENCH_BOUND_BF16_RESIDUAL}
    def opt_in(policy, n_steps=None):
        """``n_steps``: timed EXACTLY like the headline (VERDICT r05 #2a): one warm-up pass, then n_steps steps with a HIP event at every step
        boundary on the launch stream, bracketed by synchronize(); rate = docs x steps / wall time of the bracket, per-step median / min from
        the events."""
        n_steps = n_steps or time_steps
        eng.set_precision(policy)
        try:
            e = ops.pool_norm(eng.forward(si, sm, borrow=True), sm, "mean", True).float().clone()
            d = omc(e, ref)
            rate, extra = None, {}
            if n_steps:
                ops.pool_norm(eng.forward(ids, mask, borrow=True), mask, "mean", True)
                torch.cuda.synchronize()
                tm = ops.KernelTimer()                 # the same per-launch HIP events as the primary timed region
                ops.set_timer(tm)
                marks = []
                t0 = time.perf_counter()
                for _ in range(n_steps):
                    marks.append(torch.cuda.Event(enable_timing=True)); marks[-1].record()
                    ops.pool_norm(eng.forward(ids, mask, borrow=True), mask, "mean", True)
                marks.append(torch.cuda.Event(enable_timing=True)); marks[-1].record()
                torch.cuda.synchronize()
                rate = ids.shape[0] * n_steps / (time.perf_counter() - t0)
                ops.set_timer(None)
                sm_ = sorted(a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:]))
                extra["timed_steps"] = n_steps
                extra["per_step"] = {"median_ms": sm_[len(sm_) // 2], "min_ms": sm_[0], "max_ms": sm_[-1], "mean_ms": 1e3 * ids.shape[0] / rate}
                extra["kernels"] = {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 3), "tflops": v["work"] / (v["total_ms"] * 1e-3) / 1e12,
                                        **({"by_shape_tflops": {t: round(x["work"] / (x["total_ms"] * 1e-3) / 1e12, 1) for t, x in v["by_tag"].items()}}
                                           if "by_tag" in v else {})} for k, v in tm.summary().items()}
            if policy in ("f16_operands", "f16_stream"):
                st = eng.f16_weight_stats or {}
                extra.update({"fp16_overflow_flag": bool(ops.f16_overflow_flag(eng.device)),
                              "weights_subnormal_in_fp16_frac": st.get("subnormal", 0) / max(st.get("total", 1), 1)})
        finally:
            eng.set_precision("bf16")
            eng._ws.clear()
        return d, rate, extra

    d, rate, extra = opt_in("fp32_residual")
    out["engine_fp32_residual_opt_in"] = {**d, "bound": BENCH_BOUND_FP32_RESIDUAL, "within_bound": d["max_one_minus_cos"] < BENCH_BOUND_FP32_RESIDUAL,
                                          "docs_per_s": rate, **extra, "how": "GritLM(..., precision='fp32_residual') / engine.set_precision('fp32_residual')"}
    d, rate, extra = opt_in("f16_operands", north_star_steps)
    out["engine_f16_operands_opt_in"] = {**d, "bound": BENCH_BOUND_F16_OPERANDS,
                                         "within_bound": d["max_one_minus_cos"] < BENCH_BOUND_F16_OPERANDS and not extra.get("fp16_overflow_flag", True),
                                         "docs_per_s": rate, **extra, "how": "GritLM(..., precision='f16_operands') / engine.set_precision('f16_operands'): "
                                         "fp32 residual stream, fp16 MFMA operands (x, q|k|v, P, ctx, act, weights), one rounding each"}
    out["stock_module_bf16_this_gpu"] = {**omc(e_stock, ref), "what": "stock transformers module, bf16, sdpa, the reference's mask rule, same weights, "
                                         "through PyTorch-ROCm: what the reference's Python computes on this GPU (reported; bounds nothing)"}
    out["engine_default_vs_stock_module_bf16"] = omc(emb_default[:n], e_stock)
    d, rate, extra = opt_in("f16_stream", north_star_steps)
    out["engine_f16_stream_opt_in"] = {**d, "bound": BENCH_BOUND_F16_OPERANDS,
                                       "within_bound": d["max_one_minus_cos"] < BENCH_BOUND_F16_OPERANDS and not extra.get("fp16_overflow_flag", True),
                                       "docs_per_s": rate, **extra, "how": "GritLM(..., precision='f16_stream'): f16_operands with the residual stream "
                                       "itself in fp16 (16-bit residual epilogues and norms; an activation of the stream beyond 65504 raises)"}
    out["within_bound"] = bool(out["engine_bf16_residual_default"]["within_bound"] and out["engine_fp32_residual_opt_in"]["within_bound"]
                               and out["engine_f16_operands_opt_in"]["within_bound"] and out["engine_f16_stream_opt_in"]["within_bound"])
    out["north_star_met"] = bool(out["engine_f16_operands_opt_in"]["max_one_minus_cos"] < 1e-4 and not out["engine_f16_operands_opt_in"].get("fp16_overflow_flag", True))
    return out


def full_depth_parity(dev):
    """32-layer datum on the FIXTURE model (the model of tests/golden/encoder_7b-depth32.npz, which the reference itself ran): the HIP engine
    on the SAME weights and token ids the ``cpu_baseline_numpy_oracle`` leg pushes through all 32 fp32 layers (1 doc x 512 tokens, 7B
    layer shape).  Numeric bound (FULL_DEPTH_BOUND_BF16_RESIDUAL); the GPU test `full_depth_parity_32_layers` holds the same engine to
    the reference-generated embeddings of that fixture."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    from gritlm_amd import ops
    from gritlm_amd.encoder import EncoderConfig, MistralEncoderEngine
    cfg, w, ids, mask = oracle_full_depth_case()
    t0 = time.perf_counter()
    ref = oracle_full_depth_run(cfg, w, ids, mask)                                  # fp32 numpy oracle, all 32 layers
    dt = time.perf_counter() - t0
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    eng = MistralEncoderEngine.from_state_dict(EncoderConfig.from_dict(cfg), sd, dev)
    tid, tm = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    cosd = lambda a, b: float(np.max(1.0 - np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))))
    hip = cosd(ops.pool_norm(eng.forward(tid, tm, borrow=True), tm, "mean", True).float().cpu().numpy(), ref)
    eng.set_precision("fp32_residual")
    hip32 = cosd(ops.pool_norm(eng.forward(tid, tm, borrow=True), tm, "mean", True).float().cpu().numpy(), ref)
    eng.set_precision("f16_operands")
    hip16 = cosd(ops.pool_norm(eng.forward(tid, tm, borrow=True), tm, "mean", True).float().cpu().numpy(), ref)
    ovf16 = bool(ops.f16_overflow_flag(eng.device))
    eng.set_precision("f16_stream")
    hip16s = cosd(ops.pool_norm(eng.forward(tid, tm, borrow=True), tm, "mean", True).float().cpu().numpy(), ref)
    ovf16 = ovf16 or bool(ops.f16_overflow_flag(eng.device))
    del eng
    torch.cuda.empty_cache()
    return {"what": "1 doc x 512 tokens through all 32 layers at the 7B layer shape (the repeated-layer model of tests/golden/encoder_7b-depth32.npz), "
                    "HIP engine vs the fp32 numpy oracle on identical bf16-representable weights",
            "one_minus_cos_vs_fp32_oracle": hip, "bound": FULL_DEPTH_BOUND_BF16_RESIDUAL,
            "fp32_residual_opt_in_one_minus_cos_vs_fp32_oracle": hip32, "fp32_residual_bound": FULL_DEPTH_BOUND_FP32_RESIDUAL,
            "f16_operands_opt_in_one_minus_cos_vs_fp32_oracle": hip16, "f16_operands_bound": FULL_DEPTH_BOUND_F16_OPERANDS,
            "f16_stream_opt_in_one_minus_cos_vs_fp32_oracle": hip16s,
            "f16_operands_overflow_flag": ovf16, "north_star_met": bool(hip16 < 1e-4 and hip16s < 1e-4 and not ovf16),
            "within_bound": bool(hip < FULL_DEPTH_BOUND_BF16_RESIDUAL and hip32 < FULL_DEPTH_BOUND_FP32_RESIDUAL
                                 and hip16 < FULL_DEPTH_BOUND_F16_OPERANDS and hip16s < FULL_DEPTH_BOUND_F16_OPERANDS and not ovf16)}, {
            "value": ids.shape[0] / dt, "unit": "docs/s", "cores": len(os.sched_getaffinity(0)), "kind": "port",
            "sample": f"numpy oracle (oracle/gritlm_oracle.py, fp32 OpenBLAS), {ids.shape[0]} doc(s) x {ids.shape[1]} tok through all "
                      f"{cfg['num_hidden_layers']} layers, {dt:.2f} s", "seconds": dt}


def oracle_full_depth_case(sample_docs=1, seq=512, layers=32):
    """Weights / ids of the full-depth oracle leg: 7B layer shape, small vocabulary, the SAME bf16-representable arrays for every layer
    (host memory stays at one layer; timing and error accumulation do not care)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import synth
    cfg = dict(synth.CONFIGS["7b"]); cfg["num_hidden_layers"] = layers; cfg["vocab_size"] = 2048
    rng = np.random.default_rng(0)
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    d = H // cfg["num_attention_heads"]; nkv = cfg["num_key_value_heads"]
    lin = lambda o, i: synth._bf16_round((rng.random((o, i), dtype=np.float32) - 0.5) * 0.07)
    nrm = lambda: synth._bf16_round(1.0 + 0.1 * rng.standard_normal(H, dtype=np.float32))
    w = {"embed_tokens.weight": lin(cfg["vocab_size"], H), "norm.weight": nrm()}
    base = {"self_attn.q_proj.weight": lin(H, H), "self_attn.k_proj.weight": lin(nkv * d, H),
            "self_attn.v_proj.weight": lin(nkv * d, H), "self_attn.o_proj.weight": lin(H, H),
            "mlp.gate_proj.weight": lin(I, H), "mlp.up_proj.weight": lin(I, H), "mlp.down_proj.weight": lin(H, I),
            "input_layernorm.weight": nrm(), "post_attention_layernorm.weight": nrm()}
    for li in range(layers):
        for k, v in base.items():
            w[f"layers.{li}.{k}"] = v
    ids, mask = synth.make_batch(cfg, sample_docs, seq, seed=1234)
    return cfg, w, ids, mask


def oracle_full_depth_run(cfg, w, ids, mask):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import gritlm_oracle as O
    O.encode_core(w, cfg, ids[:1, :64], mask[:1, :64], "mean", True, acc_dtype=np.float32)   # warm BLAS threads
    return O.encode_core(w, cfg, ids, mask, "mean", True, acc_dtype=np.float32)


def main():
    global DOCS, SEQ
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=32, help="debug only; anything but 32 marks the line invalid")
    ap.add_argument("--full", action="store_true", help="also run every comparator, baseline, parity and secondary leg (the --no-* flags "
                    "below select among them); without it only the headline steps run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the embeddings of the last timed step to DIR/embeddings.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-contrastive", action="store_true", help="skip the contrastive pairs/s leg")
    ap.add_argument("--no-ragged", action="store_true", help="skip the ragged-batch (padded vs packed) leg")
    ap.add_argument("--pairs", type=int, default=256, help="contrastive pairs per GPU per step (BASELINE configs[2]: 256)")
    ap.add_argument("--chunk", type=int, default=32, help="GradCache chunk size (BASELINE configs[2]: 32)")
    ap.add_argument("--contrastive-steps", type=int, default=1, help="timed contrastive steps (after one warm-up step); ~52 s each at configs[2] "
                    "(1 keeps --full within ten minutes; earlier lines used 3)")
    ap.add_argument("--pass1-precision", default="f16_stream", choices=("bf16", "f16_stream", "f16_operands"),
                    help="precision policy of GradCache pass 1 in the contrastive leg (the pass that defines the loss); default: the policy that "
                         "meets the north-star's |loss - fp32 loss| < 1e-3 at depth 32")
    ap.add_argument("--contrastive-parity-pairs", type=int, default=16, help="pairs of the timed batch re-run through the fp32 reference "
                    "(forward + backward) for the contrastive leg's parity object; 0 = skip")
    ap.add_argument("--contrastive-parity-loss-pairs", type=int, default=64, help="pairs for the forward-only loss datum of that object "
                    "(default 64: ~40 s of fp32 reference, keeps --full within ten minutes; 256 = the whole per-GPU batch of configs[2], ~2.5 minutes)")
    ap.add_argument("--no-torch-baseline", action="store_true", help="skip the stock PyTorch-ROCm encode on this GPU")
    ap.add_argument("--no-mixtral", action="store_true", help="skip the BASELINE configs[3] leg (Mixtral-8x7B shape, 64 x seq2048)")
    ap.add_argument("--no-rag", action="store_true", help="skip the BASELINE configs[4] leg (512 passages x seq2048 with KV + 128 new tokens)")
    ap.add_argument("--dry-cpu", action="store_true",
                    help="plumbing check without a GPU: gloo ranks, a tiny Hugging Face model on the host instead of the HIP engine; "
                         "the line is marked INVALID (tests/test_bench_cli.py)")
    args = ap.parse_args()
    dry = args.dry_cpu
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    forced = bool(os.environ.get("GRIT_BENCH_FORCE_DIST"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not forced:
        if not dry and torch.cuda.device_count() < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but only {torch.cuda.device_count()} GPU(s) are visible", file=sys.stderr)
            sys.exit(2)
        sys.exit(self_launch(args.gpus))
    emit = claim_stdout()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(args.gpus, 1) and not forced:
        print(f"bench.py: launched with WORLD_SIZE={world} but --gpus {args.gpus}; reporting n_gpus = {world}", file=sys.stderr)
    if dry:
        dev = torch.device("cpu")
        DOCS, SEQ = 8, 16
        torch.set_num_threads(2)
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    dist = None
    # GRIT_BENCH_FORCE_DIST=1 (single process): run the N > 1 code path -- RCCL process group, barriers, max-over-ranks reduction,
    # cross-device loss, chunk-wise gathers, overlapped gradient all-reduce, deadline guard -- on a ONE-rank group, the only form of it
    # a one-GPU box can execute
    multi = world > 1 or forced
    backend = "gloo" if dry else "nccl"                                      # "nccl" == RCCL on ROCm
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        import datetime
        kw = {} if dry else {"device_id": dev}
        dist.init_process_group(backend, timeout=datetime.timedelta(minutes=10), rank=rank, world_size=world, **kw)

    sync = (lambda: None) if dry else torch.cuda.synchronize
    if dry:
        eng = DryEncoder(args.layers)
        ops = timer = None
        cfg = eng.config
    else:
        from gritlm_amd import ops
        from gritlm_amd.encoder import EncoderConfig, MistralEncoderEngine
        cfg = EncoderConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=args.layers, num_attention_heads=32,
                            num_key_value_heads=8, vocab_size=32000, rms_norm_eps=1e-5, rope_theta=10000.0)
        eng = MistralEncoderEngine.random_init(cfg, dev, seed=0)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    ids = torch.randint(3, cfg.vocab_size, (DOCS, SEQ), generator=gen, device=dev, dtype=torch.int64)
    mask = torch.ones((DOCS, SEQ), dtype=torch.int64, device=dev)

    def step():
        if dry:
            return eng.encode(ids, mask)
        h = eng.forward(ids, mask, borrow=True)
        return ops.pool_norm(h, mask, "mean", True)

    for _ in range(args.warmup):
        emb = step()
    if not dry:
        timer = ops.KernelTimer()
    sync()
    if dist is not None:
        dist.barrier()
    sync()
    if not dry:
        ops.set_timer(timer)
    marks = []                          # one HIP event per step boundary on the launch stream (no sync inside the timed region)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if not dry:
            marks.append(torch.cuda.Event(enable_timing=True)); marks[-1].record()
        emb = step()
    if not dry:
        marks.append(torch.cuda.Event(enable_timing=True)); marks[-1].record()
    sync()
    if dist is not None:
        dist.barrier()
    sync()
    dt = time.perf_counter() - t0
    if not dry:
        ops.set_timer(None)
    step_ms = sorted(a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:]))
    assert torch.isfinite(emb).all(), "non-finite embeddings"
    flops_per_token = 0.0 if dry else eng.flops_per_token(SEQ)

    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    if dist is not None:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt_max = float(t.item())
    if args.dump_outputs:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        name = "embeddings.npy" if rank == 0 else f"embeddings_rank{rank}.npy"
        np.save(os.path.join(args.dump_outputs, name), emb.float().cpu().numpy())

    # ---- ragged batch (SURVEY §8d "C2 padded variant"): lengths ~ U{64..512}, right-padded; padded vs packed (un-padded) path
    ragged = None
    if args.full and not args.no_ragged and not dry:
        g2 = torch.Generator(device=dev).manual_seed(99 + rank)
        lens = torch.randint(64, SEQ + 1, (DOCS,), generator=g2, device=dev)
        lens[0] = SEQ
        rmask = (torch.arange(SEQ, device=dev).unsqueeze(0) < lens.unsqueeze(1)).to(torch.int64)

        def timed(packed):
            for _ in range(1):
                eng.encode_pooled(ids, rmask, "mean", True, packed=packed)
            torch.cuda.synchronize()
            t0r = time.perf_counter()
            for _ in range(2):
                e = eng.encode_pooled(ids, rmask, "mean", True, packed=packed)
            torch.cuda.synchronize()
            return 2 * DOCS / (time.perf_counter() - t0r), e

        dps_pad, e_pad = timed(False)
        dps_pack, e_pack = timed(True)
        ragged = {"lengths": "U{64..512} right-padded to 512", "mean_len": float(lens.float().mean().item()),
                  "docs_per_s_padded_path": dps_pad, "docs_per_s_packed_path": dps_pack,
                  "bit_identical": bool(torch.equal(e_pad, e_pack))}

    baselines = args.full and not multi and not dry and not args.no_torch_baseline
    hf_sd = eng.to_hf_state_dict() if baselines else None           # views of the engine's weights: the stock module is loaded from them
    emb_engine = emb.float().clone()
    if not dry:
        eng._ws.clear()
    del emb
    if not baselines and not dry:
        del eng
    if not dry:
        torch.cuda.empty_cache()
    vendor = None
    if baselines:
        try:
            vendor = vendor_gemm_comparator(dev)
        except Exception as e:  # noqa: BLE001
            vendor = {"error": repr(e)[:200]}
    torch_baseline = parity_sw = vendor_sustained = None
    if baselines:
        try:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import torch_reference as TR
            torch_baseline = TR.time_gpu(dev, DOCS, SEQ, args.layers, state_dict=hf_sd, ids=ids, mask=mask)
            e_hf = torch_baseline.pop("embeddings")
            cos = torch.nn.functional.cosine_similarity(e_hf.float(), emb_engine, dim=1)
            torch_baseline["engine_vs_stock_hf_same_weights_bf16"] = {
                "what": f"the {DOCS} embeddings of the timed batch: HIP engine vs the stock Hugging Face module loaded from the engine's own "
                        f"weights, bf16 on both sides, {args.layers} layers", "max_one_minus_cos": float((1 - cos).max().item()),
                "mean_one_minus_cos": float((1 - cos).mean().item())}
            del e_hf
        except Exception as e:  # noqa: BLE001
            torch_baseline = {"error": repr(e)[:300]}
        try:
            parity_sw = parity_same_weights(eng, hf_sd, ids, mask, emb_engine, dev, args.layers, north_star_steps=args.steps)
        except Exception as e:  # noqa: BLE001
            parity_sw = {"error": repr(e)[:300]}
        try:
            vendor_sustained = vendor_gemm_sustained(dev)
        except Exception as e:  # noqa: BLE001
            vendor_sustained = {"error": repr(e)[:200]}
        del hf_sd, eng
        torch.cuda.empty_cache()
    line = None
    if rank == 0:
        docs_per_s = world * DOCS * args.steps / dt_max
        flops_per_doc = flops_per_token * SEQ
        line = {
            "metric": "encoded docs/sec @ seq512", "value": docs_per_s, "unit": "docs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            **({"per_step": {"what": "HIP events at the step boundaries on the launch stream of rank 0 (SURVEY 8d: median and min next to "
                                     "the mean the contract's `value` is computed from)", "median_ms": step_ms[len(step_ms) // 2],
                             "min_ms": step_ms[0], "max_ms": step_ms[-1], "docs_per_s_median_step": DOCS / step_ms[len(step_ms) // 2] * 1e3,
                             "docs_per_s_best_step": DOCS / step_ms[0] * 1e3}} if step_ms else {}),
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "GritLM-7B (Mistral-7B shape, 32L, random-init) bf16 bidirectional encode, batch 256 x seq512, "
                                   "mean pooling + L2 normalise, per GPU", "docs_per_step_per_gpu": DOCS, "seq_len": SEQ,
                       "layers": args.layers, "parallelism": f"replicas x{world} (no data-path collective)"},
        }
        if not dry:
            ks = timer.summary()
            g = ks["gemm_bf16_nt"]
            achieved = g["work"] / (g["total_ms"] * 1e-3) / 1e12           # TFLOP/s over all launches == avg flops / avg duration
            shapes = {t: {"launches": v["launches"], "avg_ms": v["total_ms"] / v["launches"], "tflops": v["work"] / (v["total_ms"] * 1e-3) / 1e12}
                      for t, v in g.get("by_tag", {}).items()}
            att = [v for t, v in g.get("by_tag", {}).items() if t.startswith("N=6144,K=4096") or t.startswith("N=4096,K=4096")]
            att_tf = sum(v["work"] for v in att) / (sum(v["total_ms"] for v in att) * 1e-3) / 1e12 if att else None
            traffic, traffic_note = measured_traffic()
            line["model_flops_utilisation"] = docs_per_s / world * flops_per_doc / (MFMA_BF16_PEAK_TFLOPS * 1e12)
            line["roofline"] = {"bound": "mfma", "kernel": "gemm_bf16_nt_k", "achieved": achieved, "peak": MFMA_BF16_PEAK_TFLOPS,
                                "unit": "TFLOP/s", "frac": achieved / MFMA_BF16_PEAK_TFLOPS, "traffic": traffic, **traffic_note,
                                "launches": g["launches"], "avg_launch_ms": g["avg_ms"],
                                "avg_flops_per_launch": g["work"] / g["launches"], "by_shape": shapes,
                                "attention_gemms_qkv_oproj": None if att_tf is None else
                                {"achieved": att_tf, "frac": att_tf / MFMA_BF16_PEAK_TFLOPS}}
            line["kernels"] = {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 3),
                                   "tflops": v["work"] / (v["total_ms"] * 1e-3) / 1e12} for k, v in ks.items()}
    # N > 1: the contrastive leg is the only part with data-path collectives.  If a rank dies or stalls inside it the others would sit in a
    # collective until the RCCL watchdog aborts the job and the primary line would be lost: a deadline thread on every rank prints the
    # primary line (with the leg marked as timed out) and exits the process cleanly instead.
    guard, emitted = None, []
    run_contrastive = args.full and not args.no_contrastive
    if multi and run_contrastive:
        def _late_line():
            if rank != 0 or emitted:
                return None
            if ragged is not None:
                line["ragged_batch"] = ragged
            line["contrastive"] = {"error": f"contrastive leg exceeded its deadline on {world} ranks; primary line emitted by the deadline guard"}
            line["collectives"] = {"backend": backend, "ranks": world, "encode_data_path_collectives": 0}
            return json.dumps(line)
        guard = deadline_guard(float(os.environ.get("GRIT_BENCH_CONTRASTIVE_DEADLINE_S", "900")), _late_line, emit)
    contrastive = None
    if run_contrastive:
        try:
            if dry:
                contrastive = dry_contrastive_leg(eng, world, rank, dist, pairs=args.pairs, group=2, chunk=args.chunk, seq=SEQ)
            else:
                torch.cuda.reset_peak_memory_stats()
                contrastive = contrastive_leg(cfg, dev, world, rank, dist, pairs=args.pairs, chunk=args.chunk, steps=args.contrastive_steps,
                                              ragged_pairs=0 if args.no_ragged else 32, pass1_precision=args.pass1_precision,
                                              parity_pairs=args.contrastive_parity_pairs, parity_loss_pairs=args.contrastive_parity_loss_pairs)
        except Exception as e:  # noqa: BLE001  -- never lose the primary metric line to the secondary leg
            contrastive = {"error": repr(e)[:300]}

    if rank == 0:
        if vendor is not None:
            line["roofline"]["vendor_gemm_tflops_same_shapes_no_epilogue"] = vendor
            vs = {"what": "this kernel (epilogues fused) / hipBLASLt behind torch.matmul (plain store), same GPU, same process"}
            if "flop_weighted" in vendor:
                vs["in_model_over_5_launch_comparator"] = line["roofline"]["achieved"] / vendor["flop_weighted"]
            if vendor_sustained is not None:
                vs["sustained_interleaved"] = vendor_sustained
            line["roofline"]["vs_vendor_same_run"] = vs
            # the box-independent ratios again at the TOP level (a reader of the first-level keys sees them: VERDICT r04 #8)
            line["gemm_over_vendor_in_model"] = vs.get("in_model_over_5_launch_comparator")
            line["gemm_over_vendor_sustained"] = (vendor_sustained or {}).get("ours_over_vendor")
        if ragged is not None:
            line["ragged_batch"] = ragged
        if contrastive is not None:
            line["contrastive"] = contrastive
        if dry:
            line["INVALID"] = "--dry-cpu: plumbing check on the host (tiny Hugging Face model, gloo); no number here is a measurement"
        elif args.layers != 32:
            line["INVALID"] = "debug run with --layers != 32"
        if torch_baseline is not None:
            line["rocm_torch_baseline"] = torch_baseline
            if "value" in torch_baseline:
                line["speedup_vs_rocm_torch"] = docs_per_s / torch_baseline["value"]
        if multi:
            line["collectives"] = {"backend": dist.get_backend(), "library": "gloo (dry run)" if dry else
                                   "RCCL (torch.distributed 'nccl' backend on ROCm)",
                                   "ranks": dist.get_world_size(), "encode_data_path_collectives": 0}
        if args.full and not multi and not dry and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline()
            try:
                fixture_datum, line["cpu_baseline_numpy_oracle"] = full_depth_parity(dev)
            except Exception as e:  # noqa: BLE001
                fixture_datum = {"error": repr(e)[:300]}
            line["parity_full_depth"] = {
                "vs_reference_fp32_same_weights": parity_sw, "fixture_model_vs_fp32_numpy_oracle": fixture_datum,
                "depth_curve": "profiles/r04_depth_parity.json (1 - cos at depth 1/2/4/8/16/32, both bf16-operand policies, stock bf16 under both mask "
                               "rules); profiles/r05_precision_budget.json (per-operand error budget, emulated)",
                "north_star": NORTH_STAR_NOTE,
                "within_bound": bool((parity_sw or {}).get("within_bound")) and bool(fixture_datum.get("within_bound")),
                "north_star_met": bool((parity_sw or {}).get("north_star_met")) and bool(fixture_datum.get("north_star_met"))}
            # top-level copies (VERDICT r04 #8 / ADVICE r04): does every policy hold its numeric bound, and does the f16_operands policy meet
            # the north-star's 1 - cos < 1e-4 on the timed batch AND on the reference-run fixture model
            line["parity_within_bound"] = line["parity_full_depth"]["within_bound"]
            line["north_star_met"] = line["parity_full_depth"]["north_star_met"]
            # the policies that meet 1 - cos < 1e-4 on the timed batch, and the fastest of them
            cands = {k: (parity_sw or {}).get(f"engine_{k}_opt_in") or {} for k in ("f16_operands", "f16_stream")}
            ok_c = {k: v for k, v in cands.items() if v.get("within_bound") and (v.get("max_one_minus_cos") or 1.0) < 1e-4}
            best = max(ok_c, key=lambda k: ok_c[k].get("docs_per_s") or 0.0) if ok_c else "f16_operands"
            line["north_star_policy"] = {"precision": best, "max_one_minus_cos_timed_batch": cands[best].get("max_one_minus_cos"),
                                         "docs_per_s": cands[best].get("docs_per_s"), "timed_steps": cands[best].get("timed_steps"),
                                         "per_step": cands[best].get("per_step"),
                                         "how_timed": "like the headline: one warm-up pass, then --steps steps, a HIP event per step boundary on the launch "
                                                      "stream, synchronize() on both sides",
                                         "docs_per_s_over_default": (cands[best].get("docs_per_s") or 0.0) / docs_per_s,
                                         "all": {k: {"max_one_minus_cos": v.get("max_one_minus_cos"), "docs_per_s": v.get("docs_per_s"),
                                                     "docs_per_s_over_default": (v.get("docs_per_s") or 0.0) / docs_per_s} for k, v in cands.items()}}
        if args.full and not multi and not dry:
            import gc as _gc
            _gc.collect()
            torch.cuda.empty_cache()
            if not args.no_mixtral:
                line["mixtral_8x7b_seq2048"] = secondary_leg(
                    "mixtral_bench.py", ["--docs", 64, "--seq", 2048, "--steps", 3, "--warmup", 1], 600,
                    ("metric", "value", "unit", "ms_per_step", "tokens_per_s", "config", "roofline", "model_flops_utilisation", "hbm_allocated_gb",
                     "expert_load_max_over_mean", "finite", "kernels", "parity", "north_star_policy", "native_decode"))
            if not args.no_rag:
                line["rag_doc_caching"] = secondary_leg(
                    "rag_cache_bench.py", ["--passages", 512, "--seq", 2048, "--new-tokens", 128, "--queries", 4], 600,
                    ("metric", "passages", "seq", "encode_s", "passages_per_s", "encode_tokens_per_s", "encode_mfma_roofline_frac", "kv_cache_gb",
                     "generate_s_per_query", "decode_tokens_per_s", "decode_path", "native_decode", "decode_frac_of_weight_streaming_roofline", "parity",
                     "hbm_allocated_gb"))
        if not dry:
            line["summary"] = compact_summary(line)          # LAST key: the tail of the line the driver keeps holds the round's numbers
        emit(json.dumps(line))
        emitted.append(True)
    if dist is not None:
        dist.destroy_process_group()          # still under the deadline guard: a rank that never arrives cannot wedge the job
    if guard is not None:
        guard.set()


if __name__ == "__main__":
    main()
