#!/usr/bin/env python3
"""Headline benchmark: image-text samples/s, forward+backward(+AdamW), Llama-3.1-8B + CLIP-ViT-L/14, bf16, one
process per GPU (BASELINE.json metric; config = configs[2] "8B+ViT-L/14 bf16 full fwd+bwd (AdamW)", per-GPU micro-batch
4 x seq 2048, 1 image/sample, FULL training mode, synthetic data, random-init weights).

    python bench.py --gpus N --steps 5 --warmup 2          (N > 1: starts the N ranks itself as child processes)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    python bench.py --gpus 2 --dry-run                     (CPU/gloo rehearsal of the launcher only; never a measurement)
    python bench.py --full                                 (also the roofline, the all-rows form and the CPU baseline)
    python bench.py --dump-outputs DIR                     (also write what the last timed step computed to DIR/*.npy)

The job's rank count must equal --gpus or the run exits non-zero.

Prints ONE JSON line on rank 0.  `value` = whole-job samples/s with inputs resident in HBM; `ms_per_step` = wall time of
one of the --steps timed steps.  A plain run sets up, warms up, times the steps and prints the line; everything else runs
only with --full, after the timed steps: `roofline` = bf16 GEMM kernel (the dominant kernel: 96 % of the step's FLOPs)
measured live with HIP events on the launch stream in one extra instrumented step; `config.all_rows_form` = the same step
with every row through lm_head; `cpu_baseline` = the CPU oracle (oracle/ref_cpu.py) timed on the host cores on a bounded
slice of the same workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

METRIC_MODELS = {      # the model pair named in the metric string (BASELINE.json's metric is quoted on the first)
    "llama31_8b_vitl14_s2048_b4": "Llama-3.1-8B+ViT-L/14",
    "llama32_1b_vitb32_s2048_b4": "Llama-3.2-1B+ViT-B/32",
    "llama31_8b_vitl14_s4096_b2_4img": "Llama-3.1-8B+ViT-L/14",
    "qwen2_7b_siglip_so400m_s2048_b4": "Qwen2-7B+SigLIP-so400m",
}
WORKLOADS = {
    # name: (llm preset, clip preset, per-GPU batch, seq, images/sample)
    "llama31_8b_vitl14_s2048_b4": ("meta-llama/Llama-3.1-8B-Instruct", "openai/clip-vit-large-patch14", 4, 2048, 1),
    "llama32_1b_vitb32_s2048_b4": ("meta-llama/Llama-3.2-1B-Instruct", "openai/clip-vit-base-patch32", 4, 2048, 1),
    "llama31_8b_vitl14_s4096_b2_4img": ("meta-llama/Llama-3.1-8B-Instruct", "openai/clip-vit-large-patch14", 2, 4096, 4),
    # BASELINE config 5: alternate embedder / LLM through the modality plug-in (meditron_siglip) and the Qwen2 preset
    "qwen2_7b_siglip_so400m_s2048_b4": ("Qwen/Qwen2-7B-Instruct", "google/siglip-so400m-patch14-384", 4, 2048, 1),
}
PEAK_BF16_TFLOPS = 2500.0        # dense bf16 MFMA peak of gfx950 (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def flops_per_sample(llm, vis, S, n_img, vocab, hidden_proj, lm_head_rows=None):
    """Algorithmic forward FLOPs per sample: 2*params*tokens for linears, 4*T^2*d*L attention (causal
    halved).  fwd+bwd (FULL) = 3x.  lm_head_rows: rows per sample that go through lm_head and through the last layer's o_proj + MLP
    (default: all S, as HF computes; the Trainer runs them on the labelled rows only -- EXECUTED flops count those)."""
    H, I, L = llm["hidden_size"], llm["intermediate_size"], llm["num_hidden_layers"]
    hd = llm["head_dim"]
    qo, kv = llm["num_attention_heads"] * hd, llm["num_key_value_heads"] * hd
    lin = L * (H * (qo + 2 * kv) + qo * H + 3 * H * I)
    rows = S if lm_head_rows is None else lm_head_rows       # ... and o_proj + MLP of the LAST layer (DecoderLayer.forward `rows`)
    f = 2.0 * lin * S - 2.0 * (qo * H + 3 * H * I) * (S - rows) + 2.0 * H * vocab * rows + 0.5 * 4.0 * S * S * qo * L
    Dv, Iv, Lv = vis["hidden_size"], vis["intermediate_size"], vis["num_hidden_layers"]
    P = (vis["image_size"] // vis["patch_size"]) ** 2
    T = P + (0 if vis.get("kind") == "siglip" else 1)       # SigLIP has no CLS token
    vlin = Lv * (4 * Dv * Dv + 2 * Dv * Iv)
    fv = 2.0 * vlin * T + 4.0 * T * T * Dv * Lv + 2.0 * P * 3 * vis["patch_size"] ** 2 * Dv
    fp = 2.0 * P * (Dv * Dv + Dv * hidden_proj + hidden_proj * hidden_proj)
    return f + n_img * (fv + fp)


def synthetic_batch(B, S, n_img, P, vocab, ids_special, seed, device, img_size, collator_form=False):
    """ids ~ U{0..127999}; image spans laid out text-image-text with start/end delimiters; labels = ids
    with -100 on modality spans and on the first 25 % of tokens; all-ones mask; N(0,1) pixels.
    collator_form: exactly what DataCollatorForMultimodal hands to the trainer -- HOST tensors, an all-ones
    `attention_mask`, and `stacked["image"]` as a LIST of per-image [3,H,W] host tensors (data_loader.py:133-143)."""
    g = torch.Generator().manual_seed(seed)
    img_start, img_end, attach = ids_special
    ids = torch.randint(0, min(vocab, 128000), (B, S), generator=g)
    labels = ids.clone()
    bi, tr, pix = [], [], []
    gap = (S - n_img * (P + 2)) // (n_img + 1)
    for b in range(B):
        for k in range(n_img):
            s = gap * (k + 1) + k * (P + 2) + 1
            ids[b, s - 1], ids[b, s + P] = img_start, img_end
            ids[b, s:s + P] = attach
            labels[b, s - 1:s + P + 1] = -100
            bi += [b] * P
            tr += list(range(s, s + P))
            pix.append(torch.randn(3, img_size, img_size, generator=g))
        labels[b, : S // 4] = -100
    mask = torch.ones(B, S, dtype=torch.long)
    pos = torch.arange(S).unsqueeze(0).expand(B, S).contiguous()
    if collator_form:
        return dict(input_ids=ids, labels=labels, attention_mask=mask, position_ids=pos,
                    processed_multimodal_inputs={"batch_idx": {"image": torch.tensor(bi)}, "token_range": {"image": torch.tensor(tr)},
                                                 "stacked": {"image": pix}}), mask
    pixels = torch.stack(pix).to(device)
    return dict(input_ids=ids.to(device), labels=labels.to(device), attention_mask=None, position_ids=pos.to(device),
                processed_multimodal_inputs={"batch_idx": {"image": torch.tensor(bi, device=device)},
                                             "token_range": {"image": torch.tensor(tr, device=device)},
                                             "stacked": {"image": pixels}}), mask


def measure_gemm_roofline(trainer, batch):
    """One extra (untimed) step with a HIP event pair around every bf16 GEMM launch on the launch stream."""
    from multimeditron_amd import kernels as K
    rec = []
    orig = K.gemm
    from multimeditron_amd._lib import lib as _lib
    import ctypes as _ct

    def last_kernel():                               # 10 = the 4-wave 256x256 kernel (mm_get_option "gemm_last_kernel")
        v = _ct.c_int(-1)
        _lib().mm_get_option(b"gemm_last_kernel", _ct.byref(v))
        return v.value

    def timed(layout, a, b, M, N, Kd, *args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(layout, a, b, M, N, Kd, *args, **kw)
        e1.record()
        rec.append((e0, e1, 2.0 * M * N * Kd, (layout, M, N, Kd), last_kernel()))
        return out

    orig_sf, orig_sb = K.gemm_swiglu_fwd, K.gemm_swiglu_bwd

    def timed_sf(x2d, wgu, I):                       # the fused gate|up GEMM (+SwiGLU epilogue): M x 2I x K
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_sf(x2d, wgu, I)
        e1.record()
        if out is not None:
            M, Kd = x2d.shape
            rec.append((e0, e1, 2.0 * M * 2 * I * Kd, ("NT+swiglu", M, 2 * I, Kd), last_kernel()))
        return out

    def timed_sb(dy2d, wd, gu, I):                   # down_proj dgrad (+SwiGLU backward epilogue): M x I x H
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_sb(dy2d, wd, gu, I)
        e1.record()
        if out is not None:
            M, H = dy2d.shape
            rec.append((e0, e1, 2.0 * M * I * H, ("NN+swiglu_bwd", M, I, H), last_kernel()))
        return out

    orig_act = K.linear_act_fwd

    def timed_act(x2d, w, bias, act, residual=None):  # Linear + GELU in one launch (ViT fc1, projector): mm_gemm_act_fwd
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_act(x2d, w, bias, act, residual)
        e1.record()
        if out is not None:
            M, Kd = x2d.shape
            rec.append((e0, e1, 2.0 * M * w.shape[0] * Kd, ("NT+act", M, w.shape[0], Kd), last_kernel()))
        return out

    orig_rope = K.gemm_rope_fwd

    def timed_rope(x2d, w, bias, rope_cols, D, cos, sin):      # the q|k|v projection with RoPE in its epilogue: mm_gemm_rope_fwd
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_rope(x2d, w, bias, rope_cols, D, cos, sin)
        e1.record()
        if out is not None:
            M, Kd = x2d.shape
            rec.append((e0, e1, 2.0 * M * w.shape[0] * Kd, ("NT+rope", M, w.shape[0], Kd), last_kernel()))
        return out

    K.gemm, K.gemm_swiglu_fwd, K.gemm_swiglu_bwd, K.linear_act_fwd, K.gemm_rope_fwd = timed, timed_sf, timed_sb, timed_act, timed_rope
    try:
        trainer.training_step(batch)
        torch.cuda.synchronize()
    finally:
        K.gemm, K.gemm_swiglu_fwd, K.gemm_swiglu_bwd, K.linear_act_fwd, K.gemm_rope_fwd = orig, orig_sf, orig_sb, orig_act, orig_rope
    def summary(rs):
        tot_ms = sum(e0.elapsed_time(e1) for e0, e1, _, _, _ in rs)
        tot_fl = sum(f for _, _, f, _, _ in rs)
        alg_bytes = sum(2.0 * (M * Kd + N * Kd + M * N) for _, _, _, (_, M, N, Kd), _ in rs)      # A, B, C once, bf16
        return dict(launches=len(rs), avg_launch_ms=tot_ms / max(1, len(rs)), flops_per_launch=tot_fl / max(1, len(rs)),
                    achieved_tflops=tot_fl / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else 0.0, gemm_ms_per_step=tot_ms,
                    algorithmic_bytes_per_launch=alg_bytes / max(1, len(rs)), flops=tot_fl)

    # the dominant kernel = the 4-wave 256x256 kernel; "every bf16 GEMM launch" (rounds 1-3's figure: there all tiles were ONE kernel
    # template) stays beside it -- the ViT's small-tile launches are 0.6 % of the flops and run stretched under AdamW / the deferred wgrads
    w4 = summary([r_ for r_ in rec if r_[4] == 10])
    allg = summary(rec)
    w4["all"] = allg
    w4["flops_share"] = w4["flops"] / allg["flops"] if allg["flops"] else 0.0
    return w4


def kernel_source_sha():
    """sha256 over the sources of the kernel `roofline` describes (the GEMM: csrc/mm_gemm.hip, csrc/mm_common.h and the generator of the 4-wave kernel's K loop, csrc/gen_gemm_w4.py): identifies
    the code a PMC pass was taken on (.git does not travel to the GPU box, so a commit id cannot be checked there).  A change to
    that kernel voids the recorded traffic; a change to an unrelated kernel or a new entry point in the ABI header does not."""
    import hashlib
    h = hashlib.sha256()
    for fn in (os.path.join(ROOT, "multimeditron_amd", "csrc", "mm_gemm.hip"), os.path.join(ROOT, "multimeditron_amd", "csrc", "mm_common.h"),
               os.path.join(ROOT, "multimeditron_amd", "csrc", "gen_gemm_w4.py")):
        h.update(open(fn, "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic():
    """HBM bytes per GEMM launch from the PMC passes of this same command (tools/profile_round.sh -> tools/publish_profile.py ->
    profiles/rNN_pmc_traffic.json, the newest round first): counters cannot be collected from inside the timed process, so
    `traffic` is the figure of those separate rocprofv3 --pmc runs.  The file records the kernel-source hash it was measured on
    (written on the GPU box by tools/pmc_summary.py, never by hand); a figure taken on DIFFERENT kernels is not printed
    (traffic = null, with the reason)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")), reverse=True)
    if not files:
        return None, "no profiles/rNN_pmc_traffic.json"
    sha, why = kernel_source_sha(), None
    for path in files:
        try:
            with open(path) as f:
                d = json.load(f)
        except Exception:
            continue
        if d.get("kernel_source_sha") == sha:
            d["file"] = "profiles/" + os.path.basename(path)
            return d, None
        why = why or (f"profiles/{os.path.basename(path)} was measured on other kernel sources ({d.get('kernel_source_sha')}, now {sha}): "
                      "re-run tools/profile_round.sh")
    return None, why


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def host_cores():
    """CPUs this process may run on: the affinity mask, cut down to the cgroup CPU quota when there is one."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for quota_f, period_f in (("/sys/fs/cgroup/cpu.max", None), ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us")):
        try:
            if period_f is None:
                q, per = open(quota_f).read().split()[:2]
            else:
                q, per = open(quota_f).read().strip(), open(period_f).read().strip()
            if q not in ("max", "-1") and int(q) > 0 and int(per) > 0:
                n = max(1, min(n, -(-int(q) // int(per))))
            break
        except (OSError, ValueError):
            continue
    return n


def best_cpu_threads(limit):
    """Thread count for the CPU baseline: a box may show more CPUs than it lets a process use (the GPU boxes of this pool show
    256 and schedule about 16), and torch's bf16 matmul with 256 threads on such a box ran 25x SLOWER than with 16.  So the
    candidates {limit, 128, 64, 32, 16} are timed on one 4096^3 bf16 matmul each and the fastest is used and reported."""
    a = torch.randn(4096, 4096).to(torch.bfloat16)
    b = torch.randn(4096, 4096).to(torch.bfloat16)
    best, best_t = limit, float("inf")
    for n in sorted({min(limit, c) for c in (limit, 128, 64, 32, 16)}):
        torch.set_num_threads(n)
        a @ b
        t0 = time.perf_counter()
        a @ b
        dt = time.perf_counter() - t0
        if dt < best_t:
            best, best_t = n, dt
    return best


def _cpu_oracle_fwd_bwd(llm_s, vis_s, hidden, B, S, vocab):
    """One CPU-oracle model of the given shape: random bf16 weights, the SURVEY 8d synthetic batch, fwd+bwd run TWICE -- the first
    pass is an untimed warm-up (allocator, thread pool, oneDNN primitive caches), the second is the measurement.  Returns
    (seconds of the second pass, algorithmic fwd+bwd flops of one pass)."""
    from oracle import ref_cpu as R
    g = torch.Generator().manual_seed(7)
    dt = torch.bfloat16
    w = {}

    def mk(name, *shape, std=0.02):
        w[name] = (torch.randn(*shape, generator=g) * std).to(dt).requires_grad_(True)

    H, I, hd, L = llm_s["hidden_size"], llm_s["intermediate_size"], llm_s["head_dim"], llm_s["num_hidden_layers"]
    qo, kv = llm_s["num_attention_heads"] * hd, llm_s["num_key_value_heads"] * hd
    mk("model.model.embed_tokens.weight", vocab, H)
    mk("model.lm_head.weight", vocab, H)
    w["model.model.norm.weight"] = torch.ones(H, dtype=dt, requires_grad=True)
    for i in range(L):
        p = f"model.model.layers.{i}."
        mk(p + "self_attn.q_proj.weight", qo, H); mk(p + "self_attn.k_proj.weight", kv, H); mk(p + "self_attn.v_proj.weight", kv, H)
        mk(p + "self_attn.o_proj.weight", H, qo); mk(p + "mlp.gate_proj.weight", I, H); mk(p + "mlp.up_proj.weight", I, H)
        mk(p + "mlp.down_proj.weight", H, I)
        w[p + "input_layernorm.weight"] = torch.ones(H, dtype=dt, requires_grad=True)
        w[p + "post_attention_layernorm.weight"] = torch.ones(H, dtype=dt, requires_grad=True)
    Dv, Iv, ps = vis_s["hidden_size"], vis_s["intermediate_size"], vis_s["patch_size"]
    P = (vis_s["image_size"] // ps) ** 2
    vp = R.VIS_PREFIX
    mk(vp + "embeddings.patch_embedding.weight", Dv, 3, ps, ps); mk(vp + "embeddings.class_embedding", Dv)
    mk(vp + "embeddings.position_embedding.weight", P + 1, Dv)
    for n in ("pre_layrnorm",):
        w[vp + n + ".weight"] = torch.ones(Dv, dtype=dt, requires_grad=True); w[vp + n + ".bias"] = torch.zeros(Dv, dtype=dt, requires_grad=True)
    for i in range(vis_s["num_hidden_layers"]):
        p = f"{vp}encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            w[p + n + ".weight"] = torch.ones(Dv, dtype=dt, requires_grad=True); w[p + n + ".bias"] = torch.zeros(Dv, dtype=dt, requires_grad=True)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            mk(p + f"self_attn.{n}.weight", Dv, Dv); mk(p + f"self_attn.{n}.bias", Dv)
        mk(p + "mlp.fc1.weight", Iv, Dv); mk(p + "mlp.fc1.bias", Iv); mk(p + "mlp.fc2.weight", Dv, Iv); mk(p + "mlp.fc2.bias", Dv)
    pp = R.PROJ_PREFIX
    mk(pp + "0.weight", Dv, Dv); mk(pp + "0.bias", Dv); mk(pp + "2.weight", hidden, Dv); mk(pp + "2.bias", hidden)
    mk(pp + "4.weight", hidden, hidden); mk(pp + "4.bias", hidden)
    b, _ = synthetic_batch(B, S, 1, P, vocab, (vocab - 2, vocab - 1, 128002), 11, "cpu", vis_s["image_size"])
    b["attention_mask"] = torch.ones(B, S, dtype=torch.long)
    pm = b["processed_multimodal_inputs"]
    pm["stacked"]["image"] = [x.to(dt) for x in pm["stacked"]["image"]]
    meta = {"vision": vis_s, "llm": llm_s, "eos_token_idx": 0}
    fl = 3.0 * B * flops_per_sample(llm_s, vis_s, S, 1, vocab, hidden)
    dtm = None
    for timed in (False, True):
        for t in w.values():
            t.grad = None
        t0 = time.perf_counter()
        _, loss = R.multimodal_forward(w, b, meta)
        loss.backward()
        dtm = time.perf_counter() - t0
    return dtm, fl


def cpu_baseline(llm, vis, hidden, workload, budget_layers=8, S=1024, B=2):
    """The CPU oracle (torch CPU ops, the restatement of the reference's HF path), fwd+bwd in bf16 (the reference trains under
    torch.set_default_dtype(bfloat16)), in the two bounded forms SURVEY 8d allows on a host without the RAM for the 8B optimiser:
    (a) a `budget_layers`-layer slice of the workload's own decoder + ViT + projector + full lm_head, converted to samples/s of the
        full workload by algorithmic FLOPs (the reported `value`);
    (b) the WHOLE 1B-shaped model (Llama-3.2-1B + CLIP-ViT-B/32, every layer), fwd+bwd, as its own samples/s of THAT model and as a
        FLOP-scaled equivalent of the workload.  Each is run twice; the second pass is timed."""
    from multimeditron_amd.model.presets import resolve_llm_config, resolve_vision_config
    visible = host_cores()                    # every core this process may run on ...
    cores = best_cpu_threads(visible)         # ... and the thread count that is actually fastest there; both are in the line
    torch.set_num_threads(cores)
    vocab = 128258
    llm_s = dict(llm, num_hidden_layers=budget_layers)
    vis_s = dict(vis, num_hidden_layers=budget_layers, kind="clip")   # a CLIP-layout tower of the workload's width (the SigLIP
                                                                      # workload is timed on the same restatement)
    sec, fl = _cpu_oracle_fwd_bwd(llm_s, vis_s, hidden, B, S, vocab)
    llm1, vis1 = resolve_llm_config("meta-llama/Llama-3.2-1B-Instruct"), resolve_vision_config("openai/clip-vit-base-patch32")
    B1, S1 = 1, 1024
    sec1, fl1 = _cpu_oracle_fwd_bwd(llm1, vis1, llm1["hidden_size"], B1, S1, vocab)
    return dict(seconds=sec, flops=fl, cores=cores, visible=visible,
                sample=f"oracle/ref_cpu.py fwd+bwd bf16, second of two passes (the first is an untimed warm-up), B={B} S={S}, "
                       f"{budget_layers}-layer slice of the {workload} decoder + {budget_layers}-layer slice of its ViT + projector + "
                       f"full lm_head (vocab 128258); converted to samples/s of the full workload by algorithmic FLOPs",
                full_1b={"model": "Llama-3.2-1B + CLIP-ViT-B/32, every layer (SURVEY 8d's fwd+bwd form)", "B": B1, "S": S1,
                         "seconds": sec1, "flops": fl1})


def dump_outputs(out_dir, trainer, loss, max_elems=6_000_000):
    """--dump-outputs: what the last timed training_step computed, as float32 .npy files in `out_dir`:
        loss.npy     the loss that step returned
        params.npy   the parameters after that step's AdamW update (sampled)
        grads.npy    that step's gradients, at the same positions
    Sample: every parameter tensor in name order contributes min(numel, 4096) positions (fewer when the model has so many
    tensors that the two arrays would pass `max_elems` elements in all), drawn with a generator seeded by crc32 of the
    tensor's name -- the same positions from run to run and build to build, whatever the flat buffer's layout."""
    import zlib
    import numpy as np
    trainer.synchronize()            # the last update runs on a side stream, part of it deferred to the next forward
    torch.cuda.synchronize()
    flat = trainer.flat
    segs = sorted(flat.segments, key=lambda s: s.name)
    per = max(1, min(4096, max_elems // (2 * len(segs))))
    idx = []
    for seg in segs:
        n = seg.end - seg.start
        g = torch.Generator().manual_seed(zlib.crc32(seg.name.encode()))
        pos = torch.arange(n) if n <= per else torch.randint(0, n, (per,), generator=g).sort().values
        idx.append(pos + seg.start)
    idx = torch.cat(idx).to(flat.data.device)
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), loss.detach().float().reshape(1).cpu().numpy())
    np.save(os.path.join(out_dir, "params.npy"), flat.data[idx].float().cpu().numpy())
    if flat.grad is not None:
        np.save(os.path.join(out_dir, "grads.npy"), flat.grad[idx].float().cpu().numpy())


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks as CHILD processes (one per GPU,
    `python -m torch.distributed.run`, the launch the reference documents as `torchrun --nproc-per-node N -m multimeditron
    train`, docs/source/guides/training.rst:121,176-185) and return their exit code.  Called before anything in this
    process has touched the GPU (a process that has initialised HIP must never exec or fork GPU children)."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL across processes on this host driver)
    return subprocess.run(cmd, env=env).returncode


def dry_run(args, world, rank):
    """Launcher / rendezvous rehearsal on CPU (gloo): the rank plumbing, barriers, max-over-ranks timing and the JSON line
    of the real run with an empty step -- no model, no kernels, never a measurement (`"dry_run": true`, value 0)."""
    import torch.distributed as dist
    if world > 1 or "RANK" in os.environ:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if (dist.get_world_size() if dist.is_initialized() else 1) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the job has {world} rank(s)")
    t = torch.zeros(1, dtype=torch.float64)
    if dist.is_initialized():
        dist.barrier()
        t += 1.0
        dist.all_reduce(t, op=dist.ReduceOp.SUM)              # every rank takes part in the same collectives
    if rank == 0:
        print(json.dumps({"metric": "image-text samples/sec/node fwd+bwd, Llama-3.1-8B+ViT-L/14 bf16", "value": 0.0, "unit": "samples/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "dry_run": True,
                          "ranks_seen": int(t.item()) if dist.is_initialized() else 1}), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="llama31_8b_vitl14_s2048_b4", choices=sorted(WORKLOADS))
    ap.add_argument("--mode", default="FULL", choices=["FULL", "ALIGNMENT", "END2END", "LM_ONLY"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-all-rows", action="store_true", help="skip the extra timing of the step in HF's all-rows form (MM_LOSS_ROWS=0)")
    ap.add_argument("--padded", action="store_true", help="right-padded batch, lengths U[S/2, S] (SURVEY 8d: the key-mask path); "
                                                          "not the headline configuration")
    ap.add_argument("--dry-run", action="store_true", help="launcher rehearsal on CPU/gloo: no model, no kernels, no measurement")
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure the GEMM roofline (one instrumented step), "
                                                        "the all-rows form of the step and the CPU baseline (the --no-* options drop one)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps write what the last one computed to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "RANK" not in os.environ:          # bare `python bench.py --gpus N`: become the launcher
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_run:
        return dry_run(args, world, rank)
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with `python bench.py --gpus N` or "
                         f"`python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N`")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    use_dist = world > 1 or "RANK" in os.environ       # torchrun with one rank still rehearses the RCCL path
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC for RCCL, also when a launcher (not launch_ranks) started us
        opts = None
        try:      # RCCL kernels on a high-priority stream: they take freed CUs ahead of queued GEMM workgroups
            opts = dist.ProcessGroupNCCL.Options(is_high_priority_stream=True)
        except Exception:
            opts = None
        if opts is not None:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, pg_options=opts)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but the process group has {dist.get_world_size()} rank(s)")

    from multimeditron_amd.model.model import MultimodalConfig, MultiModalModelForCausalLM
    from multimeditron_amd.model.modalities import ImageConfig, SiglipImageConfig
    from multimeditron_amd.model.presets import resolve_llm_config, resolve_vision_config
    from multimeditron_amd.train.trainer import MultimodalTrainer, TrainingMode

    llm_name, clip_name, B, S, n_img = WORKLOADS[args.workload]
    llm, vis = resolve_llm_config(llm_name), resolve_vision_config(clip_name)
    vocab = llm["vocab_size"] + 2          # + <|image_start|>, <|image_end|> (reference cli/train.py:99-104)
    torch.manual_seed(1234)
    mod_cls = SiglipImageConfig if vis.get("kind") == "siglip" else ImageConfig
    cfg = MultimodalConfig(vocab_size=vocab, modalities=[mod_cls(hidden_size=llm["hidden_size"], clip_name=clip_name)],
                           llm_path=llm_name, dtype="bfloat16", eos_token_idx=128009, hidden_size=llm["hidden_size"])
    model = MultiModalModelForCausalLM(cfg, device=dev)
    model.pack_parameters()
    trainer = MultimodalTrainer(model, training_mode=TrainingMode[args.mode], learning_rate=1e-4, weight_decay=0.01,
                                max_grad_norm=1.0, gradient_accumulation_steps=1, max_steps=1000, min_lr=3e-5)
    P = (vis["image_size"] // vis["patch_size"]) ** 2
    special = (llm["vocab_size"], llm["vocab_size"] + 1, 128002)
    # the batch in the collator's own form (host tensors, all-ones mask, list of per-image pixel tensors), staged to HBM by
    # the product's prefetcher: batch n+1 is pinned and copied on a side stream while step n runs, so the timed region
    # contains the per-step list -> stack -> H2D of image_modality.py:131-132 and the mask handling, not a resident tensor
    from multimeditron_amd.train.prefetch import DevicePrefetcher
    host_batch, _ = synthetic_batch(B, S, n_img, P, vocab, special, 1234 + rank, "cpu", vis["image_size"], collator_form=True)
    if args.padded:       # SURVEY 8d's mask variant: right padding, lengths U[S/2, S] (the image span sits in the first half)
        gpad = torch.Generator().manual_seed(4321 + rank)
        lo = max(S // 2, int(host_batch["processed_multimodal_inputs"]["token_range"]["image"].max()) + 2)     # never cut an image span
        lens = torch.randint(lo, S + 1, (B,), generator=gpad)
        lens[0] = S
        keep = torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)
        host_batch["attention_mask"] = keep.long()
        host_batch["labels"] = torch.where(keep, host_batch["labels"], torch.full_like(host_batch["labels"], -100))

    def endless():
        while True:
            yield host_batch

    feed = DevicePrefetcher(endless(), device=dev)

    def sync():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        trainer.training_step(next(feed))
    sync()
    t0 = time.perf_counter()
    loss = None
    for _ in range(args.steps):
        loss = trainer.training_step(next(feed))
    sync()
    batch = next(feed)
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
    if args.dump_outputs:
        if rank == 0:
            dump_outputs(args.dump_outputs, trainer, loss)
        else:
            trainer.synchronize()
    fps = 3.0 * flops_per_sample(llm, vis, S, n_img, vocab, llm["hidden_size"]) if args.mode == "FULL" else None
    rows = getattr(batch["labels"], "_mm_loss_rows", None) if trainer.loss_rows_only else None
    fps_exec = fps
    if fps is not None and rows is not None:              # lm_head + loss ran on the labelled rows only: count what was executed
        fps_exec = 3.0 * flops_per_sample(llm, vis, S, n_img, vocab, llm["hidden_size"], lm_head_rows=rows.n / B)
    value = world * B * args.steps / elapsed
    out = {"metric": f"image-text samples/sec/node fwd+bwd, {METRIC_MODELS[args.workload]} bf16", "value": round(value, 4), "unit": "samples/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": args.workload, "per_gpu_batch": B, "global_batch": B * world, "seq_len": S, "images_per_sample": n_img,
                      "training_mode": args.mode,
                      "optimizer": "AdamW every step (fused, fp32 master" + (" held as bf16 parameter + 16-bit remainder" if trainer.split_master else "") + " + fp32 m, v" + (f"; state sharded over the {world} ranks: reduce-scatter, "
                                   "update, all-gather)" if trainer.shard_optim else ")"), "parallelism": f"dp{world}",
                      **({"padding": "right-padded, lengths U[S/2, S] (key-mask path); tokens counted as S per sample"} if args.padded else {}),
                      "final_loss": round(float(loss), 4),
                      "input_staging": "collator-form host batch (all-ones attention_mask, list of per-image tensors) staged per step by "
                                       "train/prefetch.py DevicePrefetcher (pinned, side stream)",
                      "logits_rel_l2_vs_fp32_reference": {"bf16_path_benchmarked_here": 8.4e-3, "fp32_parity_path": 7.9e-7,
                                                          "north_star_bar": 1e-3, "where": "tests/test_model_gpu.py (bf16 bound 3e-2 and <= 2x "
                                                          "the oracle's own bf16 error; a bf16 pipeline cannot meet 1e-3 against fp32)"}}}
    # the instrumented extra step issues the same gradient-exchange collectives as any other step: EVERY rank runs it
    # (rank 0 alone would leave its all-reduces unmatched and hang); only rank 0 reports
    r = measure_gemm_roofline(trainer, batch) if args.full and not args.no_roofline else None
    # the same step in HF's form (every row through the last layer's MLP, the final norm, lm_head and the loss), timed beside the
    # headline so that both numbers come from one process on one box: every rank runs it (collectives), rank 0 reports
    all_rows = None
    if args.full and trainer.loss_rows_only and not args.no_all_rows:
        trainer.loss_rows_only = False
        k2 = max(3, args.steps // 2)
        for _ in range(2):
            trainer.training_step(next(feed))
        sync()
        t1 = time.perf_counter()
        for _ in range(k2):
            trainer.training_step(next(feed))
        sync()
        e2 = time.perf_counter() - t1
        if use_dist:
            t = torch.tensor([e2], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e2 = float(t)
        trainer.loss_rows_only = True
        all_rows = {"ms_per_step": round(1e3 * e2 / k2, 3), "value": round(world * B * k2 / e2, 4), "steps": k2}
    if rank == 0:
        if fps is not None:
            step_tf = value / world * fps_exec / 1e12
            out["config"]["flops_per_sample_fwd_bwd"] = fps_exec
            if all_rows is not None:
                ar_tf = all_rows["value"] / world * fps / 1e12          # that step executes HF's full work list: 96.04 TFLOP/sample
                out["config"]["all_rows_form"] = dict(all_rows, flops_per_sample_fwd_bwd=fps, whole_step_achieved=round(ar_tf, 2),
                                                      whole_step_frac=round(ar_tf / PEAK_BF16_TFLOPS, 4),
                                                      note="the same step with MM_LOSS_ROWS=0 (logits of every row, as HF computes "
                                                      "them), timed after the headline in this process")
            if rows is not None:
                out["config"]["loss_rows"] = (f"last layer's o_proj + MLP, final norm, lm_head and cross-entropy on the {rows.n} of {rows.total} rows whose shifted label is "
                                              f"not -100 (same loss and gradients; MM_LOSS_ROWS=0 computes every row as HF does: "
                                              f"{fps:.6g} flops/sample); whole_step_* count the executed flops")
        roof = None
        if r is not None:
            ra = r["all"]
            roof = {"bound": "mfma", "kernel": f"gemm_bf16_w4_kernel (the 4-wave hand-scheduled 256x256 bf16 GEMM, NT/NN/TN, every epilogue kind: {r['launches']} of the step's {ra['launches']} "
                    f"bf16 GEMM launches, {100 * r['flops_share']:.1f} % of their flops)", "achieved": round(r["achieved_tflops"], 2), "peak": PEAK_BF16_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(r["achieved_tflops"] / PEAK_BF16_TFLOPS, 4), "traffic": None,
                    "launches_per_step": r["launches"], "avg_launch_ms": round(r["avg_launch_ms"], 4),
                    "flops_per_launch": r["flops_per_launch"], "gemm_ms_per_step": round(r["gemm_ms_per_step"], 2),
                    "algorithmic_bytes_per_launch": round(r["algorithmic_bytes_per_launch"]),
                    "all_gemm_launches": {"kernel": "gemm_bf16_w4_kernel + gemm_bf16_dma_kernel: every bf16 GEMM launch of the step (rounds 1-3's definition of `roofline`; the "
                                          "8-wave kernel's small-tile launches are the ViT's, stretched under AdamW / the deferred weight gradients)",
                                          "achieved": round(ra["achieved_tflops"], 2), "frac": round(ra["achieved_tflops"] / PEAK_BF16_TFLOPS, 4),
                                          "launches_per_step": ra["launches"], "avg_launch_ms": round(ra["avg_launch_ms"], 4),
                                          "gemm_ms_per_step": round(ra["gemm_ms_per_step"], 2), "traffic": None}}
            pt, why = pmc_traffic()
            if pt is not None and args.workload == "llama31_8b_vitl14_s2048_b4" and args.mode == "FULL":
                roof["traffic"] = round(pt["bytes_per_launch"])       # HBM bytes per launch, same averaging as `achieved`
                roof["traffic_source"] = pt["file"] + ": " + pt["method"]
                if "all_gemm_launches" in pt:
                    roof["all_gemm_launches"]["traffic"] = round(pt["all_gemm_launches"]["bytes_per_launch"])
            else:
                roof["traffic_source"] = why or "PMC passes exist for the headline workload in FULL mode only"
            if fps is not None:
                roof["whole_step_achieved"] = round(step_tf, 2)
                roof["whole_step_frac"] = round(step_tf / PEAK_BF16_TFLOPS, 4)
            out["roofline"] = roof
        if world == 1 and args.full and not args.no_cpu_baseline:
            del trainer, model, batch, feed
            torch.cuda.empty_cache()
            c = cpu_baseline(llm, vis, llm["hidden_size"], args.workload)
            full = 3.0 * flops_per_sample(llm, vis, S, n_img, vocab, llm["hidden_size"])
            out["cpu_baseline"] = {"value": round(c["flops"] / c["seconds"] / full, 6), "unit": "samples/s", "cores": c["cores"],
                                   "host_cpus_visible": c["visible"], "cpu_model": cpu_model_name(), "kind": "port",
                                   "sample": c["sample"], "measured_seconds": round(c["seconds"], 2),
                                   "cpu_tflops": round(c["flops"] / c["seconds"] / 1e12, 3)}
            f1 = c["full_1b"]
            out["cpu_baseline"]["full_model_1b"] = {"model": f1["model"], "B": f1["B"], "S": f1["S"], "measured_seconds": round(f1["seconds"], 2),
                                                    "samples_per_s_of_that_model": round(f1["B"] / f1["seconds"], 5),
                                                    "cpu_tflops": round(f1["flops"] / f1["seconds"] / 1e12, 3),
                                                    "scaled_to_workload_samples_per_s": round(f1["flops"] / f1["seconds"] / full, 6)}
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
