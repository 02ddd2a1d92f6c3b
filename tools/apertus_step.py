#!/usr/bin/env python3
"""Training step at the Apertus-8B shape: swiss-ai/Apertus-8B-Instruct-2509 (preset: q/k norm, xIELU MLP with I = 21504) + CLIP
ViT-L/14, bf16, B = 4, S = 2048, one image per sample, FULL mode, random init -- bench.py's recipe (synthetic batch in the
collator's form, staged by the prefetcher, AdamW every step) on a model bench.py's workload list does not hold.  Prints ms/step,
samples/s and the final loss as one JSON line.

    python tools/apertus_step.py [--steps 10] [--warmup 3] [--mode FULL] [--layers N]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench

LLM, CLIP, B, S, N_IMG = "swiss-ai/Apertus-8B-Instruct-2509", "openai/clip-vit-large-patch14", 4, 2048, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="FULL", choices=["FULL", "ALIGNMENT", "END2END", "LM_ONLY"])
    ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the preset's 32)")
    args = ap.parse_args()
    from multimeditron_amd.model.model import MultimodalConfig, MultiModalModelForCausalLM
    from multimeditron_amd.model.modalities import ImageConfig
    from multimeditron_amd.model.presets import resolve_llm_config, resolve_vision_config
    from multimeditron_amd.train.prefetch import DevicePrefetcher
    from multimeditron_amd.train.trainer import MultimodalTrainer, TrainingMode

    llm, vis = resolve_llm_config(LLM), resolve_vision_config(CLIP)
    if args.layers:
        llm["num_hidden_layers"] = args.layers
    vocab = llm["vocab_size"] + 2
    torch.manual_seed(1234)
    cfg = MultimodalConfig(vocab_size=vocab, modalities=[ImageConfig(hidden_size=llm["hidden_size"], clip_name=CLIP)], llm_path=LLM,
                           dtype="bfloat16", eos_token_idx=llm["vocab_size"] - 1, hidden_size=llm["hidden_size"])
    model = MultiModalModelForCausalLM(cfg, device="cuda", llm_config=llm)
    model.pack_parameters()
    trainer = MultimodalTrainer(model, training_mode=TrainingMode[args.mode], learning_rate=1e-4, weight_decay=0.01, max_grad_norm=1.0,
                                gradient_accumulation_steps=1, max_steps=1000, min_lr=3e-5)
    P = (vis["image_size"] // vis["patch_size"]) ** 2
    special = (llm["vocab_size"], llm["vocab_size"] + 1, 128002)
    host, _ = bench.synthetic_batch(B, S, N_IMG, P, vocab, special, 1234, "cpu", vis["image_size"], collator_form=True)

    def endless():
        while True:
            yield host

    feed = DevicePrefetcher(endless(), device="cuda")
    for _ in range(args.warmup):
        trainer.training_step(next(feed))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = None
    for _ in range(args.steps):
        loss = trainer.training_step(next(feed))
    trainer.synchronize()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(json.dumps({"workload": "apertus_8b_vitl14_s2048_b4", "layers": llm["num_hidden_layers"], "mode": args.mode, "ms_per_step": round(ms, 2),
                      "samples_per_s": round(B / ms * 1e3, 3), "loss": float(loss), "steps": args.steps, "warmup": args.warmup}))
    trainer.close()


if __name__ == "__main__":
    main()
