#!/usr/bin/env python3
"""The MoE gating network (ResNet-50 on the NHWC convolution kernels) in time: the gate alone at n images of 224x224 in bf16, its
largest kernels, and the forward of tools/moe_bench.py's modality (E ViT-L/14 experts, frozen towers, graph replay) with the real
gate against the same forward with a constant-callable gate -- both in this process, interleaved round by round.
   python tools/gating_bench.py [E] [n] [rounds]
   python tools/gating_bench.py --train [E] [n] [rounds]     the trainable gate's training forward + backward beside its eval forward
                                                             (timed, not judged: no threshold)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multimeditron_amd import kernels as K
from multimeditron_amd.nn import FlatParams
from multimeditron_amd.model.modalities import GatingNetwork, GatingNetworkConfig, MOEImageConfig, MOEImageModality

TRAIN = "--train" in sys.argv
sys.argv = [a for a in sys.argv if a != "--train"]
E = int(sys.argv[1]) if len(sys.argv) > 1 else 4
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
torch.manual_seed(0)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


gate = GatingNetwork(GatingNetworkConfig(num_classes=E, top_k=1), dtype=torch.bfloat16, device="cuda")
with torch.no_grad():
    for k, p in gate.named_parameters():          # a trained gate's scale: BatchNorm keeps the activations of order 1
        if p.dim() == 1 and k.endswith("weight"):
            p.fill_(0.5)
px = torch.randn(n, 3, 224, 224, device="cuda")
for _ in range(3):
    gate(px)
alone = [timed(lambda: gate(px), 10) for _ in range(rounds)]

if TRAIN:
    gate.set_trainable(True).train()
    dw = torch.randn(n, E, device="cuda").to(torch.bfloat16)

    def fwd_bwd():
        gate(px)[2].backward(dw)

    def fwd_only():
        with torch.no_grad():          # the training forward's launches without the autograd node's bookkeeping being used
            gate(px)

    for _ in range(3):
        fwd_bwd()
    both = [timed(fwd_bwd, 10) for _ in range(rounds)]
    fwd = [timed(fwd_only, 10) for _ in range(rounds)]
    print(json.dumps({"E": E, "n": n, "gate_eval_forward_ms": {"median": statistics.median(alone), "min": min(alone)},
                      "gate_train_forward_ms": {"median": statistics.median(fwd), "min": min(fwd)},
                      "gate_train_forward_backward_ms": {"median": statistics.median(both), "min": min(both)}}))
    sys.exit(0)

# per-convolution times (each shape once, 20 launches), largest first
per = {}
pk = gate.packed()
x = K.nchw_to_nhwc(px, 8, torch.bfloat16)
acts = {}


def conv_time(xin, c, name):
    w, scale, shift = pk[id(c)]
    y = K.conv2d_nhwc(xin, w, scale, shift, c.stride, c.pad, relu=True)
    ms = timed(lambda: K.conv2d_nhwc(xin, w, scale, shift, c.stride, c.pad, relu=True), 20)
    flop = 2.0 * y.numel() * w.shape[1] * w.shape[2] * w.shape[3]
    per[name] = (ms, flop / ms / 1e9, tuple(xin.shape), tuple(w.shape))
    return y


r = gate.resnet
x = K.maxpool2d_nhwc(conv_time(x, r.conv1, "conv1"))
for i in range(4):
    for b, blk in enumerate(getattr(r, f"layer{i + 1}")):
        p = f"layer{i + 1}.{b}"
        idn = x if blk.downsample is None else conv_time(x, blk.downsample[0], p + ".downsample")
        x = conv_time(conv_time(conv_time(x, blk.conv1, p + ".conv1"), blk.conv2, p + ".conv2"), blk.conv3, p + ".conv3")
top = sorted(per.items(), key=lambda kv: -kv[1][0])[:5]

cfg = MOEImageConfig(hidden_size=4096, expert_clip_names=["openai/clip-vit-large-patch14"] * E, image_processor="openai/clip-vit-large-patch14",
                     top_k_experts=E, generalist_idx=E - 1, fusion_method="weighted_average", cross_attn_heads=8)
const_w = torch.full((n, E), 1.0 / E, device="cuda")
const_l = torch.zeros(n, E, device="cuda")
const_i = torch.zeros(n, 1, dtype=torch.long, device="cuda")
m = MOEImageModality(cfg, dtype=torch.bfloat16, device="cuda", gating_network=lambda p: (const_l, const_i, const_w))
FlatParams([(k, p, "projector" if k.startswith("projector") else "encoder") for k, p in m.named_parameters()], "cuda", torch.bfloat16)
m.freeze_modality_embedder()
m.eval()
plugs = {"constant gate": m.gating_network, "ResNet-50 gate": lambda p: gate(p)}
res = {k: [] for k in plugs}
with torch.no_grad():
    for k, fn in plugs.items():
        m.gating_network = fn
        for _ in range(3):
            m(px)
    for _ in range(rounds):
        for k, fn in plugs.items():
            m.gating_network = fn
            res[k].append(timed(lambda: m(px), 10))

med = {k: statistics.median(v) for k, v in res.items()}
out = {"E": E, "n": n, "gate_alone_ms": {"median": statistics.median(alone), "min": min(alone)},
       "moe_forward_ms": {k: {"median": med[k], "min": min(v)} for k, v in res.items()},
       "gate_share_of_forward": (med["ResNet-50 gate"] - med["constant gate"]) / med["constant gate"],
       "sum_of_conv_ms": sum(v[0] for v in per.values()),
       "largest_convs": [{"name": k, "ms": v[0], "tflops": v[1], "x": v[2], "w": v[3]} for k, v in top]}
print(json.dumps(out))
