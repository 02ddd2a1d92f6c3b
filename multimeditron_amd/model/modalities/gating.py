"""The MoE image modalities' gating network (reference model/modalities/moe/gating.py:9-89): a torchvision ResNet-50 whose `fc` has
one output per expert, run in eval mode on libmmhip's NHWC convolution kernels (csrc/mm_conv.hip).

torchvision is not needed: ResNet-50 is a fixed, public architecture (He et al. 2015; torchvision's v1.5 variant puts the stride of
a stage's first bottleneck on its 3x3 convolution) with a fixed key set, and its eval-mode forward is convolutions followed by a
per-channel scale and shift, one max-pool, a mean and a small linear layer.  Parameters and buffers carry exactly torchvision's
names under `resnet.` (conv1, bn1, layer{1..4}.{i}.conv{1,2,3} / bn{1,2,3} / downsample.{0,1}, fc; running_mean, running_var,
num_batches_tracked), in torchvision's shapes, so a checkpoint the reference wrote loads as it is.

What runs: mm_nchw_to_nhwc (pixels -> NHWC, 3 -> 8 channels) -> 53 x mm_conv2d_nhwc_fwd (BatchNorm as the fp32 epilogue scale /
shift, ReLU and the bottleneck's residual add fused; one rounding per convolution output) + mm_maxpool2d_nhwc -> mm_gate_head
(mean, fc, softmax, top-k): 56 launches on the calling stream, under no_grad.  scale = gamma / sqrt(running_var + eps) and
shift = beta - running_mean * scale are computed in fp32 from the stored tensors, and the filters are repacked to
[Cout, R, S, Cin], once per weight load (`_packed`: rebuilt when a parameter or buffer has been written or moved), never per forward.

By default the gate is FROZEN: eval mode always (`train()` does not change it), no parameter requires a gradient.  Training it
(the reference's FULL mode, image_modality_moe.py:233-241) is opt-in: after `set_trainable(True)`, `train(mode)` takes effect and
the training-mode forward runs as one autograd node (`_GateTrainFn`, csrc/mm_conv_bwd.hip): convolution -> BatchNorm with batch
statistics per unit, and in reverse BatchNorm backward, convolution weight and data gradients and the max-pool's backward; the
parameter gradients come back in torchvision's shapes.  In eval mode, and always while not trainable, the fused scale / shift
forward above runs unchanged, bit for bit.  The MoE modalities switch this on from their `train_gate` config field (DESIGN.md
section 7)."""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional

import torch
import torch.nn as nn

BN_EPS = 1e-5
LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))          # (bottleneck width, blocks, stride of the first block)
EXPANSION = 4


class GatingNetworkConfig:
    """reference moe/gating.py:9-34 (same fields; what HF's PretrainedConfig would write beside them is kept on load)."""
    model_type = "gating_network"

    def __init__(self, num_classes: int = 2, top_k: int = 1, image_processor_path: str = "openai/clip-vit-base-patch32",
                 class_names: Optional[List[str]] = None, **kwargs):
        self.num_classes = int(num_classes)
        self.top_k = int(top_k)
        self.image_processor_path = image_processor_path
        self.class_names = list(class_names or [])
        self._extra = {k: v for k, v in kwargs.items() if k != "model_type"}

    def to_dict(self) -> Dict[str, Any]:
        d = dict(self._extra)
        d.update(num_classes=self.num_classes, top_k=self.top_k, image_processor_path=self.image_processor_path,
                 class_names=list(self.class_names), model_type=self.model_type)
        return d

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "GatingNetworkConfig":
        return cls(**d)

    def __eq__(self, other):
        return isinstance(other, GatingNetworkConfig) and self.to_dict() == other.to_dict()


class _Pretrained(nn.Module):
    _mm_pretrained = True            # MultiModalModelForCausalLM._init_weights leaves these modules' tensors alone


class _Conv(_Pretrained):
    def __init__(self, cin, cout, k, stride, pad):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k), requires_grad=False)
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")
        self.k, self.stride, self.pad = k, stride, pad


class _BatchNorm(_Pretrained):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _Linear(_Pretrained):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        nn.init.normal_(self.weight, std=cin ** -0.5)


class _Bottleneck(_Pretrained):
    def __init__(self, cin, width, stride):
        super().__init__()
        cout = width * EXPANSION
        self.conv1, self.bn1 = _Conv(cin, width, 1, 1, 0), _BatchNorm(width)
        self.conv2, self.bn2 = _Conv(width, width, 3, stride, 1), _BatchNorm(width)          # v1.5: the stride sits on the 3x3
        self.conv3, self.bn3 = _Conv(width, cout, 1, 1, 0), _BatchNorm(cout)
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(_Conv(cin, cout, 1, stride, 0), _BatchNorm(cout))
        else:
            self.downsample = None


class _ResNet50(_Pretrained):
    def __init__(self, num_classes):
        super().__init__()
        self.conv1, self.bn1 = _Conv(3, 64, 7, 2, 3), _BatchNorm(64)
        cin = 64
        for i, (width, blocks, stride) in enumerate(LAYERS):
            seq = nn.Sequential()
            for b in range(blocks):
                seq.append(_Bottleneck(cin, width, stride if b == 0 else 1))
                cin = width * EXPANSION
            setattr(self, f"layer{i + 1}", seq)
        self.fc = _Linear(cin, num_classes)

    def units(self):
        """[(key, conv, bn)] in launch order; key is the module path of the convolution"""
        out = [("conv1", self.conv1, self.bn1)]
        for i in range(4):
            for b, blk in enumerate(getattr(self, f"layer{i + 1}")):
                pre = f"layer{i + 1}.{b}."
                out += [(pre + "conv1", blk.conv1, blk.bn1), (pre + "conv2", blk.conv2, blk.bn2), (pre + "conv3", blk.conv3, blk.bn3)]
                if blk.downsample is not None:
                    out.append((pre + "downsample.0", blk.downsample[0], blk.downsample[1]))
        return out

    def conv_bn_pairs(self):
        """[(conv, bn)] in launch order."""
        return [(c, bn) for _key, c, bn in self.units()]


class GatingNetwork(_Pretrained):
    config_class = GatingNetworkConfig

    def __init__(self, config: GatingNetworkConfig, dtype: Optional[torch.dtype] = None, device=None):
        super().__init__()
        self.config = config
        self.top_k = config.top_k
        self.resnet = _ResNet50(config.num_classes)
        self._packed = None
        self._packed_key = None
        self._trainable = False
        if dtype is not None or device is not None:
            self.to(device=device, dtype=dtype)
        super().train(False)

    # ---- frozen and eval only, unless made trainable
    def set_trainable(self, flag: bool):
        """Switch `requires_grad` of all 161 parameters and let `train(mode)` take effect; switching off returns to eval mode."""
        self._trainable = bool(flag)
        for p in self.parameters():
            p.requires_grad = self._trainable
        if not self._trainable:
            super().train(False)
        return self

    def train(self, mode: bool = True):
        if self._trainable:
            self._packed = None        # a trainer writes the parameters behind their version counters: repack on the next eval forward
        return super().train(bool(mode) and self._trainable)

    @property
    def dtype(self):
        return self.resnet.fc.weight.dtype

    @property
    def device(self):
        return self.resnet.fc.weight.device

    # ---- packed operands
    def _key(self):
        ts = list(self.parameters()) + list(self.buffers())
        return (ts[0].data_ptr(), ts[0].dtype, sum(t._version for t in ts))

    def _pack(self):
        """Filters [Cout, Cin, R, S] -> [Cout, R, S, Cin] (the stem's Cin 3 -> 8 with zeros) in the storage type; eval-mode BatchNorm
        -> fp32 scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
        packed = {}
        with torch.no_grad():
            for conv, bn in self.resnet.conv_bn_pairs():
                w = conv.weight.permute(0, 2, 3, 1)
                if w.shape[3] % 8:
                    w = torch.nn.functional.pad(w, (0, 8 - w.shape[3] % 8))
                scale = bn.weight.float() / torch.sqrt(bn.running_var.float() + BN_EPS)
                shift = bn.bias.float() - bn.running_mean.float() * scale
                packed[id(conv)] = (w.contiguous(), scale.contiguous(), shift.contiguous())
        return packed

    def packed(self):
        key = self._key()
        if self._packed is None or key != self._packed_key:
            self._packed, self._packed_key = self._pack(), key
        return self._packed

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._packed = None
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._packed = None
        return out

    # ---- forward
    def forward(self, pixel_values: torch.Tensor, stages: Optional[Dict[str, Any]] = None):
        """pixels [n, 3, H, W] -> (logits [n, E], topk_indices [n, top_k] int64, weights [n, E]) (reference gating.py:73-89).
        Trainable and in training mode: batch statistics, `logits` and `weights` carry a grad_fn (`_GateTrainFn`); `stages`, when
        given, receives the operands and results of every launch of that path.  Otherwise the frozen eval forward below."""
        if self._trainable and self.training:
            params = [p for _, p in self.resnet.named_parameters()]
            px = pixel_values.detach().to(device=self.device, dtype=torch.float32).contiguous()
            logits, weights, topk = _GateTrainFn.apply(self, stages, px, *params)
            self._packed = None                          # the running statistics were written behind autograd's back
            return logits, topk, weights
        with torch.no_grad():
            return self._forward_eval(pixel_values)

    def _forward_eval(self, pixel_values: torch.Tensor):
        from ... import kernels as K
        r = self.resnet
        pk = self.packed()

        def conv(x, c, residual=None, relu=True):
            w, scale, shift = pk[id(c)]
            return K.conv2d_nhwc(x, w, scale, shift, c.stride, c.pad, residual=residual, relu=relu)

        px = pixel_values.detach().to(device=self.device, dtype=torch.float32).contiguous()
        x = K.nchw_to_nhwc(px, 8, self.dtype)
        x = K.maxpool2d_nhwc(conv(x, r.conv1))
        for i in range(4):
            for blk in getattr(r, f"layer{i + 1}"):
                identity = x if blk.downsample is None else conv(x, blk.downsample[0], relu=False)
                x = conv(conv(conv(x, blk.conv1), blk.conv2), blk.conv3, residual=identity)
        n, H, W, C = x.shape
        return K.gate_head(x.view(n, H * W, C), r.fc.weight, r.fc.bias, self.top_k)

    def units(self):
        return self.resnet.units()

    # ---- HF layout: config.json + model.safetensors (keys resnet.*)
    def save_pretrained(self, path: str):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config.to_dict(), f, indent=2, sort_keys=True)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        save_file({k: v.detach().cpu().contiguous().clone() for k, v in self.state_dict().items()},
                  os.path.join(path, "model.safetensors"), metadata={"format": "pt"})

    @classmethod
    def from_pretrained(cls, path: str, dtype: Optional[torch.dtype] = None, device=None) -> "GatingNetwork":
        from safetensors.torch import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg = GatingNetworkConfig.from_dict(json.load(f))
        gate = cls(cfg)
        sd = load_file(os.path.join(path, "model.safetensors"))
        if dtype is None:
            dtype = sd["resnet.fc.weight"].dtype
        gate.to(dtype=dtype)
        own = gate.state_dict()
        gate.load_state_dict({k: v.to(own[k].dtype) if k in own else v for k, v in sd.items()}, strict=True)
        if device is not None:
            gate.to(device=device)
        return gate


def is_gate_dir(path) -> bool:
    return isinstance(path, str) and bool(path) and os.path.isdir(path) and os.path.isfile(os.path.join(path, "config.json"))


def _pack_filter(weight):
    """[Cout, Cin, R, S] -> a packed COPY [Cout, R, S, Cin] (the stem's Cin 3 -> 8 with zeros)"""
    w = weight.detach().permute(0, 2, 3, 1)
    if w.shape[3] % 8:
        return torch.nn.functional.pad(w, (0, 8 - w.shape[3] % 8)).contiguous()
    return w.clone(memory_format=torch.contiguous_format)


class _GateTrainFn(torch.autograd.Function):
    """The gate in training mode as ONE autograd node.  Forward, per convolution unit: z = mm_conv2d_nhwc_fwd (scale 1, shift 0: the
    raw convolution, one rounding) -> mm_bn_train_fwd (batch statistics, residual and ReLU fused; running statistics updated in
    place), then the max-pool after the stem and mm_gate_head.  Backward walks the units in reverse: the head in torch on [n, E] and
    [n, 2048] tensors (it differentiates weights = T(softmax_fp32(float(T(logits)))) with the pooled mean in fp32, the roundings
    taken as identities), then per unit mm_bn_train_bwd -> mm_conv2d_nhwc_wgrad and mm_conv2d_nhwc_dgrad, whose addend joins a
    bottleneck's residual branch with its identity path in one rounding, and mm_maxpool2d_nhwc_bwd in front of the stem.
    The backward reads COPIES of the filters, gamma and the fc weight taken by the forward (a trainer may update the parameters in
    between), and writes the parameter gradients, in torchvision's shapes, where every Function of this package writes them
    (functional.grad_target: the trainer's flat gradient buffer, overwrite or accumulate)."""

    @staticmethod
    def forward(ctx, gate, stages, px, *params):
        from ... import kernels as K
        r = gate.resnet
        T, dev = gate.dtype, px.device
        saved = {}
        affine = {}

        def unit(key, x, c, bn, residual=None, relu=True):
            w = _pack_filter(c.weight)
            cout = w.shape[0]
            if cout not in affine:
                affine[cout] = (torch.ones(cout, dtype=torch.float32, device=dev), torch.zeros(cout, dtype=torch.float32, device=dev))
            z = K.conv2d_nhwc(x, w, affine[cout][0], affine[cout][1], c.stride, c.pad)
            gamma = bn.weight.detach().clone()
            y, mean, invstd = K.bn_train_fwd(z, gamma, bn.bias.detach(), residual, relu, eps=BN_EPS, running_mean=bn.running_mean,
                                             running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked)
            saved[key] = dict(x=x, w=w, gamma=gamma, z=z, y=y, mean=mean, invstd=invstd, relu=relu, k=c.k, stride=c.stride, pad=c.pad,
                              cin=c.weight.shape[1])
            return y

        x0 = K.nchw_to_nhwc(px, 8, T)
        stem = unit("conv1", x0, r.conv1, r.bn1)
        x = K.maxpool2d_nhwc(stem)
        for i in range(4):
            for b, blk in enumerate(getattr(r, f"layer{i + 1}")):
                pre = f"layer{i + 1}.{b}."
                identity = x if blk.downsample is None else unit(pre + "downsample.0", x, blk.downsample[0], blk.downsample[1], relu=False)
                y = unit(pre + "conv1", x, blk.conv1, blk.bn1)
                y = unit(pre + "conv2", y, blk.conv2, blk.bn2)
                x = unit(pre + "conv3", y, blk.conv3, blk.bn3, residual=identity)
        n, H, W, C = x.shape
        fc_w = r.fc.weight.detach().clone()
        logits, topk, weights = K.gate_head(x.view(n, H * W, C), fc_w, r.fc.bias.detach(), gate.top_k)
        ctx.stages, ctx.saved, ctx.last, ctx.T = stages, saved, x, T
        ctx.blocks = [(f"layer{i + 1}.{b}.", blk.downsample is not None) for i in range(4) for b, blk in enumerate(getattr(r, f"layer{i + 1}"))]
        ctx.params = dict(zip([nm for nm, _ in r.named_parameters()], params))
        ctx.head = (logits, fc_w)
        if stages is not None:
            for key, u in saved.items():
                for f in ("x", "z", "y", "mean", "invstd"):
                    stages[f"{key}.{f}"] = u[f]
            stages["pool.x"], stages["head.x"], stages["logits"], stages["weights"] = stem, x, logits, weights
        ctx.mark_non_differentiable(topk)
        return logits, weights, topk

    @staticmethod
    def backward(ctx, dlogits, dweights, _dtopk):
        from ... import functional as Fm
        from ... import kernels as K
        stages, saved, last, T = ctx.stages, ctx.saved, ctx.last, ctx.T
        if saved is None:
            raise RuntimeError("the gate's training backward ran twice: its saved activations are released after the first pass "
                               "(retain_graph is not supported)")

        def rec(key, **kw):
            if stages is not None:
                for f, v in kw.items():
                    stages[f"{key}.{f}"] = v

        def emit(name, g):
            """the gradient of parameter `name` is complete: into its buffer (overwrite or accumulate), then the trainer's hook"""
            p = ctx.params[name]
            if not p.requires_grad:
                return
            buf, acc = Fm.grad_target(p)
            if acc:
                buf.add_(g.view(buf.shape))
            else:
                buf.copy_(g.view(buf.shape))
            Fm._ready(p)

        # ---- head: logits = T(pooled . W^T + b), weights = T(softmax_fp32(float(logits)))
        logits, fc_w = ctx.head
        n, H, W, C = last.shape
        p = torch.softmax(logits.float(), dim=-1)
        dl = dlogits.float() if dlogits is not None else torch.zeros_like(p)
        if dweights is not None:
            dw32 = dweights.float()
            dl = dl + p * (dw32 - (p * dw32).sum(-1, keepdim=True))
        pooled = last.view(n, H * W, C).float().mean(1)
        emit("fc.weight", (dl.t() @ pooled).to(T))
        emit("fc.bias", dl.sum(0).to(T))
        dpooled = dl @ fc_w.float()
        dy = (dpooled / (H * W)).to(T).view(n, 1, 1, C).expand(n, H, W, C).contiguous()
        rec("head", dl=dl, dx=dy)

        def bn_bwd(key, dy, want_dres=False):
            u = saved[key]
            dz, dres, dgamma, dbeta = K.bn_train_bwd(dy, u["y"], u["z"], u["mean"], u["invstd"], u["gamma"], u["relu"], want_dres=want_dres)
            dw = K.conv2d_nhwc_wgrad(dz, u["x"], u["k"], u["stride"], u["pad"])
            name = key[:-len("conv1")] + "bn" + key[-1] if not key.endswith("downsample.0") else key[:-1] + "1"
            emit(key + ".weight", dw[..., :u["cin"]].permute(0, 3, 1, 2).contiguous())
            emit(name + ".weight", dgamma)
            emit(name + ".bias", dbeta)
            rec(key, dy=dy, dz=dz, dres=dres, dw=dw, dgamma=dgamma, dbeta=dbeta)
            return dz, dres

        def dgrad(key, dz, addend=None):
            u = saved[key]
            wp = u["w"].permute(3, 1, 2, 0).contiguous()                         # the forward's filter as [Cin, R, S, Cout]
            dx = K.conv2d_nhwc_dgrad(dz, wp, u["x"].shape[1], u["x"].shape[2], u["stride"], u["pad"], addend=addend)
            rec(key, dx=dx)
            return dx

        for pre, has_down in reversed(ctx.blocks):
            dz3, dres = bn_bwd(pre + "conv3", dy, want_dres=True)
            dz2, _ = bn_bwd(pre + "conv2", dgrad(pre + "conv3", dz3))
            dz1, _ = bn_bwd(pre + "conv1", dgrad(pre + "conv2", dz2))
            if has_down:
                dzd, _ = bn_bwd(pre + "downsample.0", dres)
                dres = dgrad(pre + "downsample.0", dzd)
            dy = dgrad(pre + "conv1", dz1, addend=dres)                          # the join of the two paths: one rounding
        dy = K.maxpool2d_nhwc_bwd(saved["conv1"]["y"], dy)
        rec("pool", dx=dy)
        bn_bwd("conv1", dy)
        ctx.saved = ctx.last = None
        return (None,) * (3 + len(ctx.params))
