"""Reference for the MoE gating network (multimeditron_amd/model/modalities/gating.py), independent of the package: the torchvision
ResNet-50 key set spelt out by construction rule, seeded weights, and the eval-mode forward as plain torch.nn.functional ops on the CPU.

This restates torchvision.models.resnet50 (v1.5: the stride of a stage's first bottleneck sits on its 3x3 convolution) from the
public architecture; torchvision itself is not available to check it against.  The facts it encodes (key set, shapes, parameter
count) are asserted by tests/test_gating_cpu.py.

`forward(sd, pixels)` runs in float64 on the tensors it is given (the storage-rounded weights the kernels read).
`forward(sd, pixels, storage=T)` is the EMULATED forward: fp32 arithmetic with the kernels' documented rounding points in T
(include/mm_hip.h): pixels -> T; every convolution output T(relu(conv * scale + shift (+ identity))) with fp32 scale / shift computed
from the stored BatchNorm tensors; max-pool exact; pooled mean kept in fp32; logits -> T; weights = T(softmax_fp32(logits))."""
import torch
import torch.nn.functional as F

LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))
EPS = 1e-5


def conv_bn_specs():
    """[(conv key, bn key, Cout, Cin, k, stride, pad)] in torchvision's module order."""
    out = [("conv1", "bn1", 64, 3, 7, 2, 3)]
    cin = 64
    for li, (width, blocks, stride) in enumerate(LAYERS):
        for b in range(blocks):
            p = f"layer{li + 1}.{b}"
            s = stride if b == 0 else 1
            out.append((f"{p}.conv1", f"{p}.bn1", width, cin, 1, 1, 0))
            out.append((f"{p}.conv2", f"{p}.bn2", width, width, 3, s, 1))
            out.append((f"{p}.conv3", f"{p}.bn3", width * 4, width, 1, 1, 0))
            if b == 0:
                out.append((f"{p}.downsample.0", f"{p}.downsample.1", width * 4, cin, 1, s, 0))
            cin = width * 4
    return out


def key_shapes(E):
    """{key: shape} of torchvision's resnet50 state dict with an E-way fc, under `resnet.`."""
    ks = {}
    for ck, bk, cout, cin, k, _s, _p in conv_bn_specs():
        ks[f"resnet.{ck}.weight"] = (cout, cin, k, k)
        for nm in ("weight", "bias", "running_mean", "running_var"):
            ks[f"resnet.{bk}.{nm}"] = (cout,)
        ks[f"resnet.{bk}.num_batches_tracked"] = ()
    ks["resnet.fc.weight"] = (E, 2048)
    ks["resnet.fc.bias"] = (E,)
    return ks


def make_state(E, seed=0, dtype=torch.float32):
    """Seeded weights: Kaiming-normal convolutions (fan_out, ReLU gain), gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1), running_mean ~
    N(0, 0.1), running_var ~ U(0.5, 1.5), fc.weight ~ N(0, 1e-4 / 2048) (the pooled features of such a
    network are of order 100, so the fc term is of order 1), fc.bias = 4 * arange(E) (well separated logits).  Floating
    tensors are rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for ck, bk, cout, cin, k, _s, _p in conv_bn_specs():
        sd[f"resnet.{ck}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5
        sd[f"resnet.{bk}.weight"] = torch.rand(cout, generator=g) + 0.5
        sd[f"resnet.{bk}.bias"] = torch.randn(cout, generator=g) * 0.1
        sd[f"resnet.{bk}.running_mean"] = torch.randn(cout, generator=g) * 0.1
        sd[f"resnet.{bk}.running_var"] = torch.rand(cout, generator=g) + 0.5
        sd[f"resnet.{bk}.num_batches_tracked"] = torch.tensor(7, dtype=torch.long)
    sd["resnet.fc.weight"] = torch.randn(E, 2048, generator=g) * (0.01 * 2048 ** -0.5)
    sd["resnet.fc.bias"] = 4.0 * torch.arange(E, dtype=torch.float32)
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def forward(sd, pixels, storage=None):
    """-> (logits [n, E], weights [n, E]) as float64 CPU tensors.  storage None: float64 throughout; storage = a dtype: emulated."""
    emu = storage is not None
    wt = torch.float32 if emu else torch.float64

    def rnd(t):
        return t.to(storage).to(wt) if emu else t

    def get(k):
        return sd["resnet." + k].detach().cpu().to(wt)

    def affine(bk):
        scale = get(bk + ".weight") / torch.sqrt(get(bk + ".running_var") + EPS)
        return scale, get(bk + ".bias") - get(bk + ".running_mean") * scale

    def conv(x, ck, bk, stride, pad, identity=None, relu=True):
        scale, shift = affine(bk)
        y = F.conv2d(x, get(ck + ".weight"), None, stride, pad) * scale[None, :, None, None] + shift[None, :, None, None]
        if identity is not None:
            y = y + identity
        return rnd(F.relu(y) if relu else y)

    x = rnd(pixels.detach().cpu().to(torch.float32).to(wt))
    x = conv(x, "conv1", "bn1", 2, 3)
    x = F.max_pool2d(x, 3, 2, 1)
    for li, (_width, blocks, stride) in enumerate(LAYERS):
        for b in range(blocks):
            p = f"layer{li + 1}.{b}"
            s = stride if b == 0 else 1
            identity = conv(x, f"{p}.downsample.0", f"{p}.downsample.1", s, 0, relu=False) if b == 0 else x
            y = conv(x, f"{p}.conv1", f"{p}.bn1", 1, 0)
            y = conv(y, f"{p}.conv2", f"{p}.bn2", s, 1)
            x = conv(y, f"{p}.conv3", f"{p}.bn3", 1, 0, identity=identity)
    pooled = x.mean(dim=(2, 3))
    logits = rnd(pooled @ get("fc.weight").t() + get("fc.bias"))
    weights = rnd(torch.softmax(logits, dim=-1))
    return logits.double(), weights.double()
