"""The MoE gating network without a GPU: torchvision's ResNet-50 key set and parameter count, the HF-layout round trip, how the MoE
modalities pick the gate up from `gating_path`, that the gate stays frozen, argument validation of the convolution entry points
before any launch, and that the bf16 convolution kernel was built without scratch."""
import json
import os
import re
import warnings

import pytest
import torch

from tests import gating_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gate(E=5, **kw):
    from multimeditron_amd.model.modalities.gating import GatingNetwork, GatingNetworkConfig
    return GatingNetwork(GatingNetworkConfig(num_classes=E, **kw))


def test_key_set_and_counts():
    E = 5
    sd = _gate(E).state_dict()
    want = GR.key_shapes(E)
    assert len(want) == 320 and len(sd) == 320
    assert set(sd) == set(want), sorted(set(sd) ^ set(want))[:8]
    for k, shape in want.items():
        assert tuple(sd[k].shape) == tuple(shape), k
        assert sd[k].dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
    g = _gate(E)
    params, bufs = dict(g.named_parameters()), dict(g.named_buffers())
    assert len(params) == 161 and len(bufs) == 159
    assert sum(p.numel() for p in params.values()) == 23_508_032 + 2048 * E + E
    # blocks per stage 3, 4, 6, 3; the stride of a stage's first bottleneck on its 3x3 convolution (torchvision v1.5)
    r = g.resnet
    assert [len(getattr(r, f"layer{i}")) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    for i in (2, 3, 4):
        b0 = getattr(r, f"layer{i}")[0]
        assert (b0.conv1.stride, b0.conv2.stride, b0.conv3.stride, b0.downsample[0].stride) == (1, 2, 1, 2)
    assert r.layer1[0].conv2.stride == 1 and r.layer1[0].downsample is not None and r.layer1[1].downsample is None


def _write_gate(path, E=3, class_names=None, dtype=torch.float32):
    g = _gate(E, top_k=2, class_names=class_names or [])
    g.load_state_dict(GR.make_state(E, seed=4, dtype=dtype))
    g.save_pretrained(str(path))
    return g


def test_round_trip(tmp_path):
    from multimeditron_amd.model.modalities.gating import GatingNetwork
    g = _write_gate(tmp_path / "gate", class_names=["b", "c", "a"])
    assert sorted(os.listdir(tmp_path / "gate")) == ["config.json", "model.safetensors"]
    cfg = json.load(open(tmp_path / "gate" / "config.json"))
    assert cfg["model_type"] == "gating_network" and cfg["num_classes"] == 3 and cfg["top_k"] == 2 and cfg["class_names"] == ["b", "c", "a"]
    assert "image_processor_path" in cfg
    h = GatingNetwork.from_pretrained(str(tmp_path / "gate"))
    assert h.config == g.config and h.top_k == 2
    a, b = g.state_dict(), h.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert int(b["resnet.bn1.num_batches_tracked"]) == 7
    assert not h.training and not any(p.requires_grad for p in h.parameters())


def _modality(tmp_path, gating_path, pep=False, names=("a", "b", "c"), **kw):
    from multimeditron_amd.model.modalities import MOEImageConfig, MOEImageConfigPEP, MOEImageModality, MOEImageModalityPEP
    vis = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1, image_size=32, patch_size=16)
    dirs = []
    for nm in names:
        d = os.path.join(str(tmp_path), nm)
        os.makedirs(d, exist_ok=True)
        json.dump({"vision_config": vis}, open(os.path.join(d, "config.json"), "w"))
        dirs.append(d)
    cfg = (MOEImageConfigPEP if pep else MOEImageConfig)(hidden_size=64, expert_clip_names=dirs, image_processor=dirs[0],
                                                        gating_path=gating_path, top_k_experts=len(names))
    return (MOEImageModalityPEP if pep else MOEImageModality)(cfg, dtype=torch.float32, device="cpu", **kw), dirs


@pytest.mark.parametrize("pep", [False, True])
def test_modality_builds_the_gate_from_gating_path(tmp_path, pep):
    from multimeditron_amd.model.modalities.gating import GatingNetwork
    _write_gate(tmp_path / "gate")
    m, _ = _modality(tmp_path, str(tmp_path / "gate"), pep)
    assert isinstance(m.gating_network, GatingNetwork)
    sd = m.state_dict()
    assert "gating_network.resnet.conv1.weight" in sd and "gating_network.resnet.bn1.num_batches_tracked" in sd
    assert sum(k.startswith("gating_network.") for k in sd) == 320
    assert m._gating_to_expert_perm.tolist() == [0, 1, 2]
    # "stub" (not a directory with a config.json) leaves the plug empty; an argument wins over the path
    m2, _ = _modality(tmp_path, "stub", pep)
    assert m2.gating_network is None
    os.makedirs(tmp_path / "empty", exist_ok=True)
    m3, _ = _modality(tmp_path, str(tmp_path / "empty"), pep)
    assert m3.gating_network is None
    fn = lambda px: None
    m4, _ = _modality(tmp_path, str(tmp_path / "gate"), pep, gating_network=fn)
    assert m4.gating_network is fn


@pytest.mark.parametrize("pep", [False, True])
def test_class_names_give_the_expert_permutation(tmp_path, pep):
    m, dirs = _modality(tmp_path, "stub", pep)
    _write_gate(tmp_path / "gate", class_names=[dirs[2], dirs[0], dirs[1]])
    m, _ = _modality(tmp_path, str(tmp_path / "gate"), pep)
    assert m._gating_to_expert_perm.tolist() == [2, 0, 1]
    _write_gate(tmp_path / "gate2", class_names=[dirs[2], "nobody", dirs[1]])
    with pytest.raises(ValueError, match="not found in expert_clip_names"):
        _modality(tmp_path, str(tmp_path / "gate2"), pep)


@pytest.mark.parametrize("pep", [False, True])
def test_gate_stays_frozen(tmp_path, pep):
    _write_gate(tmp_path / "gate")
    m, _ = _modality(tmp_path, str(tmp_path / "gate"), pep)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.train()
        m.unfreeze_modality_embedder()
        assert not any(p.requires_grad for p in m.gating_network.parameters())
        assert not m.gating_network.training and not any(mod.training for mod in m.gating_network.modules())
        assert all(p.requires_grad for p in m.experts.parameters()) and m.training
        m.unfreeze_all()
        assert not any(p.requires_grad for p in m.gating_network.parameters())
        m.freeze_modality_embedder()
        m.train()
        assert not m.gating_network.training


def test_argument_validation_without_launch():
    from multimeditron_amd import _lib
    L = _lib.lib()
    OK_PTR = 4096

    def conv(dtype=0, x=OK_PTR, Cin=64, w=OK_PTR, Cout=64, R=3, stride=1, pad=1, y=OK_PTR, res=None):
        return L.mm_conv2d_nhwc_fwd(dtype, x, 2, 9, 7, Cin, w, Cout, R, stride, pad, OK_PTR, OK_PTR, res, 1, y, None)

    ARG, ALIGN, UNSUP = -1, -2, -3
    assert conv(Cin=12) == ALIGN
    assert conv(Cout=72) == ALIGN
    assert conv(R=5) == UNSUP
    assert conv(stride=3) == UNSUP
    assert conv(pad=2) == UNSUP
    assert conv(x=OK_PTR + 8) == ALIGN and conv(y=OK_PTR + 2) == ALIGN and conv(w=OK_PTR + 4) == ALIGN and conv(res=OK_PTR + 8) == ALIGN
    assert conv(x=None) == ARG and conv(dtype=7) == UNSUP
    assert conv(dtype=1, Cin=12) == ALIGN and conv(dtype=1, R=5) == UNSUP

    def head(E=5, top_k=1, C=2048, x=OK_PTR):
        return L.mm_gate_head(0, x, 3, 6, C, OK_PTR, OK_PTR, E, top_k, OK_PTR, OK_PTR, OK_PTR, None)

    assert head(E=65) == UNSUP
    assert head(top_k=0) == ARG and head(top_k=6) == ARG
    assert head(C=2052) == ALIGN and head(x=OK_PTR + 2) == ALIGN and head(C=16384) == UNSUP
    assert L.mm_nchw_to_nhwc(0, OK_PTR, 2, 3, 9, 7, 6, OK_PTR, None) == ALIGN
    assert L.mm_nchw_to_nhwc(0, OK_PTR, 2, 3, 9, 7, 2, OK_PTR, None) == ARG
    assert L.mm_maxpool2d_nhwc(0, OK_PTR, 2, 9, 7, 12, OK_PTR, None) == ALIGN


def test_bf16_conv_kernel_uses_no_scratch():
    path = os.path.join(ROOT, "multimeditron_amd", "csrc", "build", "mm_conv.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    name, seen = None, 0
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name and "conv_bf16_kernel" in name:
            assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes/lane of scratch"
            seen += 1
    assert seen == 1
