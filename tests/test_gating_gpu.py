"""The MoE gating network on the GPU (model/modalities/gating.py on csrc/mm_conv.hip).

Whole gate: logits and softmax weights of the 56-launch forward against the float64 forward of tests/gating_ref.py on the same
storage-rounded weights.  The bound is the error of gating_ref's EMULATED forward (fp32 arithmetic, the kernels' documented
rounding points in the storage type) times 2: the factor covers a different accumulation order at identical rounding points.
Measured on the MI355X, max|logits - fp64| / max|fp64| of the kernels (of the emulated forward):
    bf16 2x3x64x64 2.03e-3 (2.46e-3), 2x3x96x64 1.79e-3 (1.79e-3), 1x3x224x224 2.32e-3 (2.32e-3);
    fp32 2x3x64x64 1.16e-7 (1.82e-7), 2x3x96x64 1.27e-7 (2.14e-7).
In the modality: a gate built from `gating_path` equals the same modality with a plug that returns that gate's outputs, bit for bit;
`class_names` reorder the weights; a checkpoint saved from the model carries the gate and reloads strictly; no gate tensor gets a
gradient."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

from tests import gating_ref as GR

pytestmark = pytest.mark.gpu
E = 5
SEED = 0


def _gate(dtype, top_k=1, class_names=None):
    from multimeditron_amd.model.modalities.gating import GatingNetwork, GatingNetworkConfig
    g = GatingNetwork(GatingNetworkConfig(num_classes=E, top_k=top_k, class_names=class_names or []))
    sd = GR.make_state(E, SEED, dtype)
    g.to(dtype=dtype)
    g.load_state_dict(sd)
    return g.to("cuda"), sd


_REF = {}


def _reference(dtype, shape):
    """(fp64 logits, fp64 weights, emulated logits, emulated weights) on the CPU, computed once per (dtype, shape)."""
    key = (dtype, shape)
    if key not in _REF:
        sd = GR.make_state(E, SEED, dtype)
        px = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
        _REF[key] = (px,) + GR.forward(sd, px) + GR.forward(sd, px, dtype)
    return _REF[key]


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, (2, 3, 64, 64)), (torch.float32, (2, 3, 64, 64)),
                                         (torch.bfloat16, (2, 3, 96, 64)), (torch.float32, (2, 3, 96, 64)),      # final map 3x2
                                         (torch.bfloat16, (1, 3, 224, 224))],                                    # error bound only
                         ids=["bf16-64x64", "f32-64x64", "bf16-96x64", "f32-96x64", "bf16-224x224"])
def test_whole_gate(dtype, shape):
    px, l64, w64, lem, wem = _reference(dtype, shape)
    err_emu_abs = float((lem - l64).abs().max())
    err_emu = err_emu_abs / float(l64.abs().max())
    werr_emu = float((wem - w64).abs().max())
    full = shape[-1] != 224
    if full:        # the top-k comparison below is meaningful only when the fp64 logits are further apart than the rounding noise
        srt = l64.sort(-1).values
        gap = float((srt[:, 1:] - srt[:, :-1]).min())
        assert gap > 4 * err_emu_abs, (gap, err_emu_abs)
    gate, _ = _gate(dtype, top_k=E)
    logits, topk, weights = gate(px.cuda())
    torch.cuda.synchronize()
    assert logits.dtype == dtype and weights.dtype == dtype and topk.dtype == torch.int64 and topk.shape == (shape[0], E)
    err = float((logits.double().cpu() - l64).abs().max()) / float(l64.abs().max())
    werr = float((weights.double().cpu() - w64).abs().max())
    print(f"gate {dtype} {shape}: logits err {err:.4g} (emulated {err_emu:.4g}), weights err {werr:.4g} (emulated {werr_emu:.4g})")
    assert err <= 2 * err_emu, (err, err_emu)
    if full:
        assert werr <= 2 * werr_emu, (werr, werr_emu)
        assert torch.equal(topk.cpu(), l64.topk(E, dim=-1).indices)
        one, _ = _gate(dtype, top_k=1)
        assert torch.equal(one(px.cuda())[1].cpu(), l64.topk(1, dim=-1).indices)


def test_repack_follows_the_weights():
    """scale / shift and the packed filters are rebuilt after a weight load, not per forward."""
    gate, sd = _gate(torch.bfloat16)
    px = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    a = gate(px)[0].clone()
    packed = gate._packed
    assert gate(px)[0].equal(a) and gate._packed is packed
    sd2 = dict(sd)
    sd2["resnet.fc.bias"] = sd["resnet.fc.bias"] + 1
    sd2["resnet.bn1.running_var"] = sd["resnet.bn1.running_var"] * 2
    gate.load_state_dict(sd2)
    b = gate(px)[0]
    assert gate._packed is not packed and not b.equal(a)
    with torch.no_grad():
        gate.resnet.bn1.running_var.copy_(sd["resnet.bn1.running_var"].cuda())
        gate.resnet.fc.bias.copy_(sd["resnet.fc.bias"].cuda())
    assert gate(px)[0].equal(a)


# ---- in the modality -------------------------------------------------------------------------------------------------------
def _fixture(golden_dir, pep):
    stem = "tiny_moe_clip_pep" if pep else "tiny_moe_clip"
    meta = json.load(open(os.path.join(golden_dir, stem + ".meta.json")))
    return meta, load_file(os.path.join(golden_dir, stem + ".weights.safetensors")), load_file(os.path.join(golden_dir, stem + ".vectors.safetensors"))


def _write_gate(path, n_exp, dtype, class_names=None):
    from multimeditron_amd.model.modalities.gating import GatingNetwork, GatingNetworkConfig
    g = GatingNetwork(GatingNetworkConfig(num_classes=n_exp, top_k=1, class_names=class_names or []))
    g.load_state_dict(GR.make_state(n_exp, SEED, dtype))
    g.save_pretrained(str(path))


def _build(meta, w, tmp, dtype, gating_path, gating_network=None, fusion="weighted_average"):
    from multimeditron_amd.model.modalities import MOEImageConfig, MOEImageModality
    if meta.get("per_expert_projection"):
        from multimeditron_amd.model.modalities import MOEImageConfigPEP as MOEImageConfig, MOEImageModalityPEP as MOEImageModality
    from multimeditron_amd.nn import FlatParams
    n_exp = meta["num_experts"]
    dirs = []
    for e in range(n_exp):
        d = os.path.join(str(tmp), f"clip{e}")
        os.makedirs(d, exist_ok=True)
        json.dump({"vision_config": meta["vision"]}, open(os.path.join(d, "config.json"), "w"))
        dirs.append(d)
    cfg = MOEImageConfig(hidden_size=meta["hidden_size"], expert_clip_names=dirs, image_processor=dirs[0], gating_path=gating_path,
                         top_k_experts=n_exp, generalist_idx=meta["generalist_idx"], fusion_method=fusion,
                         cross_attn_heads=meta["cross_attn_heads"])
    m = MOEImageModality(cfg, dtype=dtype, device="cuda", gating_network=gating_network)
    own = {k: p for k, p in m.named_parameters() if not k.startswith("gating_network.")}
    with torch.no_grad():
        for k, p in own.items():
            p.copy_(w[k].to(dtype).reshape(p.shape))
    FlatParams([(k, p, "projector" if k.startswith("projector") else "encoder") for k, p in own.items()], "cuda", dtype)
    for p in own.values():
        p.requires_grad_(True)
    return m.eval(), dirs


@pytest.mark.parametrize("pep", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_modality_with_the_real_gate(golden_dir, tmp_path, dtype, pep):
    from multimeditron_amd.model.modalities.gating import GatingNetwork
    meta, w, v = _fixture(golden_dir, pep)
    n_exp = meta["num_experts"]
    _write_gate(tmp_path / "gate", n_exp, dtype)
    m, dirs = _build(meta, w, tmp_path, dtype, str(tmp_path / "gate"), fusion="cross_attn")
    assert isinstance(m.gating_network, GatingNetwork) and m.gating_network.dtype == dtype and m.gating_network.device.type == "cuda"
    px = [v["pixels"][i] for i in range(v["pixels"].shape[0])]
    y = m(px)
    gate = m.gating_network
    plug, _ = _build(meta, w, tmp_path, dtype, "stub", gating_network=lambda p: gate(p), fusion="cross_attn")
    assert not isinstance(plug.gating_network, torch.nn.Module)
    assert torch.equal(y, plug(px))
    # the gate's weights are not constant over the experts, and they reach the output
    wts = gate(torch.stack(px).cuda())[2].float()
    assert float((wts.max(-1).values - wts.min(-1).values).min()) > 0.1
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is None and not p.requires_grad for p in gate.parameters())
    assert any(p.grad is not None for k, p in m.named_parameters() if not k.startswith("gating_network."))
    # class_names in a non-identity order: gate_weights returns the weights in EXPERT order
    if not pep:
        order = [2, 0, 1] + list(range(3, n_exp)) if n_exp >= 3 else list(range(n_exp))[::-1]
        _write_gate(tmp_path / "gate_named", n_exp, dtype, class_names=[dirs[i] for i in order])
        named, _ = _build(meta, w, tmp_path, dtype, str(tmp_path / "gate_named"))
        assert named._gating_to_expert_perm.tolist() == order
        gw = named.gate_weights(torch.stack(px).cuda())
        assert torch.equal(gw, wts.index_select(-1, torch.tensor(order, device="cuda")))


def test_checkpoint_carries_the_gate(tmp_path):
    """A model built from a recipe that names a gate directory saves the gate's 320 tensors under the reference's names and reloads
    them strictly (integer num_batches_tracked included): the reloaded model reproduces the modality forward bit for bit, also for
    gate weights that differ from the directory's."""
    from tests.test_training_config_cpu import ATTACH, make_tokenizer
    from multimeditron_amd.model.model import MultiModalModelForCausalLM
    from multimeditron_amd.train import from_training_config
    llm = os.path.join(str(tmp_path), "llm")
    os.makedirs(llm, exist_ok=True)
    json.dump(dict(model_type="llama", hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                   num_key_value_heads=1, head_dim=64, vocab_size=32, rms_norm_eps=1e-5, tie_word_embeddings=False,
                   rope_parameters={"rope_type": "default", "rope_theta": 10000.0}), open(os.path.join(llm, "config.json"), "w"))
    clips = []
    for i in range(3):
        d = os.path.join(str(tmp_path), f"clip{i}")
        os.makedirs(d, exist_ok=True)
        json.dump({"vision_config": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=32,
                                         patch_size=16)}, open(os.path.join(d, "config.json"), "w"))
        json.dump({"size": {"shortest_edge": 32}, "crop_size": {"height": 32, "width": 32}}, open(os.path.join(d, "preprocessor_config.json"), "w"))
        clips.append(d)
    _write_gate(tmp_path / "gate", 3, torch.bfloat16)
    recipe = {
        "base_llm": llm, "base_model": None, "attachment_token": ATTACH, "tokenizer_type": "llama", "token_size": 128,
        "loaders": [{"loader_type": "raw-image", "modality_type": "image"}],
        "modalities": [{"model_type": "moe_meditron_clip_shared", "image_processor": clips[0], "hidden_size": 128, "expert_clip_names": clips,
                        "generalist_idx": -1, "gating_path": str(tmp_path / "gate"), "fusion_method": "weighted_average", "top_k_experts": 3,
                        "cross_attn_heads": 2}],
        "training_mode": "FULL",
        "training_args": {"learning_rate": 1.0e-3, "bf16": True, "per_device_train_batch_size": 2, "gradient_accumulation_steps": 1,
                          "max_steps": 5, "max_grad_norm": 1.0, "lr_scheduler_type": "constant", "weight_decay": 0.01},
    }
    torch.manual_seed(0)
    with pytest.warns(UserWarning, match="gating network stays frozen"):
        setup = from_training_config(recipe, make_tokenizer(), device="cuda", dtype="bfloat16")
    model, tr = setup.model, setup.trainer
    try:
        mod = model.modalities_by_type["image"]
        gate = mod.gating_network
        # FULL mode: the towers train, the gate does not, and it is in neither the flat buffer nor the optimiser
        assert not any(p.requires_grad for p in gate.parameters()) and not gate.training
        assert all(getattr(p, "_mm_flat", None) is None for p in gate.parameters())
        assert any(p.requires_grad for p in mod.experts.parameters())
        ref_sd = GR.make_state(3, SEED, torch.bfloat16)
        assert torch.equal(gate.resnet.conv1.weight.cpu(), ref_sd["resnet.conv1.weight"])      # not re-initialised by the model's init
        with torch.no_grad():
            gate.resnet.fc.bias.add_(1.5)
            gate.resnet.layer1[0].bn1.running_mean.add_(0.25)
            gate.resnet.bn1.num_batches_tracked.fill_(11)
        model.eval()
        px = [torch.randn(3, 32, 32, generator=torch.Generator().manual_seed(i)) for i in range(2)]
        with torch.no_grad():
            y = mod(px).clone()
        model.save_pretrained(str(tmp_path / "ckpt"))
    finally:
        tr.close()
    saved = load_file(str(tmp_path / "ckpt" / "model.safetensors"))
    gk = [k for k in saved if ".gating_network.resnet." in k]
    assert len(gk) == 320 and saved["modalities_with_projection.0.gating_network.resnet.bn1.num_batches_tracked"].dtype == torch.int64
    model2 = MultiModalModelForCausalLM.from_pretrained(str(tmp_path / "ckpt"), device="cuda", strict=True).eval()
    model2.pack_parameters()
    mod2 = model2.modalities_by_type["image"]
    assert int(mod2.gating_network.resnet.bn1.num_batches_tracked) == 11
    with torch.no_grad():
        assert torch.equal(mod2(px), y)
