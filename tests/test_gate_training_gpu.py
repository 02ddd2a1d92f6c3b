"""The trainable MoE gate on the GPU (model/modalities/gating.py: `set_trainable`, `_GateTrainFn`).

No test here compares a gradient of the whole network, or of a block, with an independently computed run: single ReLU flips and
the BatchNorm backward's cancellation make torch's own bf16 gradient differ from float64 by 100 %.  Instead every backward launch is
checked LOCALLY (tests/conv_train_check.py, c = 2) against the operands it read, collected through `stages`, and the wiring
between the launches is checked bit for bit.  The train-mode FORWARD is well conditioned and is compared as a whole: logits against
a float64 forward with batch statistics on the same rounded weights, within 8 x the error of the emulated restatement (fp32
arithmetic, the documented rounding points in T); the factor is for summation order.  The test is inconclusive (fails) if 8 x that
floor exceeds 2e-2 (bf16) / 1e-5 (f32)."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_train_check as TC
from tests import gating_ref as GR
from tests.kernel_check import check_bits

pytestmark = pytest.mark.gpu
E = 4
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "f32"]


def _gate(dtype, trainable=True):
    from multimeditron_amd.model.modalities.gating import GatingNetwork, GatingNetworkConfig
    g = GatingNetwork(GatingNetworkConfig(num_classes=E, top_k=1))
    g.to(dtype=dtype)
    g.load_state_dict(GR.make_state(E, 0, dtype))
    g = g.to("cuda")
    if trainable:
        g.set_trainable(True).train()
    return g


def _train_forward_ref(sd, pixels, storage=None):
    """tests/gating_ref.forward with BATCH statistics: float64, or (storage = T) fp32 arithmetic with the rounding points of the
    training path: z = T(conv), y = T(act((z - mean) invstd gamma + beta (+ identity))) from the stored z."""
    emu = storage is not None
    wt = torch.float32 if emu else torch.float64
    rnd = (lambda t: t.to(storage).to(wt)) if emu else (lambda t: t)
    get = lambda k: sd["resnet." + k].detach().cpu().to(wt)

    def unit(x, ck, bk, stride, pad, identity=None, relu=True):
        z = rnd(F.conv2d(x, get(ck + ".weight"), None, stride, pad))
        mean = z.mean(dim=(0, 2, 3), keepdim=True)
        var = ((z - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        y = (z - mean) / torch.sqrt(var + GR.EPS) * get(bk + ".weight")[None, :, None, None] + get(bk + ".bias")[None, :, None, None]
        if identity is not None:
            y = y + identity
        return rnd(F.relu(y) if relu else y)

    x = rnd(pixels.detach().cpu().to(torch.float32).to(wt))
    x = F.max_pool2d(unit(x, "conv1", "bn1", 2, 3), 3, 2, 1)
    for li, (_w, blocks, stride) in enumerate(GR.LAYERS):
        for b in range(blocks):
            p = f"layer{li + 1}.{b}"
            s = stride if b == 0 else 1
            identity = unit(x, f"{p}.downsample.0", f"{p}.downsample.1", s, 0, relu=False) if b == 0 else x
            y = unit(unit(x, f"{p}.conv1", f"{p}.bn1", 1, 0), f"{p}.conv2", f"{p}.bn2", s, 1)
            x = unit(y, f"{p}.conv3", f"{p}.bn3", 1, 0, identity=identity)
    logits = rnd(x.mean(dim=(2, 3)) @ get("fc.weight").t() + get("fc.bias"))
    return logits.double()


_RUN = {}


def _run(dtype):
    """one training forward + backward of the gate on n = 4 images of 64 x 64 (layer4 is 2 x 2), everything recorded; shared"""
    if dtype not in _RUN:
        gate = _gate(dtype)
        px = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(1))
        stages = {}
        logits, topk, weights = gate(px.cuda(), stages=stages)
        dweights = torch.randn(4, E, generator=torch.Generator().manual_seed(2)).to(dtype).cuda()
        weights.backward(dweights)
        torch.cuda.synchronize()
        _RUN[dtype] = (gate, px, stages, logits, topk, weights)
    return _RUN[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_train_forward_against_float64(dtype):
    gate, px, stages, logits, topk, weights = _run(dtype)
    sd = GR.make_state(E, 0, dtype)
    l64 = _train_forward_ref(sd, px)
    lem = _train_forward_ref(sd, px, dtype)
    rel = lambda a: float((a - l64).norm() / l64.norm())
    floor, err = rel(lem), rel(logits.detach().double().cpu())
    print(f"train-mode gate {dtype}: logits err {err:.4g}, emulated floor {floor:.4g}")
    assert 8 * floor <= (2e-2 if dtype == torch.bfloat16 else 1e-5), f"inconclusive: floor {floor:.4g}"
    assert err <= 8 * floor, (err, floor)
    assert logits.grad_fn is not None and weights.grad_fn is not None and logits.dtype == dtype and topk.dtype == torch.int64
    assert torch.equal(topk.cpu(), l64.topk(1, dim=-1).indices)
    for _key, _c, bn in gate.units():
        assert int(bn.num_batches_tracked) == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_backward_launch_locally(dtype):
    gate, px, st, *_ = _run(dtype)
    units = gate.units()
    for key, conv, bn in units:
        x, z, y = st[key + ".x"], st[key + ".z"], st[key + ".y"]
        M, C = z.numel() // z.shape[-1], z.shape[-1]
        relu = not key.endswith("downsample.0")
        ref = TC.bn_bwd_reference(st[key + ".dy"].reshape(M, C), y.reshape(M, C), z.reshape(M, C), st[key + ".mean"], st[key + ".invstd"],
                                  bn.weight.detach(), relu)
        TC.check(f"{key} dz", st[key + ".dz"].reshape(M, C), *ref["dz"], "gate.bn.dz", dtype)
        TC.check(f"{key} dgamma", st[key + ".dgamma"], *ref["dgamma"], "gate.bn.dgamma", dtype)
        TC.check(f"{key} dbeta", st[key + ".dbeta"], *ref["dbeta"], "gate.bn.dbeta", dtype)
        if key.endswith("conv3"):
            TC.check(f"{key} dres", st[key + ".dres"].reshape(M, C), *ref["dres"], "gate.bn.dres", dtype)
        w = conv.weight.detach().permute(0, 2, 3, 1)
        if w.shape[3] % 8:
            w = F.pad(w, (0, 8 - w.shape[3] % 8))
        TC.check(f"{key} dw", st[key + ".dw"], *TC.wgrad_reference(st[key + ".dz"], x, conv.k, conv.stride, conv.pad), "gate.wgrad", dtype)
        if key == "conv1":
            assert bool((st[key + ".dw"][..., 3:].float() == 0).all())
            continue
        addend = None
        if key.endswith(".conv1"):                              # the join: dres of the block's conv3, or its downsample's dx
            blk = key[:-len("conv1")]
            addend = st[blk + "downsample.0.dx"] if (blk + "downsample.0.dx") in st else st[blk + "conv3.dres"]
        TC.check(f"{key} dx", st[key + ".dx"], *TC.dgrad_reference(st[key + ".dz"], w.contiguous(), x.shape[1], x.shape[2], conv.stride,
                                                                     conv.pad, addend), "gate.dgrad", dtype)
    TC.check("pool dx", st["pool.dx"], *TC.maxpool_bwd_reference(st["pool.x"], st["layer1.0.conv1.dx"]), "gate.pool", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wiring(dtype):
    gate, px, st, *_ = _run(dtype)
    keys = [k for k, _c, _b in gate.units()]
    blocks = sorted({k[:-len("conv1")] for k in keys if k.endswith(".conv1")})
    for bi, blk in enumerate(blocks):
        # one consumer: the unit's dy is that consumer's dx, bit for bit
        check_bits(blk + "conv2.dy", st[blk + "conv2.dy"], st[blk + "conv3.dx"])
        check_bits(blk + "conv1.dy", st[blk + "conv1.dy"], st[blk + "conv2.dx"])
        if blk + "downsample.0.dy" in st:
            check_bits(blk + "downsample.0.dy", st[blk + "downsample.0.dy"], st[blk + "conv3.dres"])
        # a block output's dy is the next block's joined conv1 dx: ONE rounding of (conv1's data gradient + the identity path's)
        if bi + 1 < len(blocks):
            check_bits(blk + "conv3.dy", st[blk + "conv3.dy"], st[blocks[bi + 1] + "conv1.dx"])
    check_bits("conv1.dy", st["conv1.dy"], st["pool.dx"])
    check_bits("last block dy", st[blocks[-1] + "conv3.dy"], st["head.dx"])
    # the parameter gradients are the recorded dw / dgamma / dbeta in torchvision's shapes
    params = dict(gate.resnet.named_parameters())
    assert len(params) == 161 and all(p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == dtype for p in params.values())
    for key, conv, bn in gate.units():
        check_bits(key + ".weight.grad", conv.weight.grad, st[key + ".dw"][..., :conv.weight.shape[1]].permute(0, 3, 1, 2).contiguous())
        check_bits(key + " bn.weight.grad", bn.weight.grad, st[key + ".dgamma"])
        check_bits(key + " bn.bias.grad", bn.bias.grad, st[key + ".dbeta"])
    # the head in torch: fc gradients from the recorded d(logits)
    dl, last = st["head.dl"], st["head.x"]
    pooled = last.reshape(last.shape[0], -1, last.shape[-1]).float().mean(1)
    check_bits("fc.weight.grad", params["fc.weight"].grad, (dl.t() @ pooled).to(dtype))
    check_bits("fc.bias.grad", params["fc.bias"].grad, dl.sum(0).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eval_and_frozen_forward_unchanged(dtype):
    """not trainable, or trainable but in eval mode: the frozen forward's bits, no grad_fn"""
    px = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    want = _gate(dtype, trainable=False)(px)
    g = _gate(dtype)
    g.eval()
    got = g(px)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert got[0].grad_fn is None
    g.train()
    assert g(px)[0].grad_fn is not None
    g.eval()                                                    # the running statistics moved: the eval forward follows them
    assert not torch.equal(g(px)[0], want[0])


# ---- in the modalities -------------------------------------------------------------------------------------------------------------
def _modality(golden_dir, tmp_path, pep, fusion, train_gate, dtype=torch.bfloat16):
    from tests.test_gating_gpu import _build, _fixture, _write_gate
    meta, w, v = _fixture(golden_dir, pep)
    if not os.path.isdir(tmp_path / "gate"):
        _write_gate(tmp_path / "gate", meta["num_experts"], dtype)
    m, _ = _build(meta, w, tmp_path, dtype, str(tmp_path / "gate"), fusion=fusion)
    m.config.train_gate = train_gate
    m.train()
    m.unfreeze_modality_embedder()
    m.unfreeze_projection()
    return m, [v["pixels"][i] for i in range(v["pixels"].shape[0])]


@pytest.mark.parametrize("pep", [False, True], ids=["shared", "pep"])
@pytest.mark.parametrize("fusion", ["weighted_average", "cross_attn", "sequence_append"])
def test_gate_gradients_through_the_modalities(golden_dir, tmp_path, pep, fusion, monkeypatch):
    import warnings
    from multimeditron_amd import functional as Fm
    from multimeditron_amd.model.modalities.image_modality_moe import _FrozenGate
    monkeypatch.setattr(_FrozenGate, "_warned_frozen_gate", True)       # the once-per-process warning is left for the tests that pin it
    grads = {}
    for train_gate in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m, px = _modality(golden_dir, tmp_path, pep, fusion, train_gate)
        gate = m.gating_network
        if not train_gate:                                      # frozen, but in the SAME (train) mode: batch statistics, no gradient
            gate._trainable = True
            gate.train()
            for p in gate.parameters():
                p.requires_grad = False
        torch.manual_seed(0)                                    # the dropout streams of cross_attn: same key, same call counter
        monkeypatch.setattr(Fm, "_dropout_calls", 0)
        y = m(px)
        y.float().square().mean().backward()
        torch.cuda.synchronize()
        grads[train_gate] = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    on, off = grads[True], grads[False]
    gk = [k for k in on if k.startswith("gating_network.")]
    assert len(gk) == 161
    if fusion == "sequence_append":                             # the gate's output is unused there
        assert all(on[k] is None for k in gk)
    else:
        assert all(on[k] is not None and bool(torch.isfinite(on[k]).all()) for k in gk)
        assert float(on["gating_network.resnet.fc.weight"].float().abs().max()) > 0
        for k in gk:
            if ".bn" in k and k.endswith(".weight") or k.endswith("downsample.1.weight"):
                assert float(on[k].float().abs().max()) > 0, k
    assert all(off[k] is None for k in gk)
    for k in on:                                                # the gate's gradient adds a path, it changes none
        if k not in gk and on[k] is not None:
            check_bits(k, on[k], off[k])


@pytest.mark.parametrize("pep", [False, True], ids=["shared", "pep"])
@pytest.mark.parametrize("fusion", ["weighted_average", "cross_attn"])
def test_eval_mode_modality_returns_the_default_bits(golden_dir, tmp_path, pep, fusion, monkeypatch):
    """a `train_gate` modality, unfrozen and then put in eval mode, returns the bits of the default modality"""
    import warnings
    from multimeditron_amd.model.modalities.image_modality_moe import _FrozenGate
    monkeypatch.setattr(_FrozenGate, "_warned_frozen_gate", True)
    out = {}
    for train_gate in (False, True):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m, px = _modality(golden_dir, tmp_path, pep, fusion, train_gate)
        assert m.gating_network.training == train_gate
        m.eval()
        with torch.no_grad():
            out[train_gate] = m(px)
    check_bits("eval output", out[True], out[False])


# ---- in the trainer ------------------------------------------------------------------------------------------------------------------
IMG = 64


def _recipe(tmp_path):
    import json
    from tests.test_gating_gpu import _write_gate
    from tests.test_training_config_cpu import ATTACH
    llm = os.path.join(str(tmp_path), "llm")
    os.makedirs(llm, exist_ok=True)
    json.dump(dict(model_type="llama", hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                   num_key_value_heads=1, head_dim=64, vocab_size=32, rms_norm_eps=1e-5, tie_word_embeddings=False,
                   rope_parameters={"rope_type": "default", "rope_theta": 10000.0}), open(os.path.join(llm, "config.json"), "w"))
    clips = []
    for i in range(3):
        d = os.path.join(str(tmp_path), f"clip{i}")
        os.makedirs(d, exist_ok=True)
        # 64 x 64 images: with the fixture's 32 x 32 and two images, layer4 is 1 x 1 and its BatchNorms see M = 2 rows, where
        # xhat = +-1 and the BatchNorm backward cancels to nothing: no gradient would reach the layers below
        json.dump({"vision_config": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=IMG,
                                         patch_size=16)}, open(os.path.join(d, "config.json"), "w"))
        json.dump({"size": {"shortest_edge": IMG}, "crop_size": {"height": IMG, "width": IMG}}, open(os.path.join(d, "preprocessor_config.json"), "w"))
        clips.append(d)
    if not os.path.isdir(tmp_path / "gate"):
        _write_gate(tmp_path / "gate", 3, torch.bfloat16)
    return {
        "base_llm": llm, "base_model": None, "attachment_token": ATTACH, "tokenizer_type": "llama", "token_size": 128,
        "loaders": [{"loader_type": "raw-image", "modality_type": "image"}],
        "modalities": [{"model_type": "moe_meditron_clip_shared", "image_processor": clips[0], "hidden_size": 128, "expert_clip_names": clips,
                        "generalist_idx": -1, "gating_path": str(tmp_path / "gate"), "fusion_method": "weighted_average", "top_k_experts": 3,
                        "cross_attn_heads": 2, "train_gate": True}],
        "training_mode": "FULL",
        # learning rate 1e-2: one AdamW step moves a weight by about lr.  Half a bf16 ulp is 3.9e-3 for weights in [1, 2) (gamma is
        # U(0.5, 1.5)), so at the fixture recipe's 1e-3 three steps (<= 3e-3) cannot change such a weight's stored bits at all, whatever
        # the code does; at 1e-2 a single step crosses the rounding midpoint of every weight below 2.56
        "training_args": {"learning_rate": 1.0e-2, "bf16": True, "per_device_train_batch_size": 2, "gradient_accumulation_steps": 1,
                          "max_steps": 5, "max_grad_norm": 1.0, "lr_scheduler_type": "constant", "weight_decay": 0.01},
    }


def _batch(model, step):
    import bench
    vocab = model.config.vocab_size
    batch, _ = bench.synthetic_batch(2, 40, 1, (IMG // 16) ** 2, vocab, (vocab - 3, vocab - 2, vocab - 1), 100 + step, "cpu", IMG,
                                     collator_form=True)
    batch["input_ids"].clamp_(max=vocab - 1)
    batch["labels"] = torch.where(batch["labels"] >= 0, batch["labels"].clamp(max=vocab - 1), batch["labels"])
    return batch


def _gate_state(model):
    gate = model.modalities_by_type["image"].gating_network
    return {k: v.detach().clone() for k, v in gate.state_dict().items()}


def _train(tmp_path, steps, overlap=True, save_at=None, resume=None, first_step=0):
    """`steps` optimiser steps of the FULL + train_gate recipe from the same seed -> (gate state dict, flat parameters, start state)"""
    import warnings
    from tests.test_training_config_cpu import make_tokenizer
    from multimeditron_amd.train import from_training_config
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*gating network stays frozen.*")      # a train_gate recipe does not emit it
        setup = from_training_config(_recipe(tmp_path), make_tokenizer(), device="cuda", dtype="bfloat16")
    model, tr = setup.model, setup.trainer
    try:
        if not overlap:                                                 # the update on the compute stream, no per-block events
            tr._wait_optimizer()
            for h in tr._hooks:
                h.remove()
            tr._hooks, tr._blocks, tr.overlap_optimizer = [], [], False
        gate = model.modalities_by_type["image"].gating_network
        assert model.modalities_by_type["image"].config.train_gate is True                 # the recipe key reached the config
        assert len(list(gate.parameters())) == 161
        assert all(getattr(p, "_mm_flat", None) is tr.flat and p.requires_grad for p in gate.parameters())
        assert gate.training
        comps = {seg.component for seg in tr.flat.segments if ".gating_network." in seg.name}
        assert comps == {"gate0"}
        decay = {seg.name.split(".gating_network.resnet.")[1]: seg.decay for seg in tr.flat.segments if ".gating_network." in seg.name}
        assert decay["bn1.weight"] and decay["layer1.0.downsample.1.weight"] and decay["conv1.weight"] and decay["fc.weight"]
        assert not decay["bn1.bias"] and not decay["fc.bias"]                               # HF Trainer's rule
        if resume is not None:
            tr.load_state(resume)
        start = _gate_state(model)
        for step in range(first_step, first_step + steps):
            loss = float(tr.training_step(_batch(model, step)))
            assert loss == loss
            if overlap and step > first_step:
                assert id(gate) not in tr._unfired                     # the gate's pre-hook fired: it waited for its own update
            if save_at is not None and step + 1 == save_at[0]:
                tr.save_state(save_at[1])
                tr._unfired = []                                        # the save waited for every block: nothing is pending next step
        tr.synchronize()
        torch.cuda.synchronize()
        return _gate_state(model), tr.flat.data.detach().clone(), start
    finally:
        tr.close()


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def test_trainer_steps_the_gate(tmp_path):
    """FULL recipe + train_gate through from_training_config: the gate's parameters are in the flat buffer and the optimiser; after
    three steps every gate tensor moved and num_batches_tracked is 3 + the fixture's 7; the overlapped and the in-line optimiser
    agree bit for bit; a second identical run reproduces them."""
    on, flat_on, start = _train(tmp_path, 3, overlap=True)
    for k, v in on.items():
        assert not torch.equal(v, start[k]), f"{k} did not change in three steps"
        if k.endswith("num_batches_tracked"):
            assert int(v) == 10
        else:
            assert bool(torch.isfinite(v.float()).all()), k
    off, flat_off, _ = _train(tmp_path, 3, overlap=False)
    _same(on, off, "overlap on vs off")
    assert torch.equal(flat_on, flat_off)
    again, flat_again, _ = _train(tmp_path, 3, overlap=True)
    _same(on, again, "second identical run")
    assert torch.equal(flat_on, flat_again)


def test_trainer_resume_is_bit_exact(tmp_path):
    """save at step 2, reload, step once: the uninterrupted run's bits, BatchNorm buffers included"""
    ck = str(tmp_path / "checkpoint-2")
    whole, flat_whole, _ = _train(tmp_path, 3, save_at=(2, ck))
    resumed, flat_resumed, at2 = _train(tmp_path, 1, resume=ck, first_step=2)
    assert int(at2["resnet.bn1.num_batches_tracked"]) == 9
    _same(whole, resumed, "resumed vs uninterrupted")
    assert torch.equal(flat_whole, flat_resumed)
