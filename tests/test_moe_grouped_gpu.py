"""The MoE image modalities with `grouped_towers` (model/vision_grouped.py: the E expert towers as ONE chain of grouped launches)
on the GPU: against the reference's vectors, against the sequential eager towers bit for bit, under the Trainer, and a count of
library calls that shows the expert really is a batch dimension."""
import json
import os
import warnings
from contextlib import contextmanager

import pytest
import torch

from tests.test_moe_modality_gpu import _build, moe, moe_pep, rel  # noqa: F401  (moe / moe_pep are fixtures)

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


EAGER = {"MM_MOE_GRAPH": "0", "MM_MOE_TRAIN_GRAPH": "0", "MM_MOE_STREAMS": "0"}      # sequential eager: one tower after the other


@contextmanager
def _recorded():
    """names of the library calls made through multimeditron_amd.kernels inside the block"""
    from multimeditron_amd import kernels
    names, real = [], kernels.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    kernels.call = spy
    try:
        yield names
    finally:
        kernels.call = real


def _mode(monkeypatch, m, grouped):
    """grouped: the switch on, the graph / stream switches left at their defaults (the grouped path must win over them);
    otherwise sequential eager towers"""
    monkeypatch.delenv("MM_MOE_GROUPED", raising=False)
    for k, v in EAGER.items():
        if grouped:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    m.config.grouped_towers = bool(grouped)


def _no_graphs(m):
    return not getattr(m.experts, "_mm_graphs", None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fusion", ["weighted_average", "sequence_append", "cross_attn"])
@pytest.mark.parametrize("pep", [False, True], ids=["shared", "pep"])
def test_grouped_fusions_match_reference(moe, moe_pep, tmp_path, monkeypatch, pep, fusion, dtype):
    """test_moe_fusions_match_reference / test_moe_pep_fusions_match_reference with the grouped towers, at their tolerances"""
    meta, w, v = moe_pep if pep else moe
    m = _build(meta, w, v, fusion, dtype, tmp_path)
    _mode(monkeypatch, m, True)
    px = v["pixels"]
    with _recorded() as names:
        y = m([px[i] for i in range(px.shape[0])])
    assert "mm_layernorm_fwd_batched" in names and "mm_layernorm_fwd" not in names and _no_graphs(m)
    tol_o, tol_g = (1e-4, 1e-3) if dtype == torch.float32 else (3e-2, 6e-2)
    assert y.shape == v[f"{fusion}.out"].shape
    assert rel(y.float(), v[f"{fusion}.out"]) < tol_o
    y.backward(v[f"{fusion}.dout"].to(dtype).cuda())
    torch.cuda.synchronize()
    own = dict(m.named_parameters())
    n = 0
    for key, ref in v.items():
        if not key.startswith(f"{fusion}.grad.") or ref.dim() < 2:
            continue
        g = own[key[len(fusion) + 6:]].grad
        assert g is not None, key
        assert rel(g.float().reshape(ref.shape), ref) < tol_g, key
        n += 1
    assert n >= 10


def _same_grads(g0, g1, dtype, what):
    if dtype == torch.bfloat16:
        assert torch.equal(g0, g1), (what, float((g0.float() - g1.float()).abs().max()))
    else:       # the fp32 attention backward sums with atomics: equal to rounding (test_trainable_towers_graph_replay_equals_eager's rule)
        assert float((g0 - g1).norm()) <= 1e-6 * float(g0.norm()), (what, float((g0 - g1).abs().max()))


@pytest.mark.parametrize("pep", [False, True], ids=["shared", "pep"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_grouped_towers_equal_sequential_eager(moe, moe_pep, tmp_path, pep, dtype, monkeypatch):
    """The five-call protocol of test_trainable_towers_graph_replay_equals_eager (new pixels every call, call 3 accumulates onto
    call 2's gradients): outputs bit for bit, the flat gradient bit for bit in bf16, the gradient-ready hook once per tower parameter
    per backward."""
    from multimeditron_amd import functional as Fm
    meta, w, v = moe_pep if pep else moe
    px = v["pixels"]
    g = torch.Generator().manual_seed(5)
    batches = [[px[i] for i in range(px.shape[0])]] + [[torch.randn_like(px[0], generator=g) for _ in range(px.shape[0])] for _ in range(4)]
    reset = [True, True, True, False, True]
    got = {}
    for grouped in (False, True):
        m = _build(meta, w, v, "cross_attn", dtype, tmp_path / f"g{int(grouped)}")
        _mode(monkeypatch, m, grouped)
        flat = next(iter(m.parameters()))._mm_flat
        tower = [p for k, p in m.named_parameters() if k.startswith("experts.")]
        fired = []
        Fm.set_grad_ready_hook(lambda p: fired.append(id(p)))
        try:
            rec = []
            for b, fresh in zip(batches, reset):
                if fresh:
                    flat.attach_grads(fresh=True)
                fired.clear()
                y = m(b)
                (y.float() * torch.linspace(-1, 1, y.numel(), device=y.device).view_as(y)).sum().backward()
                torch.cuda.synchronize()
                assert sorted(i for i in fired if i in {id(p) for p in tower}) == sorted(id(p) for p in tower)
                rec.append((y.detach().clone(), flat.grad.detach().clone()))
        finally:
            Fm.set_grad_ready_hook(None)
        got[grouped] = rec
        assert _no_graphs(m)
    for i, ((y0, g0), (y1, g1)) in enumerate(zip(got[False], got[True])):
        assert torch.equal(y0, y1), i
        _same_grads(g0, g1, dtype, i)
    assert not torch.equal(got[True][1][1], got[True][2][1])


@pytest.mark.parametrize("pep", [False, True], ids=["shared", "pep"])
def test_grouped_frozen_towers_and_no_grad_equal_sequential_eager(moe, moe_pep, tmp_path, pep, monkeypatch):
    """frozen towers (alignment / end2end recipes) and no-grad calls take the grouped chain too: same outputs, same gradients of what
    still trains, no tower gradient, no graph"""
    meta, w, v = moe_pep if pep else moe
    px = v["pixels"]
    g = torch.Generator().manual_seed(3)
    batches = [[px[i] for i in range(px.shape[0])], [torch.randn_like(px[0], generator=g) for _ in range(px.shape[0])],
               [torch.randn_like(px[0], generator=g) for _ in range(2)]]
    got = {}
    for grouped in (False, True):
        m = _build(meta, w, v, "cross_attn", torch.bfloat16, tmp_path / f"f{int(grouped)}")
        _mode(monkeypatch, m, grouped)
        with torch.no_grad(), _recorded() as names:
            quiet = [m(b).clone() for b in batches]                      # trainable towers, no-grad calls
        assert ("mm_layernorm_fwd_batched" in names) == grouped
        m.freeze_modality_embedder()
        flat = next(iter(m.parameters()))._mm_flat
        rec = []
        for b in batches:
            flat.attach_grads(fresh=True)
            with _recorded() as names:
                y = m(b)
            assert ("mm_layernorm_fwd_batched" in names) == grouped
            y.float().square().mean().backward()
            torch.cuda.synchronize()
            rec.append((y.detach().clone(), flat.grad.detach().clone()))
        assert all(p.grad is None for k, p in m.named_parameters() if k.startswith("experts."))
        assert _no_graphs(m)
        got[grouped] = (quiet, rec)
    for a, b in zip(got[False][0], got[True][0]):
        assert torch.equal(a, b)
    for i, ((y0, g0), (y1, g1)) in enumerate(zip(got[False][1], got[True][1])):
        assert torch.equal(y0, y1) and torch.equal(g0, g1), i


@pytest.mark.parametrize("pep", [False, True], ids=["shared", "pep"])
def test_grouped_two_forwards_before_one_backward(moe, moe_pep, tmp_path, pep, monkeypatch):
    """No shared buffers, no `pending` state: two forwards whose losses are summed before ONE backward, and a forward whose backward
    never runs followed by a normal step, are both grouped and equal sequential eager bit for bit (bf16)."""
    meta, w, v = moe_pep if pep else moe
    px = v["pixels"]
    g = torch.Generator().manual_seed(9)
    b0 = [px[i] for i in range(px.shape[0])]
    b1 = [torch.randn_like(px[0], generator=g) for _ in range(px.shape[0])]
    got = {}
    for grouped in (False, True):
        m = _build(meta, w, v, "weighted_average", torch.bfloat16, tmp_path / f"two{int(grouped)}")
        _mode(monkeypatch, m, grouped)
        flat = next(iter(m.parameters()))._mm_flat
        for rep in range(2):
            flat.attach_grads(fresh=True)
            with _recorded() as names:
                y0, y1 = m(b0), m(b1)
            assert names.count("mm_drop_cls_fwd") == (2 if grouped else 2 * meta["num_experts"])      # both forwards took the same path
            wgt = torch.linspace(-1, 1, y0.numel(), device=y0.device).view_as(y0)
            ((y0.float() * wgt).sum() + (y1.float() * wgt.flip(0)).sum()).backward()
            torch.cuda.synchronize()
        two = (y0.detach().clone(), y1.detach().clone(), flat.grad.detach().clone())
        lost = m(b1)                                                     # a forward whose backward never runs ...
        del lost
        flat.attach_grads(fresh=True)
        with _recorded() as names:
            y = m(b0)                                                    # ... then a normal step
        assert names.count("mm_drop_cls_fwd") == (1 if grouped else meta["num_experts"])
        (y.float() * wgt).sum().backward()
        torch.cuda.synchronize()
        got[grouped] = two + (y.detach().clone(), flat.grad.detach().clone())
        assert _no_graphs(m)
    for a, b in zip(got[False], got[True]):
        assert torch.equal(a, b), float((a.float() - b.float()).abs().max())


def test_grouped_full_recipe_trainer_steps_equal_eager(tmp_path, monkeypatch):
    """The `full` recipe of test_moe_full_recipe_trainer_steps_graph_equals_eager with `grouped_towers: true` against sequential
    eager towers: three optimiser steps (the overlapped optimiser on: the grouped chain fires the per-block parameter-read hooks by
    hand), same losses, same flat parameters bit for bit."""
    import bench
    from tests.test_training_config_cpu import ATTACH, make_tokenizer
    from multimeditron_amd.train import from_training_config
    llm = os.path.join(str(tmp_path), "llm")
    os.makedirs(llm, exist_ok=True)
    json.dump(dict(model_type="llama", hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                   num_key_value_heads=1, head_dim=64, vocab_size=32, rms_norm_eps=1e-5, tie_word_embeddings=False,
                   rope_parameters={"rope_type": "default", "rope_theta": 10000.0}), open(os.path.join(llm, "config.json"), "w"))
    clips = []
    for i in range(3):
        d = os.path.join(str(tmp_path), f"clip{i}")
        os.makedirs(d, exist_ok=True)
        json.dump({"vision_config": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=32,
                                         patch_size=16)}, open(os.path.join(d, "config.json"), "w"))
        json.dump({"size": {"shortest_edge": 32}, "crop_size": {"height": 32, "width": 32}}, open(os.path.join(d, "preprocessor_config.json"), "w"))
        clips.append(d)
    res = {}
    for grouped in (False, True):
        monkeypatch.delenv("MM_MOE_GROUPED", raising=False)
        for k, val in EAGER.items():
            monkeypatch.setenv(k, val) if not grouped else monkeypatch.delenv(k, raising=False)
        modality = {"model_type": "moe_meditron_clip_shared", "image_processor": clips[0], "hidden_size": 128, "expert_clip_names": clips,
                    "generalist_idx": -1, "gating_path": "stub", "fusion_method": "cross_attn", "top_k_experts": 3, "cross_attn_heads": 2}
        if grouped:
            modality["grouped_towers"] = True
        recipe = {
            "base_llm": llm, "base_model": None, "attachment_token": ATTACH, "tokenizer_type": "llama", "token_size": 128,
            "loaders": [{"loader_type": "raw-image", "modality_type": "image"}], "modalities": [modality], "training_mode": "FULL",
            "training_args": {"learning_rate": 1.0e-3, "bf16": True, "per_device_train_batch_size": 2, "gradient_accumulation_steps": 2,
                              "max_steps": 50, "max_grad_norm": 1.0, "lr_scheduler_type": "constant", "weight_decay": 0.01},
        }
        torch.manual_seed(0)
        setup = from_training_config(recipe, make_tokenizer(), device="cuda", dtype="bfloat16")
        model, tr = setup.model, setup.trainer
        mod = model.modalities_by_type["image"]
        assert mod.config.grouped_towers is grouped

        def gate(px):                    # test-side stand-in for the reference's ResNet gate (a plug: DESIGN.md section 7)
            logits = px.float().mean(dim=(2, 3)) @ torch.tensor([[1.0, 0.5, -0.5], [0.2, -0.3, 0.7], [-0.4, 0.9, 0.1]], device=px.device)
            return logits, logits.topk(1, dim=-1).indices, torch.softmax(logits, dim=-1)

        mod.gating_network = gate
        model.eval()                     # no dropout: the two runs must agree bit for bit
        model.train = lambda *_a, **_k: model
        vocab = model.config.vocab_size
        losses = []
        with _recorded() as names:
            for step in range(6):        # 6 micro-batches = 3 optimiser steps (the second micro-batch of a step accumulates)
                batch, _ = bench.synthetic_batch(2, 24, 1, 4, vocab, (vocab - 3, vocab - 2, vocab - 1), 100 + step, "cpu", 32, collator_form=True)
                batch["input_ids"].clamp_(max=vocab - 1)
                batch["labels"] = torch.where(batch["labels"] >= 0, batch["labels"].clamp(max=vocab - 1), batch["labels"])
                losses.append(float(tr.training_step(batch)))
        tr.synchronize()
        torch.cuda.synchronize()
        assert ("mm_layernorm_bwd_batched" in names) == grouped and _no_graphs(mod)
        res[grouped] = (losses, tr.flat.data.detach().clone())
        tr.close()
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    assert torch.equal(res[False][1], res[True][1])
    assert all(l == l for l in res[False][0])


def test_the_expert_is_a_batch_dimension(moe, tmp_path, monkeypatch):
    """Library calls of forward + backward: the grouped E = 3 towers make no more calls than ONE tower, but for the embedding stage,
    which runs once per tower (not once per layer) and stays E calls."""
    from multimeditron_amd import functional as Fm
    from multimeditron_amd.model.expert_towers import run_experts as _run_experts
    meta, w, v = moe
    m = _build(meta, w, v, "weighted_average", torch.bfloat16, tmp_path)
    _mode(monkeypatch, m, True)
    E = len(m.experts)
    flat = next(iter(m.parameters()))._mm_flat
    px = v["pixels"].cuda()
    n = px.shape[0]

    def count(fn):
        flat.attach_grads(fresh=True)
        with _recorded() as names:
            out = fn()
            sum(o.float().sum() for o in out).backward()
        torch.cuda.synchronize()
        return len(names)

    def one_tower():
        hs = m.experts[0](px).last_hidden_state
        return [Fm.drop_cls(hs.reshape(n * hs.shape[1], -1), n, hs.shape[1])]

    grouped = count(lambda: _run_experts(m.experts, px, grouped=True))
    single = count(one_tower)
    embed = count(lambda: [m.experts[0].embeddings(px)])
    assert embed > 0 and single > embed
    assert grouped - single <= (E - 1) * embed, (grouped, single, embed)
    for k, val in EAGER.items():
        monkeypatch.setenv(k, val)
    eager = count(lambda: _run_experts(m.experts, px, grouped=False))
    assert eager == E * single                                            # what the switch saves


def test_ineligible_experts_take_the_old_paths_with_one_warning(moe, tmp_path, monkeypatch):
    """one expert with a different layer count: the switch changes nothing but for ONE warning"""
    import dataclasses
    from multimeditron_amd.model import expert_towers as mod
    from multimeditron_amd.model.vision import VisionTransformer
    from multimeditron_amd.nn import FlatParams
    meta, w, v = moe
    m = _build(meta, w, v, "weighted_average", torch.bfloat16, tmp_path)
    odd = VisionTransformer(dataclasses.replace(m.experts[1].config, num_hidden_layers=1), torch.bfloat16, "cuda")
    src = dict(m.experts[1].named_parameters())
    with torch.no_grad():
        for k, p in odd.named_parameters():
            p.copy_(src[k])
    FlatParams([(k, p, "encoder") for k, p in odd.named_parameters()], "cuda", torch.bfloat16)      # q|k|v adjacent: one GEMM operand
    m.experts[1] = odd
    px = [v["pixels"][i] for i in range(v["pixels"].shape[0])]
    monkeypatch.setattr(mod, "_warned_ineligible", False)
    _mode(monkeypatch, m, False)
    for k in EAGER:
        monkeypatch.delenv(k, raising=False)
    with torch.no_grad(), warnings.catch_warnings(record=True) as off:
        warnings.simplefilter("always")
        y_off = m(px).clone()
    m.config.grouped_towers = True
    with torch.no_grad(), warnings.catch_warnings(record=True) as on, _recorded() as names:
        warnings.simplefilter("always")
        y_on = [m(px).clone() for _ in range(2)]
    assert not [x for x in off if "grouped_towers" in str(x.message)]
    assert len([x for x in on if "grouped_towers" in str(x.message)]) == 1
    assert "mm_layernorm_fwd_batched" not in names
    assert torch.equal(y_off, y_on[0]) and torch.equal(y_off, y_on[1])
