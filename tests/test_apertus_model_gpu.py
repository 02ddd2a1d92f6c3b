"""Apertus decoders on the GPU against the fixtures the REAL reference wrote (tests/golden/tiny_clip_apertus*, HF 5.15
ApertusForCausalLM behind the reference's MultiModalModelForCausalLM), with tests/test_qwen3_model_gpu.py's bounds:
  fp32: stage activations, logits rel-L2 <= 1e-4, loss |d| <= 1e-4, grads (alpha_p / alpha_n / q_norm / k_norm of layer 0 included)
        rel-L2 <= 1e-3, greedy ids bit-exact at T = 0.1 / 0.7;
  bf16: logits rel-L2 <= 3e-2, loss |d| <= 3e-2, grads rel-L2 <= 6e-2.
Plus the bf16 KV-cache decode step against the last row of a full-sequence forward, trainer steps (the xIELU scalars move, the
optimizer overlap changes no bit, reruns reproduce), gradient accumulation, a save -> from_pretrained round trip, and one forward +
backward at Apertus-8B layer shapes (2 layers, B = 1, S = 2048, random init: properties only)."""
import pytest
import torch

from oracle import ref_cpu as R
from tests.apertus_fixture import FIXTURES, load_apertus_golden
from tests.model_utils import build_from_golden, to_device

pytestmark = pytest.mark.gpu
CASES = ["right", "left", "textonly", "interleaved4"]
SCALARS = ("act_fn.alpha_p", "act_fn.alpha_n", "q_norm.weight", "k_norm.weight")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module", params=FIXTURES)
def gold(request, golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return load_apertus_golden(request.param, golden_dir)


@pytest.fixture(scope="module")
def model_f32(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("a32"), "float32")


@pytest.fixture(scope="module")
def model_bf16(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("a16"), "bfloat16")


def _fwd(m, gb, labels=True):
    return m(input_ids=gb["input_ids"], attention_mask=gb["attention_mask"], position_ids=gb["position_ids"],
             labels=gb["labels"] if labels else None, processed_multimodal_inputs=gb["processed_multimodal_inputs"])


@pytest.mark.parametrize("case", CASES)
def test_f32_forward_matches_reference(gold, model_f32, case):
    meta, w, v = gold
    if case not in meta["cases"]:
        pytest.skip(f"{meta['name']} holds no '{case}' case")
    batch = R.golden_batch(v, case)
    gb = to_device(batch)
    stages = {}
    with torch.no_grad():
        e = model_f32.embed_modalities_with_text(gb["input_ids"], gb["processed_multimodal_inputs"], stages=stages)
        out = _fwd(model_f32, gb)
    torch.cuda.synchronize()
    stages["spliced_embeds"] = e
    for name, t in stages.items():
        assert rel(t, v[f"{case}.act.{name}"]) < 1e-4, name
    valid = batch["attention_mask"].bool()
    ref = v[f"{case}.logits"]
    assert out.logits.shape == ref.shape
    assert rel(out.logits.cpu()[valid], ref[valid]) < 1e-4
    assert abs(float(out.loss) - float(v[f"{case}.loss"])) < 1e-4
    assert torch.equal(out.logits.cpu()[valid].argmax(-1), ref[valid].argmax(-1))


def _grads(m, v):
    gb = to_device(R.golden_batch(v, "right"))
    m.unfreeze()
    for p in m.parameters():
        p.grad = None
    _fwd(m, gb).loss.backward()
    torch.cuda.synchronize()
    return dict(m.named_parameters())


def test_f32_grads_match_reference(gold, model_f32):
    meta, w, v = gold
    params = _grads(model_f32, v)
    n, scalars = 0, set()
    for key, ref in v.items():
        if not key.startswith("right.grad."):
            continue
        name = key[len("right.grad."):]
        g = params[name].grad
        assert g is not None, name
        assert g.shape == ref.shape, name
        err = float((g.double().cpu() - ref.double()).norm())
        assert err <= 1e-3 * float(ref.double().norm()) + 1e-6, (name, err)
        n += 1
        for s in SCALARS:
            if name == f"model.model.layers.0.{'mlp' if 'act_fn' in s else 'self_attn'}.{s}":
                scalars.add(s)
    assert n > 20 and scalars == set(SCALARS), (n, scalars)


@pytest.mark.parametrize("case", ["left", "textonly"])
@pytest.mark.parametrize("T", [0.1, 0.7])
def test_f32_greedy_ids_bit_exact(gold, model_f32, case, T):
    meta, w, v = gold
    if f"{case}.greedy_T{T}" not in v:
        pytest.skip(f"{meta['name']} holds no greedy ids for '{case}'")
    ids = model_f32.generate(R.golden_batch(v, case), max_new_tokens=8, temperature=T, do_sample=False)
    assert torch.equal(ids, v[f"{case}.greedy_T{T}"])


@pytest.mark.parametrize("case", CASES)
def test_bf16_forward_within_bf16_noise(gold, model_bf16, case):
    meta, w, v = gold
    if case not in meta["cases"]:
        pytest.skip(f"{meta['name']} holds no '{case}' case")
    batch = R.golden_batch(v, case)
    with torch.no_grad():
        out = _fwd(model_bf16, to_device(batch))
    valid = batch["attention_mask"].bool()
    assert rel(out.logits.float().cpu()[valid], v[f"{case}.logits"][valid]) < 3e-2
    assert abs(float(out.loss) - float(v[f"{case}.loss"])) < 3e-2


def test_bf16_grads(gold, model_bf16):
    meta, w, v = gold
    params = _grads(model_bf16, v)
    seen = 0
    for key, ref in v.items():
        if not key.startswith("right.grad."):
            continue
        name = key[len("right.grad."):]
        if ref.dim() < 2 and not name.endswith(SCALARS):
            continue
        e = rel(params[name].grad.float(), ref)
        assert e < 6e-2, (name, e)
        seen += 1
    assert seen > 12


def test_bf16_kv_cache_decode_step_matches_full_forward(gold, model_bf16, monkeypatch):
    """Prefill S-1 tokens into the KV cache, then one decode step (the unfused DecoderLayer.infer: q/k-norm layers never take the fused
    decode kernels): its MLP is up_proj, mm_xielu_fwd, down_proj, and its logits equal the last row of a full-sequence forward within
    bf16 noise."""
    from multimeditron_amd import kernels as K
    meta, w, v = gold
    lm = model_bf16.model
    ids = v["textonly.in.input_ids" if "textonly" in meta["cases"] else "right.in.input_ids"].cuda()
    calls = []
    orig = K.xielu_fwd
    monkeypatch.setattr(K, "xielu_fwd", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    L = meta["llm"]["num_hidden_layers"]
    with torch.no_grad():
        full = lm(input_ids=ids).logits[:, -1].float()
        pre = lm(input_ids=ids[:, :-1], use_cache=True, max_new_tokens=4)
        before = len(calls)
        step = lm(input_ids=ids[:, -1:], past_key_values=pre.past_key_values, use_cache=True).logits[:, -1].float()
    torch.cuda.synchronize()
    assert before == 2 * L and len(calls) == 3 * L
    assert not any(layer.can_decode_step_fused(torch.empty(ids.shape[0], 128, dtype=torch.bfloat16, device="cuda"), ids.shape[0], 1,
                                               pre.past_key_values[i]) for i, layer in enumerate(lm.model.layers))
    assert rel(step, full) < 2e-2, rel(step, full)
    assert torch.equal(step.argmax(-1), full.argmax(-1))


def _two_steps(golden_dir, tmp, overlap):
    from multimeditron_amd.train.trainer import MultimodalTrainer, TrainingMode
    meta, w, v = load_apertus_golden("tiny_clip_apertus", golden_dir)
    m = build_from_golden(meta, w, tmp, "bfloat16")      # the throughput path: every kernel deterministic (fp32 attention backward uses atomics)
    tr = MultimodalTrainer(m, training_mode=TrainingMode.FULL, learning_rate=1e-2, weight_decay=0.01, max_grad_norm=1.0,
                           overlap_optimizer=overlap)
    losses = [float(tr.training_step(to_device(R.golden_batch(v, c)))) for c in ("right", "interleaved4")]
    tr.synchronize()
    torch.cuda.synchronize()
    flat = m.flat_params().data.clone()
    f = m.model.model.layers[0].mlp.act_fn
    out = (losses, flat, float(f.alpha_p.detach()), float(f.alpha_n.detach()), float(v["right.loss"]), w)
    tr.close()
    return out


def test_trainer_steps_move_the_scalars_and_reproduce(golden_dir, tmp_path):
    """Two FULL-mode bf16 steps (lr 1e-2, so that a step is visible in a bf16 scalar): finite, the loss of the first is the
    reference's within the bf16 bound, both xIELU scalars of layer 0 move; the optimizer on its side stream (overlap) changes no
    bit; a rerun reproduces every bit."""
    losses, flat, ap, an, ref_loss, w = _two_steps(golden_dir, tmp_path / "a", True)
    assert all(torch.isfinite(torch.tensor(losses))) and bool(torch.isfinite(flat).all())
    assert abs(losses[0] - ref_loss) < 3e-2
    assert ap != float(w["model.model.layers.0.mlp.act_fn.alpha_p"]) and an != float(w["model.model.layers.0.mlp.act_fn.alpha_n"])
    losses2, flat2, *_ = _two_steps(golden_dir, tmp_path / "b", False)
    assert losses2 == losses and torch.equal(flat2, flat), "overlap on / off"
    losses3, flat3, *_ = _two_steps(golden_dir, tmp_path / "c", True)
    assert losses3 == losses and torch.equal(flat3, flat), "rerun"


def _double(b):
    """the batch twice over: the same mean loss, the same gradients"""
    B = b["input_ids"].shape[0]
    out = {k: torch.cat([b[k], b[k]], 0) for k in ("input_ids", "attention_mask", "position_ids", "labels")}
    pm = b["processed_multimodal_inputs"]
    out["processed_multimodal_inputs"] = {
        "batch_idx": {t: torch.cat([x, x + B]) for t, x in pm["batch_idx"].items()},
        "token_range": {t: torch.cat([x, x]) for t, x in pm["token_range"].items()},
        "stacked": {t: list(x) + list(x) for t, x in pm["stacked"].items()}}
    return out


def test_bf16_gradient_accumulation_equals_doubled_batch(golden_dir, tmp_path):
    """Two half-weighted backward passes (overwrite, then accumulate: grad_target) against one pass over the doubled batch, within the
    bf16 bound on the gradients; the xIELU scalars and the q/k norms among them."""
    meta, w, v = load_apertus_golden("tiny_clip_apertus", golden_dir)
    m = build_from_golden(meta, w, tmp_path, "bfloat16")
    m.unfreeze()
    batch = R.golden_batch(v, "right")
    for p in m.parameters():
        p.grad = None
    for _ in range(2):
        loss = _fwd(m, to_device(batch)).loss
        loss.backward(gradient=torch.full_like(loss, 0.5))
    torch.cuda.synchronize()
    acc = {n: p.grad.float().clone() for n, p in m.named_parameters() if p.grad is not None}
    for p in m.parameters():
        p.grad = None
    _fwd(m, to_device(_double(batch))).loss.backward()
    torch.cuda.synchronize()
    seen = set()
    for n, p in m.named_parameters():
        if n.startswith("model.model.layers.0.") and (p.dim() >= 2 or n.endswith(SCALARS)):
            e = rel(acc[n], p.grad.float())
            assert e < 6e-2, (n, e)
            seen.add(n.rsplit(".", 2)[-2] + "." + n.rsplit(".", 1)[-1])
    assert {"act_fn.alpha_p", "act_fn.alpha_n", "q_norm.weight", "k_norm.weight", "up_proj.weight"} <= seen, seen


def test_save_from_pretrained_roundtrip_reproduces_logits(golden_dir, tmp_path):
    from multimeditron_amd.model.model import MultiModalModelForCausalLM
    meta, w, v = load_apertus_golden("tiny_clip_apertus", golden_dir)
    m = build_from_golden(meta, w, tmp_path / "a", "float32")
    gb = to_device(R.golden_batch(v, "right"))
    with torch.no_grad():
        l1 = _fwd(m, gb).logits.clone()
    m.save_pretrained(str(tmp_path / "ckpt"))
    m2 = MultiModalModelForCausalLM.from_pretrained(str(tmp_path / "ckpt"), device="cuda")
    cfg = m2.model.config
    assert cfg.model_type == "apertus" and cfg.qk_norm and cfg.hidden_act == "xielu"
    with torch.no_grad():
        l2 = _fwd(m2, gb).logits
    assert torch.equal(l1, l2)


def test_apertus_8b_layer_shapes_forward_backward_properties():
    """Apertus-8B's layer shapes (hidden 4096, I 21504, 32 / 8 heads of 128, vocab 131072) with 2 layers and random init, B = 1,
    S = 2048: finite loss and gradients, and a second forward + backward gives the same bits (the scalar gradients included: their
    sums run over 2048 x 21504 elements in 4096 workgroups of 6 passes each)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from multimeditron_amd.model.model import MultimodalConfig, MultiModalModelForCausalLM
    from multimeditron_amd.model.modalities import ImageConfig
    from multimeditron_amd.model.presets import resolve_llm_config
    from tests.test_fullsize_gpu import _batch
    llm = dict(resolve_llm_config("swiss-ai/Apertus-8B-Instruct-2509"), num_hidden_layers=2)
    torch.manual_seed(5)
    cfg = MultimodalConfig(vocab_size=llm["vocab_size"] + 2, modalities=[ImageConfig(hidden_size=4096, clip_name="openai/clip-vit-base-patch32")],
                           llm_path="swiss-ai/Apertus-8B-Instruct-2509", dtype="bfloat16", eos_token_idx=2, hidden_size=4096)
    m = MultiModalModelForCausalLM(cfg, device="cuda", llm_config=llm)
    m.pack_parameters()
    m.unfreeze()
    V = llm["vocab_size"] + 2
    b = _batch(1, 2048, 1, 49, V, 9)
    runs = []
    for _ in range(2):
        for p in m.parameters():
            p.grad = None
        loss = _fwd(m, b).loss
        loss.backward()
        torch.cuda.synchronize()
        f = m.model.model.layers[0].mlp.act_fn
        runs.append((loss.detach().clone(), f.alpha_p.grad.clone(), f.alpha_n.grad.clone(),
                     m.model.model.layers[0].mlp.up_proj.weight.grad.clone()))
    for t in runs[0]:
        assert bool(torch.isfinite(t.float()).all())
    assert float(runs[0][1].abs()) > 0 and float(runs[0][2].abs()) > 0
    for a, c in zip(*runs):
        assert torch.equal(a, c), "forward + backward must be bit-reproducible"
