"""The launches and gradient-ready calls of a training pass, by name and in order: the recorder behind
tests/golden/train_launches.jsonl.

`python tools/make_golden.py train_launches` writes the file with record() below, tests/test_train_launch_trace_gpu.py runs the same
record() and compares.  Only the public model call, multimeditron_amd.kernels.call and functional.set_grad_ready_hook are used
(names only, as in generate_trace.py), so one recorder serves every revision of the autograd layer (functional.py) and of the
wrappers (kernels.py).  An entry is a C symbol or `ready:<parameter name>`.

Every case runs TWO consecutive forward + backward passes without clearing gradients: the first writes every gradient (overwrite),
the second accumulates.  Models: the tiny golden models with pack_parameters(), bf16 unless the case says fp32, on their "right"
batch.  The MoE modality (no decoder: the modality alone, as tests/test_moe_modality_gpu.py builds it) runs with MM_MOE_GRAPH,
MM_MOE_TRAIN_GRAPH and MM_MOE_STREAMS at "0" for the call, so that no captured graph replays in place of the Python under test;
`moe_grouped` adds MM_MOE_GROUPED=1 (the expert towers as one chain of grouped launches)."""
import json
import os

import torch

from multimeditron_amd import functional as Fm
from multimeditron_amd import kernels as K
from oracle import ref_cpu as R
from tests.model_utils import build_from_golden, to_device

FIXTURE = "train_launches.jsonl"
MOE_EAGER = {"MM_MOE_GRAPH": "0", "MM_MOE_TRAIN_GRAPH": "0", "MM_MOE_STREAMS": "0"}


def _all(model):
    model.unfreeze()


def _vision_frozen(model):
    model.unfreeze()
    for m in model.modalities_with_projection:
        m.freeze_modality_embedder()


def _head_and_norms(model):
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("model.") and "norm" in n
    model.model.lm_head.weight.requires_grad = True


def _load(fixture, golden_dir):
    """-> (meta, weights, vectors); the Qwen3 and Apertus fixtures are sharded (tests/qwen3_fixture.py, tests/apertus_fixture.py)"""
    if "qwen3" in fixture:
        from tests.qwen3_fixture import load_qwen3_golden
        return load_qwen3_golden(fixture, golden_dir)
    if "apertus" in fixture:
        from tests.apertus_fixture import load_apertus_golden
        return load_apertus_golden(fixture, golden_dir)
    return R.load_golden(fixture, golden_dir)


CASES = [  # name, golden model, dtype, which parameters train
    ("llama_d128", "tiny_clip_llama_d128", "bfloat16", _all),            # RoPE epilogue, fused SwiGLU where the shapes qualify
    ("qwen2", "tiny_clip_qwen2", "bfloat16", _all),                      # q/k/v bias
    ("qwen3", "tiny_clip_qwen3", "bfloat16", _all),                      # q/k norm
    ("apertus", "tiny_clip_apertus", "bfloat16", _all),                  # xIELU
    ("siglip_qwen2", "tiny_siglip_qwen2", "bfloat16", _all),             # conv bias, no CLS row, head padding
    ("llama_vision_frozen", "tiny_clip_llama_d128", "bfloat16", _vision_frozen),
    ("llama_head_and_norms", "tiny_clip_llama_d128", "bfloat16", _head_and_norms),
    ("llama_f32", "tiny_clip_llama_d128", "float32", _all),
]
MOE_CASES = [("moe", {}), ("moe_grouped", {"MM_MOE_GROUPED": "1"})]      # name, switches on top of MOE_EAGER
NAMES = [c[0] for c in CASES] + [c[0] for c in MOE_CASES]


def recorded(params, step, passes=2):
    """run step() `passes` times under the two spies -> the entries, in order"""
    who = {id(p): n for n, p in params}
    seen, call, hook = [], K.call, Fm._grad_ready_hook

    def recording(name, *args):
        seen.append(name)
        return call(name, *args)

    K.call = recording
    Fm.set_grad_ready_hook(lambda p: seen.append("ready:" + who[id(p)]))
    try:
        for _ in range(passes):
            step()
        torch.cuda.synchronize()
    finally:
        K.call = call
        Fm.set_grad_ready_hook(hook)
    return seen


def build_case(name, golden_dir, tmpdir):
    """-> (named parameters, step): step() is one forward + backward and returns the loss (a 0-d tensor)."""
    for case, fixture, dtype, policy in CASES:
        if case == name:
            meta, w, v = _load(fixture, golden_dir)
            model = build_from_golden(meta, w, os.path.join(str(tmpdir), name), dtype)
            policy(model)
            gb = to_device(R.golden_batch(v, "right"))

            def step():
                out = model(input_ids=gb["input_ids"], attention_mask=gb["attention_mask"], position_ids=gb["position_ids"],
                            labels=gb["labels"], processed_multimodal_inputs=gb["processed_multimodal_inputs"])
                out.loss.backward()
                return out.loss.detach()

            return list(model.named_parameters()), step
    from safetensors.torch import load_file
    from tests.test_moe_modality_gpu import _build
    meta = json.load(open(os.path.join(golden_dir, "tiny_moe_clip.meta.json")))
    w = load_file(os.path.join(golden_dir, "tiny_moe_clip.weights.safetensors"))
    v = load_file(os.path.join(golden_dir, "tiny_moe_clip.vectors.safetensors"))
    m = _build(meta, w, v, "weighted_average", torch.bfloat16, os.path.join(str(tmpdir), name))
    px = [v["pixels"][i] for i in range(v["pixels"].shape[0])]
    dout = v["weighted_average.dout"].to(torch.bfloat16).cuda()

    def step():
        y = m(px)
        y.backward(dout)
        return (y.detach().float() * dout.float()).sum()      # the scalar this backward differentiates

    return list(m.named_parameters()), step


class switches:
    """the environment switches of a case, for the call; what stood there before comes back"""

    def __init__(self, name):
        self.env = dict(MOE_EAGER, **dict(MOE_CASES)[name]) if name in dict(MOE_CASES) else {}

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, old in self.before.items():
            if old is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = old


def record(golden_dir, tmpdir):
    """-> [(case name, [entry, ...]), ...] in the order of NAMES"""
    rows = []
    for name in NAMES:
        with switches(name):
            params, step = build_case(name, golden_dir, tmpdir)
            rows.append((name, recorded(params, step)))
    return rows


def write(rows, golden_dir):
    """One header line with the table of entries, then one line per case: its entries as indices into the table."""
    table = sorted({n for _, names in rows for n in names})
    index = {n: i for i, n in enumerate(table)}
    with open(os.path.join(golden_dir, FIXTURE), "w") as f:
        f.write(json.dumps({"symbols": table}, separators=(",", ":")) + "\n")
        for name, names in rows:
            f.write(json.dumps({"case": name, "launches": [index[n] for n in names]}, separators=(",", ":")) + "\n")


def read(golden_dir):
    with open(os.path.join(golden_dir, FIXTURE)) as f:
        header, *lines = [json.loads(line) for line in f]
    return [(r["case"], [header["symbols"][i] for i in r["launches"]]) for r in lines]
