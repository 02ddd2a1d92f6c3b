"""The launches of CausalLM.forward on every inference route, by name and in order, recorded without a GPU: the recorder behind
tests/golden/decoder_routes.jsonl.

`python tools/make_golden.py decoder_routes` writes the file with record() below, tests/test_decoder_routes_cpu.py runs the same record()
and compares.  Nothing is launched: multimeditron_amd.kernels.call is replaced by a function that notes the C symbol, kernels._p by a
constant and kernels._stream by 0, so the decoder walks its routes on CPU tensors whose values are never read (the host-side queries
of the built library -- buffer sizes, split counts -- are the real ones).  Only the public surface is used (CausalLM, new_cache,
forward with inputs_embeds, the caches' `tables` / `shared` holders), so one recorder serves every revision of what lies between.

Models: the 1-layer tiny decoder of test_decode_launch_trace_gpu.py (hidden 256, intermediate 384, 2 query heads on 1 key/value head of
128, vocab 1003) in the four families, and "llama-wide", the same with intermediate 4608: there 16 rows of 4608 bf16 features exceed
the weight-streaming kernel's LDS stage, 8 rows do not.  CASES is the full product FAMILIES x FUSED x CACHES x WEIGHTS plus WIDE; a
combination that new_cache, quantize_decode_weights or forward refuses is recorded as the exception's text."""
import itertools
import json
import os
from contextlib import contextmanager

import torch

from multimeditron_amd import kernels as K

FIXTURE = "decoder_routes.jsonl"
S_, Q_ = 37, 4          # prompt positions; positions of a verify step (lookup = 3 drafts + 1)

FAMILIES = {  # model_type, attention_bias, qk_norm, hidden_act
    "llama": ("llama", False, False, "silu"),
    "qwen2": ("qwen2", True, False, "silu"),
    "qwen3": ("qwen3", False, True, "silu"),
    "apertus": ("apertus", False, True, "xielu"),
}
FUSED = ("1", "0")      # MM_DECODE_FUSED
# name -> (prompts, new_cache arguments, rows of the step, positions of the step, model dtype[, prompt positions])
CACHES = {
    "plain": (2, {}, 2, 1, torch.bfloat16),
    "kv8": (2, {"kv_cache": "mxfp8"}, 2, 1, torch.bfloat16),
    "samples3": (2, {"samples": 3, "prompt_len": S_}, 6, 1, torch.bfloat16),
    "beams3": (2, {"beams": 3, "prompt_len": S_}, 6, 1, torch.bfloat16),
    "lookup3": (2, {"lookup": 3}, 2, Q_, torch.bfloat16),
    "lookup3-S1": (2, {"lookup": 3}, 2, Q_, torch.bfloat16, 1),      # a one-token prompt: its prefill is S = 1 into the empty cache
    "rows17": (17, {}, 17, 1, torch.bfloat16),
    "fp32": (2, {}, 2, 1, torch.float32),
}
# name -> (forward arguments of the prefill, of the step)
WEIGHTS = {
    "bf16": ({}, {}),
    "dw": ({}, {"decode_weights": "mxfp8"}),
    "dw+pw": ({"prefill_weights": "mxfp8"}, {"decode_weights": "mxfp8"}),
}
# the wide model's verify steps: 4 x 4 = 16 rows (fused down_proj must be mm_gemm) and 2 x 4 = 8 rows (mm_decode_linear)
WIDE = [("llama-wide", f, c, w) for f in FUSED for c in ("lookup3-B4", "lookup3-B2") for w in ("bf16", "dw")]
WIDE_CACHES = {"lookup3-B4": (4, {"lookup": 3}, 4, Q_, torch.bfloat16), "lookup3-B2": CACHES["lookup3"]}

CASES = list(itertools.product(FAMILIES, FUSED, CACHES, WEIGHTS)) + WIDE


def case_id(case):
    return "-".join((case[0], "fused" if case[1] == "1" else "separate") + tuple(case[2:]))


def decoder(family, dtype, intermediate=384):
    from multimeditron_amd.model.llm import CausalLM, LLMConfig
    from multimeditron_amd.nn import FlatParams
    mt, bias, qkn, act = FAMILIES[family]
    cfg = LLMConfig(model_type=mt, hidden_size=256, intermediate_size=intermediate, num_hidden_layers=1, num_attention_heads=2,
                    num_key_value_heads=1, head_dim=128, vocab_size=1003, attention_bias=bias, qk_norm=qkn, hidden_act=act,
                    pad_token_id=3 if mt == "apertus" else None)
    m = CausalLM(cfg, dtype=dtype, device="cpu")
    FlatParams([(k, p, "llm") for k, p in m.named_parameters()], "cpu", dtype)
    return m.eval()


@contextmanager
def recording(names):
    """kernels.call notes the symbol and launches nothing; pointers and the stream are constants"""
    saved = K.call, K._p, K._stream
    K.call, K._p, K._stream = (lambda name, *args: names.append(name)), (lambda t: None if t is None else 4096), (lambda: 0)
    try:
        yield
    finally:
        K.call, K._p, K._stream = saved


def _one(case):
    """-> {"prefill": [symbols] or the refusal's text, "step": the same}; what follows a refusal is absent"""
    family, fused, cache_name, weights = case
    wide = family == "llama-wide"
    B, cache_kw, rows, Q, dtype, Sp = ((WIDE_CACHES if wide else CACHES)[cache_name] + (S_,))[:6]
    kw_prefill, kw_step = WEIGHTS[weights]
    out, names = {}, []
    os.environ["MM_DECODE_FUSED"] = fused
    with recording(names), torch.no_grad():
        m = decoder("llama" if wide else family, dtype, 4608 if wide else 384)
        H = m.config.hidden_size
        stage = "prefill"
        try:
            if kw_step:
                m.quantize_decode_weights()                       # outside the traces: forward would make them on first use
            cache = m.new_cache(B, Sp + 2 * Q, **cache_kw)
            c0 = cache[0]
            if "lookup" in cache_kw:                              # as generate's loop: the base positions stand before the prefill
                c0.shared.base, c0.shared.bound = torch.full((B,), Sp, dtype=torch.int32), Sp
            del names[:]
            m(inputs_embeds=torch.zeros(B, Sp, H, dtype=dtype), past_key_values=cache, use_cache=True, logits_to_keep=1, **kw_prefill)
            out["prefill"] = list(names)
            stage = "step"
            if "beams" in cache_kw:
                c0.tables.current = torch.zeros((2, rows), dtype=torch.int32)
            pos = (torch.arange(Q) + Sp).unsqueeze(0).expand(rows, Q)
            del names[:]
            m(inputs_embeds=torch.zeros(rows, Q, H, dtype=dtype), past_key_values=cache, use_cache=True, position_ids=pos,
              logits_to_keep=0 if Q > 1 else 1, **kw_step)
            out["step"] = list(names)
        except (ValueError, NotImplementedError) as e:
            out[stage] = f"{type(e).__name__}: {e}"
    return out


def record():
    """-> [(case id, {"prefill": ..., "step": ...}), ...] in the order of CASES"""
    fused = os.environ.get("MM_DECODE_FUSED")
    try:
        return [(case_id(c), _one(c)) for c in CASES]
    finally:
        os.environ.pop("MM_DECODE_FUSED", None)
        if fused is not None:
            os.environ["MM_DECODE_FUSED"] = fused


def write(rows, golden_dir):
    """One header line with the table of symbol names, then one line per case: its launches as indices into the table, a refusal as
    its text."""
    table = sorted({n for _, r in rows for v in r.values() if isinstance(v, list) for n in v})
    index = {n: i for i, n in enumerate(table)}
    with open(os.path.join(golden_dir, FIXTURE), "w") as f:
        f.write(json.dumps({"symbols": table}, separators=(",", ":")) + "\n")
        for name, r in rows:
            enc = {k: [index[n] for n in v] if isinstance(v, list) else v for k, v in r.items()}
            f.write(json.dumps({"case": name, **enc}, separators=(",", ":")) + "\n")


def read(golden_dir):
    with open(os.path.join(golden_dir, FIXTURE)) as f:
        header, *lines = [json.loads(line) for line in f]
    sym = header["symbols"]
    return [(r.pop("case"), {k: [sym[i] for i in v] if isinstance(v, list) else v for k, v in r.items()}) for r in lines]
