"""The launches of generate(), by name and in order: the recorder behind tests/golden/generate_launches.jsonl.

`python tools/make_golden.py generate_launches` writes the file with record() below, tests/test_generate_launch_trace_gpu.py runs the
same record() and compares.  Only the public generate() and multimeditron_amd.kernels.call are used (names only, as in
test_decode_launch_trace_gpu.py), so one recorder serves every revision of the loops behind generate().

Model: the tiny_clip_llama_d128 golden model in bf16 (head_dim 128: the shared, beam and lookup caches need it).  CASES run on its
"left" batch (B = 2, one image each, row 1 left-padded) for 4 new tokens: prefill + 3 decoder passes, the vision tower and the first-use
weight quantisation included (the MXFP8 copies are dropped before every case).  EARLY run one text-only row of 24 ids for up to 8 tokens with
sync_every = 3 and config.eos_token_idx set, for the call, to the id plain greedy decoding emits second: every row has finished by the
second step, so the number of decoder passes in the trace is where the loop looked at its done flag."""
import json
import os

import torch

from multimeditron_amd import kernels as K
from oracle import ref_cpu as R
from tests.model_utils import build_from_golden

FIXTURE = "generate_launches.jsonl"
DEVICE_SAMPLER = dict(do_sample=True, temperature=0.7, top_k=20, seed=7)
CASES = [  # name, generate() arguments
    ("greedy", dict(do_sample=False)),
    ("multinomial", dict(do_sample=True, temperature=0.7)),
    ("device_sampler", DEVICE_SAMPLER),
    ("processors", dict(do_sample=False, repetition_penalty=1.2, no_repeat_ngram_size=2)),
    ("samples3", dict(DEVICE_SAMPLER, num_return_sequences=3)),
    ("beams3", dict(do_sample=False, num_beams=3)),
    ("lookup3", dict(do_sample=False, prompt_lookup_num_tokens=3)),
    ("decode_weights", dict(do_sample=False, decode_weights="mxfp8")),
    ("kv_cache", dict(do_sample=False, kv_cache="mxfp8")),
    ("prefill_weights", dict(do_sample=False, prefill_weights="mxfp8")),
]
EARLY = [("early_greedy", dict(do_sample=False)), ("early_beams3", dict(do_sample=False, num_beams=3)),
         ("early_lookup3", dict(do_sample=False, prompt_lookup_num_tokens=3))]


def load(golden_dir, tmpdir):
    """-> (model, the "left" batch, one text-only row: the last 24 ids of the "left" batch's unpadded row)"""
    meta, w, v = R.load_golden("tiny_clip_llama_d128", golden_dir)
    model = build_from_golden(meta, w, tmpdir, "bfloat16")
    left = R.golden_batch(v, "left")
    assert bool(left["attention_mask"][0].all())
    ids = left["input_ids"][:1, -24:].clone()
    one = dict(input_ids=ids, attention_mask=torch.ones_like(ids), position_ids=torch.arange(24).view(1, 24), labels=None,
               processed_multimodal_inputs={"batch_idx": {}, "token_range": {}, "stacked": {}})
    return model, left, one


def _launches(model, batch, **kw):
    names, call = [], K.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    model.model.drop_decode_weights()
    torch.manual_seed(0)
    K.call = recording
    try:
        out = model.generate(batch, **kw)
    finally:
        K.call = call
    return names, out


def record(model, left, one):
    """-> [(case name, [C symbol, ...]), ...] in the order of CASES + EARLY"""
    rows = [(name, _launches(model, left, max_new_tokens=4, **kw)[0]) for name, kw in CASES]
    second = int(model.generate(one, max_new_tokens=2, do_sample=False)[0, -1])
    eos = model.config.eos_token_idx
    model.config.eos_token_idx = second
    try:
        for name, kw in EARLY:
            names, out = _launches(model, one, max_new_tokens=8, sync_every=3, **kw)
            n_out = (out[0] if isinstance(out, tuple) else out).shape[1]
            # greedy and lookup rows end at their second id; a beam search ends once its finished hypotheses cannot be beaten
            assert n_out < 8 if "num_beams" in kw else n_out <= 2, (name, out)
            rows.append((name, names))
    finally:
        model.config.eos_token_idx = eos
    return rows


def write(rows, golden_dir):
    """One header line with the table of symbol names, then one line per case: its launches as indices into the table."""
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
