"""Loader of the Apertus golden fixtures (tests/golden/tiny_clip_apertus*, written by tools/make_golden.py apertus).  Their weights
and vectors are sharded so that every file stays below 1 MiB; meta.json's `shards` lists the files.  The weights carry the xIELU
state under HF's names: `mlp.act_fn.alpha_p` / `alpha_n` ([1]) and the buffers `mlp.act_fn.beta` / `eps` (0-dim, eps = bf16(-1e-6))."""
import json
import os

from safetensors.torch import load_file

FIXTURES = ["tiny_clip_apertus", "tiny_clip_apertus_long"]


def load_apertus_golden(name, golden_dir):
    """-> (meta, weights, vectors) like oracle.ref_cpu.load_golden."""
    meta = json.load(open(os.path.join(golden_dir, f"{name}.meta.json")))
    out = []
    for kind in ("weights", "vectors"):
        d = {}
        for f in meta["shards"][kind]:
            part = load_file(os.path.join(golden_dir, f))
            assert not set(part) & set(d), f
            d.update(part)
        out.append(d)
    return meta, out[0], out[1]
