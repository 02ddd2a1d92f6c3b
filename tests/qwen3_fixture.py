"""Loader of the Qwen3 golden fixtures (tests/golden/tiny_clip_qwen3*, written by tools/make_golden.py qwen3).  Their weights and
vectors are sharded so that every file stays below 1 MiB; meta.json's `shards` lists the files."""
import json
import os

from safetensors.torch import load_file

FIXTURES = ["tiny_clip_qwen3", "tiny_clip_qwen3_long"]


def load_qwen3_golden(name, golden_dir):
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
