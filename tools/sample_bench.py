#!/usr/bin/env python3
"""mm_sample alone on the decoder's vocabulary (V = 128 258, bf16 logits) beside the greedy selection mm_argmax_softmax_split on the
same rows, and the logits processors' launch mm_logits_process (repetition penalty 1.2, 3-gram ban, a history of 2048 + 512 ids) on
them, and classifier-free guidance's mm_cfg_combine (two launches) on 1 / 4 / 8 pairs of such rows (run on the GPU box).  HIP events
around 200 back-to-back calls after 20 warm-up calls.
   python tools/sample_bench.py [--iters N]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multimeditron_amd import kernels as K

CONFIGS = [("plain", dict()), ("top_k=50", dict(top_k=50)), ("top_p=0.95", dict(top_p=0.95)),
           ("top_k=50+top_p=0.9", dict(top_k=50, top_p=0.9))]


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--V", type=int, default=128258)
    args = ap.parse_args()
    V, ld = args.V, (args.V + 63) // 64 * 64
    torch.manual_seed(0)
    for rows in (1, 4, 16):
        buf = (torch.randn(rows, ld, device="cuda") * 3).to(torch.bfloat16)
        lg = buf[:, :V]
        ws = K.sample_ws(rows, V, "cuda")
        out = torch.empty(rows, dtype=torch.int64, device="cuda")
        greedy = timed(lambda: K.argmax_softmax(lg, V, 0.7), args.iters)
        line = [f"rows={rows:2d}  argmax_softmax_split {greedy:6.1f} us"]
        for name, kw in CONFIGS:
            us = timed(lambda: K.sample(lg, V, 0.7, seed=1, offset=0, ws=ws, out=out, **kw), args.iters)
            line.append(f"{name} {us:6.1f} us")
        print(" | ".join(line), flush=True)
        # the logits processors' one launch on the same rows: a history of 2048 prompt + 512 generated ids, p = 1.2, g = 3; then the
        # history scans alone (p = 1, g = 0 with min_new_tokens: the copy to fp32 and one banned id)
        hist_len, room = 2048 + 512, 8
        st = K.LogitsState(rows, V, "cuda", 1.2, 3, prompt_ids=torch.randint(0, V, (rows, hist_len), device="cuda"),
                           prompt_mask=torch.ones(rows, hist_len, dtype=torch.long, device="cuda"), room=room)
        last = torch.randint(0, V, (rows,), device="cuda")
        full = timed(lambda: K.logits_process(lg, st, room, last, 0), args.iters)          # step = room: the same slot every call
        st0 = K.LogitsState(rows, V, "cuda", min_new_tokens=room + 1)
        copy = timed(lambda: K.logits_process(lg, st0, room, last, 0), args.iters)
        mb = rows * V * 6 / 1e6
        print(f"rows={rows:2d}  logits_process p=1.2 g=3 history {hist_len + room} {full:6.1f} us | no history (min_new_tokens only) "
              f"{copy:6.1f} us | {mb:.1f} MB of logits in and scores out, {mb / full:.2f} TB/s", flush=True)
    # classifier-free guidance: the conditional and the unconditional rows of one logits tensor -> fp32 scores (2 launches)
    for pairs in (1, 4, 8):
        lg = (torch.randn(2 * pairs, ld, device="cuda") * 3).to(torch.bfloat16)[:, :V]
        st = K.GuidanceState(pairs, V, "cuda")
        us = timed(lambda: K.cfg_combine(lg, st, 3.0), args.iters)
        mb = pairs * V * (2 * 2 * 2 + 4) / 1e6               # both rows read twice (bf16), the scores written once (fp32)
        print(f"pairs={pairs:2d} ({2 * pairs:2d} rows)  cfg_combine {us:6.1f} us | {mb:.1f} MB of logits in (twice) and scores out, "
              f"{mb / us:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
