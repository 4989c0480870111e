#!/usr/bin/env python
"""A bucketed LRS epoch prefix, eager against one recorded step list per batch shape (engine.TrainStep(native=True, max_shapes=...)).

The full LRS config at B = 16, the first --steps steps in sampler order of lrs_data.LengthBucketBatchSampler over the reference's length
histogram (width 16, clips <= 160 frames), targets padded to a multiple of 16 tokens (lrs_data.collate_pad).  Pass 1 runs the steps
once with a synchronisation after each (the recording steps of the native mode happen here and are timed); pass 2 runs the same steps
again back to back and gives the throughput.  One mode per process; one JSON line:

    timeout -k 10 900 python scripts/lrs_mix.py --mode eager && timeout -k 10 900 python scripts/lrs_mix.py --mode native
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import syncvsr_amd  # noqa: E402,F401  (sets the hardware-queue count before the HIP runtime starts)

import torch  # noqa: E402


def batches(args, lrs_args, odim, dev):
    """-> [(device batch, valid frames, padded frames)] of the first args.steps steps of epoch 0."""
    from syncvsr_amd.lrs_data import LengthBucketBatchSampler, collate_pad, reference_length_histogram
    from syncvsr_amd.lrs_init import lrs_synthetic_batch

    pool = reference_length_histogram(4096, seed=7)
    sampler = LengthBucketBatchSampler(pool, args.batch, width=16, max_frames=args.max_frames, seed=11)
    out = []
    for i, (idx, bound) in enumerate(zip(sampler, sampler.padded_frames())):
        if i == args.steps:
            break
        lengths = torch.as_tensor(sampler.lengths[idx])
        x, lens, tokens, label = lrs_synthetic_batch(lrs_args, args.batch, int(bound), odim=odim, seed=1000 + i, lengths=lengths)
        rows = [{"target": r[0][r[0] != -1]} for r in label]
        label = collate_pad(rows, pad_targets_to_multiple=args.target_multiple)["targets"]
        out.append(([x.to(dev), lens.to(dev), tokens.to(dev), label.to(dev)], int(lengths.sum()), int(bound) * args.batch))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("eager", "native"), required=True)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max-frames", type=int, default=160)
    ap.add_argument("--target-multiple", type=int, default=16)
    ap.add_argument("--dropout", type=float, default=0.1)
    args = ap.parse_args()

    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_init import LRS_ODIM, default_lrs_args
    from syncvsr_amd.lrs_model import E2E
    from syncvsr_amd.shape_cache import shape_key

    dev = torch.device("cuda:0")
    lrs_args = default_lrs_args(dropout_rate=args.dropout, transformer_attn_dropout_rate=args.dropout)
    model = E2E(LRS_ODIM, lrs_args, seed=0).to(dev).train()
    steps = batches(args, lrs_args, LRS_ODIM, dev)
    keys = {shape_key(model.prepare_batch(*b)) for b, _, _ in steps}
    kw = dict(native=True, max_shapes=len(keys)) if args.mode == "native" else {}
    ts = TrainStep(model, lrs_train_config(), **kw)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()

    # pass 1: every step synchronised; the native mode records each key at its first occurrence
    rec_ms, first_ms = [], []
    seen = set()
    for b, _, _ in steps:
        k = shape_key(model.prepare_batch(*b))
        t0 = time.perf_counter()
        ts.step(*b)
        torch.cuda.synchronize()
        (first_ms if k not in seen else rec_ms).append((time.perf_counter() - t0) * 1e3)
        seen.add(k)
    # pass 2: the same steps back to back
    ts.host_ms.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b, _, _ in steps:
        ts.step(*b)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    state = ts.state()

    def med(v):
        return round(sorted(v)[len(v) // 2], 3) if v else None

    n = len(steps)
    out = {"mode": args.mode, "steps": n, "batch": args.batch, "keys": len(keys),
           "clips_per_s": round(n * args.batch / el, 2),
           "valid_frames_per_s": round(sum(v for _, v, _ in steps) / el, 1),
           "padded_frames_per_s": round(sum(p for _, _, p in steps) / el, 1),
           "ms_per_step": round(el / n * 1e3, 3),
           "host_ms_per_step": med(ts.host_ms),
           "first_occurrence_step_ms": med(first_ms),        # native: the recording steps
           "repeat_step_ms": med(rec_ms),                     # synchronised steps of a key seen before
           "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
           "skipped_steps": state["skipped_steps"]}
    if args.mode == "native":
        shapes = ts.recorded_shapes()
        b = [v["bytes"] for v in shapes.values()]
        out.update(lists=len(shapes), recorded_bytes_mean_gb=round(sum(b) / len(b) / 2 ** 30, 3), recorded_bytes_max_gb=round(max(b) / 2 ** 30, 3),
                   recorded_bytes_total_gb=round(sum(b) / 2 ** 30, 2), launches_mean=round(sum(v["launches"] for v in shapes.values()) / len(shapes)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
