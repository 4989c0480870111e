#!/usr/bin/env python
"""The shipped LRW encoder (xtransformers_lrw_config(True): x-transformers, depth 12, 513 wide, layer drop 0.2, ff-dropout 0.3), eager
against the native step list (engine.TrainStep(native=True): every block an op group, the skipped ones left out per step).

Per batch size (29 x 88 x 88 clips) and mode, a fresh model from the same seed — so both modes draw the same skipped blocks step for step —
runs --warmup steps (the native mode records its list in the first), then --steps back-to-back steps timed with HIP events on the main
stream; host_ms is the median enqueue time of TrainStep.step over the timed steps.  One JSON line:

    timeout -k 10 900 python scripts/xt_native_ab.py --batches 32,96
"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import syncvsr_amd  # noqa: E402,F401  (sets the hardware-queue count before the HIP runtime starts)

import torch  # noqa: E402


def measure(B: int, native: bool, args) -> dict:
    from syncvsr_amd.config import xtransformers_lrw_config
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.init import synthetic_batch
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg = xtransformers_lrw_config(True)
    cfg.train.batch_size = B
    model = Model(cfg, seed=0).to(dev).train()
    batch = [t.to(dev) for t in synthetic_batch(cfg, B, seed=1234)]
    ts = TrainStep(model, cfg, native=native)
    for _ in range(args.warmup):
        ts.step(*batch)
        if native and ts.input_buffers() is not None:
            batch = list(ts.input_buffers())          # the loader writes into the recorded inputs (bench.py's default)
    torch.cuda.synchronize()
    ts.host_ms.clear()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        ts.step(*batch)
    e1.record()
    ts.synchronize()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    host = sorted(ts.host_ms[-args.steps:])
    state = ts.state()
    out = {"ms_per_step": round(ms, 3), "host_ms": round(host[len(host) // 2], 3), "clips_per_s": round(B * 1e3 / ms, 1),
           "skipped_steps": state["skipped_steps"]}
    if native:
        out["launches_recorded"] = ts._rec.calls()
        out["launches_last_replay"] = ts._rec.last_issued
    del ts, model, batch
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,96")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    if args.steps < 50:
        raise SystemExit("--steps must be >= 50")
    rows = []
    for B in (int(b) for b in args.batches.split(",")):
        e = measure(B, False, args)
        n = measure(B, True, args)
        rows.append({"batch": B, "eager": e, "native": n, "native_speedup": round(e["ms_per_step"] / n["ms_per_step"], 3)})
    print(json.dumps({"workload": "lrw-xt (depth 12, word boundary, layer drop 0.2), 29x88x88", "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0), "results": rows}), flush=True)


if __name__ == "__main__":
    main()
