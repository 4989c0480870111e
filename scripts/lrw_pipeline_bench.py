"""The LRW training inputs at the benchmark's shape (B = 32 clips of T = 29 frames, stored uint8 96 x 96 -> 96 x 96, RandomResizedCrop,
one time-mask run of up to 15 frames, CutMix on): `augment.DeviceLRWPipeline` (svsr_lrw_clip_sums + svsr_lrw_clip_mix: two launches)
beside the route a user had before: `ops.clip_prep`, `augment.TimeMask` per clip on the device, `CutMix.forward`.

    python scripts/lrw_pipeline_bench.py [--batch 32] [--frames 29] [--rounds 7] [--iters 20] [--kiters 200] [--out profiles/lrw_pipeline.json]

Both routes run in this one process on the same device-resident inputs, in alternating rounds.  Reported:
  * each route end to end, draws included (the host draws its integers inside the timed call on both sides), wall clock between device
    synchronisations, median over rounds; the acceptance condition is new <= parent;
  * launches per batch of each route, counted by the profiler hooks of `ops` for the library's entry points and from the route's
    structure for torch's kernels (TimeMask: a reduction and a fill per clip; CutMix: the gather and its copy);
  * the two new entry points alone, `--kiters` calls back to back between two device events; bytes from the shapes: the clips are read
    twice as uint8 (once by each launch) and the batch is written once as fp32 — the bound the time is set against at the 6.3 TB/s an
    MI355X sustains from HBM.  The 43 MB working set stays in the 256 MiB last-level cache between calls and launch gaps are inside the
    time, so the ratio is an end-to-end figure of the calls, not a kernel's share of the HBM peak.
Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_BPS = 6.3e12          # what an MI355X sustains from HBM (8 TB/s peak)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--stored", type=int, default=96)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kiters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrw_pipeline.json"))
    a = ap.parse_args()
    from syncvsr_amd import _lib, ops
    from syncvsr_amd.augment import CutMix, DeviceClipPipeline, DeviceLRWPipeline, TimeMask

    _lib.load()
    dev = torch.device("cuda:0")
    B, T, S, H, L, A = a.batch, a.frames, a.stored, a.size, 500, 2
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (B, T, S, S), dtype=torch.uint8, generator=g).to(dev)
    tokens = torch.randint(0, 320, (B, T * A, 2), generator=g).to(dev)
    labels = torch.randint(0, L, (B,), generator=g).to(dev)
    wm = (torch.rand(B, T, generator=g) < 0.5).float().to(dev)

    pipe = DeviceLRWPipeline(H, L, seed=0)
    clips, tmask, cutmix = DeviceClipPipeline(H, True, seed=0), TimeMask(T=15, n_mask=1), CutMix(L)

    def new_route():
        return pipe(frames, tokens, labels, wm)

    def parent_route():
        x = clips(frames)
        x = torch.stack([tmask(x[b, 0]) for b in range(B)]).unsqueeze(1)      # (TimeMask in front of Normalize is not reachable here: the
        return cutmix(x, tokens, labels, wm)                                  # same launches on the normalised clip)

    def wall(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    random.seed(0)
    torch.manual_seed(0)
    for fn in (new_route, parent_route):
        wall(fn, 3)
    nts, pts = [], []
    for _ in range(a.rounds):
        nts.append(wall(new_route, a.iters))
        pts.append(wall(parent_route, a.iters))

    ops.start_event_timing()
    new_route()
    new_launches = {k: v["launches"] for k, v in ops.stop_event_timing().items()}

    # ---- the entry points alone ----
    plan = pipe.plan(B, T, S, S, T * A)
    plan["runs"][:, 0] = torch.tensor([3, 12], dtype=torch.int32)             # every clip masks 12 frames: the sums are needed
    par, fsrc, runs = plan["params"].to(dev), plan["cutmix"].frame_src.to(torch.int32).to(dev), plan["runs"].to(dev)

    def events(fn):
        fn()
        ts = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.kiters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / a.kiters)
        return ts

    sums = ops.lrw_clip_sums(frames, par, H, H)
    sts = events(lambda: ops.lrw_clip_sums(frames, par, H, H))
    mts = events(lambda: ops.lrw_clip_mix(frames, par, fsrc, H, H, runs, sums))
    cts = events(lambda: ops.clip_prep(frames, par, H, H))
    s_us, m_us, c_us = statistics.median(sts), statistics.median(mts), statistics.median(cts)
    bound_bytes = 2 * frames.numel() + 4 * B * T * H * H
    bound_us = bound_bytes / HBM_BPS * 1e6
    new_ms, par_ms = statistics.median(nts), statistics.median(pts)
    out = dict(what="LRW training inputs: augment.DeviceLRWPipeline (svsr_lrw_clip_sums + svsr_lrw_clip_mix) vs ops.clip_prep + TimeMask per clip "
                    "on the device + CutMix.forward, same process, same inputs, alternating rounds",
               device=torch.cuda.get_device_name(0), batch=B, frames=T, stored=[S, S], size=H, n_mask=1, timemask_T=15, rounds=a.rounds,
               iters=a.iters, kiters=a.kiters,
               new_route_ms_median=round(new_ms, 3), new_route_ms_min=round(min(nts), 3),
               parent_route_ms_median=round(par_ms, 3), parent_route_ms_min=round(min(pts), 3),
               parent_over_new=round(par_ms / new_ms, 2), new_not_slower=bool(new_ms <= par_ms),
               new_route_launches=dict(new_launches, torch_small_tensor_mixing="as the parent route"),
               parent_route_launches={"svsr_clip_prep": 1, "TimeMask (clone, mean, fill) per clip": 3 * B, "stack": 1, "CutMix clip gather + contiguous": 2,
                                      "torch_small_tensor_mixing": "as the new route"},
               clip_sums_us_median=round(s_us, 2), clip_sums_us_min=round(min(sts), 2), clip_sums_bytes=frames.numel() + 4 * B * T,
               clip_mix_us_median=round(m_us, 2), clip_mix_us_min=round(min(mts), 2), clip_mix_bytes=frames.numel() + 4 * B * T * H * H,
               clip_prep_us_median=round(c_us, 2),
               bound_bytes=bound_bytes, bound="two uint8 reads of the clips + one fp32 write of the batch", bound_us_at_6p3_TBps=round(bound_us, 2),
               two_launches_us=round(s_us + m_us, 2), two_launches_over_bound=round((s_us + m_us) / bound_us, 2),
               parent_route_clip_bytes=frames.numel() + 4 * B * T * H * H * (1 + 2 + 2 + 2),
               note="routes: wall clock between synchronisations, host draws included; entry points alone: device events around back-to-back calls "
                    "on resident inputs (launch gaps and the wrapper's output allocation included, working set cache-resident between calls). "
                    "parent_route_clip_bytes: clip_prep's write, then TimeMask's clone (read + write), the stack (read + write) and CutMix's "
                    "gather (read + write) of the fp32 batch; the means read it once more per run")
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
