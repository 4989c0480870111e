"""The DC-TCN training inputs at the shipped configuration's shape (B = 96 clips of T = 29 frames, stored uint8 96 x 96 -> 96 x 96, no
RandomResizedCrop, one frame-mask run of up to 15 frames, the trim, mixup): `augment.DeviceDCTCNPipeline` (svsr_dctcn_clip_sums +
svsr_dctcn_clip_mix + svsr_dctcn_wave_trim: three launches) beside the same work done with torch ops per clip on the device, as a user
of `loss_and_backend_grads(train_stats=True, lam=...)` had to do it before: scale, mean fill, roll, zero, / 255, flip, Normalize per clip,
stack, and the module's own torch.lerp pass over the fp32 batch.

    python scripts/dctcn_pipeline_bench.py [--batch 96] [--frames 29] [--rounds 7] [--iters 10] [--kiters 200] [--out profiles/dctcn_pipeline.json]

Both routes run in this one process on the same device-resident inputs with the same plan per call, in alternating rounds.  Reported:
  * each route end to end, the host's draws included, wall clock between device synchronisations, median over rounds;
  * launches per batch of the new route, counted by the profiler hooks of `ops`;
  * svsr_dctcn_clip_mix alone (`--kiters` calls back to back between two device events, lam = 0.3 and lam = 0) against its HBM write
    bound: B * T * H * W * 4 bytes over the copy bandwidth measured here (a 512 MiB device-to-device copy, read + write bytes per second).
    The uint8 reads are a quarter (a half with mixup) of the written bytes on top.  The 103 MB batch fits the 256 MiB last-level cache,
    and launch gaps and the wrapper's allocation are inside the time: the ratio is an end-to-end figure of the call.
The numbers are reported, not gated.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--stored", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kiters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dctcn_pipeline.json"))
    a = ap.parse_args()
    from syncvsr_amd import _lib, ops
    from syncvsr_amd.augment import DeviceDCTCNPipeline

    _lib.load()
    dev = torch.device("cuda:0")
    B, T, S, L = a.batch, a.frames, a.stored, 640 * a.frames
    MEAN, STD = 0.421, 0.165
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (B, T, S, S), dtype=torch.uint8, generator=g).to(dev)
    waves = torch.randn(B, L, generator=g).to(dev)
    labels = torch.randint(0, 500, (B,), generator=g).to(dev)
    wbs = torch.randint(3, 20, (B,), generator=g)
    pipe = DeviceDCTCNPipeline(S, max_time_masks=15, seed=0)

    def new_route():
        return pipe(frames, waves, labels, wbs, lam=DeviceDCTCNPipeline.draw_lam(0.4))

    def torch_route():
        lam = DeviceDCTCNPipeline.draw_lam(0.4)
        plan = pipe.plan(B, T, S, S, L, wbs)
        vids, auds, words, atts = [], [], [], []
        for b in range(B):
            flip = int(plan["params"][b, 4])
            shift, trunc, moff, mlen = (int(v) for v in plan["time"][b])
            ashift, azero = (int(v) for v in plan["audio"][b])
            wb = int(wbs[b])
            v = 2 * frames[b].float() / 255 - 1
            v[moff:moff + mlen] = v.mean()
            v = v.roll(shift, 0)
            v[trunc:] = 0
            au = waves[b].roll(ashift, 0)
            au[azero:] = 0
            word = torch.zeros(T, dtype=torch.long)
            word[(T - wb) // 2:(T - wb) // 2 + wb] = 1
            word = word.roll(shift, 0)
            word[trunc:] = 0
            att = torch.ones(T, dtype=torch.long)
            att[trunc:] = 0
            x = v / 255
            if flip:
                x = x.flip(-1)
            vids.append(((x - MEAN) / STD).unsqueeze(0))
            auds.append(au)
            words.append(word)
            atts.append(att)
        videos = torch.stack(vids)
        videos = torch.lerp(videos, videos.roll(1, 0), lam)          # the module's pass (loss_and_backend_grads without videos_mixed)
        return {"videos": videos, "audios": torch.stack(auds), "labels": labels, "word_mask": torch.stack(words).to(dev),
                "attention_mask": torch.stack(atts).to(dev)}

    def wall(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    np.random.seed(0)
    for fn in (new_route, torch_route):
        wall(fn, 2)
    nts, pts = [], []
    for _ in range(a.rounds):
        nts.append(wall(new_route, a.iters))
        pts.append(wall(torch_route, a.iters))

    ops.start_event_timing()
    new_route()
    new_launches = {k: v["launches"] for k, v in ops.stop_event_timing().items()}

    def events(fn, iters):
        fn()
        ts = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / iters)
        return ts

    # ---- the copy bandwidth of this device, then the entry points alone ----
    src = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_us = statistics.median(events(lambda: dst.copy_(src), 20))
    copy_bps = 2 * src.numel() / (copy_us * 1e-6)
    del src, dst
    plan = pipe.plan(B, T, S, S, L, wbs)
    plan["time"][:, 2:] = torch.tensor([3, 12], dtype=torch.int32)            # every clip masks 12 frames: the sums are needed
    table = torch.cat([plan["params"], plan["time"]], dim=1).to(dev)
    audio = plan["audio"].to(dev)
    sums = ops.dctcn_clip_sums(frames)
    out = torch.empty((B, 1, T, S, S), dtype=torch.float32, device=dev)
    s_us = statistics.median(events(lambda: ops.dctcn_clip_sums(frames), a.kiters))
    m_us = statistics.median(events(lambda: ops.dctcn_clip_mix(frames, table, S, S, sums, 0.3, MEAN, STD, out=out), a.kiters))
    m0_us = statistics.median(events(lambda: ops.dctcn_clip_mix(frames, table, S, S, sums, 0.0, MEAN, STD, out=out), a.kiters))
    w_us = statistics.median(events(lambda: ops.dctcn_wave_trim(waves, audio), a.kiters))
    write_bytes = 4 * B * T * S * S
    bound_us = write_bytes / copy_bps * 1e6
    new_ms, par_ms = statistics.median(nts), statistics.median(pts)
    res = dict(what="DC-TCN training inputs: augment.DeviceDCTCNPipeline (svsr_dctcn_clip_sums + svsr_dctcn_clip_mix + svsr_dctcn_wave_trim) vs the "
                    "same work with torch ops per clip on the device + the module's torch.lerp, same process, same inputs, alternating rounds",
               device=torch.cuda.get_device_name(0), batch=B, frames=T, stored=[S, S], size=[S, S], wave_samples=L, max_time_masks=15,
               rounds=a.rounds, iters=a.iters, kiters=a.kiters,
               new_route_ms_median=round(new_ms, 3), new_route_ms_min=round(min(nts), 3),
               torch_route_ms_median=round(par_ms, 3), torch_route_ms_min=round(min(pts), 3), torch_over_new=round(par_ms / new_ms, 2),
               new_route_launches=new_launches,
               copy_512MiB_us=round(copy_us, 1), copy_bandwidth_TBps=round(copy_bps / 1e12, 3),
               clip_sums_us_median=round(s_us, 2), clip_mix_us_median_lam0p3=round(m_us, 2), clip_mix_us_median_lam0=round(m0_us, 2),
               wave_trim_us_median=round(w_us, 2),
               clip_mix_write_bytes=write_bytes, clip_mix_read_bytes_lam0p3=2 * frames.numel(), clip_mix_read_bytes_lam0=frames.numel(),
               clip_mix_write_bound_us=round(bound_us, 2), clip_mix_over_write_bound_lam0p3=round(m_us / bound_us, 2),
               clip_mix_over_write_bound_lam0=round(m0_us / bound_us, 2),
               note="routes: wall clock between synchronisations, host draws included; entry points alone: device events around back-to-back "
                    "calls on resident inputs into one output buffer (launch gaps included, working set cache-resident between calls); "
                    "copy bandwidth: read + written bytes of a 512 MiB device-to-device torch copy per second. Reported, not gated.")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
