"""The LRS input transforms at the LRS benchmark batch of bench.py (16 clips of its longest length bucket): `lrs_data.DeviceLRSPipeline` on
`collate_packed`'s uint8 crops and int16 waveforms (svsr_lrs_clip_prep + svsr_wave_prep: three launches) beside the route a user had
before: the same transforms per sample in torch on the CPU (16 threads), `collate_pad`, and an upload of the padded fp32 batch.

    python scripts/lrs_pipeline_bench.py [--batch 16] [--frames 150] [--rounds 7] [--iters 20] [--kiters 300] [--out profiles/lrs_pipeline.json]

Inputs: seeded synthetic stored crops (uint8 96 x 96), int16 waveforms of 640 samples per frame and a 60 s fp32 noise bank; the lengths are
the ones bench.py's LRS leg draws (lrs_bucket_batch).  Reported, not gated:
  * the two kernels' entry points alone, on device-resident inputs: `--kiters` calls back to back between two device events, median over
    rounds.  Bytes are counted from the shapes (video: every stored byte of the real frames read once + 4 bytes written per output element,
    padding included; audio: samples and noise of the real spans read by both launches + 4 bytes written per padded sample) and set against
    the 6.3 TB/s an MI355X sustains from HBM; launch gaps are inside the time, and a 20 - 100 MB working set stays in the 256 MiB last-level cache
    between calls, so the rate is an end-to-end figure of the call, not a kernel's share of the HBM peak;
  * the whole device route, pinned host batch -> device batch (uploads, draws, three launches), wall clock between synchronisations;
  * the CPU route on torch.set_num_threads(16): transforms + collate_pad, and the upload of its pinned fp32 result, separately;
  * host-to-device bytes of both routes: the frames and waveforms (and the per-clip numbers the kernels read); the lengths and targets, a few
    hundred bytes that both routes upload alike, are left out of both counts.
The two routes use different random streams, so only their shapes are compared.  Prints one JSON line and writes it to --out."""
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
import torch.nn.functional as F  # noqa: E402

HBM_BPS = 6.3e12          # what an MI355X sustains from HBM (8 TB/s peak)
SIZE, SPF = 96, 640


def cpu_sample(clip_u8, wave_i16, noise, rng):
    """One sample of the reference's train transforms in torch fp32 (transforms.py:89-135), draws from `rng`."""
    import math

    x = clip_u8.float().unsqueeze(1) / 255.0
    Hs, Ws = x.shape[-2:]
    top, left, h, w = 0, 0, Hs, Ws
    for _ in range(10):
        target = Hs * Ws * rng.uniform(0.7, 1.0)
        ratio = math.exp(rng.uniform(math.log(96 / 112), math.log(112 / 96)))
        ww, hh = int(round(math.sqrt(target * ratio))), int(round(math.sqrt(target / ratio)))
        if 0 < ww <= Ws and 0 < hh <= Hs:
            top, left, h, w = int(rng.integers(0, Hs - hh + 1)), int(rng.integers(0, Ws - ww + 1)), hh, ww
            break
    x = F.interpolate(x[:, :, top:top + h, left:left + w], size=(SIZE, SIZE), mode="bilinear", align_corners=False)
    if rng.random() < 0.5:
        x = x.flip(-1)
    x = (x - 0.421) / 0.165
    a = wave_i16.float() / 32768.0
    start = int(rng.integers(0, noise.numel() - a.numel() + 1))
    n = noise[start:start + a.numel()]
    snr = (-5, 0, 5, 10, 15, 20, 999999)[int(rng.integers(0, 7))]
    a = a + torch.sqrt(a.pow(2).sum() / n.pow(2).sum()) * 10.0 ** (-snr / 20.0) * n
    return x, F.layer_norm(a, a.shape, eps=1e-8)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kiters", type=int, default=300)
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrs_pipeline.json"))
    a = ap.parse_args()
    from syncvsr_amd import _lib, ops
    from syncvsr_amd.lrs_data import DeviceLRSPipeline, LengthBucketBatchSampler, collate_pad, collate_packed, reference_length_histogram

    _lib.load()
    dev = torch.device("cuda:0")
    # bench.py lrs_bucket_batch: the longest bucket of the reference's length histogram rescaled to --frames
    pool = reference_length_histogram(4096, seed=7) * a.frames // 155
    sampler = LengthBucketBatchSampler(pool, a.batch, 1, 0, width=16, seed=11)
    step = max(range(len(sampler)), key=lambda i: sampler.padded_frames()[i])
    lens, Tpad = [int(v) for v in pool[list(sampler)[step]]], sampler.padded_frames()[step]
    g = torch.Generator().manual_seed(1)
    noise = torch.randn(60 * 16000, generator=g) * 0.1
    samples = [{"input": torch.randint(0, 256, (T, SIZE, SIZE), dtype=torch.uint8, generator=g),
                "audio": (torch.randn(T * SPF, generator=g) * 0.1 * 32768).to(torch.int16), "target": torch.randint(1, 5000, (20,), generator=g)} for T in lens]
    B, Spad = len(lens), Tpad * SPF

    # ---- the device route ----
    pipe = DeviceLRSPipeline(train=True, size=SIZE, seed=0, noise=noise)
    packed = collate_packed(samples, pad_frames_to=Tpad)
    batch = pipe(packed)                                                          # warm-up (uploads the noise bank)
    torch.cuda.synchronize()
    assert batch["inputs"].shape == (B, Tpad, 1, SIZE, SIZE) and batch["audios"].shape == (B, 1, Spad)

    def device_side():
        return pipe(packed)

    # ---- the CPU route ----
    torch.set_num_threads(16)
    rng = np.random.default_rng(0)

    def cpu_side():
        out = []
        for s in samples:
            x, au = cpu_sample(s["input"], s["audio"], noise, rng)
            out.append({"input": x, "audio": au, "target": s["target"]})
        return collate_pad(out, pad_frames_to=Tpad, frames_per_unit={"audio": SPF})

    ref = cpu_side()
    assert ref["inputs"].shape == batch["inputs"].shape and ref["audios"].shape == batch["audios"].shape
    pinned = {k: ref[k].pin_memory() for k in ("inputs", "audios")}

    def upload_fp32():
        return [pinned[k].to(dev, non_blocking=True) for k in ("inputs", "audios")]

    def wall(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    upload_fp32()
    dts, cts, uts = [], [], []
    for _ in range(a.rounds):
        dts.append(wall(device_side, a.iters))
        uts.append(wall(upload_fp32, a.iters))
    for _ in range(max(a.cpu_iters, 1)):
        cts.append(wall(cpu_side, 1))

    # ---- the entry points alone, device-resident inputs ----
    draws = pipe.draw(lens, SIZE, SIZE, [T * SPF for T in lens], Tpad)
    frames_d, wave_d = packed["frames"].to(dev), packed["audios"].to(dev)
    off_d, par_d = packed["offsets"].to(dev), draws["params"].to(dev)
    alen_d, nst_d, snr_d = packed["audio_lengths"].to(torch.int32).to(dev), draws["nstart"].to(dev), draws["snr_db"].to(dev)

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

    vts = events(lambda: ops.lrs_clip_prep(frames_d, off_d, par_d, Tpad, SIZE, SIZE))
    ats = events(lambda: ops.wave_prep(wave_d, alen_d, pipe.noise, nst_d, snr_d))
    real_frames, real_samples = sum(lens), sum(lens) * SPF
    v_bytes = real_frames * SIZE * SIZE + 4 * B * Tpad * SIZE * SIZE
    a_bytes = 2 * real_samples * (2 + 4) + 4 * B * Spad
    v_us, a_us = statistics.median(vts), statistics.median(ats)
    h2d_dev = packed["frames"].numel() + packed["audios"].numel() * 2 + 4 * (9 * B + 1)
    h2d_cpu = 4 * (ref["inputs"].numel() + ref["audios"].numel())
    out = dict(what="LRS input transforms: lrs_data.DeviceLRSPipeline (uint8 crops + int16 waveforms up, three launches) vs the same transforms per "
                    "sample in torch on 16 CPU threads + collate_pad + an upload of the padded fp32 batch",
               device=torch.cuda.get_device_name(0), batch=B, padded_frames=Tpad, lengths=lens, real_frames=real_frames, stored=[SIZE, SIZE], size=SIZE,
               padded_samples=Spad, noise_bank_samples=noise.numel(), rounds=a.rounds, iters=a.iters, kiters=a.kiters, cpu_threads=torch.get_num_threads(),
               clip_prep_us_median=round(v_us, 2), clip_prep_us_min=round(min(vts), 2), clip_prep_bytes=v_bytes,
               clip_prep_GBps=round(v_bytes / (v_us * 1e-6) / 1e9, 1), clip_prep_share_of_6p3_TBps=round(v_bytes / (v_us * 1e-6) / HBM_BPS, 3),
               wave_prep_us_median=round(a_us, 2), wave_prep_us_min=round(min(ats), 2), wave_prep_bytes=a_bytes,
               wave_prep_GBps=round(a_bytes / (a_us * 1e-6) / 1e9, 1), wave_prep_share_of_6p3_TBps=round(a_bytes / (a_us * 1e-6) / HBM_BPS, 3),
               device_route_ms_median=round(statistics.median(dts), 3), device_route_ms_min=round(min(dts), 3), device_route_h2d_bytes=h2d_dev,
               cpu_transforms_ms_median=round(statistics.median(cts), 1), cpu_transforms_ms_min=round(min(cts), 1),
               cpu_route_upload_ms_median=round(statistics.median(uts), 3), cpu_route_h2d_bytes=h2d_cpu, h2d_ratio=round(h2d_cpu / h2d_dev, 2),
               note="entry points alone: device events around back-to-back calls on resident inputs (launch gaps and the wrapper's output allocation "
                    "included, working set cache-resident between calls: a rate of the call, not an HBM share of the kernel); routes: wall clock "
                    "between synchronisations; the CPU figure shares the host with other work")
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
