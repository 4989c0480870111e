"""Measures the vq-wav2vec k-means audio tokeniser (syncvsr_amd/audio_codec.VqWav2VecCodec, csrc/vq_codec.hip) at the word-level training
shape, beside a torch-eager bf16 run of its restatement (tests/vq_codec_ref.py) on the same device.

    python scripts/vq_codec_bench.py [--batch 32] [--samples 19456] [--steps 20] [--out profiles/vq_codec.json]

Prints (and with --out writes) one JSON line:
  tokenizer_ms            median time of one tokenisation (B clips of `samples` samples, keep = all frames), HIP events around the call
  layers                  per launch label: launches, ms and achieved TFLOP/s (one eager call with per-launch events)
  eager_bf16_ms           median time of the restatement's modules in bf16 (nn.Conv1d / nn.GroupNorm / argmin of the broadcast-free score form)
  token_agreement         share of tokens on which the two agree (the eager run rounds differently: near-ties flip)
Weights are the seeded full-size ones of tests/vq_codec_ref.py (timing does not depend on their values).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _time(fn, steps: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return _median(ts)


def main() -> None:
    import vq_codec_ref as R

    from syncvsr_amd import ops
    from syncvsr_amd.audio_codec import VQ_KERNELS, VqWav2VecCodec, vq_frame_counts

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=19456)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ref = R.seeded_model(1)
    codec = VqWav2VecCodec.from_state_dict(ref.state_dict(), R.fairseq_args()).to(dev)
    wave = R.synthetic_waveform(a.batch, a.samples, 5).to(dev)
    fr = vq_frame_counts(a.samples)
    gflop = 2.0 * a.batch * (2 * fr[0] * 512 * 10 + sum(fr[i] * 512 * 512 * VQ_KERNELS[i] for i in range(1, 8)) + fr[7] * 512 * (256 + 320)) / 1e9
    res = dict(batch=a.batch, samples=a.samples, audio_frames=fr, gflop=round(gflop, 1), workspace_mb=round(codec.workspace_bytes(a.batch, a.samples) / 2**20, 1))
    res["tokenizer_ms"] = round(_time(lambda: codec(wave), a.steps), 4)
    res["tokenizer_tflops"] = round(gflop / res["tokenizer_ms"], 1)
    ops.start_event_timing()
    tok = codec(wave)
    per = ops.stop_event_timing()
    res["layers"] = {k: dict(launches=v["launches"], ms=round(v["ms"], 4), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1)) for k, v in per.items()}

    eager = R.seeded_model(1).to(dev).to(torch.bfloat16)
    wave16 = wave.to(torch.bfloat16)

    def run_eager():
        with torch.no_grad():
            x = eager.feature_extractor(wave16)
            return R.scores(eager, eager.vector_quantizer.project(x)).argmin(-1)

    res["eager_bf16_ms"] = round(_time(run_eager, a.steps), 4)
    res["token_agreement"] = round(float((run_eager() == tok).float().mean()), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
