"""Measures the wav2vec2 audio tokeniser (syncvsr_amd/audio_codec.py, csrc/w2v_codec.hip) at the LRS benchmark shape and its cost inside the
LRS training step.

    python scripts/codec_bench.py [--batch 16] [--frames 160] [--steps 20] [--mode layer|group]

Prints one JSON line:
  tokenizer_ms            median time of one tokenisation (B clips of frames * 640 samples + 8000 zeros), HIP events around the call
  layers                  per launch label: ms and achieved TFLOP/s (one eager call with per-launch events)
  step_tokens_ms          TrainStep(native=True) step time of the shipped LRS E2E fed pre-computed tokens
  step_waveform_ms        the same step fed waveforms (tokenised inside the step, training-mode sampling on)
  peak_gb_tokens / peak_gb_waveform   torch.cuda.max_memory_allocated after each leg
Weights are the seeded full-size ones of tests/w2v_codec_ref.py (timing does not depend on their values).
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


def tokenizer_leg(codec, wave, steps: int) -> dict:
    from syncvsr_amd import ops
    from syncvsr_amd.audio_codec import LRS_PAD

    for _ in range(3):
        codec(wave, pad=LRS_PAD)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        codec(wave, pad=LRS_PAD)
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ops.start_event_timing()
    codec(wave, pad=LRS_PAD)
    per = ops.stop_event_timing()
    layers = {k: dict(launches=v["launches"], ms=round(v["ms"], 4), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1)) for k, v in per.items()}
    return dict(tokenizer_ms=round(_median(ts), 4), layers=layers)


def step_leg(codec, B: int, T: int, steps: int, waveform: bool) -> dict:
    import w2v_codec_ref as R

    from syncvsr_amd.audio_codec import LRS_PAD
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_init import LRS_ODIM, default_lrs_args, lrs_synthetic_batch
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args = default_lrs_args(dropout_rate=0.1, transformer_attn_dropout_rate=0.1, codec="wav2vec2")
    model = E2E(LRS_ODIM, args, seed=0).to(dev).train()
    model.reseed_dropout(1000)
    x, lengths, tokens, label = lrs_synthetic_batch(args, B, T, odim=LRS_ODIM, seed=1234, label_len=(5, 20))
    wave = R.synthetic_waveform(B, T * 640, 5).to(dev)
    if waveform:
        model.attach_audio_codec(codec, sample_in_training=True)
        audios = wave
    else:
        audios = codec(wave, pad=LRS_PAD, keep=2 * T)
    batch = (x.to(dev), lengths.to(dev), audios, label.to(dev))
    torch.cuda.reset_peak_memory_stats()
    ts = TrainStep(model, lrs_train_config(), native=True)
    for _ in range(3):
        ts.step(*batch)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        ts.step(*batch)
    e.record()
    e.synchronize()
    ts.synchronize()
    out = dict(ms=round(s.elapsed_time(e) / steps, 3), peak_gb=round(torch.cuda.max_memory_allocated() / 2**30, 2))
    del ts, model
    torch.cuda.empty_cache()
    return out


def main() -> None:
    import w2v_codec_ref as R

    from syncvsr_amd.audio_codec import LRS_PAD, Wav2Vec2Codec, frame_counts

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mode", default="layer", choices=["layer", "group"])
    ap.add_argument("--no-step", action="store_true", help="tokeniser only")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    codec = Wav2Vec2Codec.from_state_dict(R.seeded_weights(a.mode, 1), R.hf_config_kwargs(a.mode)).to(dev)
    wave = R.synthetic_waveform(a.batch, a.frames * 640, 5).to(dev)
    L = a.frames * 640 + LRS_PAD
    fr = frame_counts(L)
    gflop = 2.0 * a.batch * (fr[0] * 512 * 10 + sum(fr[i] * 512 * 512 * k for i, k in zip(range(1, 7), (3, 3, 3, 3, 2, 2))) + fr[6] * 512 * 640) / 1e9
    res = dict(mode=a.mode, batch=a.batch, frames=a.frames, samples=L, audio_frames=fr, gflop=round(gflop, 1),
               workspace_mb=round(codec.workspace_bytes(a.batch, L) / 2**20, 1))
    res.update(tokenizer_leg(codec, wave, a.steps))
    res["tokenizer_tflops"] = round(gflop / res["tokenizer_ms"], 1)
    if not a.no_step:
        t = step_leg(codec, a.batch, a.frames, a.steps, waveform=False)
        w = step_leg(codec, a.batch, a.frames, a.steps, waveform=True)
        res.update(step_tokens_ms=t["ms"], step_waveform_ms=w["ms"], peak_gb_tokens=t["peak_gb"], peak_gb_waveform=w["peak_gb"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
