"""Torch restatement of the LRS input transforms (reference LRS/video/datamodule/transforms.py:89-135, av_dataset.py:30-41, data_module.py:12-43)
on the CPU, the yardstick of tests/test_lrs_pipeline_cpu.py and tests/test_gpu_lrs_pipeline.py.  torchvision and torchaudio cannot be imported
here, so their formulas are written out:

  video   Normalize(mean, std)(flip(resize(window(x / 255)))), resize = F.interpolate(mode="bilinear", align_corners=False, antialias=False),
          a frame marked in tmask zeroed in front of Normalize (AdaptiveTimeMask), frames behind the clip's length 0.0 (collate_pad)
  audio   torchaudio.functional.add_noise, then F.layer_norm(x, x.shape, eps=1e-8), over the real samples; samples behind the length 0.0:
              Ex = sum x^2, En = sum n^2, scale = sqrt(Ex / En) * 10^(-snr_db / 20), y = x + scale * n
          scale is DEFINED as 0 where Ex == 0, En == 0 or no noise is given (the noise-free normalisation; the quotient has no value there).

Everything is evaluated in `dtype`: float64 is the yardstick, float32 is the reference's own arithmetic (what its dataloader workers compute)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F


def video_ref(clips: Sequence[torch.Tensor], params: torch.Tensor, Tpad: int, size: int, mean: float = 0.421, std: float = 0.165,
              tmask: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """clips: uint8 [T_b, Hs, Ws] each; params int32 [B, 5] = (top, left, h, w, flip) -> [B, Tpad, 1, size, size]."""
    out = torch.zeros(len(clips), Tpad, 1, size, size, dtype=dtype)
    for b, clip in enumerate(clips):
        top, left, h, w, flip = (int(v) for v in params[b])
        x = clip.to(dtype) / 255.0
        x = F.interpolate(x[:, None, top:top + h, left:left + w], size=(size, size), mode="bilinear", align_corners=False, antialias=False)
        if flip:
            x = x.flip(-1)
        if tmask is not None:
            x = x * (tmask[b, : len(clip)] == 0).to(dtype)[:, None, None, None]
        out[b, : len(clip)] = (x - mean) / std
    return out


def snr_scale(x: torch.Tensor, n: Optional[torch.Tensor], snr_db: float) -> torch.Tensor:
    """The factor of the noise, 0-d, in x's dtype."""
    zero = torch.zeros((), dtype=x.dtype)
    if n is None:
        return zero
    ex, en = x.pow(2).sum(), n.pow(2).sum()
    if ex == 0 or en == 0:
        return zero
    return torch.sqrt(ex / en) * torch.tensor(10.0, dtype=x.dtype) ** (-torch.tensor(float(snr_db), dtype=x.dtype) / 20.0)


def mixed_ref(wave: torch.Tensor, lengths: Sequence[int], noise: Optional[torch.Tensor] = None, nstart: Optional[Sequence[int]] = None,
              snr_db: Optional[Sequence[float]] = None, dtype: torch.dtype = torch.float64) -> list[torch.Tensor]:
    """The noisy waveforms y = x + scale * n, one [len] tensor per clip, in dtype (add_noise; int16 samples = v / 32768)."""
    ys = []
    for b, L in enumerate(int(v) for v in lengths):
        x = (wave[b, :L].to(torch.float32) / 32768.0 if wave.dtype == torch.int16 else wave[b, :L]).to(dtype)
        n = None if noise is None else noise[int(nstart[b]): int(nstart[b]) + L].to(dtype)
        ys.append(x if n is None else x + snr_scale(x, n, float(snr_db[b])) * n)
    return ys


def audio_ref(wave: torch.Tensor, lengths: Sequence[int], noise: Optional[torch.Tensor] = None, nstart: Optional[Sequence[int]] = None,
              snr_db: Optional[Sequence[float]] = None, eps: float = 1e-8, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """wave fp32 or int16 [B, Spad], noise fp32 [Nn] -> [B, Spad] in dtype: the layer norm of mixed_ref over each clip's real samples."""
    out = torch.zeros(wave.shape, dtype=dtype)
    for b, y in enumerate(mixed_ref(wave, lengths, noise, nstart, snr_db, dtype)):
        if len(y):
            out[b, : len(y)] = F.layer_norm(y, y.shape, eps=eps)
    return out


def synthetic_clips(lengths: Sequence[int], Hs: int, Ws: int, seed: int) -> list[torch.Tensor]:
    """Seeded uint8 clips: a smooth gradient plus noise, so a shifted window or a missed flip moves every pixel."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(Hs, dtype=torch.float32), torch.arange(Ws, dtype=torch.float32), indexing="ij")
    clips = []
    for i, T in enumerate(lengths):
        base = 40.0 + 1.3 * yy + 0.7 * xx + 5.0 * i
        clips.append((base[None] + torch.arange(T, dtype=torch.float32)[:, None, None] + 25.0 * torch.randn(T, Hs, Ws, generator=g)).clamp(0, 255).to(torch.uint8))
    return clips


def synthetic_wave(lengths: Sequence[int], Spad: int, seed: int, offset: float = 0.0, amplitude: float = 0.1) -> torch.Tensor:
    """fp32 [B, Spad]: seeded noise around `offset`, zero behind each length."""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(len(lengths), Spad)
    for b, L in enumerate(lengths):
        w[b, :L] = offset + amplitude * torch.randn(L, generator=g)
    return w
