"""fp64 host restatement of the LRW device input pipeline (augment.DeviceLRWPipeline; csrc/lrw_prep.hip), the yardstick of
tests/test_lrw_pipeline_cpu.py and tests/test_gpu_lrw_pipeline.py.  Reference: LRW/video/src/data.py:157-164 and augment.py:27-141.

For every stored clip s, uint8 [T, Hs, Ws], with crop parameters (top, left, h, w, flip):
  x_s      = flip(resize(window(x / 255))), resize = F.interpolate(mode="bilinear", align_corners=False, antialias=False) — the formula
             tests/test_gpu_misc.py::test_device_clip_pipeline restates svsr_clip_prep with
  TimeMask   runs (start_j, len_j) in order; fill_j = mean over all T * H * W values of the clip AS MASKED SO FAR; frames
             [start_j, start_j + len_j) become fill_j (0 with replace_with_zero); a run of length 0 changes nothing
  Normalize  y_s = (x_s - mean) / std
  CutMix     out[b, 0, t] = y_{frame_src[b, t]}[t]
`frame_fills` is the recurrence the kernel walks over a clip's T frame sums, here in Python floats (fp64)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F


def sampled_clips(frames_u8: torch.Tensor, params: torch.Tensor, H: int, W: int, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """uint8 [B, T, Hs, Ws], params int32 [B, 5] = (top, left, h, w, flip) -> x [B, T, H, W] in front of TimeMask and Normalize."""
    out = []
    for b in range(frames_u8.shape[0]):
        top, left, h, w, flip = (int(v) for v in params[b])
        x = frames_u8[b].to(dtype) / 255.0
        x = F.interpolate(x[:, None, top:top + h, left:left + w], size=(H, W), mode="bilinear", align_corners=False, antialias=False)[:, 0]
        out.append(x.flip(-1) if flip else x)
    return torch.stack(out)


def frame_fills(frame_sums: Sequence[float], runs: Sequence[tuple[int, int]], T: int, HW: int, replace_with_zero: bool = False) -> list[Optional[float]]:
    """Per frame of ONE clip: the value TimeMask leaves in it, or None where the frame is not masked.
        S = sum_t fs[t];  per run: m = S / (T HW), for t in the run: S += HW m - cur[t], cur[t] = HW m
    (m = 0 with replace_with_zero).  A later run overwrites an earlier one; a run of length 0 changes nothing."""
    cur = [float(v) for v in frame_sums]
    assert len(cur) == T
    S = 0.0
    for v in cur:
        S += v
    fills: list[Optional[float]] = [None] * T
    for start, length in runs:
        m = 0.0 if replace_with_zero else S / (T * HW)
        for t in range(int(start), int(start) + int(length)):
            S += HW * m - cur[t]
            cur[t] = HW * m
            fills[t] = m
    return fills


def clip_fills(x: torch.Tensor, runs, replace_with_zero: bool = False) -> list[list[Optional[float]]]:
    """x [B, T, H, W] (sampled_clips), runs [B][n_mask] (start, length) or None -> frame_fills of every clip."""
    B, T, H, W = x.shape
    if runs is None:
        return [[None] * T for _ in range(B)]
    return [frame_fills(x[s].sum(dim=(1, 2)).tolist(), [(int(a), int(n)) for a, n in runs[s]], T, H * W, replace_with_zero) for s in range(B)]


def pipeline_ref(frames_u8: torch.Tensor, params: torch.Tensor, frame_src: torch.Tensor, runs, H: int, W: int, mean: float = 0.421,
                 std: float = 0.165, replace_with_zero: bool = False):
    """-> (out fp64 [B, 1, T, H, W], masked bool [B, T]: whether out[b, 0, t] is a masked frame of its SOURCE clip)."""
    x = sampled_clips(frames_u8, params, H, W)
    fills = clip_fills(x, runs, replace_with_zero)
    B, T = frame_src.shape
    y = x.clone()
    for s in range(B):
        for t in range(T):
            if fills[s][t] is not None:
                y[s, t] = fills[s][t]
    y = (y - mean) / std
    out = torch.empty(B, 1, T, H, W, dtype=torch.float64)
    masked = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            s = int(frame_src[b, t])
            out[b, 0, t] = y[s, t]
            masked[b, t] = fills[s][t] is not None
    return out, masked


def synthetic_frames(B: int, T: int, Hs: int, Ws: int, seed: int) -> torch.Tensor:
    """Seeded uint8 clips [B, T, Hs, Ws]: a gradient that differs per clip and frame plus noise, so a wrong source clip, frame, window or
    flip moves every pixel, and the clips' means differ."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(Hs, dtype=torch.float32), torch.arange(Ws, dtype=torch.float32), indexing="ij")
    base = 30.0 + 2.0 * yy + 1.5 * xx
    clip = 17.0 * torch.arange(B, dtype=torch.float32)[:, None, None, None]
    frame = 3.0 * torch.arange(T, dtype=torch.float32)[None, :, None, None]
    return (base[None, None] + clip + frame + 20.0 * torch.randn(B, T, Hs, Ws, generator=g)).clamp(0, 255).to(torch.uint8)
