"""fp64 host restatement of the DC-TCN device input pipeline (augment.DeviceDCTCNPipeline; csrc/dctcn_prep.hip), the yardstick of
tests/test_dctcn_pipeline_cpu.py and tests/test_gpu_dctcn_pipeline.py.  Reference: LRW/video/src/data.py:70-139 (LRWDatasetForDCTCN) and
lightning.py:264-270.  Test infrastructure only: it loops per clip, as the reference does.

Per stored clip u8 [T, Hs, Ws] with word length wb, waveform [L] and the integers (shift, trunc, mask_off, mask_len, ashift, azero):
  videos     v = 2 u8 / 255 - 1
  mask       v[mask_off : mask_off + mask_len] = mean of the whole clip v (m = 2 S / (255 T Hs Ws) - 1, S the integer sum of the clip)
  trim       v = roll(v, shift) in time (rolled[t] = v[(t - shift) mod T]); v[trunc:] = 0
             audio = roll(audio, ashift); audio[azero:] = 0
             word mask [(T - wb) // 2, + wb) and the all-ones attention mask: rolled by shift, zeroed from trunc on
  transform  x = v / 255 (the second division), window (top, left, h, w) resized to H x W (bilinear, align_corners=False, no antialias),
             flipped, y = (x - mean) / std
  mixup      out[b] = lerp(y[b], y[b - 1], lam) — Normalize is affine, so mixing behind it is mixing in front of it
`mask_trim` is the part the golden (tests/golden/dctcn_data.npz) records from the reference's own _mask_frames + _trim_frames."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def clip_sums(frames_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [B, T, Hs, Ws] -> int64 [B, T]: the exact sum of every stored frame."""
    return frames_u8.to(torch.int64).sum(dim=(2, 3))


def mask_trim(clip_u8: torch.Tensor, wave: torch.Tensor, wb: int, shift: int, trunc: int, mask_off: int, mask_len: int, ashift: int, azero: int):
    """One clip u8 [T, Hs, Ws], waveform [L] -> (videos fp64 [T, Hs, Ws] in [-1, 1], audio [L], word mask int64 [T], attention mask int64 [T],
    kind [T]: 'z' trimmed, 'm' masked, or the index of the stored frame).  `trunc` and `azero` slice as Python does."""
    T = clip_u8.shape[0]
    v = 2.0 * clip_u8.to(torch.float64) / 255.0 - 1.0
    kind: list = list(range(T))
    S = int(clip_u8.to(torch.int64).sum())
    m = 2.0 * S / (255.0 * clip_u8.numel()) - 1.0
    for t in range(mask_off, mask_off + mask_len):
        v[t] = m
        kind[t] = "m"
    v = torch.stack([v[(t - shift) % T] for t in range(T)])
    kind = [kind[(t - shift) % T] for t in range(T)]
    word = torch.zeros(T, dtype=torch.int64)
    word[(T - wb) // 2: (T - wb) // 2 + wb] = 1
    word = torch.stack([word[(t - shift) % T] for t in range(T)])
    att = torch.ones(T, dtype=torch.int64)
    for t in range(trunc, T):
        v[t] = 0.0
        kind[t] = "z"
        word[t] = 0
        att[t] = 0
    audio = torch.roll(wave, ashift, 0)          # rolled[i] = wave[(i - ashift) mod L]
    audio[azero:] = 0
    return v, audio, word, att, kind


def transform(v: torch.Tensor, window, H: int, W: int, mean: float = 0.421, std: float = 0.165) -> torch.Tensor:
    """v fp64 [T, Hs, Ws] (mask_trim) + (top, left, h, w, flip) -> Normalize(flip(resize(window(v / 255)))) fp64 [T, H, W]."""
    top, left, h, w, flip = (int(a) for a in window)
    x = v / 255.0
    x = F.interpolate(x[:, None, top:top + h, left:left + w], size=(H, W), mode="bilinear", align_corners=False, antialias=False)[:, 0]
    if flip:
        x = x.flip(-1)
    return (x - mean) / std


def pipeline_ref(frames_u8: torch.Tensor, waves: torch.Tensor, boundaries, table: torch.Tensor, audio: torch.Tensor, H: int, W: int, lam: float = 0.0,
                 mean: float = 0.421, std: float = 0.165) -> dict:
    """frames uint8 [B, T, Hs, Ws], waves [B, L], table int [B, 9] = (top, left, h, w, flip, shift, trunc, mask_off, mask_len), audio int [B, 2]
    = (ashift, azero) -> the pipeline's dict in fp64 / int64 (labels left out)."""
    B = frames_u8.shape[0]
    ys, auds, words, atts = [], [], [], []
    for b in range(B):
        top, left, h, w, flip, shift, trunc, moff, mlen = (int(a) for a in table[b])
        v, a, word, att, _ = mask_trim(frames_u8[b], waves[b].to(torch.float64), int(boundaries[b]), shift, trunc, moff, mlen, int(audio[b][0]), int(audio[b][1]))
        ys.append(transform(v, (top, left, h, w, flip), H, W, mean, std))
        auds.append(a)
        words.append(word)
        atts.append(att)
    y = torch.stack(ys)
    if lam:
        y = torch.stack([y[b] + lam * (y[(b - 1) % B] - y[b]) for b in range(B)])
    return {"videos": y.unsqueeze(1), "audios": torch.stack(auds), "word_mask": torch.stack(words), "attention_mask": torch.stack(atts)}
