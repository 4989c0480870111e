"""Sequential-frame CutMix of the reference (LRW/video/src/augment.py:11-118) with a host-side plan and one device gather.

The reference loops over the batch in Python and splices frames IN PLACE, so a later sample can copy frames that an
earlier iteration already replaced.  Here the same random decisions are drawn on the host in the same order from torch's
CPU generator (so a seeded run reproduces the reference bit for bit), the in-place chain is resolved on the host into a
[B, T] source map (which original sample each frame finally comes from), and the clip / token / mask tensors are produced
by a single gather on the device — no per-sample launches, no device->host sync.

Quirks kept on purpose: the audio tokens are spliced with the FRAME indices (not frame*alignment) exactly as
augment.py:104-109 does; labels become [B, num_labels] probabilities and word masks become float.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F


class CutMixPlan:
    def __init__(self, frame_src: torch.Tensor, token_src: torch.Tensor, target_ids: torch.Tensor, mix: torch.Tensor):
        self.frame_src = frame_src      # int64 [B, T]   original sample whose frame t ends up in sample b
        self.token_src = token_src      # int64 [B, Ta]  same for the audio-token axis
        self.target_ids = target_ids    # int64 [B]
        self.mix = mix                  # float32 [B]    effective mix rate (0 where no cut happened)


def make_plan(batch_size: int, frames: int, token_steps: int, generator: Optional[torch.Generator] = None) -> CutMixPlan:
    """Draws exactly the random numbers CutMix.forward / mask_video draw, in the same order (augment.py:34-36,86,97-99)."""
    target_ids = torch.randint(0, batch_size, (batch_size,), generator=generator)
    target_rates = torch.rand(batch_size, generator=generator)
    frame_src = torch.arange(batch_size).unsqueeze(1).repeat(1, frames)
    token_src = torch.arange(batch_size).unsqueeze(1).repeat(1, token_steps)
    mix = torch.zeros(batch_size)
    for i in range(batch_size):
        rate = target_rates[i].item()
        cut_out_flag = torch.randint(0, 2, (1,), generator=generator)[0].item()
        if cut_out_flag != 1:
            continue
        cut = int(frames * rate)
        if cut <= 0:
            continue
        start = torch.randint(0, frames - cut, (1,), generator=generator).item()
        t = int(target_ids[i])
        # in-place semantics: the target's CURRENT frames (already spliced if t < i, or i itself) are copied
        frame_src[i, start : start + cut] = frame_src[t, start : start + cut].clone()
        hi = min(start + cut, token_steps)
        if start < token_steps:
            token_src[i, start:hi] = token_src[t, start:hi].clone()
        mix[i] = rate
    return CutMixPlan(frame_src, token_src, target_ids, mix)


class CutMix(torch.nn.Module):
    """Drop-in for the reference's ``CutMix(num_labels, wav2vec=None)``.  wav2vec: an audio_codec.VqWav2VecCodec; float waveforms in the
    `audios` slot are then tokenised first (augment.py:38-40) and the tokens spliced as pre-tokenised audio is.  The codec is BORROWED: it
    is kept in a plain tuple, not as a sub-module, so this module's ``state_dict()`` and ``.to()`` leave it alone — whoever owns it (the
    model it is attached to, or the caller of a stand-alone CutMix) moves it to the device and lists its buffers, once."""

    def __init__(self, num_labels: int, wav2vec=None) -> None:
        super().__init__()
        self.num_labels = num_labels
        self.set_codec(wav2vec)
        self.generator: Optional[torch.Generator] = None     # None = torch's global CPU generator, as the reference uses

    def set_codec(self, wav2vec) -> None:
        """None, or the vq tokeniser (class docstring).  As attach_audio_codec: TypeError for what is no codec, ValueError for the wrong kind."""
        from .audio_codec import VqWav2VecCodec, Wav2Vec2Codec

        if isinstance(wav2vec, Wav2Vec2Codec):
            raise ValueError("CutMix belongs to the word-level models, whose codec is 'vq': it tokenises with a VqWav2VecCodec, not the wav2vec2 tokeniser")
        if wav2vec is not None and not isinstance(wav2vec, VqWav2VecCodec):
            raise TypeError("CutMix(wav2vec=...) takes a syncvsr_amd.audio_codec.VqWav2VecCodec or None")
        self._codec = (wav2vec,)

    @property
    def wav2vec(self):
        return self._codec[0]

    def forward(self, videos: torch.Tensor, audios: torch.Tensor, labels: torch.Tensor, word_mask: torch.Tensor):
        B, _, T = videos.shape[:3]
        if self.wav2vec is not None and audios.is_floating_point():
            audios = self.wav2vec(audios)
        plan = make_plan(B, T, audios.shape[1], self.generator)
        dev = videos.device
        fsrc = plan.frame_src.to(dev, non_blocking=True)
        tidx = torch.arange(T, device=dev).unsqueeze(0).expand(B, T)
        mixed_videos = videos[fsrc, :, tidx].permute(0, 2, 1, 3, 4).contiguous()          # [B, 1, T, H, W]
        return (mixed_videos, *mix_small_tensors(plan, audios, labels, word_mask, self.num_labels, dev))


def mix_small_tensors(plan: CutMixPlan, audios: torch.Tensor, labels: torch.Tensor, word_mask: torch.Tensor, num_labels: int, dev):
    """What CutMix mixes besides the clips, for a resolved plan: audio tokens gathered by `token_src`, labels as [B, num_labels]
    probabilities, float word masks (augment.py:104-116).  Shared by CutMix.forward and DeviceLRWPipeline."""
    B = audios.shape[0]
    tsrc = plan.token_src.to(dev, non_blocking=True)
    aidx = torch.arange(audios.shape[1], device=dev).unsqueeze(0).expand(B, -1)
    mixed_audios = audios[tsrc, aidx].contiguous()
    mix = plan.mix.to(dev)
    tgt = plan.target_ids.to(dev)
    one_hot = F.one_hot(labels, num_labels)
    # integer one-hots promoted by the float mix rate, as in augment.py:111-113; untouched samples stay integer there,
    # the concatenation makes the batch float — here everything is float32 from the start
    mixed_labels = (1.0 - mix).unsqueeze(1) * one_hot.float() + mix.unsqueeze(1) * one_hot[tgt].float()
    wm = word_mask.float()
    mixed_word_mask = (1.0 - mix).view(B, *([1] * (wm.dim() - 1))) * wm + mix.view(B, *([1] * (wm.dim() - 1))) * wm[tgt]
    return mixed_audios, mixed_labels, mixed_word_mask


def draw_time_runs(n_frames: int, max_run, n_mask: int) -> list[tuple[int, int]]:
    """(start, length) of every masked run, drawn from Python's `random` with the two calls per mask the reference makes
    (LRW/video/src/augment.py:130-132): the run length first, then where it starts."""
    import random

    runs = []
    for _ in range(n_mask):
        length = random.randint(0, min(max_run, n_frames))
        runs.append((random.randint(0, n_frames - length), length))
    return runs


class TimeMask(torch.nn.Module):
    """The reference's TimeMask (LRW/video/src/augment.py:120-141; `train.use_timemask`, T = 0.6 * 25 frames, one mask):
    random runs of up to T frames of one clip [T, ...] are replaced by the clip's mean (or zero).  `draw_time_runs` makes the
    random decisions in the reference's order, so a seeded run reproduces it; every run is then one fill on the clip's device
    (CPU or HIP; no host sync: the mean stays a 0-d tensor)."""

    def __init__(self, T: float = 6400, n_mask: int = 2, replace_with_zero: bool = False):
        super().__init__()
        self.T, self.n_mask, self.replace_with_zero = T, n_mask, replace_with_zero

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = x.clone()
        for start, length in draw_time_runs(out.size(0), self.T, self.n_mask):
            # the mean is that of the clip as masked so far: a later run sees the earlier fills, as in the reference
            out[start : start + length] = 0 if self.replace_with_zero else out.mean()
        return out


class DeviceClipPipeline:
    """The reference's per-clip transform chain (LRW/video/src/data.py:150,157-171) on the device in one kernel: stored uint8 mouth
    crops [B, T, Hs, Ws] -> fp32 [B, 1, T, H, W] = Normalize(RandomResizedCrop | CenterCrop(flip(x / 255))) — the host only draws
    five integers per clip, and the uint8 clips cross PCIe at a quarter of the fp32 size.

    train=True:  RandomHorizontalFlip(0.5) and, with use_rrc, RandomResizedCrop(size, scale=(0.6, 1.0), ratio=(3/4, 4/3)) with
                 torchvision's rejection sampling (10 tries, then the central fallback); without use_rrc the frame passes through
                 at its stored size (nn.Identity, data.py:160).
    train=False: CenterCrop(size) (or Resize with use_val_resize).
    The draws come from a numpy generator (torchvision, whose RNG order the reference follows, is not available to pin them);
    the resize is bilinear without antialias."""

    def __init__(self, size: int, train: bool, use_rrc: bool = True, use_val_resize: bool = False, mean: float = 0.421,
                 std: float = 0.165, seed: int = 0):
        import numpy as np

        self.size, self.train, self.use_rrc, self.use_val_resize, self.mean, self.std = int(size), train, use_rrc, use_val_resize, mean, std
        self.rng = np.random.default_rng(seed)

    def draw(self, B: int, Hs: int, Ws: int) -> torch.Tensor:
        """int32 [B, 5] = (top, left, h, w, flip) per clip."""
        import math

        import numpy as np

        out = np.zeros((B, 5), dtype=np.int32)
        for b in range(B):
            if self.train and self.use_rrc:
                area = Hs * Ws
                for _ in range(10):
                    target = area * self.rng.uniform(0.6, 1.0)
                    ratio = math.exp(self.rng.uniform(math.log(3 / 4), math.log(4 / 3)))
                    w, h = int(round(math.sqrt(target * ratio))), int(round(math.sqrt(target / ratio)))
                    if 0 < w <= Ws and 0 < h <= Hs:
                        out[b, :4] = (self.rng.integers(0, Hs - h + 1), self.rng.integers(0, Ws - w + 1), h, w)
                        break
                else:       # torchvision's fallback (RandomResizedCrop.get_params): the central crop with the nearest admissible ratio
                    in_ratio = Ws / Hs
                    if in_ratio < 3 / 4:
                        w, h = Ws, int(round(Ws / (3 / 4)))
                    elif in_ratio > 4 / 3:
                        h = Hs
                        w = int(round(h * (4 / 3)))
                    else:
                        w, h = Ws, Hs
                    out[b, :4] = ((Hs - h) // 2, (Ws - w) // 2, h, w)
            elif (self.train and not self.use_rrc) or (not self.train and self.use_val_resize):
                out[b, :4] = (0, 0, Hs, Ws)
            else:
                out[b, :4] = ((Hs - self.size) // 2, (Ws - self.size) // 2, self.size, self.size)
            out[b, 4] = int(self.train and self.rng.random() < 0.5)
        return torch.from_numpy(out)

    def __call__(self, frames_u8: torch.Tensor, params: Optional[torch.Tensor] = None) -> torch.Tensor:
        from . import ops

        B, T, Hs, Ws = frames_u8.shape
        if params is None:
            params = self.draw(B, Hs, Ws)
        if params.device.type == "cpu":         # (device-resident windows are clamped into the frame by the kernel instead)
            top, left, h, w = (params[:, i] for i in range(4))
            if bool(((top < 0) | (left < 0) | (h < 1) | (w < 1) | (top + h > Hs) | (left + w > Ws)).any()):
                raise ValueError("crop window outside the stored frame")
        identity = self.train and not self.use_rrc          # nn.Identity: output size = stored size
        H, W = (Hs, Ws) if identity else (self.size, self.size)
        return ops.clip_prep(frames_u8.contiguous(), params.to(frames_u8.device, non_blocking=True), H, W, self.mean, self.std)


class DeviceLRWPipeline:
    """The word-level training inputs on the device in two launches per batch: what the reference spreads over its dataset transform
    (LRW/video/src/data.py:157-164: x / 255 -> RandomHorizontalFlip -> RandomResizedCrop | Identity -> Grayscale -> TimeMask -> Normalize,
    per clip in the loader workers) and its sequential CutMix (augment.py:27-118, per batch in the training step), from the stored uint8
    crops [B, T, Hs, Ws] and a few host-drawn integers.  svsr_lrw_clip_sums writes the per-frame sums that TimeMask's clip means are made
    of; svsr_lrw_clip_mix writes the batch, every frame sampled from the clip that CutMix's in-place chain finally takes it from, with that
    clip's crop, flip and mask (csrc/lrw_prep.hip).  No per-clip launches and no second pass over the fp32 clips.

    `__call__(frames_u8, audios, labels, word_mask)` returns `(videos, audios, labels, word_mask)` as CutMix.forward does: with use_cutmix
    the audio tokens are spliced, the labels are [B, num_labels] probabilities and the word mask is float; without it the three pass
    through.  The batch is ALREADY mixed: hand it to `model(*batch)` or `engine.TrainStep.step(*batch)`, not to `model.training_step`,
    which applies CutMix itself when `train.use_cutmix` is on.

    Draws, all on the host, in this order per batch (`plan`):
      1. `DeviceClipPipeline.draw`: window and flip of every clip, from the numpy generator seeded with `seed`;
      2. `draw_time_runs` per clip in batch order, from Python's `random` (two calls per mask, as the reference's dataset makes them);
      3. `make_plan`, from `self.generator`, or torch's global CPU generator when that is None (as CutMix).
    A stage that is off draws nothing.  train=False, or use_timemask and use_cutmix both off, is `DeviceClipPipeline.__call__` — one
    svsr_clip_prep launch; the sums launch is also left out when no clip has a run of positive length, and with replace_with_zero.

    codec: a VqWav2VecCodec; float waveforms in the `audios` slot are then tokenised first, as `CutMix(wav2vec=)` does.  It is BORROWED
    (kept in a plain tuple): whoever owns it moves it to the device."""

    def __init__(self, size: int, num_labels: int, train: bool = True, use_rrc: bool = True, use_timemask: bool = True, use_cutmix: bool = True,
                 timemask_T: float = 0.6 * 25, n_mask: int = 1, replace_with_zero: bool = False, use_val_resize: bool = False,
                 mean: float = 0.421, std: float = 0.165, seed: int = 0, codec=None):
        from .audio_codec import VqWav2VecCodec, Wav2Vec2Codec

        if isinstance(codec, Wav2Vec2Codec):
            raise ValueError("DeviceLRWPipeline belongs to the word-level models, whose codec is 'vq': it tokenises with a VqWav2VecCodec, not the wav2vec2 tokeniser")
        if codec is not None and not isinstance(codec, VqWav2VecCodec):
            raise TypeError("DeviceLRWPipeline(codec=...) takes a syncvsr_amd.audio_codec.VqWav2VecCodec or None")
        if int(n_mask) < 0:
            raise ValueError("n_mask must be >= 0")
        self._codec = (codec,)
        self.clips = DeviceClipPipeline(size, train, use_rrc=use_rrc, use_val_resize=use_val_resize, mean=mean, std=std, seed=seed)
        self.size, self.num_labels, self.train = int(size), int(num_labels), bool(train)
        self.use_timemask, self.use_cutmix = bool(train and use_timemask and int(n_mask) > 0), bool(train and use_cutmix)
        # (an integral float bound, the reference's 0.6 * 25, draws what the integer draws; `random` refuses floats from Python 3.12 on)
        self.timemask_T = int(timemask_T) if float(timemask_T).is_integer() else timemask_T
        self.n_mask, self.replace_with_zero = int(n_mask), bool(replace_with_zero)
        self.mean, self.std = float(mean), float(std)
        self.generator: Optional[torch.Generator] = None     # None = torch's global CPU generator, as CutMix

    @property
    def codec(self):
        return self._codec[0]

    def plan(self, B: int, T: int, Hs: int, Ws: int, token_steps: int) -> dict:
        """Every host decision of one batch, drawn in the documented order: {"params": int32 [B, 5] = (top, left, h, w, flip), "runs": int32
        [B, n_mask, 2] = (start, length) per clip as drawn (None without the time mask), "cutmix": the CutMixPlan (None without CutMix)}."""
        params = self.clips.draw(B, Hs, Ws)
        runs = None
        if self.use_timemask:
            runs = torch.tensor([draw_time_runs(T, self.timemask_T, self.n_mask) for _ in range(B)], dtype=torch.int32).reshape(B, self.n_mask, 2)
        cut = make_plan(B, T, token_steps, self.generator) if self.use_cutmix else None
        return {"params": params, "runs": runs, "cutmix": cut}

    def __call__(self, frames_u8: torch.Tensor, audios: torch.Tensor, labels: torch.Tensor, word_mask: torch.Tensor, plan: Optional[dict] = None):
        from . import ops

        if frames_u8.dim() != 4 or frames_u8.dtype != torch.uint8:
            raise ValueError("frames_u8 must be uint8 [B, T, Hs, Ws]")
        B, T, Hs, Ws = frames_u8.shape
        if self.codec is not None and audios.is_floating_point():
            audios = self.codec(audios)
        if plan is None:
            plan = self.plan(B, T, Hs, Ws, audios.shape[1])
        params, runs, cut = plan["params"], plan.get("runs"), plan.get("cutmix")
        if not (self.use_timemask or self.use_cutmix) or (runs is None and cut is None):
            return self.clips(frames_u8, params), audios, labels, word_mask
        if T > ops.LRW_CLIP_MAX_FRAMES:
            raise ValueError(f"clips of {T} frames: the LRW clip kernels take at most {ops.LRW_CLIP_MAX_FRAMES}")
        if params.dtype != torch.int32 or params.shape != (B, 5):
            raise ValueError(f"params must be int32 [B, 5] = {(B, 5)}")
        top, left, h, w = (params[:, i] for i in range(4))
        if bool(((top < 0) | (left < 0) | (h < 1) | (w < 1) | (top + h > Hs) | (left + w > Ws)).any()):
            raise ValueError("crop window outside the stored frame")
        if cut is not None and (cut.frame_src.shape != (B, T) or int(cut.frame_src.min()) < 0 or int(cut.frame_src.max()) >= B):
            raise ValueError("frame_src must be [B, T] with entries in [0, B)")
        if runs is not None:
            if runs.dim() != 3 or runs.shape[0] != B or runs.shape[2] != 2:
                raise ValueError("runs must be [B, n_mask, 2]")
            start, length = runs[..., 0].long(), runs[..., 1].long()
            if bool(((start < 0) | (length < 0) | (start + length > T)).any()):
                raise ValueError("time-mask run outside the clip")
            if not bool((length > 0).any()):
                runs = None                              # nothing is masked: no sums, no run table
        dev = frames_u8.device
        identity = self.clips.train and not self.clips.use_rrc          # nn.Identity: output size = stored size
        H, W = (Hs, Ws) if identity else (self.size, self.size)
        fsrc = torch.arange(B, dtype=torch.int32).unsqueeze(1).repeat(1, T) if cut is None else cut.frame_src.to(torch.int32)
        # every drawn integer in ONE small upload: params | frame_src | runs
        parts = [params.reshape(-1), fsrc.reshape(-1)] + ([runs.to(torch.int32).reshape(-1)] if runs is not None else [])
        meta = torch.cat(parts).to(dev, non_blocking=True)
        par_d, fsrc_d = meta[: 5 * B].view(B, 5), meta[5 * B: 5 * B + B * T].view(B, T)
        runs_d = meta[5 * B + B * T:].view(B, -1, 2) if runs is not None else None
        frames_u8 = frames_u8.contiguous()
        sums = ops.lrw_clip_sums(frames_u8, par_d, H, W) if runs_d is not None and not self.replace_with_zero else None
        videos = ops.lrw_clip_mix(frames_u8, par_d, fsrc_d, H, W, runs_d, sums, self.replace_with_zero, self.mean, self.std)
        if cut is None:
            return videos, audios, labels, word_mask
        return (videos, *mix_small_tensors(cut, audios, labels, word_mask, self.num_labels, dev))


class DeviceDCTCNPipeline:
    """The DC-TCN training inputs on the device in at most three launches per batch: what the reference's LRWDatasetForDCTCN does per clip
    in the loader workers (LRW/video/src/data.py:70-139) and the clip mixup of its module (lightning.py:264-270), from the stored uint8
    crops [B, T, Hs, Ws], the fp32 waveforms [B, L] and a few host-drawn integers per clip (csrc/dctcn_prep.hip):
      scaling        videos = 2 x / 255 - 1, and the transform chain divides by 255 a SECOND time in front of Normalize(mean, std) — a quirk a
                     trained checkpoint depends on: every input lies in about [-2.575, -2.528];
      _mask_frames   a run of randint(max_time_masks) frames becomes the mean of the whole stored clip;
      _trim_frames   clip, waveform, word mask and attention mask are rolled in time by a drawn shift and zeroed behind a drawn length;
      transform      RandomHorizontalFlip, RandomResizedCrop | Identity (train), CenterCrop | Resize (eval): DeviceClipPipeline.draw;
      mixup          torch.lerp(videos, videos.roll(1, 0), lam) with the caller's lam (draw_lam).
    svsr_dctcn_clip_sums writes the stored frames' integer sums (only when some clip masks a run of positive length), svsr_dctcn_clip_mix
    the batch, svsr_dctcn_wave_trim the waveforms.  train=False is the reference's validation=True: no mask, no trim, no flip, and the
    waveforms pass through — one launch.

    `__call__(frames_u8, waves, labels, boundaries, lam)` returns the keyword arguments of DCTCNLightningModule.forward: videos fp32
    [B, 1, T, H, W], audios fp32 [B, L], labels, word_mask and attention_mask int64 [B, T].  The videos are ALREADY mixed: hand the dict
    to `loss_and_backend_grads(**batch, train_stats=True, lam=lam, videos_mixed=True)` with the same lam.

    Draws, all on the host, per batch (`plan`): window and flip of every clip from the numpy generator seeded with `seed`
    (DeviceClipPipeline.draw), then per clip in batch order from numpy's GLOBAL np.random, as the reference's dataset draws them:
    length = randint(max_time_masks), offset = randint(T - length), truncated = randint(boundary, T),
    off2 = randint(truncated - boundary + 1); shift = off2 - (T - boundary) // 2."""

    def __init__(self, size: int, max_time_masks: int = 15, train: bool = True, use_rrc: bool = False, use_val_resize: bool = False,
                 mean: float = 0.421, std: float = 0.165, seed: int = 0):
        if train and int(max_time_masks) < 1:
            raise ValueError("max_time_masks must be >= 1 (the reference draws randint(max_time_masks))")
        self.clips = DeviceClipPipeline(size, train, use_rrc=use_rrc, use_val_resize=use_val_resize, mean=mean, std=std, seed=seed)
        self.size, self.max_time_masks, self.train = int(size), int(max_time_masks), bool(train)
        self.mean, self.std = float(mean), float(std)

    @classmethod
    def from_config(cls, config, train: bool, seed: int = 0) -> "DeviceDCTCNPipeline":
        """From a dc-tcn configuration: data.input_size, data.max_time_masks (15 when absent), train.use_rrc and train.use_val_resize
        (absent: off, as in the shipped dc-tcn-base.yaml).  train.use_timemask, the transform-level TimeMask on top of _mask_frames, is
        not implemented."""
        data, tr = config.get("data", {}), config.get("train", {})
        if tr.get("use_timemask", False):
            raise NotImplementedError("train.use_timemask: the transform-level TimeMask on top of the dataset's _mask_frames is not part of "
                                      "DeviceDCTCNPipeline")
        return cls(int(data["input_size"]), max_time_masks=int(data.get("max_time_masks", 15)), train=train, use_rrc=bool(tr.get("use_rrc", False)),
                   use_val_resize=bool(tr.get("use_val_resize", False)), seed=seed)

    @staticmethod
    def draw_lam(alpha: float) -> float:
        """The module's mixup weight (lightning.py:266), one draw per batch from numpy's global np.random: in [0, 0.5]."""
        import numpy as np

        return float(0.5 - abs(0.5 - np.random.beta(alpha, alpha)))

    def plan(self, B: int, T: int, Hs: int, Ws: int, L: int, boundaries) -> dict:
        """Every host decision of one batch: {"params": int32 [B, 5] = (top, left, h, w, flip), "time": int32 [B, 4] = (shift, trunc,
        mask_off, mask_len), "audio": int32 [B, 2] = (ashift, azero)}.  boundaries: the word length of every clip in frames.  Raises
        ValueError where the reference's own draw would (boundary >= T, T - length <= 0), at the draw that fails."""
        import numpy as np

        wbs = [int(v) for v in (boundaries.tolist() if hasattr(boundaries, "tolist") else boundaries)]
        if len(wbs) != B:
            raise ValueError(f"boundaries must hold one word length per clip: {B}")
        params = self.clips.draw(B, Hs, Ws)
        time, audio = np.zeros((B, 4), dtype=np.int32), np.zeros((B, 2), dtype=np.int32)
        time[:, 1], audio[:, 1] = T, L
        if self.train:
            stride = T / L                                          # audio_stride of the reference: a Python float
            for b, wb in enumerate(wbs):
                length = int(np.random.randint(self.max_time_masks))
                if T - length <= 0:
                    raise ValueError(f"clip {b}: a mask run of {length} frames does not fit a clip of {T} (the reference's randint(T - length) raises)")
                offset = int(np.random.randint(T - length))
                if not 0 <= wb < T:
                    raise ValueError(f"clip {b}: word boundary {wb} must lie in [0, {T}) (the reference's randint(boundary, T) raises)")
                truncated = int(np.random.randint(wb, T))
                off2 = int(np.random.randint(truncated - wb + 1))
                shift = int(off2 - (T - wb) // 2)
                time[b] = (shift, truncated, offset, length)
                audio[b] = (int(shift / stride), int(truncated / stride))
        return {"params": params, "time": torch.from_numpy(time), "audio": torch.from_numpy(audio)}

    def __call__(self, frames_u8: torch.Tensor, waves: torch.Tensor, labels: torch.Tensor, boundaries, lam: float = 0.0,
                 plan: Optional[dict] = None) -> dict:
        import numpy as np

        from . import ops

        if frames_u8.dim() != 4 or frames_u8.dtype != torch.uint8:
            raise ValueError("frames_u8 must be uint8 [B, T, Hs, Ws]")
        B, T, Hs, Ws = frames_u8.shape
        if not torch.is_tensor(waves) or not waves.is_floating_point():
            raise ValueError("waves must be fp32 waveforms [B, L]: pre-tokenised audio cannot be trimmed here, because a waveform shifted by "
                             "int(shift / (T / L)) samples is not a token row shifted by whole tokens — tokenise after the trim (attach_audio_codec)")
        if waves.dtype != torch.float32 or waves.dim() != 2 or waves.shape[0] != B:
            raise ValueError(f"waves must be fp32 [B, L] with B = {B}")
        L = waves.shape[1]
        if T > ops.DCTCN_CLIP_MAX_FRAMES:
            raise ValueError(f"clips of {T} frames: the DC-TCN clip kernels take at most {ops.DCTCN_CLIP_MAX_FRAMES}")
        lam = float(lam)
        if not 0.0 <= lam <= 0.5:
            raise ValueError("lam must lie in [0, 0.5] (draw_lam)")
        wbs = np.asarray(boundaries.tolist() if hasattr(boundaries, "tolist") else boundaries, dtype=np.int64).reshape(-1)
        if wbs.shape[0] != B or bool(((wbs < 0) | (wbs > T)).any()):
            raise ValueError(f"boundaries must hold one word length in [0, {T}] per clip")
        if plan is None:
            plan = self.plan(B, T, Hs, Ws, L, wbs)
        params, time, audio = plan["params"], plan["time"], plan["audio"]
        if params.dtype != torch.int32 or params.shape != (B, 5) or time.dtype != torch.int32 or time.shape != (B, 4) or \
                audio.dtype != torch.int32 or audio.shape != (B, 2):
            raise ValueError("plan: params, time and audio must be int32 [B, 5], [B, 4] and [B, 2]")
        top, left, h, w = (params[:, i] for i in range(4))
        if bool(((top < 0) | (left < 0) | (h < 1) | (w < 1) | (top + h > Hs) | (left + w > Ws)).any()):
            raise ValueError("crop window outside the stored frame")
        shift, trunc, moff, mlen = (time[:, i].numpy().astype(np.int64) for i in range(4))
        if bool(((trunc < 0) | (trunc > T)).any()):
            raise ValueError("trim length outside the clip")
        if bool(((moff < 0) | (mlen < 0) | (moff + mlen > T)).any()):
            raise ValueError("frame-mask run outside the clip")
        trimmed = bool((shift != 0).any() or (trunc != T).any() or (audio[:, 0] != 0).any() or (audio[:, 1] < L).any())
        # the two [B, T] masks, on the host: the untrimmed word mask [(T - wb) // 2, + wb) rolled by shift, both zeroed from trunc on
        t = np.arange(T, dtype=np.int64)[None, :]
        ts = (t - shift[:, None]) % T
        start = ((T - wbs) // 2)[:, None]
        alive = t < trunc[:, None]
        word = (alive & (ts >= start) & (ts < start + wbs[:, None])).astype(np.int32)
        # every drawn integer and both masks in ONE upload: table [B, 9] | audio [B, 2] | word mask [B, T] | attention mask [B, T]
        table = torch.cat([params, time], dim=1)
        meta = torch.cat([table.reshape(-1), audio.reshape(-1), torch.from_numpy(word).reshape(-1), torch.from_numpy(alive.astype(np.int32)).reshape(-1)])
        dev = frames_u8.device
        meta = meta.to(dev, non_blocking=True)
        table_d, audio_d = meta[: 9 * B].view(B, 9), meta[9 * B: 11 * B].view(B, 2)
        masks = meta[11 * B:].view(2, B, T).long()
        identity = self.clips.train and not self.clips.use_rrc          # nn.Identity: output size = stored size
        H, W = (Hs, Ws) if identity else (self.size, self.size)
        frames_u8 = frames_u8.contiguous()
        sums = ops.dctcn_clip_sums(frames_u8) if bool((mlen > 0).any()) else None
        videos = ops.dctcn_clip_mix(frames_u8, table_d, H, W, sums, lam, self.mean, self.std)
        audios = ops.dctcn_wave_trim(waves.contiguous(), audio_d) if trimmed else waves
        return {"videos": videos, "audios": audios, "labels": labels, "word_mask": masks[0], "attention_mask": masks[1]}
