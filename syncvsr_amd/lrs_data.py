"""Length-bucketed data-parallel batching for the LRS (sentence-level) model — BASELINE.json configs[4].

The reference pads every batch to its longest clip (`collate_pad`, LRS/video/datamodule/data_module.py:12-43) and leaves the
place for a batch sampler commented out (`# batch_sampler=sampler`, data_module.py:66-74): with a plain DataLoader the padded
length differs from rank to rank, so under DistributedDataParallel every step waits for the rank that drew the longest clip,
and every new padded length is a new set of kernel shapes.  `LengthBucketBatchSampler` is the sampler for that hook:

  * clips are grouped into buckets of similar length (bucket = ceil(length / width) * width frames);
  * one training step takes `world_size * batch_size` clips from ONE bucket and deals them to the ranks, so every rank pads
    to the SAME number of frames in the same step (no stragglers) and only len(buckets) different shapes ever occur;
  * the order of steps and the clips inside a bucket are shuffled from (seed, epoch) identically on every rank — no
    communication — and every rank sees the same number of steps (a requirement of the gradient all-reduce).

`collate_pad` reproduces the reference's batch layout and can pad the frame axis to the bucket's bound instead of the longest
clip in the batch.  Sampler and `collate_pad` are pure host code (numpy / torch CPU).

`collate_packed` + `DeviceLRSPipeline` are the other front door: the dataset hands over what it STORES (uint8 mouth crops, raw waveforms)
and the reference's per-sample transforms (LRS/video/datamodule/transforms.py) and the padding run on the device, in three launches per batch.
"""
from __future__ import annotations

from typing import Iterator, Optional, Sequence

import numpy as np
import torch
import torch.utils.data


class LengthBucketBatchSampler:
    """`batch_sampler` for `torch.utils.data.DataLoader`: yields this rank's list of dataset indices per step.

    lengths     clip lengths in frames, one per dataset item (e.g. the reference's datamodule/video_length.npy, 12..155)
    batch_size  clips per rank and step (`batch_size: 16`, LRS/video/config/lrs3.yaml:1)
    width       bucket width in frames; the padded length of a step is a multiple of it
    max_frames  clips longer than this are treated as max_frames long (the dataset crops them, av_dataset.py:72-80)
    drop_last   drop the clips of a bucket that do not fill a whole global batch (True keeps every rank's batch full; False
                deals the remainder round-robin and pads short ranks by repeating clips of the same bucket)
    """

    def __init__(self, lengths: Sequence[int], batch_size: int, world_size: int = 1, rank: int = 0, width: int = 16,
                 max_frames: Optional[int] = None, seed: int = 0, shuffle: bool = True, drop_last: bool = True):
        if not 0 <= rank < world_size:
            raise ValueError("rank must be in [0, world_size)")
        if batch_size < 1 or width < 1:
            raise ValueError("batch_size and width must be positive")
        self.lengths = np.asarray(lengths, dtype=np.int64)
        if max_frames is not None:
            self.lengths = np.minimum(self.lengths, int(max_frames))
        self.batch_size, self.world, self.rank, self.width = int(batch_size), int(world_size), int(rank), int(width)
        self.seed, self.shuffle, self.drop_last = int(seed), bool(shuffle), bool(drop_last)
        self.epoch = 0
        self.bounds = ((self.lengths + self.width - 1) // self.width) * self.width       # padded length of each clip's bucket
        self._buckets = {int(b): np.nonzero(self.bounds == b)[0] for b in np.unique(self.bounds)}

    def set_epoch(self, epoch: int) -> None:
        """Same contract as DistributedSampler.set_epoch: call once per epoch on every rank with the same value."""
        self.epoch = int(epoch)

    def _steps(self) -> list[tuple[int, np.ndarray]]:
        """[(padded frames, global batch of world*batch indices)] in this epoch's order — identical on every rank."""
        rng = np.random.default_rng([self.seed, self.epoch])
        G = self.world * self.batch_size
        steps: list[tuple[int, np.ndarray]] = []
        for bound in sorted(self._buckets):
            idx = self._buckets[bound]
            if self.shuffle:
                idx = rng.permutation(idx)
            full = len(idx) // G
            for s in range(full):
                steps.append((bound, idx[s * G:(s + 1) * G]))
            rest = idx[full * G:]
            if len(rest) and not self.drop_last:
                fill = idx[rng.integers(0, len(idx), G - len(rest))] if self.shuffle else np.resize(idx, G - len(rest))
                steps.append((bound, np.concatenate([rest, fill])))
        if self.shuffle:
            order = rng.permutation(len(steps))
            steps = [steps[i] for i in order]
        return steps

    def __iter__(self) -> Iterator[list[int]]:
        for _, g in self._steps():
            yield [int(i) for i in g[self.rank::self.world]]          # dealt round-robin: neighbours in the shuffle go to different ranks

    def __len__(self) -> int:
        G = self.world * self.batch_size
        n = 0
        for idx in self._buckets.values():
            n += len(idx) // G + (1 if (len(idx) % G and not self.drop_last) else 0)
        return n

    def padded_frames(self) -> list[int]:
        """Padded clip length of every step of the current epoch (the same list on every rank)."""
        return [b for b, _ in self._steps()]

    def padding_waste(self) -> float:
        """Fraction of padded frames that are padding, over the current epoch."""
        real = padded = 0
        for bound, g in self._steps():
            real += int(self.lengths[g].sum())
            padded += bound * len(g)
        return 1.0 - real / max(padded, 1)


def pad(samples: list[torch.Tensor], pad_val: float = 0.0, pad_to: Optional[int] = None) -> tuple[torch.Tensor, list[int]]:
    """Stack variable-length samples along a new batch axis, padding axis 0 of each to the longest (or to `pad_to`).
    Layout as the reference's `pad` (data_module.py:12-32): 1-D samples (targets) come back as [B, 1, L]."""
    lengths = [len(s) for s in samples]
    size = max(lengths) if pad_to is None else int(pad_to)
    if size < max(lengths):
        raise ValueError(f"pad_to={size} is shorter than the longest sample ({max(lengths)})")
    out = samples[0].new_full([len(samples), size] + list(samples[0].shape[1:]), pad_val)
    for i, s in enumerate(samples):
        out[i, : len(s)] = s
    if samples[0].dim() == 1:
        out = out.unsqueeze(1)
    return out, lengths


def collate_pad(batch: list[dict], pad_frames_to: Optional[int] = None, frames_per_unit: Optional[dict] = None,
                pad_targets_to_multiple: Optional[int] = None) -> dict:
    """The reference's `collate_pad` (data_module.py:34-43): {"inputs", "input_lengths", "targets", "target_lengths", ...} with
    targets padded by -1 and everything else by 0.  `pad_frames_to` (the sampler's bucket bound) pads "input" — and every key
    listed in `frames_per_unit` at its own rate, e.g. {"audio": 640} samples or {"audio": 4} tokens per video frame — to a fixed
    length, so that all ranks of a step produce the same shapes.

    `pad_targets_to_multiple=k` pads the "target" tails with -1 up to the next multiple of k tokens (target_lengths stay the real
    lengths), so that a bucketed epoch meets a few label shapes instead of one per longest transcript — what engine.TrainStep(native=True,
    max_shapes=...) keeps one recorded list for.  The losses do not depend on it mathematically (prepare_targets drops -1 wherever it sits; CTC
    uses per-row target lengths; the decoder's extra positions sit after the real ones under the causal mask; the label-smoothing loss is
    normalised by the batch with length_norm off; the accuracy ignores -1), but the step is NOT bit-identical: the reductions over the target
    rows change their row counts.  Measured on the tiny LRS case (tests/test_gpu_native_shapes.py, 3 steps): losses and accuracy
    bit-identical, parameters within 3e-8 (one or two ulps)."""
    if pad_targets_to_multiple is not None:
        if int(pad_targets_to_multiple) < 1:
            raise ValueError("pad_targets_to_multiple must be >= 1")
        if frames_per_unit and "target" in frames_per_unit:
            raise ValueError("'target' is padded either per video frame (frames_per_unit) or to a multiple of tokens, not both")
    out = {}
    for key in batch[0].keys():
        vals = [s[key] for s in batch if s[key] is not None]
        if not vals:
            continue
        to = None
        if pad_frames_to is not None:
            if key == "input":
                to = pad_frames_to
            elif frames_per_unit and key in frames_per_unit:
                to = pad_frames_to * int(frames_per_unit[key])
        if key == "target" and pad_targets_to_multiple is not None:
            k = int(pad_targets_to_multiple)
            to = -(-max(len(v) for v in vals) // k) * k
        c, lens = pad(vals, -1 if key == "target" else 0.0, to)
        out[key + "s"] = c
        out[key + "_lengths"] = torch.tensor(lens)
    return out


def collate_packed(batch: list[dict], pad_frames_to: Optional[int] = None, pad_targets_to_multiple: Optional[int] = None,
                   samples_per_frame: int = 640, pin: Optional[bool] = None) -> dict:
    """Host side of `DeviceLRSPipeline`: samples as the dataset STORES them, {"input": uint8 [T, Hs, Ws] or [T, 1, Hs, Ws] (one channel:
    AVDataset decodes with TJPF_GRAY, av_dataset.py:102), "audio": fp32 or int16 [S] (int16 = the decoded samples, which pydub_to_np divides
    by 32768), "target": int64 [L]}, with no transform applied -> one packed batch.  Nothing is padded but the waveforms and the targets:

        frames          uint8 [sum T_b, Hs, Ws], the clips back to back        offsets        int32 [B + 1], clip b = frames[offsets[b] : offsets[b + 1]]
        input_lengths   int64 [B] (T_b)                                        pad_frames     Tpad: pad_frames_to (the sampler's bucket bound) or the longest clip
        audios          fp32 or int16 [B, Spad], zero-padded; Spad = pad_frames_to * samples_per_frame, or the longest waveform
        audio_lengths   int64 [B]
        targets, target_lengths    exactly collate_pad's (-1 padding, [B, 1, L]; pad_targets_to_multiple as there)

    frames and audios are pinned (pin=None) when CUDA is available and the call runs in the main process, so the uploads can be
    asynchronous.  As the collate_fn of a DataLoader with workers it runs in a worker process, where nothing is pinned and CUDA is not
    touched: let the loader pin the batch in the parent, DataLoader(pin_memory=True).  Clips of differing Hs, Ws raise ValueError, as do a
    clip or a waveform longer than the bound."""
    if not batch:
        raise ValueError("empty batch")
    clips = []
    for s in batch:
        v = torch.as_tensor(s["input"])
        if v.dim() == 4 and v.size(1) == 1:
            v = v[:, 0]
        if v.dim() != 3 or v.dtype != torch.uint8:
            raise ValueError("'input' must be stored uint8 frames [T, Hs, Ws] or [T, 1, Hs, Ws]")
        clips.append(v)
    if any(v.shape[1:] != clips[0].shape[1:] for v in clips):
        raise ValueError(f"clips of one batch must share the stored frame size, got {sorted({tuple(v.shape[1:]) for v in clips})}")
    lens = [int(v.size(0)) for v in clips]
    Tpad = max(lens) if pad_frames_to is None else int(pad_frames_to)
    if Tpad < max(lens):
        raise ValueError(f"pad_frames_to={Tpad} is shorter than the longest clip ({max(lens)})")
    waves = [torch.as_tensor(s["audio"]).reshape(-1) for s in batch]
    if any(w.dtype != waves[0].dtype for w in waves) or waves[0].dtype not in (torch.float32, torch.int16):
        raise ValueError("'audio' must be fp32 or int16 samples, the same for every clip")
    alens = [int(w.numel()) for w in waves]
    Spad = max(alens) if pad_frames_to is None else Tpad * int(samples_per_frame)
    if Spad < max(alens):
        raise ValueError(f"a waveform of {max(alens)} samples is longer than pad_frames_to * samples_per_frame = {Spad}")
    if pin is None:          # (never from a DataLoader worker: it must not open the GPU, and pinning does not survive the hand-over to the parent)
        pin = torch.utils.data.get_worker_info() is None and torch.cuda.is_available()
    frames = torch.empty((sum(lens),) + tuple(clips[0].shape[1:]), dtype=torch.uint8, pin_memory=pin)
    offsets = torch.zeros(len(clips) + 1, dtype=torch.int32)
    offsets[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)
    for v, o, n in zip(clips, offsets.tolist(), lens):
        frames[o:o + n] = v
    audios = torch.zeros((len(waves), Spad), dtype=waves[0].dtype, pin_memory=pin)
    for b, w in enumerate(waves):
        audios[b, : alens[b]] = w
    tg = collate_pad([{"target": s["target"]} for s in batch], pad_targets_to_multiple=pad_targets_to_multiple)
    return {"frames": frames, "offsets": offsets, "input_lengths": torch.tensor(lens), "pad_frames": Tpad, "audios": audios,
            "audio_lengths": torch.tensor(alens), "targets": tg["targets"], "target_lengths": tg["target_lengths"]}


class DeviceLRSPipeline:
    """The reference's per-sample LRS transforms (LRS/video/datamodule/transforms.py:89-135; val / test: av_dataset.py:30-41) and the padding
    of `collate_pad`, on the device in three launches per batch: `collate_packed` hands over the stored uint8 crops and the raw waveforms, the
    host draws a few numbers per clip, and svsr_lrs_clip_prep / svsr_wave_prep (csrc/lrs_prep.hip) write the padded fp32 batch.

    train=True   video: x / 255 -> RandomResizedCrop(size, scale=(0.7, 1.0), ratio=(96/112, 112/96)) with torchvision's rejection sampling
                 (10 tries, then the central fallback) -> RandomHorizontalFlip(0.5) -> Normalize(mean, std); Grayscale() is the identity on
                 one stored channel.  time_mask=(window, stride) adds AdaptiveTimeMask(window, stride) in front of Normalize — (10, 25) is
                 the line the reference keeps commented out, so it is off by default.
                 audio: AddNoise — a segment of the noise bank at a uniform start in [0, Nn - S_b] and a level drawn from snr_levels
                 (999999 = clean) — then F.layer_norm over the whole waveform (eps 1e-8).  noise=None: the layer norm alone.
    train=False  video: the full stored frame resized to size x size (Resize(96) on the square stored crops, the LRS3 pipeline), or with
                 center_crop=True CenterCrop(size) (the LRS2 pipeline); no flip, no mask.  audio: noise only with snr_target (AddNoise(snr_target)),
                 then the layer norm.  snr_target=0 mixes at exactly 0 dB — a deviation: the reference tests `if snr_target`, so its
                 AddNoise(snr_target=0) falls back to the whole level list.

    The resize is bilinear, align_corners=False, WITHOUT antialias.  torchvision antialiases a tensor only when it shrinks; the LRS crops are
    stored at 96 x 96 and RandomResizedCrop(96) never draws a window larger than the stored frame, so there it only enlarges and antialias
    never acts.  A larger stored frame with a window above `size` is sampled without antialias, which torchvision would not do.
    The draws come from ONE numpy generator, per clip in the order window tries, flip, noise start, noise level, mask runs; torchvision and
    `random` (whose streams the reference consumes) cannot be pinned here, so the distributions are the reference's and the stream is not."""

    SCALE = (0.7, 1.0)
    RATIO = (96 / 112, 112 / 96)

    def __init__(self, train: bool, size: int = 96, seed: int = 0, noise: Optional[torch.Tensor] = None,
                 snr_levels: Sequence[float] = (-5, 0, 5, 10, 15, 20, 999999), time_mask: Optional[tuple[int, int]] = None, mean: float = 0.421,
                 std: float = 0.165, center_crop: bool = False, snr_target: Optional[float] = None):
        self.train, self.size, self.mean, self.std, self.center_crop = bool(train), int(size), float(mean), float(std), bool(center_crop)
        self.snr_levels = [float(snr_target)] if snr_target is not None else [float(v) for v in snr_levels]
        self.time_mask = None if time_mask is None else (int(time_mask[0]), int(time_mask[1]))
        self.mix = noise is not None and (self.train or snr_target is not None)
        self.noise = None if noise is None else torch.as_tensor(noise, dtype=torch.float32).reshape(-1).contiguous()      # (uploaded once, at the first batch)
        self.rng = np.random.default_rng(seed)

    def _window(self, Hs: int, Ws: int) -> tuple[int, int, int, int]:
        """RandomResizedCrop.get_params: (top, left, h, w)."""
        import math

        lo, hi = self.RATIO
        for _ in range(10):
            target = Hs * Ws * self.rng.uniform(*self.SCALE)
            ratio = math.exp(self.rng.uniform(math.log(lo), math.log(hi)))
            w, h = int(round(math.sqrt(target * ratio))), int(round(math.sqrt(target / ratio)))
            if 0 < w <= Ws and 0 < h <= Hs:
                return int(self.rng.integers(0, Hs - h + 1)), int(self.rng.integers(0, Ws - w + 1)), h, w
        in_ratio = Ws / Hs                     # the central crop with the nearest admissible ratio
        if in_ratio < lo:
            w, h = Ws, int(round(Ws / lo))
        elif in_ratio > hi:
            h = Hs
            w = int(round(h * hi))
        else:
            w, h = Ws, Hs
        return (Hs - h) // 2, (Ws - w) // 2, h, w

    def _mask_runs(self, T: int) -> list[tuple[int, int]]:
        """AdaptiveTimeMask.forward (transforms.py:50-64): [(start, length)] as drawn.  Each of the n_mask rows of its randint(0, window) table
        is (t, length): t bounds the start, randrange(0, T - t), and decides the two skips (T - t <= 0 before the start is drawn, t == 0
        after it); the zeroed frames are x[start : start + length], so a length of 0 is a run that masks nothing and a run that passes
        T is cut there by the slice."""
        window, stride = self.time_mask
        runs = []
        for t, length in self.rng.integers(0, window, size=(int((T + stride - 0.1) // stride), 2)):
            if T - t <= 0:
                continue
            start = int(self.rng.integers(0, T - t))
            if t == 0:
                continue
            runs.append((start, int(length)))
        return runs

    def draw(self, lengths: Sequence[int], Hs: int, Ws: int, audio_lengths: Optional[Sequence[int]] = None,
             pad_frames_to: Optional[int] = None) -> dict:
        """The host decisions of one batch: {"params": int32 [B, 5] = (top, left, h, w, flip), "nstart": int32 [B], "snr_db": fp32 [B],
        "runs": per clip [(start, length)] of the time mask as drawn (a length may be 0 or pass the clip's end), "tmask": uint8 [B, Tpad]
        the frames they zero (None without time_mask)}."""
        lengths = [int(t) for t in lengths]
        B, S = len(lengths), self.size
        audio_lengths = [0] * B if audio_lengths is None else [int(s) for s in audio_lengths]
        Nn = 0 if self.noise is None else self.noise.numel()
        if self.mix and max(audio_lengths) > Nn:
            raise ValueError(f"the noise bank ({Nn} samples) is shorter than the longest waveform ({max(audio_lengths)})")
        Tpad = max(lengths) if pad_frames_to is None else int(pad_frames_to)
        params = np.zeros((B, 5), dtype=np.int32)
        nstart, snr = np.zeros(B, dtype=np.int32), np.full(B, 999999.0, dtype=np.float32)
        masked = self.train and self.time_mask is not None
        tmask = np.zeros((B, Tpad), dtype=np.uint8) if masked else None
        runs: list[list[tuple[int, int]]] = [[] for _ in range(B)]
        for b in range(B):
            if self.train:
                params[b, :4] = self._window(Hs, Ws)
                params[b, 4] = int(self.rng.random() < 0.5)
            elif self.center_crop:
                if S > Hs or S > Ws:
                    raise ValueError(f"CenterCrop({S}) of a {Hs} x {Ws} frame")
                params[b, :4] = ((Hs - S) // 2, (Ws - S) // 2, S, S)
            else:
                params[b, :4] = (0, 0, Hs, Ws)
            if self.mix:
                nstart[b] = self.rng.integers(0, Nn - audio_lengths[b] + 1)
                snr[b] = self.snr_levels[int(self.rng.integers(0, len(self.snr_levels)))]
            if masked:
                runs[b] = self._mask_runs(lengths[b])
                for start, n in runs[b]:
                    tmask[b, start:min(start + n, lengths[b])] = 1
        return {"params": torch.from_numpy(params), "nstart": torch.from_numpy(nstart), "snr_db": torch.from_numpy(snr), "runs": runs,
                "tmask": None if tmask is None else torch.from_numpy(tmask)}

    def __call__(self, packed: dict, draws: Optional[dict] = None, device: Optional[torch.device] = None) -> dict:
        """`collate_packed`'s batch -> the dictionary `collate_pad` returns, on the device: inputs fp32 [B, Tpad, 1, size, size], input_lengths,
        audios fp32 [B, 1, Spad], audio_lengths, targets, target_lengths — what E2E.forward(batch["inputs"], batch["input_lengths"],
        batch["audios"], batch["targets"]) and TrainStep take.  Three launches, asynchronous copies, no host synchronisation."""
        from . import ops

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        frames, audios = packed["frames"], packed["audios"]
        lens, alens, Tpad = packed["input_lengths"], packed["audio_lengths"], int(packed["pad_frames"])
        B, (Hs, Ws) = lens.numel(), frames.shape[1:]
        if draws is None:
            draws = self.draw(lens.tolist(), Hs, Ws, alens.tolist(), Tpad)
        params, nstart = draws["params"], draws["nstart"]
        top, left, h, w = (params[:, i] for i in range(4))
        if params.shape != (B, 5) or bool(((top < 0) | (left < 0) | (h < 1) | (w < 1) | (top + h > Hs) | (left + w > Ws)).any()):
            raise ValueError("crop window outside the stored frame")
        if self.mix:
            Nn = self.noise.numel()
            if int(alens.max()) > Nn:
                raise ValueError(f"the noise bank ({Nn} samples) is shorter than the longest waveform ({int(alens.max())})")
            if bool(((nstart < 0) | (nstart.long() + alens > Nn)).any()):
                raise ValueError("noise segment outside the noise bank")
            if self.noise.device != dev:
                self.noise = self.noise.to(dev)
        # every per-clip number in ONE small upload: offsets | params | audio lengths | noise starts | SNR bits
        meta = torch.cat([packed["offsets"].to(torch.int32), params.reshape(-1).to(torch.int32), alens.to(torch.int32), nstart.to(torch.int32),
                          draws["snr_db"].to(torch.float32).view(torch.int32)]).to(dev, non_blocking=True)
        off, par, alen_d, nst, snr = meta[: B + 1], meta[B + 1: 6 * B + 1].view(B, 5), meta[6 * B + 1: 7 * B + 1], meta[7 * B + 1: 8 * B + 1], meta[8 * B + 1:].view(torch.float32)
        tmask = draws.get("tmask")
        if tmask is not None:
            if tmask.shape != (B, Tpad):
                raise ValueError(f"tmask must be [B, pad_frames] = {(B, Tpad)}")
            tmask = tmask.to(dev, non_blocking=True)
        x = ops.lrs_clip_prep(frames.to(dev, non_blocking=True), off, par, Tpad, self.size, self.size, self.mean, self.std, tmask)
        a = ops.wave_prep(audios.to(dev, non_blocking=True), alen_d, self.noise if self.mix else None, nst, snr)
        return {"inputs": x, "input_lengths": lens.to(dev, non_blocking=True), "audios": a.unsqueeze(1), "audio_lengths": alens.to(dev, non_blocking=True),
                "targets": packed["targets"].to(dev, non_blocking=True), "target_lengths": packed["target_lengths"].to(dev, non_blocking=True)}


def reference_length_histogram(n: int, seed: int = 0, lo: int = 12, hi: int = 155, mean: float = 84.7) -> np.ndarray:
    """Synthetic clip lengths with the range and mean of the reference's training set (video_length.npy: 31,982 clips,
    min 12 / max 155 / mean 84.7 frames) — for benchmarks and tests; the real file cannot travel."""
    rng = np.random.default_rng(seed)
    a = (mean - lo) / (hi - lo)
    x = rng.beta(2.0 * a / (1 - a) if a < 0.5 else 2.0, 2.0 if a < 0.5 else 2.0 * (1 - a) / a, n)
    return np.clip(np.round(lo + x * (hi - lo)), lo, hi).astype(np.int64)
