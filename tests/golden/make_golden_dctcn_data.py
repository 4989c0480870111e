"""Golden for the DC-TCN dataset's augmentations (reference LRW/video/src/data.py:83-106).  RUNS ONLY IN THE BUILD CONTAINER.
Runs the reference's LRWDatasetForDCTCN._mask_frames + _trim_frames under fixed np.random seeds on small clips (frames 1 x 6 x 5, T = 29
and T = 8, a waveform of L = 1000 samples so that T / L is no integer ratio, word lengths 1, 5 and T - 1) and stores the inputs, the
integers np.random.randint returned, and the four outputs; tests/test_dctcn_pipeline_cpu.py replays tests/dctcn_pipeline_restatement.py
and augment.DeviceDCTCNPipeline.plan with the same seeds.  The reference's module imports turbojpeg, pandas, torchvision and omegaconf
when it is loaded; where one is missing an empty stand-in goes under its name first (none of them is used by the two methods).  The
spatial transform is not in the golden (torchvision is not available): csrc/clip_sample.h has its own tests."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for name, attrs in (("turbojpeg", dict(TJPF_GRAY=0, TurboJPEG=lambda: None)), ("pandas", dict(DataFrame=object)), ("torchvision", {}),
                    ("omegaconf", dict(DictConfig=dict))):
    try:
        importlib.import_module(name)
    except ImportError:
        stand_in = types.ModuleType(name)
        stand_in.__dict__.update(attrs)
        sys.modules[name] = stand_in
sys.path.insert(0, "/root/reference/LRW/video/src")
from data import LRWDatasetForDCTCN  # noqa: E402  (the reference's)

MAX_TIME_MASKS, L = 15, 1000
res = {"max_time_masks": np.int64(MAX_TIME_MASKS)}
cases = []
real_randint = np.random.randint
for T, max_masks in ((29, MAX_TIME_MASKS), (8, 6)):
    g = torch.Generator().manual_seed(100 + T)
    clip = torch.randint(0, 256, (T, 1, 6, 5), dtype=torch.uint8, generator=g)
    wave = torch.randn(L, generator=g)
    res[f"clip_T{T}"], res[f"wave_T{T}"] = clip[:, 0].numpy(), wave.numpy()
    ds = LRWDatasetForDCTCN([], [], None, None, max_time_masks=max_masks)
    for wb in (1, 5, T - 1):
        for seed in (0, 1, 2, 3):
            drawn = []

            def recording(*a, **k):
                drawn.append(int(real_randint(*a, **k)))
                return drawn[-1]

            start = (T - wb) // 2
            batch = {"videos": 2 * clip.float() / 0xFF - 1, "audios": wave.clone(), "attention_mask": torch.ones(T, dtype=torch.long),
                     "word_mask": torch.zeros(T, dtype=torch.long)}
            batch["word_mask"][start:start + wb] = 1
            np.random.seed(seed)
            np.random.randint = recording
            try:
                ds._mask_frames(batch)
                ds._trim_frames(batch)
            finally:
                np.random.randint = real_randint
            assert len(drawn) == 4
            tag = f"T{T}_wb{wb}_s{seed}"
            cases.append((T, max_masks, wb, seed))
            res[f"drawn_{tag}"] = np.asarray(drawn, dtype=np.int64)          # length, offset, truncated, off2
            res[f"videos_{tag}"] = batch["videos"][:, 0].numpy()
            res[f"audios_{tag}"] = batch["audios"].numpy()
            res[f"word_mask_{tag}"] = batch["word_mask"].numpy()
            res[f"attention_mask_{tag}"] = batch["attention_mask"].numpy()
res["cases"] = np.asarray(cases, dtype=np.int64)          # T, max_time_masks, word length, seed
np.savez_compressed(os.path.join(HERE, "dctcn_data.npz"), **res)
print(len(cases), "cases,", os.path.getsize(os.path.join(HERE, "dctcn_data.npz")), "bytes")
