"""Seeded cases of the DC-TCN tests (tests/test_dctcn_cpu.py, tests/test_gpu_dctcn*.py): configuration, weights regenerated from a seed
under the reference's state-dict names (syncvsr_amd/dctcn_init.py), inputs, and the golden numbers tests/golden/make_golden_dctcn.py recorded
from the reference's own `tcn.model.Lipreading` in fp64."""
from __future__ import annotations

import os

import numpy as np
import torch

from syncvsr_amd.dctcn_init import (dctcn_dims, dctcn_init_state_dict, dctcn_synthetic_batch, default_dctcn_config, tiny_dctcn_config)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# golden file -> sub-cases (tag, config factory, weight seed, B, T, frame size, batch seed, clip lengths, labels).  Lengths: one all-ones attention row, the
# others with a fully padded tail.  The seeds and the classifier gain (dctcn_init_state_dict head_gain) were fixed before any kernel ran; the
# generator asserts on the REFERENCE alone that three quarters of the clips have a top-1 / top-2 gap above ten times the bf16 floor.
# Labels are chosen from the reference's own predictions so that the accuracies are not trivially zero: one clip labelled with its top-1
# class, one with its second class (inside the top five, not first), and in the tiny cases one with a class far down the ranking:
# top-1 / top-5 = 1/3, 2/3 (tiny) and 1/2, 1 (full).  The generator asserts each label's top-1 and top-5 membership holds by a margin of ten
# times the absolute bf16 floor of the logits.
DCTCN_CASES = {
    "dctcn_tiny": [
        ("wb_t29", lambda: tiny_dctcn_config(True), 3, 3, 29, 40, 24, [29, 17, 22], [492, 407, 29]),
        ("nowb_t7", lambda: tiny_dctcn_config(False), 6, 3, 7, 40, 22, [7, 4, 5], [412, 308, 96]),
    ],
    "dctcn_full": [
        ("full", lambda: default_dctcn_config(), 7, 2, 29, 96, 23, [29, 19], [118, 431]),
    ],
}


def audio_rows(B: int, T: int) -> list:
    """Rows b * T + t of logits_audio [B*T, 2560] the goldens keep (first / last frames of clips, frames inside padded tails)."""
    return [r for r in (0, 6, 7, 13, 20, 28, 29, 45, 57, 86) if r < B * T]


def dctcn_subcase(name: str, tag: str):
    """-> (cfg, dims, state dict, batch = (videos, tokens, labels, word_mask, attention_mask))"""
    for t, mk, wseed, B, T, size, bseed, lengths, labels in DCTCN_CASES[name]:
        if t == tag:
            cfg = mk()
            sd = dctcn_init_state_dict(cfg, seed=wseed)
            videos, tokens, _, word, attention = dctcn_synthetic_batch(cfg, B, T, size=size, seed=bseed, lengths=lengths)
            batch = (videos, tokens, torch.tensor(labels, dtype=torch.long), word, attention)
            return cfg, dctcn_dims(cfg), sd, batch
    raise KeyError((name, tag))


def dctcn_tags(name: str) -> list:
    return [c[0] for c in DCTCN_CASES[name]]


def load_golden(name: str):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)


def rel_err(a, b) -> float:
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))
