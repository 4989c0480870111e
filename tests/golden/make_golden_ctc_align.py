"""Golden vectors for CTC forced alignment.  RUNS ONLY IN THE BUILD CONTAINER: imports the reference itself (import stub of
make_golden_lrs.py) and records what ITS `CTC.forced_align_batch` (espnet/nets/pytorch_backend/ctc.py:246-328) returns for seeded fp32
activations: ragged batches of 1-4 clips, 3-39 frames, 1-6 labels drawn from five of the 41 units so that repeated labels are frequent.
Only numbers are stored: per batch the activations hs [Tmax, B, V], ys [B, Lmax] padded with -1, ilens [B], the clip indices that were
recorded and the reference's alignments [B, Tmax] padded with -1.

Every clip is generated feasible (the reference is undefined otherwise), and two assertions keep the fixture from pinning a defect: every
reference output collapses to its transcript, and tests/ctc_align_restatement.py equals the reference on every clip.

    python tests/golden/make_golden_ctc_align.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from ctc_align_restatement import align_one, collapse, frames_needed  # noqa: E402
from make_golden_lrs import import_reference  # noqa: E402

V = 41
ALPHABET = (3, 7, 12, 25, 40)
BATCHES = 20
SEED = 20240


def make_batches() -> list:
    """(hs fp32 [Tmax, B, V], ys int64 [B, Lmax], ilens int64 [B]) per batch; the first ones pin the corners of the ranges."""
    rng = np.random.default_rng(SEED)
    corners = [(1, 3, 1), (4, 39, 6), (2, 12, 6), (3, 3, 1)]                  # (B, Tmax, Lmax)
    out = []
    for i in range(BATCHES):
        B, Tmax, Lmax = corners[i] if i < len(corners) else (int(rng.integers(1, 5)), int(rng.integers(3, 40)), int(rng.integers(1, 7)))
        ys = np.full((B, Lmax), -1, np.int64)
        ilens = np.zeros(B, np.int64)
        for b in range(B):
            while True:
                L = Lmax if b == 0 else int(rng.integers(1, Lmax + 1))
                y = rng.choice(ALPHABET, size=L)
                if frames_needed(y) <= Tmax:
                    break
            ys[b, :L] = y
            ilens[b] = Tmax if b == 0 else int(rng.integers(frames_needed(y), Tmax + 1))
        hs = (rng.standard_normal((Tmax, B, V)) * 3.0).astype(np.float32)
        out.append((hs, ys, ilens))
    return out


def main() -> None:
    import_reference()
    from espnet.nets.pytorch_backend.ctc import CTC

    if not hasattr(np, "bool"):          # ctc.py:290 spells the dtype `np.bool`
        np.bool = bool
    ctc = CTC(V, 8, 0.0)
    res: dict[str, np.ndarray] = {"n_batches": np.int64(BATCHES), "V": np.int64(V)}
    clips = 0
    for i, (hs, ys, ilens) in enumerate(make_batches()):
        Tmax, B, _ = hs.shape
        ali = ctc.forced_align_batch(torch.from_numpy(hs), torch.from_numpy(ys), torch.from_numpy(ilens), blank_id=0)
        lp = torch.log_softmax(torch.from_numpy(hs), dim=-1).numpy()
        rec = np.full((B, Tmax), -1, np.int64)
        for b in range(B):
            y = ys[b][ys[b] != -1]
            a = np.asarray(ali[b])
            assert a.dtype == np.int64 and a.shape == (ilens[b],)
            assert collapse(a, 0) == y.tolist(), (i, b, "the reference's alignment does not spell its transcript")
            mine = align_one(lp[: ilens[b], b], y, 0)[0]
            assert np.array_equal(mine, a), (i, b, "the restatement differs from the reference")
            rec[b, : ilens[b]] = a
            clips += 1
        res[f"b{i}.hs"], res[f"b{i}.ys"], res[f"b{i}.ilens"], res[f"b{i}.ali"] = hs, ys, ilens, rec
        res[f"b{i}.clips"] = np.arange(B, dtype=np.int64)
    path = os.path.join(HERE, "ctc_align.npz")
    np.savez_compressed(path, **res)
    print(f"{clips} clips in {BATCHES} batches, all valid and equal to the restatement -> {path} ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
