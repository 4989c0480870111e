"""CTC forced alignment at the shipped LRS size: `lrs_align.align_features` (ctc_lo + log_softmax over the batch, one svsr_ctc_align launch,
one device-to-host copy) beside the numpy restatement of the reference's algorithm (tests/ctc_align_restatement.py) on the same posteriors
downloaded to the host — what `CTC.forced_align_batch` does, and what a user had before.  B = 16 clips of 160 frames, 48 labels each,
5,049 units.

    python scripts/align_bench.py [--clips 16] [--frames 160] [--labels 48] [--rounds 7] [--iters 20] [--out profiles/ctc_align.json]

Inputs: seeded synthetic encoder outputs and seeded weights (ctc_lo scaled up so the posteriors are peaked, as scripts/beam_bench.py does),
seeded transcripts.  Times are wall-clock between device synchronisations, host dispatch and the copy included; the two sides alternate
round by round after a warm-up; per side the median over rounds of the mean of its calls (`--iters` for the device side, one for the numpy
side), and the minimum.  The numpy side's time includes the download of the [B, T, V] posteriors, as the reference's `.cpu()` does.  The
kernel is a chain of `frames` dependent steps per clip: the figure is a latency, no rate is derived from it.  Both sides must return the same
frames.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

VOCAB = 5049


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--labels", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align.json"))
    a = ap.parse_args()
    from ctc_align_restatement import align_batch
    from syncvsr_amd.lrs_align import align_features
    from syncvsr_amd.lrs_infer import CTCPrefixScorer
    from syncvsr_amd.lrs_init import default_lrs_args, lrs_init_state_dict
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args = default_lrs_args()
    sd = lrs_init_state_dict(args, VOCAB, seed=0, perturb_norm=False)
    sd["ctc.ctc_lo.weight"] = sd["ctc.ctc_lo.weight"] * 8.0
    model = E2E(VOCAB, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    B, T, L = a.clips, a.frames, a.labels
    lens = [T - (7 * c) % 40 for c in range(B)]
    xs = torch.zeros(B, T, model.adim)
    for c, t in enumerate(lens):
        xs[c, :t] = torch.randn(t, model.adim, generator=g)
    xs = xs.to(dev)
    targets = torch.randint(1, VOCAB - 1, (B, L), generator=g)

    scorer = CTCPrefixScorer(model, model.eos)

    def device_side():
        return align_features(model, xs, lens, targets)

    def numpy_side():
        logp = scorer.ctc_log_softmax(xs.reshape(B * T, model.adim)).view(B, T, -1).cpu().numpy()       # the posteriors align_features aligns
        return align_batch(logp, lens, targets.numpy(), 0)

    alis, (frames, _, score) = device_side(), numpy_side()                       # warm-up, and the two sides against each other
    torch.cuda.synchronize()
    same = all(np.array_equal(al.frames, frames[c, : lens[c]]) for c, al in enumerate(alis))
    dts, nts = [], []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            device_side()
        torch.cuda.synchronize()
        dts.append((time.perf_counter() - t0) * 1e3 / a.iters)
        t0 = time.perf_counter()
        numpy_side()
        nts.append((time.perf_counter() - t0) * 1e3)
    out = dict(what="CTC forced alignment: lrs_align.align_features vs the numpy restatement of the reference's algorithm on downloaded posteriors",
               device=torch.cuda.get_device_name(0), clips=B, frames=T, labels=L, vocab=VOCAB, lengths=lens, rounds=a.rounds, iters=a.iters,
               align_features_ms_median=round(statistics.median(dts), 3), align_features_ms_min=round(min(dts), 3),
               numpy_restatement_ms_median=round(statistics.median(nts), 3), numpy_restatement_ms_min=round(min(nts), 3),
               same_frames=bool(same),
               note="wall clock between synchronisations; both sides include ctc_lo + log_softmax; the numpy side includes the download of the posteriors; "
                    "a latency chain of `frames` dependent steps per clip, no rate is claimed")
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    if not same:
        raise SystemExit("the two sides disagree")


if __name__ == "__main__":
    main()
