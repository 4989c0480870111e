"""CTC greedy decoding at the shipped LRS size: `lrs_align.greedy_features` (one ctc_lo over the batch to fp32 logits, svsr_ctc_frame_best,
svsr_ctc_collapse, one device-to-host copy) beside the path a user had before: `E2E.ctc.argmax` (per clip ctc_lo + a stored [T, odim] fp32
log-softmax + torch.argmax), a download of the [C, T] ids and `itertools.groupby` on the host.  C = 8 clips of 150 frames, 5,049 units.

    python scripts/greedy_bench.py [--clips 8] [--frames 150] [--rounds 7] [--iters 20] [--out profiles/ctc_greedy.json]

Inputs: seeded synthetic encoder outputs and seeded weights (ctc_lo scaled up so the posteriors are peaked, as scripts/align_bench.py does);
every feature row is held for three frames, so there are runs to collapse.  Times are wall-clock between device synchronisations, host
dispatch and the copy included; the two sides alternate round by round after a warm-up; per side the median over rounds of the mean of
`--iters` calls, and the minimum.  The old side returns transcripts only (no spans, no confidences).  Both sides must return the same
transcripts.  The frame kernel is also timed alone: `--kiters` launches of the C entry point back to back on the same logits between two
device events; bytes read (live rows * units * 4) over that time is a read rate that includes the launch gaps, and the 22 MB of logits stay
in the last-level cache between launches — it is not an HBM rate.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

VOCAB = 5049


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kiters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_greedy.json"))
    a = ap.parse_args()
    from syncvsr_amd import _lib, ops
    from syncvsr_amd.lrs_align import greedy_features
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
    C, T = a.clips, a.frames
    lens = [T - (7 * c) % 40 for c in range(C)]
    xs = torch.zeros(C, T, model.adim)
    for c, t in enumerate(lens):
        xs[c, :t] = torch.randn(t, model.adim, generator=g).repeat_interleave(3, dim=0)[:t]      # (runs of three frames: something to collapse)
    xs = xs.to(dev)

    def new_side():
        return greedy_features(model, xs, lens)

    def old_side():
        ids = model.ctc.argmax(xs).cpu().numpy()
        return [np.array([v for v, _ in itertools.groupby(ids[c, : lens[c]].tolist()) if v != 0], dtype=np.int64) for c in range(C)]

    paths, old = new_side(), old_side()                                          # warm-up, and the two sides against each other
    torch.cuda.synchronize()
    same = all(np.array_equal(p.tokens, o) for p, o in zip(paths, old))
    nts, ots = [], []
    for _ in range(a.rounds):
        for side, ts in ((new_side, nts), (old_side, ots)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                side()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / a.iters)

    logits = CTCPrefixScorer(model, model.eos).ctc_logits(xs.reshape(C * T, model.adim))
    tlen = torch.tensor(lens, dtype=torch.int32, device=dev)
    best, best_logp = ops.ctc_frame_best(logits, tlen, Tmax=T, V=VOCAB)
    fn, stream = _lib.load().svsr_ctc_frame_best, torch.cuda.current_stream().cuda_stream
    argv = (logits.data_ptr(), logits.stride(0), tlen.data_ptr(), C, T, VOCAB, best.data_ptr(), best_logp.data_ptr(), stream)

    def launches(n):                                                             # the C entry point itself: no allocation, no wrapper between two launches
        for _ in range(n):
            if fn(*argv) != 0:
                raise SystemExit("svsr_ctc_frame_best refused the launch")

    launches(10)
    kts = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        launches(a.kiters)
        e1.record()
        torch.cuda.synchronize()
        kts.append(e0.elapsed_time(e1) * 1e3 / a.kiters)
    nbytes = 4 * VOCAB * sum(lens)
    k_us = statistics.median(kts)
    out = dict(what="CTC greedy decoding: lrs_align.greedy_features vs E2E.ctc.argmax per clip + a download of the ids + groupby on the host",
               device=torch.cuda.get_device_name(0), clips=C, frames=T, vocab=VOCAB, lengths=lens, rounds=a.rounds, iters=a.iters,
               tokens=[int(len(p.tokens)) for p in paths],
               greedy_features_ms_median=round(statistics.median(nts), 3), greedy_features_ms_min=round(min(nts), 3),
               argmax_groupby_ms_median=round(statistics.median(ots), 3), argmax_groupby_ms_min=round(min(ots), 3),
               same_tokens=bool(same),
               frame_best_us_per_launch_median=round(k_us, 2), frame_best_us_per_launch_min=round(min(kts), 2), frame_best_launches=a.kiters,
               frame_best_bytes_read=nbytes, frame_best_read_GBps=round(nbytes / (k_us * 1e-6) / 1e9, 1),
               note="wall clock between synchronisations for the two sides, both include ctc_lo; the frame kernel alone: device events around "
                    "back-to-back launches on the same logits (launch gaps included, logits cache-resident between launches: a read rate, not an HBM rate)")
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    if not same:
        raise SystemExit("the two sides disagree")


if __name__ == "__main__":
    main()
