"""Edit distance of a batch of transcript pairs: `ops.edit_distance` (svsr_edit_distance, one wave per pair) beside what a user has without it:
a plain Python two-row DP over the host copies of the same ids.  (The reference calls torchaudio.functional.edit_distance; torchaudio is
not installed beside this project, and neither is editdistance, so the Python DP is the comparison that can be run.)

    python scripts/eval_bench.py [--rounds 7] [--iters 50] [--py-rounds 2] [--out profiles/lrs_eval.json]

Two shapes: 640 pairs of about 20 words (16 clips x an n-best of 40 at the word level: ids drawn from 2,000 words, the hypothesis a copy of
the reference with a fifth of its words substituted, dropped or doubled), and 16 pairs of 1,024 tokens (the length cap, 5,000 ids).  The
device side is timed twice: wall clock between two synchronisations around `--iters` calls of `ops.edit_distance` on device tensors
(allocation of the output and host dispatch included, no copy), and device events around `--iters` back-to-back launches of the C entry
point (launch gaps included).  The Python side is timed once per round on host lists (no copy included).  Per side the median over the
rounds.  No target is set; the two sides must agree on every distance.  Prints one JSON line and writes it to --out.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def python_dp(a: list, b: list) -> int:
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def make_pairs(rng, n: int, length: int, spread: int, vocab: int) -> tuple[list, list]:
    hyps, refs = [], []
    for _ in range(n):
        ref = rng.integers(0, vocab, size=max(1, length + int(rng.integers(-spread, spread + 1)))).tolist()
        hyp = []
        for w in ref:
            u = rng.random()
            if u < 0.07:
                hyp.append(int(rng.integers(0, vocab)))
            elif u < 0.14:
                continue
            elif u < 0.20:
                hyp += [w, w]
            else:
                hyp.append(w)
        hyps.append(hyp[:length + spread])
        refs.append(ref)
    return hyps, refs


def pad(rows: list) -> tuple[torch.Tensor, torch.Tensor]:
    out = torch.full((len(rows), max(len(r) for r in rows)), -1, dtype=torch.int64)
    for n, r in enumerate(rows):
        out[n, : len(r)] = torch.tensor(r, dtype=torch.int64)
    return out, torch.tensor([len(r) for r in rows], dtype=torch.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--py-rounds", type=int, default=2, help="rounds of the Python side (16 pairs of 1,024 tokens take it seconds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrs_eval.json"))
    a = ap.parse_args()
    from syncvsr_amd import _lib, ops

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    shapes = {"nbest_640x20_words": make_pairs(rng, 640, 20, 6, 2000), "long_16x1024_tokens": make_pairs(rng, 16, 1024, 0, 5000)}
    out = dict(what="ops.edit_distance (svsr_edit_distance, one wave per pair) vs a plain Python two-row DP over the host copies",
               device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, py_rounds=a.py_rounds,
               note="torchaudio (the reference's torchaudio.functional.edit_distance) and editdistance are not installed: the Python DP stands for "
                    "what a user has today; op: wall clock between synchronisations, output allocation and dispatch included, no copy; kernel: "
                    "device events around back-to-back launches of the C entry point, launch gaps included")
    agree = True
    for name, (hyps, refs) in shapes.items():
        (hyp, hyp_len), (ref, ref_len) = pad(hyps), pad(refs)
        hyp, hyp_len, ref, ref_len = (t.to(dev) for t in (hyp, hyp_len, ref, ref_len))
        got = ops.edit_distance(hyp, hyp_len, ref, ref_len)                      # warm-up, and the two sides against each other
        torch.cuda.synchronize()
        agree = agree and got[:, 0].cpu().tolist() == [python_dp(h, r) for h, r in zip(hyps, refs)]
        fn, stream = _lib.load().svsr_edit_distance, torch.cuda.current_stream().cuda_stream
        argv = (hyp.data_ptr(), hyp.stride(0), hyp_len.data_ptr(), ref.data_ptr(), ref.stride(0), ref_len.data_ptr(), hyp.shape[0], got.data_ptr(), stream)
        ops_ms, ker_us, py_ms = [], [], []
        for rnd in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                ops.edit_distance(hyp, hyp_len, ref, ref_len)
            torch.cuda.synchronize()
            ops_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                if fn(*argv) != 0:
                    raise SystemExit("svsr_edit_distance refused the launch")
            e1.record()
            torch.cuda.synchronize()
            ker_us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
            if rnd < a.py_rounds:
                t0 = time.perf_counter()
                for h, r in zip(hyps, refs):
                    python_dp(h, r)
                py_ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(pairs=len(hyps), mean_hyp_len=round(float(np.mean([len(h) for h in hyps])), 1),
                         mean_ref_len=round(float(np.mean([len(r) for r in refs])), 1), mean_distance=round(float(got[:, 0].float().mean()), 2),
                         op_ms_median=round(statistics.median(ops_ms), 4), op_ms_min=round(min(ops_ms), 4),
                         kernel_us_per_launch_median=round(statistics.median(ker_us), 2), kernel_us_per_launch_min=round(min(ker_us), 2),
                         python_dp_ms_median=round(statistics.median(py_ms), 2), python_dp_ms_min=round(min(py_ms), 2))
    out["same_distances"] = bool(agree)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    if not agree:
        raise SystemExit("the two sides disagree")


if __name__ == "__main__":
    main()
