"""Clips per second of the LRS beam search at the shipped model size (beam 40, CTC weight 0.1, 5,049 units): `BatchBeamSearch.forward` clip
after clip beside `BatchBeamSearch.forward_clips` over the same clips C at a time, C = 1, 8, 32, 64, with and without the transformer
language model.  `forward` is a one-clip group of the multi-clip search, so the "forward, clip after clip" row (`seq`) times the same code
path as the `forward_clips` C = 1 row and the two should agree within their spread; run on a checkout from before the searches were merged,
the first row times the separate single-clip loop the package had then.

    python scripts/beam_bench.py [--clips 64] [--groups 1,8,32,64] [--reps 3] [--lm 0,1] [--out profiles/round9_beam_clips.json]

Inputs: seeded synthetic encoder outputs, lengths drawn from the LRS length histogram of syncvsr_amd/lrs_data.py; seeded weights (the output
layers are scaled up so that hypotheses end as they do on a trained model, see tests/golden_cases.py).  Times are wall-clock between device
synchronisations, host dispatch included: one warm-up pass, then `--reps` passes; median and (min, max) are reported.  Launches per
position are counted with ops' event timing over one extra pass.  Prints one JSON line per row and writes all of them to --out.
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

import torch  # noqa: E402

LM_ARGS = dict(layer=16, unit=2048, att_unit=512, embed_unit=128, head=8, pos_enc="sinusoidal")
VOCAB = 5049


def _timed(fn, reps: int):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--groups", default="1,8,32,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lm", default="0,1")
    ap.add_argument("--max-frames", type=int, default=155)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round9_beam_clips.json"))
    a = ap.parse_args()
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_data import reference_length_histogram
    from syncvsr_amd.lrs_infer import get_beam_search_decoder
    from syncvsr_amd.lrs_init import default_lrs_args, lrs_init_state_dict
    from syncvsr_amd.lrs_lm import TransformerLM
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args = default_lrs_args()
    sd = lrs_init_state_dict(args, VOCAB, seed=0, perturb_norm=False)
    for k in ("decoder.output_layer.weight", "ctc.ctc_lo.weight"):
        sd[k] = sd[k] * 8.0                                   # peaked posteriors: hypotheses end (tests/golden_cases.py does the same)
    sd["decoder.output_layer.bias"][VOCAB - 1] += 4.0
    model = E2E(VOCAB, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    lm = TransformerLM(VOCAB, LM_ARGS).to(dev)
    tokens = [f"t{i}" for i in range(VOCAB)]
    lens = [min(int(t), a.max_frames) for t in reference_length_histogram(a.clips, seed=0)]
    g = torch.Generator().manual_seed(1)
    xs = torch.zeros(a.clips, max(lens), model.adim)
    for c, t in enumerate(lens):
        xs[c, :t] = torch.randn(t, model.adim, generator=g)
    xs = xs.to(dev)
    rows = []
    for with_lm in [int(v) for v in a.lm.split(",")]:
        bs = get_beam_search_decoder(model, tokens, rnnlm=lm if with_lm else None, ctc_weight=0.1, lm_weight=0.3 if with_lm else 0.0, beam_size=40)
        positions = {}

        def sequential():
            positions["seq"] = sum(max(len(h.yseq) for h in bs.forward(xs[c, : lens[c]])) - 1 for c in range(a.clips))

        med, lo, hi = _timed(sequential, a.reps)
        ops.start_event_timing()
        sequential()
        torch.cuda.synchronize()
        launches = sum(v.get("launches", 0) for v in ops.stop_event_timing().values())
        rows.append(dict(path="forward, clip after clip", lm=bool(with_lm), C=1, clips=a.clips, seconds_median=round(med, 4), seconds_min=round(lo, 4),
                         seconds_max=round(hi, 4), clips_per_s=round(a.clips / med, 2), hip_launches_per_position=round(launches / positions["seq"], 1)))
        print(json.dumps(rows[-1]), flush=True)
        for C in [int(v) for v in a.groups.split(",")]:
            def batched():
                n = 0
                for c0 in range(0, a.clips, C):
                    ls = lens[c0 : c0 + C]
                    out = bs.forward_clips(xs[c0 : c0 + C, : max(ls)], ls)
                    n += max(len(h.yseq) for nb in out for h in nb) - 1
                positions["clips"] = n

            med, lo, hi = _timed(batched, a.reps)
            ops.start_event_timing()
            batched()
            torch.cuda.synchronize()
            launches = sum(v.get("launches", 0) for v in ops.stop_event_timing().values())
            rows.append(dict(path="forward_clips", lm=bool(with_lm), C=C, clips=a.clips, seconds_median=round(med, 4), seconds_min=round(lo, 4),
                             seconds_max=round(hi, 4), clips_per_s=round(a.clips / med, 2),
                             hip_launches_per_position=round(launches / positions["clips"], 1)))
            print(json.dumps(rows[-1]), flush=True)
    out = dict(what="LRS beam search, clips per second: forward per clip vs forward_clips", device=torch.cuda.get_device_name(0), beam=40, ctc_weight=0.1,
               vocab=VOCAB, lengths=lens, reps=a.reps, note="hip_launches_per_position counts this library's launches only (torch glue is not in it)",
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
