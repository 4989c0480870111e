"""Microseconds per search step of the recurrent language-model scorer (syncvsr_amd/lrs_lm.py RNNLM) at beam 40 x {1, 8} clips, unit 650,
2 layers, 5,000 vocabulary units, beside torch-eager nn.LSTMCell stacks driven the way the reference drives them (lm/default.py:168-213: the
per-hypothesis dict-of-lists state is re-stacked before every step and taken apart after it) on the same GPU; and the tolerance
measurement of tests/test_gpu_rnnlm.py: the error of the float64 restatement with bf16-rounded weights and contraction inputs against the
recorded fp32-weight reference (tests/golden/lrs_rnnlm_tiny.npz), on the host.

    python scripts/rnnlm_bench.py [--beam 40] [--clips 1,8] [--iters 50] [--out profiles/rnnlm.json]

A step = select_states(prev) + batch_score(ys, state): wall-clock between device synchronisations (host dispatch included: that is what a
search pays), median of `--iters` steps after 10 warm-up steps.  The times are reported, not gated.  Prints one JSON line and writes --out.
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

LM_ARGS = dict(type="lstm", layer=2, unit=650, embed_unit=None, tie_weights=False)
VOCAB = 5000


def tolerance_measurement() -> dict:
    from rnnlm_cases import RNNLM_CASES, load_golden, rnnlm_state_dict
    from rnnlm_restatement import RNNLMRestatement

    gold, out = load_golden(), {}
    for case, (conf, seed) in RNNLM_CASES.items():
        lp, h, c = RNNLMRestatement(rnnlm_state_dict(conf, seed), conf, bf16_weights=True, bf16_inputs=True).run(gold[f"{case}.tok"], gold[f"{case}.prev"])
        m = dict(logp_abs=float(np.abs(lp - gold[f"{case}.logp"]).max()), h_abs=float(np.abs(h - gold[f"{case}.h"]).max()))
        if c is not None:
            m["c_abs"] = float(np.abs(c - gold[f"{case}.c"]).max())
        m["state_bound"] = {k[:-4]: 2.0 * v for k, v in m.items() if k in ("h_abs", "c_abs")}
        out[case] = m
    return dict(what="float64 restatement, weights and contraction inputs rounded to bf16, against the recorded fp32-weight reference over the "
                     "recorded steps (max abs); the tests bound the states by twice this and the log-probabilities by abs 0.1 / relative 1e-2",
                cases=out)


class EagerReferenceLM(torch.nn.Module):
    """nn.Embedding -> nn.LSTMCell stack -> nn.Linear -> log_softmax with the reference's batch_score state handling."""

    def __init__(self, V: int, layers: int, U: int):
        super().__init__()
        self.embed = torch.nn.Embedding(V, U)
        self.rnn = torch.nn.ModuleList([torch.nn.LSTMCell(U, U) for _ in range(layers)])
        self.lo = torch.nn.Linear(U, V)
        self.layers, self.U = layers, U

    @torch.no_grad()
    def batch_score(self, ys, states):
        n = len(ys)
        if states[0] is None:
            z = torch.zeros(n, self.U, device=ys.device)
            st = {"c": [z] * self.layers, "h": [z] * self.layers}
        else:
            st = {k: [torch.stack([states[b][k][i] for b in range(n)]) for i in range(self.layers)] for k in ("c", "h")}
        x = self.embed(ys[:, -1])
        h, c = [None] * self.layers, [None] * self.layers
        for i in range(self.layers):
            h[i], c[i] = self.rnn[i](x, (st["h"][i], st["c"][i]))
            x = h[i]
        logp = torch.log_softmax(self.lo(x), dim=1)
        return logp, [{"c": [c[i][b] for i in range(self.layers)], "h": [h[i][b] for i in range(self.layers)]} for b in range(n)]


def _median_us(step, iters: int, warmup: int = 10) -> float:
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam", type=int, default=40)
    ap.add_argument("--clips", default="1,8")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnlm.json"))
    a = ap.parse_args()
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_lm import RNNLM

    dev = torch.device("cuda:0")
    lm = RNNLM(VOCAB, LM_ARGS).to(dev)
    eager = EagerReferenceLM(VOCAB, LM_ARGS["layer"], LM_ARGS["unit"]).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    res = dict(device=torch.cuda.get_device_name(0), lm=dict(LM_ARGS, vocab=VOCAB, unit_pad=lm.unit_pad), beam=a.beam, iters=a.iters, steps=[])
    for clips in (int(c) for c in a.clips.split(",")):
        n = a.beam * clips
        ys = torch.randint(1, VOCAB - 1, (n, 12), generator=g).to(dev)
        prev = torch.randint(0, n, (n,), generator=g).to(dev)
        lm.beam_hint = a.beam
        box = {"s": lm.batch_score(ys, lm.batch_init_state_clips(torch.zeros(clips, 4, 8, device=dev), [4] * clips), None)[1]}

        def hip_step():
            box["s"] = lm.batch_score(ys, lm.select_states(box["s"], prev, None), None)[1]

        n0 = ops._ENQUEUED
        hip_step()
        launches = ops._ENQUEUED - n0
        ebox = {"s": eager.batch_score(ys, [None] * n)[1]}
        plist = prev.tolist()

        def eager_step():
            ebox["s"] = eager.batch_score(ys, [ebox["s"][p] for p in plist])[1]

        hip, ref = _median_us(hip_step, a.iters), _median_us(eager_step, a.iters)
        res["steps"].append(dict(clips=clips, rows=n, hip_us=round(hip, 1), torch_eager_us=round(ref, 1), library_launches=launches,
                                 state_bytes=lm.workspace_bytes(n)))
    res["tolerance"] = tolerance_measurement()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
