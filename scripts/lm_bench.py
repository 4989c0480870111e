"""Milliseconds per beam step of the language-model scorer (syncvsr_amd/lrs_lm.py) at beam 40 for prefixes of L tokens, beside the same
figure for the attention decoder's `DecoderScorer.batch_score` in the same process (its per-layer cost is the only comparable number the
package had before the LM), and the bytes a step moves for STATE: the row-table gather of the pooled cache against what a concatenated
per-layer cache [n, L, 3 * D] moves (gather by `prev` + concatenation of the new position).

    python scripts/lm_bench.py [--beam 40] [--lengths 10,50,100] [--iters 30] [--out profiles/round8_lm_step.json]

Times are wall-clock per `batch_score` call between device synchronisations (host dispatch included: that is what a search pays), median
of `--iters` calls after 5 warm-up calls.  Prints one JSON line and writes it to --out.
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


def _median_ms(fn, iters: int, warmup: int = 5) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam", type=int, default=40)
    ap.add_argument("--lengths", default="10,50,100")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round8_lm_step.json"))
    a = ap.parse_args()
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_init import default_lrs_args, lrs_init_state_dict
    from syncvsr_amd.lrs_lm import TransformerLM
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    n = a.beam
    lm = TransformerLM(VOCAB, LM_ARGS).to(dev)
    args = default_lrs_args()
    model = E2E(VOCAB, args)
    model.load_state_dict(lrs_init_state_dict(args, VOCAB, seed=0, perturb_norm=False), strict=True)
    model.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    T = 100
    enc = torch.randn(T, model.adim, generator=g).to(dev)
    xs = enc.unsqueeze(0).expand(n, T, model.adim)
    rows = []
    for L in [int(v) for v in a.lengths.split(",")]:
        ys = torch.randint(1, VOCAB - 1, (n, L), generator=g).to(dev)
        ys[:, 0] = VOCAB - 1
        prev = torch.randperm(n, generator=g).to(dev)
        # language model: the state after L - 1 positions, re-ordered as a search would; one step appends n rows per layer
        state = lm.batch_init_state(enc, beam=n, maxlen=L + a.iters + 8)
        _, st = lm.batch_score(ys[:, : L - 1][prev.argsort()], state, None)
        lm_ms = _median_ms(lambda: lm.batch_score(ys, lm.select_states(st, prev, ys[:, -1]), None), a.iters)
        ops.start_event_timing()
        lm.batch_score(ys, lm.select_states(st, prev, ys[:, -1]), None)
        torch.cuda.synchronize()
        ev = ops.stop_event_timing()
        att = ev.get("k_mha_table", {})
        # attention decoder: the same step on its concatenated cache
        _, dst = model.decoder.batch_score(ys[:, : L - 1][prev.argsort()], None, xs)
        dec_ms = _median_ms(lambda: model.decoder.batch_score(ys, model.decoder.select_states(dst, prev, ys[:, -1]), xs), a.iters)
        D = lm.att_unit
        rows.append(dict(
            L=L, beam=n, lm_step_ms=round(lm_ms, 3), lm_layers=lm.layers, lm_step_ms_per_layer=round(lm_ms / lm.layers, 4),
            decoder_step_ms=round(dec_ms, 3), decoder_layers=model.dlayers, decoder_step_ms_per_layer=round(dec_ms / model.dlayers, 4),
            table_attention_ms_all_layers=att.get("ms"), table_attention_launches=att.get("launches"),
            table_attention_gather_bytes_per_launch=n * lm.head * L * 256,
            lm_state_bytes_moved=n * (L - 1) * 4 + n * L * 4,                       # gather of the table by `prev` + the table with its new column
            concatenated_cache_bytes_moved=lm.layers * n * L * 3 * D * 2 * 2,       # per layer: gather [n, L-1, 3D] by `prev`, then re-concatenate [n, L, 3D] (read + write counted once each)
            pool_bytes_appended=lm.layers * n * 3 * D * 2))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(what="LM scorer beam step vs DecoderScorer.batch_score, same process", device=torch.cuda.get_device_name(0), lm_args=LM_ARGS,
               vocab=VOCAB, workspace_bytes_beam40_len100=lm.workspace_bytes(40, 100), iters=a.iters, rows=rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
