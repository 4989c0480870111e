"""Golden vectors for the WHOLE DC-TCN model in TRAINING mode (DCTCNLightningModule.loss_and_grads).  RUNS ONLY WHERE THE REFERENCE TREE IS
PRESENT: imports the reference's own `tcn.model.Lipreading`, loads the seeded weights of tests/dctcn_whole_restatement.whole_case with
strict=True, puts the whole module in .train() in fp64 (batch statistics in BatchNorm3d, every BatchNorm2d and every BatchNorm1d), swaps every
nn.Dropout of the dense layers for a multiply by syncvsr_amd.dropout.keep_mask (the counter-based mask the kernels generate) and applies
lightning.py:264-299 (mixup of the clips and of the two losses) around it.  NUMBERS ONLY are stored.

    python tests/golden/make_golden_dctcn_whole.py

Per run `r` (plain: no dropout, lam 0; mix: dropout seed 5, lam 0.3) of the tiny configuration at B = 2, T = 7, 40 x 40, in
tests/golden/dctcn_whole_train_tiny.npz: `{r}.loss_*` fp64, `{r}.stat.{norm}.running_mean / running_var` (GOLD_STATS: the stem's norm and
one trunk norm) and `{r}.grad.{name}` (GOLD_GRADS, flattened, about a thousand evenly spaced elements: `sub`).  The script asserts that the
fp64 restatement (tests/dctcn_whole_restatement.py) reproduces all of it to 1e-9, the bound make_golden_dctcn_train.py applies."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from dctcn_cases import rel_err  # noqa: E402
import dctcn_whole_restatement as WR  # noqa: E402
from make_golden_dctcn_train import MaskDrop  # noqa: E402
from make_golden_lrw import REF  # noqa: E402
from syncvsr_amd import dropout  # noqa: E402


def reference_run(cfg, dims, sd, batch, seed, lam):
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from tcn.model import Lipreading

    videos, tokens, labels, word_mask, attention_mask = batch
    model = Lipreading(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in cfg.model.dctcn.items()})
    classifier = model.tcn.tcn_output                                  # lightning.py:238-239
    model.tcn.consensus_func = lambda x, lengths, B: x
    model.tcn.tcn_output = nn.Identity()
    C = dims["out_size"]
    audio = nn.Linear(C, dims["A"] * dims["G"] * dims["V"])

    class Whole(nn.Module):
        def __init__(self):
            super().__init__()
            self.model, self.video_classifier, self.audio_projection = model, classifier, audio

    whole = Whole()
    missing, unexpected = whole.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    whole = whole.double().train()
    o = cfg.model.dctcn.densetcn_options
    sites = dropout.dctcn_sites(cfg)
    feats = whole.model.tcn.tcn_trunk.features
    for bi, nl in enumerate(dims["blocks"]):
        for li in range(nl):
            layer = getattr(getattr(feats, f"denseblock{bi + 1}"), f"denselayer{li + 1}")
            for s in (0, 1):
                site = sites[f"block{bi + 1}.layer{li + 1}.drop{s}"]
                setattr(layer, f"dropout{s}", nn.Identity() if seed is None else MaskDrop(seed, site, float(o.dropout)))
    v = videos.double()
    if lam:
        v = torch.lerp(v, v.roll(1, 0), lam)                           # lightning.py:264-267 (word boundaries are not mixed)
    h = whole.model(v, lengths=None, boundaries=word_mask.double().unsqueeze(2))
    am = attention_mask.double()
    logits_c = whole.video_classifier((h * am.unsqueeze(1)).sum(2) / (am.sum(1, keepdim=True) + 1e-6))
    T = videos.size(2)
    tok = tokens[:, : T * dims["A"]]
    la = whole.audio_projection(h.transpose(1, 2)).unflatten(2, (-1, dims["V"])).flatten(0, 2)
    loss_c = torch.lerp(F.cross_entropy(logits_c, labels), F.cross_entropy(logits_c, labels.roll(1, 0)), lam)
    loss_a = torch.lerp(F.cross_entropy(la, tok.flatten()), F.cross_entropy(la, tok.roll(1, 0).flatten()), lam)
    total = loss_c + loss_a * float(cfg.optim.lambda_audio)
    total.backward()
    params = dict(whole.named_parameters())
    grads = {n: (params[n].grad if params[n].grad is not None else torch.zeros_like(params[n])).detach() for n in WR.GOLD_GRADS}
    bufs = {k: v.detach() for k, v in whole.named_buffers()}
    return dict(loss_total=total.detach(), loss_category=loss_c.detach(), loss_audio=loss_a.detach(), grads=grads, bufs=bufs)


def run() -> None:
    store = {}
    cfg, dims, sd, batch = WR.whole_case(2)
    lam_a = float(cfg.optim.lambda_audio)
    for r, kw in WR.RUNS.items():
        ref = reference_run(cfg, dims, sd, batch, **kw)
        out, grads, _, new_stats = WR.whole_grads(cfg, dims, sd, batch, lam_a, None, **kw)
        for k in ("loss_total", "loss_category", "loss_audio"):
            assert rel_err(out[k], ref[k]) < 1e-9, (r, k)
            store[f"{r}.{k}"] = np.float64(ref[k])
        for bn in WR.GOLD_STATS:
            for b in ("running_mean", "running_var"):
                assert rel_err(new_stats[f"{bn}.{b}"], ref["bufs"][f"{bn}.{b}"]) < 1e-9, (r, bn, b)
                store[f"{r}.stat.{bn}.{b}"] = ref["bufs"][f"{bn}.{b}"].numpy()
            assert int(ref["bufs"][f"{bn}.num_batches_tracked"]) == 1
        for n in WR.GOLD_GRADS:
            e = rel_err(grads[n], ref["grads"][n])
            assert e < 1e-9, (r, n, e)
            store[f"{r}.grad.{n}"] = WR.sub(ref["grads"][n])
        print(f"{r}: losses {float(ref['loss_total']):.6f} {float(ref['loss_category']):.6f} {float(ref['loss_audio']):.6f}")
    path = os.path.join(HERE, "dctcn_whole_train_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    run()
