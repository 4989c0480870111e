"""Golden vectors for the DC-TCN back-end in TRAINING mode (loss_and_backend_grads(train_stats=True)).  RUNS ONLY WHERE THE REFERENCE TREE IS
PRESENT: imports the reference's own `tcn.models.densetcn.DenseTemporalConvNet`, puts it in .train() in fp64, swaps every nn.Dropout for a
multiply by syncvsr_amd.dropout.keep_mask (the counter-based mask the kernels generate), feeds it the frozen front-end's features
(tests/dctcn_restatement.frontend, eval statistics) of the mixed clips and applies lightning.py:274-299 around it.  NUMBERS ONLY are stored.

    python tests/golden/make_golden_dctcn_train.py

Per sub-case `tag` (wb_t29, nowb_t7 of dctcn_tiny) and run `r` (plain: no dropout, lam 0; mix: dropout seed 5, lam 0.3), in
tests/golden/dctcn_train_tiny.npz: `{tag}.{r}.loss_*` fp64, `{tag}.{r}.hidden` (last_hidden_states rows ROWS, channels ::7) fp64,
`{tag}.{r}.stat.{buffer}` (the updated running statistics of the norms in STATS) and `{tag}.{r}.grad.{name}` (GRADS, flattened, about a
thousand evenly spaced elements: `sub`).  The script asserts the fp64 restatement (tests/dctcn_train_restatement.py) reproduces all of it to 1e-9, and that the variant with
statistics over the T kept rows does not."""
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

from dctcn_cases import dctcn_subcase, rel_err  # noqa: E402
import dctcn_restatement as R  # noqa: E402
import dctcn_train_restatement as TR  # noqa: E402
from make_golden_lrw import REF  # noqa: E402
from syncvsr_amd import dropout  # noqa: E402

from dctcn_train_restatement import GRADS, ROWS, RUNS, STATS, TCN, sub  # noqa: E402


class MaskDrop(nn.Module):
    """nn.Dropout's place: x [B, G, T] times the counter-based mask of (seed, site), element (b * T + t) * G + c."""
    def __init__(self, seed, site, p):
        super().__init__()
        self.seed, self.site, self.p = seed, site, p

    def forward(self, x):
        B, G, T = x.shape
        keep = torch.from_numpy(dropout.keep_mask(self.seed, self.site, self.p, B * T * G)).view(B, T, G).transpose(1, 2)
        return x * keep.to(x.dtype) / (1.0 - self.p)


def reference_run(cfg, dims, sd, batch, seed, lam):
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from tcn.models.densetcn import DenseTemporalConvNet

    videos, tokens, labels, word_mask, attention_mask = batch
    o = cfg.model.dctcn.densetcn_options
    net = DenseTemporalConvNet(list(o.block_config), list(o.growth_rate_set), dims["in_size"], int(o.reduced_size), list(o.kernel_size_set),
                               list(o.dilation_size_set), dropout=float(o.dropout), relu_type="swish", squeeze_excitation=True)
    pre = "model.tcn.tcn_trunk."
    missing, unexpected = net.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    assert not missing and not unexpected
    net = net.double().train()
    sites = dropout.dctcn_sites(cfg)
    for bi, nl in enumerate(dims["blocks"]):
        for li in range(nl):
            layer = getattr(getattr(net.features, f"denseblock{bi + 1}"), f"denselayer{li + 1}")
            for s in (0, 1):
                site = sites[f"block{bi + 1}.layer{li + 1}.drop{s}"]
                setattr(layer, f"dropout{s}", nn.Identity() if seed is None else MaskDrop(seed, site, float(o.dropout)))
    C = dims["out_size"]
    cls, aud = nn.Linear(C, dims["classes"]).double(), nn.Linear(C, dims["A"] * dims["G"] * dims["V"]).double()
    with torch.no_grad():
        cls.weight.copy_(sd["video_classifier.weight"]); cls.bias.copy_(sd["video_classifier.bias"])
        aud.weight.copy_(sd["audio_projection.weight"]); aud.bias.copy_(sd["audio_projection.bias"])
    W = R._weights(sd, lambda t: t)
    feats = TR.features(W, videos, word_mask, dims, lambda t: t, lam).clone().requires_grad_(True)
    x = torch.cat([feats, word_mask.double().unsqueeze(2)], dim=-1) if dims["in_size"] == 513 else feats
    h = net(x.transpose(1, 2))                                                            # [B, C, T]
    am = attention_mask.double()
    logits_c = cls((h * am.unsqueeze(1)).sum(2) / (am.sum(1, keepdim=True) + 1e-6))
    T = videos.size(2)
    tok = tokens[:, : T * dims["A"]]
    la = aud(h.transpose(1, 2)).unflatten(2, (-1, dims["V"])).flatten(0, 2)
    loss_c = torch.lerp(F.cross_entropy(logits_c, labels), F.cross_entropy(logits_c, labels.roll(1, 0)), lam)
    loss_a = torch.lerp(F.cross_entropy(la, tok.flatten()), F.cross_entropy(la, tok.roll(1, 0).flatten()), lam)
    total = loss_c + loss_a * float(cfg.optim.lambda_audio)
    total.backward()
    params = {pre + k: v for k, v in net.named_parameters()}
    params.update({"video_classifier.weight": cls.weight})
    grads = {n: (feats.grad.reshape(-1, 512) if n == "grad_features" else
                 (params[n].grad if params[n].grad is not None else torch.zeros_like(params[n]))).detach() for n in GRADS}
    bufs = {pre + k: v.detach() for k, v in net.named_buffers()}
    return dict(loss_total=total.detach(), loss_category=loss_c.detach(), loss_audio=loss_a.detach(), hidden=h.detach(), grads=grads, bufs=bufs)


def run() -> None:
    store = {}
    for tag in ("wb_t29", "nowb_t7"):
        cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
        lam_a = float(cfg.optim.lambda_audio)
        for r, kw in RUNS.items():
            ref = reference_run(cfg, dims, sd, batch, **kw)
            out, grads, gf, new_stats = TR.train_grads(cfg, dims, sd, batch, lam_a, None, **kw)
            grads["grad_features"] = gf
            wrong, gwrong, gfw, _ = TR.train_grads(cfg, dims, sd, batch, lam_a, None, stats="kept", **kw)
            for k in ("loss_total", "loss_category", "loss_audio"):
                assert rel_err(out[k], ref[k]) < 1e-9, (tag, r, k)
                store[f"{tag}.{r}.{k}"] = np.float64(ref[k])
            assert rel_err(out["last_hidden_states"], ref["hidden"]) < 1e-9, (tag, r)
            moved = rel_err(wrong["last_hidden_states"], ref["hidden"])
            print(f"{tag}.{r}: statistics over the kept rows move last_hidden_states by {moved:.3e}")
            assert moved > 1e-2, (tag, r, moved)
            store[f"{tag}.{r}.hidden"] = ref["hidden"][:, ::7, list(t for t in ROWS if t < ref["hidden"].size(2))].numpy()
            for bn in STATS:
                for b in ("running_mean", "running_var"):
                    assert rel_err(new_stats[f"{bn}.{b}"], ref["bufs"][f"{bn}.{b}"]) < 1e-9, (tag, r, bn, b)
                    store[f"{tag}.{r}.stat.{bn}.{b}"] = ref["bufs"][f"{bn}.{b}"].numpy()
                assert int(ref["bufs"][f"{bn}.num_batches_tracked"]) == 1
            for n in GRADS:
                e = rel_err(grads[n], ref["grads"][n])
                tiny = max(float(ref["grads"][n].abs().max()), float(grads[n].abs().max())) < 1e-10          # (a cbcr* conv bias: rounding noise around 0)
                assert e < 1e-9 or tiny, (tag, r, n, e)
                store[f"{tag}.{r}.grad.{n}"] = sub(ref["grads"][n])
            print(f"{tag}.{r}: conv bias gradient of the reference: max |g| = {float(ref['grads'][GRADS[4]].abs().max()):.3e}")
    path = os.path.join(HERE, "dctcn_train_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    run()
