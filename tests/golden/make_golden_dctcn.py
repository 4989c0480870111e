"""Golden vectors for the DC-TCN word-level model (syncvsr_amd/dctcn.py).  RUNS ONLY WHERE THE REFERENCE TREE IS PRESENT: imports the
reference's own `tcn.model.Lipreading` (pure torch), loads the seeded weights of tests/dctcn_cases.py with strict=True, applies
lightning.py:238-239 (classifier moved out, identity consensus) and :268-312 (masked mean, the two heads, the five metrics; lam = 0 in
eval) around it in fp64, and stores NUMBERS ONLY; weights are regenerated from the seed.

    python tests/golden/make_golden_dctcn.py [dctcn_tiny] [dctcn_full]

Per sub-case `tag` of a file: `{tag}.state_keys` / `{tag}.state_shapes` (the reference module's own state dict plus the two heads),
`{tag}.last_hidden_states` fp32 [B, C, T], `{tag}.logits_category` fp64, `{tag}.logits_audio` fp32 (rows dctcn_cases.audio_rows(B, T) only),
the five metrics in fp64, and for the tiny sub-case nowb_t7 `{tag}.transition0` / `{tag}.denseblock{i}` (fp32).  fp32 storage of the large tensors is
exact to 6e-8 relative: three decimal orders below anything compared against them.

The script ASSERTS that a case is not vacuous: (a) the fp64 restatement (tests/dctcn_restatement.py) matches the reference to 1e-9;
(b) removing the gates, or the dilation, from the restatement moves last_hidden_states by more than ten times the bf16 floor (the
deviation of the restatement's round_to=bfloat16 mode from its fp64 mode); (c) at least three quarters of the clips have a top-1 / top-2
logit gap above ten times the absolute bf16 floor of the logits (largest absolute deviation of the bf16 mode); (d) every label's top-1
and top-5 membership holds by that margin too, and 0 < accuracy_top1 < accuracy_top5 (labels: tests/dctcn_cases.py)."""
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

from dctcn_cases import DCTCN_CASES, audio_rows, dctcn_subcase, rel_err  # noqa: E402
from dctcn_restatement import dctcn_forward  # noqa: E402
from make_golden_lrw import REF  # noqa: E402


def reference_forward(cfg, dims, sd, batch) -> dict:
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
    whole = whole.eval().double()
    out = {"state_keys": np.array(list(whole.state_dict().keys())),
           "state_shapes": np.array([",".join(str(d) for d in v.shape) for v in whole.state_dict().values()])}
    keep = {}
    feats = whole.model.tcn.tcn_trunk.features
    hooks = [getattr(feats, n).register_forward_hook(lambda m, i, o, n=n: keep.__setitem__(n, o.detach()))
             for n in ["transition0"] + [f"denseblock{i + 1}" for i in range(len(dims["blocks"]))]]
    with torch.no_grad():
        h = whole.model(videos.double(), lengths=None, boundaries=word_mask.double().unsqueeze(2))            # lightning.py:268-276, lam = 0
        am = attention_mask.double()
        logits_c = (h * am.unsqueeze(1)).sum(2)
        logits_c = whole.video_classifier(logits_c / (am.sum(1, keepdim=True) + 1e-6))
        loss_c = F.cross_entropy(logits_c, labels)
        tok = tokens[:, : videos.size(2) * dims["A"]]
        logits_a = whole.audio_projection(h.transpose(1, 2))
        loss_a = F.cross_entropy(logits_a.unflatten(2, (-1, dims["V"])).flatten(0, 2), tok.flatten())
        pred = logits_c.topk(5, dim=-1)[1] == labels.unsqueeze(1)
    for hk in hooks:
        hk.remove()
    lam_a = float(cfg.optim.lambda_audio)
    out.update(last_hidden_states=h, logits_category=logits_c, logits_audio=logits_a, loss_category=loss_c, loss_audio=loss_a,
               loss_total=loss_c + loss_a * lam_a, accuracy_top1=pred[:, 0].double().mean(), accuracy_top5=pred.double().amax(1).mean(), **keep)
    return out


def run(name: str) -> None:
    store = {}
    for tag, *_ in DCTCN_CASES[name]:
        cfg, dims, sd, batch = dctcn_subcase(name, tag)
        ref = reference_forward(cfg, dims, sd, batch)
        lam_a = float(cfg.optim.lambda_audio)
        keep = {}
        r64 = dctcn_forward(sd, dims, *batch, lambda_audio=lam_a, keep=keep)
        for k in ("last_hidden_states", "logits_category", "logits_audio", "loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5"):
            e = rel_err(r64[k], ref[k])
            assert e < 1e-9, (tag, k, e)                                                        # (a)
        for k, v in keep.items():
            assert rel_err(v, ref[k]) < 1e-9, (tag, k)
        r16 = dctcn_forward(sd, dims, *batch, lambda_audio=lam_a, round_to=torch.bfloat16)
        floor = rel_err(r16["last_hidden_states"], ref["last_hidden_states"])
        for what in ("no_gate", "no_dilation"):                                               # (b)
            moved = rel_err(dctcn_forward(sd, dims, *batch, lambda_audio=lam_a, **{what: True})["last_hidden_states"], ref["last_hidden_states"])
            assert moved > 10 * floor, (tag, what, moved, floor)
            print(f"{name}/{tag}: {what} moves last_hidden_states by {moved:.3e} (bf16 floor {floor:.3e})")
        afloor = float((r16["logits_category"] - ref["logits_category"]).abs().max())         # (c)
        top2 = ref["logits_category"].topk(2, dim=-1)[0]
        gaps = (top2[:, 0] - top2[:, 1])
        clear = int((gaps > 10 * afloor).sum())
        print(f"{name}/{tag}: top-1/top-2 gaps {[round(float(g), 3) for g in gaps]}, absolute bf16 floor of the logits {afloor:.3e}: {clear}/{len(gaps)} clear")
        assert clear * 4 >= 3 * len(gaps), (tag, gaps, afloor)
        labels, lg = batch[2], ref["logits_category"]                                        # (d) the accuracies are neither trivial nor fragile
        for b in range(len(labels)):
            srt = lg[b].sort(descending=True)[0]
            l = lg[b, labels[b]]
            m1 = abs(l - (srt[1] if l >= srt[0] else srt[0]))
            m5 = abs(l - (srt[5] if l >= srt[4] else srt[4]))
            assert min(float(m1), float(m5)) > 10 * afloor, (tag, b, float(m1), float(m5), afloor)
        assert 0.0 < float(ref["accuracy_top1"]) < float(ref["accuracy_top5"]), (tag, ref["accuracy_top1"], ref["accuracy_top5"])
        B, C, T = ref["last_hidden_states"].shape
        la = ref["logits_audio"].reshape(B * T, -1)[audio_rows(B, T)]
        store[f"{tag}.state_keys"], store[f"{tag}.state_shapes"] = ref["state_keys"], ref["state_shapes"]
        store[f"{tag}.last_hidden_states"] = ref["last_hidden_states"].float().numpy()
        store[f"{tag}.logits_category"] = ref["logits_category"].numpy()
        store[f"{tag}.logits_audio"] = la.float().numpy()
        for k in ("loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5"):
            store[f"{tag}.{k}"] = np.float64(ref[k])
        if tag == "nowb_t7":                      # intermediate features of ONE tiny sub-case (the file stays within the size of the other goldens)
            for k in keep:
                store[f"{tag}.{k}"] = ref[k].float().numpy()
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for n in (sys.argv[1:] or list(DCTCN_CASES)):
        run(n)
