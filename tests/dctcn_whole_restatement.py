"""fp64 torch restatement of the WHOLE DC-TCN model in the reference's training arithmetic: tests/dctcn_train_restatement.py (the back-end
and the heads under .train(), lightning.py:264-299 around them) with the front-end under autograd on BATCH statistics as well — BatchNorm3d
of the stem and every BatchNorm2d of the Swish ResNet18 normalise with the batch's biased variance and update their running buffers
(momentum 0.1, unbiased variance).  What DCTCNLightningModule.loss_and_grads computes.

`round_to` rounds what the device stores in bf16, at the points tests/dctcn_restatement.frontend and dctcn_train_restatement.backend_train
round; the statistics are taken over the rounded convolution outputs (the device sums the bf16 tensor it stored).

    python -m tests.dctcn_whole_restatement --write      # measures the bf16 floor of every tensor class into profiles/dctcn_step.json"""
from __future__ import annotations

import json
import os
import sys

import torch
import torch.nn.functional as F

try:
    import dctcn_restatement as R
    import dctcn_train_restatement as TR
    from dctcn_backward_ref import backend_names, rel_l2
except ImportError:          # run as `python -m tests.dctcn_whole_restatement`
    from tests import dctcn_restatement as R
    from tests import dctcn_train_restatement as TR
    from tests.dctcn_backward_ref import backend_names, rel_l2

from syncvsr_amd.dctcn_init import dctcn_dims, dctcn_init_state_dict, dctcn_synthetic_batch, tiny_dctcn_config

BN_EPS, MOMENTUM = R.BN_EPS, 0.1
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dctcn_step.json")

# what tests/golden/make_golden_dctcn_whole.py records (tests/golden/dctcn_whole_train_tiny.npz) and tests/test_dctcn_whole_cpu.py reads back
RUNS = {"plain": dict(seed=None, lam=0.0), "mix": dict(seed=5, lam=0.3)}
TR_L = "model.trunk.layer"
GOLD_STATS = ("model.frontend3D.1", f"{TR_L}2.0.bn1")
GOLD_GRADS = ("model.frontend3D.0.weight", f"{TR_L}1.0.conv1.weight", f"{TR_L}2.0.downsample.0.weight", "model.frontend3D.1.weight",
              f"{TR_L}1.0.bn1.weight", f"{TR_L}2.0.bn2.weight", f"{TR_L}3.1.bn1.weight", f"{TR_L}4.0.downsample.1.weight",
              f"{R.TCN}.transition0.conv.weight", f"{R.TCN}.transition0.norm.weight", f"{R.TCN}.transition0.prelu.weight",
              "video_classifier.weight", "video_classifier.bias", "audio_projection.weight", "audio_projection.bias")
sub = TR.sub


def whole_case(B: int = 2, T: int = 7, size: int = 40):
    """The tiny configuration (word boundaries on) with B clips of T frames: -> (cfg, dims, state dict, batch)."""
    cfg = tiny_dctcn_config(True)
    sd = dctcn_init_state_dict(cfg, seed=6)
    batch = dctcn_synthetic_batch(cfg, B, T, size=size, seed=40 + B, lengths=[7, 4, 5, 6][:B])
    return cfg, dctcn_dims(cfg), sd, batch


def frontend_names(sd: dict) -> dict:
    """{parameter name: class} of the front-end: "fe_conv" (the stem and trunk convolutions) or "fe_bn" (BatchNorm weights and biases)."""
    return {n: ("fe_conv" if v.dim() >= 2 else "fe_bn") for n, v in sd.items()
            if n.startswith(("model.frontend3D", "model.trunk")) and v.is_floating_point() and "running_" not in n}


def _bn_batch(x, W, p, new_stats: dict):
    """BatchNorm2d / 3d in training mode on x [N, C, ...]."""
    dims = [i for i in range(x.dim()) if i != 1]
    n = x.numel() // x.size(1)
    mean, var = x.mean(dims), x.var(dims, unbiased=False)
    with torch.no_grad():
        new_stats[f"{p}.running_mean"] = (1 - MOMENTUM) * W[f"{p}.running_mean"] + MOMENTUM * mean
        new_stats[f"{p}.running_var"] = (1 - MOMENTUM) * W[f"{p}.running_var"] + MOMENTUM * var * n / (n - 1)
    shape = [1, -1] + [1] * (x.dim() - 2)
    return (x - mean.view(shape)) / torch.sqrt(var.view(shape) + BN_EPS) * W[f"{p}.weight"].view(shape) + W[f"{p}.bias"].view(shape)


def frontend_train(W: dict, videos: torch.Tensor, rnd, new_stats: dict) -> torch.Tensor:
    """tests/dctcn_restatement.frontend with every BatchNorm on batch statistics: videos [B,1,T,H,W] -> [B,T,512]."""
    B, _, T = videos.shape[:3]
    h = rnd(F.conv3d(rnd(videos.double()), W["model.frontend3D.0.weight"], None, stride=(1, 2, 2), padding=(2, 3, 3)))
    h = R._swish(_bn_batch(h, W, "model.frontend3D.1", new_stats))
    h = rnd(F.max_pool3d(h, (1, 3, 3), (1, 2, 2), (0, 1, 1)))
    h = h.transpose(1, 2).reshape(B * T, 64, h.size(3), h.size(4))
    for li in range(1, 5):
        for bi in range(2):
            p = f"model.trunk.layer{li}.{bi}"
            stride = 2 if (bi == 0 and li > 1) else 1
            o = rnd(F.conv2d(h, W[f"{p}.conv1.weight"], None, stride=stride, padding=1))
            o = rnd(R._swish(_bn_batch(o, W, f"{p}.bn1", new_stats)))
            o = rnd(F.conv2d(o, W[f"{p}.conv2.weight"], None, stride=1, padding=1))
            if f"{p}.downsample.0.weight" in W:
                r = rnd(F.conv2d(h, W[f"{p}.downsample.0.weight"], None, stride=stride))
                r = rnd(_bn_batch(r, W, f"{p}.downsample.1", new_stats))
            else:
                r = h
            h = rnd(R._swish(_bn_batch(o, W, f"{p}.bn2", new_stats) + r))
    return rnd(h.mean((2, 3))).view(B, T, 512)


def whole_forward(cfg, dims, W: dict, batch, lambda_audio: float, rnd, seed=None, lam: float = 0.0, new_stats: dict | None = None):
    """-> (losses and last_hidden_states, the features [B, T, 512] as a graph node)."""
    videos, tokens, labels, word_mask, attention_mask = batch
    new_stats = {} if new_stats is None else new_stats
    v = torch.lerp(videos.double(), videos.double().roll(1, 0), lam) if lam else videos.double()          # (word boundaries are not mixed)
    feats = frontend_train(W, v, rnd, new_stats)
    x = torch.cat([feats, word_mask.double().unsqueeze(2)], dim=-1) if dims["in_size"] == 513 else feats
    h = TR.backend_train(W, dims, x, rnd, new_stats, TR.drop_of(cfg, seed))
    return TR.heads_mix(W, dims, h, tokens, labels, attention_mask, lambda_audio, rnd, lam), feats


def _rnd(round_to):
    rnd = (lambda t: t) if round_to is None else (lambda t: t.to(round_to).double())
    if round_to is not None:
        rnd.f32 = lambda t: t.float().double()
    return rnd


def whole_grads(cfg, dims, sd, batch, lambda_audio: float, round_to, seed=None, lam: float = 0.0, loss_scale: float = 1.0):
    """-> (losses and last_hidden_states, {name: fp64 gradient} of EVERY parameter, grad_features fp64 [B*T, 512], the BatchNorm buffers
    after the step: running_mean / running_var of every norm, front-end included)."""
    rnd = _rnd(round_to)
    names = [n for n, v in sd.items() if v.is_floating_point() and "running_" not in n]
    with torch.no_grad():
        W = R._weights(sd, rnd)
    for n in names:
        W[n] = W[n].clone().requires_grad_(True)
    new_stats: dict = {}
    out, feats = whole_forward(cfg, dims, W, batch, lambda_audio, rnd, seed, lam, new_stats)
    feats.retain_grad()
    (out["loss_total"] * loss_scale).backward()
    grads = {n: (W[n].grad.detach() if W[n].grad is not None else torch.zeros_like(W[n])) for n in names}
    return {k: v.detach() for k, v in out.items()}, grads, feats.grad.detach().reshape(-1, 512), new_stats


def eval_forward(cfg, dims, sd, batch, lambda_audio: float, round_to):
    """The eval forward of tests/dctcn_restatement.py on a state dict (the stepped weights and running statistics of a training run)."""
    return R.dctcn_forward(sd, dims, *batch, lambda_audio=lambda_audio, round_to=round_to)


# ----------------------------------------------------------------------------------------------------
# the bf16 floor of the front-end's gradients, for the classes no existing bound fits
# ----------------------------------------------------------------------------------------------------
FLOOR_RUNS = (dict(seed=None, lam=0.0), dict(seed=5, lam=0.0), dict(seed=None, lam=0.3), dict(seed=5, lam=0.3))


def classes(cfg, sd) -> dict:
    out = dict(backend_names(cfg))
    out.update(frontend_names(sd))
    return out


def cos_ratio(a, b) -> tuple:
    """(cosine, norm ratio |a| / |b|) of two tensors."""
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300)), float(a.norm() / (b.norm() + 1e-300))


def measure_floor(B: int):
    """-> ({class: the largest relative L2 distance of any one tensor}, loss, running statistic, {front-end class: (the smallest cosine, the
    largest |norm ratio - 1|) of any one tensor}): the restatement with its bf16 rounding points against its float64 run on the same inputs,
    over FLOOR_RUNS."""
    cfg, dims, sd, batch = whole_case(B)
    lam_a = float(cfg.optim.lambda_audio)
    cls = classes(cfg, sd)
    floor, loss, stat = {c: 0.0 for c in set(cls.values()) | {"grad_features"}}, 0.0, 0.0
    shape = {c: [1.0, 0.0] for c in ("fe_conv", "fe_bn")}
    for run in FLOOR_RUNS:
        oa, ga, fa, sa = whole_grads(cfg, dims, sd, batch, lam_a, torch.bfloat16, **run)
        ob, gb, fb, sb = whole_grads(cfg, dims, sd, batch, lam_a, None, **run)
        for n, c in cls.items():
            if not n.endswith(".net.0.bias"):
                floor[c] = max(floor[c], rel_l2(ga[n], gb[n]))
                if c in shape:
                    cs, ratio = cos_ratio(ga[n], gb[n])
                    shape[c] = [min(shape[c][0], cs), max(shape[c][1], abs(ratio - 1.0))]
        floor["grad_features"] = max(floor["grad_features"], rel_l2(fa, fb))
        loss = max([loss] + [abs(float(oa[k]) - float(ob[k])) / abs(float(ob[k])) for k in ("loss_total", "loss_category", "loss_audio")])
        stat = max([stat] + [rel_l2(sa[k], sb[k]) for k in sa])
    return floor, loss, stat, shape


def recorded_floor(B: int) -> dict:
    """{class: floor, "loss": ., "stat": ., "shape": {front-end class: [smallest cosine, largest |norm ratio - 1|]}}"""
    with open(PROFILE) as f:
        doc = json.load(f)["bf16_floor"][f"b{B}"]
    return dict(doc["classes"], loss=doc["loss"], stat=doc["stat"], shape=doc["shape"])


if __name__ == "__main__":
    measured = {f"b{B}": measure_floor(B) for B in (2, 3)}
    print(json.dumps(measured, indent=1))
    if "--write" in sys.argv:
        doc = {}
        if os.path.exists(PROFILE):
            with open(PROFILE) as f:
                doc = json.load(f)
        doc["bf16_floor"] = {k: dict(classes=m[0], loss=m[1], stat=m[2], shape=m[3]) for k, m in measured.items()}
        doc["bf16_floor_note"] = ("whole-model training of the tiny configuration (tests/dctcn_whole_restatement.whole_case, B = 2 and 3, T = 7, "
                                  "40 x 40): per class the largest relative L2 distance of one tensor's gradient, the largest relative deviation "
                                  "of a loss, the largest relative L2 distance of an updated running statistic and, for the front-end's two classes (shape), "
                                  "the smallest cosine and the largest |norm ratio - 1| of one tensor's gradient, between the restatement with "
                                  "its bf16 rounding points and its float64 run on the same inputs, over (seed, lam) in {None, 5} x {0, 0.3} "
                                  "(python -m tests.dctcn_whole_restatement --write)")
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
