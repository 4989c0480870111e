"""fp64 torch restatement of the DC-TCN back-end in the reference's TRAINING arithmetic (tcn/models/densetcn.py under .train(), with
lightning.py:264-299 around it), the front-end frozen in eval statistics: what loss_and_backend_grads(train_stats=True) computes.

The fact everything here turns on: TemporalConvLayer is Conv1d(padding = (k - 1) d) -> BatchNorm1d -> Chomp1d(symmetric) -> Swish, so in
training mode a cbcr* BatchNorm takes its statistics over T + (k - 1) d positions a clip, computed from the zero-padded edge and chomped off
afterwards.  `stats="kept"` takes them over the T kept positions instead: the WRONG variant tests/test_dctcn_train_cpu.py pins the gap of.

Dropout is a multiply by syncvsr_amd.dropout.keep_mask (site per (layer, stage): dropout.dctcn_sites; element row * growth + channel of the
stage's [B*T, growth] output).  `round_to` rounds what the device stores in bf16, as tests/dctcn_restatement.py does; the accumulators the
statistics are taken over stay unrounded (fp32 on the device), norm5's are taken over the stored (rounded) stack.

    python -m tests.dctcn_train_restatement --write      # re-measures the bf16 floor of the gradients into profiles/dctcn_train.json"""
from __future__ import annotations

import json
import os
import sys

import torch
import torch.nn.functional as F

from syncvsr_amd import dropout
try:
    import dctcn_restatement as R
    from dctcn_backward_ref import CLASSES, backend_names, rel_l2
except ImportError:          # run as `python -m tests.dctcn_train_restatement`
    from tests import dctcn_restatement as R
    from tests.dctcn_backward_ref import CLASSES, backend_names, rel_l2

TCN, BN_EPS, MOMENTUM = R.TCN, R.BN_EPS, 0.1
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dctcn_train.json")


# what tests/golden/make_golden_dctcn_train.py records (tests/golden/dctcn_train_tiny.npz) and tests/test_dctcn_train_cpu.py reads back
RUNS = {"plain": dict(seed=None, lam=0.0), "mix": dict(seed=5, lam=0.3)}
ROWS = (0, 3, 6)          # time steps kept of last_hidden_states
L = f"{TCN}.denseblock1.denselayer"
STATS = (f"{TCN}.transition0.norm", f"{L}1.cbcr0_0.net.1", f"{L}3.cbcr0_2.net.1", f"{L}3.cbcr1_2.net.1", f"{TCN}.norm5")
GRADS = (f"{TCN}.transition0.conv.weight", f"{TCN}.transition0.prelu.weight", f"{L}1.cbcr0_se_1.fc.0.weight", f"{L}3.cbcr0_2.net.0.weight",
         f"{L}3.cbcr0_2.net.0.bias", f"{L}3.cbcr0_2.net.1.weight", f"{L}3.cbcr1_2.net.1.bias", f"{L}2.downsample.weight", f"{L}2.downsample.bias",
         f"{TCN}.denseblock2.denselayer1.cbcr1_1.net.0.weight", f"{TCN}.norm5.weight", "video_classifier.weight", "grad_features")


def sub(v):
    """About a thousand evenly spaced elements (tests/test_dctcn_train_cpu.py takes the same ones)."""
    v = v.flatten()
    return v[:: max(1, v.numel() // 997)].double().numpy()


def _bn_batch(x, W, p, new_stats: dict, conv_bias=None, stat_src=None):
    """BatchNorm1d in training mode on x [B, C, L]: biased variance over (B, L) for the normalisation; new_stats gets the buffers after the
    update (momentum 0.1, unbiased variance).  stat_src: the positions the statistics are taken over when they are not x's own."""
    src = x if stat_src is None else stat_src
    n = src.size(0) * src.size(2)
    mean, var = src.mean((0, 2)), src.var((0, 2), unbiased=False)
    with torch.no_grad():
        new_stats[f"{p}.running_mean"] = (1 - MOMENTUM) * W[f"{p}.running_mean"] + MOMENTUM * mean
        new_stats[f"{p}.running_var"] = (1 - MOMENTUM) * W[f"{p}.running_var"] + MOMENTUM * var * n / (n - 1)
    return (x - mean.view(1, -1, 1)) / torch.sqrt(var.view(1, -1, 1) + BN_EPS) * W[f"{p}.weight"].view(1, -1, 1) + W[f"{p}.bias"].view(1, -1, 1)


def _tconv_bn(x, W, c, k, d, new_stats, stats):
    """Conv1d(padding = (k - 1) d) -> BatchNorm1d(batch statistics) -> symmetric chomp (densetcn.py:25-36)."""
    full = F.conv1d(x, W[f"{c}.0.weight"], W[f"{c}.0.bias"], padding=(k - 1) * d, dilation=d)
    h = (k - 1) * d // 2
    kept = full[:, :, h: full.size(2) - h] if h else full
    if stats == "kept":
        return _bn_batch(kept, W, f"{c}.1", new_stats)
    y = _bn_batch(full, W, f"{c}.1", new_stats)
    return y[:, :, h: y.size(2) - h] if h else y


def _drop(x, drop, site):
    """x [B, G, T]; element (b * T + t) * G + c."""
    if drop is None or drop["p"] <= 0.0:
        return x
    B, G, T = x.shape
    keep = torch.from_numpy(dropout.keep_mask(drop["seed"], drop["sites"][site], drop["p"], B * T * G)).view(B, T, G).transpose(1, 2)
    return x * keep.to(x.dtype) / (1.0 - drop["p"])


def backend_train(W: dict, dims: dict, x: torch.Tensor, rnd, new_stats: dict, drop: dict | None = None, stats: str = "all",
                  keep: dict | None = None) -> torch.Tensor:
    """x [B, T, in_size] -> last_hidden_states [B, C, T] (densetcn.py:143-192 in training mode)."""
    x = x.transpose(1, 2)
    p = f"{TCN}.transition0"
    a = W[f"{p}.prelu.weight"].view(1, -1, 1)
    h = _bn_batch(F.conv1d(x, W[f"{p}.conv.weight"]), W, f"{p}.norm", new_stats)
    x = rnd(torch.where(h >= 0, h, a * h))
    ks, ds = dims["ks"], dims["ds"]
    for bi, nl in enumerate(dims["blocks"]):
        for li in range(nl):
            p = f"{TCN}.denseblock{bi + 1}.denselayer{li + 1}"
            d = ds[li % len(ds)]
            outs = []
            for ki, k in enumerate(ks):
                y = x.mean(2)
                y = torch.sigmoid(R._swish(y @ W[f"{p}.cbcr0_se_{ki}.fc.0.weight"].T) @ W[f"{p}.cbcr0_se_{ki}.fc.2.weight"].T)
                y = getattr(rnd, "f32", lambda t: t)(y)
                outs.append(R._swish(_tconv_bn(rnd(x * y.unsqueeze(2)), W, f"{p}.cbcr0_{ki}.net", k, d, new_stats, stats)))
            o0 = rnd(_drop(torch.cat(outs, 1), drop, f"block{bi + 1}.layer{li + 1}.drop0"))
            if keep is not None:
                keep[f"b{bi + 1}l{li + 1}.out0"] = o0
            outs = [R._swish(_tconv_bn(o0, W, f"{p}.cbcr1_{ki}.net", k, d, new_stats, stats)) for ki, k in enumerate(ks)]
            o1 = _drop(torch.cat(outs, 1), drop, f"block{bi + 1}.layer{li + 1}.drop1")
            res = rnd(F.conv1d(x, W[f"{p}.downsample.weight"], W[f"{p}.downsample.bias"]))
            x = torch.cat([x, rnd(R._swish(o1 + res))], 1)
        if keep is not None:
            keep[f"denseblock{bi + 1}"] = x
        if bi != len(dims["blocks"]) - 1:
            p = f"{TCN}.transition{bi + 1}"
            x = rnd(R._swish(_bn_batch(F.conv1d(x, W[f"{p}.conv.weight"]), W, f"{p}.norm", new_stats)))
    return rnd(_bn_batch(x, W, f"{TCN}.norm5", new_stats))


def heads_mix(W: dict, dims: dict, h: torch.Tensor, tokens, labels, attention_mask, lambda_audio: float, rnd, lam: float) -> dict:
    """lightning.py:274-299.  h [B, C, T]."""
    B, C, T = h.shape
    am = attention_mask.double()
    pooled = rnd((h * am.unsqueeze(1)).sum(2) / (am.sum(1, keepdim=True) + 1e-6))
    logits_c = pooled @ W["video_classifier.weight"].T + W["video_classifier.bias"]
    logits_a = rnd(h.transpose(1, 2) @ W["audio_projection.weight"].T + W["audio_projection.bias"])
    tok = tokens[:, : T * dims["A"]]
    la = logits_a.unflatten(2, (-1, dims["V"])).flatten(0, 2)
    loss_c = torch.lerp(F.cross_entropy(logits_c, labels), F.cross_entropy(logits_c, labels.roll(1, 0)), lam)
    loss_a = torch.lerp(F.cross_entropy(la, tok.flatten()), F.cross_entropy(la, tok.roll(1, 0).flatten()), lam)
    return dict(loss_category=loss_c, loss_audio=loss_a, loss_total=loss_c + loss_a * lambda_audio, last_hidden_states=h)


def drop_of(cfg, seed) -> dict | None:
    if seed is None:
        return None
    return dict(seed=int(seed), p=float(cfg.model.dctcn.densetcn_options.dropout), sites=dropout.dctcn_sites(cfg))


def features(W: dict, videos, word_mask, dims, rnd, lam: float) -> torch.Tensor:
    """The frozen front-end (eval statistics) on the mixed clips -> fp64 [B, T, 512]."""
    with torch.no_grad():
        v = torch.lerp(videos.float(), videos.float().roll(1, 0), lam) if lam else videos
        return R.frontend(W, v, rnd)


def train_grads(cfg, dims, sd, batch, lambda_audio: float, round_to, seed=None, lam: float = 0.0, loss_scale: float = 1.0, stats: str = "all",
                keep: dict | None = None, feats=None):
    """-> (losses and last_hidden_states, {name: fp64 gradient}, grad_features fp64 [B*T, 512], the BatchNorm buffers after the step).
    feats [B, T, 512] (bf16-representable values): the front-end is skipped, as loss_and_backend_grads_from_features skips it; with lam they
    are the features of already-mixed clips and only the losses are mixed."""
    videos, tokens, labels, word_mask, attention_mask = batch
    rnd = (lambda t: t) if round_to is None else (lambda t: t.to(round_to).double())
    if round_to is not None:
        rnd.f32 = lambda t: t.float().double()
    names = backend_names(cfg)
    with torch.no_grad():
        W = R._weights(sd, rnd)
    feats = features(W, videos, word_mask, dims, rnd, lam) if feats is None else feats.double()
    for n in names:
        W[n] = W[n].clone().requires_grad_(True)
    feats = feats.clone().requires_grad_(True)
    x = torch.cat([feats, word_mask.double().unsqueeze(2)], dim=-1) if dims["in_size"] == 513 else feats
    new_stats: dict = {}
    h = backend_train(W, dims, x, rnd, new_stats, drop_of(cfg, seed), stats, keep)
    out = heads_mix(W, dims, h, tokens, labels, attention_mask, lambda_audio, rnd, lam)
    (out["loss_total"] * loss_scale).backward()
    grads = {n: (W[n].grad.detach() if W[n].grad is not None else torch.zeros_like(W[n])) for n in names}
    return {k: v.detach() for k, v in out.items()}, grads, feats.grad.detach().reshape(-1, 512), new_stats


FLOOR_RUNS = (dict(seed=None, lam=0.0), dict(seed=5, lam=0.0), dict(seed=5, lam=0.3))          # the runs tests/test_gpu_dctcn_train_model.py makes
FLOOR_TAGS = ("wb_t29", "nowb_t7")


def spread_features(tag: str, B: int, T: int) -> torch.Tensor:
    """bf16 [B, T, 512] N(0, 1) features for sub-case `tag`: what tests/test_gpu_dctcn_train_model.py drives
    loss_and_backend_grads_from_features with.  The random front-end on random 40 x 40 clips gives features whose spread over the rows is
    small against their size, and the batch mean subtraction then amplifies the bf16 rounding noise until the floor of a gradient is 0.1 .. 1;
    features with a spread of their own size keep it at 0.01 .. 0.04, where 4 x the floor is a bound a wrong gradient cannot meet."""
    g = torch.Generator().manual_seed(11 + T)
    return torch.randn(B, T, 512, generator=g).to(torch.bfloat16)


def measure_floor(tag: str, from_features: bool = False):
    """-> (per class the LARGEST relative L2 error of any one tensor, the largest relative deviation of a loss, the largest relative L2 error
    of a running statistic after the step): the bf16-rounded restatement against the fp64 one in training mode, over FLOOR_RUNS, on sub-case
    `tag` of the tiny configuration — from its videos, or (from_features) from spread_features.  Per sub-case, because the floor depends on
    how many positions a statistic is taken over and on the input's spread: batch statistics subtract a mean, which the rounding noise
    (relative to the values, not to their spread) does not shrink with."""
    try:
        from dctcn_cases import dctcn_subcase
    except ImportError:
        from tests.dctcn_cases import dctcn_subcase
    cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
    lam_a = float(cfg.optim.lambda_audio)
    feats = spread_features(tag, batch[0].shape[0], batch[0].shape[2]) if from_features else None
    floor, loss, stat = {c: 0.0 for c in CLASSES}, 0.0, 0.0
    for run in FLOOR_RUNS:
        oa, ga, fa, sa = train_grads(cfg, dims, sd, batch, lam_a, torch.bfloat16, feats=feats, **run)
        ob, gb, fb, sb = train_grads(cfg, dims, sd, batch, lam_a, None, feats=feats, **run)
        for n, c in backend_names(cfg).items():
            if not n.endswith(".net.0.bias"):          # (a cbcr* conv bias cancels: autograd leaves rounding noise around zero on both sides)
                floor[c] = max(floor[c], rel_l2(ga[n], gb[n]))
        floor["grad_features"] = max(floor["grad_features"], rel_l2(fa, fb))
        loss = max([loss] + [abs(float(oa[k]) - float(ob[k])) / abs(float(ob[k])) for k in ("loss_total", "loss_category", "loss_audio")])
        stat = max([stat] + [rel_l2(sa[k], sb[k]) for k in sa])
    return floor, loss, stat


def recorded_floor_doc() -> dict:
    with open(PROFILE) as f:
        return json.load(f)


def recorded_floor(tag: str, from_features: bool = False) -> dict:
    """{class: floor, "loss": ., "stat": .} of sub-case `tag`."""
    doc = recorded_floor_doc()["from_features" if from_features else "from_videos"]
    return dict(doc["bf16_floor"][tag], loss=doc["loss_floor"][tag], stat=doc["stat_floor"][tag])


if __name__ == "__main__":
    measured = {ff: {tag: measure_floor(tag, ff) for tag in FLOOR_TAGS} for ff in (False, True)}
    print(json.dumps({str(k): v for k, v in measured.items()}, indent=1))
    if "--write" in sys.argv:
        doc = {}
        if os.path.exists(PROFILE):
            with open(PROFILE) as f:
                doc = json.load(f)
        for k in ("bf16_floor", "loss_floor"):
            doc.pop(k, None)
        for ff, key in ((False, "from_videos"), (True, "from_features")):
            doc[key] = dict(bf16_floor={tag: m[0] for tag, m in measured[ff].items()}, loss_floor={tag: m[1] for tag, m in measured[ff].items()},
                            stat_floor={tag: m[2] for tag, m in measured[ff].items()})
        doc["bf16_floor_note"] = ("per sub-case of the tiny configuration: largest per-tensor relative L2 error of a class, largest relative "
                                  "deviation of a loss and largest relative L2 error of an updated running statistic; autograd of "
                                  "tests/dctcn_train_restatement.py with its bf16 rounding points against the same restatement in fp64, training "
                                  "mode, over the runs (no dropout, lam 0), (seed 5, lam 0), (seed 5, lam 0.3); from_videos: the sub-case's clips "
                                  "through the frozen front-end; from_features: N(0, 1) features (spread_features) "
                                  "(python -m tests.dctcn_train_restatement --write)")
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
