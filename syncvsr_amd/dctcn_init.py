"""Parameter inventory + deterministic initialisation for the DC-TCN word-level model (``DCTCNLightningModule``).

Names and shapes follow the reference state dict of ``LRW/video/src/lightning.py:226-253`` around ``tcn.model.Lipreading``
(``tcn/model.py:93-155``: ``model.frontend3D`` / ``model.trunk`` Swish ResNet18, ``model.tcn.tcn_trunk.features.*`` =
``tcn/models/densetcn.py:143-187``); ``model.tcn.tcn_output`` is replaced by ``Identity`` there, so the classifier lives under
``video_classifier.*`` only.  The same generator runs where the goldens are made and on the GPU box: goldens never carry weights.
"""
from __future__ import annotations

import math
from typing import Any

import torch

from .config import Config
from .init import RESNET_PLANES, Spec

SE_REDUCTION = 16            # densetcn.py:51 SELayer(n_inputs, reduction=16)
TCN = "model.tcn.tcn_trunk.features"


def default_dctcn_config(**kw: Any) -> Config:
    """``LRW/video/config/dc-tcn-base.yaml``; overrides as ``model__dctcn__use_boundary=False`` (``__`` = ``.``)."""
    cfg = Config(
        data=dict(input_size=96),
        model=dict(
            name="dc-tcn",
            wav2vec=dict(path="./LRW/vq-wav2vec_kmeans.pt", alignment=4),
            dctcn=dict(
                modality="video", num_classes=500,
                densetcn_options=dict(block_config=[3, 3, 3, 3], growth_rate_set=[384, 384, 384, 384], reduced_size=512,
                                      kernel_size_set=[3, 5, 7], dilation_size_set=[1, 2, 5], squeeze_excitation=True, dropout=0.2),
                backbone_type="resnet", relu_type="swish", width_mult=1.0, use_boundary=True, extract_feats=False),
        ),
        optim=dict(
            optimizer=dict(opt="adamw", betas=[0.9, 0.999], eps=1e-6, weight_decay=1e-2),
            scheduler=dict(max_lr=3e-4, pct_start=0.0, anneal_strategy="cos", three_phase=False),
            mixup_alpha=0.4, lambda_audio=10.0),
        train=dict(batch_size=96, label_smoothing=0.0),
    )
    for k, v in kw.items():
        cfg.set_path(k.replace("__", "."), v)
    return cfg


def tiny_dctcn_config(use_boundary: bool = True, **kw: Any) -> Config:
    """A cut-down back-end that keeps every mechanism: dilations 1/2/5 (three layers in the first block), kernel sizes 3/5/7,
    squeeze-and-excitation, a transition between blocks, PReLU in transition0."""
    cfg = default_dctcn_config(model__dctcn__use_boundary=bool(use_boundary))
    cfg.model.dctcn.densetcn_options.update(block_config=[3, 1], growth_rate_set=[192, 192], reduced_size=128)
    cfg.data.input_size = 40
    for k, v in kw.items():
        cfg.set_path(k.replace("__", "."), v)
    return cfg


def dctcn_dims(cfg: Config) -> dict:
    d = cfg.model.dctcn
    o = d.densetcn_options
    blocks, growth = [int(v) for v in o.block_config], [int(v) for v in o.growth_rate_set]
    reduced = int(o.reduced_size)
    return dict(blocks=blocks, growth=growth, reduced=reduced, ks=[int(v) for v in o.kernel_size_set], ds=[int(v) for v in o.dilation_size_set],
                se=bool(o.squeeze_excitation), in_size=512 + (1 if d.use_boundary else 0), out_size=reduced + blocks[-1] * growth[-1],
                classes=int(d.num_classes), A=int(cfg.model.wav2vec.alignment), G=2, V=320)


def dctcn_layers(cfg: Config):
    """(prefix, n_in, growth, dilation) of every dense layer, in forward order, and (name, n_in) of every transition behind a block."""
    dm = dctcn_dims(cfg)
    layers, trans = [], []
    for bi, nl in enumerate(dm["blocks"]):
        g = dm["growth"][bi]
        for li in range(nl):
            layers.append((f"{TCN}.denseblock{bi + 1}.denselayer{li + 1}", dm["reduced"] + li * g, g, dm["ds"][li % len(dm["ds"])], bi))
        if bi != len(dm["blocks"]) - 1:
            trans.append((f"{TCN}.transition{bi + 1}", dm["reduced"] + nl * g, bi))
    return layers, trans


def _bn(p: str, c: int) -> list[Spec]:
    return [(f"{p}.weight", (c,), "norm_w"), (f"{p}.bias", (c,), "norm_b")]


def dctcn_param_specs(cfg: Config) -> list[Spec]:
    dm = dctcn_dims(cfg)
    specs: list[Spec] = [("model.frontend3D.0.weight", (64, 1, 5, 7, 7), "conv")] + _bn("model.frontend3D.1", 64)
    inplanes = 64
    for li, planes in enumerate(RESNET_PLANES, start=1):
        for bi in range(2):
            p = f"model.trunk.layer{li}.{bi}"
            stride = 2 if (bi == 0 and li > 1) else 1
            specs += [(f"{p}.conv1.weight", (planes, inplanes, 3, 3), "conv")] + _bn(f"{p}.bn1", planes)
            specs += [(f"{p}.conv2.weight", (planes, planes, 3, 3), "conv")] + _bn(f"{p}.bn2", planes)
            if bi == 0 and (stride != 1 or inplanes != planes):
                specs += [(f"{p}.downsample.0.weight", (planes, inplanes, 1, 1), "conv")] + _bn(f"{p}.downsample.1", planes)
            inplanes = planes
    R = dm["reduced"]
    specs += [(f"{TCN}.transition0.conv.weight", (R, dm["in_size"], 1), "tconv_w")] + _bn(f"{TCN}.transition0.norm", R)
    specs += [(f"{TCN}.transition0.prelu.weight", (R,), "prelu")]
    layers, trans = dctcn_layers(cfg)
    trans = {bi: (name, n) for name, n, bi in trans}
    for i, (p, n_in, g, d, bi) in enumerate(layers):
        gb = g // len(dm["ks"])
        for ki, k in enumerate(dm["ks"]):
            if dm["se"]:
                specs += [(f"{p}.cbcr0_se_{ki}.fc.0.weight", (n_in // SE_REDUCTION, n_in), "linear_w"),
                          (f"{p}.cbcr0_se_{ki}.fc.2.weight", (n_in, n_in // SE_REDUCTION), "linear_w")]
            specs += [(f"{p}.cbcr0_{ki}.net.0.weight", (gb, n_in, k), "tconv_w"), (f"{p}.cbcr0_{ki}.net.0.bias", (gb,), "tconv_b")]
            specs += _bn(f"{p}.cbcr0_{ki}.net.1", gb)
        for ki, k in enumerate(dm["ks"]):
            specs += [(f"{p}.cbcr1_{ki}.net.0.weight", (gb, g, k), "tconv_w"), (f"{p}.cbcr1_{ki}.net.0.bias", (gb,), "tconv_b")]
            specs += _bn(f"{p}.cbcr1_{ki}.net.1", gb)
        if n_in != g:
            specs += [(f"{p}.downsample.weight", (g, n_in, 1), "tconv_w"), (f"{p}.downsample.bias", (g,), "tconv_b")]
        last_of_block = i + 1 == len(layers) or layers[i + 1][4] != bi
        if last_of_block and bi in trans:
            name, n = trans[bi]
            specs += [(f"{name}.conv.weight", (R, n, 1), "tconv_w")] + _bn(f"{name}.norm", R)
    C = dm["out_size"]
    specs += _bn(f"{TCN}.norm5", C)
    specs += [("video_classifier.weight", (dm["classes"], C), "linear_w"), ("video_classifier.bias", (dm["classes"],), "linear_b")]
    NA = dm["A"] * dm["G"] * dm["V"]
    specs += [("audio_projection.weight", (NA, C), "linear_w"), ("audio_projection.bias", (NA,), "linear_b")]
    return specs


def dctcn_buffer_specs(cfg: Config) -> list[Spec]:
    """Running statistics of every BatchNorm (3d, 2d and 1d)."""
    out: list[Spec] = []
    for name, shape, kind in dctcn_param_specs(cfg):
        if kind == "norm_w":
            base = name[: -len(".weight")]
            out += [(f"{base}.running_mean", shape, "bn_mean"), (f"{base}.running_var", shape, "bn_var"),
                    (f"{base}.num_batches_tracked", (), "bn_count")]
    return out


def dctcn_init_state_dict(cfg: Config, seed: int = 0, head_gain: float = 4.0) -> dict[str, torch.Tensor]:
    """Deterministic fp32 CPU state dict.  Weights follow the reference's own rule (``tcn/model.py:180-204``: N(0, sqrt(2 / (prod(kernel) *
    out_channels))) for convolutions, N(0, sqrt(2 / fan_in)) for Linear); everything that rule makes trivial is perturbed, otherwise the eval
    BatchNorm, the conv biases and PReLU are not exercised: running means / variances, affine weights / biases, conv biases, PReLU slopes
    around 0.25.  `head_gain` scales the classifier so that the top-1 / top-2 gaps of random clips clear the bf16 floor."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    sd: dict[str, torch.Tensor] = {}

    def u(shape, lo, hi):
        return lo + (hi - lo) * torch.rand(shape, generator=g)

    for name, shape, kind in dctcn_param_specs(cfg):
        if kind in ("conv", "tconv_w"):
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[0] * math.prod(shape[2:])))
        elif kind == "linear_w":
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / shape[1])
            if name.startswith("video_classifier"):
                t = t * head_gain
        elif kind in ("tconv_b", "linear_b", "norm_b"):
            t = u(shape, -0.1, 0.1)
        elif kind == "norm_w":
            t = u(shape, 0.9, 1.1)
        elif kind == "prelu":
            t = u(shape, 0.1, 0.4)
        else:  # pragma: no cover
            raise AssertionError(kind)
        sd[name] = t.float().contiguous()
    for name, shape, kind in dctcn_buffer_specs(cfg):
        sd[name] = u(shape, -0.1, 0.1).float() if kind == "bn_mean" else u(shape, 0.8, 1.25).float() if kind == "bn_var" else torch.zeros((), dtype=torch.long)
    return sd


def dctcn_synthetic_batch(cfg: Config, batch: int, frames: int = 29, size: int | None = None, seed: int = 1234, lengths=None):
    """(videos [B,1,T,H,W] N(0,1), audio tokens int64 [B, A*T, 2], labels int64 [B], word_mask fp32 [B,T], attention_mask fp32 [B,T]).
    attention_mask row b is ones up to lengths[b] (default: the first clip whole, the others a random tail padded); word_mask marks a
    random interval inside it."""
    dm = dctcn_dims(cfg)
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    size = int(cfg.data.input_size) if size is None else int(size)
    videos = torch.randn(batch, 1, frames, size, size, generator=g)
    tokens = torch.randint(0, dm["V"], (batch, frames * dm["A"], dm["G"]), generator=g)
    labels = torch.randint(0, dm["classes"], (batch,), generator=g)
    if lengths is None:
        lengths = torch.randint(max(1, frames // 2), frames + 1, (batch,), generator=g)
        lengths[0] = frames
    lengths = torch.as_tensor(lengths, dtype=torch.long)
    attention = (torch.arange(frames)[None, :] < lengths[:, None]).float()
    lo = (torch.rand(batch, generator=g) * lengths * 0.5).long()
    hi = torch.minimum(lo + 1 + (torch.rand(batch, generator=g) * lengths * 0.5).long(), lengths)
    word = ((torch.arange(frames)[None, :] >= lo[:, None]) & (torch.arange(frames)[None, :] < hi[:, None])).float()
    return videos, tokens, labels, word, attention
