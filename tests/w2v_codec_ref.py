"""fp32 CPU restatement of the wav2vec2 audio tokeniser (HF Wav2Vec2FeatureEncoder + feature_projection.layer_norm + the Gumbel quantiser's
weight_proj / argmax, as the reference's `forward_audios` uses them: LRS e2e_asr_transformer.py:167-180, LRW lightning.py:121-131), plain
torch, and a seeded full-size weight generator.  The GPU tests compare syncvsr_amd.audio_codec.Wav2Vec2Codec with it;
tests/golden/make_golden_w2v_codec.py checks it against HF transformers itself.

Weights use the reference's state-dict names without the `wav2vec.` prefix (`wav2vec2.feature_extractor.conv_layers.{i}.conv.weight`, ...).
Training-mode noise replays csrc/w2v_codec.hip: g = -log(-log u), u = (hash + 0.5) 2^-32, hash of syncvsr_amd/dropout.py's counter hash.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

KERNELS = (10, 3, 3, 3, 3, 2, 2)
STRIDES = (5, 2, 2, 2, 2, 2, 2)
C = 512
G, V = 2, 320
GUMBEL_SITE = 0x57325601          # syncvsr_amd/audio_codec.py
FE = "wav2vec2.feature_extractor.conv_layers"
PROJ = "wav2vec2.feature_projection.layer_norm"
QW = "quantizer.weight_proj"


def frames(L: int) -> list[int]:
    """Frame count after every layer for L samples (padding included)."""
    out, n = [], L
    for k, s in zip(KERNELS, STRIDES):
        n = (n - k) // s + 1
        out.append(n)
    return out


def seeded_weights(mode: str, seed: int = 0) -> dict[str, torch.Tensor]:
    """Full-size weights (512 channels, 7 layers) scaled so activations stay O(1): He-scaled convolutions (GELU halves the second moment),
    norms near identity, weight_proj rows of norm ~2 (logits of standard deviation ~2 on unit-variance features)."""
    g = torch.Generator().manual_seed(seed)
    sd: dict[str, torch.Tensor] = {}
    cin = 1
    for i, k in enumerate(KERNELS):
        fan = cin * k
        gain = 1.0 if i == 0 else 2.0
        sd[f"{FE}.{i}.conv.weight"] = torch.randn(C, cin, k, generator=g) * (gain / fan) ** 0.5 * (4.0 if i == 0 else 1.0)
        if mode == "layer":
            sd[f"{FE}.{i}.conv.bias"] = 0.1 * torch.randn(C, generator=g)
            sd[f"{FE}.{i}.layer_norm.weight"] = 1.0 + 0.1 * torch.randn(C, generator=g)
            sd[f"{FE}.{i}.layer_norm.bias"] = 0.1 * torch.randn(C, generator=g)
        elif i == 0:
            sd[f"{FE}.0.layer_norm.weight"] = 1.0 + 0.1 * torch.randn(C, generator=g)
            sd[f"{FE}.0.layer_norm.bias"] = 0.1 * torch.randn(C, generator=g)
        cin = C
    sd[f"{PROJ}.weight"] = 1.0 + 0.1 * torch.randn(C, generator=g)
    sd[f"{PROJ}.bias"] = 0.1 * torch.randn(C, generator=g)
    sd[f"{QW}.weight"] = torch.randn(G * V, C, generator=g) * (4.0 / C) ** 0.5
    sd[f"{QW}.bias"] = 0.1 * torch.randn(G * V, generator=g)
    return sd


def hf_config_kwargs(mode: str) -> dict:
    """Wav2Vec2Config keywords of the supported shape (conv_dim 512 x 7, the kernels / strides above, 2 x 320 codevectors)."""
    return dict(feat_extract_norm=mode, conv_bias=(mode == "layer"), conv_dim=(C,) * 7, conv_kernel=KERNELS, conv_stride=STRIDES,
                num_codevector_groups=G, num_codevectors_per_group=V, feat_extract_activation="gelu", layer_norm_eps=1e-5,
                hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, codevector_dim=2 * G,
                proj_codevector_dim=8, do_stable_layer_norm=False)


def synthetic_waveform(B: int, L: int, seed: int = 0) -> torch.Tensor:
    """[B, 1, L] fp32: a few tones plus noise, amplitude ~0.3 (16 kHz speech-like range)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 16000.0
    out = torch.zeros(B, L, dtype=torch.float64)
    for b in range(B):
        f = 100.0 + 900.0 * torch.rand(3, generator=g, dtype=torch.float64)
        for j in range(3):
            out[b] += 0.1 * torch.sin(2 * np.pi * f[j] * t + j)
        out[b] += 0.05 * torch.randn(L, generator=g, dtype=torch.float64)
    return out.float().unsqueeze(1)


def features(sd: dict, mode: str, wave: torch.Tensor, pad: int = 0, eps: float = 1e-5, layers_out: list | None = None) -> torch.Tensor:
    """wave [B, L] or [B, 1, L] -> projection LayerNorm output [B, F6, 512] fp32 (the quantiser's input).  layers_out: per-layer outputs
    [B, F_i, 512] (after the norm / GELU)."""
    x = wave.reshape(wave.size(0), -1).float()
    if pad:
        x = torch.cat([x, torch.zeros(x.size(0), pad)], dim=1)
    h = x.unsqueeze(1)
    for i, (k, s) in enumerate(zip(KERNELS, STRIDES)):
        h = F.conv1d(h, sd[f"{FE}.{i}.conv.weight"].float(), sd.get(f"{FE}.{i}.conv.bias"), stride=s)
        if mode == "layer":
            h = F.layer_norm(h.transpose(1, 2), (C,), sd[f"{FE}.{i}.layer_norm.weight"], sd[f"{FE}.{i}.layer_norm.bias"], 1e-5).transpose(1, 2)
        elif i == 0:
            h = F.group_norm(h, C, sd[f"{FE}.0.layer_norm.weight"], sd[f"{FE}.0.layer_norm.bias"], 1e-5)
        h = F.gelu(h)
        if layers_out is not None:
            layers_out.append(h.transpose(1, 2).contiguous())
    return F.layer_norm(h.transpose(1, 2), (C,), sd[f"{PROJ}.weight"], sd[f"{PROJ}.bias"], eps)


def logits(sd: dict, feats: torch.Tensor) -> torch.Tensor:
    """[B, F, 512] -> [B, F, 640] fp32."""
    return F.linear(feats, sd[f"{QW}.weight"].float(), sd[f"{QW}.bias"].float())


def gumbel(seed_word: int, R: int, site: int = GUMBEL_SITE) -> torch.Tensor:
    """The noise k_w2v_quantize adds in training: [R, 640] fp32, element (r, c) from counter r * 640 + c."""
    from syncvsr_amd.dropout import _mix

    m = np.uint64(0xFFFFFFFF)
    key = _mix(np.array([(seed_word * 0x9E3779B9 + site * 0x7F4A7C15 + 0x165667B1) & 0xFFFFFFFF], dtype=np.uint64))[0]
    idx = np.arange(R * G * V, dtype=np.uint64)
    h = _mix((idx * np.uint64(2654435761) + key) & m)
    u = (h.astype(np.float64) + 0.5) * 2.0 ** -32
    return torch.from_numpy((-np.log(-np.log(u))).astype(np.float32)).view(R, G * V)


def tokens_from_logits(z: torch.Tensor) -> torch.Tensor:
    """[..., 640] -> int64 [..., 2] = (argmax of group 0, 320 + argmax of group 1) — the reference's codevectors = arange(640) trick."""
    idx = z.unflatten(-1, (G, V)).argmax(-1)
    return idx + torch.arange(G) * V


def tokenize(sd: dict, mode: str, wave: torch.Tensor, pad: int = 0, seed_word: int | None = None, eps: float = 1e-5):
    """-> (tokens int64 [B, F6, 2], logits fp32 [B, F6, 640]).  seed_word: the training-mode draw (argmax of logits + noise)."""
    z = logits(sd, features(sd, mode, wave, pad, eps))
    if seed_word is None:
        return tokens_from_logits(z), z
    B, Fr = z.shape[:2]
    return tokens_from_logits(z + gumbel(seed_word, B * Fr).view(B, Fr, -1)), z


def margins(z: torch.Tensor) -> torch.Tensor:
    """Top-1 minus top-2 logit per (frame, group): [..., 2]."""
    top = z.unflatten(-1, (G, V)).topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]
