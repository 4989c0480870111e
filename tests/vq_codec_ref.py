"""fp32 CPU restatement of the vq-wav2vec k-means audio tokeniser, as the reference's `forward_audios` uses it (LRW lightning.py:121-131:
``wav2vec.feature_extractor(audios)`` then ``wav2vec.vector_quantizer.forward_idx(...)[1]``), built from nn.Conv1d / nn.GroupNorm in fairseq's
module tree (Wav2VecModel.feature_extractor = ConvFeatureExtractionModel, .vector_quantizer = KmeansVectorQuantizer) so that ``state_dict()``
gives exactly fairseq's names.  The GPU tests compare syncvsr_amd.audio_codec.VqWav2VecCodec with it.

`replay()` is the same computation with the roundings of csrc/vq_codec.hip: layer 0 in fp32, bf16 weights and bf16 stored activations in
layers 1-7 (the contraction's output is stored as bf16 before its GroupNorm reads it, and again after), a bf16-weight projection kept in fp32,
bf16 normalised projections against bf16 centroids.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

KERNELS = (10, 8, 4, 4, 4, 1, 1, 1)
STRIDES = (5, 4, 2, 2, 2, 1, 1, 1)
C = 512
G, V, D = 2, 320, 256
FE = "feature_extractor.conv_layers"
VQ = "vector_quantizer"
CONV_FEATURE_LAYERS = "[(512, 10, 5), (512, 8, 4), (512, 4, 2), (512, 4, 2), (512, 4, 2), (512, 1, 1), (512, 1, 1), (512, 1, 1)]"


def frames(L: int) -> list[int]:
    """Frame count after every layer for L samples (padding included)."""
    out, n = [], L
    for k, s in zip(KERNELS, STRIDES):
        n = (n - k) // s + 1
        out.append(n)
    return out


def fairseq_args(**over) -> dict:
    """The wav2vec args of the released vq-wav2vec_kmeans.pt that the codec looks at."""
    d = dict(vq_type="kmeans", conv_feature_layers=CONV_FEATURE_LAYERS, skip_connections_feat=False, log_compression=True, vq_groups=G,
             vq_vars=V, vq_dim=0, combine_groups=False)
    d.update(over)
    return d


class ConvFeatureExtractionModel(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 1
        for k, s in zip(KERNELS, STRIDES):
            layers.append(nn.Sequential(nn.Conv1d(cin, C, k, stride=s, bias=False), nn.Dropout(0.0), nn.GroupNorm(1, C), nn.ReLU()))
            cin = C
        self.conv_layers = nn.ModuleList(layers)

    def forward(self, x: torch.Tensor, layers_out: list | None = None) -> torch.Tensor:
        x = x.unsqueeze(1)
        for i, conv in enumerate(self.conv_layers):
            x = conv(x)
            if i == len(self.conv_layers) - 1:
                x = (x.abs() + 1).log()
            if layers_out is not None:
                layers_out.append(x.transpose(1, 2).contiguous())
        return x


class KmeansVectorQuantizer(nn.Module):
    def __init__(self, combine_groups: bool = False):
        super().__init__()
        self.combine_groups = combine_groups
        self.embedding = nn.Parameter(torch.zeros(V, 1 if combine_groups else G, D))
        self.projection = nn.Sequential(nn.Conv1d(C, C, 1, groups=G, bias=False), nn.GroupNorm(G, C))

    def expand_embedding(self) -> torch.Tensor:
        return self.embedding.expand(V, G, D)

    def project(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 512, T] -> ze as [B, T, G, D]"""
        ze = self.projection(x)
        B, _, T = ze.shape
        return ze.view(B, G, D, T).permute(0, 3, 1, 2)

    def forward_idx(self, x: torch.Tensor) -> torch.Tensor:
        """fairseq's form: the broadcast difference, its 2-norm, argmin over the centroids -> int64 [B, T, G]."""
        ze_ = self.project(x)
        d = (ze_.unsqueeze(0) - self.expand_embedding().unsqueeze(1).unsqueeze(1)).norm(dim=-1, p=2)
        return d.argmin(dim=0)


class VqWav2Vec(nn.Module):
    def __init__(self, combine_groups: bool = False):
        super().__init__()
        self.feature_extractor = ConvFeatureExtractionModel()
        self.vector_quantizer = KmeansVectorQuantizer(combine_groups)


def seeded_model(seed: int = 0, combine_groups: bool = False) -> VqWav2Vec:
    """Full-size weights: He-scaled convolutions (ReLU halves the second moment), affines 1 + 0.1 randn / 0.1 randn, unit-variance centroids:
    with unit-variance normalised projections the scores |e|^2 - 2 z.e have a standard deviation of ~40, so margins are meaningful."""
    g = torch.Generator().manual_seed(seed)
    m = VqWav2Vec(combine_groups).eval().requires_grad_(False)
    for name, p in m.state_dict().items():
        if name.endswith(".0.weight"):
            fan = p.size(1) * p.size(2)
            p.copy_(torch.randn(p.shape, generator=g) * (2.0 / fan) ** 0.5)
        elif name.endswith(".weight"):
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
        elif name.endswith(".bias"):
            p.copy_(0.1 * torch.randn(p.shape, generator=g))
        else:
            assert name == f"{VQ}.embedding", name
            p.copy_(torch.randn(p.shape, generator=g))
    return m


def synthetic_waveform(B: int, L: int, seed: int = 0) -> torch.Tensor:
    """[B, L] fp32: an amplitude-modulated tone plus noise; pitch and amplitude differ from clip to clip."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 16000.0
    out = torch.zeros(B, L, dtype=torch.float64)
    for b in range(B):
        pitch = 120.0 + 140.0 * b + 60.0 * float(torch.rand((), generator=g, dtype=torch.float64))
        amp = 0.08 * (1.0 + 1.5 * b)
        out[b] = amp * (1.0 + 0.5 * torch.sin(2 * np.pi * 4.0 * t + b)) * torch.sin(2 * np.pi * pitch * t)
        out[b] += 0.2 * amp * torch.randn(L, generator=g, dtype=torch.float64)
    return out.float()


def _pad(wave: torch.Tensor, pad: int) -> torch.Tensor:
    x = wave.reshape(wave.size(0), -1).float()
    return torch.cat([x, torch.zeros(x.size(0), pad)], dim=1) if pad else x


def scores(m: VqWav2Vec, ze_: torch.Tensor, emb: torch.Tensor | None = None) -> torch.Tensor:
    """ze_ [B, T, G, D] -> |e|^2 - 2 z.e as [B, T, G, V] (the squared distance without the row's own |z|^2)."""
    e = m.vector_quantizer.expand_embedding() if emb is None else emb          # [V, G, D]
    return e.square().sum(-1).t() - 2.0 * torch.einsum("btgd,vgd->btgv", ze_, e)


def oracle(m: VqWav2Vec, wave: torch.Tensor, pad: int = 0, layers_out: list | None = None):
    """fp32 -> (tokens int64 [B, T, G], scores [B, T, G, V])."""
    with torch.no_grad():
        x = m.feature_extractor(_pad(wave, pad), layers_out)
        s = scores(m, m.vector_quantizer.project(x))
    return s.argmin(-1), s


def bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def gn_relu_step(x: torch.Tensor, gn: nn.GroupNorm, log: bool) -> torch.Tensor:
    """One in-place pass of the kernels on x [B, 512, T] (values already on the bf16 grid): fp32 GroupNorm(1) + ReLU (+ log), stored as bf16."""
    y = F.relu(F.group_norm(x, 1, gn.weight, gn.bias, gn.eps))
    return bf((y + 1).log() if log else y)


def replay(m: VqWav2Vec, wave: torch.Tensor, pad: int = 0, layers_out: list | None = None):
    """The oracle with the kernels' roundings -> (tokens, scores)."""
    with torch.no_grad():
        x = _pad(wave, pad).unsqueeze(1)
        for i, (conv, _, gn, _) in enumerate(m.feature_extractor.conv_layers):
            if i == 0:
                x = bf(F.relu(gn(conv(x))))
            else:
                x = gn_relu_step(bf(F.conv1d(x, bf(conv.weight), stride=conv.stride)), gn, i == len(KERNELS) - 1)
            if layers_out is not None:
                layers_out.append(x.transpose(1, 2).contiguous())
        q = m.vector_quantizer
        ze = F.group_norm(F.conv1d(x, bf(q.projection[0].weight), groups=G), G, q.projection[1].weight, q.projection[1].bias, q.projection[1].eps)
        B, _, T = ze.shape
        s = scores(m, bf(ze.view(B, G, D, T).permute(0, 3, 1, 2)), bf(q.expand_embedding()))
    return s.argmin(-1), s


def margins(s: torch.Tensor) -> torch.Tensor:
    """Second-smallest minus smallest score per (frame, group): [B, T, G]."""
    low = s.topk(2, dim=-1, largest=False).values
    return low[..., 1] - low[..., 0]


# The shapes of the GPU end-to-end test (tests/test_gpu_vq_codec.py) and their waveforms, here so that the measurement its bounds rest on
# and the test itself cannot drift apart.
SHAPES = [(3, 465), (3, 2960), (3, 2963), (2, 18960)]


def case_waveform(B: int, L: int) -> torch.Tensor:
    return synthetic_waveform(B, L, 11 + L % 7)


def measure_replay(seed: int = 1) -> dict:
    """max |oracle - replay| of the scores and the replay's flipped tokens per shape of SHAPES, on the CPU: what EPS and REPLAY_FLIP_SHARE
    of the GPU test are derived from (`python tests/vq_codec_ref.py` prints it)."""
    m = seeded_model(seed)
    rows = []
    for B, L in SHAPES:
        wave = case_waveform(B, L)
        t0, s0 = oracle(m, wave)
        t1, s1 = replay(m, wave)
        rows.append(dict(B=B, L=L, max_abs=round((s0 - s1).abs().max().item(), 4), flips=int((t0 != t1).sum()), tokens=t0.numel()))
    return dict(shapes=rows, max_abs=max(r["max_abs"] for r in rows), flips=sum(r["flips"] for r in rows), tokens=sum(r["tokens"] for r in rows))


if __name__ == "__main__":
    import json

    print(json.dumps(measure_replay()))
