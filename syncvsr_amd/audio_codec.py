"""The frozen wav2vec2 audio tokeniser of SyncVSR's `wav2vec2` codec, on the GPU: raw 16 kHz waveform -> int64 tokens [B, F, 2] =
(i0, 320 + i1) per 20 ms frame, what the reference's ``forward_audios`` computes (LRS e2e_asr_transformer.py:145-157,167-180,
LRW lightning.py:121-131) with HF ``Wav2Vec2ForPreTraining``'s feature encoder, ``feature_projection.layer_norm`` and quantiser.

Launches (csrc/w2v_codec.hip, include/syncvsr_hip.h):
  svsr_w2v_conv0          layer 0 (1 -> 512, k 10, s 5) in fp32, with its LayerNorm + GELU ("layer" models) or GroupNorm partial sums ("group")
  svsr_w2v_norm_gelu      GroupNorm finalise + apply + GELU of layer 0 ("group"), LayerNorm + GELU behind layers 1-6 ("layer")
  svsr_igemm_fwd x 6      layers 1-6: a stride-2 kernel-k convolution over channels-last rows is a dense contraction whose row t reads the
                          contiguous k*512 values of frames 2t .. 2t+k-1 (rows of pitch 1024 that overlap for k = 3; weights [Co][k][Ci])
  svsr_w2v_quantize       LayerNorm(512) + weight_proj + per-group argmax (eval) / argmax of logits + Gumbel noise (training)

Frames of a clip start on an even row (frame counts padded to even) so that clip n's rows begin at n * rows / 2 of the overlapping view;
the padding rows are never read by a valid output.  Two ping-pong bf16 buffers of B * F0 * 512 elements are the workspace.

The module holds frozen BUFFERS, not parameters, under the reference's state-dict names (``wav2vec2.feature_extractor.conv_layers.{i}.
{conv,layer_norm}.*``, ``wav2vec2.feature_projection.layer_norm.*``, ``quantizer.weight_proj.*``).  This file does not import transformers:
``Wav2Vec2Codec.from_hf(model)`` only reads ``model.config`` and ``model.state_dict()``.
"""
from __future__ import annotations

from typing import Any, Mapping, Optional

import torch
import torch.nn as nn

from . import ops

KERNELS = (10, 3, 3, 3, 3, 2, 2)
STRIDES = (5, 2, 2, 2, 2, 2, 2)
C = 512
GROUPS, VARS = 2, 320
GUMBEL_SITE = 0x57325601       # counter-hash site of the training-mode noise (dropout sites are small integers)
LRS_PAD = 8000                 # zeros the LRS forward_audios appends to every row (e2e_asr_transformer.py:168-170)
FE = "wav2vec2.feature_extractor.conv_layers"
PROJ = "wav2vec2.feature_projection.layer_norm"
QW = "quantizer.weight_proj"


def frame_counts(L: int) -> list[int]:
    """Frames after each of the 7 convolutions for L samples (padding included)."""
    out, n = [], int(L)
    for k, s in zip(KERNELS, STRIDES):
        n = (n - k) // s + 1
        out.append(n)
    return out


def _cfg_get(cfg: Any, key: str, default=None):
    if isinstance(cfg, Mapping):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def check_config(cfg: Any) -> str:
    """-> "layer" or "group"; NotImplementedError for any shape the kernels do not take."""
    bad = []
    conv_dim = tuple(_cfg_get(cfg, "conv_dim", (C,) * 7))
    if conv_dim != (C,) * 7:
        bad.append(f"conv_dim must be (512,)*7 (the kernels keep 512 channels in every layer), got {conv_dim}")
    if tuple(_cfg_get(cfg, "conv_kernel", KERNELS)) != KERNELS:
        bad.append(f"conv_kernel must be {KERNELS}")
    if tuple(_cfg_get(cfg, "conv_stride", STRIDES)) != STRIDES:
        bad.append(f"conv_stride must be {STRIDES}")
    act = _cfg_get(cfg, "feat_extract_activation", "gelu")
    if act != "gelu":
        bad.append(f"feat_extract_activation must be gelu (exact), got {act!r}")
    if int(_cfg_get(cfg, "num_codevector_groups", GROUPS)) != GROUPS or int(_cfg_get(cfg, "num_codevectors_per_group", VARS)) != VARS:
        bad.append("the quantiser must have 2 groups of 320 codevectors (audio_vocab_size 640)")
    mode = _cfg_get(cfg, "feat_extract_norm", "group")
    if mode not in ("layer", "group"):
        bad.append(f"feat_extract_norm must be 'layer' or 'group', got {mode!r}")
    conv_bias = bool(_cfg_get(cfg, "conv_bias", mode == "layer"))
    if mode == "group" and conv_bias:
        bad.append("feat_extract_norm='group' with conv_bias=True is not a released wav2vec2 layout")
    if mode == "layer" and not conv_bias:
        bad.append("feat_extract_norm='layer' needs conv_bias=True (facebook/wav2vec2-large-xlsr-53)")
    if bad:
        raise NotImplementedError("; ".join(bad))
    return mode


class _Buffers(nn.Module):
    """A node of the state-dict tree that holds frozen buffers only."""

    def __init__(self, **bufs: torch.Tensor):
        super().__init__()
        for k, v in bufs.items():
            self.register_buffer(k, v)


class Wav2Vec2Codec(nn.Module):
    """Frozen wav2vec2 tokeniser.  ``codec(audios, pad=0, sample=False, seed_word=None) -> int64 [B, F, 2]`` for float audios [B, 1, L]
    or [B, L] on the device (pad zeros appended to every row; sample=True draws argmax(logits + Gumbel noise) keyed by the int32 device
    word `seed_word`)."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor], config: Any):
        super().__init__()
        self.mode = check_config(config)
        self.eps_proj = float(_cfg_get(config, "layer_norm_eps", 1e-5))
        sd = {k: v.detach().float().clone() for k, v in state_dict.items()}

        def need(key: str, shape: tuple) -> torch.Tensor:
            if key not in sd:
                raise KeyError(f"wav2vec2 state dict lacks {key}")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"{key}: shape {tuple(sd[key].shape)}, expected {shape}")
            return sd[key]

        layers = []
        cin = 1
        for i, k in enumerate(KERNELS):
            conv = {"weight": need(f"{FE}.{i}.conv.weight", (C, cin, k))}
            if self.mode == "layer":
                conv["bias"] = need(f"{FE}.{i}.conv.bias", (C,))
            node = nn.Module()
            node.conv = _Buffers(**conv)
            if self.mode == "layer" or i == 0:
                node.layer_norm = _Buffers(weight=need(f"{FE}.{i}.layer_norm.weight", (C,)), bias=need(f"{FE}.{i}.layer_norm.bias", (C,)))
            layers.append(node)
            cin = C
        self.wav2vec2 = nn.Module()
        self.wav2vec2.feature_extractor = nn.Module()
        self.wav2vec2.feature_extractor.conv_layers = nn.ModuleList(layers)
        self.wav2vec2.feature_projection = nn.Module()
        self.wav2vec2.feature_projection.layer_norm = _Buffers(weight=need(f"{PROJ}.weight", (C,)), bias=need(f"{PROJ}.bias", (C,)))
        self.quantizer = nn.Module()
        self.quantizer.weight_proj = _Buffers(weight=need(f"{QW}.weight", (GROUPS * VARS, C)), bias=need(f"{QW}.bias", (GROUPS * VARS,)))
        self._packed: Optional[dict] = None
        self._retired: list[dict] = []          # forms of devices left behind: a step list recorded there may still name them
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())
        self.requires_grad_(False)

    @classmethod
    def from_hf(cls, model: Any) -> "Wav2Vec2Codec":
        """From an HF ``Wav2Vec2ForPreTraining`` (duck-typed: ``.config`` and ``.state_dict()``)."""
        sd = {k: v for k, v in model.state_dict().items() if k.startswith((FE, PROJ, QW))}
        return cls(sd, model.config)

    @classmethod
    def from_state_dict(cls, state_dict: Mapping[str, torch.Tensor], config: Mapping[str, Any]) -> "Wav2Vec2Codec":
        """From the reference's state-dict entries (with or without the `wav2vec.` prefix) and a plain config dict (HF Wav2Vec2Config keys)."""
        sd = {(k[len("wav2vec."):] if k.startswith("wav2vec.") else k): v for k, v in state_dict.items()}
        return cls(sd, config)

    # The device forms of the weights (packed()) are made once per device and then only ever updated IN PLACE: a native step list
    # (engine.TrainStep(native=True)) records their addresses, so a load_state_dict / same-device _apply after a recorded step must leave
    # them where the list reads them and put the new values there.  Forms of a device the codec has left are kept alive, not freed.
    def _invalidate(self) -> None:
        self._refresh()

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._refresh()
        return out

    def _refresh(self) -> None:
        p = self._packed
        if p is None:
            return
        with torch.no_grad():
            new = self._forms(p["dev"])
            for k, v in new.items():
                if k == "dev":
                    continue
                for dst, src in (zip(p[k], v) if isinstance(v, list) else ((p[k], v),)):
                    if dst is not None:
                        dst.copy_(src)

    def _conv(self, i: int):
        return self.wav2vec2.feature_extractor.conv_layers[i]

    def _forms(self, dev: torch.device) -> dict:
        p = {"dev": dev}
        c0 = self._conv(0)
        p["w0"] = c0.conv.weight.to(dev, torch.float32).reshape(C, 10).contiguous()
        p["w"] = [None] + [self._conv(i).conv.weight.to(dev, torch.float32).permute(0, 2, 1).reshape(C, -1).to(torch.bfloat16).contiguous()
                           for i in range(1, 7)]
        p["b"] = [self._conv(i).conv.bias.to(dev, torch.float32).contiguous() if self.mode == "layer" else None for i in range(7)]
        p["g"] = [self._conv(i).layer_norm.weight.to(dev, torch.float32).contiguous() if hasattr(self._conv(i), "layer_norm") else None
                  for i in range(7)]
        p["be"] = [self._conv(i).layer_norm.bias.to(dev, torch.float32).contiguous() if hasattr(self._conv(i), "layer_norm") else None
                   for i in range(7)]
        pl = self.wav2vec2.feature_projection.layer_norm
        p["pg"], p["pb"] = pl.weight.to(dev, torch.float32).contiguous(), pl.bias.to(dev, torch.float32).contiguous()
        q = self.quantizer.weight_proj
        p["qw"] = q.weight.to(dev, torch.bfloat16).contiguous()
        p["qb"] = q.bias.to(dev, torch.float32).contiguous()
        return p

    def packed(self, dev: torch.device) -> dict:
        """Device forms the kernels read: fp32 layer-0 weights, bf16 [Co][k][Ci] weights of layers 1-6, bf16 weight_proj.  Stable
        addresses per device (see _refresh)."""
        p = self._packed
        if p is not None and p["dev"] == dev:
            return p
        if p is not None:
            self._retired.append(p)
        with torch.no_grad():
            p = self._forms(dev)
        self._packed = p
        return p

    @staticmethod
    def as_rows(audios: torch.Tensor) -> torch.Tensor:
        """[B, 1, L] or [B, L] float -> [B, L] fp32 contiguous view (a copy only when the input is not already one)."""
        if audios.dim() == 3 and audios.size(1) == 1:
            audios = audios.reshape(audios.size(0), audios.size(2))
        if audios.dim() != 2 or not audios.is_floating_point():
            raise ValueError("audio waveforms must be float [B, 1, L] or [B, L]")
        if audios.dtype != torch.float32 or not audios.is_contiguous():
            audios = audios.float().contiguous()
        return audios

    def __call__(self, audios: torch.Tensor, *, pad: int = 0, sample: bool = False, seed_word: Optional[torch.Tensor] = None,
                 keep: Optional[int] = None, logits_out: Optional[torch.Tensor] = None, layers_out: Optional[list] = None) -> torch.Tensor:
        return self.tokenize(audios, pad=pad, sample=sample, seed_word=seed_word, keep=keep, logits_out=logits_out, layers_out=layers_out)

    def tokenize(self, audios: torch.Tensor, *, pad: int = 0, sample: bool = False, seed_word: Optional[torch.Tensor] = None,
                 keep: Optional[int] = None, logits_out: Optional[torch.Tensor] = None, layers_out: Optional[list] = None) -> torch.Tensor:
        """-> int64 [B, F6, 2], or [B, keep, 2] (the first `keep` frames, contiguous: the LRS crop tokens[:, :T*A]; ValueError when the clip
        has fewer frames).  The Gumbel noise of frame t is the same whatever `keep`.  logits_out (tests): fp32 [B * F6, 640] receives the logits; layers_out (tests): receives the 7 layer
        outputs as bf16 [B, F_i, 512] copies."""
        if audios.device.type != "cuda":
            raise RuntimeError("syncvsr_amd runs on an MI355X HIP device only; there is no CPU fallback (tests/w2v_codec_ref.py is the fp32 restatement)")
        x = self.as_rows(audios)
        if sample and seed_word is None:
            raise ValueError("sample=True needs the int32 device seed word")
        B, L_in = x.shape
        fr = frame_counts(L_in + int(pad))
        if fr[-1] < 1:
            raise ValueError(f"{L_in + int(pad)} samples give no frame")
        keep = fr[-1] if keep is None else int(keep)
        if not 1 <= keep <= fr[-1]:
            raise ValueError(f"{L_in} samples (+ {int(pad)} zeros) give {fr[-1]} audio frames, need {keep}")
        dev = x.device
        p = self.packed(dev)
        rows = [f + (f & 1) for f in fr[:-1]] + [fr[-1]]         # rows per clip in each layer's output (even: clip n starts on a row boundary)
        cap = B * rows[0] * C
        bufs = (torch.empty(cap, dtype=torch.bfloat16, device=dev), torch.empty(cap, dtype=torch.bfloat16, device=dev))
        group = self.mode == "group"
        stats = torch.empty(ops.w2v_stats_floats(B, fr[0]), dtype=torch.float32, device=dev) if group else None
        ops.w2v_conv0(x, B, L_in, int(pad), p["w0"], p["b"][0], p["g"][0], p["be"][0], 1e-5, bufs[0], rows[0], stats, group)
        if group:
            ops.w2v_norm_gelu(bufs[0], B, fr[0], rows[0], p["g"][0], p["be"][0], 1e-5, stats=stats, group=True)
        if layers_out is not None:
            layers_out.append(bufs[0][: B * rows[0] * C].view(B, rows[0], C)[:, : fr[0]].clone())
        cur = 0
        for i in range(1, 7):
            k = KERNELS[i]
            src, dst = bufs[cur], bufs[1 - cur]
            plan = ops.rows_plan(B, fr[i], 0, 0, C)
            ops.igemm_fwd(plan, src, p["w"][i], dst, Nimg=B, in_pix=rows[i - 1] // 2, Ci=k * C, in_pitch=2 * C, Co=C, out_pix=rows[i],
                          out_pitch=C, bias=p["b"][i], gelu=group, flops=2.0 * B * fr[i] * C * k * C)
            if not group:
                ops.w2v_norm_gelu(dst, B, fr[i], rows[i], p["g"][i], p["be"][i], 1e-5)
            if layers_out is not None:
                layers_out.append(dst[: B * rows[i] * C].view(B, rows[i], C)[:, : fr[i]].clone())
            cur = 1 - cur
        R = B * fr[-1]
        tok = torch.empty(B * keep * GROUPS, dtype=torch.int64, device=dev)
        ops.w2v_quantize(bufs[cur], R, fr[-1], keep, p["pg"], p["pb"], self.eps_proj, p["qw"], p["qb"], tok, seed=seed_word if sample else None,
                         site=GUMBEL_SITE, logits_out=logits_out)
        return tok.view(B, keep, GROUPS)

    def workspace_bytes(self, B: int, L: int) -> int:
        """Device bytes one call allocates for B clips of L samples (padding included): the two ping-pong buffers, the GroupNorm partials."""
        fr = frame_counts(L)
        r0 = fr[0] + (fr[0] & 1)
        n = 2 * B * r0 * C * 2 + B * fr[-1] * GROUPS * 8
        if self.mode == "group":
            n += 4 * ops.w2v_stats_floats(B, fr[0])
        return n
