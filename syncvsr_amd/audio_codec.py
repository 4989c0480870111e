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

The `vq` codec of the word-level configurations (fairseq vq-wav2vec, k-means) is ``VqWav2VecCodec`` in the second half of this file.
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


# ---- vq-wav2vec, k-means variant: the codec of the word-level configurations (config.audio_codec_dims: ("vq", A = 4, G = 2, V = 320)) ----------
#
# fairseq Wav2VecModel.feature_extractor + vector_quantizer.forward_idx (LRW lightning.py:121-131), restated in tests/vq_codec_ref.py.
# Launches (csrc/vq_codec.hip):
#   svsr_vq_conv0_stats, svsr_vq_conv0_apply   layer 0 computed twice: statistics of its clip-wide GroupNorm, then normalise + ReLU; no pre-norm tensor
#   svsr_igemm_fwd x 7                         layers 1-7: a stride-s kernel-k convolution is a dense contraction over rows of pitch s*512
#   svsr_vq_gn_partial, svsr_vq_gn_relu x 7    GroupNorm(1, 512) + ReLU in place behind each (+ log(x + 1) behind the last)
#   svsr_vq_project, svsr_vq_assign            grouped projection + GroupNorm(2, 512) + nearest centroid per group
# Frames of a clip start on a multiple of the next layer's stride (frame counts padded up), so clip n's rows begin at n * rows / s of the
# overlapping view; the padding rows are never read by a valid output.
VQ_KERNELS = (10, 8, 4, 4, 4, 1, 1, 1)
VQ_STRIDES = (5, 4, 2, 2, 2, 1, 1, 1)
VQ_LAYERS = tuple((C, k, s) for k, s in zip(VQ_KERNELS, VQ_STRIDES))
VQ_D = C // GROUPS
VQ_EPS = 1e-5                  # nn.GroupNorm default, which fairseq's Fp32GroupNorm keeps
VQ_FE = "feature_extractor.conv_layers"
VQ_Q = "vector_quantizer"


def vq_frame_counts(L: int) -> list[int]:
    """Frames after each of the 8 convolutions for L samples (padding included); the total stride is 160, the receptive field 465 samples."""
    out, n = [], int(L)
    for k, s in zip(VQ_KERNELS, VQ_STRIDES):
        n = (n - k) // s + 1
        out.append(n)
    return out


def vq_min_samples(frames: int) -> int:
    """Samples that give `frames` tokens: 160 * (frames - 1) + 465 (keep = A * T = 4 T needs 640 T + 305)."""
    return 160 * (int(frames) - 1) + 465


def vq_check_config(cfg: Any) -> bool:
    """fairseq wav2vec args (namespace or mapping; None: the released layout) -> combine_groups.  NotImplementedError, with the reason,
    for anything but the released k-means layout."""
    if cfg is None:
        return False
    bad = []
    vq_type = _cfg_get(cfg, "vq_type", "kmeans")
    if vq_type != "kmeans":
        bad.append(f"vq_type must be 'kmeans' (the Gumbel variant is not built), got {vq_type!r}")
    layers = _cfg_get(cfg, "conv_feature_layers", VQ_LAYERS)
    if isinstance(layers, str):
        import ast
        try:
            layers = ast.literal_eval(layers)
        except (ValueError, SyntaxError):
            layers = None
    try:
        layers = tuple(tuple(int(v) for v in l) for l in layers)
    except (TypeError, ValueError):
        layers = None
    if layers != VQ_LAYERS:
        bad.append(f"conv_feature_layers must be {list(VQ_LAYERS)} (the kernels keep 512 channels and these kernel / stride pairs), got {layers}")
    if bool(_cfg_get(cfg, "skip_connections_feat", False)):
        bad.append("skip_connections_feat is not supported (the released model has no skip connections in the feature extractor)")
    if not bool(_cfg_get(cfg, "log_compression", True)):
        bad.append("log_compression must be True (log(|x| + 1) is fused into the last GroupNorm pass)")
    groups = int(_cfg_get(cfg, "vq_groups", GROUPS))
    if groups != GROUPS:
        bad.append(f"vq_groups must be {GROUPS}, got {groups}")
    nvars = int(_cfg_get(cfg, "vq_vars", VARS))
    if nvars != VARS:
        bad.append(f"vq_vars must be {VARS} (audio_vocab_size 320 per group), got {nvars}")
    vq_dim = int(_cfg_get(cfg, "vq_dim", 0))
    if vq_dim not in (0, C):            # (0: fairseq takes the feature dimension, 512)
        bad.append(f"vq_dim must be {C}, got {vq_dim}")
    if bad:
        raise NotImplementedError("; ".join(bad))
    return bool(_cfg_get(cfg, "combine_groups", False))


class VqWav2VecCodec(nn.Module):
    """Frozen vq-wav2vec (k-means) tokeniser.  ``codec(audios, pad=0, keep=None) -> int64 [B, keep or F, 2]``, both entries in 0..319, for
    float audios [B, 1, L] or [B, L] on the device (pad zeros appended to every row).  Deterministic in train and eval mode."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor], config: Any = None):
        super().__init__()
        vq_check_config(config)
        sd = {k: v.detach().float().clone() for k, v in state_dict.items()}

        def need(key: str, *shapes: tuple) -> torch.Tensor:
            if key not in sd:
                raise KeyError(f"vq-wav2vec state dict lacks {key}")
            if tuple(sd[key].shape) not in shapes:
                raise ValueError(f"{key}: shape {tuple(sd[key].shape)}, expected {' or '.join(map(str, shapes))}")
            return sd[key]

        def affine(prefix: str) -> _Buffers:          # a GroupNorm without affine is the identity one
            if f"{prefix}.weight" not in sd and f"{prefix}.bias" not in sd:
                return _Buffers(weight=torch.ones(C), bias=torch.zeros(C))
            return _Buffers(weight=need(f"{prefix}.weight", (C,)), bias=need(f"{prefix}.bias", (C,)))

        layers = []
        cin = 1
        for i, k in enumerate(VQ_KERNELS):
            node = nn.Module()
            node.add_module("0", _Buffers(weight=need(f"{VQ_FE}.{i}.0.weight", (C, cin, k))))
            node.add_module("2", affine(f"{VQ_FE}.{i}.2"))
            layers.append(node)
            cin = C
        self.feature_extractor = nn.Module()
        self.feature_extractor.conv_layers = nn.ModuleList(layers)
        proj = nn.Module()
        proj.add_module("0", _Buffers(weight=need(f"{VQ_Q}.projection.0.weight", (C, VQ_D, 1))))
        proj.add_module("1", affine(f"{VQ_Q}.projection.1"))
        self.vector_quantizer = _Buffers(embedding=need(f"{VQ_Q}.embedding", (VARS, GROUPS, VQ_D), (VARS, 1, VQ_D)))
        self.vector_quantizer.projection = proj
        self._packed: Optional[dict] = None
        self._retired: list[dict] = []          # forms of devices left behind: a step list recorded there may still name them
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())
        self.requires_grad_(False)

    # The device forms (packed()) follow Wav2Vec2Codec's contract — made once per device, then only ever updated in place, because a native
    # step list records their addresses — and are kept by its very functions, which only rely on _forms(dev) and the two attributes above.
    _invalidate = Wav2Vec2Codec._invalidate
    _refresh = Wav2Vec2Codec._refresh
    packed = Wav2Vec2Codec.packed
    as_rows = staticmethod(Wav2Vec2Codec.as_rows)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._refresh()
        return out

    @classmethod
    def from_state_dict(cls, state_dict: Mapping[str, torch.Tensor], config: Any = None) -> "VqWav2VecCodec":
        """From fairseq's state-dict entries (with or without the reference's `wav2vec.` prefix; the aggregator and prediction heads are
        ignored) and, optionally, fairseq's wav2vec args."""
        sd = {(k[len("wav2vec."):] if k.startswith("wav2vec.") else k): v for k, v in state_dict.items()}
        return cls({k: v for k, v in sd.items() if k.startswith((VQ_FE, VQ_Q))}, config)

    @classmethod
    def from_checkpoint(cls, ckpt: Mapping[str, Any]) -> "VqWav2VecCodec":
        """From an already loaded fairseq checkpoint (``torch.load`` of vq-wav2vec_kmeans.pt): ``ckpt["model"]`` and, where they are a plain
        namespace or mapping, ``ckpt["args"]``."""
        import argparse
        import types

        args = ckpt.get("args")
        if isinstance(args, (argparse.Namespace, types.SimpleNamespace)):
            args = vars(args)
        elif not (args is None or type(args) is dict):
            # anything else (an omegaconf node, fairseq's own config classes) is not read: attribute access on it could give defaults for
            # keys it spells differently, and a layout other than the released one would pass unseen
            raise NotImplementedError(f"checkpoint args of type {type(args).__name__} are not read: pass a plain namespace or dict "
                                      f"(VqWav2VecCodec.from_state_dict(ckpt['model'], args))")
        return cls.from_state_dict(ckpt["model"], args)

    def _forms(self, dev: torch.device) -> dict:
        p = {"dev": dev}
        cl = self.feature_extractor.conv_layers
        conv = lambda i: getattr(cl[i], "0").weight
        norm = lambda i: getattr(cl[i], "2")
        p["w0"] = conv(0).to(dev, torch.float32).reshape(C, 10).contiguous()
        p["w"] = [None] + [conv(i).to(dev, torch.float32).permute(0, 2, 1).reshape(C, -1).to(torch.bfloat16).contiguous() for i in range(1, 8)]
        p["g"] = [norm(i).weight.to(dev, torch.float32).contiguous() for i in range(8)]
        p["be"] = [norm(i).bias.to(dev, torch.float32).contiguous() for i in range(8)]
        pr = self.vector_quantizer.projection
        p["pw"] = getattr(pr, "0").weight.to(dev, torch.float32).reshape(C, VQ_D).to(torch.bfloat16).contiguous()
        p["pg"] = getattr(pr, "1").weight.to(dev, torch.float32).contiguous()
        p["pb"] = getattr(pr, "1").bias.to(dev, torch.float32).contiguous()
        emb = self.vector_quantizer.embedding.to(dev, torch.float32).expand(VARS, GROUPS, VQ_D)      # (combine_groups: one table for both groups)
        p["emb"] = emb.permute(1, 0, 2).to(torch.bfloat16).contiguous()
        p["e2"] = p["emb"].float().square().sum(-1).contiguous()
        return p       # fp32 layer-0 weights, bf16 [Co][k][Ci] weights of layers 1-7, bf16 projection [512][256], bf16 centroids [2][320][256] + their squared norms

    @staticmethod
    def frame_counts(L: int) -> list[int]:
        return vq_frame_counts(L)

    @staticmethod
    def _rows(fr: list[int]) -> list[int]:
        """Rows per clip of each layer's output: the frames rounded up to a multiple of the next layer's stride."""
        return [-(-f // s) * s for f, s in zip(fr[:-1], VQ_STRIDES[1:])] + [fr[-1]]

    def __call__(self, audios: torch.Tensor, *, pad: int = 0, keep: Optional[int] = None, scores_out: Optional[torch.Tensor] = None,
                 layers_out: Optional[list] = None) -> torch.Tensor:
        return self.tokenize(audios, pad=pad, keep=keep, scores_out=scores_out, layers_out=layers_out)

    def tokenize(self, audios: torch.Tensor, *, pad: int = 0, keep: Optional[int] = None, scores_out: Optional[torch.Tensor] = None,
                 layers_out: Optional[list] = None) -> torch.Tensor:
        """-> int64 [B, F, 2], or [B, keep, 2] (the first `keep` frames, contiguous: the crop tokens[:, :T*A]; ValueError when the clip has fewer
        frames).  scores_out (tests): fp32 [B * F, 2, 320] receives |e|^2 - 2 z.e; layers_out (tests): receives the 8 layer outputs as bf16
        [B, F_i, 512] copies and the projection as fp32 [B, F, 512]."""
        if audios.device.type != "cuda":
            raise RuntimeError("syncvsr_amd runs on an MI355X HIP device only; there is no CPU fallback (tests/vq_codec_ref.py is the fp32 restatement)")
        x = self.as_rows(audios)
        B, L_in = x.shape
        L = L_in + int(pad)
        fr = vq_frame_counts(L)
        if fr[-1] < 1:
            raise ValueError(f"{L_in} samples (+ {int(pad)} zeros) give no audio frame: 1 frame needs {vq_min_samples(1)} samples")
        F = fr[-1]
        keep = F if keep is None else int(keep)
        if not 1 <= keep <= F:
            raise ValueError(f"{L_in} samples (+ {int(pad)} zeros) give {F} audio frames, need {keep} frames ({vq_min_samples(max(keep, 1))} samples)")
        dev = x.device
        p = self.packed(dev)
        rows = self._rows(fr)
        slack = max(VQ_KERNELS[1:]) * C          # the overlapping view of the last clip's padding rows stays inside the allocation
        bufs = (torch.empty(B * rows[0] * C + slack, dtype=torch.bfloat16, device=dev),
                torch.empty(B * rows[1] * C + slack, dtype=torch.bfloat16, device=dev))
        part = torch.empty(ops.vq_part_floats(B, fr[0], 0), dtype=torch.float32, device=dev)
        ops.vq_conv0_stats(x, B, L_in, int(pad), p["w0"], part)
        ops.vq_conv0_apply(x, B, L_in, int(pad), p["w0"], p["g"][0], p["be"][0], VQ_EPS, part, bufs[0], rows[0])
        if layers_out is not None:
            layers_out.append(bufs[0][: B * rows[0] * C].view(B, rows[0], C)[:, : fr[0]].clone())
        cur = 0
        for i in range(1, 8):
            k, s = VQ_KERNELS[i], VQ_STRIDES[i]
            src, dst = bufs[cur], bufs[1 - cur]
            plan = ops.rows_plan(B, fr[i], 0, 0, C)
            ops.igemm_fwd(plan, src, p["w"][i], dst, Nimg=B, in_pix=rows[i - 1] // s, Ci=k * C, in_pitch=s * C, Co=C, out_pix=rows[i],
                          out_pitch=C, flops=2.0 * B * fr[i] * C * k * C)
            ops.vq_gn_partial(dst, B, fr[i], rows[i], part)
            ops.vq_gn_relu(dst, B, fr[i], rows[i], p["g"][i], p["be"][i], VQ_EPS, part, log=i == 7)
            if layers_out is not None:
                layers_out.append(dst[: B * rows[i] * C].view(B, rows[i], C)[:, : fr[i]].clone())
            cur = 1 - cur
        ze = torch.empty(B * F, C, dtype=torch.float32, device=dev)
        qpart = torch.empty(ops.vq_part_floats(B, F, 1), dtype=torch.float32, device=dev)
        ops.vq_project(bufs[cur], B, F, p["pw"], ze, qpart)
        if layers_out is not None:
            layers_out.append(ze.view(B, F, C).clone())
        tok = torch.empty(B * keep * GROUPS, dtype=torch.int64, device=dev)
        ops.vq_assign(ze, B, F, keep, p["pg"], p["pb"], VQ_EPS, qpart, p["emb"], p["e2"], tok, scores_out=scores_out)
        return tok.view(B, keep, GROUPS)

    def workspace_bytes(self, B: int, L: int) -> int:
        """Device bytes one call allocates for B clips of L samples (padding included): the two ping-pong buffers, the projection, the
        GroupNorm partials, the tokens."""
        fr = vq_frame_counts(L)
        rows = self._rows(fr)
        slack = max(VQ_KERNELS[1:]) * C
        n = 2 * (B * rows[0] * C + slack) + 2 * (B * rows[1] * C + slack) + 4 * B * fr[-1] * C + B * fr[-1] * GROUPS * 8
        return n + 4 * (ops.vq_part_floats(B, fr[0], 0) + ops.vq_part_floats(B, fr[-1], 1))
