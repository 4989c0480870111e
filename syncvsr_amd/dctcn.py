"""HIP-native twin of the reference's ``DCTCNLightningModule`` (``LRW/video/src/lightning.py:226-334``): the word-level model of
``LRW/video/config/dc-tcn-base.yaml`` — Conv3d stem + Swish ResNet18 (the front-end the LRS model already runs, ``model._frontend_forward``)
followed by the densely connected temporal convolution network (``tcn/models/densetcn.py``) with squeeze-and-excitation gates, the masked-mean
consensus and the two heads.

EVAL / INFERENCE PATH (``validation_step`` / ``test_step`` / ``inference.py``) and, in the same statistics mode, the gradients of the temporal
network and the two heads (``loss_and_backend_grads``: fine-tuning with the front-end and the BatchNorm statistics frozen) — or, with
``train_stats=True``, in the reference's training arithmetic for the back-end: batch-statistic BatchNorm1d (over the chomped positions of
the full-padding convolutions too), dropout0 / dropout1, mixup; the front-end stays frozen in eval statistics there.

WHOLE-MODEL TRAINING (``training_step``): ``loss_and_grads`` runs the front-end on batch statistics too (``model._frontend_forward`` in
training mode: the stem's BatchNorm3d, every BatchNorm2d, the pooling arg-max windows kept), the taped back-end walk on those features, the
back-end's backward and then ``model._frontend_backward`` from the gradient of the features: every parameter's ``.grad`` is a view of the
store's flat fp32 gradient buffer and every running statistic is updated.  ``dctcn_train.DCTCNTrainStep`` puts mixup's draw, the device
input pipeline, the global-norm clip and the OneCycle AdamW launch (``svsr_adamw_onecycle_step``) around it.  All of it is entered on a
module in EVAL mode: the training arithmetic is an entry point, not a mode, and a forward under ``.train()`` raises NotImplementedError —
it never runs a wrong forward silently.  The train step also runs data-parallel ranks (an engine.GradReducer fed by the backward's
gradient-ready notifications) and gradient accumulation over windows of micro-steps.  Not built: native step lists, HIP-graph capture.

ONE WALK, TWO STAGE SETS.  ``_backend`` is the only function that walks the network forward (transition0 -> per dense layer: SE gates, first
stage, downsample, second stage -> transitions) and ``_backward`` the only one that walks it back; both serve every entry point in either
statistics mode.  What depends on the mode sits below the walks, in two small classes with one signature per function: ``_RunningStats`` and
``_BatchStats`` each hold a stage forward, a stage backward, norm5's coefficients and norm5's data gradient.  ``_run`` picks the set once per
call; the walks never ask which one they hold.  A stage's static description (kernel sizes, dilation, widths, parameter names, forward
branch tables, transposed shadows) is built once in ``_prepare`` / ``_prepare_bwd``; a taped forward leaves one record per stage under
``tape["rec"]`` (keys ``"t0"``, ``(layer, 0)``, ``(layer, 1)``, ``("tr", block)``, ``"norm5"``).

Back-end layout (csrc/dctcn.hip): channels-last bf16 rows; ONE [B*T, reduced + layers * growth] buffer per dense block is the feature
stack (a layer reads a channel prefix through the row pitch and writes its channels at an offset: no ``torch.cat``).  Per layer: one launch
for the three gates (svsr_tcn_se_fwd), one for the three gated first-stage branches, one for the 1x1 downsample, one for the three
second-stage branches with ``Swish(out1 + res)`` in the epilogue (svsr_tconv_fwd).  BatchNorm(eval) and the conv bias are a per-channel fp32
scale / shift applied to the fp32 accumulator; the bf16 weights are never scaled.

Reference defects resolved here: ``self.vq_groups`` is never set there (2, as TransformerLightningModule); the module reads
``config.optim.loss_audio_weight`` while the yaml has ``optim.lambda_audio`` (either is accepted); fairseq is not imported — audio tokens
arrive pre-tokenised or, after ``attach_audio_codec(audio_codec.VqWav2VecCodec...)``, as float waveforms tokenised on the device; without
that codec ``load_state_dict`` ignores ``wav2vec.*`` keys (as inference.py's strict=False does) while staying strict about everything else.
"""
from __future__ import annotations

from typing import Any, Optional

import torch

from . import dropout, ops
from .config import Config
from .dctcn_init import (SE_REDUCTION, TCN, dctcn_buffer_specs, dctcn_dims, dctcn_init_state_dict, dctcn_layers, dctcn_param_specs)
from .model import _frontend_backward, _frontend_forward, _ParamStore, _ready, _StoreModule

BF16 = torch.bfloat16


def _unsupported(config: Config) -> list[str]:
    """Every reason this configuration cannot run, together (as lrs_model.E2E lists them)."""
    why: list[str] = []
    d = config.model.dctcn
    if str(d.get("modality", "video")) != "video":
        why.append("modality must be video")
    if str(d.get("backbone_type", "resnet")) != "resnet":
        why.append("backbone_type must be resnet (the ResNet18 trunk is the one front-end built here)")
    if str(d.get("relu_type", "prelu")) != "swish":
        why.append("relu_type must be swish (the shipped dc-tcn-base.yaml)")
    if float(d.get("width_mult", 1.0)) != 1.0:
        why.append("width_mult must be 1.0")
    if bool(d.get("extract_feats", False)):
        why.append("extract_feats is not supported (it returns the front-end features and skips the temporal network)")
    if d.get("tcn_options"):
        why.append("tcn_options (the multi-branch TCN back-end) is not built: use densetcn_options")
    o = d.get("densetcn_options")
    if not o:
        why.append("densetcn_options is required")
        return why
    ks, ds = [int(v) for v in o.kernel_size_set], [int(v) for v in o.dilation_size_set]
    blocks, growth, reduced = [int(v) for v in o.block_config], [int(v) for v in o.growth_rate_set], int(o.reduced_size)
    if not 1 <= len(ks) <= 3:
        why.append("kernel_size_set must hold one to three kernel sizes (svsr_tconv_fwd takes up to three branches per launch)")
    if len(growth) != len(blocks):
        why.append("growth_rate_set needs one entry per block")
        return why
    if not bool(o.squeeze_excitation):
        why.append("squeeze_excitation must be true (the shipped configuration)")
    if reduced % 64:
        why.append("reduced_size must be a multiple of 64")
    for bi, nl in enumerate(blocks):
        g = growth[bi]
        if g % len(ks) or (g // len(ks)) % 64:
            why.append(f"growth rate {g} of block {bi + 1}: every branch must be a multiple of 64 channels wide")
            continue
        for li in range(nl):
            n_in, dl = reduced + li * g, ds[li % len(ds)]
            for k in ks:
                if not (ops.tconv_ok(n_in, g // len(ks), k, dl) and ops.tconv_ok(g, g // len(ks), k, dl)):
                    why.append(f"block {bi + 1} layer {li + 1}: kernel size {k} with dilation {dl} on {n_in} channels is outside what svsr_tconv_fwd "
                               f"takes (odd k <= 7, (k - 1) * d / 2 <= {ops.TCONV_MAX_HALO}, channels a multiple of 64)")
    return why


class DCTCNLightningModule(_StoreModule):
    def __init__(self, config: Config, seed: Optional[int] = None):
        super().__init__()
        if not isinstance(config, Config):
            config = Config(config)
        self.config = config
        why = _unsupported(config)
        if why:
            raise NotImplementedError("; ".join(why))
        self.dims = dctcn_dims(config)
        self.audio_alignment, self.vq_groups, self.audio_vocab_size = self.dims["A"], self.dims["G"], self.dims["V"]
        self.codec = "vq"                    # vq-wav2vec tokens, pre-computed or from an attached audio_codec.VqWav2VecCodec
        optim = config.get("optim", Config())
        w = optim.get("loss_audio_weight", optim.get("lambda_audio"))         # the module reads the first, the shipped yaml holds the second
        if w is None:
            raise ValueError("config.optim needs loss_audio_weight or lambda_audio")
        self.lambda_audio = float(w)
        self.mixup_alpha = float(optim.get("mixup_alpha", 0.0))
        self.label_smoothing = float(config.get_path("train.label_smoothing", 0.0))
        self.use_boundary = bool(config.model.dctcn.use_boundary)
        self._attach_state(dctcn_param_specs(config), dctcn_buffer_specs(config), dctcn_init_state_dict(config, seed=0 if seed is None else seed))
        self.stem_name, self.trunk_name = "model.frontend3D", "model.trunk"
        self.stem_act = self.trunk_act = ops.ACT_SWISH                        # tcn/model.py:118-119, tcn/models/resnet.py with relu_type swish
        self._prep: Optional[dict] = None
        self._last: dict[str, Any] = {}
        self._n_cache: dict = {}
        self.eval()

    # ------------------------------------------------------------------------------------------------
    takes_vq_waveforms = True

    @staticmethod
    def _fwd_rank(name: str) -> int:
        return 0 if name.startswith("model.frontend3D") else 1 if name.startswith("model.trunk") else 2

    def _transposed_entries(self, offsets) -> list:
        return []                    # none in the store: the back-end's backward builds its transposed, tap-flipped shadows itself (_prepare_bwd)

    def mark_params_dirty(self) -> None:
        """Call after changing parameters or buffers in place: the bf16 shadows, the tap-major convolution weights and the folded BatchNorm
        coefficients are rebuilt at the next forward (load_state_dict and .to(device) do this themselves)."""
        self._prep = None
        super().mark_params_dirty()

    def store(self) -> _ParamStore:
        old = self._store
        if super().store() is not old:
            self._prep = None
        return self._store

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Without an attached codec `wav2vec.*` keys (the frozen codec of a reference checkpoint) are ignored — with one they are its buffers
        (the aggregator and prediction heads, which it does not hold, still are); everything else is checked as `strict` says."""
        codec = self._modules.get("wav2vec")
        own = () if codec is None else tuple("wav2vec." + k for k in codec.state_dict())
        kept = {k: v for k, v in state_dict.items() if not k.startswith("wav2vec.") or k in own}
        return super().load_state_dict(kept, strict=strict, assign=assign)

    # ------------------------------------------------------------------------------------------------
    def _bn_affine(self, st: _ParamStore, bn: str, bias: Optional[str]):
        """BatchNorm1d(eval) after a convolution with bias -> fp32 (scale, shift) for the accumulator: y = scale * acc + shift."""
        scale = st.p32(f"{bn}.weight") * torch.rsqrt(st.buffers[f"{bn}.running_var"] + ops.BN_EPS)
        shift = st.p32(f"{bn}.bias") - st.buffers[f"{bn}.running_mean"] * scale
        if bias is not None:
            shift = shift + st.p32(bias) * scale
        return scale.contiguous(), shift.contiguous()

    def _w16(self, st: _ParamStore, name: str, pad_to: Optional[int] = None) -> torch.Tensor:
        """bf16 shadow of Conv1d weight [co, ci, k] as tap-major [co, k, ci] (ci zero-padded to pad_to)."""
        shape = st.offsets[name][2]
        w = st.s16(name).view(shape).permute(0, 2, 1)
        if pad_to is not None and pad_to != shape[1]:
            out = torch.zeros((shape[0], shape[2], pad_to), dtype=BF16, device=w.device)
            out[:, :, : shape[1]] = w
            return out
        return w.contiguous()

    def _stage(self, st: _ParamStore, convs, *, n_in: int, co: int, d: int, act: int, out_off: int = 0, pad_to: Optional[int] = None, slope=None,
               drop_site: Optional[str] = None) -> dict:
        """The static description of one convolution stage, built once and read by both walks and both statistics modes.  convs: per branch
        (k, conv, BatchNorm, conv bias or None) by parameter name; branch j writes channels [out_off + j * co, out_off + (j + 1) * co) of the
        stage's output rows.  branches: what ops.tconv_fwd takes (the folded running-statistic scale / shift included); _prepare_bwd adds the
        transposed shadows (wt) and the stage-wide scale / shift vectors."""
        brs = []
        for j, (k, conv, bn, bias) in enumerate(convs):
            sc, sh = self._bn_affine(st, bn, bias)
            brs.append(dict(k=k, w=self._w16(st, f"{conv}.weight", pad_to), scale=sc, shift=sh, slope=slope, out_off=out_off + j * co, res_off=j * co))
        return dict(ks=[c[0] for c in convs], d=d, co=co, n_in=n_in, act=act, slope=slope, out_off=out_off, drop_site=drop_site, branches=brs,
                    weights=[f"{c[1]}.weight" for c in convs], norms=[c[2] for c in convs], biases=[c[3] for c in convs])

    @staticmethod
    def _stages(P: dict):
        yield P["t0"]
        for L in P["layers"]:
            yield from L["stages"]
        yield from P["trans"].values()

    @staticmethod
    def _fold_stage(D: dict) -> None:
        """The stage-wide BatchNorm(eval) vectors the epilogue backward reads: the branches' scale / shift side by side."""
        brs = D["branches"]
        one = len(brs) == 1
        D["scale"] = brs[0]["scale"] if one else torch.cat([br["scale"] for br in brs]).contiguous()
        D["shift"] = brs[0]["shift"] if one else torch.cat([br["shift"] for br in brs]).contiguous()

    def _prepare(self, st: _ParamStore, fold: bool = True) -> dict:
        """fold=False (the batch-statistic path): the folded running-statistic coefficients are not needed; after a train_stats step they are
        stale (P["folded"] False) and only a caller that reads them pays for folding them again (_refold)."""
        if self._prep is not None:
            if fold and not self._prep["folded"]:
                self._refold(st, self._prep)
            return self._prep
        st.refresh_shadows()
        st.shadow_fresh = True          # eval only: nothing but load_state_dict / mark_params_dirty changes a weight
        dm, dev = self.dims, st.device
        ks, R = dm["ks"], dm["reduced"]
        P: dict[str, Any] = {}
        p = f"{TCN}.transition0"
        self.in_pad = (dm["in_size"] + 63) // 64 * 64
        P["t0"] = self._stage(st, [(1, f"{p}.conv", f"{p}.norm", None)], n_in=self.in_pad, co=R, d=1, act=ops.ACT_PRELU, pad_to=self.in_pad,
                              slope=st.p32(f"{p}.prelu.weight"))
        layers, trans = dctcn_layers(self.config)
        P["layers"], li = [], 0
        for p, n_in, g, d, bi in layers:
            gb = g // len(ks)
            li = li + 1 if P["layers"] and P["layers"][-1]["bi"] == bi else 1
            L: dict[str, Any] = dict(p=p, n_in=n_in, g=g, bi=bi)
            L["se_w1"] = torch.stack([st.s16(f"{p}.cbcr0_se_{i}.fc.0.weight").view(n_in // SE_REDUCTION, n_in) for i in range(len(ks))]).contiguous()
            L["se_w2"] = torch.stack([st.s16(f"{p}.cbcr0_se_{i}.fc.2.weight").view(n_in, n_in // SE_REDUCTION) for i in range(len(ks))]).contiguous()
            L["stages"] = [self._stage(st, [(k, f"{p}.cbcr{s}_{i}.net.0", f"{p}.cbcr{s}_{i}.net.1", f"{p}.cbcr{s}_{i}.net.0.bias") for i, k in enumerate(ks)],
                                       n_in=g if s else n_in, co=gb, d=d, act=ops.ACT_SWISH, out_off=n_in if s else 0,
                                       drop_site=f"block{bi + 1}.layer{li}.drop{s}") for s in (0, 1)]
            L["down"] = dict(k=1, w=self._w16(st, f"{p}.downsample.weight"), scale=torch.ones(g, dtype=torch.float32, device=dev),
                             shift=st.p32(f"{p}.downsample.bias"), out_off=0)
            P["layers"].append(L)
        P["trans"] = {bi: self._stage(st, [(1, f"{name}.conv", f"{name}.norm", None)], n_in=n, co=R, d=1, act=ops.ACT_SWISH) for name, n, bi in trans}
        P["norm5"] = self._bn_affine(st, f"{TCN}.norm5", None)
        P["folded"] = True
        self._prep = P
        return P

    def _refold(self, st: _ParamStore, P: dict) -> None:
        """The BatchNorm(eval) coefficients of _prepare again, from the current running statistics; weights and shadows are kept."""
        for D in self._stages(P):
            for br, bn, bias in zip(D["branches"], D["norms"], D["biases"]):
                br["scale"], br["shift"] = self._bn_affine(st, bn, bias)
            if "bwd" in P:
                self._fold_stage(D)
        P["norm5"] = self._bn_affine(st, f"{TCN}.norm5", None)
        P["folded"] = True

    # ------------------------------------------------------------------------------------------------
    def _x0(self, feats: torch.Tensor, word_mask: Optional[torch.Tensor], B: int, T: int) -> torch.Tensor:
        """transition0's input rows: the features, with use_boundary the word-boundary column beside them (zero-padded to in_pad)."""
        if not self.use_boundary:
            return feats
        if word_mask is None:
            raise ValueError("use_boundary: word_mask [B, T] is required")
        x0 = torch.zeros((B * T, self.in_pad), dtype=BF16, device=feats.device)
        x0[:, :512] = feats
        x0[:, 512] = word_mask.reshape(B * T).to(BF16)
        return x0

    def _backend(self, S, feats: torch.Tensor, word_mask: Optional[torch.Tensor], B: int, T: int, keep: Optional[dict] = None,
                 tape: Optional[dict] = None):
        """feats bf16 [B*T, 512] -> the last block's feature stack bf16 [B*T, C] (before norm5): THE forward walk of the network.  S: the stage
        set of the call's statistics mode (_RunningStats / _BatchStats); with a tape what the backward reads is kept, one record per stage under
        tape["rec"]: "t0", (layer, 0), (layer, 1), ("tr", block), and "norm5" (_run)."""
        P, dm, dev, rec = self._prepare(S.st, fold=S.folds), self.dims, feats.device, None
        if tape is not None:
            rec = {}
            tape.update(rec=rec, layers=[], stacks=[], stats=S)          # (the set holds the model and the store, never the tape)
        R = dm["reduced"]
        x0 = self._x0(feats, word_mask, B, T)
        width = lambda bi: R + dm["blocks"][bi] * dm["growth"][bi]          # noqa: E731
        stack = torch.empty((B * T, width(0)), dtype=BF16, device=dev)
        S.stage(rec, "t0", P["t0"], x0, stack, B=B, T=T)
        if tape is not None:
            tape["x0"] = x0
            tape["stacks"].append(stack)
        if keep is not None:
            keep["transition0"] = stack[:, :R].float().view(B, T, R)
        nlayers = len(P["layers"])
        for i, L in enumerate(P["layers"]):
            n_in, g, bi = L["n_in"], L["g"], L["bi"]
            gates = ops.tcn_se_fwd(stack, L["se_w1"], L["se_w2"], B=B, T=T, n_in=n_in)
            out0 = torch.empty((B * T, g), dtype=BF16, device=dev)
            S.stage(rec, (i, 0), L["stages"][0], stack, out0, B=B, T=T, gates=gates)
            res = torch.empty((B * T, g), dtype=BF16, device=dev)
            ops.tconv_fwd(stack, B=B, T=T, n_in=n_in, d=1, branches=[L["down"]], co=g, act=ops.ACT_NONE, out=res)
            S.stage(rec, (i, 1), L["stages"][1], out0, stack, B=B, T=T, res=res, res_act=ops.ACT_SWISH)
            if tape is not None:
                tape["layers"].append(dict(stack=stack, gates=gates, out0=out0, res=res))
            if i + 1 == nlayers or P["layers"][i + 1]["bi"] != bi:
                if keep is not None:
                    keep[f"denseblock{bi + 1}"] = stack.float().view(B, T, -1)
                if bi in P["trans"]:
                    nxt = torch.empty((B * T, width(bi + 1)), dtype=BF16, device=dev)
                    S.stage(rec, ("tr", bi), P["trans"][bi], stack, nxt, B=B, T=T)
                    stack = nxt
                    if tape is not None:
                        tape["stacks"].append(stack)
        return stack

    def _run(self, videos: torch.Tensor, word_mask, attention_mask, keep: Optional[dict] = None, tape: Optional[dict] = None,
             feats: Optional[torch.Tensor] = None, train: Optional[dict] = None):
        """feats (bf16 [B*T, 512], with videos = the (B, T) pair): the front-end is skipped (loss_and_backend_grads_from_features).
        train (loss_and_backend_grads(train_stats=True), loss_and_grads): the back-end runs on batch statistics (_BatchStats); the front-end
        does too when train carries a tape for it (train["fe_tape"]: loss_and_grads), otherwise it stays in eval statistics.  The statistics
        mode is picked here, once per call; the walks only call the stage set."""
        if self.training:
            raise NotImplementedError("DCTCNLightningModule: a forward under .train() is not built: call .eval() first; the whole model trains "
                                      "through loss_and_grads / dctcn_train.DCTCNTrainStep and the back-end alone through "
                                      "loss_and_backend_grads(train_stats=True), both on a module in eval mode")
        src = videos if feats is None else feats
        if src.device.type != "cuda":
            raise RuntimeError("syncvsr_amd runs on an MI355X HIP device only; there is no CPU fallback")
        if feats is None:
            if videos.dim() != 5 or videos.size(1) != 1:
                raise ValueError("videos must be [B, 1, T, H, W]")
            B, _, T = videos.shape[:3]
        else:
            B, T = videos
            if feats.dtype != BF16 or tuple(feats.shape) != (B * T, 512) or not feats.is_contiguous():
                raise ValueError("features must be a contiguous bf16 [B*T, 512] tensor")
        st = self.store()
        S = _RunningStats(self, st) if train is None else _BatchStats(self, st, train)
        self._prepare(st, fold=S.folds)
        C = self.dims["out_size"]
        with torch.no_grad():
            if feats is None:
                fe_tape = None if train is None else train.get("fe_tape")          # batch statistics, pooling windows kept: loss_and_grads
                feats = _frontend_forward(self, st, {} if fe_tape is None else fe_tape, videos.float().contiguous(), fe_tape is not None)
                if tape is not None:
                    tape["feats"] = feats
            stack = self._backend(S, feats, word_mask, B, T, keep, tape)
            scale, shift = S.norm5(None if tape is None else tape["rec"], stack, B, T)
            if attention_mask is None:
                attention_mask = torch.ones((B, T), dtype=torch.float32, device=src.device)
            mask = attention_mask.to(torch.float32).contiguous()
            h, pooled = ops.tcn_norm_pool_fwd(stack, scale, shift, mask, B=B, T=T, C=C)
            if tape is not None:
                tape.update(mask=mask, pooled=pooled, B=B, T=T)
            logits_c, _ = ops.linear_fwd(pooled, st.s16("video_classifier.weight"), st.p32("video_classifier.bias"), rows=B, K=C,
                                         N=self.dims["classes"], x_pitch=C, out_f32=True)
        return st, h, logits_c

    def features(self, videos: torch.Tensor, word_mask: Optional[torch.Tensor] = None, keep: Optional[dict] = None) -> torch.Tensor:
        """last_hidden_states of the reference, time-major: fp32 [B, T, C] (C = 1664 for the shipped configuration)."""
        B, _, T = videos.shape[:3]
        _, h, _ = self._run(videos, word_mask, None, keep)
        return h.float().view(B, T, -1)

    def predict(self, videos: torch.Tensor, word_mask: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 word logits [B, num_classes] (what inference.py takes the argmax of)."""
        return self._run(videos, word_mask, attention_mask)[2]

    def forward(self, videos: torch.Tensor, audios: torch.Tensor, labels: torch.Tensor, word_mask: torch.Tensor,
                attention_mask: torch.Tensor) -> dict[str, torch.Tensor]:
        """lightning.py:255-312 in eval mode (lam = 0).  audios: pre-computed vq-wav2vec tokens int64 [B, >= A*T, 2], or, with the tokeniser
        attached (attach_audio_codec), float waveforms [B, L] / [B, 1, L] on the device."""
        return self._losses(videos, audios, labels, word_mask, attention_mask, None)

    def _losses(self, videos, audios, labels, word_mask, attention_mask, tape: Optional[dict], feats=None,
                train: Optional[dict] = None) -> dict[str, torch.Tensor]:
        """The eval forward; with a tape (loss_and_backend_grads) the same launches keep what the backward reads."""
        B, T = (videos.shape[0], videos.shape[2]) if feats is None else videos
        A, G, V = self.audio_alignment, self.vq_groups, self.audio_vocab_size
        if tuple(labels.shape) != (B,):          # (the cross-entropy kernels read B labels: checked here, before anything is launched)
            raise ValueError(f"labels must be [B] = [{B}], got {list(labels.shape)}")
        audios = self._tokenize_waveforms(audios, T * A)
        if audios.dtype != torch.int64 or audios.dim() != 3 or audios.size(2) != G:
            raise ValueError("pass pre-computed audio tokens int64 [B, >= A*T, 2] in the `audios` slot (no audio tokeniser is attached)")
        if audios.size(1) < T * A:
            raise ValueError(f"audio tokens have {audios.size(1)} steps, need >= {T * A}")
        st, h, logits_c = self._run(videos, word_mask, attention_mask, None, tape, feats, train)
        lam = 0.0 if train is None else train["lam"]
        C, NA = self.dims["out_size"], A * G * V
        with torch.no_grad():
            lab = labels.long().contiguous()
            loss_c, lse_c = ops.ce_fwd(logits_c, self.dims["classes"], lab, None, B, self.dims["classes"], self.label_smoothing)
            tok = audios[:, : T * A].contiguous().reshape(-1)
            # (the logits are stored: svsr_linear_ce_ok takes K up to 576, the shipped width is 1664)
            logits_a, _ = ops.linear_fwd(h, st.s16("audio_projection.weight"), st.p32("audio_projection.bias"), rows=B * T, K=C, N=NA, x_pitch=C)
            loss_a, lse_a = ops.ce_fwd(logits_a, V, tok, None, B * T * A * G, V, 0.0)
            if lam:          # mixup (lightning.py:278-298): both losses lerp towards the rolled targets' (the same kernels, called twice)
                lab2, tok2 = lab.roll(1, 0).contiguous(), audios[:, : T * A].roll(1, 0).contiguous().reshape(-1)
                loss_c = torch.lerp(loss_c, ops.ce_fwd(logits_c, self.dims["classes"], lab2, None, B, self.dims["classes"], self.label_smoothing)[0], lam)
                loss_a = torch.lerp(loss_a, ops.ce_fwd(logits_a, V, tok2, None, B * T * A * G, V, 0.0)[0], lam)
                if tape is not None:
                    tape.update(lab2=lab2, tok2=tok2, lam=lam)
            acc = ops.topk_acc(logits_c, lab, None)
            loss_total = ops.lincomb2(loss_c, loss_a, self.lambda_audio)
        self._last = dict(last_hidden_states=h, logits_category=logits_c, logits_audio=logits_a)
        if tape is not None:
            tape.update(st=st, h=h, logits_c=logits_c, logits_a=logits_a, lab=lab, tok=tok, lse_c=lse_c, lse_a=lse_a)
        return {"loss_total": loss_total, "loss_category": loss_c, "loss_audio": loss_a, "accuracy_top1": acc[0], "accuracy_top5": acc[1]}

    # ------------------------------------------------------------------------------------------------
    # backward of the back-end and the two heads, in the statistics mode its forward ran in
    # ------------------------------------------------------------------------------------------------
    def backend_parameters(self) -> list:
        """The nn.Parameters loss_and_backend_grads fills: everything but the front-end, in state-dict order."""
        return [p for n, p in self.named_parameters() if self._fwd_rank(n) == 2]

    def _prepare_bwd(self, st: _ParamStore, fold: bool = True) -> dict:
        """Transposed, tap-flipped shadows for the data gradients and the stage-wide BatchNorm vectors, stored with each stage's description
        (rebuilt with _prepare's); -> the heads' transposed weights."""
        P = self._prepare(st, fold)
        if "bwd" in P:
            return P["bwd"]
        dev = st.device
        wt = lambda name: ops.tconv_wt(st.s16(name).view(st.offsets[name][2]))          # noqa: E731
        Q: dict[str, Any] = {}
        for D in self._stages(P):
            D["wt"] = [wt(name) for name in D["weights"]]
            self._fold_stage(D)
        w = torch.zeros((self.in_pad, 1, self.dims["reduced"]), dtype=BF16, device=dev)          # transition0's, zero rows for the padding
        w[: self.dims["in_size"]] = P["t0"]["wt"][0]
        P["t0"]["wt"] = [w]
        for L in P["layers"]:
            L["down_wt"] = wt(f"{L['p']}.downsample.weight")

        def head_t(name):                    # [N, K] -> [K, N padded to 64] for ops.linear_dgrad
            N, K = st.offsets[name][2]
            out = torch.zeros((K, (N + 63) // 64 * 64), dtype=BF16, device=dev)
            out[:, :N] = st.s16(name).view(N, K).t()
            return out
        Q["wc_t"], Q["wa_t"] = head_t("video_classifier.weight"), head_t("audio_projection.weight")
        P["bwd"] = Q
        return Q

    def _grad_of(self, st: _ParamStore, name: str, accumulate: bool):
        """-> (the fp32 gradient buffer of `name` in the parameter's own layout, add?).  The buffer is the store's; a .grad that is None or a
        foreign tensor is replaced by it (a foreign one's values are carried over when accumulating)."""
        p = st._params[name]
        view = st._view(st.grad, name)
        if accumulate and p.grad is None:
            view.zero_()          # nothing to add to: every tensor of one call then shares one flag (the SE launch writes six of them)
        elif accumulate and p.grad.data_ptr() != view.data_ptr():
            view.copy_(p.grad)
        p.grad = view
        return view, accumulate

    @staticmethod
    def _put(dst: torch.Tensor, add: bool, val: torch.Tensor) -> None:
        if add:
            dst.add_(val.view(dst.shape))
        else:
            dst.copy_(val.view(dst.shape))

    def _bn_grads(self, st, accumulate, sums, bn: str, bias: Optional[str], lo: int = 0, hi: Optional[int] = None) -> None:
        s0, s1 = sums[0, lo:hi], sums[1, lo:hi]
        dw, db, dcb = ops.bn_conv_param_grads(s0, s1, st.p32(f"{bn}.weight"), st.buffers[f"{bn}.running_mean"], st.buffers[f"{bn}.running_var"],
                                             None if bias is None else st.p32(bias))
        self._put(*self._grad_of(st, f"{bn}.weight", accumulate), dw)
        self._put(*self._grad_of(st, f"{bn}.bias", accumulate), db)
        if bias is not None:
            self._put(*self._grad_of(st, bias, accumulate), dcb)

    def _loss_and_grads(self, videos, audios, labels, word_mask, attention_mask, loss_scale, accumulate, want_input_grad, feats=None,
                        train_stats: bool = False, dropout_seed: Optional[int] = None, lam: float = 0.0, videos_mixed: bool = False,
                        whole: bool = False):
        """whole (loss_and_grads; train_stats and want_input_grad are then on): the front-end runs on batch statistics too and its backward
        follows the back-end's."""
        tape: dict[str, Any] = {}
        train = None
        if videos_mixed and not train_stats:
            raise ValueError("videos_mixed belongs to train_stats=True, like lam (the eval-statistics gradients have no mixup)")
        if train_stats:
            lam = float(lam)
            if not 0.0 <= lam <= 1.0:
                raise ValueError("lam must lie in [0, 1]")
            p = float(self.config.model.dctcn.densetcn_options.get("dropout", 0.0)) if dropout_seed is not None else 0.0
            train = dict(lam=lam, seed=None if dropout_seed is None else int(dropout_seed), p=p)
            if whole:
                train["fe_tape"] = {}
                self._drop_backward_state()          # what a call that aborted between its forward and the end of its backward left behind
            if lam and feats is None and not videos_mixed:
                videos = torch.lerp(videos.float(), videos.float().roll(1, 0), lam)          # (word boundaries are not mixed)
        elif dropout_seed is not None or float(lam) != 0.0:
            raise ValueError("dropout_seed and lam belong to train_stats=True (the eval-statistics gradients have no dropout and no mixup)")
        out = self._losses(videos, audios, labels, word_mask, attention_mask, tape, feats, train)
        with torch.no_grad():
            gf = self._backward(tape, float(loss_scale), bool(accumulate), bool(want_input_grad))
            if whole:
                # the back-end walk wrote the last of its parameters (transition0): everything above the front-end in the decayed region is
                # final, and a reducer sends those buckets while the front-end's backward runs (no hook attached: nothing happens)
                _ready(self, tape["st"], self._backend_first(tape["st"]))
                self._frontend_grads(tape["st"], train["fe_tape"], gf, bool(accumulate))
                out["features"] = tape["feats"]
            if train is not None:
                self._update_running(tape)
        if want_input_grad:
            out["grad_features"] = gf
        return out

    def _frontend_spans(self, st: _ParamStore) -> list:
        """The front-end's parameters as merged [lo, hi) element ranges of the flat buffers (two: its convolution weights open the decayed
        region, its BatchNorm vectors the other one)."""
        spans = st._vc.get("fe_spans")          # (kept with the store's cached views: the offsets never change while the store lives)
        if spans is None:
            spans = []
            for lo, n in sorted(st.offsets[name][:2] for name, _, _ in self._specs if self._fwd_rank(name) < 2):
                if spans and lo - spans[-1][1] < 4:          # (every tensor starts on a 16-byte boundary: up to three pad elements between two)
                    spans[-1][1] = lo + n
                else:
                    spans.append([lo, lo + n])
            st._vc["fe_spans"] = spans
        return spans

    def _backend_first(self, st: _ParamStore) -> str:
        """The decayed tensor that opens the back-end's part of the flat buffers (at st.front_end): what the gradient-ready notification
        behind the back-end's backward names."""
        name = st._vc.get("be_first")
        if name is None:
            name = st._vc["be_first"] = min((st.offsets[n][0], n) for n, s, _ in self._specs if len(s) >= 2 and self._fwd_rank(n) == 2)[1]
        return name

    def _frontend_grads(self, st: _ParamStore, fe_tape: dict, grad_features: torch.Tensor, accumulate: bool) -> None:
        """model._frontend_backward from the gradient of the features: every launch of it ADDS into the flat gradient buffer, so the
        front-end's ranges are zero-filled first (accumulate: left as they are, with _grad_of's rule for a .grad that is None or foreign).
        The weight-gradient side stream stays off: the launches run in line, and the trunk's chain of 3x3 weight gradients is closed by
        _frontend_backward itself (model._flush_w3_chain) before the stem.  The gradient-ready notifications are no-ops unless a reducer is
        attached (dctcn_train.DCTCNTrainStep under data parallelism).  The buckets it then has in flight hold back-end gradients only (the
        notification behind _backward names the front-end's upper edge), and the zero-fill below touches front-end ranges only — the bottom
        of the decayed region and the front-end's BatchNorm vectors in the 1-D tail, which no bucket holds before on_ready(0) — so it races
        none of them; keep it that way."""
        for name, _, _ in self._specs:
            if self._fwd_rank(name) < 2:
                self._grad_of(st, name, accumulate)
        if not accumulate:
            for lo, hi in self._frontend_spans(st):
                ops.memset(st.grad[lo:hi], 0)
        _frontend_backward(self, st, fe_tape, grad_features)
        if self._w3_pending is not None:          # (cannot happen: _frontend_backward flushes; a gradient left in slabs would be silently short)
            raise RuntimeError("loss_and_grads: a 3x3 weight-gradient chain is still pending")

    def loss_and_grads(self, videos: torch.Tensor, audios: torch.Tensor, labels: torch.Tensor, word_mask: torch.Tensor,
                       attention_mask: torch.Tensor, loss_scale: float = 1.0, accumulate: bool = False, dropout_seed: Optional[int] = None,
                       lam: float = 0.0, videos_mixed: bool = False) -> dict[str, torch.Tensor]:
        """The reference's training_step arithmetic for the WHOLE model, on a module in eval mode (as loss_and_backend_grads(train_stats=True)
        is): model._frontend_forward in training mode (batch statistics in the stem's BatchNorm3d and every BatchNorm2d, the pooling arg-max
        windows kept), the taped back-end walk on batch statistics over those features, the back-end's backward, then
        model._frontend_backward from the gradient of the features.  Afterwards EVERY nn.Parameter has .grad = d(loss_total * loss_scale) /
        d(param), a view of the store's flat fp32 gradient buffer (accumulate=True adds, with _grad_of's rule); the running statistics of
        all BatchNorms are updated as a .train() forward of the reference updates them (momentum 0.1, unbiased variance,
        num_batches_tracked: the front-end's inside its forward, the back-end's when the backward is through) and the folded eval
        coefficients are stale until the next eval forward folds them again.  dropout_seed / lam / videos_mixed: as
        loss_and_backend_grads(train_stats=True); mixup lerps the clips ahead of the front-end.  Beside the five metrics the dict carries
        "features" (bf16 [B*T, 512], the training-mode front-end features) and "grad_features" (their gradient)."""
        return self._loss_and_grads(videos, audios, labels, word_mask, attention_mask, loss_scale, accumulate, True, train_stats=True,
                                    dropout_seed=dropout_seed, lam=lam, videos_mixed=videos_mixed, whole=True)

    def loss_and_backend_grads(self, videos: torch.Tensor, audios: torch.Tensor, labels: torch.Tensor, word_mask: torch.Tensor,
                               attention_mask: torch.Tensor, loss_scale: float = 1.0, accumulate: bool = False,
                               want_input_grad: bool = False, train_stats: bool = False, dropout_seed: Optional[int] = None,
                               lam: float = 0.0, videos_mixed: bool = False) -> dict[str, torch.Tensor]:
        """The eval forward (the same launches: the metrics are forward()'s bits) followed by the hand-written backward of the temporal network
        and the two heads: afterwards every parameter of backend_parameters() has .grad = d(loss_total * loss_scale)/d(param) in fp32
        (accumulate=True adds to an existing .grad).  The front-end and every BatchNorm running statistic are frozen and untouched.  With
        want_input_grad the dict also carries "grad_features": bf16 [B*T, 512], the gradient of the front-end features.

        train_stats=True: the reference's TRAINING arithmetic for the back-end (the front-end stays frozen in eval statistics).  Every
        BatchNorm1d uses batch statistics — for the cbcr* norms over all B * (T + (k - 1) d) positions of the full-padding convolution, the
        chomped ones included, as the reference's Conv1d -> BatchNorm1d -> Chomp1d order has it; padded frames count (lengths=None) — and
        running_mean / running_var / num_batches_tracked are updated afterwards (momentum 0.1, unbiased variance).  The gradients carry the
        statistics' chain rule; a cbcr* conv bias cancels and its gradient is exact zeros.  dropout_seed: dropout0 / dropout1 of every dense
        layer with p = densetcn_options.dropout and the counter-based mask of dropout.py (sites: dropout.dctcn_sites).  lam: mixup, drawn by
        the caller: videos lerp towards videos.roll(1, 0), both losses towards the rolled targets' (lightning.py:264-299).  videos_mixed=True
        (train_stats only): the videos arrive already lerped with this lam (augment.DeviceDCTCNPipeline) and are taken as they are; the
        losses still mix."""
        return self._loss_and_grads(videos, audios, labels, word_mask, attention_mask, loss_scale, accumulate, want_input_grad,
                                    train_stats=train_stats, dropout_seed=dropout_seed, lam=lam, videos_mixed=videos_mixed)

    def loss_and_backend_grads_from_features(self, feats: torch.Tensor, B: int, T: int, audios: torch.Tensor, labels: torch.Tensor,
                                             word_mask: torch.Tensor, attention_mask: torch.Tensor, loss_scale: float = 1.0,
                                             accumulate: bool = False, want_input_grad: bool = False, train_stats: bool = False,
                                             dropout_seed: Optional[int] = None, lam: float = 0.0) -> dict[str, torch.Tensor]:
        """loss_and_backend_grads from pre-computed front-end features (bf16 [B*T, 512]) instead of videos: the frozen front-end need not
        run again for a clip whose features are cached (and what scripts/dctcn_bench.py --backward times).  With lam the features are those
        of already-mixed clips; the losses are mixed here."""
        return self._loss_and_grads((int(B), int(T)), audios, labels, word_mask, attention_mask, loss_scale, accumulate, want_input_grad, feats,
                                    train_stats=train_stats, dropout_seed=dropout_seed, lam=lam)

    def _heads_backward(self, tape: dict, loss_scale: float, accumulate: bool):
        """The two heads' parameter gradients -> (dh bf16 [B*T, C], dpooled bf16 [B, C]): the gradients of norm5's output and of the pooled row."""
        st: _ParamStore = tape["st"]
        Q, dm = self._prepare_bwd(st, fold=tape["stats"].folds), self.dims
        B, T, dev = tape["B"], tape["T"], st.device
        rows, C = B * T, dm["out_size"]
        A, G, V, NC = self.audio_alignment, self.vq_groups, self.audio_vocab_size, dm["classes"]
        NA, NCp = A * G * V, (NC + 63) // 64 * 64
        grad = lambda name: self._grad_of(st, name, accumulate)          # noqa: E731
        # heads: the cross-entropy and linear kernels the transformer model's heads run
        g_c = torch.full((), loss_scale, dtype=torch.float32, device=dev)
        g_a = torch.full((), loss_scale * self.lambda_audio, dtype=torch.float32, device=dev)
        dlc = torch.empty((B, NCp), dtype=BF16, device=dev)
        dla = torch.empty((rows, NA), dtype=BF16, device=dev)
        if "lab2" in tape:          # mixup: the two targets' gradients, weighted 1 - lam and lam, from the same kernel
            lam = tape["lam"]
            dlc2, dla2 = torch.zeros_like(dlc), torch.empty_like(dla)
            dlc.zero_()
            ops.ce_bwd(tape["logits_c"], NC, tape["lab"], None, B, NC, self.label_smoothing, tape["lse_c"], g_c * (1.0 - lam), dlc, NCp)
            ops.ce_bwd(tape["logits_c"], NC, tape["lab2"], None, B, NC, self.label_smoothing, tape["lse_c"], g_c * lam, dlc2, NCp)
            ops.ce_bwd(tape["logits_a"], V, tape["tok"], None, rows * A * G, V, 0.0, tape["lse_a"], g_a * (1.0 - lam), dla, V)
            ops.ce_bwd(tape["logits_a"], V, tape["tok2"], None, rows * A * G, V, 0.0, tape["lse_a"], g_a * lam, dla2, V)
            dlc.add_(dlc2)
            dla.add_(dla2)
        else:
            ops.ce_bwd(tape["logits_c"], NC, tape["lab"], None, B, NC, self.label_smoothing, tape["lse_c"], g_c, dlc, NCp)
            ops.ce_bwd(tape["logits_a"], V, tape["tok"], None, rows * A * G, V, 0.0, tape["lse_a"], g_a, dla, V)
        for wname, bname, x, dy, n_rows, N, pitch in (("audio_projection.weight", "audio_projection.bias", tape["h"], dla, rows, NA, NA),
                                                     ("video_classifier.weight", "video_classifier.bias", tape["pooled"], dlc, B, NC, NCp)):
            (gw, addw), (gb, addb) = grad(wname), grad(bname)
            if not addw:
                gw.zero_()
            if not addb:
                gb.zero_()
            ops.linear_wgrad(x, dy, gw, rows=n_rows, K=C, N=N, x_pitch=C, dy_pitch=pitch, db=gb)          # (adds)
        dh = ops.linear_dgrad(dla, Q["wa_t"], rows=rows, N=NA, K=C, dy_pitch=NA)
        dpooled = ops.linear_dgrad(dlc, Q["wc_t"], rows=B, N=NC, K=C, dy_pitch=NCp)
        return dh, dpooled

    def _dgrad(self, tape: dict, key, D: dict, dacc: torch.Tensor, *, B: int, T: int, out: torch.Tensor, gates=None, **kw):
        """The data gradient of stage `key` from the gradient of its accumulators (extended by the record's hmax under batch statistics;
        without a halo, as under running statistics, svsr_tconv_dgrad itself)."""
        brs = [dict(k=k, wt=D["wt"][j], dy_off=j * D["co"], gate=None if gates is None else gates[j]) for j, k in enumerate(D["ks"])]
        return ops.tconv_dgrad(dacc, B=B, T=T, co=D["co"], d=D["d"], n_out=D["n_in"], out=out, branches=brs, hmax=tape["rec"][key]["hmax"] or None, **kw)

    def _backward(self, tape: dict, loss_scale: float, accumulate: bool, want_input_grad: bool):
        """THE backward walk: the forward's in reverse, through the stage set the forward ran with (tape["stats"])."""
        S, rec = tape["stats"], tape["rec"]
        st: _ParamStore = S.st
        P, dm = self._prepare(st, fold=S.folds), self.dims
        self._prepare_bwd(st, fold=S.folds)
        B, T, dev = tape["B"], tape["T"], st.device
        rows, R, nb = B * T, dm["reduced"], len(dm["ks"])
        grad = lambda name: self._grad_of(st, name, accumulate)          # noqa: E731
        dh, dpooled = self._heads_backward(tape, loss_scale, accumulate)
        # norm5 + masked mean
        stacks = tape["stacks"]
        dS = S.norm5_bwd(rec.get("norm5"), dh, dpooled, stacks[-1], tape["mask"], accumulate, B=B, T=T)
        # dense blocks, last to first; dS: the gradient of the current block's feature stack
        for i in range(len(P["layers"]) - 1, -1, -1):
            L, t = P["layers"][i], tape["layers"][i]
            n_in, g, bi, p, (D0, D1) = L["n_in"], L["g"], L["bi"], L["p"], L["stages"]
            stack = t["stack"]
            # second stage: Swish(out1 + res) sends its gradient to out1's convolutions and to the downsample branch
            dacc1, dres, sums = S.stage_bwd(rec[(i, 1)], D1, dS[:, n_in: n_in + g], t["out0"], accumulate, B=B, T=T, res=t["res"], res_act=ops.ACT_SWISH)
            self._put(*grad(f"{p}.downsample.bias"), sums[3])
            dout0 = torch.empty((rows, g), dtype=BF16, device=dev)
            self._dgrad(tape, (i, 1), D1, dacc1, B=B, T=T, out=dout0)
            # first stage (gated)
            dacc0, _, _ = S.stage_bwd(rec[(i, 0)], D0, dout0, stack, accumulate, B=B, T=T, gates=t["gates"])
            gpart = self._dgrad(tape, (i, 0), D0, dacc0, B=B, T=T, out=dS, gates=t["gates"], x=stack, addend=dS)
            g1 = [grad(f"{p}.cbcr0_se_{j}.fc.0.weight") for j in range(nb)]
            g2 = [grad(f"{p}.cbcr0_se_{j}.fc.2.weight") for j in range(nb)]
            dmean = ops.tcn_se_bwd(stack, L["se_w1"], L["se_w2"], t["gates"], gpart, [a for a, _ in g1], [a for a, _ in g2], B=B, T=T, n_in=n_in,
                                   add=g1[0][1])
            # downsample branch; the time mean's gradient (constant over a clip's rows) rides in the same write
            gw, add = grad(f"{p}.downsample.weight")
            ops.tconv_wgrad(stack, dres, gw, B=B, T=T, n_in=n_in, co=g, k=1, d=1, add=add)
            ops.tconv_dgrad(dres, B=B, T=T, co=g, d=1, n_out=n_in, out=dS, addend=dS, cadd=dmean, cadd_scale=1.0 / T,
                            branches=[dict(k=1, wt=L["down_wt"], dy_off=0)])
            if i == 0 or P["layers"][i - 1]["bi"] != bi:          # the block's input: a transition's output
                if bi == 0:
                    break
                key, x = ("tr", bi - 1), stacks[bi - 1]
                dacc, _, _ = S.stage_bwd(rec[key], P["trans"][bi - 1], dS[:, :R], x, accumulate, B=B, T=T)
                dS = torch.empty_like(x)
                self._dgrad(tape, key, P["trans"][bi - 1], dacc, B=B, T=T, out=dS)
        # transition0 (PReLU)
        dacc, _, sums = S.stage_bwd(rec["t0"], P["t0"], dS[:, :R], tape["x0"], accumulate, B=B, T=T)
        self._put(*grad(f"{TCN}.transition0.prelu.weight"), sums[2])
        if not want_input_grad:
            return None
        dx0 = torch.empty((rows, self.in_pad), dtype=BF16, device=dev)
        self._dgrad(tape, "t0", P["t0"], dacc, B=B, T=T, out=dx0)
        return dx0[:, :512].contiguous()          # (the boundary column's own gradient is discarded)

    def _counts(self, B: int, T: int, hs: tuple, co: int, dev) -> torch.Tensor:
        """fp32 [len(hs) * co]: the positions B * (T + 2 h) a channel's statistics run over; built once per shape (a host-to-device copy)."""
        key = (B, T, hs, co, str(dev))
        if key not in self._n_cache:
            self._n_cache[key] = torch.tensor([float(B * (T + 2 * h)) for h in hs], dtype=torch.float32, device=dev).repeat_interleave(co)
        return self._n_cache[key]

    def _update_running(self, tape: dict, momentum: float = 0.1) -> None:
        """BatchNorm1d's buffer update of every back-end norm from the step's statistics (the conv bias belongs to the mean, the variance is
        the unbiased one), then the folded eval coefficients are marked stale: the next eval forward folds them again, a training step does not.
        (The buffers are views of the store's one flat vector; nothing else shadows them.)"""
        st: _ParamStore = tape["st"]
        for rec in tape["rec"].values():
            D = rec["D"]
            co = D["co"]
            for j, (bn, bias) in enumerate(zip(D["norms"], D["biases"])):
                mean, var = rec["mean"][j * co: (j + 1) * co], rec["var_u"][j * co: (j + 1) * co]
                if bias is not None:
                    mean = mean + st.p32(bias)
                st.buffers[f"{bn}.running_mean"].mul_(1.0 - momentum).add_(mean, alpha=momentum)
                st.buffers[f"{bn}.running_var"].mul_(1.0 - momentum).add_(var, alpha=momentum)
                st.buffers[f"{bn}.num_batches_tracked"].add_(1)
        if self._prep is not None:
            self._prep["folded"] = False

    def validation_step(self, batch: dict, idx: int = 0) -> dict:
        return {f"val/{k}": v for k, v in self(**batch).items()}

    def test_step(self, batch: dict, idx: int = 0) -> dict:
        return {f"test/{k}": v for k, v in self(**batch).items()}


# ----------------------------------------------------------------------------------------------------
# The two stage sets.  Everything that depends on the BatchNorm statistics mode lives here, behind one signature per function: a stage
# forward, a stage backward short of its data gradient, norm5's coefficients and norm5's data gradient.  D is a stage's static description
# (DCTCNLightningModule._stage); with `rec` (tape["rec"]; None without a tape) a stage leaves its record under rec[key], which its backward
# is handed again and whose hmax the data and weight gradients take.  A set holds the model and the store, never the tape.
# ----------------------------------------------------------------------------------------------------
def _gated(D: dict, gates):
    return D["branches"] if gates is None else [dict(br, gate=gates[j]) for j, br in enumerate(D["branches"])]


class _RunningStats:
    """BatchNorm on the running statistics (features / predict / forward, loss_and_backend_grads): folded with the conv bias into the
    convolution's epilogue; no dropout.  Without a tape nothing is kept (no accumulator buffer is allocated)."""
    folds = True          # reads _prepare's folded scale / shift

    def __init__(self, model: DCTCNLightningModule, st: _ParamStore):
        self.m, self.st = model, st

    def stage(self, rec: Optional[dict], key, D: dict, x, out, *, B: int, T: int, gates=None, res=None, res_act: int = ops.ACT_NONE) -> None:
        """ops.tconv_fwd; with a tape the same kernel's saving instantiation, the fp32 accumulators kept in the record."""
        acc = None
        if rec is not None:
            acc = torch.empty((x.shape[0], len(D["ks"]) * D["co"]), dtype=torch.float32, device=x.device)
            rec[key] = dict(acc=acc, hmax=None)          # (None: svsr_tconv_dgrad / svsr_tconv_wgrad, not their _ext entries)
        ops.tconv_fwd(x, B=B, T=T, n_in=D["n_in"], d=D["d"], branches=_gated(D, gates), co=D["co"], act=D["act"], out=out, res=res, res_act=res_act,
                      acc=acc)

    def stage_bwd(self, rec: dict, D: dict, dy, x, accumulate: bool, *, B: int, T: int, gates=None, res=None, res_act: int = ops.ACT_NONE):
        """The epilogue backward over all branches, then per branch j (channels [j * co, (j + 1) * co)) the BatchNorm / bias gradients and
        the weight gradient over the stage's input rows x.  -> (dacc, dres, sums)"""
        m, st, co = self.m, self.st, D["co"]
        dacc, dres, sums = ops.tconv_epi_bwd(dy, rec["acc"], D["scale"], D["shift"], rows=B * T, C=len(D["ks"]) * co, act=D["act"], slope=D["slope"],
                                             res=res, res_act=res_act)
        for j, k in enumerate(D["ks"]):
            m._bn_grads(st, accumulate, sums, D["norms"][j], D["biases"][j], j * co, (j + 1) * co)
            gw, add = m._grad_of(st, D["weights"][j], accumulate)
            ops.tconv_wgrad(x, dacc[:, j * co: (j + 1) * co], gw, B=B, T=T, n_in=D["n_in"], co=co, k=k, d=D["d"],
                            gate=None if gates is None else gates[j], add=add, hmax=rec["hmax"])
        return dacc, dres, sums

    def norm5(self, rec: Optional[dict], stack, B: int, T: int):
        return self.m._prep["norm5"]

    def norm5_bwd(self, r, dh, dpooled, stack, mask, accumulate: bool, *, B: int, T: int):
        dS = torch.empty_like(stack)
        _, sums = ops.tcn_norm_pool_bwd(dh, dpooled, stack, self.m._prep["norm5"][0], mask, B=B, T=T, C=self.m.dims["out_size"], out=dS)
        self.m._bn_grads(self.st, accumulate, sums, f"{TCN}.norm5", None)
        return dS


class _BatchStats:
    """The reference's training arithmetic (loss_and_backend_grads(train_stats=True)): batch-statistic BatchNorm1d over every position the
    full-padding convolution produces, dropout0 / dropout1 when train carries a seed.  A tape is always kept; a record holds what the
    backward and the running-statistic update read."""
    folds = False

    def __init__(self, model: DCTCNLightningModule, st: _ParamStore, train: dict):
        self.m, self.st, self.train = model, st, train
        self.sites = dropout.dctcn_sites(model.config)

    def stage(self, rec: dict, key, D: dict, x, out, *, B: int, T: int, gates=None, res=None, res_act: int = ops.ACT_NONE) -> None:
        """Convolution at every position BatchNorm1d sees (the chomped ones included) -> column statistics -> scale / shift -> the epilogue
        over the T kept rows."""
        st, co, train, drop = self.st, D["co"], self.train, None
        if D["drop_site"] is not None and train["seed"] is not None and train["p"] > 0.0:
            drop = (dropout.site_key(train["seed"], self.sites[D["drop_site"]]), train["p"])
        acc, hmax, hs = ops.tconv_fwd_ext(x, B=B, T=T, n_in=D["n_in"], d=D["d"], branches=_gated(D, gates), co=co)
        stats = ops.tcn_colstats(acc, B=B, T=T, co=co, hmax=hmax, hs=hs)
        n = self.m._counts(B, T, tuple(hs), co, x.device)
        weight = torch.cat([st.p32(f"{bn}.weight") for bn in D["norms"]])
        bias = torch.cat([st.p32(f"{bn}.bias") for bn in D["norms"]])
        scale, shift, mean, invstd, var_u = ops.bn_batch_affine(stats, n, weight, bias)
        ops.tconv_apply(acc, scale, shift, B=B, T=T, co=co, hmax=hmax, hs=hs, act=D["act"], out=out[:, D["out_off"]:], slope=D["slope"], res=res,
                        res_act=res_act, drop=drop)
        rec[key] = dict(D=D, acc=acc, hmax=hmax, hs=hs, scale=scale, shift=shift, mean=mean, invstd=invstd, n=n, var_u=var_u, drop=drop)

    def stage_bwd(self, rec: dict, D: dict, dy, x, accumulate: bool, *, B: int, T: int, gates=None, res=None, res_act: int = ops.ACT_NONE):
        """Pass 1 (sums, dres), the O(C) chain rule, pass 2 (the gradient of every extended accumulator), then per branch the BatchNorm
        gradients, the conv bias's exact zeros and the weight gradient over the extended rows.
        -> (dacc bf16 [B * (T + 2 hmax), C], dres, sums)"""
        m, st, co = self.m, self.st, D["co"]
        geo = dict(B=B, T=T, co=co, hmax=rec["hmax"], hs=rec["hs"], act=D["act"], slope=D["slope"], res=res, res_act=res_act, drop=rec["drop"])
        dres, sums = ops.tconv_epi_bwd_bs(dy, rec["acc"], rec["scale"], rec["shift"], **geo)
        dw, db, ca, cb = ops.bn_batch_param_grads(sums[0], sums[1], rec["mean"], rec["invstd"], rec["n"])
        dacc = ops.tconv_bn_bwd(dy, rec["acc"], rec["scale"], rec["shift"], rec["mean"], rec["invstd"], ca, cb, **geo)
        for j, k in enumerate(D["ks"]):
            bn, bias = D["norms"][j], D["biases"][j]
            m._put(*m._grad_of(st, f"{bn}.weight", accumulate), dw[j * co: (j + 1) * co])
            m._put(*m._grad_of(st, f"{bn}.bias", accumulate), db[j * co: (j + 1) * co])
            if bias is not None:          # cancels under batch statistics: exact zeros (an accumulated .grad is left as it is)
                gb, add = m._grad_of(st, bias, accumulate)
                if not add:
                    gb.zero_()
            gw, add = m._grad_of(st, D["weights"][j], accumulate)
            ops.tconv_wgrad(x, dacc[:, j * co: (j + 1) * co], gw, B=B, T=T, n_in=D["n_in"], co=co, k=k, d=D["d"],
                            gate=None if gates is None else gates[j], add=add, hmax=rec["hmax"])
        return dacc, dres, sums

    def norm5(self, rec: dict, stack, B: int, T: int):
        """norm5 on batch statistics over the B * T rows of the bf16 stack -> (scale, shift) for svsr_tcn_norm_pool_fwd."""
        C, bn = self.m.dims["out_size"], f"{TCN}.norm5"
        stats = ops.tcn_colstats(stack, B=B, T=T, co=C)
        n = self.m._counts(B, T, (0,), C, stack.device)
        scale, shift, mean, invstd, var_u = ops.bn_batch_affine(stats, n, self.st.p32(f"{bn}.weight"), self.st.p32(f"{bn}.bias"))
        rec["norm5"] = dict(D=dict(norms=[bn], biases=[None], co=C), scale=scale, mean=mean, invstd=invstd, n=n, var_u=var_u)
        return scale, shift

    def norm5_bwd(self, r: dict, dh, dpooled, stack, mask, accumulate: bool, *, B: int, T: int):
        """The sums first, then the data gradient with the statistics' chain rule (one rounding)."""
        m, st, C = self.m, self.st, self.m.dims["out_size"]
        dS = torch.empty_like(stack)
        _, sums = ops.tcn_norm_pool_bwd(dh, dpooled, stack, r["scale"], mask, B=B, T=T, C=C, out=dS)
        dw, db, ca, cb = ops.bn_batch_param_grads(sums[0], sums[1], r["mean"], r["invstd"], r["n"])
        m._put(*m._grad_of(st, f"{TCN}.norm5.weight", accumulate), dw)
        m._put(*m._grad_of(st, f"{TCN}.norm5.bias", accumulate), db)
        ops.tcn_norm_pool_bwd_bs(dh, dpooled, stack, r["scale"], r["mean"], r["invstd"], ca, cb, mask, B=B, T=T, C=C, out=dS)
        return dS
