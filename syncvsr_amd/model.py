"""Drop-in module for the reference's ``TransformerLightningModule`` (LRW/video/src/lightning.py:36-223), HIP-native.

Same constructor (``Model(config)``), same ``forward(videos, audio_tokens, labels, word_mask) -> dict`` with the five
scalar keys, same ``forward_videos`` / ``training_step`` / ``configure_optimizers`` helpers and the same state-dict key
names (``stem3d.0.weight`` … ``encoder.encoder.layer.N.attention.self.query.weight`` … ``audio_projection.weight``).
Everything between the inputs and the two losses runs in libsyncvsr_hip.so; this file is orchestration only:
it owns the parameters (one flat fp32 buffer + flat fp32 gradient buffer + bf16 shadows for the MFMA kernels),
records the forward "tape" and replays it backwards by hand — a single autograd node stands for the whole model,
so ``loss_total.backward()`` works as in the reference loops while no per-op autograd graph is built.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Any, Optional

import torch
import torch.nn as nn

from . import ops
from .config import Config, audio_codec_dims
from .init import buffer_specs, hidden_dim, init_state_dict, pad64, param_specs, phys_shape, resnet_block_specs, xt_dims

BF16 = torch.bfloat16


class _SideStream:
    """Weight-gradient launches go to a second HIP stream: they only feed the flat gradient buffer, so they can fill the
    tails of the data-gradient / BatchNorm kernels of the main stream (every kernel here ends with a partially filled
    last round of workgroups).  Tensors handed to the side stream are kept alive until join()."""

    def __init__(self) -> None:
        self.stream: Optional[torch.cuda.Stream] = None
        self.keep: list = []
        self._issuing = False
        self.enabled = False     # set by engine.TrainStep
        # linear-layer weight gradients: neutral for the LRW encoder, a gain for the LRS linears (engine.TrainStep turns it on there)
        self.enabled_small = False

    def run(self, fn, *keep, small: bool = False, behind_main: bool = True) -> None:
        """Issues fn on the side stream, behind what the main stream has issued so far: one cross-stream wait per call (an event record
        + wait: host time in eager mode; handing several functions over at once measured slower).  The tensors fn reads must not be
        written in place before join().  fn's launches go to the side stream through ops.STREAM_OVERRIDE, which is much cheaper on the
        host than entering a torch.cuda.stream() context per launch, but its allocations still come from the main stream's pool: no
        tensor allocated inside fn may be freed before join() (keep it in `keep`, the tape or a result box).  behind_main=False: no
        cross-stream wait — fn reads only what earlier launches of the side stream itself wrote."""
        if not (self.enabled or (small and self.enabled_small)):
            fn()
            return
        self.keep.extend(keep)
        if self._issuing:        # called from inside a function that is being issued on the side stream: issue it there, now, in order
            fn()
            return
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        if behind_main:
            ops.stream_wait(self.stream, torch.cuda.current_stream())
        ops.STREAM_OVERRIDE = self.stream.cuda_stream
        self._issuing = True
        try:
            fn()
        finally:
            self._issuing = False
            ops.STREAM_OVERRIDE = None

    def join(self) -> None:
        if self.stream is not None and (self.enabled or self.enabled_small):
            ops.stream_wait(torch.cuda.current_stream(), self.stream)
        self.keep.clear()


class _Holder(nn.Module):
    """Name-space node: exists only so parameters get the reference's state-dict keys."""


def _attach(root: nn.Module, name: str, tensor: torch.Tensor, is_param: bool) -> None:
    parts = name.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Holder())
        mod = mod._modules[p]
    if is_param:
        mod.register_parameter(parts[-1], nn.Parameter(tensor))
    else:
        mod.register_buffer(parts[-1], tensor)


def _get(root: nn.Module, name: str) -> torch.Tensor:
    obj: Any = root
    for p in name.split("."):
        obj = obj._modules[p] if p in getattr(obj, "_modules", {}) else getattr(obj, p)
    return obj


def _require_device(t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        raise RuntimeError("syncvsr_amd runs on an MI355X HIP device only; there is no CPU fallback (use oracle/ for checking)")


class _NoAutogradCtx:
    """The `ctx` of an autograd Function whose forward / backward a train_step_direct calls by hand."""

    def mark_non_differentiable(self, *a):
        pass


class _StoreModule(nn.Module):
    """What the model modules share: parameters and buffers attached under the reference's state-dict names and kept in one flat
    _ParamStore, the side stream, the device seed word of the counter-based dropout, the device scalars that seed the hand-written backward
    and its "do not zero" switch.  A model calls _attach_state() from its __init__ and supplies `_fwd_rank(name)` and
    `_transposed_entries(offsets)` (see _ParamStore), `_loss_weights()` if it trains, and `grad_store_spans` if its backward has
    store-mode writers.  This class registers no module, parameter or buffer of its own."""

    layer_drop_p = 0.0          # plain defaults of what engine.TrainStep reads from every model
    emb_drop_p = 0.0
    length_norm = False

    def _attach_state(self, specs, bspecs, sd: dict, dropout_seed: int = 0) -> None:
        self._specs, self._bspecs = specs, bspecs
        for name, shape, kind in specs:
            t = sd[name]
            if kind == "conv" and len(shape) == 4:
                t = t.contiguous(memory_format=torch.channels_last)      # physical [Co][kh][kw][Ci]
            _attach(self, name, t, True)
        for name, shape, kind in bspecs:
            _attach(self, name, sd[name], False)
        self._store: Optional[_ParamStore] = None
        self._side = _SideStream()  # second stream for the weight-gradient launches (._side.enabled = False serialises)
        self.grad_ready_hook = None  # called as hook(lo, hi) when flat gradient range [lo, hi) is final (DDP buckets)
        # Dropout masks are counter based (csrc/common.h): element i of site s is kept iff hash(seed, s, i) >= p * 2^32; the seed is a
        # device word advanced once per training forward.
        self.dropout_seed = int(dropout_seed)
        self._drop_word: Optional[torch.Tensor] = None
        self._keep_grads = False    # accumulate_into_grads
        self._loss_scale = 1.0      # set_loss_scale
        # state of one hand-written backward pass (_begin_backward drops what an aborted pass left in the first four)
        self._wg_group: Optional[list] = None   # linear weight gradients awaiting one grouped launch: a backward sets [], _lin_wgrad appends, _flush_lin_wgrads issues
        self._deferred: list = []               # postponed parameter-gradient reductions: ops.add_ln_bwd / bias_act_bwd append (_defer_list), _flush_deferred issues
        self._w3_pending: Optional[dict] = None # the trunk's last halo weight gradient, still slabs: _conv_wgrad hands it to the next halo launch, _flush_w3_chain ends the chain
        self._ready_held: list = []             # gradient-ready notifications (offsets) waiting for the launch that carries _w3_pending: _ready appends, _release_ready issues
        self._early_sumsq = None                # engine.TrainStep: its optimiser state when no collective follows the backward; read by _frontend_backward
        self._metrics_on_side = False           # train_step_direct sets it around its forward; read by _LrwFunction.forward
        self._g_consts: Optional[tuple] = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.mark_params_dirty())
        # (PRE hook: the copies of load_state_dict into the flat buffer must not race with an AdamW range still running on the side stream)
        self.register_load_state_dict_pre_hook(lambda module, *a, **k: module._side.join())

    def store(self) -> "_ParamStore":
        dev = _get(self, self._specs[0][0]).device
        if self._store is None or self._store.device != dev or not self._store.owns(self):
            self._store = _ParamStore(self, dev)
        return self._store

    def mark_params_dirty(self) -> None:
        """Call after changing parameters outside engine.TrainStep (load_state_dict does it): the bf16 shadows are re-cast."""
        if self._store is not None:
            self._store.shadow_fresh = False

    def state_dict(self, *args, **kwargs):
        self._side.join()             # (a TrainStep may have left the tail of its optimiser step on the side stream)
        return super().state_dict(*args, **kwargs)

    def configure_optimizers(self):
        """LRW/video/src/lightning.py:216-223, LRS/video/lightning.py:89-96 — the two parameter groups (decay on ndim >= 2); the fused HIP
        optimiser lives in engine.TrainStep."""
        do_decay = [p for p in self.parameters() if p.requires_grad and p.ndim >= 2]
        no_decay = [p for p in self.parameters() if p.requires_grad and p.ndim < 2]
        return [{"params": do_decay}, {"params": no_decay, "weight_decay": 0.0}]

    takes_vq_waveforms = False          # the word-level models set it: their `audios` slot takes waveforms once a VqWav2VecCodec is attached

    def attach_audio_codec(self, codec, sample_in_training: bool = True):
        """Registers the frozen audio tokeniser of this model's codec — audio_codec.Wav2Vec2Codec for `wav2vec2`, audio_codec.VqWav2VecCodec
        for `vq` — as `self.wav2vec`, the reference's attribute: state_dict() gains its `wav2vec.*` buffers.  With the wav2vec2 codec the
        word-level model then has forward_audios (its forward / training_step still take pre-computed tokens); the sentence-level model's
        forward / prepare_batch / train_step_direct take float waveforms [B, 1, L] or [B, L] in the `audios` slot — 8000 zeros are appended
        to every row and the tokens are computed inside the step.  In training mode the tokens are argmax(logits + Gumbel noise) (the
        reference's frozen quantiser runs its gumbel_softmax branch under Lightning's model.train()), keyed by the dropout seed word;
        sample_in_training=False keeps the eval-mode argmax.  With the vq codec (deterministic: nothing is drawn) the word-level models take
        float waveforms in the `audios` slot wherever the reference calls forward_audios; they are tokenised first and cropped to T * A
        frames (_tokenize_waveforms).  The codec holds buffers only: it stays out of parameters(), the parameter store, the optimiser,
        clipping and the gradient / BatchNorm-statistics collectives."""
        from .audio_codec import VqWav2VecCodec, Wav2Vec2Codec

        if not isinstance(codec, (Wav2Vec2Codec, VqWav2VecCodec)):
            raise TypeError("attach_audio_codec takes a syncvsr_amd.audio_codec.Wav2Vec2Codec or VqWav2VecCodec")
        if isinstance(codec, Wav2Vec2Codec) and self.codec != "wav2vec2":
            raise ValueError(f"this model was built for the {self.codec!r} codec (model.wav2vec.path of the word-level config, args.codec of the "
                             f"sentence-level one): the wav2vec2 tokeniser gives 640-way tokens, A = 2")
        if isinstance(codec, VqWav2VecCodec) and not self.takes_vq_waveforms:
            raise ValueError("the sentence-level model tokenises waveforms with the wav2vec2 codec only; pass pre-computed vq tokens")
        if isinstance(codec, VqWav2VecCodec) and self.codec != "vq":
            raise ValueError(f"this model was built for the {self.codec!r} codec (model.wav2vec.path of the word-level config, args.codec of the "
                             f"sentence-level one): the vq-wav2vec tokeniser gives 320-way tokens, A = 4")
        codec.to(_get(self, self._specs[0][0]).device)
        self.wav2vec = codec
        if isinstance(codec, VqWav2VecCodec) and getattr(self, "cutmix", None) is not None:
            self.cutmix.set_codec(codec)        # lightning.py:85-88: CutMix(num_labels, wav2vec=self.wav2vec)
        self.codec_sample_in_training = bool(sample_in_training)
        return self

    def _tokenize_waveforms(self, audios: torch.Tensor, frames: int) -> torch.Tensor:
        """Float waveforms [B, L] / [B, 1, L] in the `audios` slot of a model with the vq tokeniser attached -> its tokens of the first
        `frames` audio frames, int64 [B, frames, 2] (lightning.py:121-131, then the crop [:, :T*A] of forward).  Anything else — tokens, or
        float audio without that codec — is returned as it came and meets the checks it always met."""
        codec = self._modules.get("wav2vec")
        if codec is None or self.codec != "vq" or not torch.is_tensor(audios) or not audios.is_floating_point():
            return audios
        return codec(audios, keep=int(frames))

    def _codec_samples(self) -> bool:
        """The tokeniser of this training step draws Gumbel noise (and so needs the seed word to advance every step)."""
        return False

    def check_targets(self) -> None:
        """Raises if a batch prepared since the last check held a target the device kernels had to replace (models with such targets)."""

    # -- dropout seed word ---------------------------------------------------------------------------
    def _seed_word(self, dev: torch.device) -> torch.Tensor:
        if self._drop_word is None or self._drop_word.device != dev:
            self._drop_word = torch.tensor([self.dropout_seed], dtype=torch.int32, device=dev)
        return self._drop_word

    def _advance_dropout(self, dev: torch.device) -> None:
        ops.word_add(self._seed_word(dev), 1)     # a device op (a library launch): graph / step-list replays keep drawing fresh masks

    def reseed_dropout(self, seed: int) -> None:
        self.dropout_seed = int(seed)
        if self._drop_word is not None:          # in place: a captured graph / recorded step list holds this word's address
            self._drop_word.fill_(self.dropout_seed)
        if hasattr(self, "_layer_rng"):          # the layer-drop draws follow the seed too (per-rank / per-run reseeding)
            self._layer_rng.seed(self.dropout_seed)

    def rng_state(self) -> dict:
        """Everything random about the next training forward, for bit-exact resume: the dropout seed word (the device counter the
        masks are hashed from) and the python generator behind layer_dropout.  engine.TrainStep.state_dict stores it."""
        word = self.dropout_seed if self._drop_word is None else int(self._drop_word.item())
        out = {"dropout_word": word}
        if hasattr(self, "_layer_rng"):
            out["layer_rng"] = self._layer_rng.getstate()
        return out

    def load_rng_state(self, state: dict) -> None:
        self.dropout_seed = int(state["dropout_word"])
        if self._drop_word is not None:
            self._drop_word.fill_(self.dropout_seed)
        if "layer_rng" in state and hasattr(self, "_layer_rng"):
            self._layer_rng.setstate(state["layer_rng"])

    # -- seeds of the hand-written backward ----------------------------------------------------------
    def _loss_weights(self) -> tuple[float, ...]:
        """d (total loss) / d (each loss the model's autograd node returns), in the node's output order."""
        raise NotImplementedError(f"{type(self).__name__} has no training step")

    def direct_constants(self, dev) -> None:
        """The loss weights as device scalars (made once per device, outside any recorded region), times the loss scale of set_loss_scale()."""
        if self._g_consts is None or self._g_consts[0].device != dev:
            self._g_consts = tuple(torch.full((), w, dtype=torch.float32, device=dev) for w in self._loss_weights())
            if self._loss_scale != 1.0:
                self.set_loss_scale(self._loss_scale)

    def set_loss_scale(self, scale: float = 1.0) -> None:
        """Gradient accumulation (engine.TrainStep(accumulate=N) drives this with 1 / N): the seeds of the hand-written backward become
        d (scale * total loss) / d (each loss) — what `(loss * scale).backward()` hands the backward, in fp32: fp32(scale) * fp32(weight).
        The device scalars are written IN PLACE and outside any recorded region: a recorded step list reads them by address, so the scale
        needs no re-recording.  The losses a step returns stay unscaled."""
        self._loss_scale = float(scale)
        if self._g_consts is not None:
            one = torch.tensor(self._loss_scale, dtype=torch.float32)
            for g, w in zip(self._g_consts, self._loss_weights()):
                g.copy_(one * torch.tensor(w, dtype=torch.float32))

    def loss_seeds(self, dev) -> tuple:
        """One seed per loss of _loss_weights(): the device scalars train_step_direct hands its backward."""
        self.direct_constants(dev)
        return self._g_consts

    def accumulate_into_grads(self, on: bool = True) -> None:
        """The "do not zero" switch of the backward.  Off (the default): every backward() zeroes the flat gradient buffer (the storage behind
        every p.grad) before it writes, so `loss.backward(); optimizer.step()` needs no zero_grad().  On: the following backward() calls ADD
        into the buffer.  Hand-rolled accumulation over N micro-batches with a foreign optimiser:

            model.accumulate_into_grads(False); (model(*b0)["loss_total"] / N).backward()      # zeroes, then writes
            model.accumulate_into_grads(True)
            for b in rest: (model(*b)["loss_total"] / N).backward()                             # adds
            optimizer.step(); model.accumulate_into_grads(False)

        (optimizer.zero_grad() only drops the p.grad views; the buffer is zeroed by the first backward.)  engine.TrainStep sets this
        per micro-step and leaves it off."""
        self._keep_grads = bool(on)

    def grad_store_spans(self, offsets: dict, phys: dict) -> list:
        """[lo, hi) element ranges of the flat gradient buffer whose first writer in a backward pass is a store-mode weight-gradient launch
        (ops.GradCoverage).  None declared: engine.TrainStep keeps the whole-buffer zero-fill."""
        return []

    def _drop_backward_state(self) -> None:
        """What a hand-written backward that aborted on a host exception left collected or postponed (linear weight gradients awaiting their
        grouped launch, deferred reductions, the trunk's pending halo slabs, held-back notifications) is dropped, not issued: its closures
        hold that pass's tensors and would add into this pass's gradients.  _begin_backward calls it; so does every backward that does not
        go through _begin_backward (dctcn.DCTCNLightningModule.loss_and_grads)."""
        self._wg_group = None
        self._deferred.clear()
        self._w3_pending = None
        self._ready_held.clear()


def _begin_backward(model: _StoreModule, st: "_ParamStore", dev: torch.device, *grads) -> tuple:
    """The first lines of a hand-written backward: the zero-fill (unless accumulate_into_grads), the p.grad views, and the incoming
    gradients as contiguous fp32 scalars (None: zero).  What a backward that aborted on a host exception left collected or postponed is
    dropped, not issued: its closures hold that pass's tensors and would add into this pass's gradients."""
    model._drop_backward_state()
    if not model._keep_grads:
        st.zero_grad()
    st.rebind_grads()
    return tuple((g if g is not None else torch.zeros((), device=dev)).float().contiguous() for g in grads)


class TransformerLightningModule(_StoreModule):
    """HIP-native twin of the reference LightningModule (word-level LRW model with the SyncVSR audio head)."""

    def __init__(self, config: Config, seed: Optional[int] = None):
        super().__init__()
        if not isinstance(config, Config):
            config = Config(config)
        self.config = config
        bert = config.model.bert
        self.encoder_type = str(bert.type)
        if self.encoder_type not in ("huggingface", "x-transformers"):
            raise NotImplementedError(f"model.bert.type {bert.type!r}: the reference knows `huggingface` and `x-transformers` (lightning.py:90-105)")
        self.use_wb = bool(config.data.use_word_boundary)
        if self.use_wb and self.encoder_type == "huggingface":
            raise NotImplementedError(
                "use_word_boundary needs a 513-wide encoder, which the reference's huggingface branch cannot build either "
                "(BertConfig.hidden_size stays 512, lightning.py:92,145); use `type: x-transformers` as the shipped yaml does")
        self.is_train = False
        self.word_labels = int(bert.num_labels)
        self.lambda_audio = float(config.optim.lambda_audio)
        # audio head as one contraction with the cross-entropy in its epilogue (csrc/audio_head.hip) whenever the shape is taken; keep_audio_logits
        # additionally materialises logits_audio in `_last` (one extra projection launch, for inspection and the parity tests)
        self.fused_audio_head = True
        self.keep_audio_logits = False
        self.label_smoothing = float(config.train.label_smoothing)
        self.codec, self.audio_alignment, self.vq_groups, self.audio_vocab_size = audio_codec_dims(config.model.wav2vec.path)
        self.dim = hidden_dim(config)
        self.dim_p = pad64(self.dim)            # row pitch of the encoder's activations (pad columns are zero)
        seed = 0 if seed is None else int(seed)
        from .dropout import lrw_sites, lrw_xt_sites

        self.emb_drop_p = float(bert.get("emb_dropout", 0.0))          # read directly by the module (lightning.py:45)
        if self.encoder_type == "huggingface":
            self.heads = int(bert.num_attention_heads)
            self.layers = int(bert.num_hidden_layers)
            self.inter = int(bert.intermediate_size)
            self.ln_eps = float(bert.get("layer_norm_eps", 1e-12))
            # missing keys take BertConfig(**config.model.bert)'s defaults, 0.1 each (lightning.py:92)
            self.drop_p = float(bert.get("hidden_dropout_prob", 0.1))
            self.attn_drop_p = float(bert.get("attention_probs_dropout_prob", 0.1))
            self._sites = lrw_sites(self.layers)
            if self.dim % 512 or self.dim // self.heads != 64:
                raise NotImplementedError("encoder width must be a multiple of 512 with 64-wide heads")
        else:
            # x_transformers.Encoder(dim, depth, heads, attn_dropout, layer_dropout, ff_dropout, use_rmsnorm, ff_glu, rotary_pos_emb)
            # (lightning.py:95-105).  The shipped combination (RMSNorm + GEGLU + rotary) is the one built here.
            if not (bool(bert.get("use_rmsnorm", False)) and bool(bert.get("ff_glu", False)) and bool(bert.get("rotary_pos_emb", False))):
                raise NotImplementedError("the x-transformers encoder is implemented for use_rmsnorm = ff_glu = rotary_pos_emb = true "
                                          "(the shipped yamls, bert-12l-512d_LRW_96_bf16_rrc_*.yaml:27-29)")
            _, self.attn_inner, self.inter, self.layers = xt_dims(config)
            self.heads = int(bert.heads)
            self.inter_p, self.glu_p = pad64(self.inter), pad64(2 * self.inter)
            self.drop_p = float(bert.get("ff_dropout", 0.0))            # FeedForward's dropout, after the gate
            self.attn_drop_p = float(bert.get("attn_dropout", 0.0))
            self.layer_drop_p = float(bert.get("layer_dropout", 0.0))
            self.final_norm = bool(bert.get("final_norm", False))
            self.rotate_value = bool(bert.get("rotate_value", True))   # x-transformers 1.x rotates q, k AND v
            self.rms_eps = 1e-8
            self._sites = lrw_xt_sites(self.layers)
            import random

            self._layer_rng = random.Random(seed)
            self.layer_skip_override: Optional[set[int]] = None     # tests: the set of `encoder.layers.{n}` indices to skip
            self._rot_tab: dict[tuple[int, str], torch.Tensor] = {}

        self._attach_state(param_specs(config), buffer_specs(config), init_state_dict(config, seed=seed), dropout_seed=seed)
        self._phys = {n: phys_shape(config, n, shp) for n, shp, _ in self._specs}
        from .augment import CutMix

        self.cutmix = CutMix(self.word_labels).eval()          # lightning.py:85-88 (attach_audio_codec hands it the vq tokeniser)
        self.stem_name, self.trunk_name = "stem3d", "resnet"
        self.stem_act, self.trunk_act = ops.ACT_GELU, ops.ACT_RELU          # lightning.py:52, timm BasicBlock

    # ------------------------------------------------------------------------------------------------
    # reference-compatible helpers
    # ------------------------------------------------------------------------------------------------
    takes_vq_waveforms = True

    def training_step(self, batch, idx: int = 0) -> torch.Tensor:
        """lightning.py:194-202: (CutMix) -> forward -> loss_total."""
        self.is_train = True
        if self.config.train.use_cutmix:
            batch = self.cutmix(*batch)
        return self(*batch)["loss_total"]

    def validation_step(self, batch, idx: int = 0) -> dict:
        """lightning.py:204-208: forward in evaluation mode (float waveforms are tokenised by the attached vq codec) -> the `val/` metrics."""
        self.is_train = False
        return {f"val/{k}": v for k, v in self(*batch).items()}

    def test_step(self, batch, idx: int = 0) -> dict:
        """lightning.py:210-214."""
        self.is_train = False
        return {f"test/{k}": v for k, v in self(*batch).items()}

    def forward_audios(self, audios: torch.Tensor) -> torch.Tensor:
        """lightning.py:121-131: float waveforms [B, L] (or [B, 1, L]) -> int64 tokens [B, F, 2] (no padding appended).  wav2vec2 codec: in
        training mode (with sample_in_training) the tokens are argmax(logits + Gumbel noise) keyed by the current dropout seed word; the vq
        codec is deterministic."""
        codec = self._modules.get("wav2vec")
        if codec is None:
            kind = "VqWav2VecCodec" if self.codec == "vq" else "Wav2Vec2Codec"
            raise ValueError(f"forward_audios needs the {self.codec} tokeniser: call attach_audio_codec({kind}...) first")
        if audios.device.type != "cuda":
            raise RuntimeError("audio waveforms must be on the MI355X device: the tokeniser has no CPU path")
        if self.codec == "vq":
            return codec(audios)
        seed = self._seed_word(audios.device) if self.training and self.codec_sample_in_training else None
        return codec(audios, sample=seed is not None, seed_word=seed)

    def _d(self, site: str, kind: str = "hidden"):
        """(seed word, site id, p) for ops.*(drop=...) or None when dropout is off (eval mode / p = 0)."""
        p = {"hidden": self.drop_p, "attn": self.attn_drop_p, "emb": self.emb_drop_p}[kind]
        if not self.training or p <= 0.0:
            return None
        return (self._drop_word, self._sites[site], p)

    @staticmethod
    def _fwd_rank(name: str) -> int:
        if name.startswith("stem3d"):
            return 0
        if name.startswith("resnet"):
            return 1
        if name == "cls_token" or name.startswith("encoder.embeddings"):
            return 2
        if name.startswith(("encoder.encoder", "encoder.layers", "encoder.final_norm")):
            return 3
        return 4

    def _transposed_entries(self, offsets) -> list[tuple[str, int, int, int]]:
        """(key, source offset, out features, in features) — storage sizes — of every linear weight whose data-gradient GEMM runs."""
        out = []
        if self.encoder_type == "x-transformers":
            Dp, E = self.dim_p, self.attn_inner
            for i in range(self.layers):
                a, f = f"encoder.layers.{2 * i}.1", f"encoder.layers.{2 * i + 1}.1.ff"
                q, k, v = (offsets[f"{a}.to_{x}.weight"][0] for x in "qkv")
                assert k == q + E * Dp and v == k + E * Dp, "to_q / to_k / to_v must be adjacent in the flat buffer"
                out.append((f"{a}.qkv", q, 3 * E, Dp))
                out.append((f"{a}.to_out.weight", offsets[f"{a}.to_out.weight"][0], Dp, E))
                out.append((f"{f}.0.proj.weight", offsets[f"{f}.0.proj.weight"][0], self.glu_p, Dp))
                out.append((f"{f}.3.weight", offsets[f"{f}.3.weight"][0], Dp, self.inter_p))
        else:
            D = self.dim
            for i in range(self.layers):
                p = f"encoder.encoder.layer.{i}"
                out.append((f"{p}.qkv", offsets[f"{p}.attention.self.query.weight"][0], 3 * D, D))
                out.append((f"{p}.attention.output.dense.weight", offsets[f"{p}.attention.output.dense.weight"][0], D, D))
                out.append((f"{p}.intermediate.dense.weight", offsets[f"{p}.intermediate.dense.weight"][0], self.inter, D))
                out.append((f"{p}.output.dense.weight", offsets[f"{p}.output.dense.weight"][0], D, self.inter))
                q, k, v = (offsets[f"{p}.attention.self.{x}.weight"][0] for x in ("query", "key", "value"))
                assert k == q + D * D and v == k + D * D, "q/k/v weights must be adjacent in the flat buffer"
                qb, kb, vb = (offsets[f"{p}.attention.self.{x}.bias"][0] for x in ("query", "key", "value"))
                assert kb == qb + D and vb == kb + D
        for n in ("audio_projection.weight", "category_classifier.weight"):
            out.append((n, offsets[n][0], offsets[n][2][0], self.dim_p))
        return out

    # ------------------------------------------------------------------------------------------------
    def forward_videos(self, videos: torch.Tensor) -> torch.Tensor:
        """lightning.py:112-119: [B,1,T,H,W] -> fp32 [B,T,512] (no autograd; use forward() for training)."""
        st = self.store()
        st.refresh_shadows()
        tape: dict[str, Any] = {}
        with torch.no_grad():
            feats = _frontend_forward(self, st, tape, videos.float().contiguous(), self.training)
        return feats.float().view(videos.size(0), -1, 512)

    def forward(self, videos: torch.Tensor, audio_tokens: torch.Tensor, labels: torch.Tensor, word_mask: torch.Tensor) -> dict[str, torch.Tensor]:
        _require_device(videos)
        st = self.store()
        T = videos.size(2)
        A = self.audio_alignment
        audio_tokens = self._tokenize_waveforms(audio_tokens, T * A)
        audio_tokens = audio_tokens[:, : T * A].contiguous()
        if audio_tokens.size(1) != T * A:
            raise ValueError(f"audio_tokens has {audio_tokens.size(1)} steps, need >= {T * A}")
        wm = None
        if self.use_wb:           # lightning.py:145: the word-boundary indicator becomes feature 513 of every frame
            if word_mask.shape != (videos.size(0), T):
                raise ValueError(f"word_mask must be [batch, frames] = {(videos.size(0), T)}, got {tuple(word_mask.shape)}")
            wm = word_mask.to(device=videos.device, dtype=torch.float32).contiguous()
        outs = _LrwFunction.apply(self.cls_token, self, st, videos.float().contiguous(), audio_tokens, labels.contiguous(),
                                   torch.is_grad_enabled(), wm)
        loss_category, loss_audio, acc = outs
        loss_total = loss_category + loss_audio * self.lambda_audio
        return {
            "loss_total": loss_total,
            "loss_category": loss_category,
            "loss_audio": loss_audio,
            "accuracy_top1": acc[0],
            "accuracy_top5": acc[1],
        }


    # ------------------------------------------------------------------------------------------------
    def prepare_batch(self, videos, audio_tokens, labels, word_mask):
        """The input conversions of forward(), done ahead of it: what engine.TrainStep keeps as the static inputs of a recorded step
        (inside the recorded region every one of them must be a no-op, so that no torch kernel is needed at replay)."""
        T = videos.size(2)
        A = self.audio_alignment
        audio_tokens = self._tokenize_waveforms(audio_tokens, T * A)
        if audio_tokens.size(1) < T * A:
            raise ValueError(f"audio_tokens has {audio_tokens.size(1)} steps, need >= {T * A}")
        hard = labels.dtype in (torch.int64, torch.int32)
        wm = word_mask
        if self.use_wb:
            if word_mask.shape != (videos.size(0), T):
                raise ValueError(f"word_mask must be [batch, frames] = {(videos.size(0), T)}, got {tuple(word_mask.shape)}")
            wm = word_mask.to(device=videos.device, dtype=torch.float32).contiguous()
        return (videos.float().contiguous(), audio_tokens[:, : T * A].contiguous(), (labels.long() if hard else labels.float()).contiguous(), wm)

    def _loss_weights(self) -> tuple[float, ...]:
        return (1.0, self.lambda_audio)          # d loss_total / d loss_{category, audio}

    def grad_store_spans(self, offsets: dict, phys: dict) -> list:
        """[lo, hi) element ranges of the flat gradient buffer whose first writer in a backward pass is a weight-gradient launch with a store
        mode (ops.GradCoverage): the trunk's convolutions (ops.conv2d_wgrad) and, with the HF encoder, its dense layers and the two heads
        (ops.linear_wgrad / linear_wgrad_group; query | key | value are ONE launch over their adjacent storage).  Each has exactly one writer
        per backward.  Tensors stored with pads (the launches write the logical corner only; pads must stay zero) are left to the zero-fill, and
        so is everything else: the stem's weight, the embeddings, every 1-D tensor.  The x-transformers encoder declares nothing — layer drop
        leaves whole blocks without a writer — and keeps the whole-buffer fill."""
        if self.encoder_type != "huggingface":
            return []
        names = [(n, 1) for n, s, k in self._specs if k == "conv" and len(s) == 4]
        for i in range(self.layers):
            p = f"encoder.encoder.layer.{i}"
            names += [(f"{p}.attention.self.query.weight", 3), (f"{p}.attention.output.dense.weight", 1), (f"{p}.intermediate.dense.weight", 1),
                      (f"{p}.output.dense.weight", 1)]
        names += [("audio_projection.weight", 1), ("category_classifier.weight", 1)]
        spans = []
        for n, mult in names:
            o, numel, shape = offsets[n]
            if tuple(phys[n]) != tuple(shape):
                continue
            if mult == 3:       # key and value follow query in storage
                kv = [offsets[n.replace("query", w)] for w in ("key", "value")]
                if [e[0] for e in kv] != [o + numel, o + 2 * numel] or any(tuple(phys[n.replace("query", w)]) != tuple(e[2]) for w, e in zip(("key", "value"), kv)):
                    continue
            spans.append((o, o + mult * numel))
        return spans

    def train_step_direct(self, videos, audio_tokens, labels, word_mask) -> dict[str, torch.Tensor]:
        """forward + backward of loss_total WITHOUT autograd: the same tape functions `forward()` + `loss_total.backward()` run,
        called directly, with loss_total and the two loss weights formed on the device.  Inputs as prepare_batch returns them.
        Every device operation in here is a library call, so the whole step can be recorded into a native step list."""
        _require_device(videos)
        st = self.store()
        self.direct_constants(videos.device)
        ctx = _NoAutogradCtx()
        self._metrics_on_side = True          # what only the caller reads (accuracy, loss_total) is computed on the side stream: joined when the backward ends
        try:
            loss_category, loss_audio, acc = _LrwFunction.forward(ctx, self.cls_token, self, st, videos, audio_tokens, labels, True,
                                                                  word_mask if self.use_wb else None)
        finally:
            self._metrics_on_side = False
        if self._side.enabled:
            box: dict = {}
            self._side.run(lambda: box.__setitem__("t", ops.lincomb2(loss_category, loss_audio, self.lambda_audio)), loss_category, loss_audio)
            loss_total = box["t"]
        else:
            loss_total = ops.lincomb2(loss_category, loss_audio, self.lambda_audio)
        _LrwFunction.backward(ctx, *self._g_consts, None)
        return {"loss_total": loss_total, "loss_category": loss_category, "loss_audio": loss_audio, "accuracy_top1": acc[0],
                "accuracy_top5": acc[1]}


Model = TransformerLightningModule


# ----------------------------------------------------------------------------------------------------
# parameter store: flat fp32 master / gradient buffers + bf16 shadows
# ----------------------------------------------------------------------------------------------------
_BnHandle = namedtuple("_BnHandle", "C gamma beta dgamma dbeta coef mean rstd running_mean running_var num_batches_tracked base")


class _ParamStore:
    """Flat fp32 master / gradient buffers + bf16 shadows for one model.  The model supplies `_specs`, `_bspecs`,
    `_fwd_rank(name)` (position of a tensor in the forward pass) and `_transposed_entries(offsets)` (which linear weights
    need a transposed bf16 shadow for their data-gradient GEMM, and which tensors must be adjacent)."""

    def __init__(self, model, device: torch.device):
        self.device = device
        specs = model._specs
        # flat order: [decayed (ndim >= 2)] then [not decayed]; q/k/v of a layer adjacent so one GEMM covers them
        # decayed tensors are laid out in FORWARD order (stem, trunk, embeddings, encoder layers, heads) so the backward
        # pass finalises the buffer from its end towards its start — contiguous all-reduce buckets (engine.DataParallel).
        fwd_rank = model._fwd_rank
        decay = sorted([(n, s) for n, s, k in specs if len(s) >= 2], key=lambda e: fwd_rank(e[0]))   # stable
        nodecay = [(n, s) for n, s, k in specs if len(s) < 2]
        self.offsets: dict[str, tuple[int, int, tuple[int, ...]]] = {}
        self._side = getattr(model, "_side", None)      # a TrainStep may leave the tail of its optimiser step there: whoever reads or rewrites flat / w16 from the main stream joins it first
        self._vc: dict = {}        # cached views of the flat buffers (p32 / g32 / s16 / t16)
        self.grad_clean = False         # engine.TrainStep zero-filled `grad` when its step began: set there, consumed by zero_grad
        self.sumsq_tail_done = False    # the squares behind the stem weight are summed already: set by _frontend_backward, consumed by TrainStep._optimizer
        off = 0
        phys = getattr(model, "_phys", {})
        self.phys: dict[str, tuple[int, ...]] = {n: tuple(phys.get(n, s)) for n, s, _ in specs}
        for n, s in decay + nodecay:
            numel = math.prod(self.phys[n])          # storage size: rows / columns padded to 64 where the model asks for it
            off = (off + 3) // 4 * 4                    # 16-byte alignment of every tensor
            self.offsets[n] = (off, numel, tuple(s))
            off += numel
            if (n, s) == decay[-1]:
                off = (off + 3) // 4 * 4
                self.decay_end = off
        self.numel = (off + 3) // 4 * 4
        # [0, sumsq_head): the stem convolution's weight, the LAST gradient of a backward pass: the global norm's sum of squares over everything
        # behind it can run while that gradient is still being computed (engine.TrainStep._optimizer; 0: the buffer does not start with it)
        first = (decay + nodecay)[0][0]
        self.sumsq_head = self.offsets[first][1] if first == getattr(model, "stem_name", "?") + ".0.weight" and self.offsets[first][1] % 4 == 0 else 0
        # [0, front_end): the visual front-end's weights (forward ranks 0 and 1), what the next forward needs first (engine.TrainStep updates the
        # rest on the side stream beside that forward)
        later = [self.offsets[n][0] for n, s in decay if fwd_rank(n) >= 2]
        self.front_end = min(later) if later else self.decay_end
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.grad = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.w16 = torch.zeros(self.numel, dtype=BF16, device=device)
        self._params: dict[str, nn.Parameter] = {}
        for n, s, kind in specs:
            p = _get(model, n)
            o, numel, shape = self.offsets[n]
            view = self._view(self.flat, n)
            view.copy_(p.data.to(device))
            p.data = view
            p.grad = self._view(self.grad, n)
            self._params[n] = p
        self.buffers = {n: _get(model, n) for n, _, _ in model._bspecs}
        for n, b in self.buffers.items():
            if b.device != device:
                raise RuntimeError("move the module to the GPU before the first forward (model.to('cuda'))")
        # the floating-point buffers (BatchNorm running statistics) are views of ONE flat vector, so data-parallel training can
        # broadcast them from rank 0 in a single collective (DDP's broadcast_buffers, engine.GradReducer)
        fbufs = [(n, b) for n, b in self.buffers.items() if b.is_floating_point()]
        self.bufflat = torch.empty(sum(b.numel() for _, b in fbufs), dtype=torch.float32, device=device)
        o = 0
        for n, b in fbufs:
            view = self.bufflat[o : o + b.numel()].view(b.shape)
            view.copy_(b)
            b.data = view
            o += b.numel()
        # transposed shadows for the data-gradient contractions
        entries = []
        toff = 0
        self.t_offsets: dict[str, tuple[int, tuple[int, int, int]]] = {}

        def add_t(key: str, src_off: int, A: int, T: int, Bd: int):
            nonlocal toff
            Apad = (A + 63) // 64 * 64
            self.t_offsets[key] = (toff, (Bd, T, Apad))
            entries.append((src_off, toff, A, T, Bd, Apad))
            toff += Bd * T * Apad

        for n, s, kind in specs:
            if kind == "conv" and len(s) == 4:
                add_t(n, self.offsets[n][0], s[0], s[2] * s[3], s[1])
        self.n_entries_front = sum(1 for e in entries if e[0] < self.front_end)       # the front-end's entries come first
        assert all(e[0] < self.front_end for e in entries[: self.n_entries_front]) and all(e[0] >= self.front_end for e in entries[self.n_entries_front:])
        for key, src_off, A, Bd in model._transposed_entries(self.offsets):
            add_t(key, src_off, A, 1, Bd)
        self.w16t = torch.zeros(max(toff, 1), dtype=BF16, device=device)
        import numpy as np

        tab = np.zeros(len(entries), dtype=np.dtype([("src", "<i8"), ("dst", "<i8"), ("A", "<i4"), ("T", "<i4"), ("Bd", "<i4"), ("Apad", "<i4")]))
        for i, e in enumerate(entries):
            tab[i] = e
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(device)
        self.n_entries = len(entries)
        # per-BatchNorm workspaces
        self.bn: dict[str, dict[str, torch.Tensor]] = {}
        for n, s, kind in specs:
            if kind == "norm_w" and (n + "").replace(".weight", ".running_mean") in self.buffers:
                C = s[0]
                base = n[: -len(".weight")]
                self.bn[base] = dict(
                    coef=torch.empty(3 * C, dtype=torch.float32, device=device),
                    mean=torch.empty(C, dtype=torch.float32, device=device),
                    rstd=torch.empty(C, dtype=torch.float32, device=device),
                )
        self.shadow_fresh = False     # True only while an optimiser that writes the shadows itself owns the step loop
        self.generation = 0           # counts weight updates (optimiser steps, shadow refreshes): caches derived from the weights key on it

    def owns(self, model) -> bool:
        lo, hi = self.flat.data_ptr(), self.flat.data_ptr() + self.flat.numel() * 4
        anchor = model._specs[0][0]
        blo, bhi = self.bufflat.data_ptr(), self.bufflat.data_ptr() + self.bufflat.numel() * 4
        bufs_ok = all(blo <= b.data_ptr() < bhi for b in self.buffers.values() if b.is_floating_point() and b.numel())
        return bufs_ok and all(lo <= p.data_ptr() < hi for p in self._params.values()) and _get(model, anchor) is self._params[anchor]

    def _view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        o, numel, shape = self.offsets[name]
        seg = flat[o : o + numel]
        if len(shape) == 4:   # conv weights are stored [Co][kh][kw][Ci]; the tensor keeps the logical [Co,Ci,kh,kw] shape
            return seg.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
        ph = self.phys[name]
        if ph != shape:       # padded storage: the tensor is the [:logical] corner of it
            return seg.view(ph)[tuple(slice(0, d) for d in shape)]
        return seg.view(shape)

    # -- accessors used by the engine -------------------------------------------------------------
    # (the views are cached: the flat buffers are never reallocated, and building ~400 tensor views per step was 0.3 ms of host time)
    def p32(self, name: str) -> torch.Tensor:
        v = self._vc.get(("p", name))
        if v is None:
            o, n, _ = self.offsets[name]
            v = self._vc[("p", name)] = self.flat[o : o + n]
        return v

    def g32(self, name: str) -> torch.Tensor:
        v = self._vc.get(("g", name))
        if v is None:
            o, n, _ = self.offsets[name]
            v = self._vc[("g", name)] = self.grad[o : o + n]
        return v

    def s16(self, name: str, numel: Optional[int] = None) -> torch.Tensor:
        v = self._vc.get(("s", name, numel))
        if v is None:
            o, n, _ = self.offsets[name]
            v = self._vc[("s", name, numel)] = self.w16[o : o + (numel or n)]
        return v

    def t16(self, key: str) -> torch.Tensor:
        v = self._vc.get(("t", key))
        if v is None:
            o, (Bd, T, Apad) = self.t_offsets[key]
            v = self._vc[("t", key)] = self.w16t[o : o + Bd * T * Apad].view(Bd, T, Apad)
        return v

    def bnh(self, base: str) -> "_BnHandle":
        """The tensors of the BatchNorm called `base` under one name, the one place where their names are spelled: views of the flat buffers,
        the workspaces of self.bn[base] and the running buffers (built once, like the views above; nothing is allocated)."""
        h = self._vc.get(("bn", base))
        if h is None:
            ws, w, b = self.bn[base], f"{base}.weight", f"{base}.bias"
            h = self._vc[("bn", base)] = _BnHandle(ws["mean"].numel(), self.p32(w), self.p32(b), self.g32(w), self.g32(b), ws["coef"], ws["mean"], ws["rstd"],
                                                   *(self.buffers[f"{base}.{k}"] for k in _BnHandle._fields[-4:-1]), base)
        return h

    def span(self, name: str, numel: Optional[int] = None) -> tuple[int, int]:
        o, n, _ = self.offsets[name]
        return o, o + (numel or n)

    def refresh_shadows(self) -> None:
        if self._side is not None:
            self._side.join()         # the side stream's AdamW range may still be writing flat / w16 (engine.TrainStep._optimizer)
        self.generation += 1
        ops.cast_bf16(self.flat, self.w16)
        ops.transpose_shadows(self.flat, self.w16, self.w16t, self.table, self.n_entries)

    def zero_grad(self) -> None:
        if self.grad_clean:       # engine.TrainStep zeroed the buffer on the side stream when the step began
            self.grad_clean = False
            return
        ops.memset(self.grad, 0)

    def rebind_grads(self) -> None:
        for n, p in self._params.items():
            g = p.grad
            if g is None or g.data_ptr() != self.grad.data_ptr() + self.offsets[n][0] * 4:
                p.grad = self._view(self.grad, n)


# ----------------------------------------------------------------------------------------------------
# forward / backward tape
# ----------------------------------------------------------------------------------------------------
def _bn_stats(bn: _BnHandle, training: bool, count: int, stats) -> None:
    """Fills bn.mean / bn.rstd.  stats: the partial sums (buffer, rows) the producing convolution just wrote on this stream (training mode)."""
    if training:
        ops.bn_finalize(stats, bn.C, count, bn.mean, bn.rstd, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    else:
        ops.bn_eval_prepare(bn.running_mean, bn.running_var, bn.mean, bn.rstd)


def _bn_from_stats(t: dict, g: torch.Tensor, stats) -> torch.Tensor:
    """Second half of the backward of tape entry t's BatchNorm, behind a launch whose epilogue took the first (g, stats)."""
    bn = t["bn"]
    return ops.bn_bwd_from_stats(g, t["c"], bn.mean, bn.rstd, bn.gamma, stats, bn.coef, bn.dgamma, bn.dbeta)


def _conv_stats(st: _ParamStore, tape: dict, x: torch.Tensor, conv: str, bn: str, k: int, stride: int, pad: int, training: bool,
                res: Optional[torch.Tensor] = None, act: int = 0) -> dict:
    """The convolution and its BatchNorm's statistics -> the tape entry; y = None until an apply pass (bn_act_fwd, bn_act_fwd2) fills it."""
    o, n, shape = st.offsets[f"{conv}.weight"]
    w16 = st.w16[o : o + n].view(shape[0], k, k, shape[1])
    c, stats = ops.conv2d_fwd(x, w16, k, stride, pad, want_stats=training)
    h = st.bnh(bn)
    _bn_stats(h, training, c.numel() // c.shape[-1], stats)
    tape[conv] = t = dict(x=x, c=c, y=None, mean=h.mean, rstd=h.rstd, k=k, stride=stride, pad=pad, act=act, bn=h, res=res)
    return t


def _conv_bn(st: _ParamStore, tape: dict, x: torch.Tensor, conv: str, bn: str, k: int, stride: int, pad: int, training: bool,
             res: Optional[torch.Tensor], act: int) -> torch.Tensor:
    t = _conv_stats(st, tape, x, conv, bn, k, stride, pad, training, res, act)
    t["y"] = ops.bn_act_fwd(t["c"], res, t["mean"], t["rstd"], t["bn"].gamma, t["bn"].beta, act)
    return t["y"]


def _trunk_blocks(model):
    """(prefix, inplanes, planes, stride, has_downsample) with the model's own trunk name (`resnet` for LRW,
    `encoder.frontend.trunk` for LRS — same BasicBlock topology, different activation)."""
    for prefix, inp, planes, stride, down in resnet_block_specs():
        yield model.trunk_name + prefix[len("resnet"):], inp, planes, stride, down


def _block_forward(model, st: "_ParamStore", tape: dict, x: torch.Tensor, blk: tuple, training: bool) -> torch.Tensor:
    prefix, inp, planes, stride, down = blk
    act, side = model.trunk_act, model._side
    conv1, conv2, convd = ((f"{prefix}.{c}", f"{prefix}.{b}") for c, b in (("conv1", "bn1"), ("conv2", "bn2"), ("downsample.0", "downsample.1")))
    # The 1x1 branch of a downsample block runs behind conv1 / bn1 on the main stream ("serial"), or
    # "fold"  ReLU trunk in training: its convolution and statistics only — on the side stream beside conv1 / bn1 / conv2 where there is one —
    #         and its BatchNorm is applied inside the block-end pass, after the join, so that its output is never written (the Swish trunk's
    #         backward recomputes its pre-activation from the stored residual input and keeps the other forms)
    # "side"  (round 6) the branch (1x1 convolution, its statistics and apply pass) meets the main branch only at the residual sum: on the
    #         side stream beside conv1 / bn1 (3 blocks x 3 launches off the main chain: -0.035 ms LRW same box, LRS unchanged; the backward
    #         twin measured SLOWER — its join waits for the weight gradients queued on that stream — and is not here)
    branch = None if not down else "fold" if training and act == 1 else "side" if training and side.enabled else "serial"
    if branch == "fold":
        side.run(lambda: _conv_stats(st, tape, x, *convd, 1, stride, 0, True), x)
    elif branch == "side":
        side.run(lambda: _conv_bn(st, tape, x, *convd, 1, stride, 0, training, None, 0), x)
    o1 = _conv_bn(st, tape, x, *conv1, 3, stride, 1, training, None, act)
    if branch == "fold":
        t2 = _conv_stats(st, tape, o1, *conv2, 3, 1, 1, True, None, 1)
        side.join()
        td = tape[convd[0]]
        b2, bd = t2["bn"], td["bn"]
        t2["y"] = ops.bn_act_fwd2(t2["c"], td["c"], b2.mean, b2.rstd, b2.gamma, b2.beta, bd.mean, bd.rstd, bd.gamma, bd.beta)      # relu(bn2(c) + bn_d(c_d))
        return t2["y"]
    idt = x
    if branch == "side":
        side.join()
        idt = tape[convd[0]]["y"]
    elif branch == "serial":
        idt = _conv_bn(st, tape, x, *convd, 1, stride, 0, training, None, 0)
    return _conv_bn(st, tape, o1, *conv2, 3, 1, 1, training, idt, act)


def _frontend_forward(model, st: "_ParamStore", tape: dict, videos: torch.Tensor, training: bool) -> torch.Tensor:
    """videos: fp32 [B,1,T,H,W] (LRW) — the LRS layout [B,T,1,H,W] is the same memory.  -> [B*T, 512] bf16."""
    bn = st.bnh(model.stem_name + ".1")
    c, stats = ops.stem_conv_fwd(videos, st.p32(model.stem_name + ".0.weight"), want_stats=training)
    _bn_stats(bn, training, c.numel() // 64, stats)
    out = ops.stem_bn_gelu_pool_fwd(c, bn.mean, bn.rstd, bn.gamma, bn.beta, model.stem_act, want_win=training)
    x, amax, xwin = out if training else (*out, None)          # xwin: the convolution output at every pooling window's arg-max, for the backward
    tape["stem"] = dict(videos=videos, c=c, amax=amax, xwin=xwin, bn=bn, pooled_shape=tuple(x.shape))
    for blk in _trunk_blocks(model):
        x = _block_forward(model, st, tape, x, blk, training)
    tape["trunk_out_shape"] = tuple(x.shape)
    return ops.avgpool_fwd(x)            # [N, 512] bf16


def _bn2_backward(t2: dict, td: Optional[dict], dx: torch.Tensor, dx_stats, act: int) -> tuple:
    """The block-end BatchNorm from dx, the gradient of the block's output -> (dc2, dres, dcd): the gradients of conv2's output, of the
    residual branch's output and — where this step finishes the 1x1 branch's BatchNorm too — of that branch's convolution (else None)."""
    bn = t2["bn"]
    if dx_stats is None:
        return (*ops.bn_act_bwd(dx, t2["y"], t2["c"], bn.mean, bn.rstd, bn.gamma, bn.coef, bn.dgamma, bn.dbeta, act, True, beta=bn.beta, res=t2["res"]), None)
    if td is None or act != 1:
        return _bn_from_stats(t2, dx, dx_stats), dx, None
    # dx is the gradient of the 1x1 branch's BatchNorm output too: bn2's apply pass takes the first pass of that BatchNorm's backward
    # along, and the branch is finished right behind it, while its partial rows are what this stream's scratch holds
    bd = td["bn"]
    dc2, d_stats = ops.bn_bwd_from_stats_ds(dx, t2["c"], bn.mean, bn.rstd, bn.gamma, dx_stats, bn.coef, bn.dgamma, bn.dbeta, td["c"], bd.mean, bd.rstd)
    return dc2, dx, _bn_from_stats(td, dx, d_stats)


def _bn1_backward(t1: dict, dc2: torch.Tensor, w2t: torch.Tensor, act: int, fused: bool) -> torch.Tensor:
    """conv2's data gradient and bn1 -> dc1, the gradient of conv1's output."""
    bn, hw = t1["bn"], t1["c"].shape[1:3]
    if fused:
        # bn1 has no residual branch: the mask / pre-activation is recomputed from its input (y is not read)
        return _bn_from_stats(t1, *ops.conv2d_dgrad_bn(dc2, w2t, 3, 1, 1, hw, None, None, t1["c"], bn.mean, bn.rstd, bn.gamma, bn.beta, act))
    return ops.bn_act_bwd(ops.conv2d_dgrad(dc2, w2t, 3, 1, 1, hw), t1["y"], t1["c"], bn.mean, bn.rstd, bn.gamma, bn.coef, bn.dgamma, bn.dbeta, act, False, beta=bn.beta)[0]


def _epilogue(t: dict, act: int) -> tuple:
    """What the epilogue of a data-gradient launch needs to turn the gradient of a block's output (t = that block's conv2 entry) into the
    gradient of bn2's output: (ReLU: the output, its mask; Swish: the residual input, whose pre-activation it rebuilds, c, ..., act)."""
    bn = t["bn"]
    return (t["y"] if act == 1 else t["res"], t["c"], bn.mean, bn.rstd, bn.gamma, bn.beta, act)


def _dgrad3x3(dy: torch.Tensor, wt: torch.Tensor, stride: int, in_hw, addend: Optional[torch.Tensor], epi: Optional[tuple]) -> tuple:
    """3x3 data gradient (+ addend, in place), with the epilogue `epi` (_epilogue) when there is one -> (dx, dx_stats or None)."""
    if epi is None:
        return ops.conv2d_dgrad(dy, wt, 3, stride, 1, in_hw, addend=addend), None
    return ops.conv2d_dgrad_bn(dy, wt, 3, stride, 1, in_hw, addend, *epi)


def _input_grad(st: "_ParamStore", blk: tuple, in_hw, dc1: torch.Tensor, dres: torch.Tensor, dcd: Optional[torch.Tensor], epi: Optional[tuple]) -> tuple:
    """The gradient of the block's input from both branches -> (dx, dx_stats or None)."""
    prefix, inp, planes, stride, down = blk
    w1t = st.t16(f"{prefix}.conv1.weight").view(inp, 3, 3, planes)
    if not down:
        return _dgrad3x3(dc1, w1t, stride, in_hw, dres, epi)
    wdt = st.t16(f"{prefix}.downsample.0.weight").view(inp, 1, 1, planes)
    if ops.DGRAD2 and stride == 2:
        # one launch: the 1x1 branch reaches exactly the pixels of the 3x3 gradient's centre tap and is one more tap of that class
        out = ops.conv2d_dgrad2(dc1, w1t, dcd, wdt, in_hw, bn=epi)
        return out if epi is not None else (out, None)
    # two launches: the 1x1 branch first (pixels its stride skips are written as zeros), the 3x3 branch adds to it
    return _dgrad3x3(dc1, w1t, stride, in_hw, ops.conv2d_dgrad(dcd, wdt, 1, stride, 0, in_hw), epi)


def _block_backward(model, st: "_ParamStore", tape: dict, blk: tuple, below: Optional[dict], dx: torch.Tensor, dx_stats) -> tuple:
    """One BasicBlock from the gradient of its output to that of its input.  below: the conv2 entry of the block below (None: the stem
    is), whose output is that input.  dx_stats not None: dx is already masked, these are its bn2's partial rows.  -> the next (dx, dx_stats)."""
    prefix, planes, act = blk[0], blk[2], model.trunk_act
    # The launch that produces the gradient of a BatchNorm + activation output also masks it (1 ReLU, LRW) or multiplies it by swish'
    # (2 Swish, LRS) and takes the first pass of that BatchNorm's backward in its epilogue (ops.conv2d_dgrad_bn)
    fused = act in (1, 2) and ops.BN_BWD_FUSED
    t2, t1, td = tape[f"{prefix}.conv2"], tape[f"{prefix}.conv1"], tape.get(f"{prefix}.downsample.0")
    dc2, dres, dcd = _bn2_backward(t2, td, dx, dx_stats, act)
    _conv_wgrad(model, st, f"{prefix}.conv2", t2, dc2)
    dc1 = _bn1_backward(t1, dc2, st.t16(f"{prefix}.conv2.weight").view(planes, 3, 3, planes), act, fused)
    _conv_wgrad(model, st, f"{prefix}.conv1", t1, dc1)
    if td is not None:
        if dcd is None:       # bn2's pass did not take the branch's BatchNorm along
            bd = td["bn"]
            dcd, _ = ops.bn_act_bwd(dres, None, td["c"], bd.mean, bd.rstd, bd.gamma, bd.coef, bd.dgamma, bd.dbeta, 0, False)
        _conv_wgrad(model, st, f"{prefix}.downsample.0", td, dcd)
    out = _input_grad(st, blk, t1["x"].shape[1:3], dc1, dres, dcd, _epilogue(below, act) if fused and below is not None else None)
    _ready(model, st, f"{prefix}.conv1.weight")
    return out


def _frontend_backward(model, st: "_ParamStore", tape: dict, dfeats: torch.Tensor) -> None:
    dx, dx_stats = ops.avgpool_bwd(dfeats, tape["trunk_out_shape"]), None
    blocks = list(_trunk_blocks(model))
    rec = tape.get("_record_grads")       # tests: {block prefix: (gradient entering the block from above, is it already masked by relu')}
    for bi in range(len(blocks) - 1, -1, -1):
        if rec is not None:
            rec[blocks[bi][0]] = (dx.clone(), dx_stats is not None)
        dx, dx_stats = _block_backward(model, st, tape, blocks[bi], tape[f"{blocks[bi - 1][0]}.conv2"] if bi > 0 else None, dx, dx_stats)
    # the chain ends here: its last reduce goes out right behind the last halo launch and runs beside the stem's light passes
    _flush_w3_chain(model)
    ts = tape["stem"]
    if rec is not None:
        rec["stem"] = (dx.clone(), False)
    bn, gw = ts["bn"], st.g32(model.stem_name + ".0.weight")
    in_wgrad = ts["xwin"] is not None and ops.stem_bwd_wgrad_ok(ts["videos"])
    dconv = ops.stem_bn_gelu_pool_bwd(dx, ts["amax"], ts["c"], bn.mean, bn.rstd, bn.gamma, bn.beta, bn.coef, bn.dgamma, bn.dbeta, model.stem_act,
                                      xwin=ts["xwin"], want_dx=not in_wgrad)
    if in_wgrad:
        # The gradient of the convolution output is made tile by tile inside the weight-gradient pass, never written.  The side stream is
        # joined FIRST: the pass is a persistent grid of two 248-register workgroups per CU, and beside the last trunk weight gradients
        # (8-wave workgroups that leave no CU room for them) half its workgroups started late and the step LOST 0.02 / 0.4 ms (LRW / LRS);
        # alone it is 223 us against 105 + 134 (928 frames) and the sentence-level step gains 0.2 ms.
        _flush_deferred(model)
        model._side.join()
        early = model._early_sumsq      # the optimiser's device state, set by engine.TrainStep when no collective follows
        if early is not None and st.sumsq_head:
            # every gradient but the stem convolution's is final: their sum of squares (the global-norm clip's) runs beside that last pass
            # (part of the optimiser tail: under gradient accumulation a recorded list leaves it out of every micro-step but the last)
            with ops.window_group("tail"):
                model._side.run(lambda: ops.grad_sumsq_parts(st.grad, st.sumsq_head, st.numel - st.sumsq_head, early, 0, ops.SUMSQ_PARTS - 1))
            st.sumsq_tail_done = True
        ops.stem_bwd_wgrad(ts["videos"], dconv, ts["amax"], ts["c"], bn.mean, bn.rstd, bn.coef, gw)
    else:
        ops.stem_conv_wgrad(ts["videos"], dconv, gw)
    _flush_deferred(model)
    model._side.join()
    _ready(model, st, None)


# Timing experiments only (results WRONG): a probe script may set this to {"conv_wgrad"} / {"lin_wgrad"} to skip those launches.
# Deliberately not an environment switch: nothing outside an explicit assignment in a probe can turn gradients off.
_ABLATE: frozenset = frozenset()


def _conv_wgrad(model, st: "_ParamStore", conv: str, t: dict, dc: torch.Tensor) -> None:
    if "conv_wgrad" in _ABLATE:
        return
    if ops.halo_wgrad_ok(t["x"], dc, t["k"], t["stride"], t["pad"]):
        # a link of the trunk's chain (ops.conv3x3_wgrad_chain): this launch adds the previous halo launch's slabs into that weight's gradient
        # and leaves its own to the next one — a stand-alone reduce between two launches cannot become resident beside the main stream's
        # persistent data-gradient kernels and held the side stream for their whole length
        def link():
            model._w3_pending = ops.conv3x3_wgrad_chain(t["x"], dc, st.g32(f"{conv}.weight"), model._w3_pending)
        model._side.run(link, dc)
        _release_ready(model)       # what waited for the carried sum is final behind this launch
        return
    model._side.run(lambda: ops.conv2d_wgrad(t["x"], dc, st.g32(f"{conv}.weight"), t["k"], t["stride"], t["pad"]), dc)


def _flush_w3_chain(model) -> None:
    """Ends the chain of halo weight gradients: the last launch's slabs go through the stand-alone reduce, on the side stream."""
    pending, model._w3_pending = model._w3_pending, None
    if pending is not None:
        # (its operands are the slabs the side stream's own last halo launch wrote: nothing of the main stream to wait for)
        model._side.run(lambda: ops.conv3x3_wgrad_flush(pending), behind_main=False)
    _release_ready(model)


def _release_ready(model) -> None:
    """Issues the gradient-ready notifications _ready held back, in their order."""
    held, hook = model._ready_held, model.grad_ready_hook
    if held and hook is not None:
        for lo in held:
            ops.host_callback(lambda lo=lo: hook(lo))
    held.clear()


def _lin_wgrad(model, x, dy, gw, gb, rows: int, K: int, N: int, x_pitch: int, dy_pitch: int) -> None:
    """Weight (+ bias) gradient of a linear layer of either training model, handed to the side stream (a function call, so that the
    deferred launch sees THIS layer's tensors and not the loop variables of a later one)."""
    if "lin_wgrad" in _ABLATE:
        return
    group = model._wg_group
    if group is not None:          # collected: one grouped launch per flush (_flush_lin_wgrads: a word-level encoder layer, a decoder layer)
        group.append(dict(x=x, dy=dy, dw=gw, db=gb, rows=rows, K=K, N=N, x_pitch=x_pitch, dy_pitch=dy_pitch))
        return
    model._side.run(lambda: ops.linear_wgrad(x, dy, gw, rows=rows, K=K, N=N, x_pitch=x_pitch, dy_pitch=dy_pitch, db=gb), x, dy, small=True)


def _flush_lin_wgrads(model, tile: Optional[int] = None) -> None:
    """The linear weight gradients collected so far as ONE launch over a device table of problems (ops.linear_wgrad_group; problems the
    grouped kernel does not take go out on their own inside that call), on the side stream when weight gradients go there: nothing
    downstream reads them before the optimiser.  At ~800 rows each contraction is a 13-chunk K loop, 22 us of latency as a launch of its own.
    tile: ops.linear_wgrad_group's (a forced tile edge for a group large enough to fill the chip by itself)."""
    group, model._wg_group = model._wg_group, None
    if not group:
        return
    keep = [t for q in group for t in (q["x"], q["dy"])]
    model._side.run(lambda: ops.linear_wgrad_group(group, tile=tile), *keep, small=True)


def _defer_list(model) -> Optional[list]:
    """The list ops.add_ln_bwd / ops.bias_act_bwd append their postponed reductions to (None: reduce in line)."""
    return model._deferred if model._side.enabled or model._side.enabled_small else None


def _flush_deferred(model) -> None:
    d = model._deferred
    if d:
        fns, keep = [f for f, _ in d], [k for _, k in d]
        d.clear()
        model._side.run(lambda: ops.run_deferred(fns), *keep, small=True)


def _ready(model, st: "_ParamStore", name: Optional[str]) -> None:
    """Gradient-ready notification for bucketed all-reduce: everything at or above `name`'s offset in the decayed
    region is final (backward walks the flat buffer from its end to its start); None = all gradients final."""
    _flush_deferred(model)                    # postponed parameter-gradient reductions: to the side stream, once per layer
    if model.grad_ready_hook is not None:     # (the reducer's comm stream waits for the side stream itself: engine.GradReducer._reduce)
        hook, lo = model.grad_ready_hook, (0 if name is None else st.offsets[name][0])
        if model._w3_pending is not None:
            # a halo weight gradient above `lo` is still slabs: its sum is written by the launch that carries them (_conv_wgrad) or by the
            # chain's flush, and the notification follows that launch — later than before, in the same order
            model._ready_held.append(lo)
            return
        ops.host_callback(lambda: hook(lo))   # a host-side step (collective): a segment boundary of a recorded step list


def _encoder_forward(model: TransformerLightningModule, st: _ParamStore, tape: dict, feats: torch.Tensor, B: int, T: int) -> torch.Tensor:
    D, S, H = model.dim, T + 1, model.heads
    R = B * S
    pos = st.p32("encoder.embeddings.position_embeddings.weight")
    type0 = st.p32("encoder.embeddings.token_type_embeddings.weight")
    d_in, d_out = model._d("emb.in", "emb"), model._d("emb.out")
    s0, x, mean0, rstd0 = ops.embed_ln_fwd(feats, st.p32("cls_token"), pos, type0, st.p32("encoder.embeddings.LayerNorm.weight"),
                                           st.p32("encoder.embeddings.LayerNorm.bias"), B, S, D, model.ln_eps, drop_in=d_in, drop_out=d_out)
    tape["emb"] = dict(sum=s0, mean=mean0, rstd=rstd0, d_in=d_in, d_out=d_out)
    if ops.enc_fused_ok(D, H, model.inter, S):
        return _encoder_forward_fused(model, st, tape, x, B, S)
    for i in range(model.layers):
        p = f"encoder.encoder.layer.{i}"
        wqkv = st.s16(f"{p}.attention.self.query.weight", 3 * D * D)
        bqkv = st.flat[st.offsets[f"{p}.attention.self.query.bias"][0] :][: 3 * D]
        qkv, _ = ops.linear_fwd(x, wqkv, bqkv, rows=R, K=D, N=3 * D, x_pitch=D)
        dpr, dao, dfo = model._d(f"enc.{i}.attn.probs", "attn"), model._d(f"enc.{i}.attn.out"), model._d(f"enc.{i}.ff.out")
        ctx, probs = ops.mha_fwd(qkv, 3 * D, qkv[:, D:], qkv[:, 2 * D:], 3 * D, B=B, H=H, Lq=S, Lk=S, drop=dpr)      # csrc/mha.hip
        ao, _ = ops.linear_fwd(ctx, st.s16(f"{p}.attention.output.dense.weight"), st.p32(f"{p}.attention.output.dense.bias"),
                               rows=R, K=D, N=D, x_pitch=D, drop=dao)                      # BertSelfOutput: dropout(dense(ctx))
        x1, m1, r1 = ops.add_ln_fwd(ao, x, st.p32(f"{p}.attention.output.LayerNorm.weight"), st.p32(f"{p}.attention.output.LayerNorm.bias"), model.ln_eps)
        hg, z = ops.linear_fwd(x1, st.s16(f"{p}.intermediate.dense.weight"), st.p32(f"{p}.intermediate.dense.bias"),
                               rows=R, K=D, N=model.inter, x_pitch=D, gelu=True)
        f, _ = ops.linear_fwd(hg, st.s16(f"{p}.output.dense.weight"), st.p32(f"{p}.output.dense.bias"), rows=R, K=model.inter, N=D,
                              x_pitch=model.inter, drop=dfo)                               # BertOutput: dropout(dense(h))
        x2, m2, r2 = ops.add_ln_fwd(f, x1, st.p32(f"{p}.output.LayerNorm.weight"), st.p32(f"{p}.output.LayerNorm.bias"), model.ln_eps)
        tape[p] = dict(x=x, qkv=qkv, ctx=ctx, probs=probs, ao=ao, x1=x1, m1=m1, r1=r1, z=z, hg=hg, f=f, m2=m2, r2=r2, dpr=dpr, dao=dao, dfo=dfo)
        x = x2
    return x


def _encoder_forward_fused(model: TransformerLightningModule, st: _ParamStore, tape: dict, x: torch.Tensor, B: int, S: int) -> torch.Tensor:
    """All encoder layers in one launch (ops.enc_fwd, csrc/enc_fused.hip); fills the same tape entries as the per-layer path."""
    D, H, I, Lc = model.dim, model.heads, model.inter, model.layers
    R = B * S
    dev = x.device
    ldp = ops.probs_pitch(S)
    # one allocation per tensor kind for all layers
    qkv = torch.empty((Lc, R, 3 * D), dtype=BF16, device=dev)
    probs = torch.empty((Lc, B * H, S, ldp), dtype=BF16, device=dev)
    act = torch.empty((5, Lc, R, D), dtype=BF16, device=dev)               # ctx, ao, x1, f, xout
    zz = torch.empty((2, Lc, R, I), dtype=BF16, device=dev)                # z, hg
    stat = torch.empty((4, Lc, R), dtype=torch.float32, device=dev)        # m1, r1, m2, r2
    training = model.training
    recs = []
    xin = x
    for i in range(Lc):
        p = f"encoder.encoder.layer.{i}"
        dpr, dao, dfo = model._d(f"enc.{i}.attn.probs", "attn"), model._d(f"enc.{i}.attn.out"), model._d(f"enc.{i}.ff.out")
        rec = dict(
            wqkv=st.s16(f"{p}.attention.self.query.weight", 3 * D * D), wo=st.s16(f"{p}.attention.output.dense.weight"),
            w1=st.s16(f"{p}.intermediate.dense.weight"), w2=st.s16(f"{p}.output.dense.weight"),
            bqkv=st.flat[st.offsets[f"{p}.attention.self.query.bias"][0]:][: 3 * D], bo=st.p32(f"{p}.attention.output.dense.bias"),
            b1=st.p32(f"{p}.intermediate.dense.bias"), b2=st.p32(f"{p}.output.dense.bias"),
            g1=st.p32(f"{p}.attention.output.LayerNorm.weight"), be1=st.p32(f"{p}.attention.output.LayerNorm.bias"),
            g2=st.p32(f"{p}.output.LayerNorm.weight"), be2=st.p32(f"{p}.output.LayerNorm.bias"),
            qkv=qkv[i], probs=probs[i], ctx=act[0, i], ao=act[1, i], x1=act[2, i], z=zz[0, i], hg=zz[1, i], f=act[3, i], xout=act[4, i],
            m1=stat[0, i], r1=stat[1, i], m2=stat[2, i], r2=stat[3, i],
            site_probs=model._sites[f"enc.{i}.attn.probs"], site_ao=model._sites[f"enc.{i}.attn.out"], site_fo=model._sites[f"enc.{i}.ff.out"])
        recs.append(rec)
        tape[p] = dict(x=xin, qkv=rec["qkv"], ctx=rec["ctx"], probs=rec["probs"], ao=rec["ao"], x1=rec["x1"], m1=rec["m1"], r1=rec["r1"], z=rec["z"],
                       hg=rec["hg"], f=rec["f"], m2=rec["m2"], r2=rec["r2"], dpr=dpr, dao=dao, dfo=dfo)
        xin = rec["xout"]
    on = training and (model.drop_p > 0.0 or model.attn_drop_p > 0.0)
    ops.enc_fwd(x, recs, B, S, model.ln_eps, model._drop_word if on else None, model.drop_p if training else 0.0,
                model.attn_drop_p if training else 0.0)
    return xin


def _encoder_layers_backward_fused(model: TransformerLightningModule, st: _ParamStore, tape: dict, dh: torch.Tensor, B: int, S: int,
                                   defer: Optional[list]) -> torch.Tensor:
    """The backward of all encoder layers in one launch (ops.enc_bwd, csrc/enc_fused.hip k_enc_bwd), then the parameter gradients it leaves
    to the weight-gradient launches.  Every operand of every layer's contractions exists when that launch returns, so with a collector
    (model._wg_group) all of them — attention.output.dense included, unsplit — go out as ONE grouped launch on ops.ENC_WGRAD_TILE-wide tiles
    and the LayerNorm parameter sums as one svsr_colsum_rows_multi launch, followed by the layers' gradient-ready notifications in the order
    the per-layer path below gives them (what was collected before, the heads' linears, is flushed first, as a group of its own).  Without a
    collector: the same calls, in the same order, as the per-layer path.  Returns the gradient of the first layer's input."""
    D, H, I, Lc = model.dim, model.heads, model.inter, model.layers
    R = B * S
    dev = dh.device
    t0 = tape["encoder.encoder.layer.0"]
    hidden_drop = t0["dfo"] is not None or t0["dao"] is not None
    act = torch.empty((6 if hidden_drop else 4, Lc, R, D), dtype=BF16, device=dev)      # ds2, dx1, ds1, dx (, df, dao)
    dz = torch.empty((Lc, R, I), dtype=BF16, device=dev)
    dqkv = torch.empty((Lc, R, 3 * D), dtype=BF16, device=dev)
    part = torch.empty((Lc, 2, B, 2 * D), dtype=torch.float32, device=dev)              # [layer][LayerNorm 1 | 2][sequence][dy*xhat | dy]
    recs = []
    for i in range(Lc):
        p = f"encoder.encoder.layer.{i}"
        t = tape[p]
        recs.append(dict(
            w2t=st.t16(f"{p}.output.dense.weight"), w1t=st.t16(f"{p}.intermediate.dense.weight"),
            wot=st.t16(f"{p}.attention.output.dense.weight"), wqkvt=st.t16(f"{p}.qkv"),
            g1=st.p32(f"{p}.attention.output.LayerNorm.weight"), g2=st.p32(f"{p}.output.LayerNorm.weight"),
            f=t["f"], x1=t["x1"], ao=t["ao"], xin=t["x"], z=t["z"], qkv=t["qkv"], probs=t["probs"], m1=t["m1"], r1=t["r1"], m2=t["m2"], r2=t["r2"],
            ds2=act[0, i], dx1=act[1, i], ds1=act[2, i], dx=act[3, i], df=act[4, i] if hidden_drop else act[0, i],
            dao=act[5, i] if hidden_drop else act[2, i], dz=dz[i], dqkv=dqkv[i], part1=part[i, 0], part2=part[i, 1],
            site_probs=model._sites[f"enc.{i}.attn.probs"], site_ao=model._sites[f"enc.{i}.attn.out"], site_fo=model._sites[f"enc.{i}.ff.out"]))
    on = hidden_drop or t0["dpr"] is not None
    ops.enc_bwd(dh, recs, B, S, model._drop_word if on else None, model.drop_p if hidden_drop else 0.0,
                model.attn_drop_p if t0["dpr"] is not None else 0.0)

    merged = model._wg_group is not None
    ln_sums: list = []         # merged: the 2 x layers LayerNorm parameter sums, one svsr_colsum_rows_multi launch behind the loop

    def ln_grads(rows, name):
        gw, gb = st.g32(f"{name}.weight"), st.g32(f"{name}.bias")
        if merged:
            ln_sums.append((ops._deferred_colsum(rows, B, 2 * D, gw, D, gb, D), rows))
        elif defer is None:
            ops.colsum_rows(rows, B, 2 * D, gw, D, gb, D)
        else:
            defer.append((lambda: ops.colsum_rows(rows, B, 2 * D, gw, D, gb, D), rows))

    if merged:
        _flush_lin_wgrads(model)
        model._wg_group = []
    for i in reversed(range(Lc)):
        p = f"encoder.encoder.layer.{i}"
        t, q = tape[p], recs[i]
        ln_grads(q["part2"], f"{p}.output.LayerNorm")
        _lin_wgrad(model, t["hg"], q["df"], st.g32(f"{p}.output.dense.weight"), st.g32(f"{p}.output.dense.bias"), R, I, D, I, D)
        # (the intermediate bias's gradient: the column sums of dz, taken by the weight-gradient launch)
        _lin_wgrad(model, t["x1"], q["dz"], st.g32(f"{p}.intermediate.dense.weight"), st.g32(f"{p}.intermediate.dense.bias"), R, D, I, D, I)
        ln_grads(q["part1"], f"{p}.attention.output.LayerNorm")
        _lin_wgrad(model, t["ctx"], q["dao"], st.g32(f"{p}.attention.output.dense.weight"), st.g32(f"{p}.attention.output.dense.bias"), R, D, D, D, D)
        gq = st.grad[st.offsets[f"{p}.attention.self.query.weight"][0]:][: 3 * D * D]
        gqb = st.grad[st.offsets[f"{p}.attention.self.query.bias"][0]:][: 3 * D]
        _lin_wgrad(model, t["x"], q["dqkv"], gq, gqb, R, D, 3 * D, D, 3 * D)
        if not merged:
            _flush_deferred(model)
            _ready(model, st, f"{p}.attention.self.query.weight")
    if merged:
        if defer is None:
            ops.run_deferred([f for f, _ in ln_sums])
        else:
            defer.extend(ln_sums)
            _flush_deferred(model)
        _flush_lin_wgrads(model, tile=ops.ENC_WGRAD_TILE)
        model._wg_group = []          # (empty: the caller's closing flush issues nothing and notifies layer 0)
        for i in reversed(range(1, Lc)):
            _ready(model, st, f"encoder.encoder.layer.{i}.attention.self.query.weight")
    return recs[0]["dx"]


def _encoder_backward(model: TransformerLightningModule, st: _ParamStore, tape: dict, dh: torch.Tensor, B: int, T: int) -> torch.Tensor:
    D, S, H, I = model.dim, T + 1, model.heads, model.inter
    R = B * S
    dx = dh
    # parameter-gradient reductions of the row passes (LayerNorm gamma / beta, the intermediate bias): nothing downstream waits for them, so
    # they leave the chain of dependent launches and run on the side stream, one hand-over per layer (_flush_deferred, from _ready)
    defer = _defer_list(model)

    fused = ops.ENC_BWD_FUSED and ops.enc_fused_ok(D, H, I, S) and model.layers <= 8
    if fused:
        dx = _encoder_layers_backward_fused(model, st, tape, dh, B, S, defer)
    for i in reversed(range(0 if fused else model.layers)):
        p = f"encoder.encoder.layer.{i}"
        t = tape[p]
        ds2 = ops.add_ln_bwd(dx, t["f"], t["x1"], st.p32(f"{p}.output.LayerNorm.weight"), t["m2"], t["r2"],
                             st.g32(f"{p}.output.LayerNorm.weight"), st.g32(f"{p}.output.LayerNorm.bias"), defer=defer)
        # ds2 is the gradient of (dropout(f) + x1): the dense layer sees it through the regenerated mask, the skip path as it is
        df = ds2 if t["dfo"] is None else ops.scale_bf16(ds2, 1.0, drop=t["dfo"])
        _lin_wgrad(model, t["hg"], df, st.g32(f"{p}.output.dense.weight"), st.g32(f"{p}.output.dense.bias"), R, I, D, I, D)
        dhg = ops.linear_dgrad(df, st.t16(f"{p}.output.dense.weight"), rows=R, N=D, K=I, dy_pitch=D)
        dz = ops.bias_act_bwd(dhg, t["z"], st.g32(f"{p}.intermediate.dense.bias"), R=R, N=I, n_valid=I, ld=I, defer=defer)
        _lin_wgrad(model, t["x1"], dz, st.g32(f"{p}.intermediate.dense.weight"), None, R, D, I, D, I)
        # (not in place: the side stream may still be reading ds2 / ds1 for the weight gradients)
        dx1 = ops.linear_dgrad(dz, st.t16(f"{p}.intermediate.dense.weight"), rows=R, N=I, K=D, dy_pitch=I, addend=ds2)
        ds1 = ops.add_ln_bwd(dx1, t["ao"], t["x"], st.p32(f"{p}.attention.output.LayerNorm.weight"), t["m1"], t["r1"],
                             st.g32(f"{p}.attention.output.LayerNorm.weight"), st.g32(f"{p}.attention.output.LayerNorm.bias"), defer=defer)
        dao_ = ds1 if t["dao"] is None else ops.scale_bf16(ds1, 1.0, drop=t["dao"])
        _lin_wgrad(model, t["ctx"], dao_, st.g32(f"{p}.attention.output.dense.weight"), st.g32(f"{p}.attention.output.dense.bias"), R, D, D, D, D)
        dctx = ops.linear_dgrad(dao_, st.t16(f"{p}.attention.output.dense.weight"), rows=R, N=D, K=D, dy_pitch=D)
        qkv = t["qkv"]
        dqkv = torch.empty_like(qkv)
        ops.mha_bwd(dctx, qkv, 3 * D, qkv[:, D:], qkv[:, 2 * D:], 3 * D, t["probs"], B=B, H=H, Lq=S, Lk=S, dq=dqkv, dq_pitch=3 * D,
                    dk=dqkv[:, D:], dv=dqkv[:, 2 * D:], dkv_pitch=3 * D, drop=t["dpr"])
        gq = st.grad[st.offsets[f"{p}.attention.self.query.weight"][0] :][: 3 * D * D]
        gqb = st.grad[st.offsets[f"{p}.attention.self.query.bias"][0] :][: 3 * D]
        _lin_wgrad(model, t["x"], dqkv, gq, gqb, R, D, 3 * D, D, 3 * D)
        dx = ops.linear_dgrad(dqkv, st.t16(f"{p}.qkv"), rows=R, N=3 * D, K=D, dy_pitch=3 * D, addend=ds1)
        _flush_deferred(model)
        if model._wg_group is None:
            _ready(model, st, f"{p}.attention.self.query.weight")
        elif i > 0:
            # the weight gradients collected so far as one launch on the side stream NOW: the encoder's backward is a chain of small
            # launches that leaves most of the chip idle, while a single launch at its end competes with the trunk's backward
            _flush_lin_wgrads(model)
            model._wg_group = []
            _ready(model, st, f"{p}.attention.self.query.weight")
    if model._wg_group is not None:
        # the remaining linear weight gradients of the encoder (and the heads) in one launch; their flat-buffer range is final from here
        _flush_lin_wgrads(model)
        _ready(model, st, "encoder.encoder.layer.0.attention.self.query.weight")
    te = tape["emb"]
    if te["d_out"] is not None:
        dx = ops.scale_bf16(dx, 1.0, drop=te["d_out"])
    ds0 = ops.add_ln_bwd(dx, te["sum"], None, st.p32("encoder.embeddings.LayerNorm.weight"), te["mean"], te["rstd"],
                         st.g32("encoder.embeddings.LayerNorm.weight"), st.g32("encoder.embeddings.LayerNorm.bias"), defer=defer)
    dfeats = ops.embed_bwd_scatter(ds0, st.g32("cls_token"), st.g32("encoder.embeddings.position_embeddings.weight"),
                                   st.g32("encoder.embeddings.token_type_embeddings.weight"), B, S, D, drop_in=te["d_in"])
    _ready(model, st, "cls_token")
    return dfeats


# ----------------------------------------------------------------------------------------------------
# `type: x-transformers` encoder (lightning.py:93-105,157-158): pre-norm residual blocks
#   x += to_out(attention(rotary(to_q|to_k|to_v(RMSNorm(x)))));   x += W2 . dropout(value * gelu(gate)) (+ biases), [value|gate] = W1 . RMSNorm(x)
# with whole blocks skipped at random in training (layer_dropout).  Rows are `dim_p` wide (513 -> 576), pads zero.
# ----------------------------------------------------------------------------------------------------
def _xt_skips(model) -> set:
    """Indices n of `encoder.layers.{n}` skipped this step: AttentionLayers.forward draws python's random() once per layer, in
    order, and skips the layer when it falls below layer_dropout (training only)."""
    if not model.training or model.layer_drop_p <= 0.0:
        return set()
    if model.layer_skip_override is not None:
        return set(model.layer_skip_override)
    return {n for n in range(2 * model.layers) if model._layer_rng.random() < model.layer_drop_p}


def _xt_block_fwd(model, st: _ParamStore, tape: dict, x: torch.Tensor, n: int, B: int, S: int, tab: torch.Tensor, nrot: int) -> torch.Tensor:
    """Block `encoder.layers.{n}` (even n: attention, odd n: feed-forward) on the residual stream x -> the block's output x1."""
    D, Dp, H, E = model.dim, model.dim_p, model.heads, model.attn_inner
    I, Ip, Up = model.inter, model.inter_p, model.glu_p
    R, i, b = B * S, n // 2, f"encoder.layers.{n}"
    h, inv = ops.rmsnorm_fwd(x, st.p32(f"{b}.0.0.g"), D, model.rms_eps)
    if n % 2 == 0:
        qkv, _ = ops.linear_fwd(h, st.s16(f"{b}.1.to_q.weight", 3 * E * Dp), None, rows=R, K=Dp, N=3 * E, x_pitch=Dp)
        ops.rotary_(qkv, tab, S, nrot, 1)
        dpr = model._d(f"enc.{i}.attn.probs", "attn")
        ctx, probs = ops.mha_fwd(qkv, 3 * E, qkv[:, E:], qkv[:, 2 * E:], 3 * E, B=B, H=H, Lq=S, Lk=S, drop=dpr)
        x1, _ = ops.linear_fwd(ctx, st.s16(f"{b}.1.to_out.weight"), None, rows=R, K=E, N=Dp, x_pitch=E, addend=x)
        tape[b] = dict(x=x, h=h, inv=inv, qkv=qkv, ctx=ctx, probs=probs, dpr=dpr)
    else:
        u, _ = ops.linear_fwd(h, st.s16(f"{b}.1.ff.0.proj.weight"), st.p32(f"{b}.1.ff.0.proj.bias"), rows=R, K=Dp, N=Up, x_pitch=Dp)
        dff = model._d(f"enc.{i}.ff.hidden")
        y = ops.geglu_fwd(u, I, Ip, drop=dff)
        x1, _ = ops.linear_fwd(y, st.s16(f"{b}.1.ff.3.weight"), st.p32(f"{b}.1.ff.3.bias"), rows=R, K=Ip, N=Dp, x_pitch=Ip, addend=x)
        tape[b] = dict(x=x, h=h, inv=inv, u=u, y=y, dff=dff)
    return x1


def _xt_block_bwd(model, st: _ParamStore, tape: dict, dx: torch.Tensor, n: int, B: int, S: int) -> torch.Tensor:
    """Backward of block `encoder.layers.{n}`: gradient of the residual stream after the block -> before it (the weight gradients go to
    the flat buffer, on the side stream)."""
    D, Dp, H, E = model.dim, model.dim_p, model.heads, model.attn_inner
    I, Ip, Up = model.inter, model.inter_p, model.glu_p
    R, b, t, tx = B * S, f"encoder.layers.{n}", tape[f"encoder.layers.{n}"], tape["xt"]
    if n % 2 == 1:
        _lin_wgrad(model, t["y"], dx, st.g32(f"{b}.1.ff.3.weight"), st.g32(f"{b}.1.ff.3.bias"), R, Ip, Dp, Ip, Dp)
        dy = ops.linear_dgrad(dx, st.t16(f"{b}.1.ff.3.weight"), rows=R, N=Dp, K=Ip, dy_pitch=Dp)
        du = ops.geglu_bwd(dy, t["u"], I, drop=t["dff"])
        _lin_wgrad(model, t["h"], du, st.g32(f"{b}.1.ff.0.proj.weight"), st.g32(f"{b}.1.ff.0.proj.bias"), R, Dp, Up, Dp, Up)
        dhn = ops.linear_dgrad(du, st.t16(f"{b}.1.ff.0.proj.weight"), rows=R, N=Up, K=Dp, dy_pitch=Up)
    else:
        _lin_wgrad(model, t["ctx"], dx, st.g32(f"{b}.1.to_out.weight"), None, R, E, Dp, E, Dp)
        dctx = ops.linear_dgrad(dx, st.t16(f"{b}.1.to_out.weight"), rows=R, N=Dp, K=E, dy_pitch=Dp)
        qkv = t["qkv"]
        dqkv = torch.empty_like(qkv)
        ops.mha_bwd(dctx, qkv, 3 * E, qkv[:, E:], qkv[:, 2 * E:], 3 * E, t["probs"], B=B, H=H, Lq=S, Lk=S, dq=dqkv, dq_pitch=3 * E,
                    dk=dqkv[:, E:], dv=dqkv[:, 2 * E:], dkv_pitch=3 * E, drop=t["dpr"])
        ops.rotary_(dqkv, tx["tab"], S, tx["nrot"], -1)           # the rotation is orthogonal: its transpose is the inverse rotation
        gq = st.grad[st.offsets[f"{b}.1.to_q.weight"][0]:][: 3 * E * Dp]
        _lin_wgrad(model, t["h"], dqkv, gq, None, R, Dp, 3 * E, Dp, 3 * E)
        dhn = ops.linear_dgrad(dqkv, st.t16(f"{b}.1.qkv"), rows=R, N=3 * E, K=Dp, dy_pitch=3 * E)
    return ops.rmsnorm_bwd(dhn, t["x"], st.p32(f"{b}.0.0.g"), t["inv"], st.g32(f"{b}.0.0.g"), D, addend=dx)


def _xt_grouped(model, rec, n: int, fn, inp: torch.Tensor) -> torch.Tensor:
    """Replayable layer drop (rec = ops.layer_groups()): block n's launches as op group n of the recorded list, then the pass-through
    copy that every replay skipping n issues instead (the block's input, whole padded rows, into its output buffer)."""
    with rec.group(n):
        out = fn()
    rec.passthrough(out, inp, n)
    return out


def _xt_encoder_forward(model, st: _ParamStore, tape: dict, feats: torch.Tensor, wm: Optional[torch.Tensor], B: int, T: int) -> torch.Tensor:
    D, Dp, S, H = model.dim, model.dim_p, T + 1, model.heads
    d_in = model._d("emb.in", "emb")
    x = ops.xt_embed_fwd(feats, wm, st.p32("cls_token"), B, S, feats.shape[-1], D, Dp, drop=d_in)
    key = (S, str(feats.device))
    if key not in model._rot_tab:
        model._rot_tab[key] = ops.rotary_table(S, feats.device)
    tab = model._rot_tab[key]
    # under a recorder that replays layer drop (engine.TrainStep(native=True)) every block is emitted: the skip set was drawn by the
    # engine, where this draws it in an eager step
    rec = ops.layer_groups()
    skip = _xt_skips(model) if rec is None else set()
    nrot = (3 if model.rotate_value else 2) * H
    tape["xt"] = dict(d_in=d_in, tab=tab, nrot=nrot, F=feats.shape[-1], grouped=rec is not None)
    for n in range(2 * model.layers):
        if n in skip:
            continue
        if rec is None:
            x = _xt_block_fwd(model, st, tape, x, n, B, S, tab, nrot)
        else:
            x = _xt_grouped(model, rec, n, lambda: _xt_block_fwd(model, st, tape, x, n, B, S, tab, nrot), x)
    if model.final_norm:
        h, inv = ops.rmsnorm_fwd(x, st.p32("encoder.final_norm.g"), D, model.rms_eps)
        tape["xt"]["final"] = dict(x=x, inv=inv)
        x = h
    return x


def _xt_encoder_backward(model, st: _ParamStore, tape: dict, dh: torch.Tensor, B: int, T: int) -> torch.Tensor:
    D, S = model.dim, T + 1
    tx = tape["xt"]
    rec = ops.layer_groups() if tx["grouped"] else None
    if tx["grouped"] and rec is None:
        raise RuntimeError("the forward emitted op groups for a recorded step list: its backward must run in the same recording")
    dx = dh
    if "final" in tx:
        dx = ops.rmsnorm_bwd(dx, tx["final"]["x"], st.p32("encoder.final_norm.g"), tx["final"]["inv"], st.g32("encoder.final_norm.g"), D)
    for i in reversed(range(model.layers)):
        for n in (2 * i + 1, 2 * i):
            if f"encoder.layers.{n}" not in tape:
                continue
            if rec is None:
                dx = _xt_block_bwd(model, st, tape, dx, n, B, S)
            else:
                dx = _xt_grouped(model, rec, n, lambda: _xt_block_bwd(model, st, tape, dx, n, B, S), dx)
        _ready(model, st, f"encoder.layers.{2 * i}.1.to_q.weight")
    dfeats = ops.xt_embed_bwd(dx, st.g32("cls_token"), B, S, tx["F"], D, drop=tx["d_in"])
    _ready(model, st, "cls_token")
    return dfeats


class _LrwFunction(torch.autograd.Function):
    """One autograd node for the whole model: forward records a tape, backward replays it by hand and writes the
    parameter gradients straight into the flat gradient buffer (the returned input gradients are all None)."""

    @staticmethod
    def forward(ctx, _anchor, model: TransformerLightningModule, st: _ParamStore, videos, audio_tokens, labels, need_grad: bool, word_mask=None):
        training = model.training
        B, _, T, H, W = videos.shape
        D, S = model.dim_p, T + 1            # storage width of the encoder rows (= dim unless the word boundary makes it 513 -> 576)
        A, G, V = model.audio_alignment, model.vq_groups, model.audio_vocab_size
        if not st.shadow_fresh:          # engine.TrainStep keeps the bf16 shadows current from its optimiser kernel
            st.refresh_shadows()
        if training and (model.drop_p > 0.0 or model.attn_drop_p > 0.0 or model.emb_drop_p > 0.0):
            model._advance_dropout(videos.device)
        tape: dict[str, Any] = {}
        feats = _frontend_forward(model, st, tape, videos, training)
        model._side.join()            # the previous step's optimiser may still be updating the encoder / heads on the side stream (engine.TrainStep)
        if model.encoder_type == "x-transformers":
            h = _xt_encoder_forward(model, st, tape, feats, word_mask, B, T)
        else:
            h = _encoder_forward(model, st, tape, feats, B, T)          # [B*S, D] bf16
        # word head: rows s = 0
        C = model.word_labels
        hard = labels.dtype in (torch.int64, torch.int32)
        lab_idx = labels.long() if hard else None
        lab_prob = None if hard else labels.float().contiguous()
        # (round 6) inside TrainStep the word head (classifier, its loss, the metric — and in the backward its loss gradient and data gradient) is a
        # branch of its own between the two encoder launches, of 1-8 workgroups per launch: it runs on the side stream beside the audio head
        side_heads = bool(model._metrics_on_side and model._side.enabled and need_grad
                          and model.encoder_type == "huggingface")       # (the heads' weight gradients then follow on the side stream too)
        hb: dict = {}

        def word_head():
            hb["logits_c"], _ = ops.linear_fwd(h, st.s16("category_classifier.weight"), st.p32("category_classifier.bias"), rows=B, K=D, N=C,
                                               x_pitch=D, out_f32=True, seq=(S, 0, 1))
            hb["loss_c"], hb["lse_c"] = ops.ce_fwd(hb["logits_c"], C, lab_idx, lab_prob, B, C, model.label_smoothing)
            if side_heads:
                hb["acc"] = ops.topk_acc(hb["logits_c"], lab_idx, lab_prob)

        if side_heads:
            model._side.run(word_head, h)
        else:
            word_head()
        logits_c, loss_c, lse_c = hb["logits_c"], hb["loss_c"], hb["lse_c"]
        # audio head: rows s = 1..T, logits [B*T, A*G*V] == [B*T*A*G, V]
        NA = A * G * V
        tok = audio_tokens.reshape(-1)
        fused_head = model.fused_audio_head and ops.linear_ce_ok(B * T, D, A * G, V)
        logits_a = None
        if not fused_head or model.keep_audio_logits:     # (keep_audio_logits: the logits tensor for inspection / the parity tests; the loss below does not read it)
            logits_a, _ = ops.linear_fwd(h, st.s16("audio_projection.weight"), st.p32("audio_projection.bias"), rows=B * T, K=D, N=NA,
                                         x_pitch=D, seq=(S, 1, T))
        if fused_head:
            # projection + per-frame cross-entropy in one contraction, logits never stored (csrc/audio_head.hip)
            loss_a, lse_a = ops.linear_ce_fwd(h, st.s16("audio_projection.weight"), st.p32("audio_projection.bias"), tok, B * T, D, A * G, V, seq=(S, 1, T))
        else:
            loss_a, lse_a = ops.ce_fwd(logits_a, V, tok, None, B * T * A * G, V, 0.0)
        if side_heads:
            acc = hb["acc"]
        elif model._metrics_on_side and model._side.enabled:
            # (round 6) inside TrainStep the metric is read when the step is over: its two launches leave the main stream's chain (the
            # side stream is joined at the end of the backward)
            box: dict = {}
            model._side.run(lambda: box.__setitem__("acc", ops.topk_acc(logits_c, lab_idx, lab_prob)), logits_c)
            acc = box["acc"]
        else:
            acc = ops.topk_acc(logits_c, lab_idx, lab_prob)
        model._last = dict(logits_category=logits_c, logits_audio=logits_a, feats=feats, hidden=h)
        if need_grad:
            tape["head"] = dict(h=h, logits_c=logits_c, lse_c=lse_c, lab_idx=lab_idx, lab_prob=lab_prob, logits_a=None if fused_head else logits_a,
                                lse_a=lse_a, tok=tok, dims=(B, T, D, S, A, G, V, C), side_heads=side_heads)
            ctx.tape = tape
            ctx.model = model
            ctx.st = st
        ctx.mark_non_differentiable(acc)
        return loss_c, loss_a, acc

    @staticmethod
    def backward(ctx, g_cat, g_audio, _g_acc):
        model, st, tape = ctx.model, ctx.st, ctx.tape
        th = tape["head"]
        B, T, D, S, A, G, V, C = th["dims"]
        dev = th["h"].device
        g_cat, g_audio = _begin_backward(model, st, dev, g_cat, g_audio)
        NA = A * G * V
        Cp = (C + 63) // 64 * 64
        dlc = torch.empty((B, Cp), dtype=BF16, device=dev)          # (svsr_ce_bwd writes the pad columns C .. Cp - 1 as zeros)
        dh = torch.empty((B * S, D), dtype=BF16, device=dev)
        side_heads = bool(th.get("side_heads")) and model._side.enabled
        if th.get("side_heads") and not side_heads:
            model._side.join()          # (the forward's half of the branch ran there)

        def word_head_bwd():
            ops.ce_bwd(th["logits_c"], C, th["lab_idx"], th["lab_prob"], B, C, model.label_smoothing, th["lse_c"], g_cat, dlc, Cp)
            if side_heads:      # (rows s = 0 of dh; the audio head's data gradient below writes rows 1..T)
                ops.linear_dgrad(dlc, st.t16("category_classifier.weight"), rows=B, N=C, K=D, dy_pitch=Cp, out=dh, seq=(S, 0, 1))

        if side_heads:
            model._side.run(word_head_bwd, dlc, dh, g_cat)
        else:
            word_head_bwd()
        dla = torch.empty((B * T, NA), dtype=BF16, device=dev)
        if th["logits_a"] is None:        # fused head: the logits are recomputed, dla = g / (B T A G) * (softmax - onehot)
            ops.linear_ce_bwd(th["h"], st.s16("audio_projection.weight"), st.p32("audio_projection.bias"), th["tok"], B * T, D, A * G, V, th["lse_a"],
                              g_audio, dla, seq=(S, 1, T))
        else:
            ops.ce_bwd(th["logits_a"], V, th["tok"], None, B * T * A * G, V, 0.0, th["lse_a"], g_audio, dla, V)
        h = th["h"]
        grouped = model.encoder_type == "huggingface"
        model._wg_group = [] if grouped else None
        heads = (dict(x=h, dy=dla, dw=st.g32("audio_projection.weight"), rows=B * T, K=D, N=NA, x_pitch=D, dy_pitch=NA, seq=(S, 1, T), db=st.g32("audio_projection.bias")),
                 dict(x=h, dy=dlc, dw=st.g32("category_classifier.weight"), rows=B, K=D, N=C, x_pitch=D, dy_pitch=Cp, seq=(S, 0, 1), db=st.g32("category_classifier.bias")))
        for q in heads:
            if grouped:
                model._wg_group.append(q)
            else:
                ops.linear_wgrad(q["x"], q["dy"], q["dw"], rows=q["rows"], K=q["K"], N=q["N"], x_pitch=q["x_pitch"], dy_pitch=q["dy_pitch"], seq=q["seq"], db=q["db"])
        ops.linear_dgrad(dla, st.t16("audio_projection.weight"), rows=B * T, N=NA, K=D, dy_pitch=NA, out=dh, seq=(S, 1, T))
        if side_heads:
            model._side.join()
        else:
            ops.linear_dgrad(dlc, st.t16("category_classifier.weight"), rows=B, N=C, K=D, dy_pitch=Cp, out=dh, seq=(S, 0, 1))
        if not grouped:
            _ready(model, st, "audio_projection.weight")
        if model.encoder_type == "x-transformers":
            dfeats = _xt_encoder_backward(model, st, tape, dh, B, T)
        else:
            dfeats = _encoder_backward(model, st, tape, dh, B, T)
        _frontend_backward(model, st, tape, dfeats)
        ctx.tape = None
        return None, None, None, None, None, None, None, None
