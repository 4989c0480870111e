"""Training-step runtime around the HIP model: what Lightning's Trainer does for the reference (DDP gradient all-reduce,
global-norm clip, AdamW, cosine schedule — LRW/video/src/train.py:23-40, lightning.py:216-223) restated
for one process per GPU:

  * gradients live in ONE flat fp32 buffer laid out in forward order; the hand-written backward (model.py) finalises it from
    its end to its start and reports progress, so contiguous buckets are all-reduced (RCCL, average) on a side HIP stream
    while the rest of the backward still runs;
  * clip + AdamW + schedule + bf16 shadow refresh are two kernels over the flat buffers, with the step counter, the gradient
    norm and the learning rate kept on the device — nothing in a step depends on host values, so
  * the whole step (forward, backward, collectives, optimiser) CAN be captured once into a HIP graph and replayed
    (`use_graph=True`); the default is eager launches with the weight-gradient kernels on a side stream, which measures faster
    (host enqueue time is about half the GPU time of a step).
"""
from __future__ import annotations

from typing import Optional

import warnings

import torch
import torch.distributed as dist

from . import ops
from .config import Config
from .model import TransformerLightningModule, _StoreModule, _xt_skips
from .shape_cache import ShapeLRU, shape_key


import os as _os

_ROCTX = _os.environ.get("SVSR_ROCTX", "0") == "1"


def lrs_train_config(**kw) -> Config:
    """Optimiser / schedule / clip values of LRS/video/config/lrs3.yaml:66-77,97 in the layout TrainStep reads."""
    cfg = Config(optimizer=Config(lr=1e-3, betas=[0.9, 0.98], eps=1e-6, weight_decay=0.03),
                 scheduler=Config(name="cosine", num_warmup_steps=25000, num_training_steps=500000),
                 trainer=Config(gradient_clip_val=5.0))
    for k, v in kw.items():
        cfg.set_path(k.replace("__", "."), v)
    return cfg


def _rng_state_to_tensor(state) -> torch.Tensor:
    """random.Random.getstate() = (version, 625 words, gauss_next or None) as an int64 vector
    [version, 625 words, has_gauss, gauss bits]: plain numbers, nothing a checkpoint reader has to unpickle."""
    import struct

    version, words, gauss = state
    if len(words) != 625:
        raise ValueError("unexpected random.Random state layout")
    bits = 0 if gauss is None else struct.unpack("<q", struct.pack("<d", float(gauss)))[0]
    return torch.tensor([int(version), *[int(w) for w in words], 0 if gauss is None else 1, bits], dtype=torch.int64)


def _rng_state_from_tensor(t: torch.Tensor):
    import struct

    if t.dtype != torch.int64 or t.numel() != 628:
        raise ValueError("layer_rng in this checkpoint is not the int64[628] generator state TrainStep.state_dict writes "
                         "(pickled states of older checkpoints are refused)")
    v = [int(x) for x in t.cpu().tolist()]
    gauss = struct.unpack("<d", struct.pack("<q", v[627]))[0] if v[626] else None
    return (v[0], tuple(v[1:626]), gauss)


class _ShapeList:
    """One recorded step list of TrainStep(native=True, max_shapes > 1): its recorder, static inputs and outputs (bytes: what the recorder
    keeps alive)."""
    __slots__ = ("rec", "static", "out", "nbytes")

    def __init__(self) -> None:
        self.rec: Optional[ops.StepRecorder] = None
        self.static: Optional[list] = None
        self.out = None
        self.nbytes = 0


class AccumWindow:
    """Host bookkeeping of gradient accumulation (Lightning's `accumulate_grad_batches`): a window is `n` consecutive micro-steps.  plan()
    says what the micro-step that is due does — zero-fill the gradient buffer (the first of a window only), reduce it across the ranks and
    run the optimiser tail (the last only); advance() moves on when that micro-step is done; flush() closes a partial window (True when
    there is an accumulated gradient to step on); abort() abandons it.  Pure host logic: no device, no model."""

    def __init__(self, n: int = 1):
        if int(n) < 1:
            raise ValueError("accumulate_grad_batches must be >= 1")
        self.n = int(n)
        self.pos = 0

    def plan(self) -> dict:
        last = self.pos == self.n - 1
        return {"zero": self.pos == 0, "reduce": last, "optimise": last}

    def advance(self) -> None:
        self.pos = (self.pos + 1) % self.n

    def flush(self) -> bool:
        due = self.pos > 0
        self.pos = 0
        return due

    def abort(self) -> None:
        self.pos = 0

    def state_dict(self) -> dict:
        """{} at a window boundary (a checkpoint taken there keeps its keys), else {"accum_window": int64 [n, position]}."""
        return {"accum_window": torch.tensor([self.n, self.pos], dtype=torch.int64)} if self.pos else {}

    def load_state_dict(self, sd: dict) -> None:
        if "accum_window" not in sd:
            self.pos = 0
            return
        n, pos = (int(x) for x in sd["accum_window"].reshape(-1).tolist())
        if n != self.n or not 0 < pos < n:
            raise ValueError(f"this checkpoint was saved at micro-step {pos} of a window of {n}: it resumes only under accumulate={n} "
                             f"(this TrainStep accumulates {self.n})")
        self.pos = pos


class TrainStep:
    """forward + backward + (all-reduce) + clip + AdamW for the LRW model (`TransformerLightningModule`; its step takes
    (videos, audio_tokens, labels, word_mask)) or the LRS model (`lrs_model.E2E`; (x, lengths, audio_tokens, label));
    optionally one HIP graph per step.

    After step() returns, the tail of the optimiser step (AdamW of everything behind the front-end, its shadow transposes) may still be
    running on the model's side stream, beside whatever the main stream does next.  The model's own entry points join it where they need
    the parameters (forward before the encoder, forward_videos, state_dict, load_state_dict, the LRS scorers, refresh_shadows); code that
    touches parameters DIRECTLY (p.data, p.cpu(), an EMA update) calls synchronize() first.

    Gradient accumulation (`accumulate=N`, or `accumulate_grad_batches` of the config: Lightning's automatic optimisation under
    strategy="ddp").  N consecutive step() calls (micro-steps) form a window: every micro-step's loss enters its backward times 1/N and the
    gradients add up in the flat buffer; the buffer is zeroed in the first micro-step only; the all-reduce (none is issued before: DDP's
    no_sync), the clip, AdamW, the shadow refresh, the schedule and state()["step"] happen in the last one only, on the accumulated gradient.
    BatchNorm statistics, the dropout word and the layer-drop draw advance in every micro-step; step() returns the unscaled losses of its
    micro-batch.  A window whose accumulated gradient norm is not finite is skipped as one unit.  flush() closes a partial window.
    An exception inside a micro-step ABANDONS the window: the micro-step may have added any part of its gradient to the buffer, so what
    the window had accumulated is not stepped on — the next step() starts a new window (and zero-fills); parameters and optimiser state
    are as the last completed window left them (BatchNorm statistics and the dropout word keep what the abandoned micro-steps did)."""

    def __init__(self, model, config: Optional[Config] = None, process_group=None,
                 use_graph: bool = False, bucket_mb: float = 32.0, always_reduce: bool = False, data_parallel: bool = True,
                 grad_comm_dtype: torch.dtype = torch.float32, native: bool = False, max_shapes: int = 1,
                 max_recorded_bytes: Optional[int] = None, accumulate: Optional[int] = None):
        """native=True: the launch sequence of the first step is recorded into a native step list (csrc/steplist.hip) and every
        later step re-issues it with one library call per segment — eager launches on the same streams (the weight-gradient side
        stream keeps overlapping, which a captured HIP graph loses) without the per-launch host cost of the Python loop.  Batch
        shapes are fixed by the first call, as with use_graph.  With layer_dropout (the x-transformers encoder) the list holds every
        encoder block as an op group; each step draws the skipped blocks on the host where an eager step draws them (model._xt_skips)
        and the replay leaves their launches out.

        max_shapes > 1 (native only): one recorded list per batch shape (shape_cache.shape_key of the prepared inputs for LRS, of the
        batch for LRW), each with its own static inputs and outputs; parameters, optimiser state, buffers, the dropout word and the
        scratch are shared.  A batch of a new shape is recorded (and executed) in its step; beyond `max_shapes` lists, or beyond
        `max_recorded_bytes` kept alive by their recorders, the least recently used list is released after a device synchronisation.

        accumulate=N (default: `train.accumulate_grad_batches` of the LRW config, `trainer.accumulate_grad_batches` of the LRS one, else 1):
        gradient accumulation over windows of N micro-steps (class docstring).  Eager and native; under native ONE recorded list per batch
        shape serves the first, middle and last micro-steps (the zero-fill and the optimiser tail are op groups a replay leaves out), and
        with max_shapes > 1 the micro-batches of a window may differ in shape."""
        if not isinstance(model, _StoreModule) or type(model)._loss_weights is _StoreModule._loss_weights:
            raise TypeError(f"TrainStep drives a model._StoreModule with a training step, one that states its _loss_weights "
                            f"(TransformerLightningModule, lrs_model.E2E), got {type(model).__name__}")
        self.model = model
        self.is_lrw = isinstance(model, TransformerLightningModule)
        if self.is_lrw:            # LRW/video/config/*.yaml: optim.optimizer / optim.scheduler / train.gradient_clip_val
            cfg = config or model.config
            opt = cfg.optim.optimizer
            sch = cfg.optim.get("scheduler", {}) or {}
            clip = cfg.train.get("gradient_clip_val", 0.0)
        else:                      # LRS/video/config/lrs3.yaml: optimizer / scheduler / trainer.gradient_clip_val
            cfg = config or lrs_train_config()
            opt = cfg.optimizer
            sch = cfg.get("scheduler", {}) or {}
            clip = (cfg.get("trainer", {}) or {}).get("gradient_clip_val", 0.0)
        accum = (cfg.get("train", {}) or {}).get("accumulate_grad_batches", 1) if self.is_lrw else (cfg.get("trainer", {}) or {}).get("accumulate_grad_batches", 1)
        accum = int(accumulate if accumulate is not None else (accum or 1))
        if accum < 1:
            raise ValueError("accumulate (accumulate_grad_batches) must be >= 1")
        if accum > 1 and use_graph:
            raise NotImplementedError("accumulate > 1 with use_graph=True: a captured HIP graph holds the whole step, optimiser included, and "
                                      "cannot leave the zero-fill or the optimiser out of a replay (use native=True or the eager step)")
        self.window = AccumWindow(accum)
        if accum > 1 or model._loss_scale != 1.0:
            model.set_loss_scale(1.0 / accum)          # the seeds of the backward: written in place, outside any recorded region
        schedule = ops.CosineSchedule(float(opt.lr), float(opt.betas[0]), int(sch.get("num_warmup_steps", 0) or 0), int(sch.get("num_training_steps", 0) or 0))
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # always_reduce: run the collective path even for a 1-rank group (exercises RCCL + graph capture on one GPU)
        # data_parallel=False: a purely local step even inside an initialised process group (no collective is ever issued — e.g. the
        # single-rank profiling leg of bench.py, which the other ranks do not take part in)
        self.dp = GradReducer(model, process_group, bucket_mb, always_reduce, grad_comm_dtype) if data_parallel and (self.world > 1 or always_reduce) else None
        if not data_parallel:
            model.grad_ready_hook = None
        model.accumulate_into_grads(False)
        self.use_graph = use_graph
        self.native = bool(native)
        if self.native and use_graph:
            raise ValueError("native=True and use_graph=True are two ways of replaying a step: pick one")
        if self.native and not self.is_lrw and model.length_norm:
            raise NotImplementedError("native=True: transformer_length_normalized_loss needs a torch kernel inside the step (use native=False)")
        if int(max_shapes) < 1:
            raise ValueError("max_shapes must be >= 1")
        if int(max_shapes) > 1 and not self.native:
            raise ValueError("max_shapes > 1 keeps one recorded step list per batch shape: it needs native=True")
        if max_recorded_bytes is not None and int(max_shapes) == 1:
            raise ValueError("max_recorded_bytes bounds the lists of max_shapes > 1")
        self.max_shapes = int(max_shapes)
        self._lists = ShapeLRU(self.max_shapes, max_recorded_bytes, weight=lambda e: e.nbytes)
        self._key: Optional[tuple] = None              # shape key of the list stepped last (max_shapes > 1)
        self._counts: dict = {}                        # shape key -> [times recorded, times replayed]
        self._rec: Optional[ops.StepRecorder] = None
        self._cover: tuple = (None, None)              # (data pointer of the gradient buffer, its ops.GradCoverage or None): _coverage
        self.fused_encoder_fallbacks = 0        # times _watch_fused_encoder switched the encoder to the launch chain
        self.host_ms: list[float] = []          # host time of the last steps' enqueue (bench.py reports the median)
        if use_graph and model.layer_drop_p > 0.0:
            raise NotImplementedError("layer_dropout skips whole encoder blocks at random: the launch sequence differs from step to "
                                      "step and cannot be replayed from one captured HIP graph (use use_graph=False)")
        # Weight-gradient launches only feed the flat gradient buffer, so in EAGER mode they run on a side stream next to the
        # data-gradient chain and fill its tails: LRW 8.06 -> 7.39 ms (trunk convs), LRS 31.9 -> 30.4 ms (trunk convs + the
        # 20-40 us linear GEMMs that fill about half the chip each).  Under HIP-graph replay the forked branches cost more than
        # they hide (LRW 7.85 -> 8.5 ms, LRS 33.2 ms), so a captured step keeps everything in line.
        model._side.enabled = not use_graph and _os.environ.get("SVSR_SIDE_TRUNK", "1") != "0"
        if not self.is_lrw:
            model._side.enabled_small = not use_graph and _os.environ.get("SVSR_SIDE_ENCODER", "1") != "0"
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._static: Optional[list[torch.Tensor]] = None
        self._out: Optional[dict[str, torch.Tensor]] = None
        # the optimiser (moments, hyper-parameters, schedule, device state); m, v, opt_state name its tensors for model._early_sumsq and checkpoints
        self.adamw = ops.AdamW(model.store(), schedule, float(opt.betas[1]), float(opt.eps), float(opt.weight_decay), float(clip or 0.0))
        self.m, self.v, self.opt_state = self.adamw.m, self.adamw.v, self.adamw.opt_state

    # -- one eager step -----------------------------------------------------------------------------
    def _step_impl(self, *batch):
        if self.window.n > 1:
            return self._micro_step_impl(*batch)
        model = self.model
        st = model.store()
        trace = _ROCTX                                   # SVSR_ROCTX=1: roctx ranges (rocprofv3 --marker-trace) around the phases
        if self.dp is not None:
            self.dp.begin_step()
        if trace:
            torch.cuda.nvtx.range_push("svsr.forward")
        self._zero_grads_early(st)
        out = model(*batch)
        if trace:
            torch.cuda.nvtx.range_pop()
            torch.cuda.nvtx.range_push("svsr.backward")
        (out["loss_total"] if self.is_lrw else out[0]).backward()
        if trace:
            torch.cuda.nvtx.range_pop()
            torch.cuda.nvtx.range_push("svsr.allreduce_join+optimizer")
        if self.dp is not None:
            self.dp.finish()
        self._optimizer(st)
        if trace:
            torch.cuda.nvtx.range_pop()
        if self.is_lrw:
            return {k: v.detach() for k, v in out.items()}
        return tuple(v.detach() for v in out)

    def _micro_step_impl(self, *batch):
        """_step_impl for accumulate > 1: one micro-step of the window (AccumWindow.plan).  The backward is seeded with the model's own
        device scalars (model.loss_seeds: 1/N folded into the loss weights) — the scalars the recorded step hands its backward."""
        model = self.model
        st = model.store()
        plan = self.window.plan()
        if self.dp is not None:
            self.dp.begin_step(sync=plan["reduce"])
        self._begin_micro_step(st, plan)
        out = model(*batch)
        losses = (out["loss_category"], out["loss_audio"]) if self.is_lrw else tuple(out[1:4])
        torch.autograd.backward(losses, model.loss_seeds(st.flat.device))
        model.accumulate_into_grads(False)
        if plan["optimise"]:
            if self.dp is not None:
                self.dp.finish()
            self._optimizer(st)
        if self.is_lrw:
            return {k: v.detach() for k, v in out.items()}
        return tuple(v.detach() for v in out)

    def _begin_micro_step(self, st, plan: dict) -> None:
        """_zero_grads_early for accumulate > 1.  The zero-fill: executed in the first micro-step of a window; inside a recording it is the
        list's "zero" op group whatever micro-step records (appended without being executed when this one is not the first).  The early
        sum of squares (model._early_sumsq) belongs to the optimiser tail: asked for in the last micro-step only — and in every recording,
        where it joins the "tail" group."""
        model = self.model
        rec = ops.active_recorder()
        self._forget_early_sumsq(st)
        model._early_sumsq = self.opt_state if self.dp is None and (plan["optimise"] or rec is not None) else None
        if plan["zero"] or rec is not None:
            with ops.window_group("zero"):
                model._side.run(lambda: ops.memset(st.grad, 0))
        if plan["zero"]:
            st.grad_clean = True
        model.accumulate_into_grads(not plan["zero"])

    def flush(self) -> bool:
        """Closes a partial window (the end of an epoch whose batch count is not a multiple of N: Lightning steps on the last batch): the
        optimiser tail — all-reduce under data parallelism, clip, AdamW, shadows, schedule — runs on what has been accumulated, which keeps
        its 1/N scale.  Nothing happens at a window boundary.  -> True when an optimiser step was made."""
        if not self.window.flush():
            return False
        model = self.model
        st = model.store()
        self._forget_early_sumsq(st)
        model.accumulate_into_grads(False)
        if self.dp is not None:
            self.dp.begin_step()
            self.dp.on_ready(0)
            self.dp.finish()
        self._optimizer(st)
        return True

    def _forget_early_sumsq(self, st) -> None:
        """Drops the early-sum-of-squares handshake with the model's backward (model._early_sumsq, st.sumsq_tail_done): it is valid only
        for the step that set it, and a step that aborted between its backward and its optimiser must not leave it behind."""
        self.model._early_sumsq = None
        st.sumsq_tail_done = False

    def _zero_grads_early(self, st) -> None:
        """The flat gradient buffer's zero-fill — the whole buffer, or with a first-touch map (_coverage) only the ranges no store-mode writer
        covers (LRW: 1.3 of 128 MB; the covered spans' first writers store) — is issued when the step BEGINS, on the side stream (behind the previous step's optimiser, which is the
        last reader; ahead of this step's weight gradients, the first writers there; the model joins the side stream before its encoder
        runs, long before the backward's main-stream writers): the fill (whole buffer: 128 MB LRW / 1 GB LRS) leaves the main stream, where it sat in front
        of the backward (17 / 140 us).  The backward's own zero_grad() then finds `grad_clean` set and does nothing."""
        model = self.model
        self._forget_early_sumsq(st)
        # no collective between the backward and the clip: the model may sum the squares of every gradient but the last while that one is
        # computed (set per step: two TrainSteps may drive one model, each with its own optimiser state)
        model._early_sumsq = self.opt_state if self.dp is None else None
        cov = self._coverage(st)
        if cov is None:
            model._side.run(lambda: ops.memset(st.grad, 0))
        else:
            # only what no store-mode writer covers is filled (one launch over the holes); the covered spans' first writers store
            model._side.run(cov.fill)
            cov.begin()
        st.grad_clean = True

    def _coverage(self, st) -> Optional["ops.GradCoverage"]:
        """The first-touch map of this model's gradient buffer (ops.GradCoverage), or None where the whole-buffer fill stays: models that declare
        no spans (model.grad_store_spans: the x-transformers encoder with its layer drop), ops.GRAD_STORE off (tests: the all-add reference).  Used by the steps of
        accumulate = 1 only: a window's micro-steps share one recorded list, whose frozen modes cannot tell the first micro-step from the rest."""
        if not ops.GRAD_STORE:
            return None
        key, cov = self._cover
        if key != st.grad.data_ptr():
            spans = self.model.grad_store_spans(st.offsets, st.phys)
            cov = ops.GradCoverage(st.grad, spans) if spans else None
            self._cover = (st.grad.data_ptr(), cov)
        return cov

    def _optimizer(self, st) -> None:
        """Global-norm clip + AdamW + bf16 shadows.  With the model's side stream in use the update is SPLIT: the visual front-end's weights
        (and every 1-D tensor: BatchNorm / LayerNorm parameters, biases), which the next forward needs first, on the main stream; everything
        behind the front-end (two thirds of the word-level model, 95 % of the sentence-level one) on the side stream, where this
        HBM-bound pass runs beside the next step's stem / trunk forward.  The model joins the side stream before its encoder runs and
        before state_dict(); the step counter advances behind the last range."""
        model, adamw = self.model, self.adamw
        early_done = st.sumsq_tail_done  # the backward already summed the squares of everything behind the stem weight
        self._forget_early_sumsq(st)     # (a backward outside a step must not write this optimiser's state)
        stale = ops.end_grad_coverage()
        if stale:
            raise RuntimeError(f"{len(stale)} gradient ranges planned as first-touch stores had no writer in this step (first: elements "
                               f"[{stale[0][0]}, {stale[0][1]})): their content is the previous step's — model.grad_store_spans is out of step "
                               f"with the backward")
        if st.sumsq_head:
            # two ranges, always the same two (one association whatever ran early): [head, n) -> partial sums 0..1022 — already summed on the
            # side stream beside the stem's weight gradient when the model could (model._early_sumsq) — and the stem weight -> partial 1023
            if not early_done:
                adamw.sumsq(st, st.sumsq_head, st.numel - st.sumsq_head, 0, ops.SUMSQ_PARTS - 1)
            adamw.sumsq(st, 0, st.sumsq_head, ops.SUMSQ_PARTS - 1, 1)
        else:
            adamw.sumsq(st)
        side = model._side
        if not (side.enabled and st.front_end < st.decay_end):
            adamw.apply(st)
            ops.transpose_shadows(st.flat, st.w16, st.w16t, st.table, st.n_entries)
        else:
            adamw.apply(st, 0, st.front_end, advance=False)
            adamw.apply(st, st.decay_end, st.numel, advance=False)
            nf = st.n_entries_front
            side.run(lambda: (adamw.apply(st, st.front_end, st.decay_end, advance=True),
                              ops.transpose_shadows_range(st.w16, st.w16t, st.table, nf, st.n_entries - nf)))
            ops.transpose_shadows_range(st.w16, st.w16t, st.table, 0, nf)
        st.shadow_fresh = True
        st.generation += 1

    def synchronize(self) -> None:
        """Joins whatever the last step left on the model's side stream (the tail of its optimiser step)."""
        self.model._side.join()

    # -- native step list ----------------------------------------------------------------------------
    def _direct_impl(self, *batch):
        """_step_impl without autograd or torch kernels: every device operation is a library call (recordable)."""
        model = self.model
        st = model.store()
        if self.window.n > 1:
            # one list for every kind of micro-step: the zero-fill and the optimiser tail are op groups (the reducer's callbacks, between
            # segments, do nothing unless the micro-step reduces: GradReducer.begin_step(sync))
            self._begin_micro_step(st, self.window.plan())
            out = model.train_step_direct(*batch)
            model.accumulate_into_grads(False)
            if self.dp is not None:
                ops.host_callback(self.dp.finish)
            with ops.window_group("tail"):
                self._optimizer(st)
            return out
        self._zero_grads_early(st)
        out = model.train_step_direct(*batch)
        if self.dp is not None:
            ops.host_callback(self.dp.finish)
        self._optimizer(st)
        return out

    def _record(self, static: Optional[list], prepped) -> tuple:
        """Records (and executes) one step on the static inputs `static` (made from `prepped` when None, else `prepped` is copied into them:
        the input buffers a loader may be writing into stay the same).  -> (static, recorder, outputs)."""
        model = self.model
        if not model.training:
            raise RuntimeError("TrainStep(native=True) records a TRAINING step: call model.train() first")
        if static is None:
            static = [t.clone() if torch.is_tensor(t) else t for t in prepped]
        else:
            for dst, src in zip(static, prepped):
                if torch.is_tensor(dst) and dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
        st = model.store()
        if not st.shadow_fresh:
            st.refresh_shadows()
            st.shadow_fresh = True
        plan = self.window.plan()
        if self.dp is not None:
            self.dp.begin_step(sync=plan["reduce"])
        if model._side.stream is None:
            model._side.stream = torch.cuda.Stream()
        model.direct_constants(static[0].device)
        if model._drop_word is None and (model.drop_p > 0.0 or model.attn_drop_p > 0.0 or model.emb_drop_p > 0.0 or model._codec_samples()):
            model._advance_dropout(static[0].device)      # creates the seed word outside the recorded region ...
            ops.word_add(model._drop_word, -1)             # ... and leaves its value where the first forward expects it
        rec = ops.StepRecorder()
        if self._layer_drop():
            rec.layer_groups = True
            rec.skips = frozenset(_xt_skips(model))       # this step's draw: recorded append-only, see StepRecorder.group
        if self.window.n > 1:
            # the window groups sit behind the layer-drop groups; the micro-step that records leaves out what its kind leaves out
            base = 2 * model.layers if rec.layer_groups else 0
            rec.window = (base, base + 1)
            rec.skips = rec.skips | frozenset(rec.window_skips(plan["zero"], plan["optimise"]))
        with ops.recording(rec):
            out = self._direct_impl(*static)
        out = {k: v.detach() for k, v in out.items()} if isinstance(out, dict) else tuple(v.detach() for v in out)
        return static, rec, out

    def _layer_drop(self) -> bool:
        """Layer drop is on: the recorded lists hold every encoder block as an op group (model._xt_encoder_forward / _backward)."""
        return self.is_lrw and self.model.layer_drop_p > 0.0

    def _count(self, key, i: int) -> None:
        self._counts.setdefault(key, [0, 0])[i] += 1

    def _native_step(self, *batch):
        if self.max_shapes > 1:
            return self._native_step_keyed(*batch)
        model = self.model
        if self._rec is None:
            self._static, self._rec, self._out = self._record(self._static, model.prepare_batch(*batch))
            self._main_stream = self._rec.main_stream
            self._count(None, 0)
            return self._out
        if not self.is_lrw:          # LRS: the conversions (and the decoder / CTC targets) are redone per batch, then copied into the static inputs
            batch = model.prepare_batch(*batch)
        self._replay(batch)
        self._count(None, 1)
        return self._out

    def _native_step_keyed(self, *batch):
        """max_shapes > 1: the list of this batch's shape key is replayed, or recorded when there is none (evicting the least recently used
        lists beyond max_shapes / max_recorded_bytes first).  _rec / _static / _out / input_buffers() follow the list stepped last."""
        model = self.model
        lists = self._lists
        last = lists.peek(self._key) if self._key is not None else None
        if last is not None and last.rec is not None and self._rec is None:
            self._release([last], keep_static=True)         # `_rec = None`: the shape stepped last is recorded again
        src = tuple(batch) if self.is_lrw else model.prepare_batch(*batch)
        key = shape_key(src)
        e = lists.get(key)
        if e is None or e.rec is None:
            if e is None:
                e = _ShapeList()
                self._release([v for _, v in lists.put(key, e)])
            prepped = model.prepare_batch(*batch) if self.is_lrw else src
            e.static, e.rec, e.out = self._record(e.static, prepped)
            e.nbytes = e.rec.kept_bytes()
            self._bind(key, e)
            self._count(key, 0)
            self._release([v for _, v in lists.shrink(keep=key)])
            return e.out
        self._bind(key, e)
        self._replay(src)
        self._count(key, 1)
        return e.out

    def _bind(self, key, e: "_ShapeList") -> None:
        self._key = key
        self._rec, self._static, self._out, self._main_stream = e.rec, e.static, e.out, e.rec.main_stream

    def _release(self, entries: list, keep_static: bool = False) -> None:
        """Drops the recorders (and, unless keep_static, the static inputs) of `entries`.  Their tensors go back to torch's caching allocator,
        which hands them to the next allocation on the main stream: the device must be done with them on EVERY stream first — the tail of
        the last step's optimiser may still run on the model's side stream after step() returned — hence one device synchronisation (rare:
        a new shape beyond the bounds, a re-recording)."""
        live = [e for e in entries if e.rec is not None or (not keep_static and e.static is not None)]
        if not live:
            return
        torch.cuda.synchronize()
        for e in live:
            if e.rec is self._rec:
                self._rec = None
            e.rec, e.out, e.nbytes = None, None, 0
            if not keep_static:
                e.static = None

    def recorded_shapes(self) -> dict:
        """Per shape key of a list held now: {launches, bytes (device memory its recorder keeps alive: unique storages), recorded (times),
        replayed (times)}.  max_shapes = 1: the one list, keyed by its static inputs.  Read-only."""
        out = {}
        if self.max_shapes == 1:
            if self._rec is not None:
                n = self._counts.get(None, [0, 0])
                out[shape_key(self._static)] = dict(launches=self._rec.size, bytes=self._rec.kept_bytes(), recorded=n[0], replayed=n[1])
            return out
        for key, e in self._lists.items():
            if e.rec is None:
                continue
            n = self._counts.get(key, [0, 0])
            out[key] = dict(launches=e.rec.size, bytes=e.nbytes, recorded=n[0], replayed=n[1])
        return out

    def _replay(self, batch) -> None:
        model = self.model
        for dst, src in zip(self._static, batch):
            if not torch.is_tensor(dst):
                continue
            if dst.shape[0] != src.shape[0] or dst.shape[2:] != src.shape[2:] or (not self.is_lrw and dst.shape != src.shape):
                raise ValueError("a recorded TrainStep needs fixed batch shapes (pad to the recorded size or use native=False)")
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src if src.dim() != 2 or src.shape[1] == dst.shape[1] else src[:, : dst.shape[1]], non_blocking=True)
        if ops._stream() != self._main_stream:
            raise RuntimeError("a recorded TrainStep must be replayed on the stream it was recorded on")
        if self._rec.window is not None:
            plan = self.window.plan()
            if self.dp is not None:
                self.dp.begin_step(sync=plan["reduce"])
            skips = _xt_skips(model) if self._rec.layer_groups else set()
            self._rec.set_skips(skips | self._rec.window_skips(plan["zero"], plan["optimise"]))
            self._rec.run()
            if plan["optimise"]:
                model._store.generation += 1
            return
        if self.dp is not None:
            self.dp.begin_step()
        if self._rec.layer_groups:
            self._rec.set_skips(_xt_skips(model))       # once per step, as the eager forward draws it
        self._rec.run()
        model._store.generation += 1

    def input_buffers(self) -> Optional[tuple]:
        """The device tensors a recorded (native / captured) step reads its batch from, in the order of step()'s arguments — None
        before the first step, for an eager TrainStep, and in the slots whose content step() derives per batch (LRS: lengths, labels).
        A loader that writes the next batch INTO these (its host-to-device copy lands where the step reads) and passes them back to
        step() saves the device-to-device copy of the clip (LRW B = 32: 29 MB, 111 us; LRS 16 x 160 frames: 79 MB, ~300 us):
        step() skips every argument that already is its static buffer."""
        if self._static is None:
            return None
        if self.is_lrw or self.use_graph:
            return tuple(self._static)
        return (self._static[0], None, self._static[2], None)

    def step(self, *batch):
        """One optimisation step; returns the model's outputs (LRW: the dict of five scalars; LRS: the 5-tuple).
        With use_graph / native the batch shapes are fixed by the first call (later batches are copied into the static buffers).
        With accumulate = N > 1 this is one micro-step of a window (class docstring); the optimiser runs in every N-th call."""
        self._watch_fused_encoder()
        if self.is_lrw:
            # float waveforms (vq codec attached): the tokeniser draws nothing, so it runs as eager launches in FRONT of the recorded /
            # replayed / captured step, which sees tokens as it always did; its device forms thereby exist before a step is recorded
            batch = (batch[0], self.model._tokenize_waveforms(batch[1], batch[0].size(2) * self.model.audio_alignment), *batch[2:])
        try:
            out = self._step(*batch)
        except BaseException:
            # an aborted step must not leave its early-sum-of-squares handshake pointing at this optimiser's state (a later stand-alone
            # backward would write partial sums into it and the next optimiser step would trust them)
            self._forget_early_sumsq(self.model.store())
            ops.end_grad_coverage()      # (and the next backward outside a step adds, as it always did)
            if self.window.n > 1:          # the window is abandoned (class docstring): the next step() starts a new one and zero-fills
                self.window.abort()
                self.model.accumulate_into_grads(False)
            raise
        self.window.advance()
        return out

    def _watch_fused_encoder(self) -> None:
        """Automatic fall-back of the fused encoder (csrc/enc_fused.hip).  Its launches need the 8 workgroups of a sequence resident together;
        when a bounded cluster wait gives up (a co-tenant kernel holding LDS or compute units — e.g. a peer-waiting collective kernel), the
        launch poisons its output with NaN and sets a flag that is also stored into pinned host memory.  The poisoned step updates nothing
        (svsr_adamw_step skips a step whose gradient norm is not finite); here, before the next step is enqueued, the flag is read WITHOUT a
        synchronisation and the encoder is re-routed to the per-layer launch chain for the rest of the run: the recorded list / captured
        graph is dropped and re-made on that path.  At most the steps already enqueued when the wait gave up are lost (skipped)."""
        if not self.is_lrw or not ops.enc_gave_up_peek():
            return
        torch.cuda.synchronize()
        ops.check_enc_clusters(reset=True)
        ops.disable_enc_fused("a cluster wait of svsr_enc_fwd / svsr_enc_bwd gave up (its workgroups were not resident together)")
        self.fused_encoder_fallbacks += 1
        self._release([e for _, e in self._lists.items()], keep_static=True)      # max_shapes > 1: every list is recorded again
        self._rec = None                 # native: record the step again (now on the chain)
        self._graph = None               # graph: capture again

    def _step(self, *batch):
        if self.native:
            import time as _time

            t0 = _time.perf_counter()
            out = self._native_step(*batch)
            self.host_ms.append((_time.perf_counter() - t0) * 1e3)
            if len(self.host_ms) > 256:
                del self.host_ms[:128]
            return out
        if not self.use_graph:
            import time as _time

            t0 = _time.perf_counter()
            out = self._step_impl(*batch)
            self.host_ms.append((_time.perf_counter() - t0) * 1e3)
            if len(self.host_ms) > 256:
                del self.host_ms[:128]
            return out
        if self._graph is None:
            self._capture(*batch)
        else:
            for dst, src in zip(self._static, batch):
                if dst.shape != src.shape:
                    raise ValueError("a captured TrainStep needs fixed batch shapes (pad to the captured size or use use_graph=False)")
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src, non_blocking=True)
        self._graph.replay()
        self.model._store.generation += 1
        return self._out

    def _capture(self, *batch) -> None:
        ops.PLAN_CACHE_PINNED = True       # the captured launches reference the plans' device words
        if self._static is None:
            self._static = [t.clone() for t in batch]
        else:                            # captured again (_watch_fused_encoder): same input buffers
            for dst, src in zip(self._static, batch):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
        # warm-up on a side stream (allocator pools, hipFuncSetAttribute, lazy module loads), state restored afterwards
        st = self.model.store()
        snap = (st.flat.clone(), self.m.clone(), self.v.clone(), self.opt_state.clone(),
                {k: b.clone() for k, b in st.buffers.items()})
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._step_impl(*self._static)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        st.flat.copy_(snap[0]); self.m.copy_(snap[1]); self.v.copy_(snap[2]); self.opt_state.copy_(snap[3])
        for k, b in st.buffers.items():
            b.copy_(snap[4][k])
        st.refresh_shadows()          # shadows follow the restored weights; inside the graph the optimiser keeps them fresh
        st.shadow_fresh = True
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        # thread-local capture mode: with a process group alive, the collective backend's watchdog thread polls HIP events at any
        # moment, which the default (global) mode turns into "operation not permitted when stream is capturing" and an abort
        with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
            self._out = self._step_impl(*self._static)

    # -- checkpoint / resume -------------------------------------------------------------------------
    def state_dict(self) -> dict[str, torch.Tensor]:
        """Optimiser state for checkpointing (what Lightning stores next to the model's state_dict): AdamW moments as flat
        fp32 vectors in the parameter store's order, and the 16-byte device state {step, -, lr, grad-norm}."""
        self.synchronize()
        sd = {**self.adamw.moments(),
              # what the order of the additions inside a weight gradient / a BatchNorm statistic depends on (ops.REDUCTION_KNOBS; the
              # compute-unit count the splits are planned for is one of them and is a fixed 256, not the device's): a resumed run is
              # bit-identical when these agree
              "reduction_plan": torch.tensor(ops.reduction_plan_params(), dtype=torch.int64)}
        rs = self.model.rng_state()                 # dropout seed word + layer-drop generator: a resumed run draws the same masks / skips
        sd["dropout_word"] = torch.tensor([rs["dropout_word"]], dtype=torch.int64)
        if "layer_rng" in rs:
            sd["layer_rng"] = _rng_state_to_tensor(rs["layer_rng"])
        # saved inside a window: its position and the gradient accumulated so far, so that a resumed run finishes the window (at a window
        # boundary neither key is written)
        win = self.window.state_dict()
        if win:
            sd.update(win)
            sd["accum_grad"] = self.model.store().grad.detach().clone()
        return sd

    def load_state_dict(self, sd: dict[str, torch.Tensor]) -> None:
        self.synchronize()
        self.adamw.load_moments(sd)
        self.opt_state[:4].copy_(sd["opt_state"][:4])
        if "reduction_plan" in sd:
            then, now = [int(x) for x in sd["reduction_plan"].tolist()], ops.reduction_plan_params()
            if then != now:
                diff = {k: (a, b) for k, a, b in zip(ops.REDUCTION_KNOBS, then, now) if a != b}
                warnings.warn(f"this checkpoint was written with other reduction-split knobs {diff} (then, now): the resumed run is numerically "
                              f"equivalent but not bit-identical to the original (ops.tune(key, value) restores them)")
        self.window.load_state_dict(sd)
        if self.window.pos:
            st = self.model.store()
            if "accum_grad" not in sd or sd["accum_grad"].numel() != st.grad.numel():
                self.window.abort()
                raise ValueError("a checkpoint saved inside a window carries the accumulated gradient (accum_grad) of this parameter layout")
            st.grad.copy_(sd["accum_grad"])
        self.opt_state[1] = 0                    # (word 1 counts the skipped steps of THIS run; older checkpoints kept a float there)
        if "dropout_word" in sd:            # (checkpoints of LRS runs written before E2E had an rng_state carry none)
            rs = {"dropout_word": int(sd["dropout_word"].reshape(-1)[0])}
            if "layer_rng" in sd:
                try:
                    rs["layer_rng"] = _rng_state_from_tensor(sd["layer_rng"])
                except ValueError as e:       # checkpoints written before the int64[628] format (pickled uint8 payload): nothing here unpickles
                    warnings.warn(f"{e}; the layer-drop generator is NOT restored (it continues from this process's seed), everything else is")
            self.model.load_rng_state(rs)

    # -- introspection ------------------------------------------------------------------------------
    def state(self) -> dict[str, float]:
        """{step, lr, grad_norm, skipped_steps} of the last optimiser step (a host synchronisation) and micro_step, the position of the
        NEXT step() inside its accumulation window (0: at a window boundary; always 0 with accumulate = 1).  skipped_steps counts steps whose gradient
        norm was not finite: they updated nothing and did not advance `step` (svsr_adamw_step).  A fused-encoder launch whose cluster wait
        gave up (csrc/enc_fused.hip) produces such a step; it is picked up here as well as before every step (_watch_fused_encoder): the
        encoder continues on the per-layer launch chain, with a warning."""
        self.synchronize()
        w = self.adamw.state()
        if self.is_lrw and ops.check_enc_clusters(reset=False):
            self._watch_fused_encoder()
        if not self.is_lrw:
            self.model.check_targets()          # a label outside [1, odim) reached svsr_lrs_targets: raises with the cause
        return {"step": w["step"], "lr": w["lr"], "grad_norm": w["gnorm"], "skipped_steps": w["skipped"], "micro_step": self.window.pos}


def reduce_metrics(metrics, process_group=None):
    """`self.log(..., sync_dist=True)` of the reference (LRW/video/src/lightning.py:208,214; LRS/video/lightning.py:143-216): the
    logged scalars are averaged over the ranks.  `metrics` is the dict (LRW) or tuple (LRS) of 0-d tensors a step returns; they are
    packed into one vector so a step's logging costs ONE collective.  With no process group (or one rank) the input is returned."""
    if not dist.is_initialized() or dist.get_world_size(process_group) == 1:
        return metrics
    keys = list(metrics.keys()) if isinstance(metrics, dict) else list(range(len(metrics)))
    vec = torch.stack([metrics[k].detach().float().reshape(()) for k in keys])
    if dist.get_backend(process_group) == "nccl":
        dist.all_reduce(vec, op=dist.ReduceOp.AVG, group=process_group)
    else:
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=process_group)
        vec = vec / dist.get_world_size(process_group)
    out = {k: vec[i] for i, k in enumerate(keys)}
    return out if isinstance(metrics, dict) else tuple(out[k] for k in keys)


class GradReducer:
    """Bucketed gradient all-reduce over the flat gradient buffer, overlapped with the backward pass.

    The flat buffer is [decayed tensors in forward order | 1-D tensors].  The backward calls `on_ready(lo)` meaning
    "decayed offsets >= lo are final"; whole buckets are peeled off the top of the decayed region as soon as they are
    complete and reduced on a side stream.  `on_ready(0)` (end of backward) flushes the rest plus the 1-D tail.
    """

    def __init__(self, model, process_group=None, bucket_mb: float = 32.0, always: bool = False, comm_dtype: torch.dtype = torch.float32):
        self.model = model
        # comm_dtype=torch.bfloat16: buckets cross the links as bf16 (half the bytes) and come back into the fp32 gradient
        # buffer — an opt-in deviation from DDP's fp32 all-reduce, for when the step is short enough for the collective to show
        if comm_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("comm_dtype must be torch.float32 or torch.bfloat16")
        self.comm_dtype = comm_dtype
        self._comm_buf: Optional[torch.Tensor] = None
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.always = always and dist.is_initialized()
        self.bucket_elems = max(1, int(bucket_mb * (1 << 20) / 4))
        # the bucket at the bottom of the buffer (stem, layer1: final only when the backward ends) is the one collective nothing can
        # hide: bucket edges are anchored so that it holds at most 4 MB, whatever is left over goes to the FIRST bucket (top of the
        # buffer, ready earliest)
        self.last_elems = min(self.bucket_elems, 1 << 20)
        self._st = None
        self.measure = False                  # bench.py: time the join in finish() with HIP events (the collective time the step is exposed to)
        self._join_events: list = []
        self._bucket_events: list = []        # measure=True: per step a list of (elements, ready event, done event), one per bucket in launch order
        self._backend = dist.get_backend(process_group) if dist.is_initialized() else None
        self.comm_stream: Optional[torch.cuda.Stream] = None
        self.top = 0
        self.launched: list[tuple[int, int]] = []
        self._fenced_at = -1                  # ops.enqueue_seq() at the comm stream's last fence of this step
        self.sync = True                      # begin_step(sync=False): the reducer sits out a micro-step
        self.collectives = 0                  # gradient all-reduces issued so far (tests count them per micro-step)
        model.grad_ready_hook = self.on_ready
        # DDP construction semantics (torch DistributedDataParallel behind Lightning's strategy="ddp", reference
        # LRW/video/src/train.py:28): every rank starts from rank 0's parameters AND buffers, whatever its own seed or a
        # per-rank load_state_dict left behind.
        if dist.is_initialized() and (self.world > 1 or self.always):
            st = model.store()
            if st.flat.is_cuda and dist.get_backend(process_group) == "nccl":
                pg = process_group if process_group is not None else dist.distributed_c10d._get_default_group()
                if getattr(pg, "bound_device_id", None) is None:
                    # measured on one MI355X with a 1-rank group: init_process_group("nccl", ..., device_id=dev) 6.18 ms per LRW step,
                    # the lazily initialised communicator (no device_id) 14.3 ms — with or without a collective inside the step
                    warnings.warn("the RCCL process group is not bound to a device: pass device_id=torch.device('cuda', local_rank) to "
                                  "init_process_group (a lazily initialised communicator measured 2.3x slower training steps)")
            dist.broadcast(st.flat, src=dist.get_global_rank(process_group, 0) if process_group is not None else 0, group=process_group)
            self._broadcast_buffers(st)
            for b in st.buffers.values():
                if not b.is_floating_point():
                    dist.broadcast(b, src=dist.get_global_rank(process_group, 0) if process_group is not None else 0, group=process_group)
            st.shadow_fresh = False          # the bf16 shadows follow the broadcast weights at the next forward

    def exposed_ms(self) -> Optional[float]:
        """Median time the main stream sat at the join of finish() (measure=True): what the step pays for collectives the backward
        did not hide.  Synchronises the device."""
        if not self._join_events:
            return None
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) for a, b in self._join_events)
        self._join_events.clear()
        return t[len(t) // 2]

    def bucket_times(self) -> list:
        """measure=True: per bucket of a step (launch order) {mb, ready_ms: start of its all-reduce after the first bucket's start, ms: ready -> done
        on the comm stream}, medians over the measured steps.  Synchronises the device."""
        steps = [s for s in self._bucket_events if s]
        if not steps:
            return []
        torch.cuda.synchronize()
        n = min(len(s) for s in steps)
        out = []
        for i in range(n):
            ready = sorted(s[0][1].elapsed_time(s[i][1]) for s in steps)
            dur = sorted(s[i][1].elapsed_time(s[i][2]) for s in steps)
            out.append({"mb": round(steps[0][i][0] * 4 / 2 ** 20, 2), "ready_ms": round(ready[len(ready) // 2], 4), "ms": round(dur[len(dur) // 2], 4)})
        self._bucket_events.clear()
        return out

    def _broadcast_buffers(self, st) -> None:
        """broadcast_buffers=True of DDP: the BatchNorm running statistics of every rank follow rank 0's — one collective over
        the flat buffer vector (model._ParamStore.bufflat).  num_batches_tracked advances identically on every rank."""
        if st.bufflat.numel():
            src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
            dist.broadcast(st.bufflat, src=src, group=self.group)

    def begin_step(self, sync: bool = True) -> None:
        """sync=False (a micro-step of an accumulation window that is not its last; DDP's no_sync): this call, and on_ready / finish until
        the next begin_step, do nothing — no collective is issued, gradient or buffer (torch's DistributedDataParallel with
        broadcast_buffers=True re-broadcasts the buffers only before a forward that FOLLOWS a synchronising one, i.e. before the first
        micro-step of a window: here that is the broadcast in the finish() of the last micro-step).  bucket_times() / exposed_ms()
        therefore describe the last micro-step."""
        self.sync = bool(sync)
        if not self.sync:
            return
        st = self._st = self.model.store()         # (store() re-validates ~300 tensors: once per step, not once per hook call)
        self.top = st.decay_end
        self.launched = []
        self._fenced_at = -1
        if self.measure:
            self._bucket_events.append([])
            if len(self._bucket_events) > 64:
                del self._bucket_events[:32]
        if self.comm_stream is None and st.flat.is_cuda:
            self.comm_stream = torch.cuda.Stream(device=st.flat.device)

    def _reduce(self, lo: int, hi: int, fence: bool = True) -> None:
        """fence=False: the comm stream already waits for this segment's producers (an earlier bucket of the same on_ready call)."""
        if hi <= lo:
            return
        self.launched.append((lo, hi))
        st = self._st if self._st is not None else self.model.store()
        seg = st.grad[lo:hi]
        if self.world == 1 and not self.always:
            return
        self.collectives += 1
        backend = self._backend
        if seg.is_cuda:
            # (nothing enqueued since the last fence — gradient-ready notifications that follow each other directly, as behind the encoder's one
            # grouped weight-gradient launch: the comm stream already waits for these producers.  Inside a HIP graph capture a second
            # event record / wait pair behind the same node gave a graph whose replay ran out of order)
            if fence and ops.enqueue_seq() != self._fenced_at:
                self.comm_stream.wait_stream(torch.cuda.current_stream())     # the segment's producers are enqueued there ...
                side = self.model._side
                if side.stream is not None and (side.enabled or side.enabled_small):
                    self.comm_stream.wait_stream(side.stream)                 # ... and, for weight gradients, on the model's side stream
                self._fenced_at = ops.enqueue_seq()
            with torch.cuda.stream(self.comm_stream):
                if self.measure and self._bucket_events:
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()              # on the comm stream, behind its waits: the bucket's producers are done
                if self.comm_dtype == torch.bfloat16:
                    if self._comm_buf is None or self._comm_buf.numel() < seg.numel():      # on the comm stream, used only there
                        self._comm_buf = torch.empty(max(seg.numel(), self.bucket_elems), dtype=torch.bfloat16, device=seg.device)
                    wire = self._comm_buf[: seg.numel()]
                    wire.copy_(seg)
                else:
                    wire = seg
                if backend == "nccl":
                    dist.all_reduce(wire, op=dist.ReduceOp.AVG, group=self.group)
                else:
                    dist.all_reduce(wire, op=dist.ReduceOp.SUM, group=self.group)
                    wire.div_(self.world)
                if wire is not seg:
                    seg.copy_(wire)
                if self.measure and self._bucket_events:
                    ev1.record()
                    self._bucket_events[-1].append((hi - lo, ev0, ev1))
        else:
            dist.all_reduce(seg, op=dist.ReduceOp.SUM, group=self.group)
            seg.div_(self.world)

    def on_ready(self, lo: int) -> None:
        if not self.sync:
            return
        st = self._st if self._st is not None else self.model.store()
        # one fence per call: every bucket launched here waits for the same producers (all enqueued by now), the later ones follow
        # the first in comm-stream order
        if lo == 0:
            self._reduce(0, self.top)
            fenced = self.top > 0
            self.top = 0
            self._reduce(st.decay_end, st.numel, fence=not fenced)
            return
        fence = True
        while self.top > self.last_elems:
            edge = self.last_elems + (self.top - 1 - self.last_elems) // self.bucket_elems * self.bucket_elems     # lower edge of the top bucket
            if edge < lo:
                break
            self._reduce(edge, self.top, fence)
            self.top, fence = edge, False

    def finish(self) -> None:
        """Joins the bucket all-reduces.  DDP re-broadcasts the buffers before every forward; here rank 0's BatchNorm running
        statistics (a few KB in one flat vector) follow the buckets on the comm stream and the ONE join below covers both, so
        nothing is left un-joined when the step ends: a captured HIP graph has no dangling branch, and an eval forward or a
        state_dict() read right after the step sees the broadcast values."""
        if not self.sync:
            return
        if (self.world > 1 or self.always) and self.comm_stream is not None:
            st = self._st if self._st is not None else self.model.store()
            self.comm_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.comm_stream):
                self._broadcast_buffers(st)
            if self.measure:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            torch.cuda.current_stream().wait_stream(self.comm_stream)
            if self.measure:
                e1.record()
                self._join_events.append((e0, e1))
        elif self.world > 1 or self.always:
            self._broadcast_buffers(self._st if self._st is not None else self.model.store())
