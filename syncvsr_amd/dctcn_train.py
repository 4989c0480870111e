"""The reference's DC-TCN training step (``LRW/video/src/lightning.py:314-334``: ``training_step`` + ``configure_optimizers``), eager:

    step = DCTCNTrainStep(model, total_steps)            # model: dctcn.DCTCNLightningModule on the device, in eval mode
    metrics = step.step(batch)                           # batch: the keyword arguments of the module's forward

One call is mixup's lam draw -> (the device input pipeline) -> ``model.loss_and_grads`` (the whole model in the reference's training
arithmetic, every gradient hand-written) -> the global-norm clip's sum of squares (``train.gradient_clip_val``, Lightning's
``gradient_clip_val``) -> ONE AdamW launch over the store's flat buffers under ``OneCycleLR`` (``svsr_adamw_onecycle_step``: the learning
rate and beta1 of the step come from the device step counter; the bf16 shadows are written in the same pass).  Nothing is read back: the
five metrics come out as device tensors.

The optimiser is timm's ``create_optimizer_v2(opt="adamw", betas, eps, weight_decay)``: decoupled weight decay on every parameter but those
with ``ndim <= 1`` or a name ending in ``.bias`` — the decayed region [0, decay_end) of the flat store.  ``OneCycleLR(**optim.scheduler,
total_steps=...)`` keeps torch's defaults for what the configuration leaves out (``div_factor`` 25, ``final_div_factor`` 1e4,
``cycle_momentum`` with ``base_momentum`` 0.85 and ``max_momentum`` 0.95, which replace beta1).

``steps`` is a HOST mirror of the device step counter (it raises past ``total_steps`` without a read-back) and ``micro_steps`` counts the
calls of ``step()`` (it picks the dropout seed).  The device does not count a step whose gradient norm is not finite (nothing is written:
``state()["skipped"]``), so after such a step the mirror runs ahead by one: the dropout seeds shift and the host refuses the last step of
the schedule.  ``resync()`` reads the device counter back into the mirror (one synchronisation; ``load_state_dict`` does it).

DATA PARALLEL (Lightning ``strategy="ddp"`` = torch ``DistributedDataParallel``; the shipped ``dc-tcn-base.yaml`` trains on four GPUs).
Inside an initialised ``torch.distributed`` process group of more than one rank (or with ``always_reduce``) the step attaches an
``engine.GradReducer``: at construction every rank takes rank 0's parameters and buffers; a step is ``begin_step`` ->
``loss_and_grads`` (whose backward notifies the reducer: the back-end's buckets cross the links under the front-end's backward, the
front-end's as the trunk walks down, the 1-D tail last) -> ``finish`` -> clip and AdamW on the AVERAGED gradient.  BatchNorm statistics are
per rank (no SyncBatchNorm, as in the reference) and the running statistics follow rank 0 after every synchronising step.  A rank's
dropout seeds are its own (``dropout_seed``), lam is a per-call argument or a draw from this process's ``np.random``.  ``last_reduce``
describes the last synchronising step's buckets.  With the defaults and no process group no collective is ever issued.

GRADIENT ACCUMULATION (``accumulate=N``; Lightning's ``accumulate_grad_batches``): the semantics of ``engine.TrainStep``'s class docstring.
N consecutive ``step()`` calls form a window; every micro-step's loss enters its backward times 1/N, the first one stores its gradients
and the others add; only the last one synchronises (DDP's ``no_sync`` before it), clips, runs AdamW, counts a step and marks the
prepared weight copies stale.  Running statistics and the dropout seed advance in every micro-step; ``step()`` returns the unscaled
metrics of its micro-batch; ``total_steps`` counts optimiser steps; ``flush()`` closes a partial window; an exception inside a
micro-step abandons the window.

NOT built here (engine.TrainStep has them for the transformer models): native step lists and HIP-graph capture."""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from . import ops
from .dctcn import DCTCNLightningModule

METRICS = ("loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5")


def dropout_seed(seed: int, rank: int, total_steps: int, accumulate: int, micro_index: int) -> int:
    """The dropout seed of micro-step `micro_index` (0-based, counted per rank) on `rank`: every rank owns the total_steps * accumulate
    seeds behind seed + rank * total_steps * accumulate, so no two (rank, micro-step) pairs of a run share one.  Rank 0 with
    accumulate = 1: seed + the step's index."""
    return int(seed) + int(rank) * int(total_steps) * int(accumulate) + int(micro_index)


class DCTCNTrainStep:
    def __init__(self, model: DCTCNLightningModule, total_steps: int, pipeline=None, seed: int = 0, *, process_group=None,
                 data_parallel: bool = True, always_reduce: bool = False, bucket_mb: float = 32.0,
                 grad_comm_dtype: torch.dtype = torch.float32, accumulate: Optional[int] = None):
        """process_group / data_parallel / always_reduce / bucket_mb / grad_comm_dtype: engine.TrainStep's (an engine.GradReducer is attached
        when data_parallel and the group has more than one rank, or always_reduce is set; data_parallel=False: a purely local step even
        inside an initialised group).  accumulate=N: windows of N micro-steps; None: 1, and a configuration whose
        train.accumulate_grad_batches is not 1 is refused (from_config reads it instead)."""
        from .engine import AccumWindow, GradReducer

        if not isinstance(model, DCTCNLightningModule):
            raise TypeError("DCTCNTrainStep drives a dctcn.DCTCNLightningModule")
        cfg = model.config
        if accumulate is None:
            if int(cfg.get_path("train.accumulate_grad_batches", 1)) != 1:
                raise ValueError("train.accumulate_grad_batches is not 1: pass accumulate=N to DCTCNTrainStep, or build the step with "
                                 "DCTCNTrainStep.from_config, which reads it")
            accumulate = 1
        if int(accumulate) < 1:
            raise ValueError("accumulate (accumulate_grad_batches) must be >= 1")
        if grad_comm_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("grad_comm_dtype must be torch.float32 or torch.bfloat16")
        opt = cfg.get_path("optim.optimizer", None)
        if opt is None or str(opt.get("opt", "adamw")).lower() != "adamw":
            raise ValueError("optim.optimizer.opt must be adamw (the shipped dc-tcn-base.yaml)")
        sch = cfg.get_path("optim.scheduler", None)
        if sch is None or "max_lr" not in sch:
            raise ValueError("optim.scheduler needs max_lr (torch.optim.lr_scheduler.OneCycleLR)")
        if not bool(sch.get("cycle_momentum", True)):
            raise NotImplementedError("optim.scheduler.cycle_momentum = false is not built (the kernel always cycles beta1)")
        betas = [float(b) for b in opt.get("betas", (0.9, 0.999))]
        self.schedule = ops.onecycle_schedule(float(sch["max_lr"]), int(total_steps), pct_start=float(sch.get("pct_start", 0.3)),
                                              anneal_strategy=str(sch.get("anneal_strategy", "cos")), three_phase=bool(sch.get("three_phase", False)),
                                              div_factor=float(sch.get("div_factor", 25.0)), final_div_factor=float(sch.get("final_div_factor", 1e4)),
                                              base_momentum=float(sch.get("base_momentum", 0.85)), max_momentum=float(sch.get("max_momentum", 0.95)))
        self.total_steps = int(total_steps)
        self.mixup_alpha = float(cfg.get_path("optim.mixup_alpha", 0.0))
        self.model, self.pipeline, self.seed = model, pipeline, int(seed)
        self.window = AccumWindow(int(accumulate))
        grouped = bool(data_parallel) and dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(process_group) if grouped else 1
        self.rank = dist.get_rank(process_group) if grouped else 0          # (of the dropout seeds: dropout_seed)
        self.dp = GradReducer(model, process_group, bucket_mb, always_reduce, grad_comm_dtype) if data_parallel and (self.world > 1 or always_reduce) else None
        if self.dp is not None:
            # the reducer's constructor broadcast rank 0's parameters and buffers into the store and marked the shadows stale; the tap-major /
            # transposed weight copies and the folded coefficients of this module are derived from them as well
            model.mark_params_dirty()
            model.grad_ready_hook = self._on_ready
        if not data_parallel:
            model.grad_ready_hook = None
        self._before_frontend = 0
        self.last_reduce: Optional[dict] = None          # the buckets of the last step (None without a reducer): _reduce_report
        self.adamw = ops.AdamW(model.store(), self.schedule, betas[1], float(opt.get("eps", 1e-8)), float(opt.get("weight_decay", 1e-2)),
                               float(cfg.get_path("train.gradient_clip_val", 0.0) or 0.0))
        self.m, self.v, self.opt_state = self.adamw.m, self.adamw.v, self.adamw.opt_state
        self.steps = 0         # host mirror of the device counter: see the module docstring and resync()
        self.micro_steps = 0   # calls of step() so far: the index of the next dropout seed

    @classmethod
    def from_config(cls, model: DCTCNLightningModule, total_steps: int, **kw) -> "DCTCNTrainStep":
        """The step of the model's own configuration: accumulate = train.accumulate_grad_batches (the reference hands it to the Trainer)
        unless the caller states one."""
        if kw.get("accumulate") is None and isinstance(model, DCTCNLightningModule):
            kw["accumulate"] = int(model.config.get_path("train.accumulate_grad_batches", 1) or 1)
        return cls(model, total_steps, **kw)

    def values(self, step: Optional[int] = None) -> tuple:
        """(learning rate, beta1) of optimiser step `step` (default: the next one) on the host, for logging: ops.onecycle_values."""
        return ops.onecycle_values(self.steps if step is None else int(step), **self.schedule)

    # -- data parallel -----------------------------------------------------------------------------------
    def _on_ready(self, lo: int) -> None:
        """The model's gradient-ready notification -> the reducer.  A notification at or above the front-end's boundary comes from the
        back-end's backward, before the front-end's starts: the buckets launched by then are counted for last_reduce."""
        dp = self.dp
        dp.on_ready(lo)
        if dp.sync and dp._st is not None and lo >= dp._st.front_end:
            self._before_frontend = len(dp.launched)

    def _reduce_report(self, synced: bool) -> None:
        """last_reduce = {"buckets": ranges handed to the reducer in this step, "before_frontend": how many of them before the front-end's
        backward began, "covered": they tile the whole gradient buffer}; all zero / False for a micro-step that did not synchronise."""
        if not synced:
            self.last_reduce = {"buckets": 0, "before_frontend": 0, "covered": False}
            return
        ranges, numel = sorted(self.dp.launched), self.model.store().numel
        covered = bool(ranges) and ranges[0][0] == 0 and ranges[-1][1] == numel and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        self.last_reduce = {"buckets": len(ranges), "before_frontend": int(self._before_frontend), "covered": covered}

    # -- one step ----------------------------------------------------------------------------------------
    def step(self, batch, lam: Optional[float] = None) -> dict:
        """One optimisation step; with accumulate = N > 1 one micro-step of a window (the optimiser runs in every N-th call).  batch: the
        keyword arguments (or the positional tuple) of DCTCNLightningModule.forward; with a pipeline attached, the keyword arguments of
        augment.DeviceDCTCNPipeline.__call__ (frames_u8, waves, labels, boundaries).  lam: mixup's weight; None draws
        0.5 - |0.5 - Beta(a, a)| from np.random as the reference does (0 when optim.mixup_alpha is 0).  The dropout seed is
        dropout_seed(seed, rank, total_steps, accumulate, micro_steps).  -> the five metrics of this micro-batch (unscaled) as device tensors."""
        model = self.model
        if model.training:
            raise RuntimeError("DCTCNTrainStep runs on a module in eval mode (the training arithmetic is loss_and_grads')")
        if self.steps >= self.total_steps:
            raise ValueError(f"Tried to step {self.steps + 1} times. The specified number of total steps is {self.total_steps}")
        if lam is None:
            lam = 0.0
            if self.mixup_alpha > 0:
                import numpy as np

                lam = float(0.5 - abs(0.5 - np.random.beta(self.mixup_alpha, self.mixup_alpha)))          # lightning.py:266
        if not isinstance(batch, dict):
            batch = dict(zip(("videos", "audios", "labels", "word_mask", "attention_mask"), batch))
        plan, n = self.window.plan(), self.window.n
        try:
            mixed = False
            if self.pipeline is not None:
                batch, mixed = self.pipeline(**batch, lam=lam), True
            if self.dp is not None:
                self._before_frontend = 0
                self.dp.begin_step(sync=plan["reduce"])          # (sync=False: DDP's no_sync — neither a gradient nor a buffer collective)
            out = model.loss_and_grads(**batch, loss_scale=1.0 / n, accumulate=not plan["zero"], lam=lam, videos_mixed=mixed,
                                       dropout_seed=dropout_seed(self.seed, self.rank, self.total_steps, n, self.micro_steps))
            self.micro_steps += 1
            if plan["optimise"]:
                self._optimise()
            elif self.dp is not None:
                self._reduce_report(False)
        except BaseException:
            # the micro-step may have added any part of its gradient to the buffer: what the window had accumulated is not stepped on, the
            # next step() starts a new window (and stores); parameters and optimiser state are as the last completed window left them
            self.window.abort()
            model._drop_backward_state()
            raise
        self.window.advance()
        return {k: out[k] for k in METRICS}

    def _optimise(self) -> None:
        """The tail of a window's last micro-step (of every step with accumulate = 1): the reducer's join, the clip's sum of squares and
        the ONE AdamW launch, on the averaged, accumulated gradient."""
        model = self.model
        st = model.store()
        if self.m.device != st.device or self.m.numel() != st.numel:
            raise RuntimeError("the model's parameter store changed under the optimiser state (moved to another device?)")
        if self.dp is not None:
            self.dp.finish()
            self._reduce_report(True)
        if self.adamw.max_norm > 0:
            self.adamw.sumsq(st)
        self.adamw.apply(st)
        self.steps += 1
        model.mark_params_dirty()          # the tap-major / transposed weight copies and the folded coefficients are rebuilt at the next forward

    def flush(self) -> bool:
        """Closes a partial window (the end of an epoch whose batch count is no multiple of N: Lightning steps on the last batch): the
        all-reduce under data parallelism (every rank calls flush()), the clip and AdamW run on what has been accumulated, which keeps
        its 1/N scale.  Nothing happens at a window boundary.  -> True when an optimiser step was made."""
        if not self.window.flush():
            return False
        if self.dp is not None:
            self._before_frontend = 0
            self.dp.begin_step()
            self.dp.on_ready(0)
        self._optimise()
        return True

    def resync(self) -> int:
        """The host mirror takes the device counter's value (synchronises) and the micro-step count follows it -> the steps counted so far."""
        self.steps = int(self.opt_state[0].item())
        self.micro_steps = self.steps * self.window.n + self.window.pos
        return self.steps

    def state(self) -> dict:
        """The device state's scalar words (synchronises): step, skipped, lr, gnorm, beta1, error (ops.opt_state_words), and micro_step, the
        position of the NEXT step() inside its window (always 0 with accumulate = 1)."""
        return {**self.adamw.state(), "micro_step": self.window.pos}

    def state_dict(self) -> dict:
        """AdamW's moments (flat fp32, parameter-store order) and the step counter with the rest of the device state.  Taken inside a
        window it also carries the window's position (accum_window) and the gradient accumulated so far (accum_grad), so that a resumed
        run finishes the window."""
        sd = {**self.adamw.moments(), "steps": int(self.steps), "micro_steps": int(self.micro_steps), "seed": int(self.seed),
              "total_steps": int(self.total_steps)}
        win = self.window.state_dict()
        if win:
            sd.update(win)
            sd["accum_grad"] = self.model.store().grad.detach().clone()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        if sd["exp_avg"].numel() != self.m.numel() or sd["opt_state"].numel() != self.opt_state.numel():
            raise ValueError("optimiser state of another model")
        if int(sd["total_steps"]) != self.total_steps:
            raise ValueError(f"the state was saved under total_steps = {int(sd['total_steps'])}, this schedule has {self.total_steps}")
        self.window.load_state_dict(sd)          # (a state saved inside a window of another N raises here, before anything is written)
        if self.window.pos:
            st = self.model.store()
            if "accum_grad" not in sd or sd["accum_grad"].numel() != st.grad.numel():
                self.window.abort()
                raise ValueError("a state saved inside a window carries the accumulated gradient (accum_grad) of this parameter layout")
            st.rebind_grads()          # (a .grad that is None would be zero-filled by the next adding backward)
            st.grad.copy_(sd["accum_grad"])
        self.adamw.load_moments(sd)
        self.opt_state.copy_(sd["opt_state"])
        self.seed = int(sd["seed"])
        self.resync()          # (the saved mirror, sd["steps"], may have run ahead of the counter: the device's count is the schedule's)
        if "micro_steps" in sd and int(sd["steps"]) == self.steps:
            self.micro_steps = int(sd["micro_steps"])          # (differs from resync()'s only after a flushed partial window)
