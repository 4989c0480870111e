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

``steps`` is a HOST mirror of the device step counter (it picks the step's dropout seed and raises past ``total_steps`` without a
read-back).  The device does not count a step whose gradient norm is not finite (nothing is written: ``state()["skipped"]``), so after such
a step the mirror runs ahead by one: the dropout seeds shift and the host refuses the last step of the schedule.  ``resync()`` reads the
device counter back into the mirror (one synchronisation; ``load_state_dict`` does it).

NOT built here (engine.TrainStep has them for the transformer models): native step lists, HIP-graph capture, data-parallel training and
gradient accumulation (``train.accumulate_grad_batches`` other than 1 raises)."""
from __future__ import annotations

from typing import Optional

from . import ops
from .dctcn import DCTCNLightningModule

METRICS = ("loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5")


class DCTCNTrainStep:
    def __init__(self, model: DCTCNLightningModule, total_steps: int, pipeline=None, seed: int = 0):
        if not isinstance(model, DCTCNLightningModule):
            raise TypeError("DCTCNTrainStep drives a dctcn.DCTCNLightningModule")
        cfg = model.config
        if int(cfg.get_path("train.accumulate_grad_batches", 1)) != 1:
            raise ValueError("train.accumulate_grad_batches must be 1: DCTCNTrainStep does not accumulate gradients")
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
        self.adamw = ops.AdamW(model.store(), self.schedule, betas[1], float(opt.get("eps", 1e-8)), float(opt.get("weight_decay", 1e-2)),
                               float(cfg.get_path("train.gradient_clip_val", 0.0) or 0.0))
        self.m, self.v, self.opt_state = self.adamw.m, self.adamw.v, self.adamw.opt_state
        self.steps = 0         # host mirror of the device counter: see the module docstring and resync()

    def values(self, step: Optional[int] = None) -> tuple:
        """(learning rate, beta1) of optimiser step `step` (default: the next one) on the host, for logging: ops.onecycle_values."""
        return ops.onecycle_values(self.steps if step is None else int(step), **self.schedule)

    def step(self, batch, lam: Optional[float] = None) -> dict:
        """One optimisation step.  batch: the keyword arguments (or the positional tuple) of DCTCNLightningModule.forward; with a pipeline
        attached, the keyword arguments of augment.DeviceDCTCNPipeline.__call__ (frames_u8, waves, labels, boundaries).  lam: mixup's
        weight; None draws 0.5 - |0.5 - Beta(a, a)| from np.random as the reference does (0 when optim.mixup_alpha is 0).  The dropout
        seed of the step is seed + its index.  -> the five metrics as device tensors."""
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
        mixed = False
        if self.pipeline is not None:
            batch, mixed = self.pipeline(**batch, lam=lam), True
        out = model.loss_and_grads(**batch, dropout_seed=self.seed + self.steps, lam=lam, videos_mixed=mixed)
        st = model.store()
        if self.m.device != st.device or self.m.numel() != st.numel:
            raise RuntimeError("the model's parameter store changed under the optimiser state (moved to another device?)")
        if self.adamw.max_norm > 0:
            self.adamw.sumsq(st)
        self.adamw.apply(st)
        self.steps += 1
        model.mark_params_dirty()          # the tap-major / transposed weight copies and the folded coefficients are rebuilt at the next forward
        return {k: out[k] for k in METRICS}

    def resync(self) -> int:
        """The host mirror takes the device counter's value (synchronises) -> the steps counted so far."""
        self.steps = int(self.opt_state[0].item())
        return self.steps

    def state(self) -> dict:
        """The device state's scalar words (synchronises): step, skipped, lr, gnorm, beta1, error (ops.opt_state_words)."""
        return self.adamw.state()

    def state_dict(self) -> dict:
        """AdamW's moments (flat fp32, parameter-store order) and the step counter with the rest of the device state."""
        return {**self.adamw.moments(), "steps": int(self.steps), "seed": int(self.seed), "total_steps": int(self.total_steps)}

    def load_state_dict(self, sd: dict) -> None:
        if sd["exp_avg"].numel() != self.m.numel() or sd["opt_state"].numel() != self.opt_state.numel():
            raise ValueError("optimiser state of another model")
        if int(sd["total_steps"]) != self.total_steps:
            raise ValueError(f"the state was saved under total_steps = {int(sd['total_steps'])}, this schedule has {self.total_steps}")
        self.adamw.load_moments(sd)
        self.opt_state.copy_(sd["opt_state"])
        self.seed = int(sd["seed"])
        self.resync()          # (the saved mirror, sd["steps"], may have run ahead of the counter: the device's count is the schedule's)
