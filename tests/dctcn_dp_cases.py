"""What tests/test_gpu_dctcn_accum.py and tests/test_gpu_dctcn_ddp_ranks.py share: the tiny whole-model case (tests/dctcn_whole_restatement
.whole_case: T = 7, 40 x 40) with the clip on, its micro-batches, and the optimiser of the BY-HAND definitions.  The definitions are built
from the entry points whose parity with the reference other suites pin — DCTCNLightningModule.loss_and_grads (tests/test_gpu_dctcn_whole_grads
.py) and ops.AdamW (tests/test_gpu_dctcn_trainstep.py, tests/test_gpu_kernels.py) — and never from dctcn_train.DCTCNTrainStep."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dctcn_whole_restatement as WR  # noqa: E402

TOTAL, STEPS, SEED, CLIP = 5, 3, 11, 1.0
LAMS = (0.0, 0.3, 0.15, 0.25, 0.05, 0.2)          # one per micro-step (a rank takes its own: lam_of)
METRICS = ("loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5")
KEYS = ("videos", "audios", "labels", "word_mask", "attention_mask")


def case(B: int = 2):
    cfg, dims, sd, batch = WR.whole_case(B)
    cfg.set_path("train.gradient_clip_val", CLIP)
    return cfg, dims, sd, batch


def second_batch(cfg, B: int = 2):
    """A micro-batch other than whole_case's (other clips, tokens, labels and lengths)."""
    from syncvsr_amd.dctcn_init import dctcn_synthetic_batch

    return dctcn_synthetic_batch(cfg, B, 7, size=40, seed=77, lengths=[5, 7, 6, 4][:B])


def to_args(batch, dev) -> dict:
    return dict(zip(KEYS, (t.to(dev) for t in batch)))


def shard(batch, rank: int, world: int):
    n = batch[0].shape[0] // world
    return [t[rank * n:(rank + 1) * n].contiguous() for t in batch]


def lam_of(rank: int, micro: int) -> float:
    """The mixup weight rank `rank` is handed for its micro-step `micro`: per rank and per micro-batch, as the reference draws it."""
    return LAMS[(micro + 2 * rank) % len(LAMS)]


def build_model(cfg, sd, dev, seed=None):
    from syncvsr_amd.dctcn import DCTCNLightningModule

    m = DCTCNLightningModule(cfg, seed=seed)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(dev).eval()


def hand_adamw(model, cfg, total: int = TOTAL):
    """ops.AdamW under OneCycleLR from the configuration, as dctcn_train builds it (torch's defaults for what the yaml leaves out)."""
    from syncvsr_amd import ops

    o, s = cfg.optim.optimizer, cfg.optim.scheduler
    sched = ops.onecycle_schedule(float(s["max_lr"]), total, pct_start=float(s.get("pct_start", 0.3)), anneal_strategy=str(s.get("anneal_strategy", "cos")),
                                  three_phase=bool(s.get("three_phase", False)), div_factor=float(s.get("div_factor", 25.0)),
                                  final_div_factor=float(s.get("final_div_factor", 1e4)), base_momentum=float(s.get("base_momentum", 0.85)),
                                  max_momentum=float(s.get("max_momentum", 0.95)))
    betas = [float(b) for b in o.get("betas", (0.9, 0.999))]
    return ops.AdamW(model.store(), sched, betas[1], float(o.get("eps", 1e-8)), float(o.get("weight_decay", 1e-2)), CLIP)


def hand_optimise(model, adamw) -> None:
    """The clip's sum of squares and the one AdamW launch on whatever the store's gradient buffer holds."""
    st = model.store()
    adamw.sumsq(st)
    adamw.apply(st)
    model.mark_params_dirty()


def metrics_of(out: dict) -> dict:
    return {k: out[k].detach().clone() for k in METRICS}


def same_metrics(a: dict, b: dict) -> None:
    for k in METRICS:
        assert torch.equal(a[k].cpu(), b[k].cpu()), (k, float(a[k]), float(b[k]))
