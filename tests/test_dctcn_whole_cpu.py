"""Whole-model DC-TCN training, host side (no GPU): the OneCycle schedule's host restatement against torch's own scheduler, the C ABI of the
two new optimiser entry points, the whole-model training restatement against the reference's recorded numbers, and the errors the training
step raises before it launches anything."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dctcn_whole_restatement as WR  # noqa: E402
from dctcn_cases import rel_err  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "dctcn_whole_train_tiny.npz")

SCHEDULES = list(itertools.product((1, 2, 3, 10, 97), (0.0, 0.3, 1.0), ("cos", "linear"), (False, True)))


@pytest.mark.parametrize("total,pct,anneal,three", SCHEDULES, ids=[f"n{t}-p{p}-{a}-{'3ph' if th else '2ph'}" for t, p, a, th in SCHEDULES])
def test_onecycle_values_are_torchs_schedule(total, pct, anneal, three):
    """lr and betas[0] of every step against OneCycleLR on an AdamW, to float64 rounding (both sides are Python floats).  A combination is
    left out only where torch itself refuses it, and then the restatement must refuse it too."""
    from syncvsr_amd import ops

    max_lr = 3e-4
    sched = ops.onecycle_schedule(max_lr, total, pct_start=pct, anneal_strategy=anneal, three_phase=three)
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999))
    try:
        torch_sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total, pct_start=pct, anneal_strategy=anneal,
                                                          three_phase=three)
    except ZeroDivisionError:          # (step 0 sits in a phase of length zero: the constructor's own first step divides by zero)
        with pytest.raises(ZeroDivisionError):
            ops.onecycle_values(0, **sched)
        return
    for step in range(total):
        lr, beta1 = ops.onecycle_values(step, **sched)
        assert isinstance(lr, float) and isinstance(beta1, float)
        tl, tb = opt.param_groups[0]["lr"], opt.param_groups[0]["betas"][0]
        assert abs(lr - tl) <= 1e-12 * abs(tl), (step, lr, tl)
        assert abs(beta1 - tb) <= 1e-12 * abs(tb), (step, beta1, tb)
        assert opt.param_groups[0]["betas"][1] == 0.999
        p.grad = torch.ones(3)
        opt.step()
        if step + 1 < total:
            try:
                torch_sched.step()
            except ZeroDivisionError:
                with pytest.raises(ZeroDivisionError):
                    ops.onecycle_values(step + 1, **sched)
                return
    with pytest.raises(ValueError, match="total number of|number of total steps"):
        ops.onecycle_values(total, **sched)


def test_shipped_schedule_starts_at_the_peak_and_ends_at_min_lr():
    """pct_start = 0.0 (dc-tcn-base.yaml): the first phase ends at step -1, so step s of n sits at (s + 1) / n of the falling phase."""
    import math

    from syncvsr_amd import ops

    s = ops.onecycle_schedule(3e-4, 10, pct_start=0.0)
    lr0, b0 = ops.onecycle_values(0, **s)
    want = s["min_lr"] + (s["max_lr"] - s["min_lr"]) / 2.0 * (math.cos(math.pi * 0.1) + 1)
    assert abs(lr0 - want) <= 1e-15 and 0.85 < b0 < 0.86
    lr9, b9 = ops.onecycle_values(9, **s)
    assert abs(lr9 - s["min_lr"]) <= 1e-12 * s["min_lr"] + 1e-19 and abs(b9 - 0.95) <= 1e-15


def test_new_symbols_are_declared_bound_and_exported():
    from syncvsr_amd import _lib, ops

    decl = _lib.parse_header()
    head = ["p", "g", "m", "v", "shadow", "n", "decay_end", "beta2", "eps", "weight_decay", "max_norm", "schedule", "opt_state"]
    assert [n for _, n in decl["svsr_adamw_onecycle_step"]] == head + ["stream"]
    assert [n for _, n in decl["svsr_adamw_onecycle_range"]] == head + ["advance", "stream"]
    # the flat contract of svsr_adamw_range: the same leading arguments, the same tail
    old = [n for _, n in decl["svsr_adamw_range"]]
    assert old[:7] == head[:7] and old[-3:] == ["opt_state", "advance", "stream"]
    types = dict((n, t) for t, n in decl["svsr_adamw_onecycle_range"])
    assert types["n"] == "int64_t" and types["decay_end"] == "int64_t" and types["schedule"] == "const void*"
    import ctypes

    assert ctypes.sizeof(ops._OneCycleRecord) == 64 and ops.ONECYCLE_STATE_WORDS == 4 + ops.SUMSQ_PARTS + 4
    src = open(os.path.join(ROOT, "syncvsr_amd", "csrc", "loss_optim.hip")).read()
    body = src[src.index("struct OneCycleState"): src.index("// shadow casts")]
    # one update kernel and one advancing kernel, templates over the schedule policy; the OneCycle policy sits in the OneCycle section
    assert src.count("void k_adamw(") == 1 and src.count("void k_opt_advance(") == 1 and "struct OneCycleSched {" in body
    assert "k_adamw_onecycle" not in src and "k_onecycle_advance" not in src
    assert src.count("beta2 * a.v[i]") == 1, "the update rule is written once"
    assert "atomic" not in body.lower(), "the OneCycle optimiser uses no atomics"
    assert "struct OneCycleState { OptState o; float beta1_last; int error; int reserved[2]; };" in body
    # svsr_adamw_range / svsr_adamw_step are as they were: what their kernels are instantiated with reads no OneCycle field
    old_body = src[src.index("struct AdamArgs"): src.index("// AdamW under torch.optim.lr_scheduler.OneCycleLR")]
    assert "struct CosineSched {" in old_body and "OneCycle" not in old_body
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    for name in ("svsr_adamw_onecycle_step", "svsr_adamw_onecycle_range"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert lib.svsr_steplist_knows(name.encode())
    # schedules no step can be taken from are refused on the host, before any launch (n = 0; the state is a real, zeroed buffer)
    state = (ctypes.c_int32 * ops.ONECYCLE_STATE_WORDS)()
    for bad in (dict(total_steps=1, pct_start=1.0), dict(total_steps=2, pct_start=0.5)):
        sched = ops.onecycle_schedule(3e-4, **bad)
        rc = lib.svsr_adamw_onecycle_range(None, None, None, None, None, 0, 0, 0.999, 1e-6, 1e-2, 0.0, ops._onecycle_record(sched), state, 1, None)
        assert rc == 1001, (bad, rc)


@pytest.mark.parametrize("run", list(WR.RUNS))
def test_whole_restatement_reproduces_the_reference(run):
    """fp64 autograd of tests/dctcn_whole_restatement.py against what the reference's own Lipreading in .train() gave (B = 2, T = 7, 40 x 40):
    losses, the updated running statistics of the stem's norm and one trunk norm, and the recorded gradients, to the 1e-9 of
    make_golden_dctcn_train.py."""
    gold = np.load(GOLD, allow_pickle=False)
    cfg, dims, sd, batch = WR.whole_case(2)
    out, grads, gf, new_stats = WR.whole_grads(cfg, dims, sd, batch, float(cfg.optim.lambda_audio), None, **WR.RUNS[run])
    for k in ("loss_total", "loss_category", "loss_audio"):
        assert rel_err(out[k], gold[f"{run}.{k}"]) < 1e-9, k
    for bn in WR.GOLD_STATS:
        for b in ("running_mean", "running_var"):
            assert rel_err(new_stats[f"{bn}.{b}"], gold[f"{run}.stat.{bn}.{b}"]) < 1e-9, (bn, b)
    seen = set()
    for n in WR.GOLD_GRADS:
        assert rel_err(WR.sub(grads[n]), gold[f"{run}.grad.{n}"]) < 1e-9, n
        assert float(np.abs(gold[f"{run}.grad.{n}"]).max()) > 0.0, n
        seen.add(n)
    # what the golden must hold: the stem, layer1.0.conv1, layer2.0.downsample.0, one bn weight per stage, the first back-end stage, both heads
    need = ["model.frontend3D.0.weight", "model.trunk.layer1.0.conv1.weight", "model.trunk.layer2.0.downsample.0.weight", "video_classifier.weight",
            "audio_projection.weight", f"{WR.R.TCN}.transition0.conv.weight"] + [f"model.trunk.layer{i}." for i in range(1, 5)]
    for n in need:
        assert any(s == n or (n.endswith(".") and s.startswith(n) and (".bn" in s or ".downsample.1" in s)) for s in seen), n


def test_mixup_moves_the_front_end_gradients():
    gold = np.load(GOLD, allow_pickle=False)
    n = "model.frontend3D.0.weight"
    assert rel_err(gold[f"mix.grad.{n}"], gold[f"plain.grad.{n}"]) > 1e-2


def test_trainstep_refuses_accumulation_and_foreign_recipes():
    from syncvsr_amd.dctcn_init import tiny_dctcn_config
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    class NoStore:
        pass

    with pytest.raises(TypeError):
        DCTCNTrainStep(NoStore(), 5)
    from syncvsr_amd.dctcn import DCTCNLightningModule

    for kw, exc, word in ((dict(train__accumulate_grad_batches=2), ValueError, "accumulate_grad_batches"),
                          (dict(optim__optimizer__opt="sgd"), ValueError, "adamw"),
                          (dict(optim__scheduler__cycle_momentum=False), NotImplementedError, "cycle_momentum")):
        m = DCTCNLightningModule(tiny_dctcn_config(True, **kw))
        with pytest.raises(exc, match=word):
            DCTCNTrainStep(m, 5)
