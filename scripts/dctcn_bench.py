"""Eval forward of the DC-TCN word-level model (syncvsr_amd/dctcn.py) beside a torch eager bf16 module built from the SAME state dict, in
the same process on the same device: the back-end alone (front-end features in, word logits out) and the whole forward (videos in, logits
out) at B = 96 and B = 32, T = 29, 96 x 96.

    python scripts/dctcn_bench.py [--batches 96,32] [--rounds 7] [--iters 50] [--out profiles/dctcn_eval.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/dctcn_bench.py --profile-only        # kernel table, in a run of its own
    python scripts/dctcn_bench.py --backward [--profile-only]      # forward + backward of the back-end and heads against eager bf16 autograd
    python scripts/dctcn_bench.py --train [--batches 96]           # the same in the training arithmetic (batch statistics, dropout) -> profiles/dctcn_train.json
    python scripts/dctcn_bench.py --step [--batches 32]            # the WHOLE training step (dctcn_train.DCTCNTrainStep, 88 x 88) -> profiles/dctcn_step.json
    python scripts/dctcn_bench.py --step --gpus N [--accumulate M] # the step on N data-parallel ranks (torch.distributed.run, one GPU each; N = 1: the
                                                                   # 1-rank always_reduce leg) -> profiles/dctcn_step_dp.json
    python scripts/dctcn_bench.py --step --accumulate M            # windows of M micro-steps in one process -> profiles/dctcn_step_dp.json

Times are wall-clock between device synchronisations (host dispatch included), the two implementations ALTERNATING round by round after
warm-up of every shape; per implementation the median over rounds of the mean of `--iters` calls, and the minimum.  The convolution
event figures (tconv_ms, se_ms: device events around the host calls, ops.start_event_timing) include dispatch gaps and are NOT kernel times:
kernel time comes from the rocprofv3 run above.  The convolution FLOPs from the shapes (2 * rows * n_in * k *
co per branch), the peak from --peak-tflops (dense bf16 of the device).  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

TCN = "model.tcn.tcn_trunk.features"


class EagerDCTCN:
    """Plain torch eager, bf16 weights and activations ([B, C, T] as torch's Conv1d wants), BatchNorm in eval mode: the baseline."""

    def __init__(self, sd: dict, dims: dict, dev):
        self.W = {k: (v.to(dev).to(torch.bfloat16) if v.is_floating_point() else v.to(dev)) for k, v in sd.items()}
        self.dims = dims
        self.train, self.p_drop = False, 0.0          # --train: batch-statistic BatchNorm1d in the back-end, dropout0 / dropout1
        self.train_frontend = False                   # --step: batch statistics in the front-end's norms too

    def bn(self, x, p):
        W = self.W
        if self.train and (self.train_frontend or p.startswith(TCN)):
            return F.batch_norm(x, W[f"{p}.running_mean"], W[f"{p}.running_var"], W[f"{p}.weight"], W[f"{p}.bias"], True, 0.1, 1e-5)
        return F.batch_norm(x, W[f"{p}.running_mean"], W[f"{p}.running_var"], W[f"{p}.weight"], W[f"{p}.bias"], False, 0.0, 1e-5)

    def frontend(self, videos):
        W = self.W
        B, _, T = videos.shape[:3]
        h = F.conv3d(videos.to(torch.bfloat16), W["model.frontend3D.0.weight"], None, stride=(1, 2, 2), padding=(2, 3, 3))
        h = F.max_pool3d(F.silu(self.bn(h, "model.frontend3D.1")), (1, 3, 3), (1, 2, 2), (0, 1, 1))
        h = h.transpose(1, 2).reshape(B * T, 64, h.size(3), h.size(4))
        for li in range(1, 5):
            for bi in range(2):
                p = f"model.trunk.layer{li}.{bi}"
                stride = 2 if (bi == 0 and li > 1) else 1
                o = F.silu(self.bn(F.conv2d(h, W[f"{p}.conv1.weight"], None, stride=stride, padding=1), f"{p}.bn1"))
                o = self.bn(F.conv2d(o, W[f"{p}.conv2.weight"], None, stride=1, padding=1), f"{p}.bn2")
                r = self.bn(F.conv2d(h, W[f"{p}.downsample.0.weight"], None, stride=stride), f"{p}.downsample.1") if f"{p}.downsample.0.weight" in W else h
                h = F.silu(o + r)
        return h.mean((2, 3)).view(B, T, 512)

    def backend(self, feats, word_mask, attention_mask, want_hidden: bool = False):
        W, dm = self.W, self.dims
        x = feats
        if dm["in_size"] == 513:
            x = torch.cat([x, word_mask.to(x.dtype).unsqueeze(2)], dim=-1)
        x = x.transpose(1, 2)
        p = f"{TCN}.transition0"
        x = F.prelu(self.bn(F.conv1d(x, W[f"{p}.conv.weight"]), f"{p}.norm"), W[f"{p}.prelu.weight"])
        ks, ds = dm["ks"], dm["ds"]
        for bi, nl in enumerate(dm["blocks"]):
            feats_list = [x]
            for li in range(nl):
                p = f"{TCN}.denseblock{bi + 1}.denselayer{li + 1}"
                d = ds[li % len(ds)]
                xc = torch.cat(feats_list, 1)
                outs = []
                for ki, k in enumerate(ks):
                    y = xc.mean(2)
                    y = torch.sigmoid(F.linear(F.silu(F.linear(y, W[f"{p}.cbcr0_se_{ki}.fc.0.weight"])), W[f"{p}.cbcr0_se_{ki}.fc.2.weight"]))
                    c = F.conv1d(xc * y.unsqueeze(2), W[f"{p}.cbcr0_{ki}.net.0.weight"], W[f"{p}.cbcr0_{ki}.net.0.bias"], padding=(k - 1) * d, dilation=d)
                    c = self.bn(c, f"{p}.cbcr0_{ki}.net.1")
                    outs.append(F.silu(c[:, :, (k - 1) * d // 2: c.size(2) - (k - 1) * d // 2].contiguous()))
                o0 = F.dropout(torch.cat(outs, 1), self.p_drop, self.train)
                outs = []
                for ki, k in enumerate(ks):
                    c = F.conv1d(o0, W[f"{p}.cbcr1_{ki}.net.0.weight"], W[f"{p}.cbcr1_{ki}.net.0.bias"], padding=(k - 1) * d, dilation=d)
                    c = self.bn(c, f"{p}.cbcr1_{ki}.net.1")
                    outs.append(F.silu(c[:, :, (k - 1) * d // 2: c.size(2) - (k - 1) * d // 2].contiguous()))
                res = F.conv1d(xc, W[f"{p}.downsample.weight"], W[f"{p}.downsample.bias"])
                feats_list.append(F.silu(F.dropout(torch.cat(outs, 1), self.p_drop, self.train) + res))
            x = torch.cat(feats_list, 1)
            if bi != len(dm["blocks"]) - 1:
                p = f"{TCN}.transition{bi + 1}"
                x = F.silu(self.bn(F.conv1d(x, W[f"{p}.conv.weight"]), f"{p}.norm"))
        h = self.bn(x, f"{TCN}.norm5")
        am = attention_mask.to(h.dtype)
        pooled = (h * am.unsqueeze(1)).sum(2) / (am.sum(1, keepdim=True) + 1e-6)
        logits = F.linear(pooled, W["video_classifier.weight"], W["video_classifier.bias"]).float()
        if not want_hidden:
            return logits
        return logits, h

    def backend_params(self) -> list:
        """Leaves of the backward leg: every floating-point tensor of the temporal network and the heads that is a parameter."""
        return [v for k, v in self.W.items() if k.startswith((TCN, "video_classifier", "audio_projection")) and v.is_floating_point()
                and "running_" not in k]

    def loss_and_grads(self, feats, word_mask, attention_mask, tokens, labels, lam: float):
        """bf16 autograd of the same modules: both cross-entropies of lightning.py:280-312 (lam = 0), gradients of every back-end parameter."""
        params = self.backend_params()
        for p in params:
            p.requires_grad_(True)
            p.grad = None
        logits, h = self.backend(feats, word_mask, attention_mask, want_hidden=True)
        B, C, T = h.shape
        la = F.linear(h.transpose(1, 2), self.W["audio_projection.weight"], self.W["audio_projection.bias"])
        A, V = self.dims["A"], self.dims["V"]
        loss = F.cross_entropy(logits, labels) + lam * F.cross_entropy(la.reshape(-1, V).float(), tokens[:, : T * A].reshape(-1))
        loss.backward()
        return loss


def _time(fn, iters: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def backward_leg(a) -> None:
    """Features in, all gradients out; same alternating / median protocol as the forward.  Merges "timing" into profiles/dctcn_backward.json
    (the file also holds the bf16 floor of the tests)."""
    from syncvsr_amd import ops
    from syncvsr_amd.dctcn import DCTCNLightningModule
    from syncvsr_amd.dctcn_init import dctcn_dims, dctcn_init_state_dict, dctcn_synthetic_batch, default_dctcn_config

    dev = torch.device("cuda:0")
    cfg = default_dctcn_config()
    sd = dctcn_init_state_dict(cfg, seed=0)
    model = DCTCNLightningModule(cfg)
    model.load_state_dict(sd)
    model.to(dev).eval()
    eager = EagerDCTCN(sd, dctcn_dims(cfg), dev)
    if a.train:
        eager.train, eager.p_drop = True, float(cfg.model.dctcn.densetcn_options.dropout)
    lam, T, rows = model.lambda_audio, a.frames, []
    for B in [int(v) for v in a.batches.split(",")]:
        videos, tokens, labels, wm, am = [t.to(dev) for t in dctcn_synthetic_batch(cfg, B, T, seed=B)]
        labels = labels.long()
        with torch.no_grad():
            feats16 = eager.frontend(videos).contiguous()
        feats_hip = feats16.reshape(B * T, 512).contiguous()
        fns = {
            "hip_backward": lambda: model.loss_and_backend_grads_from_features(feats_hip, B, T, tokens, labels, wm, am),
            "eager_backward": lambda: eager.loss_and_grads(feats16, wm, am, tokens, labels, lam),
            "hip_forward_only": lambda: model._losses((B, T), tokens, labels, wm, am, None, feats_hip),
        }
        if a.train:          # the training arithmetic beside this project's own eval-statistics backward (hip_backward) and eager .train() autograd
            fns["hip_train"] = lambda: model.loss_and_backend_grads_from_features(feats_hip, B, T, tokens, labels, wm, am, train_stats=True,
                                                                                  dropout_seed=1)
            del fns["hip_forward_only"]
        for fn in fns.values():
            _time(fn, 3)
        if a.profile_only:
            continue
        g_hip = dict(model.named_parameters())["audio_projection.weight"].grad.float().flatten()
        g_ref = eager.W["audio_projection.weight"].grad.float().flatten()
        cos = float(torch.dot(g_hip, g_ref) / (g_hip.norm() * g_ref.norm()))
        samples = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                samples[k].append(_time(fn, a.iters))
        ops.start_event_timing()
        fns["hip_train" if a.train else "hip_backward"]()
        torch.cuda.synchronize()
        ev = ops.stop_event_timing()
        row = dict(B=B, T=T)
        if not a.train:          # (with --train the two sides draw unrelated dropout masks: their gradients are not comparable)
            row["cos_grad_audio_projection"] = round(cos, 5)
        for k, v in samples.items():
            row[f"{k}_ms_median"], row[f"{k}_ms_min"] = round(statistics.median(v), 4), round(min(v), 4)
        row["eager_over_hip"] = round(row["eager_backward_ms_median"] / row["hip_train_ms_median" if a.train else "hip_backward_ms_median"], 3)
        if a.train:
            row["train_over_eval_stats"] = round(row["hip_train_ms_median"] / row["hip_backward_ms_median"], 3)
        row["event_ms_by_label"] = {k: (v.get("launches"), round(v.get("ms", 0.0), 3)) for k, v in sorted(ev.items()) if v.get("ms")}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.profile_only:
        return
    path = os.path.join(ROOT, "profiles", "dctcn_train.json" if a.train else "dctcn_backward.json") if a.out.endswith("dctcn_eval.json") else a.out
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["timing"] = dict(mode="train_stats=True, dropout on; eager in .train()" if a.train else "eval statistics", what="DC-TCN back-end + heads, forward and backward: features in, all gradients out; HIP vs torch eager bf16 autograd of the "
                              "same modules, same process, alternating rounds (event_ms_by_label: device events around host calls, not kernel times)",
                         device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, rows=rows)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def step_leg(a) -> None:
    """The whole training step at 88 x 88: dctcn_train.DCTCNTrainStep (mixup lam fixed, dropout on, clip, OneCycle AdamW) beside torch eager
    bf16 autograd of the same model in .train() + clip_grad_norm_ + torch.optim.AdamW + OneCycleLR, alternating rounds.  Merges "timing"
    into profiles/dctcn_step.json (the file also holds the bf16 floor of the tests): the commit, both medians, and the share of the step
    the optimiser launches take (device events around the host calls: dispatch gaps included, an upper bound of the kernel time)."""
    from syncvsr_amd import ops
    from syncvsr_amd.dctcn import DCTCNLightningModule
    from syncvsr_amd.dctcn_init import dctcn_dims, dctcn_init_state_dict, dctcn_synthetic_batch, default_dctcn_config
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    dev = torch.device("cuda:0")
    cfg = default_dctcn_config(data__input_size=88, train__gradient_clip_val=1.0)
    sd = dctcn_init_state_dict(cfg, seed=0)
    total = 3 * (a.rounds * a.iters + 16)          # more steps than the run takes: the schedule never ends under the timer
    lam, T, rows = 0.2, a.frames, []
    for B in [int(v) for v in a.batches.split(",")]:
        model = DCTCNLightningModule(cfg)
        model.load_state_dict(sd)
        model.to(dev).eval()
        ts = DCTCNTrainStep(model, total, seed=1)
        eager = EagerDCTCN(sd, dctcn_dims(cfg), dev)
        eager.train = eager.train_frontend = True
        eager.p_drop = float(cfg.model.dctcn.densetcn_options.dropout)
        leaves = [v for k, v in eager.W.items() if v.is_floating_point() and "running_" not in k]
        for v in leaves:
            v.requires_grad_(True)
        decay = [v for v in leaves if v.ndim > 1]
        o = cfg.optim.optimizer
        opt = torch.optim.AdamW([{"params": decay, "weight_decay": float(o.weight_decay)}, {"params": [v for v in leaves if v.ndim <= 1], "weight_decay": 0.0}],
                                lr=1e-3, betas=tuple(float(b) for b in o.betas), eps=float(o.eps))
        sch = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=total, **dict(cfg.optim.scheduler.items()))
        batch = [t.to(dev) for t in dctcn_synthetic_batch(cfg, B, T, size=88, seed=B)]
        videos, tokens, labels, wm, am = batch
        A, V = model.audio_alignment, model.audio_vocab_size

        def eager_step():
            opt.zero_grad(set_to_none=True)
            v = torch.lerp(videos, videos.roll(1, 0), lam)
            logits, h = eager.backend(eager.frontend(v), wm, am, want_hidden=True)
            la = F.linear(h.transpose(1, 2), eager.W["audio_projection.weight"], eager.W["audio_projection.bias"]).reshape(-1, V).float()
            tok = tokens[:, : T * A]
            lc = torch.lerp(F.cross_entropy(logits, labels), F.cross_entropy(logits, labels.roll(1, 0)), lam)
            laud = torch.lerp(F.cross_entropy(la, tok.reshape(-1)), F.cross_entropy(la, tok.roll(1, 0).reshape(-1)), lam)
            (lc + model.lambda_audio * laud).backward()
            torch.nn.utils.clip_grad_norm_(leaves, 1.0)
            opt.step()
            sch.step()

        fns = {"hip_step": lambda: ts.step(batch, lam=lam), "eager_step": eager_step}
        for fn in fns.values():
            _time(fn, 3)
        if a.profile_only:
            continue
        samples = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                samples[k].append(_time(fn, a.iters))
        ops.start_event_timing()
        ts.step(batch, lam=lam)
        torch.cuda.synchronize()
        ev = ops.stop_event_timing()
        row = dict(B=B, T=T, size=88, lam=lam)
        for k, v in samples.items():
            row[f"{k}_ms_median"], row[f"{k}_ms_min"] = round(statistics.median(v), 4), round(min(v), 4)
        row["eager_over_hip"] = round(row["eager_step_ms_median"] / row["hip_step_ms_median"], 3)
        opt_ms = sum(v.get("ms", 0.0) for k, v in ev.items() if k in ("svsr_adamw_onecycle_step", "svsr_grad_sumsq"))
        row["optimiser_event_ms"] = round(opt_ms, 4)
        row["adamw_onecycle_event_ms"] = round(ev.get("svsr_adamw_onecycle_step", {}).get("ms", 0.0), 4)
        row["optimiser_share_of_step"] = round(opt_ms / row["hip_step_ms_median"], 4)
        row["launches"] = int(sum(v.get("launches", 0) for v in ev.values()))
        row["parameters"] = int(model.store().numel)
        row["state"] = ts.state()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.profile_only:
        return
    path = os.path.join(ROOT, "profiles", "dctcn_step.json") if a.out.endswith("dctcn_eval.json") else a.out
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    commit, dirty = _commit(a)
    doc["timing"] = dict(what="DC-TCN whole training step (mixup, front-end + back-end forward and backward on batch statistics, dropout, clip 1.0, "
                              "OneCycle AdamW) at 88 x 88: dctcn_train.DCTCNTrainStep vs torch eager bf16 autograd + torch.optim.AdamW + OneCycleLR of "
                              "the same model, same process, alternating rounds (event ms: device events around host calls, not kernel times)",
                         commit=commit, dirty=dirty, device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, rows=rows)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def _commit(a):
    """(commit, dirty) of the tree: --commit / --dirty, else git's word."""
    import subprocess

    commit, dirty = a.commit, (True if a.dirty else None)
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
            if commit is not None:
                dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True, text=True).stdout.strip())
        except OSError:
            commit = None
    return commit, dirty


def step_dp_launch(a) -> None:
    """--step --gpus N: N ranks of step_dp_leg under torch.distributed.run, in a fresh child (this process never opens the GPU)."""
    import subprocess

    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1", f"--nproc_per_node={a.gpus}", os.path.abspath(__file__),
           "--step", "--dp-rank", "--gpus", str(a.gpus), "--accumulate", str(a.accumulate), "--batches", a.batches, "--frames", str(a.frames),
           "--rounds", str(a.rounds), "--iters", str(a.iters), "--bucket-mb", str(a.bucket_mb), "--out", a.out]
    if a.commit is not None:
        cmd += ["--commit", a.commit]
    if a.dirty:
        cmd.append("--dirty")
    raise SystemExit(subprocess.run(cmd, cwd=ROOT).returncode)


def step_dp_leg(a) -> None:
    """The training step with a reducer attached and / or gradient accumulation, HIP only (no eager twin: step_leg has it).  As a rank
    of --gpus N (one GPU per rank, the RCCL group bound to it with device_id=; N = 1: always_reduce) or, without a process group, as
    the --accumulate M leg of one process.  A timed "step" is one optimiser step: M micro-steps of B clips each per rank.  Per batch size:
    the median over rounds of the mean of --iters steps (wall clock between device synchronisations, warm-up first), the median time the
    main stream waited at the reducer's join (dp.exposed_ms) and the buckets of a step (dp.bucket_times; medians, measured in a pass of
    their own so that the events stay out of the step time), and last_reduce.  Rank 0 merges the row into profiles/dctcn_step_dp.json."""
    import platform

    import torch.distributed as dist

    from syncvsr_amd.dctcn import DCTCNLightningModule
    from syncvsr_amd.dctcn_init import dctcn_init_state_dict, dctcn_synthetic_batch, default_dctcn_config
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    ranked = bool(a.dp_rank)
    rank, world, local = (int(os.environ[k]) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK")) if ranked else (0, 1, 0)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if ranked:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    cfg = default_dctcn_config(data__input_size=88, train__gradient_clip_val=1.0)
    sd = dctcn_init_state_dict(cfg, seed=0)
    M = int(a.accumulate)
    total = 3 * (a.rounds * a.iters + 64)
    lam, T, rows = 0.2, a.frames, []
    for B in [int(v) for v in a.batches.split(",")]:
        model = DCTCNLightningModule(cfg)
        model.load_state_dict(sd)
        model.to(dev).eval()
        ts = DCTCNTrainStep(model, total, seed=1, always_reduce=ranked and world == 1, bucket_mb=a.bucket_mb, accumulate=M)
        batch = [t.to(dev) for t in dctcn_synthetic_batch(cfg, B, T, size=88, seed=B + rank)]          # (a shard of its own per rank)

        def window():
            for _ in range(M):
                ts.step(batch, lam=lam)

        _time(window, 3)
        samples = [_time(window, a.iters) for _ in range(a.rounds)]
        row = dict(B_per_rank=B, T=T, size=88, lam=lam, ranks=world, accumulate=M, always_reduce=ranked and world == 1,
                   step_ms_median=round(statistics.median(samples), 4), step_ms_min=round(min(samples), 4), step_ms_rounds=[round(v, 4) for v in samples],
                   micro_step_ms_median=round(statistics.median(samples) / M, 4), measured=True)
        if ts.dp is not None:
            ts.dp.measure = True
            _time(window, min(a.iters, 16))
            row["exposed_ms"] = ts.dp.exposed_ms()
            row["bucket_times"] = ts.dp.bucket_times()
            row["last_reduce"] = ts.last_reduce
            row["bucket_mb"] = a.bucket_mb
            ts.dp.measure = False
        row["state"] = ts.state()
        rows.append(row)
        if rank == 0:
            print(json.dumps(row), flush=True)
    if ranked:
        dist.barrier()
    if rank == 0:
        path = os.path.join(ROOT, "profiles", "dctcn_step_dp.json") if a.out.endswith("dctcn_eval.json") else a.out
        doc = {}
        if os.path.exists(path):
            with open(path) as f:
                doc = json.load(f)
        commit, dirty = _commit(a)
        key = f"ranks{world}_accumulate{M}" if ranked else f"local_accumulate{M}"
        doc.setdefault("legs", {})[key] = dict(
            what="DC-TCN whole training step (dctcn_train.DCTCNTrainStep at 88 x 88, mixup, dropout, clip 1.0, OneCycle AdamW), one optimiser step = "
                 "`accumulate` micro-steps of B_per_rank clips on each of `ranks` ranks" + ("; RCCL, one GPU per rank, group bound with device_id" if ranked else "; one process, no process group, no collective"),
            commit=commit, dirty=dirty, box=platform.node(), device=torch.cuda.get_device_name(local), gpus_visible=torch.cuda.device_count(),
            gpus_used=world, rounds=a.rounds, iters=a.iters, rows=rows)
        if ranked and world == 1:
            doc["legs"][key]["note"] = ("ONE rank: the collectives run inside a 1-rank group (always_reduce), so bucket times hold no link traffic; "
                                        "no multi-GPU number exists in this file unless a ranksN leg with N > 1 says so")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if ranked:
        dist.destroy_process_group()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=0, help="--step: run the step on this many data-parallel ranks (torch.distributed.run, one GPU per "
                    "rank; 1: the 1-rank always_reduce leg) -> profiles/dctcn_step_dp.json")
    ap.add_argument("--accumulate", type=int, default=1, help="--step: windows of this many micro-steps (alone or with --gpus) -> profiles/dctcn_step_dp.json")
    ap.add_argument("--bucket-mb", type=float, default=32.0, help="--step --gpus: the reducer's bucket size")
    ap.add_argument("--dp-rank", action="store_true", help=argparse.SUPPRESS)          # set by --gpus for its ranks
    ap.add_argument("--batches", default=None, help="comma-separated batch sizes (default 96,32; with --step 32, the one recorded shape)")
    ap.add_argument("--commit", default=None, help="--step: the commit the tree was checked out from, for a run without a .git beside it")
    ap.add_argument("--dirty", action="store_true", help="--step: the tree differs from that commit (without .git the script cannot tell)")
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--peak-tflops", type=float, default=2500.0, help="dense bf16 peak of the device (MI355X: 2.5 PFLOP/s)")
    ap.add_argument("--profile-only", action="store_true", help="a few untimed forwards per shape (for a rocprofv3 run of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dctcn_eval.json"))
    ap.add_argument("--backward", action="store_true", help="the backward leg instead: features in, all back-end gradients out, HIP "
                    "(loss_and_backend_grads_from_features) against bf16 autograd of the eager modules -> profiles/dctcn_backward.json")
    ap.add_argument("--train", action="store_true", help="with --backward semantics, the training arithmetic: loss_and_backend_grads_from_features("
                    "train_stats=True, dropout_seed=...) beside eager bf16 autograd in .train() and the eval-statistics backward -> profiles/dctcn_train.json")
    ap.add_argument("--step", action="store_true", help="the whole training step (dctcn_train.DCTCNTrainStep, 88 x 88) beside eager bf16 autograd + "
                    "torch.optim.AdamW + OneCycleLR -> profiles/dctcn_step.json")
    a = ap.parse_args()
    if a.batches is None:
        a.batches = "32" if a.step else "96,32"
    if a.step and a.dp_rank:
        return step_dp_leg(a)
    if a.step and a.gpus > 0:
        return step_dp_launch(a)
    if a.step and a.accumulate > 1:
        return step_dp_leg(a)
    if a.step:
        return step_leg(a)
    if a.train:
        return backward_leg(a)
    if a.backward:
        return backward_leg(a)
    from syncvsr_amd import ops
    from syncvsr_amd.dctcn import DCTCNLightningModule, _RunningStats
    from syncvsr_amd.dctcn_init import dctcn_dims, dctcn_init_state_dict, dctcn_synthetic_batch, default_dctcn_config

    dev = torch.device("cuda:0")
    cfg = default_dctcn_config()
    sd = dctcn_init_state_dict(cfg, seed=0)
    model = DCTCNLightningModule(cfg)
    model.load_state_dict(sd)
    model.to(dev).eval()
    eager = EagerDCTCN(sd, dctcn_dims(cfg), dev)
    T, rows = a.frames, []
    for B in [int(v) for v in a.batches.split(",")]:
        videos, _, _, wm, am = [t.to(dev) for t in dctcn_synthetic_batch(cfg, B, T, seed=B)]
        st = model.store()
        C = model.dims["out_size"]

        def hip_backend(feats):
            with torch.no_grad():
                stack = model._backend(_RunningStats(model, st), feats, wm, B, T)
                h, pooled = ops.tcn_norm_pool_fwd(stack, *model._prep["norm5"], am.contiguous(), B=B, T=T, C=C)
                return ops.linear_fwd(pooled, st.s16("video_classifier.weight"), st.p32("video_classifier.bias"), rows=B, K=C, N=model.dims["classes"],
                                      x_pitch=C, out_f32=True)[0]

        with torch.no_grad():
            model.predict(videos, wm, am)                                        # builds the store and the prepared weights
            feats16 = eager.frontend(videos).contiguous()                        # one set of features for both back-ends
            feats_hip = feats16.reshape(B * T, 512).contiguous()
            ref, got = eager.backend(feats16, wm, am), hip_backend(feats_hip)
        agree = float((got - ref).norm() / ref.norm())
        fns = {
            "hip_backend": lambda: hip_backend(feats_hip),
            "eager_backend": lambda: eager.backend(feats16, wm, am),
            "hip_forward": lambda: model.predict(videos, wm, am),
            "eager_forward": lambda: eager.backend(eager.frontend(videos), wm, am),
        }
        with torch.no_grad():
            for fn in fns.values():                                              # warm-up of every shape
                _time(fn, 3)
            if a.profile_only:
                continue
            samples = {k: [] for k in fns}
            for _ in range(a.rounds):                                            # alternating: one round of each implementation in turn
                for k, fn in fns.items():
                    samples[k].append(_time(fn, a.iters))
            ops.start_event_timing()
            hip_backend(feats_hip)
            torch.cuda.synchronize()
            ev = ops.stop_event_timing()
        row = dict(B=B, T=T, backend_agreement_rel=round(agree, 5))
        for k, v in samples.items():
            row[f"{k}_ms_median"], row[f"{k}_ms_min"] = round(statistics.median(v), 4), round(min(v), 4)
        row["backend_eager_over_hip"] = round(row["eager_backend_ms_median"] / row["hip_backend_ms_median"], 3)
        row["forward_eager_over_hip"] = round(row["eager_forward_ms_median"] / row["hip_forward_ms_median"], 3)
        tc = ev.get("k_tconv", {})
        row["tconv_launches"], row["tconv_ms"], row["tconv_gflop"] = tc.get("launches"), tc.get("ms"), None if not tc else round(tc.get("flops", 0.0) / 1e9, 2)
        if tc and tc.get("ms"):
            row["tconv_tflops"] = round(tc["flops"] / (tc["ms"] * 1e-3) / 1e12, 2)
            row["tconv_share_of_bf16_peak"] = round(row["tconv_tflops"] / a.peak_tflops, 4)
        row["se_ms"], row["norm_pool_ms"] = ev.get("k_tcn_se", {}).get("ms"), ev.get("k_tcn_norm_pool", {}).get("ms")
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.profile_only:
        return
    out = dict(what="DC-TCN eval forward: HIP back-end vs torch eager bf16 from the same state dict, same process, alternating rounds",
               device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, peak_tflops=a.peak_tflops, rows=rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
