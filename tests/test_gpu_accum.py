"""Gradient accumulation in engine.TrainStep (-m gpu): `accumulate=N` against the CPU oracle's accumulated loop, eager against native
replay bit for bit, N = 1 against the plain step, resume inside a window, two data-parallel ranks against their in-process definition,
and the foreign-optimiser path with the model's "do not zero" switch.

The oracle loop is the one of tests/test_gpu_train.py with `(loss / N).backward()` accumulated over a window and clip, AdamW and the
cosine schedule once per window (Lightning 1.9 automatic optimisation with accumulate_grad_batches = N)."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

from golden_cases import build_case, build_lrs_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------
# cases: two DIFFERENT micro-batches per window (the golden batch, and the same clips rolled along B with other labels)
# ---------------------------------------------------------------------------------------------------------
def _lrw_second(cfg, batch):
    videos, tokens, labels, mask = batch
    other = (labels + 7) % int(cfg.model.bert.num_labels)
    return [videos.roll(1, 0).contiguous(), tokens.roll(1, 0).contiguous(), other, mask.roll(1, 0).contiguous()]


def _lrs_second(odim, batch):
    x, lengths, tokens, label = batch
    label = label.roll(1, 0)
    other = torch.where(label > 0, label % (odim - 2) + 1, label)          # other units, same lengths (CTC stays feasible)
    return [x.roll(1, 0).contiguous(), lengths.roll(1, 0).contiguous(), tokens.roll(1, 0).contiguous(), other.contiguous()]


def _lrw_case(name="lrw_tiny", lr=2e-4):
    cfg, sd, batch, training, gold = build_case(name)
    cfg.optim.optimizer.lr = lr
    cfg.optim.scheduler.num_warmup_steps = 2
    cfg.optim.scheduler.num_training_steps = 10
    batch = list(batch)
    assert batch[2].dtype == torch.int64, "hard labels"
    return cfg, sd, [batch, _lrw_second(cfg, batch)]


def _lrs_case():
    from syncvsr_amd.engine import lrs_train_config

    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny_b3")
    tcfg = lrs_train_config(optimizer__lr=5e-4, scheduler__num_warmup_steps=2, scheduler__num_training_steps=10)
    batch = list(batch)
    return args, odim, sd, tcfg, [batch, _lrs_second(odim, batch)]


def _oracle_windows(which, model_cfg, sd, micro_batches, windows, n, lr, warm, total, betas, eps, wd, clip):
    """-> (per-micro-step losses, accumulated gradient of the LAST window by name).  One optimiser step per window."""
    from oracle import lrs_oracle as OS
    from oracle import lrw_oracle as O

    names = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    sd = {k: v.clone() for k, v in sd.items()}
    for k in names:
        sd[k].requires_grad_(True)
    params = [sd[k] for k in names]
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    losses, grads = [], None
    for w in range(windows):
        for p in params:
            p.grad = None
        for j in range(n):
            stats = {}
            mb = micro_batches[(w * n + j) % len(micro_batches)]
            if which == "lrw":
                loss = O.forward(sd, model_cfg, *mb, training=True, stats_out=stats)["loss_total"]
            else:
                loss = OS.forward(sd, model_cfg, *mb, training=True, stats_out=stats)["loss"]
            (loss / n).backward()
            losses.append(loss.item())
            with torch.no_grad():
                for k, val in stats.items():
                    sd[k] = val
        with torch.no_grad():
            grads = {k: p.grad.clone() for k, p in zip(names, params)}
            gl = [p.grad for p in params]
            O.clip_grad_norm(gl, clip)
            O.adamw_step(params, gl, m, v, w + 1, O.cosine_lr(w, lr, warm, total), betas, eps, wd)
    return losses, grads


def _make(which, dev, native, n, lr=None, **kw):
    """-> (model, TrainStep, micro-batches on the device, oracle arguments)"""
    from syncvsr_amd.engine import TrainStep

    if which == "lrw":
        from syncvsr_amd.model import Model

        cfg, sd, mbs = _lrw_case(lr=2e-4 if lr is None else lr)
        model = Model(cfg)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, native=native, accumulate=n, **kw)
        opt = cfg.optim.optimizer
        oracle = ("lrw", cfg, sd, mbs, float(opt.lr), 2, 10, tuple(opt.betas), float(opt.eps), float(opt.weight_decay),
                  float(cfg.train.gradient_clip_val))
    else:
        from syncvsr_amd.lrs_model import E2E

        args, odim, sd, tcfg, mbs = _lrs_case()
        if lr is not None:
            tcfg.optimizer.lr = lr
        model = E2E(odim, args)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, tcfg, native=native, accumulate=n, **kw)
        opt = tcfg.optimizer
        oracle = ("lrs", args, sd, mbs, float(opt.lr), 2, 10, tuple(opt.betas), float(opt.eps), float(opt.weight_decay),
                  float(tcfg.trainer.gradient_clip_val))
    return model, ts, [[t.to(dev) for t in mb] for mb in mbs], oracle


def _loss(which, out) -> float:
    return (out["loss_total"] if which == "lrw" else out[0]).item()


# ---------------------------------------------------------------------------------------------------------
# 1. trajectory against the CPU oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True])
@pytest.mark.parametrize("which", ["lrw", "lrs"])
def test_windows_match_the_oracle(dev, which, native):
    """N = 2, three windows of two different micro-batches.  Per micro-step loss within 1e-2 relative of the oracle's: the bound
    tests/test_gpu_train.py holds the plain LRW trajectory to (bf16 gradients on an ill-conditioned small batch)."""
    n, windows = 2, 3
    model, ts, mbs, (kind, mcfg, sd, cpu_mbs, lr, warm, total, betas, eps, wd, clip) = _make(which, dev, native, n)
    ref, _ = _oracle_windows(kind, mcfg, sd, cpu_mbs, windows, n, lr, warm, total, betas, eps, wd, clip)
    got = []
    for i in range(windows * n):
        assert ts.state()["micro_step"] == i % n
        got.append(_loss(which, ts.step(*mbs[i % 2])))
    state = ts.state()
    print(which, "native" if native else "eager", "hip", got, "oracle", ref, state,
          "rel", [abs(a - b) / abs(b) for a, b in zip(got, ref)])
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-2 * abs(b), (got, ref)
    assert state["step"] == windows and state["micro_step"] == 0 and state["skipped_steps"] == 0
    assert got[4] < got[2] and got[5] < got[3], "the loss of each micro-batch must decrease once the learning rate is non-zero"


@pytest.mark.parametrize("native", [False, True])
@pytest.mark.parametrize("which", ["lrw", "lrs"])
def test_micro_steps_of_a_window_see_the_same_weights(dev, which, native):
    """The SAME batch in every micro-step (no dropout in these cases; BatchNorm normalises with batch statistics in training): the losses
    inside a window are bit-equal — the optimiser ran in neither — and differ from the next window's once the learning rate is non-zero."""
    n = 2
    model, ts, mbs, _ = _make(which, dev, native, n)
    losses = [_loss(which, ts.step(*mbs[0])) for _ in range(3 * n)]
    print(which, losses)
    for w in range(3):
        assert losses[2 * w] == losses[2 * w + 1], (w, losses)
    assert losses[2] != losses[4], "window 1 stepped with a non-zero learning rate: window 2 must see other weights"
    assert ts.state()["step"] == 3


# ---------------------------------------------------------------------------------------------------------
# 2. accumulated gradient against the oracle's
# ---------------------------------------------------------------------------------------------------------
def _window_gradient(dev, native=False):
    """One window (N = 2) of lrw_full_b2 at learning rate 0 -> (model, flat gradient buffer after the window, micro-batches, cfg, sd)."""
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    cfg, sd, mbs = _lrw_case("lrw_full_b2", lr=0.0)
    model = Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, cfg, native=native, accumulate=2)
    gbs = [[t.to(dev) for t in mb] for mb in mbs]
    for b in gbs:
        ts.step(*b)
    torch.cuda.synchronize()
    return model, ts, model.store().grad.clone(), gbs, cfg, sd, mbs


def test_accumulated_gradient_matches_the_oracle(dev):
    """Bounds: the per-tensor ones tests/test_gpu_model.py applies to one lrw_full_b2 batch (min cosine 0.85, median 0.995, norm ratio within
    15 % wherever the oracle's norm is not numerically zero)."""
    model, ts, grad, gbs, cfg, sd, mbs = _window_gradient(dev)
    assert ts.state()["step"] == 1
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    opt = cfg.optim.optimizer
    _, ref = _oracle_windows("lrw", cfg, sd, mbs, 1, 2, 0.0, 2, 10, tuple(opt.betas), float(opt.eps), float(opt.weight_decay),
                             float(cfg.train.gradient_clip_val))
    rows = {}
    for name, p in model.named_parameters():
        g = p.grad.detach().float().cpu().flatten()
        r = ref[name].flatten()
        rn = r.norm().item()
        rows[name] = (float(torch.dot(g, r) / (g.norm() * r.norm() + 1e-30)), float(g.norm() / (rn + 1e-30)), rn)
    live = {k: v for k, v in rows.items() if v[2] > 1e-6}
    coss = sorted((v[0], k) for k, v in live.items())
    ratios = sorted((v[1], k) for k, v in live.items())
    print("worst cosines", coss[:5], "median", coss[len(coss) // 2][0], "ratios", ratios[0], ratios[-1])
    assert coss[0][0] >= 0.85 and coss[len(coss) // 2][0] >= 0.995, (coss[:3], coss[len(coss) // 2])
    for k, v in live.items():
        assert 0.85 <= v[1] <= 1.15, (k, v)


# ---------------------------------------------------------------------------------------------------------
# 3. eager and native agree bit for bit
# ---------------------------------------------------------------------------------------------------------
def _final(model, ts):
    torch.cuda.synchronize()
    st = model.store()
    return {"parameters": st.flat.clone(), "exp_avg": ts.m.clone(), "exp_avg_sq": ts.v.clone(), "BatchNorm buffers": st.bufflat.clone(),
            "optimiser device state": ts.opt_state.clone()}


def _assert_same(a, b, what=""):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}{k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} elements differ"


def _run_schedule(make, batches, n):
    """Two windows, one extra micro-step, flush().  -> (outputs per micro-step, final state, TrainStep)"""
    model, ts = make()
    outs = []
    for i in range(2 * n + 1):
        o = ts.step(*batches[i % len(batches)])
        outs.append([v.clone() for v in (o.values() if isinstance(o, dict) else o)])
    assert ts.state()["micro_step"] == 1 and ts.state()["step"] == 2
    assert ts.flush() is True and ts.flush() is False
    assert ts.state()["micro_step"] == 0 and ts.state()["step"] == 3
    return outs, _final(model, ts), ts


def _assert_outs(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for j, (u, v) in enumerate(zip(x, y)):
            assert torch.equal(u, v), f"micro-step {i}, output {j}: eager {u.item()} native {v.item()}"


@pytest.mark.parametrize("case", ["lrw_tiny", "lrw_full_b2"])
def test_eager_and_native_agree_bit_for_bit_lrw(dev, case):
    """N = 3: two windows, one more micro-step, flush() — dropout on, two different micro-batches."""
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    cfg, sd, mbs = _lrw_case(case)
    cfg.optim.scheduler.num_warmup_steps = 1
    cfg.model.bert.hidden_dropout_prob = 0.1
    cfg.model.bert.attention_probs_dropout_prob = 0.1
    gbs = [[t.to(dev) for t in mb] for mb in mbs]

    def make(native):
        def f():
            model = Model(cfg, seed=3)
            model.load_state_dict(sd)
            model.to(dev).train()
            return model, TrainStep(model, cfg, native=native, accumulate=3)
        return f

    eager, native = _run_schedule(make(False), gbs, 3), _run_schedule(make(True), gbs, 3)
    rec = native[2]._rec
    assert rec is not None and rec.window == (0, 1) and rec.size > 100
    assert native[2]._counts[None] == [1, 6], "one list serves the first, middle and last micro-steps: recorded once, replayed six times"
    _assert_outs(eager[0], native[0])
    _assert_same(eager[1], native[1])


def test_eager_and_native_agree_bit_for_bit_layer_drop(dev):
    """The x-transformers encoder with layer_dropout > 0: layer-drop groups and window groups in one list, one mask per replay."""
    from syncvsr_amd.config import xtransformers_lrw_config
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.init import init_state_dict, synthetic_batch
    from syncvsr_amd.model import Model

    cfg = xtransformers_lrw_config(True, model__bert__depth=3, model__bert__layer_dropout=0.4, optim__scheduler__num_warmup_steps=1)
    sd = init_state_dict(cfg, seed=3, perturb_norm=True)
    gbs = [[t.to(dev) for t in synthetic_batch(cfg, 2, frames=5, size=32, seed=100 + i)] for i in range(2)]

    def make(native):
        def f():
            model = Model(cfg, seed=77)
            model.load_state_dict(sd)
            model.to(dev).train()
            return model, TrainStep(model, cfg, native=native, accumulate=3)
        return f

    eager, native = _run_schedule(make(False), gbs, 3), _run_schedule(make(True), gbs, 3)
    rec = native[2]._rec
    assert rec.layer_groups and rec.window == (6, 7) and rec.groups == 8
    assert len({int(o[0].item() * 1e6) for o in native[0]}) > 2
    _assert_outs(eager[0], native[0])
    _assert_same(eager[1], native[1])


def test_eager_and_native_agree_bit_for_bit_lrs_two_shapes(dev):
    """LRS with max_shapes=2: two batch shapes alternate INSIDE a window (N = 3: A B A | B A B | A, flush) — the gradient buffer, the
    optimiser state and the window position are shared by the two recorded lists."""
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_init import lrs_synthetic_batch
    from syncvsr_amd.lrs_model import E2E

    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny", load_golden=False)
    args.dropout_rate = 0.1
    args.transformer_attn_dropout_rate = 0.1
    gbs = []
    for T, L, seed in ((9, 4, 501), (12, 8, 502)):
        x, lengths, tokens, label = lrs_synthetic_batch(args, batch=2, t_max=T, odim=odim, size=24, seed=seed, label_len=(2, 4))
        wide = torch.full((label.size(0), 1, L), -1, dtype=label.dtype)
        wide[:, :, : label.size(2)] = label
        gbs.append([x.to(dev), lengths.to(dev), tokens.to(dev), wide.to(dev)])

    def make(native):
        def f():
            model = E2E(odim, args, seed=3)
            model.load_state_dict(sd)
            model.to(dev).train()
            kw = dict(native=True, max_shapes=2) if native else {}
            return model, TrainStep(model, lrs_train_config(scheduler__num_warmup_steps=1), accumulate=3, **kw)
        return f

    eager, native = _run_schedule(make(False), gbs, 3), _run_schedule(make(True), gbs, 3)
    shapes = native[2].recorded_shapes()
    assert len(shapes) == 2 and sorted((v["recorded"], v["replayed"]) for v in shapes.values()) == [(1, 2), (1, 3)], shapes
    _assert_outs(eager[0], native[0])
    _assert_same(eager[1], native[1])


# ---------------------------------------------------------------------------------------------------------
# 4. N = 1 is the plain step
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True])
def test_accumulate_one_is_the_plain_step(dev, native):
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    cfg, sd, mbs = _lrw_case()
    gbs = [[t.to(dev) for t in mb] for mb in mbs]

    def run(**kw):
        model = Model(cfg, seed=3)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, native=native, **kw)
        losses = [ts.step(*gbs[i % 2])["loss_total"].clone() for i in range(3)]
        assert ts.flush() is False and ts.state()["micro_step"] == 0
        assert "accum_window" not in ts.state_dict() and "accum_grad" not in ts.state_dict()
        return losses, _final(model, ts), ts

    plain, one = run(), run(accumulate=1)
    assert all(torch.equal(a, b) for a, b in zip(plain[0], one[0]))
    _assert_same(plain[1], one[1])
    assert one[2].state()["step"] == 3
    if native:
        assert one[2]._rec.window is None and one[2]._rec.groups == 0, "accumulate = 1 records today's list: no window groups"
    cfg.train["accumulate_grad_batches"] = 2           # the config key the reference's trainer reads; accumulate= overrides it
    model = Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    assert TrainStep(model, cfg).window.n == 2 and TrainStep(model, cfg, accumulate=1).window.n == 1
    with pytest.raises(NotImplementedError):
        TrainStep(model, cfg, use_graph=True)
    with pytest.raises(ValueError):
        TrainStep(model, cfg, accumulate=0)


# ---------------------------------------------------------------------------------------------------------
# 5. resume inside a window
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True])
def test_resume_mid_window_is_bit_identical(dev, native):
    """Saved after micro-step 1 of 2 (of the second window), loaded into a fresh model and TrainStep, the window is finished and one more
    is run: bit-identical to the uninterrupted run.  Natively the resumed run RECORDS in a last micro-step, which must not zero-fill."""
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    cfg, sd, mbs = _lrw_case()
    cfg.optim.scheduler.num_warmup_steps = 1
    cfg.model.bert.hidden_dropout_prob = 0.2
    gbs = [[t.to(dev) for t in mb] for mb in mbs]

    def fresh(state):
        model = Model(cfg, seed=5)
        model.load_state_dict(state)
        model.to(dev).train()
        return model, TrainStep(model, cfg, native=native, accumulate=2)

    m1, ts1 = fresh(sd)
    ref = [ts1.step(*gbs[i % 2])["loss_total"].item() for i in range(6)]
    want = _final(m1, ts1)
    m2, ts2 = fresh(sd)
    first = [ts2.step(*gbs[i % 2])["loss_total"].item() for i in range(3)]
    assert ts2.state()["micro_step"] == 1
    ckpt_model = {k: v.detach().cpu().clone() for k, v in m2.state_dict().items()}
    ckpt_opt = {k: v.cpu() for k, v in ts2.state_dict().items()}
    assert ckpt_opt["accum_window"].tolist() == [2, 1] and ckpt_opt["accum_grad"].numel() == m2.store().numel
    m3, ts3 = fresh(ckpt_model)
    ts3.load_state_dict({k: v.to(dev) for k, v in ckpt_opt.items()})
    assert ts3.state()["micro_step"] == 1
    resumed = [ts3.step(*gbs[i % 2])["loss_total"].item() for i in range(3, 6)]
    assert first + resumed == ref, (first + resumed, ref)
    assert ts3.state()["step"] == 3
    _assert_same(want, _final(m3, ts3))
    # a checkpoint taken at a window boundary keeps the plain keys, and loads
    boundary = ts3.state_dict()
    assert "accum_window" not in boundary and "accum_grad" not in boundary
    ts3.load_state_dict(boundary)
    with pytest.raises(ValueError):
        TrainStep(m3, cfg, accumulate=3).load_state_dict({k: v.to(dev) for k, v in ckpt_opt.items()})


def test_exception_abandons_the_window(dev):
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    cfg, sd, mbs = _lrw_case()
    gbs = [[t.to(dev) for t in mb] for mb in mbs]
    model = Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, cfg, accumulate=2)
    ts.step(*gbs[0])
    with pytest.raises(ValueError):
        ts.step(gbs[1][0], gbs[1][1][:, :1], gbs[1][2], gbs[1][3])            # too few audio tokens: the forward refuses
    assert ts.state()["micro_step"] == 0 and ts.state()["step"] == 0
    assert model._early_sumsq is None and not getattr(model, "_keep_grads", False)
    for b in gbs:
        ts.step(*b)
    assert ts.state()["step"] == 1


# ---------------------------------------------------------------------------------------------------------
# 6. data-parallel: two ranks on one GPU against the in-process definition
# ---------------------------------------------------------------------------------------------------------
WINDOWS = 3


def _dp_case():
    cfg, sd, batch, training, gold = build_case("lrw_tiny")
    cfg.optim.scheduler.num_warmup_steps = 1
    cfg.optim.scheduler.num_training_steps = 10
    cfg.optim.optimizer.lr = 2e-4
    batch = list(batch)
    return cfg, sd, [batch, _lrw_second(cfg, batch)]


def _shard(batch, rank, world):
    k = batch[0].shape[0] // world
    return [t[rank * k:(rank + 1) * k].contiguous() for t in batch]


def _worker():
    """One rank (spawned by the test): WINDOWS windows of two micro-steps on this rank's shards, counting the reducer's collectives."""
    import torch.distributed as dist

    sys.path.insert(0, HERE)
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    backend = os.environ["SVSR_TEST_BACKEND"]
    native = os.environ["SVSR_TEST_NATIVE"] == "1"
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, sd, mbs = _dp_case()
    model = Model(cfg, seed=100 + rank)
    if rank == 0:
        model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, cfg, bucket_mb=0.25, accumulate=2, native=native)
    mine = [[t.to(dev) for t in _shard(mb, rank, world)] for mb in mbs]
    losses, collectives = [], []
    for i in range(2 * WINDOWS):
        before = ts.dp.collectives
        o = ts.step(*mine[i % 2])
        losses.append(float(o["loss_total"].item()))
        collectives.append(ts.dp.collectives - before)
    torch.cuda.synchronize()
    st = model.store()
    torch.save({"flat": st.flat.detach().cpu(), "bufflat": st.bufflat.detach().cpu()}, os.environ["SVSR_TEST_OUT"] + f".rank{rank}.pt")
    json.dump({"rank": rank, "losses": losses, "collectives": collectives, "step": ts.state()["step"]},
              open(os.environ["SVSR_TEST_OUT"] + f".rank{rank}.json", "w"))
    dist.barrier()
    dist.destroy_process_group()


def _definition(dev):
    """Two replicas in one process, one per shard: each accumulates its two micro-batches at scale 1/2 (the model's own seeds, buffer not
    zeroed in between), the window gradients are averaged by hand as (g0 + g1) / 2, one optimiser step is applied to both, and replica 1's
    BatchNorm buffers follow replica 0's at the end of the window (DDP broadcasts buffers only before a forward that follows a
    synchronising one: not between the micro-steps of a window)."""
    from syncvsr_amd import ops
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    cfg, sd, mbs = _dp_case()
    reps = []
    for r in range(2):
        m = Model(cfg, seed=100)
        m.load_state_dict(sd)
        m.to(dev).train()
        ts = TrainStep(m, cfg, data_parallel=False)
        m.set_loss_scale(0.5)
        reps.append((m, ts, [[t.to(dev) for t in _shard(mb, r, 2)] for mb in mbs]))
    losses = [[], []]
    for _ in range(WINDOWS):
        for r, (m, ts, b) in enumerate(reps):
            for j in range(2):
                m.accumulate_into_grads(j > 0)
                o = m(*b[j])
                torch.autograd.backward((o["loss_category"], o["loss_audio"]), m.loss_seeds(dev))
                losses[r].append(float(o["loss_total"].item()))
            m.accumulate_into_grads(False)
        g = (reps[0][0].store().grad + reps[1][0].store().grad) / 2
        for m, ts, b in reps:
            st = m.store()
            st.grad.copy_(g)
            ts.adamw.sumsq(st)
            ts.adamw.apply(st)
            ops.transpose_shadows(st.flat, st.w16, st.w16t, st.table, st.n_entries)
            st.shadow_fresh = True
        reps[1][0].store().bufflat.copy_(reps[0][0].store().bufflat)
    torch.cuda.synchronize()
    for m, ts, b in reps:
        m.set_loss_scale(1.0)
    st0 = reps[0][0].store()
    return losses, st0.flat.detach().cpu(), st0.bufflat.detach().cpu()


def _run_two_ranks(native: bool):
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    base = os.path.join(tempfile.mkdtemp(prefix="svsr_accum_"), "out")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   SVSR_TEST_BACKEND=backend, SVSR_TEST_OUT=base, SVSR_TEST_NATIVE="1" if native else "0", HSA_ENABLE_IPC_MODE_LEGACY="0",
                   OMP_NUM_THREADS="4", PYTHONPATH=os.pathsep.join([ROOT, HERE, os.environ.get("PYTHONPATH", "")]))
        code = "import test_gpu_accum as t; t._worker()"
        procs.append(subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=900)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    res = [json.load(open(base + f".rank{r}.json")) for r in range(2)]
    got = [torch.load(base + f".rank{r}.pt") for r in range(2)]
    return backend, res, got


@pytest.mark.parametrize("native", [False, True])
def test_two_ranks_accumulate_like_the_definition(dev, native):
    backend, res, got = _run_two_ranks(native)
    want_losses, want_flat, want_buf = _definition(dev)
    print(backend, "ranks' losses", [r["losses"] for r in res], "definition", want_losses, "collectives", [r["collectives"] for r in res])
    for r in range(2):
        c = res[r]["collectives"]
        assert c[0::2] == [0] * WINDOWS, f"rank {r}: a gradient collective in the first micro-step of a window ({c})"
        assert c[1] >= 3 and c[1::2] == [c[1]] * WINDOWS, f"rank {r}: the last micro-step reduces the accumulated buffer bucket by bucket ({c})"
        assert res[r]["step"] == WINDOWS
        assert res[r]["losses"] == want_losses[r], (backend, r, res[r]["losses"], want_losses[r])
    assert torch.equal(got[0]["flat"], got[1]["flat"]), "the ranks' parameters diverged"
    assert torch.equal(got[0]["flat"], want_flat), f"{int((got[0]['flat'] != want_flat).sum())} parameters differ from the definition"
    assert torch.equal(got[0]["bufflat"], want_buf) and torch.equal(got[1]["bufflat"], want_buf), "running statistics do not follow rank 0"


# ---------------------------------------------------------------------------------------------------------
# 7. foreign optimiser: model(...); (loss / N).backward() with the "do not zero" switch
# ---------------------------------------------------------------------------------------------------------
def test_foreign_optimiser_accumulation_equals_the_window_buffer(dev):
    """(loss / 2).backward() twice — the switch off for the first micro-batch, on for the second — leaves in p.grad exactly what
    TrainStep(accumulate=2) accumulates (test 2's buffer): the same kernels in the same order, seeded with 0.5 and 0.5 * lambda_audio
    either way.  Without the switch the second backward zeroes the buffer first: the silent failure the switch exists for."""
    from syncvsr_amd.model import Model

    _, ts, window_grad, gbs, cfg, sd, mbs = _window_gradient(dev)
    model = Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    opt.zero_grad()
    for j, b in enumerate(gbs):
        model.accumulate_into_grads(j > 0)
        (model(*b)["loss_total"] / 2).backward()
    model.accumulate_into_grads(False)
    torch.cuda.synchronize()
    st = model.store()
    for name, p in model.named_parameters():
        o, k = st.offsets[name][0], p.numel()
        assert p.grad.data_ptr() == st.grad.data_ptr() + 4 * o
    assert torch.equal(st.grad, window_grad), f"{int((st.grad != window_grad).sum())} of {st.grad.numel()} gradient elements differ"
    opt.step()
    only_second = None
    for j, b in enumerate(gbs):                      # no switch: every backward zeroes first
        (model(*b)["loss_total"] / 2).backward()
        only_second = st.grad.clone()
    assert not torch.equal(only_second, window_grad)
