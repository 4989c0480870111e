"""Training-loop parity (-m gpu): three optimiser steps of engine.TrainStep (HIP; eager and HIP-graph) against the same three
steps of the CPU oracle (forward, backward, global-norm clip 1.0, AdamW, HF cosine warm-up).  Loss trajectories must agree
to 1e-2 relative (bf16 gradients on an ill-conditioned 10-frame batch); eager and graph replay must agree with each other to 1e-4."""
import pytest
import torch

from golden_cases import build_case

pytestmark = pytest.mark.gpu


def _oracle_losses(cfg, sd, batch, steps, lr, warm, total):
    from oracle import lrw_oracle as O

    names = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    sd = {k: v.clone() for k, v in sd.items()}
    for k in names:
        sd[k].requires_grad_(True)
    params = [sd[k] for k in names]
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    opt = cfg.optim.optimizer
    losses = []
    for step in range(steps):
        for p in params:
            p.grad = None
        stats = {}
        out = O.forward(sd, cfg, *batch, training=True, stats_out=stats)
        out["loss_total"].backward()
        losses.append(out["loss_total"].item())
        with torch.no_grad():
            grads = [p.grad for p in params]
            O.clip_grad_norm(grads, float(cfg.train.gradient_clip_val))
            O.adamw_step(params, grads, m, v, step + 1, O.cosine_lr(step, lr, warm, total), tuple(opt.betas), float(opt.eps),
                         float(opt.weight_decay))
            for k, val in stats.items():
                sd[k] = val
    return losses


@pytest.mark.parametrize("use_graph", [False, True])
def test_three_steps_match_oracle(use_graph):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg, sd, batch, training, gold = build_case("lrw_tiny")
    cfg.optim.optimizer.lr = 2e-4
    cfg.optim.scheduler.num_warmup_steps = 2
    cfg.optim.scheduler.num_training_steps = 10
    ref = _oracle_losses(cfg, sd, batch, 4, 2e-4, 2, 10)
    model = Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, cfg, use_graph=use_graph)
    gb = [t.to(dev) for t in batch]
    got = []
    for _ in range(4):
        out = ts.step(*gb)
        got.append(out["loss_total"].item())
    print("hip", got, "oracle", ref, ts.state())
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-2 * abs(b), (got, ref)
    assert ts.state()["step"] == 4
    assert got[3] < got[1], "the loss must decrease once the learning rate is non-zero"


def _lrs_oracle_losses(args, sd, batch, steps, tcfg):
    from oracle import lrs_oracle as OS
    from oracle import lrw_oracle as O

    names = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    sd = {k: v.clone() for k, v in sd.items()}
    for k in names:
        sd[k].requires_grad_(True)
    params = [sd[k] for k in names]
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    opt, sch = tcfg.optimizer, tcfg.scheduler
    losses = []
    for step in range(steps):
        for p in params:
            p.grad = None
        stats = {}
        out = OS.forward(sd, args, *batch, training=True, stats_out=stats)
        out["loss"].backward()
        losses.append(out["loss"].item())
        with torch.no_grad():
            grads = [p.grad for p in params]
            O.clip_grad_norm(grads, float(tcfg.trainer.gradient_clip_val))
            lr = O.cosine_lr(step, float(opt.lr), int(sch.num_warmup_steps), int(sch.num_training_steps))
            O.adamw_step(params, grads, m, v, step + 1, lr, tuple(opt.betas), float(opt.eps), float(opt.weight_decay))
            for k, val in stats.items():
                sd[k] = val
    return losses


@pytest.mark.parametrize("use_graph", [False, True])
def test_lrs_steps_match_oracle(use_graph):
    """LRS recipe (AdamW beta2 0.98, wd 0.03, clip 5.0, cosine warm-up — LRS/video/config/lrs3.yaml:66-77,97)."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from golden_cases import build_lrs_case
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny_b3")
    tcfg = lrs_train_config(optimizer__lr=5e-4, scheduler__num_warmup_steps=2, scheduler__num_training_steps=10)
    ref = _lrs_oracle_losses(args, sd, batch, 4, tcfg)
    model = E2E(odim, args)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, tcfg, use_graph=use_graph)
    gb = [t.to(dev) for t in batch]
    got = [ts.step(*gb)[0].item() for _ in range(4)]
    print("hip", got, "oracle", ref, ts.state())
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1.5e-2 * abs(b), (got, ref)
    assert ts.state()["step"] == 4
    assert got[3] < got[1]


@pytest.mark.parametrize("which", ["lrw", "lrs"])
def test_side_stream_weight_gradients_equal_inline(which):
    """The default eager step runs the weight-gradient launches on a side HIP stream.  No kernel accumulates with atomics and
    every reduction has a fixed order, so a backward pass gives bit-identical gradients whichever stream a kernel ran on:
    side-stream runs must EQUAL in-line runs exactly (a race or a missing join shows up as any difference at all)."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dev = torch.device("cuda:0")
    if which == "lrw":
        from syncvsr_amd.model import Model

        cfg, sd, batch, training, gold = build_case("lrw_full_b2")
        model = Model(cfg)
        loss_of = lambda out: out["loss_total"]
    else:
        from golden_cases import build_lrs_case
        from syncvsr_amd.lrs_model import E2E

        args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny_b3")
        model = E2E(odim, args)
        loss_of = lambda out: out[0]
    model.load_state_dict(sd)
    model.to(dev).train()
    gb = [t.to(dev) for t in batch]

    def run(side):
        model._side.enabled = model._side.enabled_small = side
        loss = loss_of(model(*gb))
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), model.store().grad.clone()

    run(False)                                   # warm-up (lazy kernel attributes, allocator)
    inline = [run(False) for _ in range(2)]
    sided = [run(True) for _ in range(3)]
    model._side.enabled = model._side.enabled_small = False
    assert torch.equal(inline[0][0], inline[1][0]) and torch.equal(inline[0][1], inline[1][1]), "in-line runs differ from each other"
    for l, g in sided:
        assert torch.equal(l, inline[0][0]), "loss differs with the side stream"
        assert torch.equal(g, inline[0][1]), f"{int((g != inline[0][1]).sum())} gradient elements differ with the side stream"


@pytest.mark.parametrize("use_graph", [False, True])
def test_training_steps_are_bit_reproducible_at_batch_32(use_graph):
    """Two runs of three optimiser steps from the same state on the benchmark batch (32 clips of 29 x 88 x 88: the shapes and
    kernel instantiations bench.py times) end in bit-identical losses, gradients, parameters and running statistics."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.init import init_state_dict, synthetic_batch
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg = default_lrw_config()
    cfg.optim.scheduler.num_warmup_steps = 1
    sd = init_state_dict(cfg, seed=0)
    batch = [t.to(dev) for t in synthetic_batch(cfg, 32, seed=1234)]

    def run():
        model = Model(cfg)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, use_graph=use_graph)
        losses = [ts.step(*batch)["loss_total"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        st = model.store()
        return torch.stack(losses), st.grad.clone(), st.flat.clone(), st.bufflat.clone()

    a, b = run(), run()
    for name, x, y in zip(("losses", "gradients", "parameters", "running statistics"), a, b):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} of {x.numel()} elements differ between two identical runs"
    assert torch.isfinite(a[0]).all() and float(a[0][2]) < float(a[0][1])


def _rccl_single_rank_case():
    """Body of test_rccl_single_rank_collective_path_equals_plain_step (runs in a process of its own)."""
    import os

    import torch.distributed as dist

    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cfg, sd, batch, training, gold = build_case("lrw_full_b2")
    cfg.optim.scheduler.num_warmup_steps = 1
    gb = [t.to(dev) for t in batch]

    def run(**kw):
        model = Model(cfg)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, **kw)
        losses = [ts.step(*gb)["loss_total"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        st = model.store()
        launched = list(ts.dp.launched) if ts.dp is not None else []
        return torch.stack(losses), st.flat.clone(), st.bufflat.clone(), launched

    plain = run()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        eager = run(always_reduce=True, bucket_mb=8.0)
        graph = run(always_reduce=True, bucket_mb=8.0, use_graph=True)
        native = run(always_reduce=True, bucket_mb=8.0, native=True)          # bench.py's default enqueue path: recorded list + collectives
        wire16 = run(always_reduce=True, bucket_mb=8.0, grad_comm_dtype=torch.bfloat16)
    finally:
        dist.destroy_process_group()
    # opt-in bf16 wire format: gradients are rounded to bf16 on the way through the collective, so the trajectory follows the plain
    # one closely but not bit for bit
    assert not torch.equal(wire16[1], plain[1])
    assert float((wire16[0] - plain[0]).abs().max()) <= 2e-3 * float(plain[0].abs().max())
    assert float((wire16[1] - plain[1]).norm() / plain[1].norm()) <= 1e-3          # measured 2.4e-4 after three AdamW steps
    assert len(eager[3]) >= 4, "the backward must have peeled several buckets off the gradient buffer"
    covered = sorted(eager[3])
    assert covered[0][0] == 0 and all(a[1] == b[0] or b[0] >= a[1] for a, b in zip(covered, covered[1:]))
    assert len(native[3]) == len(eager[3]), "the replayed step must issue the same buckets"
    for name, got in (("eager+RCCL", eager), ("graph+RCCL", graph), ("native+RCCL", native)):
        for what, x, y in zip(("losses", "parameters", "running statistics"), got, plain):
            assert torch.equal(x, y), f"{name}: {what} differ from the plain step"
    print("RCCL_CASE_OK")


def test_rccl_single_rank_collective_path_equals_plain_step():
    """The data-parallel path on ONE rank: RCCL (torch.distributed backend "nccl") all-reduces every gradient bucket on the comm
    stream while the backward still runs, parameters and BatchNorm buffers are broadcast from rank 0 — eager and captured into
    a HIP graph.  With a single rank every collective is the identity, so the results must EQUAL the plain step bit for bit.

    Runs in a process of its own: torch's ProcessGroupNCCL watchdog thread has (once in ~40 runs, and only after other tests had
    captured graphs in the same process) aborted the interpreter with hipErrorCapturedEvent while polling its events next to a HIP
    graph capture — an abort here must not take the rest of the suite with it.  One retry for exactly that signature."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_gpu_train as t; t._rccl_single_rank_case()" % here
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), os.environ.get("PYTHONPATH", "")]))
    for attempt in range(2):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env, cwd=os.path.dirname(here))
        if r.returncode == 0 and "RCCL_CASE_OK" in r.stdout:
            return
        watchdog_abort = r.returncode in (-6, 134) and "watchdog" in r.stderr and "apturing" in r.stderr
        if not (watchdog_abort and attempt == 0):
            break
    raise AssertionError(f"RCCL single-rank case failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")


def test_checkpoint_resume_lrs():
    """model.state_dict() + TrainStep.state_dict() restore a run exactly: two more steps after a resume give the same losses
    as the uninterrupted run (the tiny LRS case is bit-stable run to run)."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from golden_cases import build_lrs_case
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny_b3")
    tcfg = lrs_train_config(optimizer__lr=5e-4, scheduler__num_warmup_steps=1, scheduler__num_training_steps=10)
    gb = [t.to(dev) for t in batch]

    def fresh():
        m = E2E(odim, args)
        m.load_state_dict(sd)
        m.to(dev).train()
        return m, TrainStep(m, tcfg, use_graph=False)

    m1, ts1 = fresh()
    ref = [ts1.step(*gb)[0].item() for _ in range(4)]
    m2, ts2 = fresh()
    first = [ts2.step(*gb)[0].item() for _ in range(2)]
    ckpt_model = {k: v.detach().cpu().clone() for k, v in m2.state_dict().items()}
    ckpt_opt = {k: v.cpu() for k, v in ts2.state_dict().items()}
    m3 = E2E(odim, args)
    m3.load_state_dict(ckpt_model)
    m3.to(dev).train()
    ts3 = TrainStep(m3, tcfg, use_graph=False)
    ts3.load_state_dict({k: v.to(dev) for k, v in ckpt_opt.items()})
    resumed = [ts3.step(*gb)[0].item() for _ in range(2)]
    print("uninterrupted", ref, "resumed", first + resumed)
    assert ts3.state()["step"] == 4
    for a, b in zip(first + resumed, ref):
        assert abs(a - b) <= 2e-4 * abs(b), (first + resumed, ref)


@pytest.mark.parametrize("case", ["lrw_tiny", "lrw_full_b2"])
def test_native_step_list_equals_eager_steps(case):
    """engine.TrainStep(native=True): the first step is recorded into a native step list (csrc/steplist.hip: every launch with its
    stream, the cross-stream waits, the memsets), later steps re-issue it with one library call.  The launches are the same launches
    on the same streams, so losses, parameters, running statistics and optimiser state must EQUAL the eager steps' bit for bit —
    with dropout on (the seed word advances on the device: a missed launch would repeat a mask) and the side stream in use."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg, sd, batch, training, gold = build_case(case)
    cfg.optim.scheduler.num_warmup_steps = 1
    cfg.model.bert.hidden_dropout_prob = 0.1
    cfg.model.bert.attention_probs_dropout_prob = 0.1
    gb = [t.to(dev) for t in batch]

    def run(native):
        model = Model(cfg, seed=3)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, native=native)
        outs = [{k: v.clone() for k, v in ts.step(*gb).items()} for _ in range(4)]
        torch.cuda.synchronize()
        st = model.store()
        return outs, st.flat.clone(), st.bufflat.clone(), ts.opt_state.clone(), ts

    eager, native = run(False), run(True)
    assert native[4]._rec is not None and native[4]._rec.size > 100, "the step was not recorded"
    for i, (a, b) in enumerate(zip(eager[0], native[0])):
        for k in a:
            assert torch.equal(a[k], b[k]), f"step {i}: {k} eager {a[k].item()} native {b[k].item()}"
    for what, x, y in zip(("parameters", "running statistics", "optimiser state"), eager[1:4], native[1:4]):
        assert torch.equal(x, y), f"{what}: {int((x != y).sum())} elements differ between eager and native steps"
    losses = [o["loss_total"].item() for o in native[0]]
    assert len(set(losses)) == 4, f"the replayed steps must keep training (and drawing fresh dropout masks): {losses}"
    # a new batch of the same shape is copied into the static inputs
    ts = native[4]
    nb = [t.clone() for t in gb]
    nb[0] = nb[0] * 0.5
    out = ts.step(*nb)
    assert torch.isfinite(out["loss_total"]).item()
    with pytest.raises(ValueError):
        ts.step(nb[0][:1], nb[1][:1], nb[2][:1], nb[3][:1])


def test_checkpoint_resume_lrw_with_dropout():
    """TrainStep.state_dict() carries the dropout seed word: a resumed LRW run draws the masks the uninterrupted run draws."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg, sd, batch, training, gold = build_case("lrw_tiny")
    cfg.optim.scheduler.num_warmup_steps = 1
    cfg.model.bert.hidden_dropout_prob = 0.2
    gb = [t.to(dev) for t in batch]

    def fresh(state):
        m = Model(cfg, seed=5)
        m.load_state_dict(state)
        m.to(dev).train()
        return m, TrainStep(m, cfg)

    m1, ts1 = fresh(sd)
    ref = [ts1.step(*gb)["loss_total"].item() for _ in range(4)]
    m2, ts2 = fresh(sd)
    first = [ts2.step(*gb)["loss_total"].item() for _ in range(2)]
    ckpt_model = {k: v.detach().cpu().clone() for k, v in m2.state_dict().items()}
    ckpt_opt = {k: v.cpu() for k, v in ts2.state_dict().items()}
    m3, ts3 = fresh(ckpt_model)
    ts3.load_state_dict({k: v.to(dev) for k, v in ckpt_opt.items()})
    resumed = [ts3.step(*gb)["loss_total"].item() for _ in range(2)]
    assert first + resumed == ref, (first + resumed, ref)


@pytest.mark.gpu
def test_checkpoint_resume_lrs_with_dropout():
    """TrainStep.state_dict() carries E2E's dropout seed word too: a resumed LRS run continues the masks where the interrupted run stopped
    (the word is an integer: exact), and its losses follow the uninterrupted run within the bound of test_checkpoint_resume_lrs."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from golden_cases import build_lrs_case
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny_b3", load_golden=False)
    args.dropout_rate = 0.1
    args.transformer_attn_dropout_rate = 0.1
    tcfg = lrs_train_config(optimizer__lr=5e-4, scheduler__num_warmup_steps=1, scheduler__num_training_steps=10)
    gb = [t.to(dev) for t in batch]

    def fresh(state):
        m = E2E(odim, args)
        m.load_state_dict(state)
        m.to(dev).train()
        return m, TrainStep(m, tcfg, use_graph=False)

    m1, ts1 = fresh(sd)
    ref = [ts1.step(*gb)[0].item() for _ in range(4)]
    m2, ts2 = fresh(sd)
    first = [ts2.step(*gb)[0].item() for _ in range(2)]
    ckpt_model = {k: v.detach().cpu().clone() for k, v in m2.state_dict().items()}
    ckpt_opt = {k: v.cpu() for k, v in ts2.state_dict().items()}
    assert int(ckpt_opt["dropout_word"]) == m2.dropout_seed + 2
    m3, ts3 = fresh(ckpt_model)
    ts3.load_state_dict({k: v.to(dev) for k, v in ckpt_opt.items()})
    resumed = [ts3.step(*gb)[0].item() for _ in range(2)]
    print("uninterrupted", ref, "resumed", first + resumed)
    assert m3.rng_state()["dropout_word"] == m1.rng_state()["dropout_word"]
    for a, b in zip(first + resumed, ref):
        assert abs(a - b) <= 2e-4 * abs(b), (first + resumed, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["lrs_tiny", "lrs_tiny_b3"])
def test_lrs_native_step_list_equals_eager_steps(case):
    """The sentence-level model under engine.TrainStep(native=True): decoder / CTC targets are prepared ahead of the recorded region
    (E2E.prepare_batch; reference add_sos_eos.py:12-31 via e2e_asr_transformer.py:203-215), the loss combination and the token accuracy
    are library launches — losses, parameters, running statistics and optimiser state equal the eager steps bit for bit, dropout on."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from golden_cases import build_lrs_case
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args, odim, sd, batch, training, gold = build_lrs_case(case, load_golden=False)
    args.dropout_rate = 0.1
    args.transformer_attn_dropout_rate = 0.1
    gb = [t.to(dev) for t in batch]
    cfg = lrs_train_config(scheduler__num_warmup_steps=1)

    def run(native):
        model = E2E(odim, args, seed=3)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, native=native)
        outs = [[v.clone() for v in ts.step(*gb)] for _ in range(4)]
        torch.cuda.synchronize()
        st = model.store()
        return outs, st.flat.clone(), st.bufflat.clone(), ts.opt_state.clone(), ts

    eager, native = run(False), run(True)
    assert native[4]._rec is not None and native[4]._rec.size > 100, "the step was not recorded"
    for i, (a, b) in enumerate(zip(eager[0], native[0])):
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"step {i}: output {k} eager {x.item()} native {y.item()}"
    for what, x, y in zip(("parameters", "running statistics", "optimiser state"), eager[1:4], native[1:4]):
        assert torch.equal(x, y), f"{what}: {int((x != y).sum())} elements differ between eager and native steps"
    losses = [o[0].item() for o in native[0]]
    assert len(set(losses)) == 4, f"the replayed steps must keep training (and drawing fresh dropout masks): {losses}"
    nb = [t.clone() for t in gb]
    nb[0] = nb[0] * 0.5
    out = native[4].step(*nb)
    assert torch.isfinite(out[0]).item()
