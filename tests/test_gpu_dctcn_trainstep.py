"""dctcn_train.DCTCNTrainStep on the GPU: three steps of the reference's training recipe (tiny configuration, B = 2, T = 7, 40 x 40, given
lam and seeds, total_steps = 5) against tests/dctcn_whole_restatement.py stepped by torch.optim.AdamW + OneCycleLR with timm's no-decay rule
written out (ndim <= 1 or a name ending in .bias), then what a training loop relies on: repeatable bits, a state-dict round trip, the device
input pipeline in front of the step, and an eval forward on the stepped weights and running statistics.

Two references, because one cannot do both jobs:
  * THE RESTATEMENT'S OWN TRAJECTORY (its gradients, torch's optimiser).  Bounds: those of tests/test_gpu_dctcn_whole_grads.py, compounded as
    the multi-step test of engine.TrainStep compounds its single-step bound (tests/test_gpu_train.py: ONE flat bound for every step, 1e-2
    where the single-step parity test of the same tiny case allows 6e-3, a factor 5/3, never multiplied by the step count): every loss of
    every step within 5/3 x 4 x the recorded loss floor, and the parameter UPDATE of every tensor after three steps (p - p0: the parameters
    themselves hide it behind their own size) within the single-step gradient bound of its class (4 x the floor, 2 x for the front-end).
    Every bound is asserted below 1: an update that is missing scores exactly 1, a reversed one 2.
  * TORCH'S OPTIMISER FED THE DEVICE'S OWN GRADIENTS (p.grad as the step left it).  With the gradients shared, what is left is the clip,
    AdamW, the schedule, the decay region and the moments, and the bound is the AdamW parity test's: every parameter tensor after every step
    within 1e-5 of its largest value and 1e-5 relative L2 (tests/test_gpu_kernels.py::test_adamw_clip_schedule).  The updates move a tensor
    by 1e-4 .. 1e-2 of its norm, so a missing, mis-scaled or undecayed update cannot pass."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dctcn_whole_restatement as WR  # noqa: E402
from dctcn_backward_ref import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
TOTAL, STEPS, SEED = 5, 3, 11
LAMS = (0.0, 0.3, 0.15)
CLIP = 1.0
METRICS = ("loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5")


def _case():
    cfg, dims, sd, batch = WR.whole_case(2)
    cfg.set_path("train.gradient_clip_val", CLIP)
    return cfg, dims, sd, batch


def _model(cfg, sd, dev):
    from syncvsr_amd.dctcn import DCTCNLightningModule

    m = DCTCNLightningModule(cfg)
    m.load_state_dict(sd)
    return m.to(dev).eval()


_REF: dict = {}


def _reference():
    """-> (losses per step, state dict after STEPS steps): the restatement (bf16 rounding points) under torch's optimiser and scheduler."""
    if _REF:
        return _REF["losses"], _REF["sd"]
    cfg, dims, sd, batch = _case()
    sd = {k: v.clone() for k, v in sd.items()}
    names = [n for n, v in sd.items() if v.is_floating_point() and "running_" not in n]
    params = {n: torch.nn.Parameter(sd[n].clone()) for n in names}
    no_decay = [n for n in names if params[n].ndim <= 1 or n.endswith(".bias")]          # timm's rule, written out
    o = cfg.optim.optimizer
    opt = torch.optim.AdamW([{"params": [params[n] for n in names if n not in no_decay], "weight_decay": float(o.weight_decay)},
                             {"params": [params[n] for n in no_decay], "weight_decay": 0.0}],
                            lr=1e-3, betas=tuple(float(b) for b in o.betas), eps=float(o.eps))
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=TOTAL, **{k: v for k, v in cfg.optim.scheduler.items()})
    losses = []
    for k in range(STEPS):
        out, grads, _, new_stats = WR.whole_grads(cfg, dims, sd, batch, float(cfg.optim.lambda_audio), torch.bfloat16, seed=SEED + k, lam=LAMS[k])
        losses.append({m: float(out[m]) for m in ("loss_total", "loss_category", "loss_audio")})
        for n in names:
            params[n].grad = grads[n].float()
        torch.nn.utils.clip_grad_norm_(list(params.values()), CLIP)
        opt.step()
        sch.step()
        for n in names:
            sd[n] = params[n].detach().clone()
        for n, v in new_stats.items():
            sd[n] = v.float()
        for n in sd:
            if n.endswith("num_batches_tracked"):
                sd[n] = sd[n] + 1
    _REF.update(losses=losses, sd=sd)
    return losses, sd


def _run(dev, steps=STEPS, state=None, first=0, pipeline=None, batches=None):
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    cfg, dims, sd, batch = _case()
    model = _model(cfg, sd if state is None else state["model"], dev)
    ts = DCTCNTrainStep(model, TOTAL, pipeline=pipeline, seed=SEED)
    if state is not None:
        ts.load_state_dict(state["opt"])
    args = dict(zip(("videos", "audios", "labels", "word_mask", "attention_mask"), (t.to(dev) for t in batch)))
    outs = [ts.step(args if batches is None else batches[k], lam=LAMS[k]) for k in range(first, first + steps)]
    return model, ts, outs


LOSS_COMPOUND = 1e-2 / 6e-3          # tests/test_gpu_train.py's flat multi-step bound over the single-step bound of the same tiny case


def test_three_steps_follow_the_restatement_under_torchs_optimiser():
    dev = torch.device("cuda:0")
    cfg, dims, sd0, batch = _case()
    losses, ref_sd = _reference()
    floor = WR.recorded_floor(2)
    model, ts, outs = _run(dev)
    torch.cuda.synchronize()
    assert set(outs[0]) == set(METRICS)
    s = ts.state()
    assert s["step"] == STEPS and s["error"] == 0 and s["skipped"] == 0, s
    rel = LOSS_COMPOUND * 4 * floor["loss"]
    assert rel < 1.0, rel
    for k, (out, ref) in enumerate(zip(outs, losses)):
        for m, b in ref.items():
            a, bound = float(out[m]), rel * abs(b)
            print(f"step {k} {m}: {a:.6f} vs {b:.6f} (bound {bound:.2e})")
            assert abs(a - b) <= bound, (k, m, a, b)
    assert float(outs[2]["loss_total"]) < float(outs[0]["loss_total"]), "three steps on one batch must lower its loss"
    cls = WR.classes(cfg, sd0)
    got = {n: p.detach().float().cpu() for n, p in model.named_parameters()}
    worst: dict = {}
    bad = []
    for n, c in cls.items():
        if n.endswith(".net.0.bias"):          # zero gradient on both sides: untouched by AdamW without decay
            assert torch.equal(got[n], sd0[n]), n
            continue
        bound = (2 if c.startswith("fe_") else 4) * floor[c]
        assert bound < 1.0, (c, bound)
        e = rel_l2(got[n].double() - sd0[n].double(), ref_sd[n].double() - sd0[n].double())
        worst[c] = max(worst.get(c, 0.0), e)
        if not e <= bound:
            bad.append((n, e, bound))
    print("worst relative L2 of a parameter update per class:", {c: round(v, 4) for c, v in worst.items()})
    assert not bad, bad
    # the shadows the next forward reads are the rounded parameters
    st = model.store()
    assert torch.equal(st.w16, st.flat.to(torch.bfloat16))
    lr, beta1 = ts.values(STEPS - 1)
    assert abs(s["lr"] - lr) <= 3e-7 * lr and abs(s["beta1"] - beta1) <= 3e-7 * beta1


def test_three_steps_are_torchs_optimiser_on_the_devices_gradients():
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    dev = torch.device("cuda:0")
    cfg, dims, sd0, batch = _case()
    model = _model(cfg, sd0, dev)
    ts = DCTCNTrainStep(model, TOTAL, seed=SEED)
    names = [n for n, _ in model.named_parameters()]
    params = {n: torch.nn.Parameter(sd0[n].clone()) for n in names}
    no_decay = [n for n in names if params[n].ndim <= 1 or n.endswith(".bias")]          # timm's rule, written out
    o = cfg.optim.optimizer
    opt = torch.optim.AdamW([{"params": [params[n] for n in names if n not in no_decay], "weight_decay": float(o.weight_decay)},
                             {"params": [params[n] for n in no_decay], "weight_decay": 0.0}],
                            lr=1e-3, betas=tuple(float(b) for b in o.betas), eps=float(o.eps))
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=TOTAL, **{k: v for k, v in cfg.optim.scheduler.items()})
    args = dict(zip(("videos", "audios", "labels", "word_mask", "attention_mask"), (t.to(dev) for t in batch)))
    moved_least = 1.0
    for k in range(STEPS):
        ts.step(args, lam=LAMS[k])
        torch.cuda.synchronize()
        dparams = dict(model.named_parameters())
        for n in names:          # (the step's gradients are still in the store's buffer behind its optimiser launch)
            params[n].grad = dparams[n].grad.detach().float().cpu().clone()
        assert all(bool(torch.isfinite(p.grad).all()) for p in params.values())
        gnorm = float(torch.nn.utils.clip_grad_norm_(list(params.values()), CLIP))
        assert gnorm > CLIP, "the clip must bite in this case"
        assert abs(ts.state()["gnorm"] - gnorm) <= 1e-5 * gnorm, (ts.state()["gnorm"], gnorm)
        opt.step()
        sch.step()
        worst = (0.0, 0.0, None)
        for n in names:
            g, r = dparams[n].detach().float().cpu(), params[n].detach()
            if float(params[n].grad.abs().max()) == 0.0:          # a cbcr* conv bias: no gradient, no decay, no update
                assert torch.equal(g, sd0[n]) and torch.equal(r, sd0[n]), n
                continue
            err = float((g - r).abs().max()) / (float(r.abs().max()) + 1e-30)
            l2 = rel_l2(g, r)
            worst = max(worst, (l2, err, n))
            assert err <= 1e-5 and l2 <= 1e-5, (k, n, err, l2)
            moved = rel_l2(r, sd0[n])          # how far torch's own update has carried the tensor: what a missing update would miss
            moved_least = min(moved_least, moved) if k == STEPS - 1 else moved_least
        print(f"step {k}: worst parameter tensor rel L2 {worst[0]:.3e}, max error {worst[1]:.3e} of its scale ({worst[2]})")
    print(f"after {STEPS} steps the least-moved tensor moved by {moved_least:.3e} of its norm")
    assert moved_least >= 1e-4, moved_least          # ten times the bound: no tensor's update hides inside it


def test_same_steps_twice_and_a_state_dict_round_trip_give_the_same_bits():
    dev = torch.device("cuda:0")
    ma, ta, oa = _run(dev)
    mb, tb, ob = _run(dev)
    for a, b in zip(oa, ob):
        for k in METRICS:
            assert torch.equal(a[k], b[k]), k
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
    assert torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v) and torch.equal(ta.opt_state, tb.opt_state)
    # two steps, save, restore into fresh objects, the third step
    mc, tc, oc = _run(dev, steps=2)
    state = dict(model={k: v.detach().cpu().clone() for k, v in mc.state_dict().items()}, opt={k: (v.clone() if torch.is_tensor(v) else v)
                                                                                              for k, v in tc.state_dict().items()})
    md, td, od = _run(dev, steps=1, state=state, first=2)
    for k in METRICS:
        assert torch.equal(od[0][k], oa[2][k]), k
    pd = dict(md.named_parameters())
    for n in pa:
        assert torch.equal(pa[n], pd[n]), n
    for n, b in ma.named_buffers():
        assert torch.equal(b, dict(md.named_buffers())[n]), n
    assert td.state()["step"] == 3
    with pytest.raises(ValueError):
        for _ in range(TOTAL):
            td.step(dict(zip(("videos", "audios", "labels", "word_mask", "attention_mask"), (t.to(dev) for t in _case()[3]))), lam=0.0)
    assert td.steps == TOTAL and td.state()["error"] == 0          # the host refused the step past the schedule before any launch


def test_pipeline_in_front_of_the_step_equals_its_output_fed_by_hand():
    import vq_codec_ref as VR
    from lrw_pipeline_restatement import synthetic_frames
    from syncvsr_amd.audio_codec import VqWav2VecCodec
    from syncvsr_amd.augment import DeviceDCTCNPipeline
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = _case()
    cfg.data.max_time_masks = 4          # (T = 7: the shipped 15 does not fit such a clip)
    B, T, size = 2, 7, int(cfg.data.input_size)
    frames = synthetic_frames(B, T, size, size, 31).to(dev)
    waves = VR.synthetic_waveform(B, 640 * T + 305, 8).to(dev)
    labels, bounds = batch[2].to(dev), [2, 3]

    def build():
        m = _model(cfg, sd, dev)
        m.attach_audio_codec(VqWav2VecCodec.from_state_dict(VR.seeded_model(1, False).state_dict(), VR.fairseq_args(combine_groups=False)).to(dev))
        return m

    raw = dict(frames_u8=frames, waves=waves, labels=labels, boundaries=bounds)
    np.random.seed(5)
    m1 = build()
    t1 = DCTCNTrainStep(m1, TOTAL, pipeline=DeviceDCTCNPipeline.from_config(cfg, train=True, seed=9), seed=SEED)
    o1 = t1.step(raw, lam=0.3)
    np.random.seed(5)
    m2 = build()
    fed = DeviceDCTCNPipeline.from_config(cfg, train=True, seed=9)(**raw, lam=0.3)
    out = m2.loss_and_grads(**fed, dropout_seed=SEED, lam=0.3, videos_mixed=True)
    g2 = {n: p.grad.clone() for n, p in m2.named_parameters()}
    torch.cuda.synchronize()
    for k in METRICS:
        assert torch.equal(o1[k], out[k]), k
        assert bool(torch.isfinite(out[k]))
    for n, p in m1.named_parameters():          # (the step's gradients are still in the store's buffer behind its optimiser launch)
        assert torch.equal(p.grad, g2[n]), n


def test_eval_forward_after_the_steps_runs_on_the_stepped_weights_and_statistics():
    dev = torch.device("cuda:0")
    cfg, dims, sd0, batch = _case()
    model, ts, outs = _run(dev)
    args = [t.to(dev) for t in batch]
    after = model(*args)
    torch.cuda.synchronize()
    assert model._prep is not None and model._prep["folded"]
    stepped = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    fresh = _model(cfg, stepped, dev)(*args)          # refolded from the new running statistics: the bits of a fresh module loaded with them
    for k in after:
        assert torch.equal(after[k], fresh[k]), k
    ref = WR.eval_forward(cfg, dims, stepped, batch, float(cfg.optim.lambda_audio), torch.bfloat16)
    ref64 = WR.eval_forward(cfg, dims, stepped, batch, float(cfg.optim.lambda_audio), None)
    for k in ("loss_total", "loss_category", "loss_audio"):
        a, b = float(after[k]), float(ref[k])
        bound = 4 * abs(float(ref[k]) - float(ref64[k])) + 1e-3 * abs(b)          # the eval tests' rule: the bf16 floor of the same case, with head-room
        print(f"eval {k}: {a:.6f} vs {b:.6f} (bound {bound:.2e})")
        assert abs(a - b) <= bound, (k, a, b)
    assert not torch.equal(after["loss_total"], _model(cfg, sd0, dev)(*args)["loss_total"])
