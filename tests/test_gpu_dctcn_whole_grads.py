"""DCTCNLightningModule.loss_and_grads on the GPU: the gradient of EVERY parameter, the metrics and every updated running statistic against
autograd of tests/dctcn_whole_restatement.py (bf16 rounding points on, as the device stores them), on the tiny configuration at B = 2 and
B = 3, T = 7, 40 x 40 (whole_case), for lam in {0, 0.3} x dropout seed in {None, 5}.

Bounds, per kind of tensor:
  * back-end, heads, grad_features, losses, running statistics: the rule of tests/test_gpu_dctcn_train_model.py — 4 x the bf16 floor of the
    tensor's class on the SAME case (profiles/dctcn_step.json "bf16_floor": the restatement's bf16 mode against its float64 run, measured on
    the CPU over the same four runs); a cbcr* conv bias cancels under batch statistics: exact zeros.
  * front-end convolution and BatchNorm gradients: the sentence-level parity test's bound for tiny clips on the same Swish front-end
    (tests/test_gpu_lrs_model.py): the median cosine over the live gradients is at least 0.97.  That test bounds no single tensor on tiny
    clips, so no existing bound fits a single front-end tensor: each lies within TWICE the recorded distance between the restatement's bf16
    mode and its float64 run for its class ("fe_conv", "fe_bn"; both figures are in profiles/dctcn_step.json).  A relative L2 of 0.3 .. 0.5
    alone would let a wrong scale through, so the same rule bounds every front-end tensor's direction and size by themselves: its cosine
    lies no further below 1, and its norm ratio no further from 1, than twice what the same two runs of the restatement show for its class
    ("shape" in the profile: cosine >= 0.94 .. 0.97, ratio within 3.6 % .. 13 %).  No tensor is exempt.
Case 2 ties the seam: loss_and_grads' back-end gradients and grad_features are the BITS of loss_and_backend_grads_from_features fed the same
training-mode features.  Case 3: clean state — repeatable bits, accumulate, an exception between forward and backward, no pending chain."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dctcn_whole_restatement as WR  # noqa: E402
from dctcn_backward_ref import backend_names, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
RUNS = list(WR.FLOOR_RUNS)
RUN_IDS = lambda r: f"seed{r['seed']}-lam{r['lam']}"          # noqa: E731
METRICS = ("loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5")


def _model(cfg, sd, dev):
    from syncvsr_amd.dctcn import DCTCNLightningModule

    m = DCTCNLightningModule(cfg)
    m.load_state_dict(sd)
    return m.to(dev).eval()


_REF: dict = {}


def _reference(B, seed, lam):
    key = (B, seed, lam)
    if key not in _REF:
        cfg, dims, sd, batch = WR.whole_case(B)
        _REF[key] = WR.whole_grads(cfg, dims, sd, batch, float(cfg.optim.lambda_audio), torch.bfloat16, seed=seed, lam=lam)
    return _REF[key]


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("B", (2, 3))
def test_every_gradient_metric_and_running_statistic(B, run):
    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = WR.whole_case(B)
    rout, rg, rgf, rstats = _reference(B, run["seed"], run["lam"])
    floor = WR.recorded_floor(B)
    model = _model(cfg, sd, dev)
    args = [t.to(dev) for t in batch]
    out = model.loss_and_grads(*args, dropout_seed=run["seed"], lam=run["lam"])
    torch.cuda.synchronize()
    assert model._w3_pending is None and not model._deferred and not model._ready_held
    # metrics
    for k in ("loss_total", "loss_category", "loss_audio"):
        a, b = float(out[k]), float(rout[k])
        print(f"B{B} {k}: {a:.6f} vs {b:.6f} (bound {4 * floor['loss'] * abs(b):.2e})")
        assert abs(a - b) <= 4 * floor["loss"] * abs(b), (k, a, b)
    assert 0.0 <= float(out["accuracy_top1"]) <= float(out["accuracy_top5"]) <= 1.0
    # running statistics: every norm, front-end included; every counter advanced once
    bufs = dict(model.named_buffers())
    assert set(rstats) == {n for n in bufs if "running_" in n}
    worst = max((rel_l2(bufs[n].double().cpu(), v), n) for n, v in rstats.items())
    print(f"B{B} running statistics: worst rel L2 {worst[0]:.3e} at {worst[1]} (bound {4 * floor['stat']:.3e})")
    assert worst[0] <= 4 * floor["stat"], worst
    assert all(int(v) == 1 for n, v in bufs.items() if n.endswith("num_batches_tracked"))
    assert model._prep is None or not model._prep["folded"]
    # gradients
    params = dict(model.named_parameters())
    cls = WR.classes(cfg, sd)
    assert set(cls) == set(params)
    bad, fe_cos = [], []
    for n, c in cls.items():
        assert params[n].grad is not None, n
        got = params[n].grad.detach().double().cpu()
        if n.endswith(".net.0.bias"):
            if float(got.abs().max()) != 0.0:
                bad.append((n, "not zero"))
            continue
        mult = 2 if c.startswith("fe_") else 4
        e = rel_l2(got, rg[n])
        print(f"B{B} {c:12s} {n}: rel L2 {e:.3e} (bound {mult * floor[c]:.3e})")
        if not e <= mult * floor[c]:
            bad.append((n, e, mult * floor[c]))
        if c.startswith("fe_"):
            cs, ratio = WR.cos_ratio(got, rg[n])
            fe_cos.append(cs)
            cos_min, dev_max = 1.0 - 2 * (1.0 - floor["shape"][c][0]), 2 * floor["shape"][c][1]
            assert cos_min > 0.9 and dev_max < 0.15, (c, cos_min, dev_max)
            print(f"B{B} {c:12s} {n}: cosine {cs:.4f} (>= {cos_min:.4f}), norm ratio {ratio:.4f} (within {dev_max:.4f} of 1)")
            if not (cs >= cos_min and abs(ratio - 1.0) <= dev_max):
                bad.append((n, "cosine / norm ratio", cs, cos_min, ratio, dev_max))
    e = rel_l2(out["grad_features"].double().cpu(), rgf)
    print(f"B{B} grad_features: rel L2 {e:.3e} (bound {4 * floor['grad_features']:.3e})")
    if not e <= 4 * floor["grad_features"]:
        bad.append(("grad_features", e))
    fe_cos.sort()
    print(f"B{B} front-end gradient cosines: min {fe_cos[0]:.4f} median {fe_cos[len(fe_cos) // 2]:.4f}")
    assert not bad, bad
    assert fe_cos[len(fe_cos) // 2] >= 0.97, fe_cos[len(fe_cos) // 2]


@pytest.mark.parametrize("run", (RUNS[0], RUNS[3]), ids=RUN_IDS)
@pytest.mark.parametrize("B", (2, 3))
def test_backend_bits_are_those_of_the_from_features_call(B, run):
    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = WR.whole_case(B)
    args = [t.to(dev) for t in batch]
    T = args[0].shape[2]
    model = _model(cfg, sd, dev)
    out = model.loss_and_grads(*args, dropout_seed=run["seed"], lam=run["lam"])
    names = backend_names(cfg)
    mine = {n: p.grad.clone() for n, p in model.named_parameters() if n in names}
    other = _model(cfg, sd, dev)
    out2 = other.loss_and_backend_grads_from_features(out["features"].clone(), B, T, *args[1:], want_input_grad=True, train_stats=True,
                                                      dropout_seed=run["seed"], lam=run["lam"])
    torch.cuda.synchronize()
    for k in METRICS + ("grad_features",):
        assert torch.equal(out[k], out2[k]), k
    for n, p in other.named_parameters():
        if n in names:
            assert torch.equal(mine[n], p.grad), n
    bo = dict(other.named_buffers())
    for n, b in model.named_buffers():
        if n.startswith("model.tcn"):
            assert torch.equal(b, bo[n]), n


def test_state_is_clean_between_calls(monkeypatch):
    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = WR.whole_case(2)
    args = [t.to(dev) for t in batch]
    kw = dict(dropout_seed=5, lam=0.3, loss_scale=0.5)

    def grads(m):
        return {n: p.grad.clone() for n, p in m.named_parameters()}

    model = _model(cfg, sd, dev)
    a = model.loss_and_grads(*args, **kw)
    ga = grads(model)
    assert model._w3_pending is None
    b = model.loss_and_grads(*args, **kw)          # two identical calls: identical bits (gradients in train mode do not read the running statistics)
    gb = grads(model)
    for k in METRICS + ("grad_features", "features"):
        assert torch.equal(a[k], b[k]), k
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    # a Python exception between forward and backward leaves the next call's bits unchanged
    real = type(model)._backward
    calls = []

    def once(self, *x, **y):
        if not calls:
            calls.append(1)
            raise RuntimeError("aborted between forward and backward")
        return real(self, *x, **y)

    monkeypatch.setattr(type(model), "_backward", once)
    with pytest.raises(RuntimeError, match="aborted"):
        model.loss_and_grads(*args, **kw)
    c = model.loss_and_grads(*args, **kw)
    gc = grads(model)
    monkeypatch.undo()
    assert model._w3_pending is None and not model._deferred
    for k in METRICS + ("grad_features",):
        assert torch.equal(a[k], c[k]), k
    for n in ga:
        assert torch.equal(ga[n], gc[n]), n


def test_accumulate_doubles_a_first_calls_gradients():
    """accumulate=True after a first call: twice the first call's gradients, within the rule of the existing accumulate test
    (tests/test_gpu_dctcn_train_model.py): 2^-22 of |base| + |g| where a gradient is one add of the finished sum, 2^-18 where a kernel adds
    its partial sums to what is there — the heads there, and here every front-end tensor too (all of model._frontend_backward's launches
    add partial sums in place)."""
    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = WR.whole_case(2)
    args = [t.to(dev) for t in batch]
    kw = dict(dropout_seed=5, lam=0.3, loss_scale=0.5)
    model = _model(cfg, sd, dev)
    model.loss_and_grads(*args, **kw)
    g = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.loss_and_grads(*args, accumulate=True, **kw)
    torch.cuda.synchronize()
    assert model._w3_pending is None
    for n, p in model.named_parameters():
        if n.endswith(".net.0.bias"):
            assert float(p.grad.abs().max()) == 0.0, n
            continue
        partial = n.startswith(("video_classifier", "audio_projection", "model.frontend3D", "model.trunk"))
        tol = (2.0 ** -18 if partial else 2.0 ** -22) * 2 * g[n].double().abs()
        err = (p.grad.double() - 2 * g[n].double()).abs()
        assert bool((err <= tol + 1e-30).all()), (n, float(err.max()), float(tol.max()))
        assert float(g[n].abs().max()) > 0.0, n
