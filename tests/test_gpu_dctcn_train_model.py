"""DCTCNLightningModule.loss_and_backend_grads(train_stats=True) on the GPU against autograd of tests/dctcn_train_restatement.py (bf16 rounding
points on, as the device stores them).

Bound, the rule of tests/test_gpu_dctcn_backward_model.py: every gradient tensor lies within 4 x the bf16 floor of its parameter class, the
floor being the TRAINING-mode one of the same case (profiles/dctcn_train.json: the restatement's bf16 mode against its fp64 mode over the
three runs made here, measured on the CPU).  Batch statistics subtract a mean that the rounding noise does not shrink with, so the floor
depends on the input's spread:
  * FROM FEATURES (loss_and_backend_grads_from_features with N(0, 1) features, spread_features): floors 0.01 .. 0.035, every bound below
    0.15 — asserted below 0.2, so a zero gradient (relative L2 1), a gradient wired to the wrong branch or a dropped term cannot pass.  This is
    the check of the backward glue: which rows feed which weight / data gradient, the halo hand-over, the gate partials, the dropout sites in
    the backward, norm5's correction, mixup of the losses.
  * FROM VIDEOS (the sub-cases' own clips through the frozen front-end): the features' spread over rows is small against their size and
    the floor is 0.1 .. 0.3 at T = 29 and about 1 at T = 7; that bound alone proves little, so the call is ALSO required to give the bits of
    the from-features call on the device's own front-end features of the mixed clips — which ties the video path to the checked one.
Losses: 4 x the relative deviation of the same two modes; running statistics: 4 x their relative L2 deviation ("loss_floor", "stat_floor")."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dctcn_train_restatement as TR  # noqa: E402
from dctcn_backward_ref import backend_names, rel_l2  # noqa: E402
from dctcn_cases import dctcn_subcase  # noqa: E402

pytestmark = pytest.mark.gpu
RUNS = list(TR.FLOOR_RUNS)
TAGS = ["wb_t29", "nowb_t7"]
RUN_IDS = lambda r: f"seed{r['seed']}-lam{r['lam']}"          # noqa: E731


def _model(cfg, sd, dev):
    from syncvsr_amd.dctcn import DCTCNLightningModule

    m = DCTCNLightningModule(cfg)
    m.load_state_dict(sd)
    return m.to(dev).eval()


_REF: dict = {}


def _reference(tag, seed, lam, from_features):
    key = (tag, seed, lam, from_features)
    if key not in _REF:
        cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
        feats = TR.spread_features(tag, batch[0].shape[0], batch[0].shape[2]) if from_features else None
        _REF[key] = TR.train_grads(cfg, dims, sd, batch, float(cfg.optim.lambda_audio), torch.bfloat16, seed=seed, lam=lam, feats=feats)
    return _REF[key]


def _check(tag, model, out, ref, cfg, floor, base=None, scale=1.0, cap=None):
    rout, rg, rgf, rstats = ref
    names = backend_names(cfg)
    params = dict(model.named_parameters())
    bad = []
    for n, c in names.items():
        got = params[n].grad.detach().double().cpu()
        if base is not None:
            got = got - base[n]
        if n.endswith(".net.0.bias"):          # cancels under batch statistics: exact zeros
            if float(got.abs().max()) != 0.0:
                bad.append((n, "not zero"))
            continue
        e = rel_l2(got, rg[n] * scale)
        print(f"{tag} {c:12s} {n}: rel L2 {e:.3e} (bound {4 * floor[c]:.3e})")
        assert cap is None or 4 * floor[c] < cap, (c, floor[c])
        if not e <= 4 * floor[c]:
            bad.append((n, e, 4 * floor[c]))
    if "grad_features" in out:
        e = rel_l2(out["grad_features"].double().cpu(), rgf * scale)
        print(f"{tag} grad_features: rel L2 {e:.3e} (bound {4 * floor['grad_features']:.3e})")
        assert cap is None or 4 * floor["grad_features"] < cap
        if not e <= 4 * floor["grad_features"]:
            bad.append(("grad_features", e))
    assert not bad, bad


def _check_losses_and_stats(tag, model, out, ref, floor):
    for k in ("loss_total", "loss_category", "loss_audio"):
        a, b = float(out[k]), float(ref[0][k])
        print(f"{tag} {k}: {a:.6f} vs {b:.6f} (bound {4 * floor['loss'] * abs(b):.2e})")
        assert abs(a - b) <= 4 * floor["loss"] * abs(b), (k, a, b)
    bufs = dict(model.named_buffers())
    for n, v in ref[3].items():
        e = rel_l2(bufs[n].double().cpu(), v)
        assert e <= 4 * floor["stat"], (n, e, 4 * floor["stat"])
    assert all(int(v) == 1 for n, v in bufs.items() if n.endswith("num_batches_tracked") and n.startswith("model.tcn"))
    assert all(int(v) == 0 for n, v in bufs.items() if n.endswith("num_batches_tracked") and not n.startswith("model.tcn"))


def _features_call(model, tag, batch, dev, **kw):
    videos, tokens, labels, wm, am = batch
    B, T = videos.shape[0], videos.shape[2]
    feats = TR.spread_features(tag, B, T).reshape(B * T, 512).contiguous().to(dev)
    return model.loss_and_backend_grads_from_features(feats, B, T, tokens.to(dev), labels.to(dev), wm.to(dev), am.to(dev), **kw)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("tag", TAGS)
def test_training_from_spread_features_gradients_losses_and_running_statistics(tag, run):
    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
    ref = _reference(tag, run["seed"], run["lam"], True)
    floor = TR.recorded_floor(tag, from_features=True)
    assert 4 * floor["stat"] < 0.02 and 4 * floor["loss"] < 0.01
    model = _model(cfg, sd, dev)
    out = _features_call(model, tag, batch, dev, want_input_grad=True, train_stats=True, dropout_seed=run["seed"], lam=run["lam"])
    torch.cuda.synchronize()
    _check_losses_and_stats(tag, model, out, ref, floor)
    _check(tag, model, out, ref, cfg, floor, cap=0.2)
    # the eval forward afterwards runs on the UPDATED statistics: the bits of a fresh module loaded with them
    args = [t.to(dev) for t in batch]
    after = model(*args)
    fresh = _model(cfg, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, dev)(*args)
    stale = _model(cfg, sd, dev)(*args)
    for k in after:
        assert torch.equal(after[k], fresh[k]), k
    assert not torch.equal(after["loss_total"], stale["loss_total"])


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("tag", TAGS)
def test_training_from_videos_is_the_from_features_call_on_the_front_ends_features(tag, run):
    from syncvsr_amd.model import _frontend_forward

    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
    ref = _reference(tag, run["seed"], run["lam"], False)
    floor = TR.recorded_floor(tag)
    kw = dict(want_input_grad=True, train_stats=True, dropout_seed=run["seed"], lam=run["lam"])
    model = _model(cfg, sd, dev)
    args = [t.to(dev) for t in batch]
    out = model.loss_and_backend_grads(*args, **kw)
    torch.cuda.synchronize()
    _check_losses_and_stats(tag, model, out, ref, floor)
    _check(tag, model, out, ref, cfg, floor)
    other = _model(cfg, sd, dev)
    v = args[0].float()
    mixed = torch.lerp(v, v.roll(1, 0), run["lam"]) if run["lam"] else v
    with torch.no_grad():
        other._prepare(other.store())          # (the bf16 shadows the front-end reads)
        feats = _frontend_forward(other, other.store(), {}, mixed.contiguous(), False)
    B, T = v.shape[0], v.shape[2]
    out2 = other.loss_and_backend_grads_from_features(feats, B, T, *args[1:], **kw)
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    po = dict(other.named_parameters())
    for n, p in model.named_parameters():
        if n in backend_names(cfg):
            assert torch.equal(p.grad, po[n].grad), n
    bo = dict(other.named_buffers())
    for n, b in model.named_buffers():
        assert torch.equal(b, bo[n]), n


@pytest.mark.parametrize("tag", TAGS)
def test_accumulate_adds_to_an_existing_grad(tag):
    """accumulate=True on a base .grad against base + the same call without accumulate (the run is deterministic).  Where a gradient is
    written by one add of the finished sum (every tensor but the two heads' weights and biases, whose kernel adds its partial sums to what is
    there) the two are equal to an fp32 rounding of the sum; the bound is 2^-22 of |base| + |g| (two roundings), 2^-18 for the heads."""
    dev = torch.device("cuda:0")
    run = RUNS[2]
    cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
    kw = dict(loss_scale=0.5, train_stats=True, dropout_seed=run["seed"], lam=run["lam"])
    plain = _model(cfg, sd, dev)
    _features_call(plain, tag, batch, dev, **kw)
    g = {n: p.grad.clone() for n, p in plain.named_parameters() if n in backend_names(cfg)}
    model = _model(cfg, sd, dev)
    model.store()          # (the parameters become views of the store here: a .grad set before would belong to the old tensors)
    gen = torch.Generator().manual_seed(1)
    base = {}
    for n, p in model.named_parameters():
        if n in g:
            base[n] = (torch.randn(p.shape, generator=gen) * float(g[n].abs().mean() + 1e-3)).to(dev)
            p.grad = base[n].clone()
    _features_call(model, tag, batch, dev, accumulate=True, **kw)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if n not in g:
            continue
        if n.endswith(".net.0.bias"):          # cancels: exact zeros without accumulate, left unchanged with it
            assert float(g[n].abs().max()) == 0.0 and torch.equal(p.grad, base[n]), n
            continue
        want = base[n].double() + g[n].double()
        tol = (2.0 ** -18 if n.startswith(("video_classifier", "audio_projection")) else 2.0 ** -22) * (base[n].double().abs() + g[n].double().abs())
        err = (p.grad.double() - want).abs()
        assert bool((err <= tol + 1e-30).all()), (n, float(err.max()), float(tol.max()))
        assert float(g[n].abs().max()) > 0.0, n


@pytest.mark.parametrize("tag", TAGS)
def test_default_arguments_keep_the_parents_path(tag):
    """train_stats=False: the metrics are forward()'s bits, the gradients those of the call without the new keywords, the buffers untouched."""
    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
    model = _model(cfg, sd, dev)
    args = [t.to(dev) for t in batch]
    fwd = model(*args)
    a = model.loss_and_backend_grads(*args, want_input_grad=True)
    ga = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    b = model.loss_and_backend_grads(*args, want_input_grad=True, train_stats=False, dropout_seed=None, lam=0.0)
    for k in fwd:
        assert torch.equal(fwd[k], a[k]) and torch.equal(a[k], b[k]), k
    assert torch.equal(a["grad_features"], b["grad_features"])
    for n, p in model.named_parameters():
        if n in ga:
            assert torch.equal(ga[n], p.grad), n
    for n, v in model.named_buffers():
        assert torch.equal(v.cpu(), sd[n].to(v.dtype)), n
    with pytest.raises(ValueError):
        model.loss_and_backend_grads(*args, dropout_seed=3)
    model.train()
    with pytest.raises(NotImplementedError):
        model(*args)
