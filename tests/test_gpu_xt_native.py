"""engine.TrainStep(native=True) on the `type: x-transformers` encoder with layer drop (-m gpu).

The recorded step list holds every encoder block as an op group (csrc/steplist.hip); each step draws the skipped blocks on the host where
an eager step draws them (model._xt_skips) and the replay leaves their launches out, with a pass-through copy in their place.  The
launches that remain are the ones the eager step issues, so every test compares an eager run with a native run from the same seed and
state dict, bit for bit: each step's five outputs and, at the end, parameters, running statistics and optimiser state."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _case(depth: int, p: float, **kw):
    from syncvsr_amd.config import xtransformers_lrw_config
    from syncvsr_amd.init import init_state_dict

    cfg = xtransformers_lrw_config(True, model__bert__depth=depth, model__bert__layer_dropout=p, optim__scheduler__num_warmup_steps=1, **kw)
    return cfg, init_state_dict(cfg, seed=3, perturb_norm=True)


def _batches(cfg, dev, sizes, frames=5, size=32):
    from syncvsr_amd.init import synthetic_batch

    return [[t.to(dev) for t in synthetic_batch(cfg, n, frames=frames, size=size, seed=100 + i)] for i, n in enumerate(sizes)]


def _model(cfg, sd, dev):
    from syncvsr_amd.model import Model

    m = Model(cfg, seed=77)
    m.load_state_dict(sd)
    return m.to(dev).train()


def _steps(model, ts, batches, overrides=None, probe=None) -> list:
    outs = []
    for i, b in enumerate(batches):
        if overrides is not None:
            model.layer_skip_override = None if overrides[i] is None else set(overrides[i])      # (None: the model's generator)
        outs.append({k: v.clone() for k, v in ts.step(*b).items()})
        if probe is not None:
            probe(i, ts)
    return outs


def _final(model, ts) -> dict:
    torch.cuda.synchronize()
    st = model.store()
    return {"parameters": st.flat.clone(), "running statistics": st.bufflat.clone(), "exp_avg": ts.m.clone(), "exp_avg_sq": ts.v.clone(),
            "optimiser device state": ts.opt_state.clone()}


def _run(cfg, sd, dev, batches, native: bool, overrides=None, probe=None, **kw):
    from syncvsr_amd.engine import TrainStep

    model = _model(cfg, sd, dev)
    ts = TrainStep(model, cfg, native=native, **kw)
    outs = _steps(model, ts, batches, overrides, probe)
    return outs, _final(model, ts), ts, model


def _assert_equal(eager_outs, native_outs, eager_final, native_final):
    assert len(eager_outs) == len(native_outs)
    for i, (a, b) in enumerate(zip(eager_outs, native_outs)):
        assert sorted(a) == sorted(b) and len(a) == 5
        for k in a:
            assert torch.equal(a[k], b[k]), f"step {i}: {k} eager {a[k].item()} native {b[k].item()}"
    for what in eager_final:
        x, y = eager_final[what], native_final[what]
        assert torch.equal(x, y), f"{what}: {int((x != y).sum())} elements differ between eager and native steps"


def test_no_layer_drop_depth2(dev):
    """layer_dropout = 0: the x-transformers encoder on the native path as it was, no op groups."""
    cfg, sd = _case(2, 0.0)
    batches = _batches(cfg, dev, [2] * 4)
    e_outs, e_fin, _, _ = _run(cfg, sd, dev, batches, False)
    n_outs, n_fin, ts, _ = _run(cfg, sd, dev, batches, True)
    assert ts._rec is not None and ts._rec.size > 100 and ts._rec.groups == 0 and not ts._rec.layer_groups
    _assert_equal(e_outs, n_outs, e_fin, n_fin)
    assert len({o["loss_total"].item() for o in n_outs}) == 4


# the scripted skips of test_scripted_skips (depth 3: blocks 0..5); the recording step skips blocks itself
SCRIPT = [{1, 2}, set(), {0}, {5}, {3, 4}, {2, 3}, {0, 1, 2, 3, 4, 5}, set(), {0, 5}, {4}]


def test_scripted_skips(dev):
    """A scripted layer_skip_override per step: nothing skipped, the first block, the last, two adjacent blocks, both blocks of one layer,
    all six — recorded on a step that skips two blocks.  A skipping replay issues exactly the list's launches minus the skipped groups'."""
    cfg, sd = _case(3, 0.2)
    batches = _batches(cfg, dev, [2] * len(SCRIPT))
    seen = []

    def probe(i, ts):
        rec = ts._rec
        assert rec.layer_groups and rec.groups == 6
        per_group = [rec.calls(g) for g in range(6)]
        assert all(n > 0 for n in per_group), per_group
        if i == 0:
            assert rec.skips == frozenset(SCRIPT[0])
            return
        expect = rec.calls() - sum(per_group[g] for g in SCRIPT[i])
        assert rec.last_issued == expect, (i, SCRIPT[i], rec.last_issued, expect)
        seen.append((i, rec.last_issued))

    e_outs, e_fin, _, _ = _run(cfg, sd, dev, batches, False, overrides=SCRIPT)
    n_outs, n_fin, ts, _ = _run(cfg, sd, dev, batches, True, overrides=SCRIPT, probe=probe)
    _assert_equal(e_outs, n_outs, e_fin, n_fin)
    assert len(seen) == len(SCRIPT) - 1
    full = dict(seen)[1]
    assert full == ts._rec.calls() and dict(seen)[6] < full           # nothing skipped: every launch; all six skipped: far fewer


def test_real_generator(dev):
    """layer_skip_override = None, p = 0.5: both runs draw from the model's own generator, once per step, and end in the same state."""
    cfg, sd = _case(3, 0.5)
    batches = _batches(cfg, dev, [2] * 10)
    e_outs, e_fin, _, e_model = _run(cfg, sd, dev, batches, False)
    n_outs, n_fin, ts, n_model = _run(cfg, sd, dev, batches, True)
    _assert_equal(e_outs, n_outs, e_fin, n_fin)
    assert e_model._layer_rng.getstate() == n_model._layer_rng.getstate()
    assert ts._rec.layer_groups and ts._counts[None] == [1, 9]


def test_resume(dev):
    """state_dict after 3 native steps, a fresh model and TrainStep load it and run 3 more: bit-equal to 6 uninterrupted steps."""
    from syncvsr_amd.engine import TrainStep

    cfg, sd = _case(3, 0.5)
    batches = _batches(cfg, dev, [2] * 6)
    ref_outs, ref_fin, _, ref_model = _run(cfg, sd, dev, batches, False)
    first, _, ts1, m1 = _run(cfg, sd, dev, batches[:3], True)
    ckpt_model = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    ckpt_opt = {k: v.cpu() for k, v in ts1.state_dict().items()}
    assert "layer_rng" in ckpt_opt
    del ts1, m1
    from syncvsr_amd.model import Model

    m2 = Model(cfg, seed=5)              # another seed: the generator state comes from the checkpoint
    m2.load_state_dict(ckpt_model)
    m2.to(dev).train()
    ts2 = TrainStep(m2, cfg, native=True)
    ts2.load_state_dict({k: v.to(dev) for k, v in ckpt_opt.items()})
    second = _steps(m2, ts2, batches[3:])
    fin = _final(m2, ts2)
    ref_fin["optimiser device state"] = ref_fin["optimiser device state"][:4]
    fin["optimiser device state"] = fin["optimiser device state"][:4]
    _assert_equal(ref_outs, first + second, ref_fin, fin)
    assert ref_model._layer_rng.getstate() == m2._layer_rng.getstate()


def test_two_batch_shapes(dev):
    """max_shapes = 2: batches of 2 and 3 clips interleaved under layer drop, each shape with its own list (and its own groups)."""
    cfg, sd = _case(3, 0.5)
    sizes = [2, 3, 2, 2, 3, 3, 2, 3]
    batches = _batches(cfg, dev, sizes)
    e_outs, e_fin, _, e_model = _run(cfg, sd, dev, batches, False)
    n_outs, n_fin, ts, n_model = _run(cfg, sd, dev, batches, True, max_shapes=2)
    _assert_equal(e_outs, n_outs, e_fin, n_fin)
    assert e_model._layer_rng.getstate() == n_model._layer_rng.getstate()
    shapes = ts.recorded_shapes()
    assert sorted((v["recorded"], v["replayed"]) for v in shapes.values()) == [(1, 3), (1, 3)], shapes
    assert all(e.rec.groups == 6 for _, e in ts._lists.items())


def test_shipped_shape(dev):
    """The shipped encoder (depth 12, word boundary, layer drop 0.2, ff-dropout 0.3) at B = 32, 29 x 88 x 88: 3 steps."""
    cfg, sd = _case(12, 0.2)
    batches = _batches(cfg, dev, [32] * 3, frames=29, size=88)
    overrides = [{3, 8, 17}, None, None]            # the recording step skips blocks; then the model's own generator
    e_outs, e_fin, _, e_model = _run(cfg, sd, dev, batches, False, overrides=overrides)
    n_outs, n_fin, ts, n_model = _run(cfg, sd, dev, batches, True, overrides=overrides)
    _assert_equal(e_outs, n_outs, e_fin, n_fin)
    assert e_model._layer_rng.getstate() == n_model._layer_rng.getstate() and ts._rec.groups == 24


def _reduce_case():
    """Body of test_collective_path (a process of its own: it initialises a one-rank RCCL process group)."""
    import torch.distributed as dist

    dev = torch.device("cuda:0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29563")
    cfg, sd = _case(3, 0.5)
    batches = _batches(cfg, dev, [2] * 6)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        e_outs, e_fin, e_ts, _ = _run(cfg, sd, dev, batches, False, always_reduce=True, bucket_mb=0.25)
        n_outs, n_fin, n_ts, _ = _run(cfg, sd, dev, batches, True, always_reduce=True, bucket_mb=0.25)
    finally:
        dist.destroy_process_group()
    assert n_ts._rec.segments > 2 and n_ts._rec.groups == 6
    assert len(n_ts.dp.launched) == len(e_ts.dp.launched) >= 3
    _assert_equal(e_outs, n_outs, e_fin, n_fin)
    print("XT_REDUCE_OK")


def test_collective_path(dev):
    """always_reduce (GradReducer on a one-rank RCCL group): the list's segment breaks sit between the encoder's op groups."""
    code = "import sys; sys.path.insert(0, %r); import test_gpu_xt_native as t; t._reduce_case()" % HERE
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0 and "XT_REDUCE_OK" in r.stdout, f"exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
