"""engine.TrainStep(native=True, max_shapes > 1) (-m gpu): one recorded step list per batch shape, interleaved in one run.

Every list re-issues the launches the eager step issues for its shape on the same streams, against the SAME parameters, optimiser state,
BatchNorm buffers and dropout seed word — so a sequence of mixed shapes must reproduce the eager run bit for bit, whichever lists were
recorded, replayed, evicted and recorded again on the way."""
import gc
import json
import os
import socket
import subprocess
import sys
import tempfile
import weakref

import pytest
import torch

from golden_cases import build_case, build_lrs_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (frames, label width) of the three LRS shape keys; the order of the steps
SHAPES = {"A": (9, 4), "B": (12, 8), "C": (14, 12)}
ORDER = "ABACBACA"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _pad_labels(label: torch.Tensor, width: int) -> torch.Tensor:
    out = torch.full((label.size(0), 1, width), -1, dtype=label.dtype)
    out[:, :, : label.size(2)] = label
    return out


def _lrs_batch(args, odim, shape: str, seed: int, dev):
    T, L = SHAPES[shape]
    from syncvsr_amd.lrs_init import lrs_synthetic_batch

    x, lengths, tokens, label = lrs_synthetic_batch(args, batch=2, t_max=T, odim=odim, size=24, seed=seed, label_len=(2, 4))
    return [x.to(dev), lengths.to(dev), tokens.to(dev), _pad_labels(label, L).to(dev)]


def _lrs_setup(dropout: float = 0.1):
    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny", load_golden=False)
    args.dropout_rate = dropout
    args.transformer_attn_dropout_rate = dropout
    return args, odim, sd


def _run_lrs(args, odim, sd, batches, dev, **ts_kw):
    """-> (outputs per step, flat, bufflat, opt_state, TrainStep, per-step hook results)"""
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_model import E2E

    model = E2E(odim, args, seed=3)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, lrs_train_config(scheduler__num_warmup_steps=1), **ts_kw)
    outs = [[v.clone() for v in ts.step(*b)] for b in batches]
    torch.cuda.synchronize()
    st = model.store()
    return outs, st.flat.clone(), st.bufflat.clone(), ts.opt_state.clone(), ts


def _assert_equal_runs(eager, native):
    for i, (a, b) in enumerate(zip(eager[0], native[0])):
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"step {i}: output {k} eager {x.item()} native {y.item()}"
    for what, x, y in zip(("parameters", "running statistics", "optimiser state"), eager[1:4], native[1:4]):
        assert torch.equal(x, y), f"{what}: {int((x != y).sum())} elements differ between eager and native steps"


def _key(ts, batch):
    from syncvsr_amd.shape_cache import shape_key

    return shape_key(ts.model.prepare_batch(*batch))


def test_lrs_interleaved_shapes_bit_exact(dev):
    """Three keys (different frames AND label widths) in the order A B A C B A C A, dropout on: max_shapes=3 records each key once and
    replays it afterwards; every output and the final parameters / running statistics / optimiser state equal the eager run's."""
    args, odim, sd = _lrs_setup()
    batches = [_lrs_batch(args, odim, s, 100 + i, dev) for i, s in enumerate(ORDER)]
    eager = _run_lrs(args, odim, sd, batches, dev)
    native = _run_lrs(args, odim, sd, batches, dev, native=True, max_shapes=3)
    _assert_equal_runs(eager, native)
    ts = native[4]
    shapes = ts.recorded_shapes()
    assert len(shapes) == 3, list(shapes)
    for s in "ABC":
        k = _key(ts, batches[ORDER.index(s)])
        assert shapes[k]["recorded"] == 1 and shapes[k]["replayed"] == ORDER.count(s) - 1, (s, shapes[k])
        assert shapes[k]["launches"] > 100 and shapes[k]["bytes"] > 0, shapes[k]
    assert ts._rec is ts._lists.peek(_key(ts, batches[-1])).rec, "_rec must point at the list of the shape stepped last"
    assert ts.input_buffers()[0].shape == batches[-1][0].shape
    losses = [o[0].item() for o in native[0]]
    assert len(set(losses)) == len(losses), f"every step must train on its own batch: {losses}"


def test_lrs_eviction_bit_exact_and_released(dev):
    """max_shapes=2 on the same sequence: every new key evicts the least recently used list (a device synchronisation, then its tensors go
    back to the allocator) and an evicted key is recorded again when it comes back — still bit-equal to eager."""
    from syncvsr_amd.shape_cache import ShapeLRU

    args, odim, sd = _lrs_setup()
    batches = [_lrs_batch(args, odim, s, 100 + i, dev) for i, s in enumerate(ORDER)]
    eager = _run_lrs(args, odim, sd, batches, dev)

    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_model import E2E

    model = E2E(odim, args, seed=3)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, lrs_train_config(scheduler__num_warmup_steps=1), native=True, max_shapes=2)
    lru, recorded = ShapeLRU(2), {s: 0 for s in "ABC"}
    outs, checked = [], 0
    for i, (s, b) in enumerate(zip(ORDER, batches)):
        victim = None
        if s not in lru and len(lru) == 2:
            victim = lru.keys()[0]
        if s not in lru:
            recorded[s] += 1
            lru.put(s, True)
        else:
            lru.get(s)
        probe = None
        if victim is not None and recorded[victim] >= 2 and recorded[s] >= 2:     # every workspace has its final size by now
            ve = ts._lists.peek(_key(ts, batches[ORDER.index(victim)]))
            probe = (weakref.ref(ve.rec), ve.nbytes, torch.cuda.memory_allocated())
        out = ts.step(*b)
        if probe is not None:
            torch.cuda.synchronize()
            after = torch.cuda.memory_allocated()
            new_bytes = ts.recorded_shapes()[_key(ts, b)]["bytes"]
            gc.collect()
            assert probe[0]() is None, "the evicted recorder is still alive"
            # without the release the step would ADD new_bytes; with it, the evicted list's bytes come off
            assert after - probe[2] <= new_bytes - probe[1] // 2, (after - probe[2], new_bytes, probe[1])
            checked += 1
        outs.append([v.clone() for v in out])
    torch.cuda.synchronize()
    st = model.store()
    _assert_equal_runs(eager, (outs, st.flat.clone(), st.bufflat.clone(), ts.opt_state.clone()))
    assert checked >= 1
    shapes = ts.recorded_shapes()
    assert len(shapes) == 2
    for s in lru.keys():
        k = _key(ts, batches[ORDER.index(s)])
        assert shapes[k]["recorded"] == recorded[s] >= 2, (s, shapes[k], recorded)
    assert sum(recorded.values()) == 6


def test_lrs_recorded_bytes_bound(dev):
    """max_recorded_bytes: lists beyond the byte budget are evicted (never the one just recorded)."""
    args, odim, sd = _lrs_setup()
    batches = [_lrs_batch(args, odim, s, 100 + i, dev) for i, s in enumerate(ORDER)]
    eager = _run_lrs(args, odim, sd, batches, dev)
    native = _run_lrs(args, odim, sd, batches, dev, native=True, max_shapes=3, max_recorded_bytes=1)
    _assert_equal_runs(eager, native)
    assert len(native[4].recorded_shapes()) == 1


def test_lrw_short_last_batch(dev):
    """The word-level model with B = 4, 4, 3, 4: the short batch gets a list of its own; bit-equal to eager, dropout on."""
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.init import synthetic_batch
    from syncvsr_amd.model import Model

    cfg, sd, _, _, _ = build_case("lrw_tiny")
    cfg.optim.scheduler.num_warmup_steps = 1
    cfg.model.bert.hidden_dropout_prob = 0.1
    cfg.model.bert.attention_probs_dropout_prob = 0.1
    batches = [[t.to(dev) for t in synthetic_batch(cfg, batch=n, frames=5, size=24, seed=300 + i)] for i, n in enumerate((4, 4, 3, 4))]

    def run(**kw):
        model = Model(cfg, seed=3)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, **kw)
        outs = [{k: v.clone() for k, v in ts.step(*b).items()} for b in batches]
        torch.cuda.synchronize()
        st = model.store()
        return outs, st.flat.clone(), st.bufflat.clone(), ts.opt_state.clone(), ts

    eager, native = run(), run(native=True, max_shapes=2)
    for i, (a, b) in enumerate(zip(eager[0], native[0])):
        for k in a:
            assert torch.equal(a[k], b[k]), f"step {i}: {k} eager {a[k].item()} native {b[k].item()}"
    for what, x, y in zip(("parameters", "running statistics", "optimiser state"), eager[1:4], native[1:4]):
        assert torch.equal(x, y), f"{what}: {int((x != y).sum())} elements differ between eager and native steps"
    shapes = native[4].recorded_shapes()
    assert sorted((v["recorded"], v["replayed"]) for v in shapes.values()) == [(1, 0), (1, 2)], shapes


def _padded_targets(label: torch.Tensor, k: int) -> torch.Tensor:
    from syncvsr_amd.lrs_data import collate_pad

    rows = [{"target": r[0][r[0] != -1]} for r in label]
    return collate_pad(rows, pad_targets_to_multiple=k)["targets"]


# Target padding against none, one eager step each, dropout off (a dropout mask is drawn per element index, which the label width moves).
# Measured on an MI355X (3 steps of one batch, the first at lr 0): losses and accuracy bit-identical, parameters differ by at most 3.0e-8
# (relative L2 of the update 1.1e-8): the gradient reductions over the target rows change their row counts, which moves AdamW's update in its
# last bits.  Bound: 2^-22 = 2.4e-7, two ulps of a parameter of magnitude 1 (8x the measured value).
PAD_STEPS = 3
PAD_LOSS_RTOL = 1e-5
PAD_PARAM_ATOL = 2.0 ** -22


def test_target_padding(dev):
    args, odim, sd = _lrs_setup(dropout=0.0)
    x, lengths, tokens, label = [t for t in _lrs_batch(args, odim, "B", 7, torch.device("cpu"))]
    plain = label[:, :, : int((label != -1).sum(2).max())]
    padded = _padded_targets(plain, 16)
    assert padded.shape[2] == 16 and plain.shape[2] < 16
    runs = {}
    for name, lab in (("plain", plain), ("padded", padded)):
        b = [x.to(dev), lengths.to(dev), tokens.to(dev), lab.to(dev)]
        runs[name] = _run_lrs(args, odim, sd, [b] * PAD_STEPS, dev)      # (the first step runs at lr 0: warm-up of one step)
    a, p = runs["plain"], runs["padded"]
    rel = [abs(u.item() - v.item()) / max(abs(u.item()), 1e-30) for oa, op in zip(a[0], p[0]) for u, v in zip(oa[:4], op[:4])]
    flat0 = _run_lrs(args, odim, sd, [], dev)[1]
    upd_a, upd_p = a[1] - flat0, p[1] - flat0
    stats = dict(loss_rel_max=max(rel), bit_identical=all(torch.equal(u, v) for oa, op in zip(a[0], p[0]) for u, v in zip(oa, op)),
                 acc=[(oa[4].item(), op[4].item()) for oa, op in zip(a[0], p[0])], param_max_abs=float((a[1] - p[1]).abs().max()),
                 update_max_abs=float(upd_a.abs().max()), update_rel_l2=float((upd_a - upd_p).norm() / upd_a.norm()))
    print("target padding:", json.dumps(stats))
    assert stats["update_max_abs"] > 0.0, "the steps must move the parameters"
    assert max(rel) <= PAD_LOSS_RTOL, stats
    assert all(u == v for u, v in stats["acc"]), stats
    assert stats["param_max_abs"] <= PAD_PARAM_ATOL, stats
    # the padded shape under the recorded path: bit-equal to its own eager run (dropout on)
    args, odim, sd = _lrs_setup()
    seq = []
    for i in range(3):
        xs, ls, tk, lb = _lrs_batch(args, odim, "B", 20 + i, torch.device("cpu"))
        seq.append([xs.to(dev), ls.to(dev), tk.to(dev), _padded_targets(lb, 16).to(dev)])
    _assert_equal_runs(_run_lrs(args, odim, sd, seq, dev), _run_lrs(args, odim, sd, seq, dev, native=True, max_shapes=2))


def test_first_step_matches_golden(dev):
    """The first (recording) step of max_shapes=3 on the lrs_tiny golden batch against the reference's golden losses, with the tolerance of
    test_gpu_lrs_model.py for the tiny cases (5e-3 relative)."""
    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny")
    out = _run_lrs(args, odim, sd, [[t.to(dev) for t in batch]], dev, native=True, max_shapes=3)[0][0]
    for i, k in enumerate(("loss", "loss_ctc", "loss_att", "loss_audio")):
        assert abs(out[i].item() - float(gold[k])) <= 5e-3 * abs(float(gold[k])), (k, out[i].item(), float(gold[k]))


# -- two ranks on one GPU (gloo), different label widths per rank in the same steps ---------------------------------------------
RANK_STEPS = 4


def _worker():
    import torch.distributed as dist

    sys.path.insert(0, HERE)
    from syncvsr_amd.engine import TrainStep, lrs_train_config
    from syncvsr_amd.lrs_model import E2E

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    native = os.environ["SVSR_TEST_MODE"] == "native"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    args, odim, sd = _lrs_setup()
    model = E2E(odim, args, seed=3)
    model.load_state_dict(sd)
    model.to(dev).train()
    kw = dict(native=True, max_shapes=2) if native else {}
    ts = TrainStep(model, lrs_train_config(scheduler__num_warmup_steps=1), bucket_mb=0.25, **kw)
    losses = []
    for i in range(RANK_STEPS):
        shape = "A" if (i + rank) % 2 == 0 else "B"          # rank 0: A B A B, rank 1: B A B A (frames and label widths differ)
        b = _lrs_batch(args, odim, shape, 500 + 10 * i + rank, dev)
        losses.append(float(ts.step(*b)[0].item()))
    torch.cuda.synchronize()
    st = model.store()
    info = {"losses": losses, "shapes": len(ts.recorded_shapes()) if native else 0}
    torch.save({"flat": st.flat.cpu(), "bufflat": st.bufflat.cpu(), "opt": ts.opt_state.cpu()}, os.environ["SVSR_TEST_OUT"] + f".rank{rank}.pt")
    json.dump(info, open(os.environ["SVSR_TEST_OUT"] + f".rank{rank}.json", "w"))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(mode: str):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    base = os.path.join(tempfile.mkdtemp(prefix="svsr_shapes_"), "out")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   SVSR_TEST_MODE=mode, SVSR_TEST_OUT=base, OMP_NUM_THREADS="4",
                   PYTHONPATH=os.pathsep.join([ROOT, HERE, os.environ.get("PYTHONPATH", "")]))
        procs.append(subprocess.Popen([sys.executable, "-c", "import test_gpu_native_shapes as t; t._worker()"], cwd=ROOT, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        logs = [p.communicate(timeout=600)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    return [json.load(open(base + f".rank{r}.json")) for r in range(2)], [torch.load(base + f".rank{r}.pt") for r in range(2)]


def test_two_ranks_different_label_buckets(dev):
    """Under DDP the ranks may hold different shape keys in the same step: every list issues the same bucket collectives (the buckets tile
    the flat gradient buffer, whatever the shape).  Both ranks end with equal parameters, bit-equal to the same ranks run eagerly."""
    e_info, e_got = _two_ranks("eager")
    n_info, n_got = _two_ranks("native")
    for r in range(2):
        assert n_info[r]["losses"] == e_info[r]["losses"], (r, n_info[r]["losses"], e_info[r]["losses"])
        assert n_info[r]["shapes"] == 2
        for k in ("flat", "bufflat", "opt"):
            assert torch.equal(n_got[r][k], e_got[r][k]), (r, k)
    assert torch.equal(n_got[0]["flat"], n_got[1]["flat"]), "the ranks' parameters diverged"
    assert torch.equal(e_got[0]["flat"], e_got[1]["flat"])
