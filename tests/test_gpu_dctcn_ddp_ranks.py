"""dctcn_train.DCTCNTrainStep across data-parallel RANKS (-m gpu), in the pattern of tests/test_gpu_ddp_ranks.py: fresh child processes, one
per rank, against the definition evaluated in ONE process.

Reference: Lightning strategy="ddp" = torch DistributedDataParallel (the shipped dc-tcn-base.yaml trains on four GPUs): every rank runs
forward / backward on its shard with its own dropout seeds and mixup weight, BatchNorm statistics are per rank (no SyncBatchNorm),
gradients are averaged, every rank applies the same optimiser step, buffers follow rank 0; under accumulate_grad_batches only the last
micro-step of a window synchronises.  The definition calls DCTCNLightningModule.loss_and_grads and ops.AdamW directly (entry points whose
parity with the reference tests/test_gpu_dctcn_whole_grads.py and tests/test_gpu_dctcn_trainstep.py pin) and averages by hand as
(g0 + g1) / 2 — one rounding, the same on both sides — so every comparison is BIT FOR BIT.

With two or more GPUs the ranks run on one GPU each over RCCL (backend "nccl"); on a single-GPU box both share cuda:0 and gloo carries
the collectives — same control flow, same assertions.  The tiny configuration (T = 7, 40 x 40), B = 2 per rank, total_steps = 5, clip 1.0."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import dctcn_dp_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
BUCKET_MB = 4.0          # 1 M elements a bucket: the tiny model's 14.4 M decayed elements make ~14 buckets, three of them back-end only
CHILD_LIMIT = 420        # seconds a rank may take (it takes a few)


def _micro_batches(cfg, world: int):
    """The micro-batches of a run, whole (B = 2 per rank): whole_case's and another one, alternating."""
    B = 2 * world
    return (C.case(B)[3], C.second_batch(cfg, B))


def _seed(rank: int, accumulate: int, micro: int) -> int:
    return C.SEED + rank * C.TOTAL * accumulate + micro          # the rule dctcn_train.dropout_seed states, written out


def _worker():
    """One rank (spawned by the test): `SVSR_TEST_MICRO` micro-steps on this rank's shards."""
    import torch.distributed as dist

    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    backend, accumulate, n_micro = os.environ["SVSR_TEST_BACKEND"], int(os.environ["SVSR_TEST_ACCUM"]), int(os.environ["SVSR_TEST_MICRO"])
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, dims, sd, _ = C.case(2)
    # different seeds, and only rank 0 loads the state dict: the reducer must bring rank 0's parameters and buffers everywhere
    model = C.build_model(cfg, sd if rank == 0 else None, dev, seed=100 + rank)
    if rank != 0:          # an eval forward first: prepared copies of this rank's OWN (wrong) weights exist when the reducer arrives
        own = C.to_args(C.case(2)[3], dev)
        model.features(own["videos"], own["word_mask"])
    ts = DCTCNTrainStep(model, C.TOTAL, seed=C.SEED, bucket_mb=BUCKET_MB, accumulate=accumulate, always_reduce=world == 1)
    st = model.store()
    mbs = [C.to_args(C.shard(b, rank, world), dev) for b in _micro_batches(cfg, world)]
    rows = []
    for i in range(n_micro):
        flat0, before = st.flat.clone(), ts.dp.collectives
        o = ts.step(mbs[i % 2] if accumulate > 1 else mbs[0], lam=C.lam_of(rank, i))
        torch.cuda.synchronize()
        rows.append(dict(metrics={k: float(o[k].item()) for k in C.METRICS}, collectives=ts.dp.collectives - before,
                         params_moved=not torch.equal(st.flat, flat0), step=int(ts.state()["step"]), reduce=ts.last_reduce))
    out = {"rank": rank, "rows": rows, "skipped": int(ts.state()["skipped"]), "error": int(ts.state()["error"])}
    torch.save({"flat": st.flat.detach().cpu(), "bufflat": st.bufflat.detach().cpu()}, os.environ["SVSR_TEST_OUT"] + f".rank{rank}.pt")
    with open(os.environ["SVSR_TEST_OUT"] + f".rank{rank}.json", "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(world: int, accumulate: int, n_micro: int):
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    base = os.path.join(tempfile.mkdtemp(prefix="svsr_dctcn_ddp_"), "out")
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   SVSR_TEST_BACKEND=backend, SVSR_TEST_OUT=base, SVSR_TEST_ACCUM=str(accumulate), SVSR_TEST_MICRO=str(n_micro),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4", PYTHONPATH=os.pathsep.join([ROOT, HERE, os.environ.get("PYTHONPATH", "")]))
        code = "import test_gpu_dctcn_ddp_ranks as t; t._worker()"
        procs.append(subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=CHILD_LIMIT)[0])
    finally:
        for p in procs:          # a rank that outlived the limit (or its peer's failure) does not stay behind
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    res = [json.load(open(base + f".rank{r}.json")) for r in range(world)]
    got = [torch.load(base + f".rank{r}.pt") for r in range(world)]
    for r in res:
        assert r["skipped"] == 0 and r["error"] == 0, r
    return backend, res, got


def _definition(accumulate: int, n_windows: int):
    """Two replicas in one process: every micro-step on each rank's shard with that rank's seed and lam, the window's gradients averaged by
    hand, rank 0's running statistics copied to both, clip and AdamW on each.  -> (metrics [rank][micro-step], flat, bufflat)"""
    dev = torch.device("cuda:0")
    cfg, dims, sd, _ = C.case(2)
    whole = _micro_batches(cfg, 2)
    reps = []
    for r in range(2):
        m = C.build_model(cfg, sd, dev)
        reps.append((m, C.hand_adamw(m, cfg), [C.to_args(C.shard(b, r, 2), dev) for b in whole]))
    metrics, i = [[], []], 0
    for _ in range(n_windows):
        for pos in range(accumulate):
            for r, (m, _, mbs) in enumerate(reps):
                o = m.loss_and_grads(**(mbs[i % 2] if accumulate > 1 else mbs[0]), loss_scale=1.0 / accumulate, accumulate=pos > 0,
                                     dropout_seed=_seed(r, accumulate, i), lam=C.lam_of(r, i))
                metrics[r].append({k: float(o[k].item()) for k in C.METRICS})
            i += 1
        g = (reps[0][0].store().grad + reps[1][0].store().grad) / 2
        reps[1][0].store().bufflat.copy_(reps[0][0].store().bufflat)          # broadcast_buffers: rank 0's running statistics
        for m, adamw, _ in reps:
            m.store().grad.copy_(g)
            C.hand_optimise(m, adamw)
    torch.cuda.synchronize()
    st0, st1 = reps[0][0].store(), reps[1][0].store()
    assert torch.equal(st0.flat, st1.flat)
    return metrics, st0.flat.detach().cpu(), st0.bufflat.detach().cpu()


def _same_end(got, want_flat, want_buf) -> None:
    assert torch.equal(got[0]["flat"], got[1]["flat"]), "the ranks' parameters diverged"
    assert torch.equal(got[0]["flat"], want_flat), f"{int((got[0]['flat'] != want_flat).sum())} parameters differ from the definition"
    assert torch.equal(got[0]["bufflat"], want_buf) and torch.equal(got[1]["bufflat"], want_buf), "running statistics do not follow rank 0"


def test_two_ranks_reproduce_the_data_parallel_definition():
    backend, res, got = _run_ranks(2, 1, C.STEPS)
    want, want_flat, want_buf = _definition(1, C.STEPS)
    print(backend, "rank 0 loss_total", [row["metrics"]["loss_total"] for row in res[0]["rows"]], "definition", [m["loss_total"] for m in want[0]])
    for r in range(2):
        for k, row in enumerate(res[r]["rows"]):
            assert row["metrics"] == want[r][k], (backend, r, k, row["metrics"], want[r][k])
            red = row["reduce"]
            assert red["covered"] and red["buckets"] >= 3 and red["before_frontend"] >= 1, (r, k, red)
            assert row["collectives"] == red["buckets"] and row["params_moved"] and row["step"] == k + 1, (r, k, row)
        assert res[r]["rows"][-1]["step"] == 3
    assert want[0][0] != want[1][0], "the two shards must differ for the average to mean anything"
    _same_end(got, want_flat, want_buf)


def test_two_ranks_with_accumulation_synchronise_once_per_window():
    backend, res, got = _run_ranks(2, 2, 4)
    want, want_flat, want_buf = _definition(2, 2)
    for r in range(2):
        for i, row in enumerate(res[r]["rows"]):
            assert row["metrics"] == want[r][i], (backend, r, i, row["metrics"], want[r][i])
            if i % 2 == 0:          # the first micro-step of a window: DDP's no_sync, and nothing but gradients and statistics moves
                assert row["collectives"] == 0 and not row["params_moved"] and row["step"] == i // 2, (r, i, row)
                assert row["reduce"] == {"buckets": 0, "before_frontend": 0, "covered": False}
            else:
                red = row["reduce"]
                assert row["collectives"] == red["buckets"] >= 3 and red["covered"] and red["before_frontend"] >= 1, (r, i, row)
                assert row["params_moved"] and row["step"] == i // 2 + 1, (r, i, row)
    _same_end(got, want_flat, want_buf)


def test_one_rank_that_always_reduces_is_the_plain_step():
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    backend, res, got = _run_ranks(1, 1, C.STEPS)
    dev = torch.device("cuda:0")
    cfg, dims, sd, batch = C.case(2)
    model = C.build_model(cfg, sd, dev)
    ts = DCTCNTrainStep(model, C.TOTAL, seed=C.SEED)
    assert ts.dp is None and ts.last_reduce is None
    args = C.to_args(_micro_batches(cfg, 1)[0], dev)
    for k in range(C.STEPS):
        o = ts.step(args, lam=C.lam_of(0, k))
        assert {m: float(o[m].item()) for m in C.METRICS} == res[0]["rows"][k]["metrics"], (backend, k)
        red = res[0]["rows"][k]["reduce"]
        assert red["covered"] and red["buckets"] >= 3 and red["before_frontend"] >= 1, red
    torch.cuda.synchronize()
    assert ts.last_reduce is None
    st = model.store()
    assert torch.equal(got[0]["flat"], st.flat.cpu()) and torch.equal(got[0]["bufflat"], st.bufflat.cpu())
