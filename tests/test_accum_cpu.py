"""Gradient accumulation (engine.TrainStep(accumulate=N)), the parts that need no GPU: the window bookkeeping, the step-list op groups
behind it (host walk only: svsr_steplist_dry_run counts what a replay would issue, and replays below leave every CALL and MEMSET out or
are dry runs) and the reducer's no_sync behaviour over two gloo processes."""
import ctypes
import os
import socket
import subprocess
import sys
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_GROUP_OPEN, ERR_NO_GROUP, ERR_MASK_SIZE = 1001, 1003, 1004, 1005


# ---------------------------------------------------------------------------------------------------------
# window bookkeeping
# ---------------------------------------------------------------------------------------------------------
def _decisions(win, micro_steps):
    out = []
    for _ in range(micro_steps):
        p = win.plan()
        out.append((p["zero"], p["reduce"], p["optimise"]))
        win.advance()
    return out


def test_window_decisions():
    from syncvsr_amd.engine import AccumWindow

    assert _decisions(AccumWindow(1), 3) == [(True, True, True)] * 3
    assert _decisions(AccumWindow(2), 5) == [(True, False, False), (False, True, True)] * 2 + [(True, False, False)]
    first, middle, last = (True, False, False), (False, False, False), (False, True, True)
    assert _decisions(AccumWindow(3), 7) == [first, middle, last] * 2 + [first]
    with pytest.raises(ValueError):
        AccumWindow(0)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_flush_in_the_middle_of_a_window(n):
    from syncvsr_amd.engine import AccumWindow

    win = AccumWindow(n)
    assert win.flush() is False and win.pos == 0, "a flush at a window boundary does nothing"
    for done in range(1, n):
        win = AccumWindow(n)
        _decisions(win, done)
        assert win.pos == done
        assert win.flush() is True, "a partial window has an accumulated gradient to step on"
        assert win.pos == 0 and win.flush() is False
        # the micro-step after a flush starts a new window: it zero-fills
        assert win.plan()["zero"] and win.plan()["optimise"] == (n == 1)
    win = AccumWindow(n)
    _decisions(win, n)                        # a whole window: back at the boundary
    assert win.pos == 0 and win.flush() is False
    win = AccumWindow(n)
    _decisions(win, max(n - 1, 0))
    win.abort()                                # an exception inside a micro-step: the window is abandoned
    assert win.pos == 0 and win.plan()["zero"]


def test_window_position_round_trips_through_a_state_dict():
    from syncvsr_amd.engine import AccumWindow

    win = AccumWindow(3)
    assert win.state_dict() == {}, "a checkpoint taken at a window boundary keeps today's keys"
    _decisions(win, 2)
    sd = win.state_dict()
    assert sd["accum_window"].dtype == torch.int64 and sd["accum_window"].tolist() == [3, 2]
    other = AccumWindow(3)
    other.load_state_dict(sd)
    assert other.pos == 2 and other.plan() == {"zero": False, "reduce": True, "optimise": True}
    other.load_state_dict({})                  # an old checkpoint (or one taken at a boundary): the boundary
    assert other.pos == 0
    with pytest.raises(ValueError):
        AccumWindow(2).load_state_dict(sd)     # the window length is part of the position
    with pytest.raises(ValueError):
        AccumWindow(3).load_state_dict({"accum_window": torch.tensor([3, 3])})


# ---------------------------------------------------------------------------------------------------------
# step-list groups
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def steplist():
    from syncvsr_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    h = lib.svsr_steplist_create()
    yield lib, h
    assert lib.svsr_steplist_destroy(h) == 0


def _call(lib, h) -> int:
    slots = (ctypes.c_int64 * 3)(0, 1, 0)          # svsr_word_add(word, delta, stream): recorded, never issued here
    return lib.svsr_steplist_push_call(h, b"svsr_word_add", slots, 3)


def _mask(*bits):
    return (ctypes.c_uint8 * max(len(bits), 1))(*bits)


def _dry(lib, h, segment=-1):
    counts = (ctypes.c_int64 * 4)()
    assert lib.svsr_steplist_dry_run(h, segment, counts) == 0
    return list(counts)                             # [CALL, WAIT, MEMSET, COPY]


MAIN, SIDE = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)      # stream handles: recorded, never used (nothing is issued)


def _push_step(lib, h, layers=0):
    """The shape of a recorded training step under accumulation: [zero group: WAIT + MEMSET] forward (with `layers` layer-drop groups and
    their pass-through copies) backward [tail group: early sum of squares behind a WAIT] BREAK (the reducer's join) [tail group: 2 sums,
    3 AdamW ranges, a WAIT, 2 transposes].  -> (zero group, tail group, calls outside any group)."""
    zero, tail = layers, layers + 1
    plain = 0
    for g in range(layers):                          # forward halves
        assert lib.svsr_steplist_push_group(h, g) == 0
        assert _call(lib, h) == 0 and _call(lib, h) == 0
        assert lib.svsr_steplist_push_group(h, -1) == 0
        assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), 64, MAIN, g) == 0
    assert lib.svsr_steplist_push_group(h, zero) == 0
    assert lib.svsr_steplist_push_wait(h, SIDE, MAIN) == 0                  # a WAIT inside a group
    assert lib.svsr_steplist_push_memset(h, ctypes.c_void_p(4096), 0, 64, SIDE) == 0
    assert lib.svsr_steplist_push_group(h, -1) == 0
    for _ in range(4):
        assert _call(lib, h) == 0
        plain += 1
    assert lib.svsr_steplist_push_wait(h, MAIN, SIDE) == 0
    for g in reversed(range(layers)):                # backward halves: the groups are opened again
        assert lib.svsr_steplist_push_group(h, g) == 0
        assert _call(lib, h) == 0
        assert lib.svsr_steplist_push_group(h, -1) == 0
        assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), 64, MAIN, g) == 0
    assert lib.svsr_steplist_push_group(h, tail) == 0
    assert lib.svsr_steplist_push_wait(h, SIDE, MAIN) == 0
    assert _call(lib, h) == 0                         # the early sum of squares
    assert lib.svsr_steplist_push_group(h, -1) == 0
    assert _call(lib, h) == 0                         # the last weight gradient
    plain += 1
    assert lib.svsr_steplist_push_wait(h, MAIN, SIDE) == 0
    assert lib.svsr_steplist_push_break(h) == 1       # the reducer's host callback: never inside a group
    assert lib.svsr_steplist_push_group(h, tail) == 0                       # the tail group is opened a second time
    for _ in range(5):
        assert _call(lib, h) == 0
    assert lib.svsr_steplist_push_wait(h, SIDE, MAIN) == 0
    assert _call(lib, h) == 0 and _call(lib, h) == 0
    assert lib.svsr_steplist_push_group(h, -1) == 0
    return zero, tail, plain


def test_window_groups_leave_out_zero_fill_and_tail_but_no_wait(steplist):
    lib, h = steplist
    zero, tail, plain = _push_step(lib, h)
    assert (zero, tail) == (0, 1) and lib.svsr_steplist_groups(h) == 2
    assert lib.svsr_steplist_calls(h, tail) == 8 and lib.svsr_steplist_calls(h, zero) == 0 and lib.svsr_steplist_calls(h, -1) == plain + 8
    waits = 5
    assert _dry(lib, h) == [plain + 8, waits, 1, 0]                          # no mask: everything
    kinds = {"first": _mask(0, 1), "middle": _mask(1, 1), "last": _mask(1, 0)}
    want = {"first": [plain, waits, 1, 0], "middle": [plain, waits, 0, 0], "last": [plain + 8, waits, 0, 0]}
    for kind, mask in kinds.items():
        assert lib.svsr_steplist_set_skips(h, mask, 2) == 0
        assert _dry(lib, h) == want[kind], kind
        per_segment = [_dry(lib, h, 0), _dry(lib, h, 1)]
        assert [a + b for a, b in zip(*per_segment)] == want[kind], kind
        assert per_segment[1][1] == 1, "the WAIT inside the skipped tail group (segment 1) is still issued"
    # the real walk under the same mask issues nothing it should not: a middle micro-step whose remaining ops are WAITs and CALLs would
    # touch the device, so only the counters are compared here; a list of skipped groups only is run for real below
    assert lib.svsr_steplist_dry_run(h, 2, (ctypes.c_int64 * 4)()) == ERR_ARG      # no such segment
    assert lib.svsr_steplist_dry_run(h, -1, None) == ERR_ARG
    assert lib.svsr_steplist_dry_run(None, -1, (ctypes.c_int64 * 4)()) == ERR_ARG


def test_dry_run_agrees_with_the_run_it_describes(steplist):
    """A list that holds only group ops (no WAIT): with both groups skipped svsr_steplist_run issues nothing (so it runs without a device)
    and svsr_steplist_dry_run says so; the two share one walk (csrc/steplist.hip: walk<ISSUE>)."""
    lib, h = steplist
    for g in (0, 1):
        assert lib.svsr_steplist_push_group(h, g) == 0
        assert _call(lib, h) == 0
        assert lib.svsr_steplist_push_memset(h, ctypes.c_void_p(4096), 0, 64, None) == 0
        assert lib.svsr_steplist_push_group(h, -1) == 0
    assert lib.svsr_steplist_set_skips(h, _mask(1, 1), 2) == 0
    assert _dry(lib, h) == [0, 0, 0, 0]
    failed = ctypes.c_int(-1)
    assert lib.svsr_steplist_run(h, -1, ctypes.byref(failed)) == 0 and lib.svsr_steplist_last_issued(h) == 0
    assert lib.svsr_steplist_set_skips(h, _mask(0, 1), 2) == 0
    assert _dry(lib, h) == [1, 0, 1, 0]
    assert lib.svsr_steplist_last_issued(h) == 0, "a dry run issues nothing and counts nothing as issued"


def test_layer_drop_skips_and_window_skips_compose(steplist):
    lib, h = steplist
    L = 4
    zero, tail, plain = _push_step(lib, h, layers=L)
    assert (zero, tail) == (L, L + 1) and lib.svsr_steplist_groups(h) == L + 2
    waits, per_layer = 5, 3

    def expect(dropped, run_zero, run_tail):
        calls = plain + per_layer * (L - len(dropped)) + (8 if run_tail else 0)
        return [calls, waits, 1 if run_zero else 0, 2 * len(dropped)]

    for dropped in ((), (1,), (0, 3), (0, 1, 2, 3)):
        for run_zero, run_tail in ((True, False), (False, False), (False, True), (True, True)):
            bits = [1 if g in dropped else 0 for g in range(L)] + [0 if run_zero else 1, 0 if run_tail else 1]
            assert lib.svsr_steplist_set_skips(h, _mask(*bits), L + 2) == 0
            assert _dry(lib, h) == expect(dropped, run_zero, run_tail), (dropped, run_zero, run_tail)


def test_wrong_mask_sizes_and_group_errors(steplist):
    lib, h = steplist
    _push_step(lib, h, layers=2)
    assert lib.svsr_steplist_groups(h) == 4
    assert lib.svsr_steplist_set_skips(h, _mask(0, 0), 2) == ERR_MASK_SIZE          # the layer-drop mask alone is too short now
    assert lib.svsr_steplist_set_skips(h, _mask(0, 0, 0, 0, 0), 5) == ERR_MASK_SIZE
    assert lib.svsr_steplist_set_skips(h, None, 4) == ERR_ARG
    assert lib.svsr_steplist_set_skips(h, _mask(0, 0, 1, 1), 4) == 0
    assert lib.svsr_steplist_push_group(h, 3) == 0
    assert lib.svsr_steplist_push_break(h) == -ERR_GROUP_OPEN                        # the reducer's callback cannot sit inside the tail group
    assert lib.svsr_steplist_push_group(h, 2) == ERR_GROUP_OPEN
    assert lib.svsr_steplist_push_group(h, -1) == 0
    assert lib.svsr_steplist_push_group(h, -1) == ERR_NO_GROUP


def test_recorder_window_groups():
    """ops.StepRecorder / ops.window_group: the window groups sit behind the layer-drop groups, a micro-step's kind and its layer-drop draw
    go into one mask, and a recording micro-step appends the groups it leaves out without executing them."""
    from syncvsr_amd import ops

    assert isinstance(ops.window_group("tail"), type(ops.nullcontext())), "outside a recording the context does nothing"
    rec = ops.StepRecorder()
    rec.layer_groups, rec.window = True, (2, 3)
    assert rec.window_skips(True, False) == {3} and rec.window_skips(False, False) == {2, 3} and rec.window_skips(False, True) == {2}
    assert rec.window_skips(True, True) == set()
    rec.skips = frozenset({1}) | frozenset(rec.window_skips(False, True))            # a LAST micro-step records (after a resume, say)
    ops._REC = rec                                   # (what ops.recording sets, without its torch patches: nothing is launched here)
    try:
        for n in (0, 1):
            with rec.group(n):
                assert rec.append_only == (n == 1)
                rec.call("svsr_word_add", (0, 1, 0))
        with ops.window_group("zero"):
            assert rec.append_only, "a micro-step that is not the first must not execute the zero-fill it records"
            rec.memset(4096, 0, 64, 0)
        with ops.window_group("tail"):
            assert not rec.append_only
            rec.call("svsr_word_add", (0, 1, 0))
        rec.add_callback(lambda: None)
        with ops.window_group("tail"):               # opened again behind the reducer's break
            rec.call("svsr_word_add", (0, 1, 0))
        with pytest.raises(ValueError):
            ops.window_group("middle")
    finally:
        ops._REC = None
    assert rec.groups == 4 and rec.calls(3) == 2 and rec.calls(2) == 0 and rec.segments == 2
    rec.set_skips({0} | rec.window_skips(True, False))
    assert rec.would_issue() == {"calls": 1, "waits": 0, "memsets": 1, "copies": 0}
    rec.set_skips(rec.window_skips(False, False))
    assert rec.would_issue() == {"calls": 2, "waits": 0, "memsets": 0, "copies": 0}
    rec.set_skips(rec.window_skips(False, True))
    assert rec.would_issue() == {"calls": 4, "waits": 0, "memsets": 0, "copies": 0}
    assert rec.would_issue(1) == {"calls": 1, "waits": 0, "memsets": 0, "copies": 0}
    plain = ops.StepRecorder()                       # accumulate = 1: no window groups, nothing to leave out
    assert plain.window is None and plain.window_skips(False, False) == set()


def test_header_binding_and_library_agree_on_the_new_symbol():
    from syncvsr_amd import _lib

    assert "svsr_steplist_dry_run" in _lib.parse_header()
    lib = _lib.load()
    assert lib.svsr_steplist_dry_run.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]


# ---------------------------------------------------------------------------------------------------------
# the reducer under accumulation: two gloo processes
# ---------------------------------------------------------------------------------------------------------
_WORKER = textwrap.dedent("""
    import os, sys, torch, torch.distributed as dist
    sys.path.insert(0, {root!r})
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.model import Model, _ParamStore
    from syncvsr_amd.engine import AccumWindow, GradReducer
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[3]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = default_lrw_config(model__bert__num_hidden_layers=1)
    model = Model(cfg)
    model._store = _ParamStore(model, torch.device("cpu"))
    st = model._store
    red = GradReducer(model, None, bucket_mb=8.0)
    from syncvsr_amd.init import resnet_block_specs
    order = ["audio_projection.weight", "encoder.encoder.layer.0.attention.self.query.weight", "cls_token"]
    order += [f"{{p}}.conv1.weight" for p, *_ in reversed(list(resnet_block_specs()))]
    base = torch.arange(st.numel, dtype=torch.float32) % 97
    win = AccumWindow(2)
    st.grad.zero_()
    buf0 = st.bufflat.clone()
    for micro in range(2):
        plan = win.plan()
        red.begin_step(sync=plan["reduce"])
        st.grad.add_(0.5 * (base + 10.0 * micro + rank))        # this micro-batch's gradient at scale 1/2, rank-dependent
        st.bufflat.add_(1.0 + rank)                             # BatchNorm statistics move per rank in every micro-step
        before = red.collectives
        for name in order:                                      # the order in which the backward reports progress
            red.on_ready(st.offsets[name][0])
        red.on_ready(0)
        red.finish()
        if micro == 0:
            assert red.collectives == before == 0 and red.launched == [], "no collective in the first micro-step (no_sync)"
            assert torch.equal(st.grad, 0.5 * (base + rank)), "the first micro-step must leave the local gradient alone"
            assert torch.equal(st.bufflat, buf0 + (1.0 + rank)), "no buffer broadcast in a micro-step that does not synchronise"
        else:
            assert red.collectives - before >= 3
        win.advance()
    # sum over the window of 0.5 * (base + 10 micro + rank), then the mean over the ranks
    expect = base + 5.0 + (world - 1) / 2.0
    assert torch.allclose(st.grad, expect), (st.grad - expect).abs().max()
    both = [torch.empty_like(st.grad) for _ in range(world)]
    dist.all_gather(both, st.grad)
    assert all(torch.equal(b, both[0]) for b in both), "both ranks hold the same reduced gradient"
    assert torch.equal(st.bufflat, buf0 + 2.0), "after the last micro-step the buffers follow rank 0"
    covered, pos = sorted(red.launched), 0
    for lo, hi in covered:
        assert lo == pos
        pos = hi
    assert pos == st.numel
    dist.barrier(); dist.destroy_process_group()
    print("ok", rank)
""")


def test_grad_reducer_sits_out_the_first_micro_step_two_process_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "2", port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o
