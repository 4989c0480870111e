"""First-touch stores of the flat gradient buffer, host side (no GPU): ops.GradCoverage and the spans the word-level model declares.

The bounds here are exact by construction: the spans and the holes must partition the buffer (up to the documented round-down of a hole's
start to 16 bytes), every declared span is a whole unpadded tensor (or query | key | value, adjacent), and what is left for the zero-fill is
exactly the rest: the stem's weight, the embeddings, padded tensors and the 1-D tail."""
import ctypes

import pytest
import torch


def _store(**over):
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.model import Model, _ParamStore

    cfg = default_lrw_config(**over)
    model = Model(cfg)
    return cfg, model, _ParamStore(model, torch.device("cpu"))


def test_plan_partitions_the_buffer():
    from syncvsr_amd import ops

    spans, holes = ops.GradCoverage.plan([(8, 14), (16, 32), (40, 48)], 64)
    assert spans == [(8, 14), (16, 32), (40, 48)]
    assert holes == [(0, 8), (12, 16), (32, 40), (48, 64)]           # (12: the hole behind [8, 14) starts at 14 rounded down to 4)
    covered = set()
    for lo, hi in spans:
        covered |= set(range(lo, hi))
    filled = set()
    for lo, hi in holes:
        assert lo % 4 == 0 and hi % 4 == 0
        filled |= set(range(lo, hi))
    assert covered | filled == set(range(64))
    assert ops.GradCoverage.plan([], 16) == ([], [(0, 16)])
    for bad in ([(2, 8)], [(0, 8), (4, 12)], [(0, 0)], [(0, 68)]):
        with pytest.raises(ValueError):
            ops.GradCoverage.plan(bad, 64)


def test_touch_stores_once_per_step_and_only_planned_spans():
    from syncvsr_amd import ops

    grad = torch.zeros(64)
    cov = ops.GradCoverage(grad, [(8, 16), (16, 32)])
    base = grad.data_ptr()
    assert ops._grad_add(grad[8:16], 8) == 1                  # nothing armed: a launch outside a step adds
    cov.begin()
    try:
        assert cov.touch(base + 8 * 4, 8) == 0                # first writer: store
        assert cov.touch(base + 8 * 4, 8) == 1                # second writer of the same span: add
        with pytest.raises(RuntimeError):
            cov.touch(base + 8 * 4, 4)                        # part of a span: neither zero-filled nor storable as a whole — refused before the launch
        with pytest.raises(RuntimeError):
            cov.touch(base + 12 * 4, 8)                       # straddles two spans
        assert cov.touch(base + 32 * 4, 8) == 1               # a hole: zero-filled, add
        assert cov.touch(base - 64, 8) == 1                   # foreign memory: add
    finally:
        assert cov.end() == [(16, 32)]                        # planned, never written: the engine refuses to step on it
    assert ops._COVER is None and ops.end_grad_coverage() == []
    cov.begin()
    assert cov.touch(base + 8 * 4, 8) == 0 and cov.touch(base + 16 * 4, 16) == 0      # the next step starts over
    assert cov.end() == []


@pytest.mark.parametrize("over", [dict(), dict(model__bert__num_hidden_layers=2)])
def test_lrw_spans_cover_the_unpadded_matrices_and_nothing_else(over):
    from syncvsr_amd import ops

    cfg, model, st = _store(**over)
    spans = model.grad_store_spans(st.offsets, st.phys)
    sp, holes = ops.GradCoverage.plan(spans, st.numel)
    covered = torch.zeros(st.numel, dtype=torch.int32)
    for lo, hi in sp:
        covered[lo:hi] += 1
    assert int(covered.max()) == 1
    D = model.dim
    for n, (o, numel, shape) in st.offsets.items():
        seg = covered[o : o + numel]
        conv = len(shape) == 4
        dense = len(shape) == 2 and (".dense.weight" in n or ".self." in n and n.endswith(".weight") or n in ("audio_projection.weight", "category_classifier.weight"))
        want = (conv or dense) and tuple(st.phys[n]) == tuple(shape)
        assert int(seg.min()) == int(seg.max()) == (1 if want else 0), n
    # the stem, the embeddings and every 1-D tensor stay with the zero-fill
    for n in ("stem3d.0.weight", "cls_token", "encoder.embeddings.position_embeddings.weight", "resnet.layer1.0.bn1.weight",
              "encoder.encoder.layer.0.attention.self.query.bias"):
        o, numel, _ = st.offsets[n]
        assert int(covered[o : o + numel].max()) == 0, n
    # holes = exactly the uncovered elements (plus at most 3 already-covered elements in front of each hole)
    filled = torch.zeros(st.numel, dtype=torch.int32)
    for lo, hi in holes:
        filled[lo:hi] += 1
    assert bool(((covered + filled) >= 1).all()) and int(((covered == 1) & (filled == 1)).sum()) <= 3 * len(holes)
    assert len(holes) <= 16                                    # one svsr_fill_ranges launch
    uncovered = int((covered == 0).sum())
    assert uncovered < st.numel // 20, (uncovered, st.numel)   # the fill shrinks to a few per cent of the buffer
    q = st.offsets["encoder.encoder.layer.0.attention.self.query.weight"][0]
    assert (q, q + 3 * D * D) in sp                            # query | key | value: one launch, one span


def test_one_launch_may_tile_adjacent_spans():
    """query | key | value as one launch: it tiles whole adjacent spans, which are stored (or added to) together; a mixed state is refused."""
    from syncvsr_amd import ops

    grad = torch.zeros(64)
    cov = ops.GradCoverage(grad, [(8, 16), (16, 24), (24, 32), (40, 48)])
    base = grad.data_ptr()
    cov.begin()
    assert cov.touch(base + 8 * 4, 24) == 0 and cov.touch(base + 8 * 4, 24) == 1
    assert cov.touch(base + 16 * 4, 8) == 1                    # one of them again, alone: add
    assert cov.end() == [(40, 48)]
    cov.begin()
    assert cov.touch(base + 16 * 4, 8) == 0
    with pytest.raises(RuntimeError):
        cov.touch(base + 8 * 4, 24)                            # one of the three already written, two not
    with pytest.raises(RuntimeError):
        cov.touch(base + 8 * 4, 40)                            # crosses the hole [32, 40)
    cov.end()


def test_fill_ranges_rejects_bad_ranges_before_any_launch():
    from syncvsr_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf) // 16 * 16 + 16
    for rng in ((0, 6), (2, 8), (8, 4), (0, 128), (-4, 4)):
        arr = (ctypes.c_int64 * 2)(*rng)
        assert lib.svsr_fill_ranges(base, 32, arr, 1, 0, None) == 1001, rng
    assert lib.svsr_fill_ranges(base + 4, 32, (ctypes.c_int64 * 2)(0, 4), 1, 0, None) == 1001      # misaligned base
    assert lib.svsr_steplist_knows(b"svsr_fill_ranges") and lib.svsr_steplist_knows(b"svsr_igemm_wgrad_v2")
    assert lib.svsr_steplist_knows(b"svsr_igemm_wgrad_group_v2") and lib.svsr_steplist_knows(b"svsr_conv3x3_wgrad_v2")


def test_unit_list_plans_give_every_task_a_unit():
    """The invariant first-touch stores rest on — every element of dW is written in either mode — for unit-list plans: a tap no position
    reaches (3 x 3 / pad 1 on a 1 x 1 map: eight of nine taps) still gets one (empty) unit per tile, so its part of dW is written as zeros.
    (The (split, task) grids of the other plan formats launch every task by construction.)"""
    from syncvsr_amd import _lib

    lib = _lib.load()
    for args in ((2048, 1, 1, 64, 64, 3, 1, 1), (2048, 2, 2, 128, 128, 3, 1, 1), (928, 11, 11, 128, 256, 1, 2, 0)):
        meta = (ctypes.c_int * 8)()
        nfl = ctypes.c_int64(0)
        n = lib.svsr_wgrad_plan(*args, None, 0, meta, ctypes.byref(nfl))
        assert n > 0
        words = (ctypes.c_int * n)()
        assert lib.svsr_wgrad_plan(*args, words, n, meta, ctypes.byref(nfl)) == n
        assert meta[7] > 0, "expected a unit-list plan"
        units, tasks = meta[3], meta[4]
        per_task = [0] * tasks
        for u in range(units):
            per_task[words[meta[7] + 4 * u]] += 1
        assert min(per_task) >= 1, (args, per_task)


def test_lrs_spans_are_the_dense_and_convolution_weights():
    """The sentence-level parameter layout: every `linear_w` tensor (written by _lin_bwd) and every 4-D convolution weight is a span, nothing
    else is; the zero-fill shrinks from 1 GB to the rest (stem, depthwise convolutions, position biases, embedding, 1-D tail)."""
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_init import LRS_ODIM, default_lrs_args
    from syncvsr_amd.lrs_model import E2E
    from syncvsr_amd.model import _ParamStore

    model = E2E(LRS_ODIM, default_lrs_args())
    st = _ParamStore(model, torch.device("cpu"))
    sp, holes = ops.GradCoverage.plan(model.grad_store_spans(st.offsets, st.phys), st.numel)
    want = sorted((st.offsets[n][0], st.offsets[n][0] + st.offsets[n][1]) for n, shape, kind in model._specs
                  if (kind == "linear_w" or (kind == "conv" and len(shape) == 4)) and tuple(st.phys[n]) == tuple(shape))
    assert sp == want and len(sp) > 100
    kinds = {kind for n, shape, kind in model._specs if (st.offsets[n][0], st.offsets[n][0] + st.offsets[n][1]) in set(sp)}
    assert kinds == {"linear_w", "conv"}
    hole = sum(hi - lo for lo, hi in holes)
    assert hole + sum(hi - lo for lo, hi in sp) >= st.numel and hole * 4 < 32 * 2 ** 20 < st.numel * 4 // 16, hole
    # fused projections: query | key | value are adjacent spans one launch can tile
    q = st.offsets["encoder.encoders.0.self_attn.linear_q.weight"]
    k = st.offsets["encoder.encoders.0.self_attn.linear_k.weight"]
    assert k[0] == q[0] + q[1]
