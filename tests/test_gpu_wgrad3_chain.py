"""Chained 3x3 halo weight gradients (csrc/wgrad3x3.hip, svsr_conv3x3_wgrad_chain / svsr_conv3x3_wgrad_reduce): a launch leaves its split-K
slabs to the NEXT halo launch on the stream, whose workgroups add them into the previous convolution's dW before their own work.  The sum goes
through the same device function as the stand-alone k_wgrad3_reduce, so every comparison here is BIT-exact against the two-launch form
(svsr_conv3x3_wgrad_v2: halo launch, then k_wgrad3_reduce), which tests/test_gpu_kernels.py pins to the oracle.

Shapes: three convolutions of different geometry and channel counts in one chain, each with more than one split and a last chunk of
128 pixels that is not full (1452, 363 and 351 pixels)."""
import ctypes
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"
ERR_ARG = 1001
# (Nimg, H, W, Ci, Co): layer1-like, layer2-like (four 64 x 64 tiles), and a non-square map with Ci != Co
SHAPES = ((3, 22, 22, 64, 64), (3, 11, 11, 128, 128), (3, 9, 13, 64, 128))


def _lib():
    from syncvsr_amd import _lib as L

    return L.load()


def _plan(shape):
    splits, nfl = ctypes.c_int(0), ctypes.c_int64(0)
    assert _lib().svsr_conv3x3_wgrad_plan(*shape, ctypes.byref(splits), ctypes.byref(nfl)) == 0
    return splits.value, nfl.value


def _operands(shape, seed):
    N, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Ci, generator=g).to(BF).to(DEV)
    dy = (torch.randn(N, H, W, Co, generator=g) * 0.25).to(BF).to(DEV)
    dw0 = torch.randn(Co, 9, Ci, generator=g).to(DEV)          # what dW holds before the launch (add = 1 adds to it, add = 0 must overwrite it)
    return x, dy, dw0


def _p(t):
    return None if t is None else t.data_ptr()


def _two_launch(shape, x, dy, dw0, add):
    """The existing form, in a workspace of its own."""
    _, nfl = _plan(shape)
    part = torch.empty(max(nfl, 1), device=DEV)
    dw = dw0.clone()
    assert _lib().svsr_conv3x3_wgrad_v2(_p(x), _p(dy), _p(dw), *shape, _p(part), nfl, add, None) == 0
    torch.cuda.synchronize()
    return dw, part


def _chain(ops_seq, sets, add, defer_last=True):
    """ops_seq: [(shape, x, dy, dw)] -> issues the chain through the C ABI: launch i writes sets[i % 2] and carries launch i - 1's slabs; the
    last launch's slabs go through svsr_conv3x3_wgrad_reduce."""
    lib, pend = _lib(), None
    for i, (shape, x, dy, dw) in enumerate(ops_seq):
        splits, nfl = _plan(shape)
        assert splits > 1, (shape, splits)
        part = sets[i % 2]
        assert part.numel() >= nfl
        pp = pend or (None, None, 0, 0, 0, 0)
        rc = lib.svsr_conv3x3_wgrad_chain(_p(x), _p(dy), _p(dw), *shape, _p(part), nfl, add, 1, _p(pp[0]), _p(pp[1]), *pp[2:], None)
        assert rc == 0, (i, rc)
        pend = (part, dw, splits, shape[3], shape[4], add)
    assert lib.svsr_conv3x3_wgrad_reduce(_p(pend[0]), _p(pend[1]), *pend[2:], None) == 0
    torch.cuda.synchronize()


@lru_cache(maxsize=None)
def _chain_case(add):
    """-> [(dW of the chain, dW of the two-launch form)] per convolution; both slab sets are NaN before the chain."""
    data = [(s, *_operands(s, 100 + i)) for i, s in enumerate(SHAPES)]
    nmax = max(_plan(s)[1] for s in SHAPES)
    sets = [torch.full((nmax,), float("nan"), device=DEV) for _ in range(2)]
    dws = [dw0.clone() for _, _, _, dw0 in data]
    _chain([(s, x, dy, dw) for (s, x, dy, _), dw in zip(data, dws)], sets, add)
    refs = [_two_launch(s, x, dy, dw0, add)[0] for s, x, dy, dw0 in data]
    return list(zip(dws, refs))


@pytest.mark.parametrize("add", [0, 1])
def test_chain_of_three_shapes_matches_two_launch_form(add):
    for i, (dw, ref) in enumerate(_chain_case(add)):
        assert torch.equal(dw.view(torch.int32), ref.view(torch.int32)), f"convolution {i} {SHAPES[i]} add={add}: dW differs from halo + k_wgrad3_reduce"
    if add == 0:      # the store mode overwrote what dW held
        for i, (dw, _) in enumerate(_chain_case(0)):
            assert not torch.equal(dw, _operands(SHAPES[i], 100 + i)[2])


@pytest.mark.parametrize("add", [0, 1])
def test_poisoned_slab_sets_reach_no_dw(add):
    """Both sets were NaN before the chain: a pending reduce that read the wrong set, or a slab its producer did not write, would show."""
    for i, (dw, _) in enumerate(_chain_case(add)):
        assert not torch.isnan(dw).any(), f"convolution {i}: NaN from the poisoned workspace reached dW"


def test_overlapping_slab_sets_are_refused_without_a_launch():
    lib = _lib()
    s0, s1 = SHAPES[0], SHAPES[1]
    x, dy, dw0 = _operands(s1, 7)
    (sp0, nfl0), (sp1, nfl1) = _plan(s0), _plan(s1)
    buf = torch.full((nfl0 + nfl1,), 3.0, device=DEV)
    dw, pdw = dw0.clone(), torch.full((s0[4], 9, s0[3]), 5.0, device=DEV)
    for off in (0, nfl1 - 1, -(nfl0 - 1)):          # the pending slabs start at / end inside / begin before the range the launch writes
        own = buf[nfl0:] if off < 0 else buf
        pend = buf[nfl0 + off:] if off < 0 else buf[off:]
        rc = lib.svsr_conv3x3_wgrad_chain(_p(x), _p(dy), _p(dw), *s1, _p(own), nfl1, 1, 1, _p(pend), _p(pdw), sp0, s0[3], s0[4], 1, None)
        assert rc == ERR_ARG, (off, rc)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw0) and bool((buf == 3.0).all()) and bool((pdw == 5.0).all()), "a refused call launched something"
    # disjoint: accepted (the pending slabs lie right behind the launch's own)
    buf.zero_()
    rc = lib.svsr_conv3x3_wgrad_chain(_p(x), _p(dy), _p(dw), *s1, _p(buf), nfl1, 1, 1, _p(buf[nfl1:]), _p(pdw), sp0, s0[3], s0[4], 1, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((pdw == 5.0).all())          # zero slabs were added


@pytest.mark.parametrize("add", [0, 1])
def test_no_pending_no_defer_is_the_old_entry_point(add):
    for i, s in enumerate(SHAPES):
        x, dy, dw0 = _operands(s, 40 + i)
        ref, ref_part = _two_launch(s, x, dy, dw0, add)
        _, nfl = _plan(s)
        part, dw = torch.empty(nfl, device=DEV), dw0.clone()
        assert _lib().svsr_conv3x3_wgrad_chain(_p(x), _p(dy), _p(dw), *s, _p(part), nfl, add, 0, None, None, 0, 0, 0, 0, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(dw.view(torch.int32), ref.view(torch.int32))
        assert torch.equal(part.view(torch.int32), ref_part[:nfl].view(torch.int32)), "the slabs differ"


def test_bad_pending_descriptor_is_refused():
    s = SHAPES[0]
    x, dy, dw0 = _operands(s, 9)
    _, nfl = _plan(s)
    part, other, dw = torch.empty(nfl, device=DEV), torch.empty(nfl, device=DEV), dw0.clone()
    for pend in ((_p(other), None, 4, 64, 64, 1), (_p(other), _p(dw0), 1, 64, 64, 1), (_p(other), _p(dw0), 4, 96, 64, 1), (_p(other), _p(dw0), 4, 64, 64, 2)):
        assert _lib().svsr_conv3x3_wgrad_chain(_p(x), _p(dy), _p(dw), *s, _p(part), nfl, 1, 1, *pend, None) == ERR_ARG, pend
    assert _lib().svsr_conv3x3_wgrad_reduce(None, _p(dw), 4, 64, 64, 1, None) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(dw, dw0)


def test_recorded_chain_replays_to_the_eager_bits():
    """The chain through ops (two slab sets per stream, pending records), recorded into a native step list, replayed on refilled inputs."""
    from syncvsr_amd import ops

    def tensors(seed):
        return [_operands(s, seed + i) for i, s in enumerate(SHAPES)]

    def run(ts, dws):
        pend = None
        for (x, dy, _), dw in zip(ts, dws):
            pend = ops.conv3x3_wgrad_chain(x, dy, dw, pend, mode=0)
            assert pend is not None
        ops.conv3x3_wgrad_flush(pend)

    t = tensors(500)
    dws = [torch.full_like(dw0, float("nan")) for _, _, dw0 in t]
    rec = ops.StepRecorder()
    with ops.recording(rec):
        run(t, dws)
    torch.cuda.synchronize()
    assert rec.calls() == len(SHAPES) + 1          # three halo launches, ONE stand-alone reduce
    first = [d.clone() for d in dws]
    fresh = tensors(900)
    for (x, dy, _), (fx, fdy, _) in zip(t, fresh):
        x.copy_(fx)
        dy.copy_(fdy)
    rec.run()
    torch.cuda.synchronize()
    for i, (s, (fx, fdy, dw0)) in enumerate(zip(SHAPES, fresh)):
        ref, _ = _two_launch(s, fx, fdy, dw0, 0)
        assert torch.equal(dws[i].view(torch.int32), ref.view(torch.int32)), f"convolution {i}: the replay differs from the eager two-launch form"
        assert not torch.equal(dws[i], first[i]), f"convolution {i}: the replay did not see the refilled inputs"
    with pytest.raises(RuntimeError):          # a chain may not enter an op group a replay can skip
        rec2 = ops.StepRecorder()
        with ops.recording(rec2), rec2.group(0):
            ops.conv3x3_wgrad_chain(*t[0][:2], dws[0], None, mode=0)
