"""-m gpu: the LRW device input pipeline (csrc/lrw_prep.hip: svsr_lrw_clip_sums, svsr_lrw_clip_mix; augment.DeviceLRWPipeline) against
svsr_clip_prep, bit for bit, on every frame that is not masked, against the fp64 restatement tests/lrw_pipeline_restatement.py on the
masked ones, against CutMix.forward on the small tensors, and through TrainStep on the tiny LRW configuration.

Bounds.
  unmasked frames   bit-identical to ops.clip_prep(frames, params) gathered through frame_src: the kernels share its sampling device
                    function (csrc/clip_sample.h).
  masked frames     within 2e-5 absolute of the fp64 restatement after Normalize: the worst case of an fp32 sum of <= 2.4 M values in
                    [0, 1], about 21 levels x 6e-8, scaled by 1 / std ~ 6, doubled.  The largest error of every case is printed.
  frame sums        within 1e-6 * H * W of the fp64 sums: <= 5 roundings of 2^-24 per sampled value in [0, 1] (3e-7 each) plus, for the
                    H * W <= 256 of these shapes, one term per thread and 10 levels of butterfly and wave adds of partial sums <= H * W
                    (6e-8 * H * W each): 3e-7 H W + 6.6e-7 H W.
Every case prints its figures before it asserts."""
from __future__ import annotations

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lrw_pipeline_restatement import clip_fills, pipeline_ref, sampled_clips, synthetic_frames  # noqa: E402

pytestmark = pytest.mark.gpu
MEAN, STD = 0.421, 0.165
MASKED_BOUND = 2e-5
I32 = torch.int32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _identity_src(B, T):
    return torch.arange(B, dtype=I32).unsqueeze(1).repeat(1, T)


def _mix(dev, frames, params, fsrc, runs, H, W, zero=False, max_blocks=0):
    """-> (frame sums or None, mixed batch), both on the host."""
    from syncvsr_amd import ops

    f, p = frames.to(dev), params.to(dev)
    r = None if runs is None else runs.to(dev)
    sums = ops.lrw_clip_sums(f, p, H, W, max_blocks) if r is not None and not zero else None
    out = ops.lrw_clip_mix(f, p, fsrc.to(dev), H, W, r, sums, zero, MEAN, STD, max_blocks)
    return None if sums is None else sums.cpu(), out.cpu()


def _check(dev, frames, params, fsrc, runs, H, W, zero=False, what=""):
    """Assertions 1, 2 and 4 for one case; returns the batch."""
    from syncvsr_amd import ops

    B, T = fsrc.shape
    base = ops.clip_prep(frames.to(dev), params.to(dev), H, W, MEAN, STD).cpu()
    sums, out = _mix(dev, frames, params, fsrc, runs, H, W, zero)
    assert out.shape == (B, 1, T, H, W) and out.dtype == torch.float32
    ref, masked = pipeline_ref(frames, params, fsrc, None if runs is None else runs.tolist(), H, W, MEAN, STD, zero)
    worst, n_masked = 0.0, 0
    for b in range(B):
        for t in range(T):
            s = int(fsrc[b, t])
            if masked[b, t]:
                n_masked += 1
                assert (out[b, 0, t] == out[b, 0, t, 0, 0]).all(), (what, b, t, "a masked frame is one constant")
                worst = max(worst, (out[b, 0, t].double() - ref[b, 0, t]).abs().max().item())
            else:
                assert torch.equal(out[b, 0, t], base[s, 0, t]), (what, b, t, s, "an unmasked frame is svsr_clip_prep's, bit for bit")
    sum_err = 0.0
    if sums is not None:
        sum_err = (sums.double() - sampled_clips(frames, params, H, W).sum(dim=(2, 3))).abs().max().item()
    print(f"{what}: {n_masked} masked frames of {B * T}, max |kernel - fp64| on them {worst:.3g} (bound {MASKED_BOUND:.3g}); "
          f"frame sums max |d| {sum_err:.3g} (bound {1e-6 * H * W:.3g})")
    assert worst <= MASKED_BOUND, (what, worst)
    assert sum_err <= 1e-6 * H * W, (what, sum_err)
    for cap in (1, 3, 0):
        s2, o2 = _mix(dev, frames, params, fsrc, runs, H, W, zero, max_blocks=cap)
        assert torch.equal(o2, out) and (sums is None or torch.equal(s2, sums)), (what, "max_blocks", cap)
    return out, base, n_masked


def _params(B, Hs, Ws, seed, size=None):
    from syncvsr_amd.augment import DeviceClipPipeline

    return DeviceClipPipeline(size or Hs, train=True, use_rrc=size is not None, seed=seed).draw(B, Hs, Ws)


def _plan_src(B, T, seed):
    """frame_src of a drawn CutMix plan in which something was cut."""
    from syncvsr_amd.augment import make_plan

    for s in range(seed, seed + 50):
        plan = make_plan(B, T, T, torch.Generator().manual_seed(s))
        if bool((plan.frame_src != _identity_src(B, T)).any()):
            return plan.frame_src.to(I32)
    raise AssertionError("no plan cuts anything")


# (B, T, Hs, Ws, H, W, runs [B][n_mask] (start, length)): the shapes of the issue; runs that overlap, of length 0, over the whole clip
CASES = {
    "3x5_12x14_to_8x8": (3, 5, 12, 14, 8, 8, [[(1, 2)], [(0, 0)], [(3, 2)]]),
    "4x29_20x24_to_16x16": (4, 29, 20, 24, 16, 16, [[(2, 15), (10, 9)], [(0, 29), (4, 3)], [(28, 1), (29, 0)], [(0, 0), (5, 0)]]),
    "frame_7x9": (2, 6, 10, 11, 7, 9, [[(0, 3)], [(4, 2)]]),
    "single_frame": (3, 1, 12, 14, 8, 8, [[(0, 1)], [(0, 0)], [(1, 0)]]),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("zero", [False, True])
def test_masked_and_spliced_frames(dev, name, zero):
    """Measured on an MI355X: the largest error of a masked frame over all cases is 3.6e-7 (4 x 29 frames of 16 x 16, mean fill), 4.9e-8
    with replace_with_zero — far below a quarter of the bound."""
    B, T, Hs, Ws, H, W, runs = CASES[name]
    frames = synthetic_frames(B, T, Hs, Ws, 3)
    params = _params(B, Hs, Ws, 5, size=8)          # windows drawn for RandomResizedCrop; the kernels take any H x W
    params[0] = torch.tensor([0, 0, Hs, Ws, 1])
    fsrc = _plan_src(B, T, 11) if T > 1 else torch.tensor([[1], [1], [0]], dtype=I32)
    _, _, n = _check(dev, frames, params, fsrc, torch.tensor(runs, dtype=I32), H, W, zero, what=f"{name} zero={zero}")
    assert n > 0


def test_no_runs_no_cuts_is_clip_prep(dev):
    """Assertion 1, second part: without runs and with frame_src[b, t] = b the whole output is svsr_clip_prep's; also with a run table that
    holds only empty runs, and through the identity of use_rrc=False (H = Hs, W = Ws, no multiple of 4)."""
    for B, T, Hs, Ws, H, W in ((3, 5, 12, 14, 8, 8), (4, 29, 20, 24, 16, 16), (2, 3, 7, 9, 7, 9)):
        frames = synthetic_frames(B, T, Hs, Ws, 7)
        params = _params(B, Hs, Ws, 9, size=None if (H, W) == (Hs, Ws) else 8)
        out, base, n = _check(dev, frames, params, _identity_src(B, T), None, H, W, what=f"plain {B}x{T} {Hs}x{Ws}->{H}x{W}")
        assert n == 0 and torch.equal(out, base)
        empty = torch.tensor([[(t % T, 0)] for t in range(B)], dtype=I32)
        out, base, n = _check(dev, frames, params, _identity_src(B, T), empty, H, W, what="empty runs")
        assert n == 0 and torch.equal(out, base)


def test_hand_made_plans(dev):
    B, T, Hs, Ws, H, W = 4, 6, 12, 14, 8, 8
    frames = synthetic_frames(B, T, Hs, Ws, 13)
    params = _params(B, Hs, Ws, 15, size=8)
    runs = torch.tensor([[(0, 0)], [(0, 0)], [(0, 0)], [(2, 2)]], dtype=I32)          # clip 3 masks its frames 2 and 3
    fsrc = _identity_src(B, T)
    fsrc[0, 1:4] = 0                                   # a clip whose target is itself: nothing moves
    fsrc[1, 2:4] = 3                                   # sample 1 takes frames 2..3 of clip 3: masked frames of the source land in another clip
    fsrc[2, 1:4] = fsrc[1, 1:4]                        # sample 2's target was spliced earlier in the chain: it takes [1, 3, 3]
    fsrc[0, 5], fsrc[3, 5] = 3, 0                      # two clips swap the same frame
    out, base, n = _check(dev, frames, params, fsrc, runs, H, W, what="hand-made plan")
    assert n == 6                                      # frames 2..3 of clip 3, in samples 1, 2 and 3
    assert torch.equal(out[0, 0, :5], base[0, 0, :5])
    assert torch.equal(out[2, 0, 1], base[1, 0, 1]) and torch.equal(out[0, 0, 5], base[3, 0, 5]) and torch.equal(out[3, 0, 5], base[0, 0, 5])
    # the mask follows the SOURCE clip's runs and mean: one constant, clip 3's mean, wherever clip 3's frames 2..3 land
    fill = clip_fills(sampled_clips(frames, params, H, W), runs.tolist())[3][2]
    for b in (1, 2, 3):
        for t in (2, 3):
            assert torch.equal(out[b, 0, t], out[3, 0, 2])
    assert abs(out[3, 0, 2, 0, 0].item() - (fill - MEAN) / STD) <= MASKED_BOUND
    assert not torch.equal(out[3, 0, 1], out[3, 0, 2]) and torch.equal(out[1, 0, 4], base[1, 0, 4])
    # frame_src outside [0, B) is clamped by the kernel: nothing outside the clips is read
    wild = fsrc.clone()
    wild[0, 0], wild[1, 0] = -7, 99
    _, o = _mix(dev, frames, params, wild, runs, H, W)
    assert torch.equal(o[0, 0, 0], base[0, 0, 0]) and torch.equal(o[1, 0, 0], base[3, 0, 0])


def test_two_calls_give_identical_bits(dev):
    B, T, Hs, Ws, H, W, runs = CASES["4x29_20x24_to_16x16"]
    frames, params = synthetic_frames(B, T, Hs, Ws, 3), _params(B, Hs, Ws, 5, size=8)
    fsrc, runs = _plan_src(B, T, 11), torch.tensor(runs, dtype=I32)
    a, b = _mix(dev, frames, params, fsrc, runs, H, W), _mix(dev, frames, params, fsrc, runs, H, W)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _pipeline_inputs(dev, B, T, Hs, Ws, Ta, num_labels, seed):
    g = torch.Generator().manual_seed(seed)
    frames = synthetic_frames(B, T, Hs, Ws, seed)
    audios = torch.randint(0, 320, (B, Ta, 2), generator=g)
    labels = torch.randint(0, num_labels, (B,), generator=g)
    wm = (torch.rand(B, T, generator=g) < 0.5).float()
    return frames, audios, labels, wm


def test_pipeline_against_cutmix_and_clip_pipeline(dev):
    """Assertion 5, and the stages that are off: tokens, soft labels and word mask are CutMix.forward's on the same plan, bit for bit, and so
    are the clips when nothing is masked; train=False and all flags off are DeviceClipPipeline.__call__ in one svsr_clip_prep launch."""
    import random

    from syncvsr_amd import ops
    from syncvsr_amd.augment import CutMix, DeviceClipPipeline, DeviceLRWPipeline

    B, T, Hs, Ws, Ta, L = 4, 29, 20, 24, 58, 11
    frames, audios, labels, wm = _pipeline_inputs(dev, B, T, Hs, Ws, Ta, L, 17)
    fd, ad, ld, wd = (t.to(dev) for t in (frames, audios, labels, wm))
    pipe = DeviceLRWPipeline(16, L, seed=3, use_timemask=False)
    pipe.generator = torch.Generator().manual_seed(41)
    ops.start_event_timing()
    v, a, l, w = pipe(fd, ad, ld, wd)
    launched = ops.stop_event_timing()
    assert {k: x["launches"] for k, x in launched.items()} == {"k_lrw_clip_mix": 1}
    cm = CutMix(L)
    cm.generator = torch.Generator().manual_seed(41)
    clips = DeviceClipPipeline(16, True, seed=3)
    v2, a2, l2, w2 = cm(clips(fd), ad, ld, wd)
    assert l.shape == (B, L) and l.dtype == torch.float32 and w.dtype == torch.float32 and a.dtype == torch.int64
    assert not torch.equal(a, ad), "the seeded plan cuts nothing: the case shows nothing"
    for got, want, what in ((v, v2, "videos"), (a, a2, "tokens"), (l, l2, "labels"), (w, w2, "word mask")):
        assert torch.equal(got, want), what
    # with the time mask: two launches, small tensors still CutMix's; without a run of positive length the sums launch is left out
    pipe = DeviceLRWPipeline(16, L, seed=3, n_mask=2)
    pipe.generator = torch.Generator().manual_seed(41)
    random.seed(2)
    plan = pipe.plan(B, T, Hs, Ws, Ta)
    assert bool((plan["runs"][..., 1] > 0).any())
    ops.start_event_timing()
    v3, a3, l3, w3 = pipe(fd, ad, ld, wd, plan=plan)
    launched = ops.stop_event_timing()
    assert {k: x["launches"] for k, x in launched.items()} == {"k_lrw_clip_sums": 1, "k_lrw_clip_mix": 1}
    assert torch.equal(a3, a2) and torch.equal(l3, l2) and torch.equal(w3, w2) and not torch.equal(v3, v2)
    ref, masked = pipeline_ref(frames, plan["params"], plan["cutmix"].frame_src, plan["runs"].tolist(), 16, 16, MEAN, STD)
    err = (v3.cpu().double() - ref).abs().max().item()
    print(f"pipeline, masked and mixed: max |kernel - fp64| {err:.3g} over the whole batch, {int(masked.sum())} masked frames")
    assert err <= MASKED_BOUND and bool(masked.any())
    ops.start_event_timing()
    v4 = pipe(fd, ad, ld, wd, plan=dict(plan, runs=plan["runs"] * torch.tensor([1, 0], dtype=I32)))[0]
    launched = ops.stop_event_timing()
    assert {k: x["launches"] for k, x in launched.items()} == {"k_lrw_clip_mix": 1} and torch.equal(v4, v2)
    # the stages that are off
    for kw in (dict(train=False), dict(use_rrc=False, use_timemask=False, use_cutmix=False), dict(train=False, use_val_resize=True)):
        p = DeviceLRWPipeline(16, L, seed=5, **kw)
        ops.start_event_timing()
        got = p(fd, ad, ld, wd)
        launched = ops.stop_event_timing()
        assert set(launched) == {"svsr_clip_prep"}, launched
        want = DeviceClipPipeline(16, kw.get("train", True), use_rrc=kw.get("use_rrc", True), use_val_resize=kw.get("use_val_resize", False), seed=5)(fd)
        assert torch.equal(got[0], want) and got[1] is ad and got[2] is ld and got[3] is wd
    # use_rrc=False with the other stages on: the stored size comes out
    p = DeviceLRWPipeline(16, L, seed=5, use_rrc=False)
    assert p(fd, ad, ld, wd)[0].shape == (B, 1, T, Hs, Ws)


def test_train_step_on_a_pipeline_batch(dev):
    """Assertion 6, on lrw_tiny: one TrainStep.step on the pipeline's batch and one on the same tensors assembled by the old route —
    DeviceClipPipeline, a per-clip fill with the restated fills, CutMix with the same plan — give bit-identical losses."""
    import random

    from golden_cases import build_case
    from syncvsr_amd.augment import CutMix, DeviceClipPipeline, DeviceLRWPipeline
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    cfg, sd, batch, _, _ = build_case("lrw_tiny")
    _, tokens, labels, wm = batch
    B, T, size, L = tokens.shape[0], 5, 24, int(cfg.model.bert.num_labels)
    frames = synthetic_frames(B, T, 30, 28, 23)
    fd, ad, ld, wd = (t.to(dev) for t in (frames, tokens, labels, wm))
    pipe = DeviceLRWPipeline(size, L, seed=1)
    plan = None
    for seed in range(100):          # a plan that masks and cuts something
        pipe.generator = torch.Generator().manual_seed(seed)
        random.seed(seed)
        plan = pipe.plan(B, T, 30, 28, tokens.shape[1])
        if bool((plan["runs"][..., 1] > 0).all()) and bool((plan["cutmix"].mix > 0).any()) and bool((plan["cutmix"].frame_src != _identity_src(B, T)).any()):
            break
    else:
        raise AssertionError("no seed masks and cuts")
    new = pipe(fd, ad, ld, wd, plan=plan)
    # the old route
    x = DeviceClipPipeline(size, True, seed=1)(fd, plan["params"])
    fills = clip_fills(sampled_clips(frames, plan["params"], size, size), plan["runs"].tolist())
    for s in range(B):
        for t in range(T):
            if fills[s][t] is not None:
                x[s, 0, t] = (fills[s][t] - MEAN) / STD
    cm = CutMix(L)
    cm.generator = torch.Generator().manual_seed(seed)
    old = cm(x, ad, ld, wd)
    for a, b in zip(new[1:], old[1:]):
        assert torch.equal(a, b)
    d = (new[0] - old[0]).abs().max().item()
    losses = []
    for route in (new, old):
        model = Model(cfg)
        model.load_state_dict(sd)
        model.to(dev).train()
        out = TrainStep(model, cfg).step(*route)
        losses.append({k: float(v) for k, v in out.items()})
    torch.cuda.synchronize()
    print(f"clips of the two routes differ by at most {d:.3g}; losses {losses[0]} | {losses[1]}")
    assert d <= MASKED_BOUND
    assert losses[0]["loss_total"] == losses[1]["loss_total"] and losses[0] == losses[1]
