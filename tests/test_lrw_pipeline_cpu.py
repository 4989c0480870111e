"""Host side of the LRW device input pipeline (no GPU): the restatement's fill recurrence (tests/lrw_pipeline_restatement.py) against
augment.TimeMask on CPU clips, the draws of augment.DeviceLRWPipeline.plan against the functions it is documented to call, the argument
errors that are raised before any launch, and the C ABI of the two entry points (declared, exported, recordable)."""
import os
import random

import pytest
import torch

from lrw_pipeline_restatement import frame_fills, pipeline_ref, sampled_clips, synthetic_frames


def _pipe(**kw):
    from syncvsr_amd.augment import DeviceLRWPipeline

    kw.setdefault("size", 8)
    kw.setdefault("num_labels", 11)
    return DeviceLRWPipeline(**kw)


def _timemask_case(T, max_run, n_mask, seed, replace_with_zero=False, H=5, W=7):
    """One random fp64 CPU clip through augment.TimeMask and through frame_fills, the runs injected by seeding `random` identically."""
    from syncvsr_amd.augment import TimeMask, draw_time_runs

    x = torch.rand(T, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(1000 + seed))
    random.seed(seed)
    got = TimeMask(max_run, n_mask, replace_with_zero)(x)
    random.seed(seed)
    runs = draw_time_runs(T, max_run, n_mask)
    fills = frame_fills(x.sum(dim=(1, 2)).tolist(), runs, T, H * W, replace_with_zero)
    for t in range(T):
        if fills[t] is None:
            assert torch.equal(got[t], x[t]), (runs, t)
        else:
            # fp64 on both sides: the recurrence updates a running sum where torch sums the clip again
            assert (got[t] - fills[t]).abs().max().item() <= 1e-12, (runs, t, fills[t])
            if replace_with_zero:
                assert fills[t] == 0.0 and not got[t].any()
    return runs


def _find(T, max_run, n_mask, want, replace_with_zero=False):
    """The first seed whose drawn runs satisfy `want`; the case is then checked like any other."""
    from syncvsr_amd.augment import draw_time_runs

    for seed in range(5000):
        random.seed(seed)
        if want(draw_time_runs(T, max_run, n_mask)):
            return _timemask_case(T, max_run, n_mask, seed, replace_with_zero)
    raise AssertionError("no seed draws the wanted runs")


@pytest.mark.parametrize("n_mask", [1, 2])
@pytest.mark.parametrize("replace_with_zero", [False, True])
def test_frame_fills_against_timemask(n_mask, replace_with_zero):
    seen = 0
    for seed in range(12):
        runs = _timemask_case(29, 15, n_mask, seed, replace_with_zero)
        seen += sum(1 for _, n in runs if n > 0)
    assert seen >= 6


def test_frame_fills_overlapping_runs():
    runs = _find(12, 8, 2, lambda r: r[0][1] > 1 and r[1][1] > 1 and r[0][0] < r[1][0] < r[0][0] + r[0][1] < r[1][0] + r[1][1])
    assert len(runs) == 2
    _find(12, 8, 2, lambda r: r[0][1] > 1 and r[1][1] > 1 and r[1][0] < r[0][0] < r[1][0] + r[1][1], replace_with_zero=True)


def test_frame_fills_zero_length_run():
    _find(9, 4, 2, lambda r: r[0][1] == 0 and r[1][1] > 0)
    _find(9, 4, 2, lambda r: r[0][1] > 0 and r[1][1] == 0)
    runs = _find(9, 4, 1, lambda r: r[0][1] == 0)
    assert frame_fills([1.0] * 9, runs, 9, 4) == [None] * 9


def test_frame_fills_whole_clip_then_a_second_run():
    """After a run over all T frames the clip is constant, so the second fill is that constant again."""
    runs = _find(4, 4, 2, lambda r: r[0] == (0, 4) and r[1][1] > 0)
    fills = frame_fills([3.0, 1.0, 2.0, 6.0], runs, 4, 2)
    assert all(abs(f - 12.0 / 8.0) < 1e-15 for f in fills)


def test_frame_fills_single_frame_clip():
    seen = set()
    for seed in range(8):
        seen.add(tuple(_timemask_case(1, 15, 1, seed)))
        _timemask_case(1, 15, 2, seed, replace_with_zero=bool(seed & 1))
    assert seen == {((0, 0),), ((1, 0),), ((0, 1),)}          # an empty run may start behind the only frame
    assert frame_fills([6.0], [(0, 1)], 1, 12) == [0.5]


def test_restatement_layout():
    frames = synthetic_frames(3, 4, 10, 12, 0)
    params = torch.tensor([[0, 0, 10, 12, 0], [1, 2, 8, 8, 1], [2, 0, 6, 9, 0]], dtype=torch.int32)
    x = sampled_clips(frames, params, 8, 8)
    assert x.shape == (3, 4, 8, 8)
    assert torch.equal(x[1], (frames[1, :, 1:9, 2:10].double() / 255.0).flip(-1))          # a window of the output size is a plain crop
    fsrc = torch.tensor([[0, 0, 0, 0], [1, 2, 2, 1], [2, 2, 1, 2]])
    out, masked = pipeline_ref(frames, params, fsrc, [[(0, 0)], [(1, 2)], [(3, 1)]], 8, 8)
    assert masked.tolist() == [[False] * 4, [False, False, False, False], [False, False, True, True]]
    assert torch.equal(out[1, 0, 1], out[2, 0, 1]) and torch.equal(out[2, 0, 2], out[1, 0, 0] * 0 + out[2, 0, 2][0, 0])
    m = x[1].mean()
    assert (out[2, 0, 2] - (m - 0.421) / 0.165).abs().max() < 1e-12          # clip 1's frame 2 is masked with clip 1's mean, and lands in sample 2


def test_plan_draws_what_the_documented_calls_draw():
    from syncvsr_amd.augment import DeviceClipPipeline, draw_time_runs, make_plan

    B, T, Hs, Ws, Ta = 6, 29, 20, 24, 58
    pipe = _pipe(size=16, seed=7, n_mask=2)
    pipe.generator = torch.Generator().manual_seed(21)
    random.seed(5)
    plans = [pipe.plan(B, T, Hs, Ws, Ta) for _ in range(2)]
    # the documented order, by hand: windows and flips, then the runs per clip in batch order, then the CutMix plan
    clips = DeviceClipPipeline(16, True, seed=7)
    g = torch.Generator().manual_seed(21)
    random.seed(5)
    for plan in plans:
        params = clips.draw(B, Hs, Ws)
        runs = [draw_time_runs(T, 15, 2) for _ in range(B)]
        cut = make_plan(B, T, Ta, g)
        assert torch.equal(plan["params"], params) and plan["params"].dtype == torch.int32
        assert plan["runs"].dtype == torch.int32 and plan["runs"].tolist() == [[list(r) for r in rs] for rs in runs]
        for k in ("frame_src", "token_src", "target_ids", "mix"):
            assert torch.equal(getattr(plan["cutmix"], k), getattr(cut, k)), k
    assert not torch.equal(plans[0]["params"], plans[1]["params"])
    # a stage that is off draws nothing
    state, tstate = random.getstate(), torch.get_rng_state()
    off = _pipe(use_timemask=False, use_cutmix=False).plan(B, T, Hs, Ws, Ta)
    assert off["runs"] is None and off["cutmix"] is None and random.getstate() == state and torch.equal(torch.get_rng_state(), tstate)
    ev = _pipe(train=False, size=16).plan(2, T, Hs, Ws, Ta)
    assert ev["runs"] is None and ev["cutmix"] is None and ev["params"].tolist() == [[2, 4, 16, 16, 0]] * 2
    assert random.getstate() == state and torch.equal(torch.get_rng_state(), tstate)
    # the default generator is torch's global one, as CutMix
    torch.manual_seed(3)
    a = _pipe(use_timemask=False).plan(B, T, Hs, Ws, Ta)["cutmix"]
    torch.manual_seed(3)
    assert torch.equal(a.frame_src, make_plan(B, T, Ta).frame_src)


def test_argument_errors_before_any_launch():
    from syncvsr_amd import ops
    from syncvsr_amd.audio_codec import Wav2Vec2Codec

    B, T = 2, 4
    frames = synthetic_frames(B, T, 10, 12, 1)
    aud, lab, wm = torch.zeros(B, T, 2, dtype=torch.long), torch.zeros(B, dtype=torch.long), torch.zeros(B, T)
    pipe = _pipe()
    plan = pipe.plan(B, T, 10, 12, T)
    with pytest.raises(ValueError, match="uint8"):
        pipe(frames.float(), aud, lab, wm, plan=plan)
    bad = dict(plan, params=plan["params"].long())
    with pytest.raises(ValueError, match="int32"):
        pipe(frames, aud, lab, wm, plan=bad)
    bad = dict(plan, params=torch.tensor([[0, 0, 10, 12, 0], [3, 0, 8, 12, 0]], dtype=torch.int32))
    with pytest.raises(ValueError, match="crop window outside"):
        pipe(frames, aud, lab, wm, plan=bad)
    bad = dict(plan, runs=torch.tensor([[[0, 1]], [[2, 3]]], dtype=torch.int32))
    with pytest.raises(ValueError, match="run outside"):
        pipe(frames, aud, lab, wm, plan=bad)
    long_clip = torch.zeros(1, ops.LRW_CLIP_MAX_FRAMES + 1, 2, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most 256"):
        _pipe(size=2).__call__(long_clip, aud[:1], lab[:1], wm[:1])
    # the wrappers themselves
    par = plan["params"]
    fsrc = torch.arange(B, dtype=torch.int32).unsqueeze(1).repeat(1, T)
    with pytest.raises(ValueError, match="uint8"):
        ops.lrw_clip_sums(frames.float(), par, 8, 8)
    with pytest.raises(ValueError, match="params"):
        ops.lrw_clip_sums(frames, par.long(), 8, 8)
    with pytest.raises(ValueError, match="at most 256"):
        ops.lrw_clip_sums(long_clip, par[:1], 2, 2)
    with pytest.raises(ValueError, match="frame_src"):
        ops.lrw_clip_mix(frames, par, fsrc.long(), 8, 8)
    with pytest.raises(ValueError, match="runs"):
        ops.lrw_clip_mix(frames, par, fsrc, 8, 8, runs=torch.zeros(B, 1, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="frame_sums"):
        ops.lrw_clip_mix(frames, par, fsrc, 8, 8, runs=torch.zeros(B, 1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="at most 256"):
        ops.lrw_clip_mix(long_clip, par[:1], torch.zeros(1, 257, dtype=torch.int32), 2, 2)
    # the codec rule of CutMix(wav2vec=)
    with pytest.raises(TypeError):
        _pipe(codec=object())
    with pytest.raises(ValueError, match="vq"):
        _pipe(codec=Wav2Vec2Codec.__new__(Wav2Vec2Codec))


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    import ctypes

    from syncvsr_amd import _lib, build

    decl = _lib.parse_header()
    assert [n for _, n in decl["svsr_lrw_clip_sums"]] == ["src_u8", "params", "frame_sums", "B", "T", "Hs", "Ws", "H", "W", "max_blocks", "stream"]
    assert [n for _, n in decl["svsr_lrw_clip_mix"]] == ["src_u8", "params", "frame_src", "runs", "frame_sums", "dst", "B", "T", "Hs", "Ws", "H", "W",
                                                         "n_mask", "replace_with_zero", "mean", "std", "max_blocks", "stream"]
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    for name in ("svsr_lrw_clip_sums", "svsr_lrw_clip_mix"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert lib.svsr_steplist_knows(name.encode())
    # refused before anything is launched (no device needed): T above the cap, null buffers, a non-positive std, runs or sums missing
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    assert lib.svsr_lrw_clip_sums(p, p, p, 1, 257, 4, 4, 4, 4, 0, None) == 1001
    assert lib.svsr_lrw_clip_sums(p, None, p, 1, 1, 4, 4, 4, 4, 0, None) == 1001
    assert lib.svsr_lrw_clip_sums(p, p, p, 1, 1, 4, 4, 4, 4, -1, None) == 1001
    assert lib.svsr_lrw_clip_mix(p, p, p, None, None, p, 1, 257, 4, 4, 4, 4, 0, 0, 0.421, 0.165, 0, None) == 1001
    assert lib.svsr_lrw_clip_mix(p, p, p, None, None, p, 1, 1, 4, 4, 4, 4, 0, 0, 0.421, 0.0, 0, None) == 1001
    assert lib.svsr_lrw_clip_mix(p, p, None, None, None, p, 1, 1, 4, 4, 4, 4, 0, 0, 0.421, 0.165, 0, None) == 1001
    assert lib.svsr_lrw_clip_mix(p, p, p, None, p, p, 1, 1, 4, 4, 4, 4, 1, 0, 0.421, 0.165, 0, None) == 1001
    assert lib.svsr_lrw_clip_mix(p, p, p, p, None, p, 1, 1, 4, 4, 4, 4, 1, 0, 0.421, 0.165, 0, None) == 1001
