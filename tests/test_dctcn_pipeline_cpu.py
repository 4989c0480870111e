"""Host side of the DC-TCN device input pipeline (no GPU): the restatement tests/dctcn_pipeline_restatement.py against what the reference's
own LRWDatasetForDCTCN._mask_frames + _trim_frames produced (tests/golden/dctcn_data.npz, made by tests/golden/make_golden_dctcn_data.py),
the draws of augment.DeviceDCTCNPipeline.plan against the integers the reference drew under the same seeds, the errors raised before any
launch, and the C ABI of the three entry points (declared, exported, recordable, 1001 on bad arguments).

What "reproduces the golden" means per output.  The golden is the reference's fp32; the restatement is fp64 and derives the clip mean from
the integer sum, so:
  audios, word_mask, attention_mask   equal, element for element (moved or zeroed, never computed);
  videos, trimmed frames              exactly 0;
  videos, every other unmasked frame  the SAME stored frame: round((g + 1) * 255 / 2) recovers the uint8 frame the restatement names, exactly
                                      (the fp32 error of g, 1.2e-7, is 1.5e-5 grey levels), and |g - restated| <= 2.4e-7, two fp32 roundings
                                      of values in [-1, 1];
  videos, masked frames               one constant per frame, within 2e-6 of the restated mean: the reference takes torch's fp32 mean of fp32
                                      values.  Each value is off by <= 1.2e-7; torch adds n = 870 (T = 29) of them in a cascade of depth
                                      <= log2(n) = 10, each level costing the mean <= 6e-8 of max |x| = 1: 7.2e-7 in all, rounded up to
                                      2e-6 — three orders below one grey level (7.8e-3)."""
import os

import numpy as np
import pytest
import torch

from dctcn_pipeline_restatement import clip_sums, mask_trim, pipeline_ref, transform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dctcn_data.npz")
L = 1000


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def _cases(g):
    return [tuple(int(v) for v in row) for row in g["cases"]]


def _ints(T, wb, drawn):
    """The reference's four draws -> (shift, trunc, mask_off, mask_len, ashift, azero), by the issue's formulas."""
    length, offset, truncated, off2 = (int(v) for v in drawn)
    shift = int(off2 - (T - wb) // 2)
    return shift, truncated, offset, length, int(shift / (T / L)), int(truncated / (T / L))


def test_restatement_reproduces_the_reference(golden):
    seen = dict(neg=0, pos=0, zero=0, masked=0, unmasked=0)
    for T, _, wb, seed in _cases(golden):
        tag = f"T{T}_wb{wb}_s{seed}"
        clip, wave = torch.from_numpy(golden[f"clip_T{T}"]), torch.from_numpy(golden[f"wave_T{T}"])
        shift, trunc, moff, mlen, ashift, azero = _ints(T, wb, golden[f"drawn_{tag}"])
        v, audio, word, att, kind = mask_trim(clip, wave, wb, shift, trunc, moff, mlen, ashift, azero)
        assert torch.equal(audio, torch.from_numpy(golden[f"audios_{tag}"])), tag
        assert torch.equal(word, torch.from_numpy(golden[f"word_mask_{tag}"])), tag
        assert torch.equal(att, torch.from_numpy(golden[f"attention_mask_{tag}"])), tag
        gv = torch.from_numpy(golden[f"videos_{tag}"])
        assert gv.dtype == torch.float32 and gv.shape == v.shape
        for t in range(T):
            if kind[t] == "z":
                assert not gv[t].any(), (tag, t)
            elif kind[t] == "m":
                assert (gv[t] == gv[t, 0, 0]).all() and (gv[t].double() - v[t]).abs().max().item() <= 2e-6, (tag, t)
            else:
                assert torch.equal(((gv[t].double() + 1.0) * 255.0 / 2.0).round().to(torch.uint8), clip[kind[t]]), (tag, t)
                assert (gv[t].double() - v[t]).abs().max().item() <= 2.4e-7, (tag, t)
        seen["neg" if shift < 0 else "pos" if shift > 0 else "zero"] += 1
        seen["masked" if mlen > 0 else "unmasked"] += 1
    assert all(seen[k] > 0 for k in ("neg", "zero", "masked", "unmasked")), seen          # (the reference's shift is never positive at wb < T)


def test_plan_reproduces_the_reference_draws(golden):
    from syncvsr_amd.augment import DeviceDCTCNPipeline

    for T, max_masks, wb, seed in _cases(golden):
        tag = f"T{T}_wb{wb}_s{seed}"
        pipe = DeviceDCTCNPipeline(6, max_time_masks=max_masks, seed=1)
        np.random.seed(seed)
        plan = pipe.plan(1, T, 6, 5, L, [wb])
        shift, trunc, moff, mlen, ashift, azero = _ints(T, wb, golden[f"drawn_{tag}"])
        assert plan["time"].dtype == torch.int32 and plan["time"].tolist() == [[shift, trunc, moff, mlen]], tag
        assert plan["audio"].dtype == torch.int32 and plan["audio"].tolist() == [[ashift, azero]], tag
        assert plan["params"].tolist()[0][:4] == [0, 0, 6, 5]          # use_rrc off: the stored frame passes through
    # several clips: per clip in batch order, one stream
    T = 29
    pipe = DeviceDCTCNPipeline(6, seed=1)
    np.random.seed(7)
    plan = pipe.plan(3, T, 6, 5, L, torch.tensor([1, 5, 28]))
    after_plan = np.random.randint(1 << 30)
    np.random.seed(7)
    for b, wb in enumerate((1, 5, 28)):
        length = np.random.randint(15)
        offset = np.random.randint(T - length)
        truncated = np.random.randint(wb, T)
        off2 = np.random.randint(truncated - wb + 1)
        assert plan["time"][b].tolist() == [off2 - (T - wb) // 2, truncated, offset, length]
    assert np.random.randint(1 << 30) == after_plan          # four draws per clip and nothing else from np.random
    # int() truncates towards zero: a negative shift's audio shift is no floor
    assert int(-3 / (29 / 1000)) == -103 and plan["audio"].dtype == torch.int32
    # the eval chain draws nothing from np.random and plans the identity
    state = np.random.get_state()[1].copy()
    ev = DeviceDCTCNPipeline(4, train=False).plan(2, T, 6, 5, L, [5, 29])
    assert np.array_equal(np.random.get_state()[1], state)
    assert ev["time"].tolist() == [[0, T, 0, 0]] * 2 and ev["audio"].tolist() == [[0, L]] * 2 and ev["params"].tolist() == [[1, 0, 4, 4, 0]] * 2


def test_draw_lam():
    from syncvsr_amd.augment import DeviceDCTCNPipeline

    np.random.seed(3)
    got = [DeviceDCTCNPipeline.draw_lam(0.4) for _ in range(20)]
    np.random.seed(3)
    assert got == [0.5 - abs(0.5 - np.random.beta(0.4, 0.4)) for _ in range(20)]
    assert all(0.0 <= v <= 0.5 for v in got)


def test_value_and_not_implemented_errors():
    from syncvsr_amd.augment import DeviceDCTCNPipeline
    from syncvsr_amd.config import Config
    from syncvsr_amd.dctcn_init import default_dctcn_config

    pipe = DeviceDCTCNPipeline(6)
    with pytest.raises(ValueError, match="clip 1"):          # boundary >= T: the reference's randint(boundary, T) raises
        DeviceDCTCNPipeline(6, max_time_masks=4).plan(2, 8, 6, 5, L, [3, 8])
    with pytest.raises(ValueError, match="clip 0"):          # T - length <= 0: a seed whose first draw is >= T
        for seed in range(100):
            np.random.seed(seed)
            if np.random.randint(15) >= 3:
                np.random.seed(seed)
                pipe.plan(1, 3, 6, 5, L, [1])
    with pytest.raises(ValueError, match="one word length per clip"):
        pipe.plan(2, 8, 6, 5, L, [3])
    with pytest.raises(ValueError, match="max_time_masks"):
        DeviceDCTCNPipeline(6, max_time_masks=0)
    # from_config: the shipped configuration has none of the flags; use_timemask is refused
    cfg = default_dctcn_config()
    p = DeviceDCTCNPipeline.from_config(cfg, train=True)
    assert (p.size, p.max_time_masks, p.train, p.clips.use_rrc, p.clips.use_val_resize) == (96, 15, True, False, False)
    cfg2 = Config(data=dict(input_size=88, max_time_masks=7), train=dict(use_rrc=True, use_val_resize=True))
    p = DeviceDCTCNPipeline.from_config(cfg2, train=False)
    assert (p.size, p.max_time_masks, p.train, p.clips.use_rrc, p.clips.use_val_resize) == (88, 7, False, True, True)
    with pytest.raises(NotImplementedError, match="use_timemask"):
        DeviceDCTCNPipeline.from_config(Config(data=dict(input_size=88), train=dict(use_timemask=True)), train=True)


def test_argument_errors_before_any_launch():
    from syncvsr_amd import ops

    B, T = 2, 4
    frames = torch.zeros(B, T, 6, 5, dtype=torch.uint8)
    waves, labels = torch.zeros(B, 100), torch.zeros(B, dtype=torch.long)
    from syncvsr_amd.augment import DeviceDCTCNPipeline

    pipe = DeviceDCTCNPipeline(6, max_time_masks=2)
    plan = pipe.plan(B, T, 6, 5, 100, [1, 2])
    with pytest.raises(ValueError, match="uint8"):
        pipe(frames.float(), waves, labels, [1, 2], plan=plan)
    with pytest.raises(ValueError, match="not a token row"):
        pipe(frames, torch.zeros(B, 16, 2, dtype=torch.long), labels, [1, 2], plan=plan)
    with pytest.raises(ValueError, match=r"fp32 \[B, L\]"):
        pipe(frames, waves.double(), labels, [1, 2], plan=plan)
    with pytest.raises(ValueError, match="lam"):
        pipe(frames, waves, labels, [1, 2], lam=0.6, plan=plan)
    with pytest.raises(ValueError, match="boundaries"):
        pipe(frames, waves, labels, [1, 5], plan=plan)
    with pytest.raises(ValueError, match="int32"):
        pipe(frames, waves, labels, [1, 2], plan=dict(plan, time=plan["time"].long()))
    with pytest.raises(ValueError, match="crop window outside"):
        pipe(frames, waves, labels, [1, 2], plan=dict(plan, params=torch.tensor([[0, 0, 6, 5, 0], [1, 0, 6, 5, 0]], dtype=torch.int32)))
    with pytest.raises(ValueError, match="trim length"):
        pipe(frames, waves, labels, [1, 2], plan=dict(plan, time=torch.tensor([[0, 5, 0, 0], [0, 4, 0, 0]], dtype=torch.int32)))
    with pytest.raises(ValueError, match="run outside"):
        pipe(frames, waves, labels, [1, 2], plan=dict(plan, time=torch.tensor([[0, 4, 3, 2], [0, 4, 0, 0]], dtype=torch.int32)))
    long_clip = torch.zeros(1, ops.DCTCN_CLIP_MAX_FRAMES + 1, 2, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most 256"):
        DeviceDCTCNPipeline(2)(long_clip, waves[:1], labels[:1], [1])
    # the wrappers themselves
    table = torch.zeros(B, 9, dtype=torch.int32)
    with pytest.raises(ValueError, match="uint8"):
        ops.dctcn_clip_sums(frames.float())
    with pytest.raises(ValueError, match="at most 256"):
        ops.dctcn_clip_sums(long_clip)
    with pytest.raises(ValueError, match="table"):
        ops.dctcn_clip_mix(frames, table.long(), 6, 5)
    with pytest.raises(ValueError, match="table"):
        ops.dctcn_clip_mix(frames, table[:, :5].contiguous(), 6, 5)
    with pytest.raises(ValueError, match="frame_sums"):
        ops.dctcn_clip_mix(frames, table, 6, 5, frame_sums=torch.zeros(B, T))
    with pytest.raises(ValueError, match="lam"):
        ops.dctcn_clip_mix(frames, table, 6, 5, lam=0.51)
    with pytest.raises(ValueError, match="std"):
        ops.dctcn_clip_mix(frames, table, 6, 5, std=0.0)
    with pytest.raises(ValueError, match="out must"):
        ops.dctcn_clip_mix(frames, table, 6, 5, out=torch.zeros(B, 1, T, 6, 4))
    with pytest.raises(ValueError, match="wave must"):
        ops.dctcn_wave_trim(waves.double(), table[:, :2].contiguous())
    with pytest.raises(ValueError, match="table"):
        ops.dctcn_wave_trim(waves, table)
    with pytest.raises(ValueError, match="must not be wave itself"):
        ops.dctcn_wave_trim(waves, table[:, :2].contiguous(), out=waves)


def test_restatement_layout():
    """The restatement itself on a case small enough to read: a window of the output size is a plain crop, the roll moves the mask with
    the frames, the neighbour of clip 0 is the last clip."""
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (2, 4, 6, 5), dtype=torch.uint8, generator=g)
    waves = torch.arange(16, dtype=torch.float32).repeat(2, 1) + 1.0
    table = torch.tensor([[1, 1, 4, 4, 1, 1, 3, 1, 2], [0, 0, 6, 5, 0, -1, 4, 0, 0]])
    audio = torch.tensor([[4, 12], [-4, 16]])
    out = pipeline_ref(frames, waves, [2, 2], table, audio, 4, 4)
    assert clip_sums(frames).shape == (2, 4) and int(clip_sums(frames)[1, 2]) == int(frames[1, 2].long().sum())
    v = out["videos"]
    assert v.shape == (2, 1, 4, 4, 4)
    m = (2.0 * frames[0].double().mean() / 255.0 - 1.0) / 255.0
    # clip 0: frames 1, 2 masked, rolled by +1 -> frames 2, 3; trunc 3 zeroes frame 3; frame 0 is stored frame 3, frame 1 stored frame 0
    assert (v[0, 0, 2] - (m - 0.421) / 0.165).abs().max() < 1e-12 and (v[0, 0, 3] - (0.0 - 0.421) / 0.165).abs().max() < 1e-12
    want = ((2.0 * frames[0, 3, 1:5, 1:5].double() / 255.0 - 1.0) / 255.0 - 0.421) / 0.165
    assert (v[0, 0, 0] - want.flip(-1)).abs().max() < 1e-12
    assert out["word_mask"].tolist() == [[0, 0, 1, 0], [1, 1, 0, 0]] and out["attention_mask"].tolist() == [[1, 1, 1, 0], [1, 1, 1, 1]]
    assert out["audios"][0].tolist() == [13.0, 14.0, 15.0, 16.0] + [float(i) for i in range(1, 9)] + [0.0] * 4
    assert out["audios"][1].tolist() == [float(i) for i in range(5, 17)] + [1.0, 2.0, 3.0, 4.0]
    mixed = pipeline_ref(frames, waves, [2, 2], table, audio, 4, 4, lam=0.25)["videos"]
    y1 = transform(mask_trim(frames[1], waves[1].double(), 2, -1, 4, 0, 0, -4, 16)[0], (0, 0, 6, 5, 0), 4, 4)
    assert (mixed[0, 0] - (0.75 * v[0, 0] + 0.25 * y1)).abs().max() < 1e-12 and (mixed[1, 0] - (0.75 * y1 + 0.25 * v[0, 0])).abs().max() < 1e-12


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    import ctypes

    from syncvsr_amd import _lib, build

    decl = _lib.parse_header()
    assert [n for _, n in decl["svsr_dctcn_clip_sums"]] == ["src_u8", "frame_sums", "B", "T", "Hs", "Ws", "max_blocks", "stream"]
    assert [n for _, n in decl["svsr_dctcn_clip_mix"]] == ["src_u8", "table", "frame_sums", "dst", "B", "T", "Hs", "Ws", "H", "W", "lam", "mean", "std",
                                                           "max_blocks", "stream"]
    assert [n for _, n in decl["svsr_dctcn_wave_trim"]] == ["wave", "table", "out", "B", "L", "max_blocks", "stream"]
    assert os.path.join(build.CSRC, "dctcn_prep.hip") in build.sources()          # the build picks the new file up
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    for name in ("svsr_dctcn_clip_sums", "svsr_dctcn_clip_mix", "svsr_dctcn_wave_trim"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert lib.svsr_steplist_knows(name.encode())
    # refused before anything is launched (no device needed)
    buf = ctypes.create_string_buffer(256)
    buf2 = ctypes.create_string_buffer(256)
    p, q = ctypes.addressof(buf), ctypes.addressof(buf2)
    sums = lambda *a: lib.svsr_dctcn_clip_sums(*a)          # noqa: E731
    assert sums(p, q, 1, 257, 4, 4, 0, None) == 1001          # T above the cap
    assert sums(p, q, 0, 1, 4, 4, 0, None) == 1001
    assert sums(p, q, 1, 1, 4097, 4096, 0, None) == 1001          # Hs * Ws > 2^24: the sum could leave 32 bits
    assert sums(None, q, 1, 1, 4, 4, 0, None) == 1001
    assert sums(p, None, 1, 1, 4, 4, 0, None) == 1001
    assert sums(p, q, 1, 1, 4, 4, -1, None) == 1001
    mix = lambda src=p, table=p, fs=None, dst=q, B=1, T=1, Hs=4, Ws=4, H=4, W=4, lam=0.0, mean=0.421, std=0.165, mb=0: \
        lib.svsr_dctcn_clip_mix(src, table, fs, dst, B, T, Hs, Ws, H, W, lam, mean, std, mb, None)          # noqa: E731
    for bad in (dict(T=257), dict(T=0), dict(B=0), dict(H=0), dict(W=0), dict(Hs=0), dict(Hs=4097, Ws=4096), dict(H=4097, W=4096), dict(std=0.0),
                dict(std=-1.0), dict(std=float("nan")), dict(lam=-0.1), dict(lam=0.6), dict(lam=float("nan")), dict(mb=-1), dict(src=None),
                dict(table=None), dict(dst=None)):
        assert mix(**bad) == 1001, bad
    trim = lambda wave=p, table=p, out=q, B=1, L=8, mb=0: lib.svsr_dctcn_wave_trim(wave, table, out, B, L, mb, None)          # noqa: E731
    for bad in (dict(B=0), dict(L=0), dict(L=(1 << 30) + 1), dict(mb=-1), dict(wave=None), dict(table=None), dict(out=None), dict(out=p)):
        assert trim(**bad) == 1001, bad
