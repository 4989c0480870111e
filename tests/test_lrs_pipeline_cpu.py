"""Host side of the LRS device input pipeline (no GPU): the draws of lrs_data.DeviceLRSPipeline against the reference's distributions
(LRS/video/datamodule/transforms.py), lrs_data.collate_packed against collate_pad, the restatement's own arithmetic
(tests/lrs_pipeline_restatement.py), and the C ABI of the two entry points (declared, exported, recordable, argument checks that return
before any launch)."""
import math
import os

import numpy as np
import pytest
import torch

from lrs_pipeline_restatement import audio_ref, snr_scale, synthetic_clips, synthetic_wave, video_ref

LEVELS = (-5, 0, 5, 10, 15, 20, 999999)
LO, HI = 96 / 112, 112 / 96


def _pipe(**kw):
    from syncvsr_amd.lrs_data import DeviceLRSPipeline

    return DeviceLRSPipeline(**kw)


def test_windows_lie_inside_and_follow_scale_and_ratio():
    pipe = _pipe(train=True, seed=3)
    for Hs, Ws in ((96, 96), (97, 101), (112, 96)):
        p = pipe.draw([5] * 400, Hs, Ws)["params"].numpy().astype(np.int64)
        top, left, h, w, flip = p.T
        assert (top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all()
        assert (top + h <= Hs).all() and (left + w <= Ws).all() and set(flip.tolist()) <= {0, 1}
        # w and h are sqrt(area * ratio) and sqrt(area / ratio) rounded to integers: each is within 0.5 of a pair that meets both bounds
        # (for these frame shapes the central fallback is the whole frame or a crop of an admissible ratio, which meets them as well)
        slack = 0.5 * (w + h) + 0.25
        assert (w * h >= 0.7 * Hs * Ws - slack).all() and (w * h <= Hs * Ws).all()
        assert ((w + 0.5) / (h - 0.5) >= LO).all() and ((w - 0.5) / (h + 0.5) <= HI).all()
        assert len({(int(a), int(b)) for a, b in zip(h, w)}) > 50          # they are drawn, not one constant


def test_fallback_for_a_frame_no_try_fits():
    """96 x 10: every admissible window (area >= 0.7 * 960, ratio >= 96/112) is at least 24 wide, so all ten tries are rejected and the
    central crop of the nearest admissible ratio is taken (RandomResizedCrop.get_params)."""
    p = _pipe(train=True, seed=0).draw([3] * 50, 96, 10)["params"]
    assert (p[:, :4] == torch.tensor([(96 - 12) // 2, 0, 12, 10], dtype=torch.int32)).all()          # w = Ws, h = round(Ws / (96 / 112)) = 12
    p = _pipe(train=True, seed=0).draw([3] * 50, 10, 96)["params"]
    assert (p[:, :4] == torch.tensor([0, (96 - 12) // 2, 10, 12], dtype=torch.int32)).all()          # h = Hs, w = round(Hs * (112 / 96)) = 12


def test_flip_and_snr_level_frequencies():
    n = 2000
    noise = torch.zeros(5000)
    d = _pipe(train=True, seed=11, noise=noise).draw([4] * n, 96, 96, [1000] * n)
    flips = int(d["params"][:, 4].sum())
    assert abs(flips - n * 0.5) <= 4 * math.sqrt(n * 0.25), flips
    p = 1 / len(LEVELS)
    for level in LEVELS:
        k = int((d["snr_db"] == level).sum())
        assert abs(k - n * p) <= 4 * math.sqrt(n * p * (1 - p)), (level, k)
    assert int(sum((d["snr_db"] == v).sum() for v in LEVELS)) == n


def test_noise_segments_lie_inside_the_bank():
    Nn = 3000
    rng = np.random.default_rng(0)
    alens = rng.integers(1, Nn + 1, 500).tolist() + [Nn, 1]
    d = _pipe(train=True, seed=5, noise=torch.zeros(Nn)).draw([4] * len(alens), 96, 96, alens)
    start = d["nstart"].long()
    assert (start >= 0).all() and (start + torch.tensor(alens) <= Nn).all()
    assert int(start[-2]) == 0 and len(set(start.tolist())) > 100          # a waveform as long as the bank has one place; the others move
    with pytest.raises(ValueError, match="noise bank"):
        _pipe(train=True, noise=torch.zeros(Nn)).draw([4], 96, 96, [Nn + 1])


class _Scripted:
    """Stands in for the generator: hands out a written randint table and written starts, and records the bounds it was asked for."""

    def __init__(self, table, starts):
        self.table, self.starts, self.bounds = np.array(table, dtype=np.int64).reshape(-1, 2), list(starts), []

    def integers(self, lo, hi, size=None):
        if size is not None:
            assert (lo, hi) == (0, 10) and tuple(size) == self.table.shape, (lo, hi, size)
            return self.table
        self.bounds.append((lo, hi))
        return self.starts.pop(0)


# (T, the randint(0, window, (n_mask, 2)) table, the randrange results) -> (bounds the starts are drawn from, runs, zeroed frames), worked out
# by hand from AdaptiveTimeMask.forward as the reference writes it (LRS/video/datamodule/transforms.py:50-64): a row is (t, t_end);
# `if length - t <= 0: continue`; `t_start = randrange(0, length - t)`; `if t_start == t_start + t: continue`; `cloned[t_start:t_start + t_end] = 0`
HAND_MASKS = [
    (26, [[3, 0], [20, 9]], [5, 4], [(0, 23), (0, 6)], [(5, 0), (4, 9)], list(range(4, 13))),      # a zero-length run masks nothing; the length is not t
    (26, [[1, 9], [0, 5]], [24, 7], [(0, 25), (0, 26)], [(24, 9)], [24, 25]),                      # cut at T by the slice; t == 0 is skipped AFTER its start is drawn
    (5, [[7, 3]], [], [], [], []),                                                                 # T - t < 0: skipped before a start is drawn
    (5, [[5, 3]], [], [], [], []),                                                                 # T - t == 0 likewise
    (24, [[9, 9]], [14], [(0, 15)], [(14, 9)], list(range(14, 23))),                               # the latest start t allows: the run may still reach past start + t
    (155, [[1, 1]] * 7, [0, 10, 20, 30, 40, 50, 154 - 1], [(0, 154)] * 7, [(0, 1), (10, 1), (20, 1), (30, 1), (40, 1), (50, 1), (153, 1)],
     [0, 10, 20, 30, 40, 50, 153]),
]


@pytest.mark.parametrize("T,table,starts,bounds,runs,zeroed", HAND_MASKS)
def test_time_mask_runs_against_the_reference_by_hand(T, table, starts, bounds, runs, zeroed):
    pipe = _pipe(train=True, time_mask=(10, 25))
    pipe.rng = _Scripted(table, starts)
    assert pipe._mask_runs(T) == runs and pipe.rng.bounds == bounds and not pipe.rng.starts
    pipe = _pipe(train=True, seed=1, time_mask=(10, 25))
    pipe._mask_runs = lambda length: runs
    tmask = pipe.draw([T], 96, 96, pad_frames_to=T + 12)["tmask"]          # a bucket bound above T: a run is cut at T, not at the bound
    assert tmask.shape == (1, T + 12) and tmask[0].nonzero().flatten().tolist() == zeroed


@pytest.mark.parametrize("T,n_mask", [(1, 1), (24, 1), (25, 1), (26, 2), (155, 7)])
def test_time_mask_run_count_and_distribution(T, n_mask):
    """n_mask = int((T + stride - 0.1) // stride) rows per clip.  A row survives unless t == 0 or t >= T, the run length is the table's second
    column — uniform on 0..9 whatever t is — and the frames zeroed are those of `cloned[t_start:t_start + t_end] = 0`."""
    assert int((T + 25 - 0.1) // 25) == n_mask
    seeds, lengths, kept, past = 400, [], 0, 0
    for seed in range(seeds):
        d = _pipe(train=True, seed=seed, time_mask=(10, 25)).draw([T], 96, 96)
        runs = d["runs"][0]
        assert len(runs) <= n_mask
        cloned = torch.ones(T)
        for start, n in runs:
            assert 0 <= start < T and 0 <= n <= 9
            cloned[start:start + n] = 0
            past += start + n > T
        assert torch.equal(d["tmask"][0], (cloned == 0).to(torch.uint8))
        kept += len(runs)
        lengths += [n for _, n in runs]
    rows = seeds * n_mask
    p_keep = sum(1 for t in range(1, 10) if t < T) / 10                      # t uniform on 0..9; t == 0 and t >= T are skipped
    assert abs(kept - rows * p_keep) <= 4 * math.sqrt(rows * p_keep * (1 - p_keep)) + 1e-9, (kept, rows * p_keep)
    if T == 1:
        assert kept == 0
        return
    for v in range(10):
        k = lengths.count(v)
        assert abs(k - kept * 0.1) <= 4 * math.sqrt(kept * 0.09), (v, k, kept)
    assert past > 0 if T <= 26 else True                                     # short clips: some run is cut at T


def test_eval_draws():
    d = _pipe(train=False, noise=torch.zeros(100), time_mask=(10, 25)).draw([3, 4], 100, 120, [50, 60])
    assert d["params"].tolist() == [[0, 0, 100, 120, 0]] * 2 and d["tmask"] is None and d["runs"] == [[], []]
    assert d["snr_db"].tolist() == [999999.0] * 2              # no snr_target: no noise
    d = _pipe(train=False, center_crop=True).draw([3], 100, 120)
    assert d["params"].tolist() == [[2, 12, 96, 96, 0]]
    d = _pipe(train=False, noise=torch.zeros(100), snr_target=5).draw([3, 4], 96, 96, [50, 100])
    assert d["snr_db"].tolist() == [5.0, 5.0] and int(d["nstart"][1]) == 0
    with pytest.raises(ValueError):
        _pipe(train=False, center_crop=True).draw([3], 90, 120)


def _samples(lens, alens, Hs=12, Ws=10, i16=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    clips = synthetic_clips(lens, Hs, Ws, seed)
    out = []
    for i, (c, S) in enumerate(zip(clips, alens)):
        a = torch.randn(S, generator=g) * 0.1
        out.append({"input": c, "audio": (a * 32768).to(torch.int16) if i16 else a, "target": torch.randint(1, 40, (2 + 3 * i,), generator=g)})
    return out


def test_collate_packed_layout_and_targets():
    from syncvsr_amd.lrs_data import collate_pad, collate_packed

    lens, alens = [3, 1, 5], [1900, 640, 3200]
    batch = _samples(lens, alens)
    p = collate_packed(batch, pin=False)
    assert p["offsets"].tolist() == [0, 3, 4, 9] and p["offsets"].dtype == torch.int32 and p["input_lengths"].tolist() == lens
    assert p["frames"].shape == (9, 12, 10) and p["frames"].dtype == torch.uint8 and p["pad_frames"] == 5
    for b, s in enumerate(batch):
        assert torch.equal(p["frames"][p["offsets"][b]: p["offsets"][b + 1]], s["input"])
        assert torch.equal(p["audios"][b, : alens[b]], s["audio"]) and not p["audios"][b, alens[b]:].any()
    assert p["audios"].shape == (3, 3200) and p["audio_lengths"].tolist() == alens
    ref = collate_pad(batch)
    assert torch.equal(p["targets"], ref["targets"]) and torch.equal(p["target_lengths"], ref["target_lengths"])
    assert torch.equal(p["input_lengths"], ref["input_lengths"]) and torch.equal(p["audio_lengths"], ref["audio_lengths"])
    # the bucket bound: frames and samples padded to it, targets to a multiple
    p = collate_packed(batch, pad_frames_to=8, pad_targets_to_multiple=16, pin=False)
    ref = collate_pad(batch, pad_frames_to=8, frames_per_unit={"audio": 640}, pad_targets_to_multiple=16)
    assert p["pad_frames"] == 8 and p["audios"].shape == (3, 8 * 640) == ref["audios"].shape[::2]
    assert torch.equal(p["targets"], ref["targets"]) and p["targets"].shape == (3, 1, 16)
    # [T, 1, Hs, Ws] clips and int16 samples pass through as they are
    b16 = _samples(lens, alens, i16=True)
    for s in b16:
        s["input"] = s["input"].unsqueeze(1)
    p16 = collate_packed(b16, pin=False)
    assert p16["audios"].dtype == torch.int16 and p16["frames"].shape == (9, 12, 10)


def test_collate_packed_leaves_cuda_alone_in_a_loader_worker(monkeypatch):
    """As the collate_fn of a DataLoader with workers it runs in a worker process: no CUDA query (a forked worker cannot initialise it) and no
    pinned allocation there — DataLoader(pin_memory=True) pins the batch in the parent."""
    import torch.utils.data

    from syncvsr_amd.lrs_data import collate_packed

    def no_cuda():
        raise AssertionError("torch.cuda was queried from a worker")

    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    monkeypatch.setattr(torch.cuda, "is_available", no_cuda)
    p = collate_packed(_samples([2, 3], [640, 700]))
    assert not p["frames"].is_pinned() and not p["audios"].is_pinned()
    loader = torch.utils.data.DataLoader(_samples([2, 3, 1, 2], [640, 700, 640, 650]), batch_size=2, collate_fn=collate_packed)
    assert [b["offsets"].tolist() for b in loader] == [[0, 2, 5], [0, 1, 3]]          # (in process here; the dictionary passes through the loader as it is)


def test_collate_packed_refuses():
    from syncvsr_amd.lrs_data import collate_packed

    batch = _samples([2, 3], [640, 700])
    batch[1]["input"] = synthetic_clips([3], 12, 11, 1)[0]
    with pytest.raises(ValueError, match="stored frame size"):
        collate_packed(batch, pin=False)
    batch = _samples([2, 3], [640, 700])
    with pytest.raises(ValueError, match="longest clip"):
        collate_packed(batch, pad_frames_to=2, pin=False)
    with pytest.raises(ValueError, match="longer than"):
        collate_packed(_samples([1, 1], [640, 700]), pad_frames_to=1, pin=False)
    batch[0]["input"] = batch[0]["input"].float()
    with pytest.raises(ValueError, match="uint8"):
        collate_packed(batch, pin=False)


def test_restatement_at_0_db_mixes_noise_of_the_signals_energy():
    g = torch.Generator().manual_seed(2)
    x, n = torch.randn(5000, generator=g, dtype=torch.float64) * 0.05 + 0.01, torch.randn(5000, generator=g, dtype=torch.float64) * 3.0
    s = snr_scale(x, n, 0.0)
    assert abs(float((s * n).pow(2).sum() / x.pow(2).sum()) - 1.0) < 1e-12
    assert abs(float((snr_scale(x, n, 20.0) * n).pow(2).sum() / x.pow(2).sum()) - 0.01) < 1e-12
    for dt in (torch.float32, torch.float64):                 # the reference's clean level: an exact zero, nothing infinite on the way
        assert float(snr_scale(x.to(dt), n.to(dt), 999999)) == 0.0
    assert float(snr_scale(x, torch.zeros_like(n), 5.0)) == 0.0 and float(snr_scale(torch.zeros_like(x), n, 5.0)) == 0.0


def test_restatement_audio_and_video_layouts():
    wave = synthetic_wave([100, 300], 320, 1)
    noise = synthetic_wave([1000], 1000, 2, amplitude=1.0)[0]
    out = audio_ref(wave, [100, 300], noise, [5, 700], [5.0, 999999.0])
    assert not out[0, 100:].any() and not out[1, 300:].any()
    for b, L in enumerate((100, 300)):
        assert abs(float(out[b, :L].mean())) < 1e-12 and abs(float(out[b, :L].pow(2).mean()) - 1.0) < 1e-4
    assert torch.equal(out[1], audio_ref(wave, [100, 300])[1])          # 999999 dB is the noise-free transform
    i16 = (wave * 32768).round().clamp(-32768, 32767).to(torch.int16)
    assert torch.equal(audio_ref(i16, [100, 300]), audio_ref(i16.float() / 32768.0, [100, 300]))
    clips = synthetic_clips([2, 3], 12, 12, 0)
    tmask = torch.zeros(2, 4, dtype=torch.uint8)
    tmask[1, 1] = 1
    v = video_ref(clips, torch.tensor([[0, 0, 12, 12, 0], [1, 2, 9, 8, 1]], dtype=torch.int32), 4, 12, tmask=tmask)
    assert v.shape == (2, 4, 1, 12, 12) and not v[0, 2:].any() and not v[1, 3:].any()
    assert torch.equal(v[0, :2, 0], (clips[0].double() / 255.0 - 0.421) / 0.165)          # the identity window is a plain crop
    assert (v[1, 1] == -0.421 / 0.165).all() and not (v[1, 0] == -0.421 / 0.165).all()


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    import ctypes

    from syncvsr_amd import _lib, build

    decl = _lib.parse_header()
    assert [n for _, n in decl["svsr_lrs_clip_prep"]] == ["src_u8", "total_frames", "off", "params", "tmask", "dst", "B", "Tpad", "Hs", "Ws", "H", "W",
                                                          "mean", "std", "max_blocks", "stream"]
    assert [n for _, n in decl["svsr_wave_prep"]] == ["wave", "wave_i16", "len", "noise", "Nn", "nstart", "snr_db", "out", "B", "Spad", "eps", "ws",
                                                      "ws_bytes", "max_blocks", "stream"]
    assert _lib._RESTYPE["svsr_wave_prep_ws_bytes"] == "int64_t"
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    for name in ("svsr_lrs_clip_prep", "svsr_wave_prep"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert lib.svsr_steplist_knows(name.encode())
    assert not lib.svsr_steplist_knows(b"svsr_wave_prep_ws_bytes")          # a host-side query
    assert lib.svsr_wave_prep_ws_bytes(2, 9300) == 2 * 3 * 5 * 8 and lib.svsr_wave_prep_ws_bytes(1, 4096) == 40 and lib.svsr_wave_prep_ws_bytes(0, 5) == 0
    # refused before anything is launched (no device needed): null buffers, a workspace too small, a non-positive std
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    assert lib.svsr_wave_prep(None, 0, p, None, 0, None, None, p, 1, 8, 1e-8, p, 40, 0, None) == 1001
    assert lib.svsr_wave_prep(p, 0, p, None, 0, None, None, p, 1, 8, 1e-8, p, 39, 0, None) == 1001
    assert lib.svsr_wave_prep(p, 0, p, p, 8, None, p, p, 1, 8, 1e-8, p, 40, 0, None) == 1001
    assert lib.svsr_lrs_clip_prep(p, 1, p, p, None, p, 1, 1, 4, 4, 4, 4, 0.421, 0.0, 0, None) == 1001
    assert lib.svsr_lrs_clip_prep(p, 1, None, p, None, p, 1, 1, 4, 4, 4, 4, 0.421, 0.165, 0, None) == 1001
    assert lib.svsr_lrs_clip_prep(p, 1, p, p, None, p, 1, 0, 4, 4, 4, 4, 0.421, 0.165, 0, None) == 1001
