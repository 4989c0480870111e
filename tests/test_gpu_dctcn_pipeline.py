"""-m gpu: the DC-TCN device input pipeline (csrc/dctcn_prep.hip: svsr_dctcn_clip_sums, svsr_dctcn_clip_mix, svsr_dctcn_wave_trim;
augment.DeviceDCTCNPipeline; DCTCNLightningModule.loss_and_backend_grads(videos_mixed=True)) against the fp64 restatement
tests/dctcn_pipeline_restatement.py.

Bounds.
  videos        |kernel - restatement| <= 2e-6 absolute.  The outputs are below 2.6 in magnitude, one fp32 ulp there is 2.4e-7, and at most about
                eight roundings act at that magnitude (the sample's three fused steps scaled down by 255 twice do not: the subtraction of the
                mean, the product with 1 / std, 1 / std itself, and with mixup the difference, its product and the sum).  One grey level of
                input moves the output by 2 / 255 / 255 / 0.165 = 1.9e-4, ninety times the bound; every case also asserts that the restatement
                with every shift off by one FAILS the same check, so the bound cannot hide a wrong frame.
  frame sums, waveforms, both masks    exact.
Every case prints its largest error before it asserts.  Measured on an MI355X: at most 2.1e-7 over all cases; a shift off by one is
off by 7.6e-3 at the least."""
from __future__ import annotations

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dctcn_pipeline_restatement import clip_sums, pipeline_ref  # noqa: E402
from lrw_pipeline_restatement import synthetic_frames  # noqa: E402

pytestmark = pytest.mark.gpu
MEAN, STD = 0.421, 0.165
BOUND = 2e-6
I32 = torch.int32
HS, WS = 12, 10


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _time_rows(T):
    """(shift, trunc, mask_off, mask_len, word length) of three clips; between them: shift negative, zero and positive; trunc = T - 1 and
    trunc = the word length; a mask of length 0; a run that ends on the last stored frame; masked frames the roll carries across the wrap
    (clip 2: stored frames T - 3 .. T - 1 land on T - 2, T - 1 — trimmed — and 0); a masked frame under the trim."""
    return [(-2, T - 1, T - 2, 2, 3), (0, 2, 1, 0, 2), (1, T - 1, T - 3, 3, 1)]


WINDOWS = {"crop": [(2, 1, 8, 8, 1), (0, 0, HS, WS, 0), (3, 2, 7, 6, 1)],          # 12 x 10 -> 8 x 8: a plain crop, the whole frame, a resized window
           "nocrop": [(0, 0, HS, WS, 0), (0, 0, HS, WS, 1), (0, 0, HS, WS, 0)]}    # the stored size: W = 10, no multiple of 4 -> scalar stores


@functools.lru_cache(maxsize=None)
def _case(B, T, geom, eval_chain=False):
    """-> (frames uint8 [B, T, 12, 10], table int32 [B, 9], word lengths, H, W); B = 1 takes clip 2's rows."""
    frames = synthetic_frames(B, T, HS, WS, 40 + T)
    pick = [2] if B == 1 else list(range(B))
    rows = _time_rows(T)
    table = torch.tensor([list(WINDOWS[geom][i]) + ([0, T, 0, 0] if eval_chain else list(rows[i][:4])) for i in pick], dtype=I32)
    H, W = (8, 8) if geom == "crop" else (HS, WS)
    return frames, table, [rows[i][4] for i in pick], H, W


@functools.lru_cache(maxsize=None)
def _ref(B, T, geom, lam, eval_chain=False, shift_off=0):
    frames, table, wbs, H, W = _case(B, T, geom, eval_chain)
    table = table.clone()
    table[:, 5] += shift_off
    waves, audio = torch.zeros(B, 4), torch.tensor([[0, 4]] * B)
    return pipeline_ref(frames, waves, wbs, table, audio, H, W, lam, MEAN, STD)["videos"]


def _mix(dev, frames, table, H, W, lam, max_blocks=0, offset=0, with_sums=True):
    """The two clip launches; dst pre-filled with NaN, `offset` elements into a larger buffer.  -> the batch on the host."""
    from syncvsr_amd import ops

    B, T = frames.shape[:2]
    f = frames.to(dev)
    sums = ops.dctcn_clip_sums(f, max_blocks) if with_sums else None
    n = B * T * H * W
    buf = torch.full((n + offset,), float("nan"), dtype=torch.float32, device=dev)
    out = buf[offset:].view(B, 1, T, H, W)
    assert out.data_ptr() % 16 == (4 * offset) % 16
    got = ops.dctcn_clip_mix(f, table.to(dev), H, W, sums, lam, MEAN, STD, max_blocks, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu()


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5])
@pytest.mark.parametrize("geom", ["crop", "nocrop"])
@pytest.mark.parametrize("B,T", [(3, 5), (1, 5), (3, 29)])
def test_clip_mix_against_restatement(dev, B, T, geom, lam):
    frames, table, _, H, W = _case(B, T, geom)
    ref = _ref(B, T, geom, lam)
    out = _mix(dev, frames, table, H, W, lam)
    assert out.shape == (B, 1, T, H, W) and out.dtype == torch.float32
    assert not torch.isnan(out).any(), "every element of dst is written"
    err = (out.double() - ref).abs().max().item()
    wrong = min((out.double() - _ref(B, T, geom, lam, shift_off=d)).abs().max().item() for d in (-1, 1))
    print(f"B{B} T{T} {geom} lam={lam}: max |kernel - fp64| {err:.3g} (bound {BOUND:.3g}); against a shift off by one {wrong:.3g}")
    assert err <= BOUND
    assert wrong > BOUND, "a restatement with the shift off by one must fail the same check"
    assert -2.58 < float(out.min()) and float(out.max()) < -2.52          # the reference's double division by 255: about [-2.575, -2.528]
    # trimmed frames are the constant (0 - mean) / std where no neighbour is mixed in; masked frames one constant
    if lam == 0.0:
        for b in range(B):
            trunc = int(table[b, 6])
            assert (out[b, 0, trunc:] == out[b, 0, trunc, 0, 0]).all() and abs(float(out[b, 0, trunc, 0, 0]) + MEAN / STD) <= BOUND
    for cap in (1, 3):
        assert torch.equal(_mix(dev, frames, table, H, W, lam, max_blocks=cap), out), ("max_blocks", cap)
    # an unaligned dst: the scalar-store fallback gives the same bits
    assert torch.equal(_mix(dev, frames, table, H, W, lam, offset=1), out)
    assert torch.equal(_mix(dev, frames, table, H, W, lam), out), "two runs give identical bits"


@pytest.mark.parametrize("geom", ["crop", "nocrop"])
def test_eval_chain_and_lam_zero_read_no_sums(dev, geom):
    """validation=True: shift 0, trunc T, no mask, lam 0 — and no frame sums are needed, so none are passed."""
    for B, T in ((3, 5), (1, 29)):
        frames, table, _, H, W = _case(B, T, geom, True)
        out = _mix(dev, frames, table, H, W, 0.0, with_sums=False)
        err = (out.double() - _ref(B, T, geom, 0.0, True)).abs().max().item()
        print(f"eval B{B} T{T} {geom}: max |kernel - fp64| {err:.3g}")
        assert not torch.isnan(out).any() and err <= BOUND
        assert (out.double() - _ref(B, T, geom, 0.0, True, 1)).abs().max().item() > BOUND


def test_wild_tables_are_clamped(dev):
    """Whatever the table holds, nothing outside the clips is read: every entry acts as its clamped (shift: reduced) value."""
    B, T, H, W = 3, 5, 8, 8
    frames = synthetic_frames(B, T, HS, WS, 9)
    wild = torch.tensor([[-3, -2, 99, 99, 1, 1000, 99, -5, 99], [5, 4, 3, 2, 0, -7, -3, 99, 4], [11, 9, 50, 50, 7, -2147483648, 4, 3, 2147483647]], dtype=I32)
    tame = torch.tensor([[0, 0, HS, WS, 1, 0, T, 0, T], [5, 4, 3, 2, 0, 3, 0, T, 0], [11, 9, 1, 1, 7, -3, 4, 3, 2]], dtype=I32)
    for lam in (0.0, 0.3):
        a, b = _mix(dev, frames, wild, H, W, lam), _mix(dev, frames, tame, H, W, lam)
        assert not torch.isnan(a).any() and torch.equal(a, b)


def test_frame_sums_are_exact(dev):
    from syncvsr_amd import ops

    for B, T, Hs, Ws in ((3, 5, 12, 10), (2, 29, 7, 9), (1, 3, 96, 96)):          # 120 and 9216 pixels: word loads; 63: byte loads
        frames = synthetic_frames(B, T, Hs, Ws, 3)
        frames[0, 0] = 255                                                      # the largest sum of the shape
        want = clip_sums(frames)
        for cap in (0, 1):
            got = ops.dctcn_clip_sums(frames.to(dev), cap)
            assert got.dtype == I32 and torch.equal(got.cpu().to(torch.int64) & 0xFFFFFFFF, want), (B, T, Hs, Ws, cap)
        # a source that is not 4-byte aligned takes the byte loads
        buf = torch.zeros(frames.numel() + 1, dtype=torch.uint8, device=dev)
        view = buf[1:].view(frames.shape)
        view.copy_(frames)
        assert view.data_ptr() % 4 == 1 and torch.equal(ops.dctcn_clip_sums(view).cpu().to(torch.int64), want)


def test_wave_trim_is_exact(dev):
    from syncvsr_amd import ops

    for L in (1003, 1000, 3):          # scalar stores, vector stores, a row shorter than one quad
        B = 4
        wave = torch.randn(B, L, generator=torch.Generator().manual_seed(L))
        table = torch.tensor([[-103, L - 35], [0, L], [68, 0], [-(L + 5), L + 9]], dtype=I32)      # shifts of both signs and past L; nothing, all kept
        want = torch.stack([torch.roll(wave[b], int(table[b, 0]), 0) for b in range(B)])
        for b in range(B):
            want[b, max(int(table[b, 1]), 0):] = 0
        got = ops.dctcn_wave_trim(wave.to(dev), table.to(dev))
        assert torch.equal(got.cpu(), want), L
        for cap in (1, 2):
            assert torch.equal(ops.dctcn_wave_trim(wave.to(dev), table.to(dev), cap).cpu(), want), (L, cap)
        buf = torch.full((B * L + 1,), float("nan"), dtype=torch.float32, device=dev)
        out = buf[1:].view(B, L)
        assert torch.equal(ops.dctcn_wave_trim(wave.to(dev), table.to(dev), out=out).cpu(), want), (L, "unaligned out")


def _counts(launched):
    return {k: v["launches"] for k, v in launched.items()}


def test_pipeline_outputs_and_launch_counts(dev):
    import numpy as np

    from syncvsr_amd import ops
    from syncvsr_amd.augment import DeviceDCTCNPipeline

    B, T, L = 3, 29, 1000
    frames = synthetic_frames(B, T, HS, WS, 21)
    waves = torch.randn(B, L, generator=torch.Generator().manual_seed(2))
    labels, wbs = torch.tensor([4, 1, 7]), torch.tensor([1, 5, 28])
    fd, wd, ld = frames.to(dev), waves.to(dev), labels.to(dev)
    pipe = DeviceDCTCNPipeline(8, seed=3, use_rrc=True)
    np.random.seed(11)
    plan = pipe.plan(B, T, HS, WS, L, wbs)
    assert bool((plan["time"][:, 3] > 0).any()), "the seeded plan masks nothing: the case shows nothing"
    lam = 0.3
    ops.start_event_timing()
    batch = pipe(fd, wd, ld, wbs, lam=lam, plan=plan)
    assert _counts(ops.stop_event_timing()) == {"k_dctcn_clip_sums": 1, "k_dctcn_clip_mix": 1, "k_dctcn_wave_trim": 1}
    assert list(batch) == ["videos", "audios", "labels", "word_mask", "attention_mask"] and batch["labels"] is ld
    table = torch.cat([plan["params"], plan["time"]], dim=1)
    ref = pipeline_ref(frames, waves, wbs.tolist(), table, plan["audio"], 8, 8, lam, MEAN, STD)
    err = (batch["videos"].cpu().double() - ref["videos"]).abs().max().item()
    print(f"pipeline, masked, trimmed and mixed: max |kernel - fp64| {err:.3g}")
    assert batch["videos"].shape == (B, 1, T, 8, 8) and err <= BOUND
    assert torch.equal(batch["audios"].cpu().double(), ref["audios"])
    for k in ("word_mask", "attention_mask"):
        assert batch[k].dtype == torch.int64 and batch[k].device.type == "cuda" and torch.equal(batch[k].cpu(), ref[k]), k
    assert bool(batch["word_mask"].any()) and not bool(batch["attention_mask"].all())
    # no clip masks anything: the sums launch is left out
    time0 = plan["time"].clone()
    time0[:, 3] = 0
    ops.start_event_timing()
    b0 = pipe(fd, wd, ld, wbs, lam=lam, plan=dict(plan, time=time0))
    assert _counts(ops.stop_event_timing()) == {"k_dctcn_clip_mix": 1, "k_dctcn_wave_trim": 1}
    table0 = torch.cat([plan["params"], time0], dim=1)
    assert (b0["videos"].cpu().double() - pipeline_ref(frames, waves, wbs.tolist(), table0, plan["audio"], 8, 8, lam, MEAN, STD)["videos"]).abs().max().item() <= BOUND
    # a drawn plan, use_rrc off: the stored size comes out
    np.random.seed(5)
    assert DeviceDCTCNPipeline(8, seed=3)(fd, wd, ld, wbs)["videos"].shape == (B, 1, T, HS, WS)
    # the eval chain: one launch, the waveforms pass through, full masks
    ev = DeviceDCTCNPipeline(8, train=False)
    ops.start_event_timing()
    be = ev(fd, wd, ld, wbs)
    assert _counts(ops.stop_event_timing()) == {"k_dctcn_clip_mix": 1}
    assert be["audios"] is wd and bool(be["attention_mask"].all()) and be["videos"].shape == (B, 1, T, 8, 8)
    pe = ev.plan(B, T, HS, WS, L, wbs)
    want = pipeline_ref(frames, waves, wbs.tolist(), torch.cat([pe["params"], pe["time"]], dim=1), pe["audio"], 8, 8, 0.0, MEAN, STD)
    assert (be["videos"].cpu().double() - want["videos"]).abs().max().item() <= BOUND and torch.equal(be["word_mask"].cpu(), want["word_mask"])


def _model(cfg, sd, dev):
    from syncvsr_amd.dctcn import DCTCNLightningModule

    m = DCTCNLightningModule(cfg)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def test_module_takes_mixed_videos(dev):
    """videos_mixed=True on torch.lerp(v, v.roll(1, 0), lam) is the lam call on v, bit for bit: metrics and every back-end gradient."""
    from dctcn_cases import dctcn_subcase

    cfg, _, sd, batch = dctcn_subcase("dctcn_tiny", "nowb_t7")
    v, tok, lab, wm, am = (t.to(dev) for t in batch)
    lam = 0.3
    a = _model(cfg, sd, dev)
    out_a = a.loss_and_backend_grads(v, tok, lab, wm, am, train_stats=True, dropout_seed=1, lam=lam)
    b = _model(cfg, sd, dev)
    out_b = b.loss_and_backend_grads(torch.lerp(v, v.roll(1, 0), lam), tok, lab, wm, am, train_stats=True, dropout_seed=1, lam=lam, videos_mixed=True)
    torch.cuda.synchronize()
    assert set(out_a) == set(out_b)
    for k in out_a:
        assert torch.equal(out_a[k], out_b[k]), k
    pa, pb = a.backend_parameters(), b.backend_parameters()
    assert len(pa) == len(pb) > 0
    for x, y in zip(pa, pb):
        assert x.grad is not None and torch.equal(x.grad, y.grad)
    # the videos are NOT mixed a second time: without the flag the already-mixed clips give other losses
    c = _model(cfg, sd, dev)
    out_c = c.loss_and_backend_grads(torch.lerp(v, v.roll(1, 0), lam), tok, lab, wm, am, train_stats=True, dropout_seed=1, lam=lam)
    assert not torch.equal(out_c["loss_total"], out_a["loss_total"])
    with pytest.raises(ValueError, match="videos_mixed"):
        a.loss_and_backend_grads(v, tok, lab, wm, am, videos_mixed=True)


def test_pipeline_batch_through_the_module(dev):
    """End to end: stored uint8 crops and waveforms -> the pipeline's dict -> loss_and_backend_grads(videos_mixed=True), the waveforms tokenised
    by the attached vq codec behind the trim."""
    import numpy as np

    import vq_codec_ref as R
    from dctcn_cases import dctcn_subcase
    from syncvsr_amd.audio_codec import VqWav2VecCodec
    from syncvsr_amd.augment import DeviceDCTCNPipeline

    cfg, _, sd, batch = dctcn_subcase("dctcn_tiny", "nowb_t7")
    B, T, size = batch[0].shape[0], batch[0].shape[2], int(cfg.data.input_size)
    model = _model(cfg, sd, dev)
    model.attach_audio_codec(VqWav2VecCodec.from_state_dict(R.seeded_model(1, False).state_dict(), R.fairseq_args(combine_groups=False)).to(dev))
    frames = synthetic_frames(B, T, size, size, 31).to(dev)
    waves = R.synthetic_waveform(B, 640 * T + 305, 8).to(dev)
    cfg.data.max_time_masks = 4          # (T = 7: the shipped 15 does not fit such a clip)
    pipe = DeviceDCTCNPipeline.from_config(cfg, train=True, seed=2)
    np.random.seed(4)
    lam = DeviceDCTCNPipeline.draw_lam(float(cfg.optim.mixup_alpha))
    assert 0.0 < lam <= 0.5
    out = pipe(frames, waves, batch[2].to(dev), [2, 3, 5], lam=lam)
    assert out["videos"].shape == (B, 1, T, size, size) and out["audios"].shape == waves.shape
    metrics = model.loss_and_backend_grads(**out, train_stats=True, dropout_seed=1, lam=lam, videos_mixed=True)
    torch.cuda.synchronize()
    print({k: float(v) for k, v in metrics.items()})
    assert all(bool(torch.isfinite(v).all()) for v in metrics.values())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.backend_parameters())
