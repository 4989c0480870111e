"""-m gpu: the LRS device input pipeline (csrc/lrs_prep.hip: svsr_lrs_clip_prep, svsr_wave_prep; lrs_data.DeviceLRSPipeline) against the fp64
torch restatement tests/lrs_pipeline_restatement.py, and through E2E.forward on the tiny LRS configuration.

Tolerances.
  video   the arithmetic is svsr_clip_prep's, so the bounds are the ones tests/test_gpu_misc.py::test_device_clip_pipeline uses for it: a resized
          window within 2e-5 * max(1, max |ref|), a plain crop (window = output size) within 1e-6 of (x / 255 - mean) / std in fp32.  Padding
          frames are exactly 0.0 and masked frames exactly fp32(-mean) / fp32(std).
  audio   the same formulas evaluated with torch in fp32 on the CPU are the reference's own arithmetic; their largest deviation from fp64 is
          measured per case and the kernel may deviate from fp64 by at most twice that, never asked below 1e-6 (_audio_bound).
  model   tests/test_gpu_lrs_model.py's bound for the tiny configuration (losses within 5e-3 relative, accuracy within 2 / live tokens) and
          tests/test_gpu_w2v_codec.py's token parity (equal wherever the top-1 margin of the logits exceeds 2 * 0.25).
Every case prints its figures before it asserts."""
from __future__ import annotations

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_codec_ref as R  # noqa: E402
from lrs_pipeline_restatement import audio_ref, mixed_ref, synthetic_clips, synthetic_wave, video_ref  # noqa: E402

pytestmark = pytest.mark.gpu
MEAN, STD = 0.421, 0.165
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _clip_prep(dev, clips, params, Tpad, size, tmask=None, max_blocks=0):
    from syncvsr_amd import ops

    off = [0]
    for c in clips:
        off.append(off[-1] + len(c))
    return ops.lrs_clip_prep(torch.cat(clips).to(dev), _i32(off, dev), params.to(dev), Tpad, size, size, MEAN, STD,
                             None if tmask is None else tmask.to(dev), max_blocks).cpu()


def _check_video(out, clips, params, Tpad, size, tmask=None, what=""):
    ref = video_ref(clips, params, Tpad, size, MEAN, STD, tmask)
    assert out.shape == ref.shape == (len(clips), Tpad, 1, size, size) and out.dtype == torch.float32
    err = (out.to(F64) - ref).abs().max().item()
    bound = 2e-5 * max(1.0, ref.abs().max().item())          # tests/test_gpu_misc.py::test_device_clip_pipeline
    print(f"{what}: max |kernel - fp64| {err:.3g} (bound {bound:.3g})")
    for b, c in enumerate(clips):
        assert not out[b, len(c):].any(), f"clip {b}: a padding frame is not exactly 0.0"
    assert err <= bound, (what, err, bound)


# ---- video ---------------------------------------------------------------------------------------------------------------------------
CLIPS_96 = synthetic_clips([1, 7, 12], 96, 96, 3)
PARAMS_96 = torch.tensor([[0, 0, 96, 96, 0], [5, 9, 84, 80, 1], [11, 2, 79, 90, 0]], dtype=torch.int32)      # the identity window, two that enlarge


def test_video_stored_96_to_96(dev):
    out = _clip_prep(dev, CLIPS_96, PARAMS_96, 16, 96)
    _check_video(out, CLIPS_96, PARAMS_96, 16, 96, what="96x96 -> 96")
    plain = (CLIPS_96[0].float() / 255.0 - MEAN) / STD
    assert (out[0, :1, 0] - plain).abs().max().item() < 1e-6          # a window of exactly H x W is a plain crop
    flipped = PARAMS_96.clone()
    flipped[:, 4] = 1 - flipped[:, 4]
    out_f = _clip_prep(dev, CLIPS_96, flipped, 16, 96)
    _check_video(out_f, CLIPS_96, flipped, 16, 96, what="96x96 -> 96, flips swapped")
    assert torch.equal(out_f[0, 0, 0], out[0, 0, 0].flip(-1))          # the flip mirrors the output


def test_video_time_mask(dev):
    tmask = torch.zeros(3, 16, dtype=torch.uint8)
    tmask[0, 0] = 1
    tmask[1, 2:5] = 1
    tmask[2, 11] = 1
    tmask[2, 13] = 1                                                   # (a padding frame: stays 0.0)
    plain = _clip_prep(dev, CLIPS_96, PARAMS_96, 16, 96)
    out = _clip_prep(dev, CLIPS_96, PARAMS_96, 16, 96, tmask=tmask)
    _check_video(out, CLIPS_96, PARAMS_96, 16, 96, tmask, what="96x96 -> 96, masked")
    fill = (torch.tensor(0.0) - torch.tensor(MEAN)) / torch.tensor(STD)          # -mean / std in fp32
    for b, c in enumerate(CLIPS_96):
        for t in range(16):
            if t < len(c) and tmask[b, t]:
                assert (out[b, t] == fill).all(), (b, t)
            else:
                assert torch.equal(out[b, t], plain[b, t]), (b, t)


@pytest.mark.parametrize("size", [24, 23])          # 24: 16-byte stores; 23: rows that are not 16-byte aligned take the pixel stores
def test_video_stored_97x101_shrinks(dev, size):
    clips = synthetic_clips([1, 7, 12], 97, 101, 5)
    params = torch.tensor([[0, 0, 97, 101, 1], [3, 7, 88, 93, 0], [20, 30, size, size, 1]], dtype=torch.int32)
    out = _clip_prep(dev, clips, params, 16, size)
    _check_video(out, clips, params, 16, size, what=f"97x101 -> {size}")
    plain = ((clips[2][:, 20:20 + size, 30:30 + size].float() / 255.0 - MEAN) / STD).flip(-1)
    assert (out[2, :12, 0] - plain).abs().max().item() < 1e-6


def test_video_output_that_is_not_16_byte_aligned(dev):
    """W % 4 == 0 but dst 4 bytes off a 16-byte boundary (never the case through ops.lrs_clip_prep, whose output is a fresh tensor): the C
    entry point must take the pixel stores and give the bits of the aligned call."""
    from syncvsr_amd import _lib, ops

    clips = synthetic_clips([2, 3], 30, 30, 41)
    params = torch.tensor([[1, 2, 27, 26, 1], [0, 0, 30, 30, 0]], dtype=torch.int32)
    want = _clip_prep(dev, clips, params, 4, 24)
    src, off, par = torch.cat(clips).to(dev), _i32([0, 2, 5], dev), params.to(dev)
    buf = torch.full((want.numel() + 2,), 7.0, device=dev)
    assert buf.data_ptr() % 16 == 0
    rc = _lib.load().svsr_lrs_clip_prep(src.data_ptr(), 5, off.data_ptr(), par.data_ptr(), None, buf.data_ptr() + 4, 2, 4, 30, 30, 24, 24, MEAN, STD, 0,
                                        ops._stream())
    assert rc == 0
    got = buf.cpu()
    assert torch.equal(got[1:-1].view_as(want), want) and got[0] == 7.0 and got[-1] == 7.0


def test_video_single_clips(dev):
    clips = synthetic_clips([5], 40, 36, 7)
    params = torch.tensor([[2, 1, 33, 31, 1]], dtype=torch.int32)
    _check_video(_clip_prep(dev, clips, params, 5, 24), clips, params, 5, 24, what="B = 1, Tpad = T")
    one = synthetic_clips([1], 40, 36, 8)
    _check_video(_clip_prep(dev, one, params, 1, 24), one, params, 1, 24, what="B = 1, one frame")


def test_video_agrees_with_the_lrw_kernel(dev):
    """Clips of one length: svsr_clip_prep's output, [B, 1, T, H, W], is this kernel's with the two axes swapped."""
    from syncvsr_amd import ops

    clips = synthetic_clips([6, 6], 96, 96, 9)
    params = torch.tensor([[4, 4, 88, 88, 0], [7, 0, 81, 96, 1]], dtype=torch.int32)
    out = _clip_prep(dev, clips, params, 6, 88)
    lrw = ops.clip_prep(torch.stack(clips).to(dev), params.to(dev), 88, 88, MEAN, STD).cpu().transpose(1, 2)
    d = (out - lrw).abs().max().item()
    print(f"svsr_lrs_clip_prep vs svsr_clip_prep: max |d| {d:.3g}, bit-identical: {torch.equal(out, lrw)}")
    assert d <= 2e-5 * max(1.0, lrw.abs().max().item())


def test_video_grid_stride_loop_and_determinism(dev):
    """3 x 155 frames: 465 items under a cap of 7 workgroups (67 trips, the last one partial); the result does not depend on the cap."""
    clips = synthetic_clips([155, 155, 155], 32, 30, 11)
    params = torch.tensor([[1, 2, 29, 27, 0], [0, 0, 32, 30, 1], [4, 3, 24, 24, 1]], dtype=torch.int32)
    tmask = torch.zeros(3, 155, dtype=torch.uint8)
    tmask[1, 100:104] = 1
    free = _clip_prep(dev, clips, params, 155, 24, tmask)
    capped = _clip_prep(dev, clips, params, 155, 24, tmask, max_blocks=7)
    _check_video(capped, clips, params, 155, 24, tmask, what="3 x 155 frames, 7 workgroups")
    assert torch.equal(free, capped) and torch.equal(free, _clip_prep(dev, clips, params, 155, 24, tmask))


# ---- audio ---------------------------------------------------------------------------------------------------------------------------
LENS = [100, 640 * 7 + 3, 9001]          # under two waves; odd; three partial rows of the first pass (one per 4096 samples): the fold runs
SPAD = 9300
NSTART = [17, 1000, 2999]
SNR = [-5.0, 20.0, 999999.0]
NOISE = synthetic_wave([12000], 12000, 21, amplitude=0.7)[0]


def _wave_prep(dev, wave, lens, noise=None, nstart=None, snr=None, max_blocks=0):
    from syncvsr_amd import ops

    if noise is None:
        return ops.wave_prep(wave.to(dev), _i32(lens, dev), max_blocks=max_blocks).cpu()
    return ops.wave_prep(wave.to(dev), _i32(lens, dev), noise.to(dev), _i32(nstart, dev), torch.tensor(snr, dtype=torch.float32, device=dev),
                         max_blocks=max_blocks).cpu()


def _audio_bound(wave, lens, noise=None, nstart=None, snr=None):
    """-> (fp64 restatement, deviation of the fp32 restatement from it, what the kernel may deviate)."""
    r64 = audio_ref(wave, lens, noise, nstart, snr, dtype=F64)
    r32 = audio_ref(wave, lens, noise, nstart, snr, dtype=torch.float32)
    dev32 = (r32.to(F64) - r64).abs().max().item()
    return r64, dev32, max(2.0 * dev32, 1e-6)


def _check_audio(out, wave, lens, noise=None, nstart=None, snr=None, what=""):
    r64, dev32, bound = _audio_bound(wave, lens, noise, nstart, snr)
    assert out.shape == r64.shape and out.dtype == torch.float32 and torch.isfinite(out).all()
    err = (out.to(F64) - r64).abs().max().item()
    print(f"{what}: max |kernel - fp64| {err:.3g}, max |torch fp32 - fp64| {dev32:.3g}, bound {bound:.3g}")
    for b, y in enumerate(mixed_ref(wave, lens, noise, nstart, snr)):
        L = len(y)
        assert not out[b, L:].any(), f"clip {b}: a padding sample is not exactly 0.0"
        if L:
            var = y.var(unbiased=False).item()
            span = out[b, :L].to(F64)
            print(f"  clip {b}: mean {span.mean().item():.3g}, mean square {span.pow(2).mean().item():.9f} (var / (var + eps) {var / (var + 1e-8):.9f})")
            assert abs(span.mean().item()) <= 1e-5 and abs(span.pow(2).mean().item() - var / (var + 1e-8)) <= 1e-4
    assert err <= bound, (what, err, bound)
    return err, dev32


def test_audio_noise_levels_fp32_and_int16(dev):
    i16 = (synthetic_wave(LENS, SPAD, 13, amplitude=0.2) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    wave = i16.float() / 32768.0
    out = _wave_prep(dev, wave, LENS, NOISE, NSTART, SNR)
    # measured on an MI355X (also in DESIGN.md section 3): kernel 1.19e-07 from fp64, torch fp32 4.82e-07, bound 1e-06 (the floor);
    # the DC-offset case below: kernel 1.19e-07, torch fp32 5.08e-05, bound 1.02e-04
    _check_audio(out, wave, LENS, NOISE, NSTART, SNR, what="fp32, -5 / 20 / 999999 dB")
    out16 = _wave_prep(dev, i16, LENS, NOISE, NSTART, SNR)
    assert torch.equal(out16, out), "int16 samples must give the bits of the fp32 samples v / 32768"
    clean = _wave_prep(dev, wave, LENS)
    _check_audio(clean, wave, LENS, what="fp32, no noise")
    assert torch.equal(out[2], clean[2]), "999999 dB must be bit-equal to noise = null"
    assert not torch.equal(out[0], clean[0]) and not torch.equal(out[1], clean[1])
    assert torch.equal(_wave_prep(dev, i16, LENS), clean)


def test_audio_dc_offset(dev):
    """Offset 0.5, amplitude 1e-3: E[y^2] - mean^2 cancels six digits.  The kernel stays inside the bound of every other case; the same
    formula accumulated in fp32 in one pass does not (shown on the CPU, so the case is known to bite)."""
    wave = synthetic_wave(LENS, SPAD, 17, offset=0.5, amplitude=1e-3)
    out = _wave_prep(dev, wave, LENS)
    _check_audio(out, wave, LENS, what="DC offset 0.5, amplitude 1e-3, no noise")
    out_n = _wave_prep(dev, wave, LENS, NOISE, NSTART, [60.0, 80.0, 999999.0])          # noise below the signal's ripple: the offset still dominates E[y^2]
    _check_audio(out_n, wave, LENS, NOISE, NSTART, [60.0, 80.0, 999999.0], what="DC offset, 60 / 80 / 999999 dB")
    r64, _, bound = _audio_bound(wave, LENS)
    for b, L in enumerate(LENS):
        y = wave[b, :L]
        m = y.mean()
        naive = (y - m) / torch.sqrt((y * y).mean() - m * m + 1e-8)
        d = (naive.to(F64) - r64[b, :L]).abs().max().item()
        print(f"  clip {b}: single-pass fp32 E[y^2] - mean^2 deviates by {d:.3g} (bound {bound:.3g})")
        assert not d <= bound


def test_audio_degenerate_energies(dev):
    """Ex = 0, En = 0 and both: scale is defined as 0, the noise-free normalisation; a silent clip stays 0.  Also a clip of length 0 and a
    noise segment that would leave the bank (never read: noise-free)."""
    wave = synthetic_wave([500, 700, 900, 0, 300], 1000, 19, amplitude=0.1)
    wave[0] = 0.0                                   # Ex = 0, En > 0
    wave[2] = 0.0                                   # Ex = 0 and En = 0
    lens = [500, 700, 900, 0, 300]
    noise = synthetic_wave([4000], 4000, 23, amplitude=0.5)[0]
    noise[1000:2000] = 0.0                          # En = 0 for clips 1 and 2
    nstart, snr = [0, 1100, 1050, 0, 3900], [5.0, 5.0, 5.0, 5.0, 5.0]          # clip 4: 3900 + 300 > 4000
    out = _wave_prep(dev, wave, lens, noise, nstart, snr)
    assert torch.isfinite(out).all()
    assert not out[0].any() and not out[2].any() and not out[3].any()
    clean = _wave_prep(dev, wave, lens)
    assert torch.equal(out, clean)
    _check_audio(out, wave, lens, noise, [0, 1100, 1050, 0, 0], [5.0, 5.0, 5.0, 5.0, 999999.0], what="degenerate energies")


def test_audio_is_bit_identical_across_runs_and_grids(dev):
    wave = synthetic_wave(LENS, SPAD, 29, offset=0.01, amplitude=0.3)
    a = _wave_prep(dev, wave, LENS, NOISE, NSTART, SNR)
    b = _wave_prep(dev, wave, LENS, NOISE, NSTART, SNR)
    c = _wave_prep(dev, wave, LENS, NOISE, NSTART, SNR, max_blocks=2)          # 9 items on 2 workgroups
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- the pipeline, and through the model ---------------------------------------------------------------------------------------------
EPS_LOGIT = 0.25          # tests/test_gpu_w2v_codec.py: a token must match wherever the top-1 margin exceeds 2 EPS


def _lrs(dev):
    from syncvsr_amd.audio_codec import Wav2Vec2Codec
    from syncvsr_amd.lrs_init import default_lrs_args, lrs_init_state_dict
    from syncvsr_amd.lrs_model import E2E

    args = default_lrs_args(adim=128, aheads=2, eunits=256, elayers=2, ddim=128, dheads=2, dunits=256, dlayers=1, codec="wav2vec2")
    model = E2E(41, args)
    model.load_state_dict(lrs_init_state_dict(args, 41, seed=7, perturb_norm=True))
    model.to(dev)
    model.attach_audio_codec(Wav2Vec2Codec.from_state_dict(R.seeded_weights("layer", 1), R.hf_config_kwargs("layer")).to(dev), sample_in_training=False)
    return model


def test_pipeline_through_the_model(dev):
    from syncvsr_amd import ops
    from syncvsr_amd.audio_codec import LRS_PAD
    from syncvsr_amd.lrs_data import DeviceLRSPipeline, collate_packed

    lens, Tpad, size = [9, 11], 12, 24
    g = torch.Generator().manual_seed(31)
    clips = synthetic_clips(lens, 32, 32, 33)
    samples = [{"input": c, "audio": R.synthetic_waveform(1, T * 640, 9 + i)[0, 0], "target": torch.randint(1, 40, (2 + 2 * i,), generator=g)}
               for i, (c, T) in enumerate(zip(clips, lens))]
    packed = collate_packed(samples, pad_frames_to=Tpad)
    noise = synthetic_wave([20000], 20000, 35, amplitude=0.3)[0]
    pipe = DeviceLRSPipeline(train=True, size=size, seed=4, noise=noise, time_mask=(10, 25))
    draws = pipe.draw(lens, 32, 32, packed["audio_lengths"].tolist(), Tpad)
    draws["snr_db"][0] = 5.0                                                     # one clip audibly noisy whatever the level draw was
    ops.start_event_timing()
    batch = pipe(packed, draws)
    launched = ops.stop_event_timing()
    assert {k: v["launches"] for k, v in launched.items()} == {"k_lrs_clip_prep": 1, "k_wave_prep": 1}          # (svsr_wave_prep: two launches in one call)
    assert set(batch) == {"inputs", "input_lengths", "audios", "audio_lengths", "targets", "target_lengths"}
    assert batch["inputs"].shape == (2, Tpad, 1, size, size) and batch["audios"].shape == (2, 1, Tpad * 640)
    assert batch["input_lengths"].tolist() == lens and batch["audio_lengths"].tolist() == [T * 640 for T in lens]

    alens = packed["audio_lengths"].tolist()
    _check_video(batch["inputs"].cpu(), clips, draws["params"], Tpad, size, draws["tmask"], what="pipeline video")
    _check_audio(batch["audios"][:, 0].cpu(), packed["audios"], alens, noise, draws["nstart"].tolist(), draws["snr_db"].tolist(), what="pipeline audio")
    x_ref = video_ref(clips, draws["params"], Tpad, size, MEAN, STD, draws["tmask"]).float().to(dev)
    a_ref = audio_ref(packed["audios"], alens, noise, draws["nstart"].tolist(), draws["snr_db"].tolist()).float().unsqueeze(1).to(dev)

    model = _lrs(dev).train()
    outs = []
    for x, a in ((batch["inputs"], batch["audios"]), (x_ref, a_ref)):
        model.reseed_dropout(5)
        outs.append([float(t.detach()) for t in model(x, batch["input_lengths"], a, batch["targets"])])
    torch.cuda.synchronize()
    print("pipeline:", outs[0], "restatement:", outs[1])
    assert len(outs[0]) == 5 and all(v == v for v in outs[0])
    for i, k in enumerate(("loss", "loss_ctc", "loss_att", "loss_audio")):
        assert abs(outs[0][i] - outs[1][i]) <= 5e-3 * abs(outs[1][i]), (k, outs[0][i], outs[1][i])
    n_live = int((packed["targets"] != -1).sum()) + len(lens)
    assert abs(outs[0][4] - outs[1][4]) <= 2.0 / n_live + 1e-6
    prepared = model.prepare_batch(batch["inputs"], batch["input_lengths"], batch["audios"], batch["targets"])          # what TrainStep records from
    assert prepared[0].data_ptr() == batch["inputs"].data_ptr() and prepared[2].shape == (2, Tpad * 640)

    # audio tokens: the pipeline's waveform and the restatement's through the same tokeniser, and the restatement alone against the CPU tokeniser
    rows = R.frames(Tpad * 640 + LRS_PAD)[-1]
    z = torch.empty(2 * rows, 640, dtype=torch.float32, device=dev)
    tok_ref = model.wav2vec(a_ref, pad=LRS_PAD, logits_out=z).cpu()
    tok = model.wav2vec(batch["audios"], pad=LRS_PAD).cpu()
    sure = R.margins(z.cpu().view(2, rows, 640)) > 2 * EPS_LOGIT
    print(f"tokens: {int((tok != tok_ref).sum())} of {tok.numel()} differ between the two waveforms, {int((~sure).sum())} positions are near-ties")
    assert torch.equal(tok[sure], tok_ref[sure])
    cpu_tok, cpu_z = R.tokenize(R.seeded_weights("layer", 1), "layer", a_ref.cpu(), pad=LRS_PAD)
    cpu_sure = R.margins(cpu_z) > 2 * EPS_LOGIT
    assert torch.equal(tok_ref[cpu_sure], cpu_tok[cpu_sure]) and torch.equal(tok[cpu_sure], cpu_tok[cpu_sure])


def test_pipeline_eval_and_refusals(dev):
    from syncvsr_amd.lrs_data import DeviceLRSPipeline, collate_packed

    lens = [3, 2]
    clips = synthetic_clips(lens, 30, 30, 37)
    i16 = [(synthetic_wave([T * 640], T * 640, 39 + T, amplitude=0.2)[0] * 32768).to(torch.int16) for T in lens]
    samples = [{"input": c.unsqueeze(1), "audio": a, "target": torch.tensor([3, 4])} for c, a in zip(clips, i16)]
    packed = collate_packed(samples)
    batch = DeviceLRSPipeline(train=False, size=24)(packed)                       # full frame resized, no noise; int16 samples uploaded as they are
    params = torch.tensor([[0, 0, 30, 30, 0]] * 2, dtype=torch.int32)
    _check_video(batch["inputs"].cpu(), clips, params, 3, 24, what="eval video")
    _check_audio(batch["audios"][:, 0].cpu(), packed["audios"], [T * 640 for T in lens], what="eval audio, int16")
    crop = DeviceLRSPipeline(train=False, size=24, center_crop=True)(packed)
    assert (crop["inputs"][0, :3, 0].cpu() - (clips[0][:, 3:27, 3:27].float() / 255.0 - MEAN) / STD).abs().max().item() < 1e-6
    with pytest.raises(ValueError, match="noise bank"):
        DeviceLRSPipeline(train=True, size=24, noise=torch.zeros(1000))(packed)
    bad = DeviceLRSPipeline(train=True, size=24).draw(lens, 30, 30)
    bad["params"][1, 3] = 31
    with pytest.raises(ValueError, match="outside the stored frame"):
        DeviceLRSPipeline(train=True, size=24)(packed, bad)
