"""The wav2vec2 audio tokeniser on the GPU (csrc/w2v_codec.hip + svsr_igemm_fwd, syncvsr_amd/audio_codec.py) against the fp32 restatement
tests/w2v_codec_ref.py (itself checked against HF transformers by tests/test_w2v_codec_cpu.py), and its integration into E2E / TrainStep.

Tolerances.  Layers 1-6 and weight_proj run on bf16 operands with fp32 accumulation and every activation is stored as bf16 (2^-9 relative
rounding).  Replaying exactly those roundings on the CPU (bf16 weights, bf16 activations after every layer, fp32 arithmetic) moves the logits
of the seeded full-size weights (logit standard deviation ~2) by at most 0.105 over T in {12, 29, 160}, both norm modes.  The end-to-end bound
EPS = 0.25 leaves 2.4x that for the kernels' own summation orders; a token must then match wherever the oracle's top-1 margin exceeds 2 EPS.
Per-kernel checks feed each launch the GPU's own bf16 input, so only that launch's rounding is left: one bf16 rounding of an O(1) output
(2^-8 relative) plus fp32 summation order — atol / rtol 2e-2.
"""
from __future__ import annotations

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_codec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 0.25
PAD = 8000


def _codec(mode: str, seed: int = 1):
    from syncvsr_amd.audio_codec import Wav2Vec2Codec

    return Wav2Vec2Codec.from_state_dict(R.seeded_weights(mode, seed), R.hf_config_kwargs(mode)).to(DEV)


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def _close(a: torch.Tensor, b: torch.Tensor, atol: float, rtol: float, what: str) -> None:
    a, b = a.float().cpu(), b.float().cpu()
    bad = (a - b).abs() > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} outside, max |d| {(a - b).abs().max().item():.4g}"


# ---- per kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["layer", "group"])
def test_layers_against_restatement(mode):
    """Every launch fed the GPU's own bf16 input: conv0 (+ its LayerNorm / GroupNorm + GELU), each contraction layer with its norm / GELU,
    and the quantiser's logits."""
    sd = R.seeded_weights(mode, 1)
    codec = _codec(mode)
    wave = R.synthetic_waveform(2, 29 * 640 + 3, 7)
    L = wave.size(-1) + PAD
    fr = R.frames(L)
    lo: list = []
    logits = torch.empty(2 * fr[-1], 640, dtype=torch.float32, device=DEV)
    codec(wave.to(DEV), pad=PAD, layers_out=lo, logits_out=logits)
    torch.cuda.synchronize()
    ref_lo: list = []
    R.features(sd, mode, wave, PAD, layers_out=ref_lo)
    _close(lo[0], ref_lo[0], 2e-2, 2e-2, f"{mode} layer 0")
    for i in range(1, 7):
        x = lo[i - 1].float().cpu().transpose(1, 2)
        h = F.conv1d(x, _bf(sd[f"{R.FE}.{i}.conv.weight"]), sd.get(f"{R.FE}.{i}.conv.bias"), stride=R.STRIDES[i])
        if mode == "layer":
            h = F.layer_norm(_bf(h).transpose(1, 2), (512,), sd[f"{R.FE}.{i}.layer_norm.weight"], sd[f"{R.FE}.{i}.layer_norm.bias"], 1e-5).transpose(1, 2)
        h = F.gelu(h).transpose(1, 2)
        assert lo[i].shape == (2, fr[i], 512)
        _close(lo[i], h, 2e-2, 2e-2, f"{mode} layer {i}")
    f = _bf(F.layer_norm(lo[6].float().cpu(), (512,), sd[f"{R.PROJ}.weight"], sd[f"{R.PROJ}.bias"], 1e-5))
    z = F.linear(f, _bf(sd[f"{R.QW}.weight"]), sd[f"{R.QW}.bias"]).reshape(-1, 640)
    _close(logits, z, 2e-2, 1e-2, f"{mode} quantize logits")


def test_conv0_group_prenorm_and_groupnorm():
    """Group mode: the pre-norm output of svsr_w2v_conv0 and the GroupNorm finalise-and-apply of svsr_w2v_norm_gelu separately."""
    from syncvsr_amd import ops

    sd = R.seeded_weights("group", 2)
    codec = _codec("group", 2)
    p = codec.packed(DEV)
    wave = R.synthetic_waveform(3, 12 * 640 + 1, 9).squeeze(1)
    B, L_in = wave.shape
    F0 = (L_in + PAD - 10) // 5 + 1
    rows = F0 + (F0 & 1)
    out = torch.empty(B * rows * 512, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(ops.w2v_stats_floats(B, F0), dtype=torch.float32, device=DEV)
    ops.w2v_conv0(wave.to(DEV).contiguous(), B, L_in, PAD, p["w0"], None, None, None, 1e-5, out, rows, stats, True)
    pre = out.view(B, rows, 512)[:, :F0].float().cpu()
    x = torch.cat([wave, torch.zeros(B, PAD)], 1).unsqueeze(1)
    ref_pre = F.conv1d(x, sd[f"{R.FE}.0.conv.weight"], None, stride=5).transpose(1, 2)
    _close(pre, ref_pre, 1e-3, 8e-3, "conv0 pre-norm")
    ops.w2v_norm_gelu(out, B, F0, rows, p["g"][0], p["be"][0], 1e-5, stats=stats, group=True)
    got = out.view(B, rows, 512)[:, :F0].float().cpu()
    ref = F.gelu(F.group_norm(ref_pre.transpose(1, 2), 512, sd[f"{R.FE}.0.layer_norm.weight"], sd[f"{R.FE}.0.layer_norm.bias"], 1e-5)).transpose(1, 2)
    _close(got, ref, 2e-2, 2e-2, "GroupNorm + GELU")


def test_norm_gelu_layer_rows():
    """svsr_w2v_norm_gelu mode 0 on rows with a clip pitch larger than the frame count: padding rows are left alone."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(4)
    B, Fr, rows = 3, 37, 40
    x = (torch.randn(B, rows, 512, generator=g) * 2 + 0.5).to(torch.bfloat16)
    gamma, beta = 1 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)
    xd = x.to(DEV).contiguous()
    ops.w2v_norm_gelu(xd, B, Fr, rows, gamma.to(DEV), beta.to(DEV), 1e-5)
    got = xd.cpu()
    ref = F.gelu(F.layer_norm(x[:, :Fr].float(), (512,), gamma, beta, 1e-5))
    _close(got[:, :Fr], ref, 2e-2, 2e-2, "LayerNorm + GELU")
    assert torch.equal(got[:, Fr:], x[:, Fr:])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["layer", "group"])
@pytest.mark.parametrize("B,T", [(2, 12), (2, 29), (16, 160)])
def test_end_to_end(mode, B, T):
    sd = R.seeded_weights(mode, 1)
    codec = _codec(mode)
    wave = R.synthetic_waveform(B, T * 640, 100 + T)
    fr = R.frames(wave.size(-1) + PAD)
    logits = torch.empty(B * fr[-1], 640, dtype=torch.float32, device=DEV)
    tok = codec(wave.to(DEV), pad=PAD, logits_out=logits).cpu()
    ref_tok, z = R.tokenize(sd, mode, wave, pad=PAD)
    assert tok.shape == ref_tok.shape == (B, fr[-1], 2)
    d = (logits.cpu().view_as(z) - z).abs().max().item()
    assert d <= EPS, f"max |dlogit| {d:.4f} > {EPS}"
    sure = R.margins(z) > 2 * EPS
    assert torch.equal(tok[sure], ref_tok[sure])
    flips = int(((tok != ref_tok) & ~sure).sum())
    print(f"{mode} B={B} T={T}: max |dlogit| {d:.4f}, near-tie flips {flips} of {tok.numel()}")
    assert tok[..., 0].lt(320).all() and tok[..., 1].ge(320).all() and tok[..., 1].lt(640).all()


@pytest.mark.parametrize("mode", ["layer", "group"])
def test_sampling_replays_noise(mode):
    sd = R.seeded_weights(mode, 1)
    codec = _codec(mode)
    B, T = 2, 29
    wave = R.synthetic_waveform(B, T * 640, 3)
    word = torch.tensor([12345], dtype=torch.int32, device=DEV)
    fr = R.frames(wave.size(-1) + PAD)
    logits = torch.empty(B * fr[-1], 640, dtype=torch.float32, device=DEV)
    tok = codec(wave.to(DEV), pad=PAD, sample=True, seed_word=word, logits_out=logits).cpu()
    _, z = R.tokenize(sd, mode, wave, pad=PAD)
    zn = z + R.gumbel(12345, B * fr[-1]).view_as(z)
    ref = R.tokens_from_logits(zn)
    sure = R.margins(zn) > 2 * EPS
    assert torch.equal(tok[sure], ref[sure])
    eval_tok = codec(wave.to(DEV), pad=PAD).cpu()
    assert not torch.equal(tok, eval_tok)
    again = codec(wave.to(DEV), pad=PAD, sample=True, seed_word=word).cpu()
    assert torch.equal(tok, again)
    other = codec(wave.to(DEV), pad=PAD, sample=True, seed_word=torch.tensor([777], dtype=torch.int32, device=DEV)).cpu()
    assert not torch.equal(tok, other)
    # the crop keeps the noise of every frame it keeps
    kept = codec(wave.to(DEV), pad=PAD, sample=True, seed_word=word, keep=2 * T).cpu()
    assert torch.equal(kept, tok[:, : 2 * T])


def test_codec_refuses_cpu_and_short_audio():
    codec = _codec("layer")
    with pytest.raises(RuntimeError):
        codec(torch.zeros(1, 1, 20000))
    with pytest.raises(ValueError):
        codec(torch.zeros(1, 1, 2000, device=DEV), keep=10)


# ---- E2E integration -------------------------------------------------------------------------------------------------------------
def _lrs(seed: int = 7, **kw):
    from syncvsr_amd.lrs_init import default_lrs_args, lrs_init_state_dict
    from syncvsr_amd.lrs_model import E2E

    args = default_lrs_args(adim=128, aheads=2, eunits=256, elayers=2, ddim=128, dheads=2, dunits=256, dlayers=1, codec="wav2vec2", **kw)
    model = E2E(41, args)
    model.load_state_dict(lrs_init_state_dict(args, 41, seed=seed, perturb_norm=True))
    return model.to(DEV), args


def _batch(B: int, T: int, L: int, seed: int = 9):
    from syncvsr_amd.lrs_init import lrs_synthetic_batch

    x, lengths, _, label = lrs_synthetic_batch(_lrs_args(), B, T, odim=41, size=24, seed=seed, label_len=(2, 4))
    wave = R.synthetic_waveform(B, L, seed)
    return x.to(DEV), lengths.to(DEV), wave.to(DEV), label.to(DEV)


def _lrs_args():
    from syncvsr_amd.lrs_init import default_lrs_args

    return default_lrs_args(adim=128, aheads=2, eunits=256, elayers=2, ddim=128, dheads=2, dunits=256, dlayers=1, codec="wav2vec2")


def test_float_audio_without_codec_still_raises():
    model, _ = _lrs()
    x, lengths, wave, label = _batch(2, 11, 11 * 640)
    with pytest.raises(ValueError, match="pass pre-computed audio tokens"):
        model(x, lengths, wave, label)
    with pytest.raises(ValueError, match="pass pre-computed audio tokens"):
        model.prepare_batch(x, lengths, wave, label)


@pytest.mark.parametrize("training", [False, True])
def test_e2e_forward_waveform_equals_tokens(training):
    from syncvsr_amd.audio_codec import LRS_PAD

    model, _ = _lrs()
    model.attach_audio_codec(_codec("layer"), sample_in_training=False)
    model.train(training)
    x, lengths, wave, label = _batch(2, 11, 11 * 640)
    model.reseed_dropout(5)
    out_w = [t.detach().clone() for t in model(x, lengths, wave, label)]
    model.reseed_dropout(5)
    tok = model.wav2vec(wave, pad=LRS_PAD)
    out_t = [t.detach().clone() for t in model(x, lengths, tok, label)]
    torch.cuda.synchronize()
    for a, b in zip(out_w, out_t):
        assert torch.equal(a, b), (a, b)
    with pytest.raises(RuntimeError):
        model(x, lengths, wave.cpu(), label)
    x40, l40, short, label40 = _batch(2, 40, 100)            # 100 samples + 8000 zeros give 25 audio frames, T*A = 80
    with pytest.raises(ValueError):
        model(x40, l40, short, label40)
    with pytest.raises(ValueError):
        model.prepare_batch(x40, l40, short, label40)


def test_e2e_training_forward_samples_under_current_word():
    """sample_in_training=True: a training forward on waveforms equals one on codec(wave, sample=True) under the seed word the step reads."""
    from syncvsr_amd.audio_codec import LRS_PAD

    model, _ = _lrs()
    model.attach_audio_codec(_codec("layer"), sample_in_training=True)
    model.train()
    x, lengths, wave, label = _batch(2, 11, 11 * 640)
    model.reseed_dropout(5)
    out_w = [t.detach().clone() for t in model(x, lengths, wave, label)]
    assert int(model._drop_word.item()) == 6                   # the word advances once per sampling step, even with every dropout p = 0
    model.reseed_dropout(5)
    tok = model.wav2vec(wave, pad=LRS_PAD, sample=True, seed_word=model._drop_word, keep=22)
    assert not torch.equal(tok, model.wav2vec(wave, pad=LRS_PAD, keep=22))
    out_t = [t.detach().clone() for t in model(x, lengths, tok, label)]
    torch.cuda.synchronize()
    for a, b in zip(out_w, out_t):
        assert torch.equal(a, b), (a, b)


def test_nan_audio_keeps_tokens_in_vocabulary():
    """A group whose logits are all NaN takes index 0, the first NaN (torch.argmax); no id leaves [0, 320) / [320, 640)."""
    codec = _codec("layer")
    wave = R.synthetic_waveform(2, 12 * 640, 3)
    wave[0, 0, 100] = float("nan")
    fr = R.frames(wave.size(-1) + PAD)
    logits = torch.empty(2 * fr[-1], 640, dtype=torch.float32, device=DEV)
    for sample in (False, True):
        tok = codec(wave.to(DEV), pad=PAD, sample=sample, seed_word=torch.tensor([9], dtype=torch.int32, device=DEV), logits_out=logits).cpu()
        assert tok[..., 0].ge(0).all() and tok[..., 0].lt(320).all() and tok[..., 1].ge(320).all() and tok[..., 1].lt(640).all()
        nan_rows = logits.cpu().isnan().all(1).view(2, fr[-1])
        assert nan_rows[0].any() and not nan_rows[1].any()
        assert (tok[nan_rows] == torch.tensor([0, 320])).all()


def test_codec_stays_out_of_training_state():
    model, _ = _lrs()
    n_params = sum(p.numel() for p in model.parameters())
    keys0 = set(model.state_dict())
    codec = _codec("group")
    model.attach_audio_codec(codec)
    assert sum(p.numel() for p in model.parameters()) == n_params
    assert not any(n.startswith("wav2vec") for n, _ in model.named_parameters())
    sd = model.state_dict()
    new = set(sd) - keys0
    assert "wav2vec.wav2vec2.feature_extractor.conv_layers.0.conv.weight" in new
    assert "wav2vec.wav2vec2.feature_extractor.conv_layers.0.layer_norm.weight" in new
    assert "wav2vec.wav2vec2.feature_projection.layer_norm.bias" in new
    assert "wav2vec.quantizer.weight_proj.weight" in new and all(k.startswith("wav2vec.") for k in new)
    # round trip into a fresh model with a differently seeded codec
    model2, _ = _lrs(seed=8)
    model2.attach_audio_codec(_codec("group", seed=5))
    model2.load_state_dict(sd)
    for k, v in model2.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    wave = R.synthetic_waveform(2, 12 * 640, 1).to(DEV)
    assert torch.equal(model.wav2vec(wave, pad=PAD), model2.wav2vec(wave, pad=PAD))
    # without a codec the keys are refused as before
    model3, _ = _lrs()
    with pytest.raises(RuntimeError):
        model3.load_state_dict(sd)


def _train(native: bool, batches, max_shapes: int = 1, steps: int = 3):
    from syncvsr_amd.engine import TrainStep

    model, _ = _lrs(dropout_rate=0.0, transformer_attn_dropout_rate=0.0)
    model.attach_audio_codec(_codec("layer"), sample_in_training=True)
    model.reseed_dropout(3)
    model.train()
    ts = TrainStep(model, native=native, max_shapes=max_shapes)
    losses = []
    for i in range(steps):
        out = ts.step(*batches[i % len(batches)])
        losses.append(torch.stack([o.float().reshape(()) for o in out[:4]]).cpu())
    ts.synchronize()
    torch.cuda.synchronize()
    return losses, model.store().flat.detach().cpu().clone(), int(model._drop_word.item())


def test_trainstep_native_matches_eager_with_sampling():
    b = _batch(2, 11, 11 * 640)
    le, pe, we = _train(False, [b])
    ln, pn, wn = _train(True, [b])
    assert we == wn == 3 + 3
    for a, c in zip(le, ln):
        assert torch.equal(a, c), (a, c)
    assert torch.equal(pe, pn)


def test_trainstep_native_two_audio_lengths():
    bs = [_batch(2, 11, 11 * 640, seed=9), _batch(2, 11, 11 * 640 + 1234, seed=10)]
    le, pe, _ = _train(False, bs, steps=4)
    ln, pn, _ = _train(True, bs, max_shapes=2, steps=4)
    for a, c in zip(le, ln):
        assert torch.equal(a, c), (a, c)
    assert torch.equal(pe, pn)


def test_lrw_forward_audios():
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.model import Model

    cfg = default_lrw_config(model__bert__num_hidden_layers=2, model__wav2vec__path="facebook/wav2vec2-large-xlsr-53")
    model = Model(cfg).to(DEV).eval()
    with pytest.raises(ValueError):
        model.forward_audios(torch.zeros(2, 19200, device=DEV))
    model.attach_audio_codec(_codec("layer"))
    sd = R.seeded_weights("layer", 1)
    wave = R.synthetic_waveform(2, 19200, 4)
    tok = model.forward_audios(wave.squeeze(1).to(DEV)).cpu()
    ref, z = R.tokenize(sd, "layer", wave)
    sure = R.margins(z) > 2 * EPS
    assert tok.shape == ref.shape and torch.equal(tok[sure], ref[sure])


def _step_load_step(native: bool, b):
    """One step (recorded when native), then new wav2vec.* weights by load_state_dict, then a second (replayed) step."""
    from syncvsr_amd.audio_codec import LRS_PAD
    from syncvsr_amd.engine import TrainStep

    model, _ = _lrs()
    model.attach_audio_codec(_codec("layer"), sample_in_training=False)
    model.train()
    ts = TrainStep(model, native=native)
    out1 = ts.step(*b)
    loss1 = torch.stack([o.float().reshape(()) for o in out1[:4]]).cpu()
    ts.synchronize()
    p = model.wav2vec.packed(DEV)
    ptrs = [p["w0"].data_ptr(), p["qw"].data_ptr()] + [w.data_ptr() for w in p["w"][1:]]
    model.load_state_dict({"wav2vec." + k: v for k, v in _codec("layer", seed=5).state_dict().items()}, strict=False)
    model.to(DEV)
    p = model.wav2vec.packed(DEV)
    assert ptrs == [p["w0"].data_ptr(), p["qw"].data_ptr()] + [w.data_ptr() for w in p["w"][1:]]      # updated in place
    wave = b[2]
    assert torch.equal(model.wav2vec(wave, pad=LRS_PAD, keep=22), _codec("layer", seed=5)(wave, pad=LRS_PAD, keep=22))
    out2 = ts.step(*b)
    loss2 = torch.stack([o.float().reshape(()) for o in out2[:4]]).cpu()
    ts.synchronize()
    torch.cuda.synchronize()
    return loss1, loss2, model.store().flat.detach().cpu().clone()


def test_native_replay_sees_codec_weights_loaded_after_recording():
    """A recorded step list holds the addresses of the codec's device weights: a load_state_dict after the recorded step must reach the
    replay (eager tokenises with the newly loaded weights, checked against a freshly built codec above)."""
    b = _batch(2, 11, 11 * 640)
    e1, e2, pe = _step_load_step(False, b)
    n1, n2, pn = _step_load_step(True, b)
    assert torch.equal(e1, n1) and torch.equal(e2, n2), (e1, n1, e2, n2)
    assert torch.equal(pe, pn)
    assert e2[3] != e1[3]            # the audio loss moved with the new targets
