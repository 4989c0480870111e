"""The vq-wav2vec k-means audio tokeniser on the GPU (csrc/vq_codec.hip + svsr_igemm_fwd, syncvsr_amd/audio_codec.VqWav2VecCodec) against
the fp32 restatement tests/vq_codec_ref.py, and its integration into the word-level models, CutMix and TrainStep.

Tolerances.  Layers 1-7 run on bf16 operands with fp32 accumulation, every activation is stored as bf16 (the contraction's output before its
GroupNorm, and again behind it), and the centroids and the normalised projections meet as bf16.  Replaying exactly those roundings on the
CPU (vq_codec_ref.replay) moves the scores |e|^2 - 2 z.e of the seeded full-size weights (score standard deviation ~38) by at most 1.634
over the four shapes below (1.016, 1.428, 1.634, 1.565 in their order) and flips 7 of their 662 tokens (1.06 %: 0 of 6, 2 of 96, 1 of 96,
4 of 464), the widest oracle margin at a flip being 0.50.  `python tests/vq_codec_ref.py` (vq_codec_ref.measure_replay, on the CPU, with
the very shapes and waveforms this file uses) prints these figures; they are the same to three decimals with 1 to 16 threads.  The
end-to-end bound EPS = 3.9 = 2.4 x 1.634 leaves the kernels' own summation orders the margin tests/test_gpu_w2v_codec.py gives, and a
shape may flip at most twice the replay's share of its tokens (or 2 tokens).
Per-kernel checks feed each launch the GPU's own input, so only that launch's rounding is left: one bf16 rounding of an O(1) output (2^-8
relative) plus fp32 summation order — atol = rtol = 2e-2, as the wav2vec2 codec's test.
"""
from __future__ import annotations

import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_codec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 3.9
REPLAY_FLIP_SHARE = 7 / 662
SHAPES = R.SHAPES


@functools.lru_cache(maxsize=None)
def _ref(seed: int = 1, combine: bool = False):
    return R.seeded_model(seed, combine)


@functools.lru_cache(maxsize=None)
def _case(B: int, L: int):
    """(wave, oracle tokens, oracle scores), computed once per shape and shared."""
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    wave = R.case_waveform(B, L)
    tok, s = R.oracle(_ref(), wave)
    return wave, tok, s


def _codec(seed: int = 1, combine: bool = False):
    from syncvsr_amd.audio_codec import VqWav2VecCodec

    return VqWav2VecCodec.from_state_dict(_ref(seed, combine).state_dict(), R.fairseq_args(combine_groups=combine)).to(DEV)


def _close(a: torch.Tensor, b: torch.Tensor, atol: float, rtol: float, what: str) -> None:
    a, b = a.float().cpu(), b.float().cpu()
    bad = (a - b).abs() > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} outside, max |d| {(a - b).abs().max().item():.4g}"


@functools.lru_cache(maxsize=None)
def _gpu_layers(B: int, L: int):
    codec = _codec()
    lo: list = []
    tok = codec(_case(B, L)[0].to(DEV), layers_out=lo)
    torch.cuda.synchronize()
    return codec, tok, lo


# ---- per kernel ------------------------------------------------------------------------------------------------------------------
def test_conv0_stats_partials():
    """F0 = 591 frames span ten 64-frame blocks: the partial {sum, sum of squares} pairs add up to the fp32 statistics of the convolution."""
    from syncvsr_amd import ops

    codec = _codec()
    p = codec.packed(DEV)
    wave = _case(3, 2960)[0]
    F0 = R.frames(2960)[0]
    part = torch.full((ops.vq_part_floats(3, F0, 0),), float("nan"), dtype=torch.float32, device=DEV)
    assert part.numel() == 3 * 10 * 2
    ops.vq_conv0_stats(wave.to(DEV), 3, 2960, 0, p["w0"], part)
    got = part.cpu().view(3, 10, 2).double().sum(1)
    pre = F.conv1d(wave.unsqueeze(1), _ref().feature_extractor.conv_layers[0][0].weight, stride=5).double()
    assert pre.shape == (3, 512, F0)
    assert torch.allclose(got[:, 1], pre.square().sum((1, 2)), rtol=1e-4, atol=0)
    assert ((got[:, 0] - pre.sum((1, 2))).abs() <= 1e-4 * pre.abs().sum((1, 2))).all()
    # a ragged last block and appended zeros: 2963 samples + 7 zeros are the frames of 2970 samples
    part2 = torch.empty(ops.vq_part_floats(3, R.frames(2970)[0], 0), dtype=torch.float32, device=DEV)
    w3 = _case(3, 2963)[0]
    ops.vq_conv0_stats(w3.to(DEV), 3, 2963, 7, p["w0"], part2)
    pre2 = F.conv1d(F.pad(w3, (0, 7)).unsqueeze(1), _ref().feature_extractor.conv_layers[0][0].weight, stride=5).double()
    assert torch.allclose(part2.cpu().view(3, -1, 2).double().sum(1)[:, 1], pre2.square().sum((1, 2)), rtol=1e-4, atol=0)


@pytest.mark.parametrize("B,L", [(3, 2960), (2, 18960)])
def test_layers_against_restatement(B, L):
    """Every launch fed the GPU's own input: conv0_apply from the waveform, each contraction + gn_partial + gn_relu (the last with the log)
    from the previous layer's bf16 rows, the projection from the last layer's."""
    m = _ref()
    wave = _case(B, L)[0]
    fr = R.frames(L)
    _, _, lo = _gpu_layers(B, L)
    assert len(lo) == 9
    conv0, _, gn0, _ = m.feature_extractor.conv_layers[0]
    with torch.no_grad():
        _close(lo[0], F.relu(gn0(conv0(wave.unsqueeze(1)))).transpose(1, 2), 2e-2, 2e-2, "layer 0")
        for i in range(1, 8):
            conv, _, gn, _ = m.feature_extractor.conv_layers[i]
            x = lo[i - 1].float().cpu().transpose(1, 2)
            h = R.gn_relu_step(R.bf(F.conv1d(x, R.bf(conv.weight), stride=conv.stride)), gn, i == 7)
            assert lo[i].shape == (B, fr[i], 512) and lo[i].dtype == torch.bfloat16
            _close(lo[i], h.transpose(1, 2), 2e-2, 2e-2, f"layer {i}")
        ze = F.conv1d(lo[7].float().cpu().transpose(1, 2), R.bf(m.vector_quantizer.projection[0].weight), groups=2).transpose(1, 2)
        assert lo[8].dtype == torch.float32
        _close(lo[8], ze, 2e-2, 2e-2, "projection")


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("layer", [1, 2])
def test_gn_partial_and_gn_relu_in_place(layer, log):
    """svsr_vq_gn_partial + svsr_vq_gn_relu on the GPU's own rows of layer 1 (146 rows: three blocks) and 2 (72 rows: a block of 8 behind a
    full one), in a buffer whose clips are two rows longer than their frames: the padding rows keep their bits."""
    from syncvsr_amd import ops

    codec, _, lo = _gpu_layers(3, 2960)
    p = codec.packed(DEV)
    x = lo[layer]
    B, Fr, _ = x.shape
    rows = Fr + 2
    buf = torch.full((B, rows, 512), -7.25, dtype=torch.bfloat16, device=DEV)
    buf[:, Fr:, ::3] = float("nan")
    buf[:, :Fr] = x
    before = buf.clone()
    part = torch.full((ops.vq_part_floats(B, Fr, 0),), float("nan"), dtype=torch.float32, device=DEV)
    ops.vq_gn_partial(buf, B, Fr, rows, part)
    got = part.cpu().view(B, -1, 2).double().sum(1)
    xd = x.double().cpu()
    assert torch.allclose(got[:, 1], xd.square().sum((1, 2)), rtol=1e-4, atol=0)
    assert torch.allclose(got[:, 0], xd.sum((1, 2)), rtol=1e-4, atol=0)            # (ReLU outputs: no cancellation)
    ops.vq_gn_relu(buf, B, Fr, rows, p["g"][layer], p["be"][layer], 1e-5, part, log=log)
    gn = _ref().feature_extractor.conv_layers[layer][2]
    with torch.no_grad():
        ref = R.gn_relu_step(x.float().cpu().transpose(1, 2), gn, log).transpose(1, 2)
    _close(buf[:, :Fr], ref, 2e-2, 2e-2, f"GroupNorm + ReLU{' + log' if log else ''}")
    assert torch.equal(buf[:, Fr:].view(torch.int16), before[:, Fr:].view(torch.int16))


def test_project_partials():
    from syncvsr_amd import ops

    codec, _, lo = _gpu_layers(2, 18960)
    B, Fr, _ = lo[7].shape
    assert Fr == 116
    ze = torch.empty(B * Fr, 512, dtype=torch.float32, device=DEV)
    part = torch.full((ops.vq_part_floats(B, Fr, 1),), float("nan"), dtype=torch.float32, device=DEV)
    assert part.numel() == B * 2 * 4 * 2
    ops.vq_project(lo[7].contiguous(), B, Fr, codec.packed(DEV)["pw"], ze, part)
    assert torch.equal(ze.view(B, Fr, 512), lo[8])
    z = ze.view(B, Fr, 2, 256).double().cpu()
    got = part.cpu().view(B, 2, 4, 2).double().sum(2)
    assert torch.allclose(got[..., 1], z.square().sum((1, 3)), rtol=1e-4, atol=0)
    assert ((got[..., 0] - z.sum((1, 3))).abs() <= 1e-4 * z.abs().sum((1, 3))).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", SHAPES)
def test_end_to_end(B, L):
    wave, ref_tok, s = _case(B, L)
    Fr = R.frames(L)[-1]
    codec = _codec()
    scores = torch.empty(B * Fr, 2, 320, dtype=torch.float32, device=DEV)
    tok = codec(wave.to(DEV), scores_out=scores).cpu()
    assert tok.dtype == torch.int64 and tok.shape == ref_tok.shape == (B, Fr, 2)
    assert tok.ge(0).all() and tok.lt(320).all()                                     # (d)
    got = scores.cpu().view_as(s)
    d = (got - s).abs().max().item()
    chosen = s.gather(-1, tok.unsqueeze(-1)).squeeze(-1)
    regret = (chosen - s.min(-1).values).max().item()
    sure = R.margins(s) > 2 * EPS
    flips = int((tok != ref_tok).sum())
    allowed = max(2, int(2 * REPLAY_FLIP_SHARE * tok.numel()))
    print(f"B={B} L={L}: max |dscore| {d:.4f}, worst regret {regret:.4f}, flips {flips} of {tok.numel()} ({flips / tok.numel():.2%}; allowed {allowed}), "
          f"sure {int(sure.sum())}")
    assert d <= EPS, f"max |dscore| {d:.4f} > {EPS}"                                 # (a)
    assert regret <= 2 * EPS, f"a GPU token is {regret:.4f} above the oracle's minimum"   # (b)
    assert torch.equal(tok[sure], ref_tok[sure])                                     # (c)
    assert torch.equal(got.argmin(-1), tok)                                          # the tokens are the argmin of the scores written
    assert flips <= allowed


def test_batch_independence():
    """A clip inside a batch of three clips of different amplitude has the tokens it has alone: no statistics or padding rows leak."""
    wave = _case(3, 2963)[0]
    codec = _codec()
    tok = codec(wave.to(DEV))
    for b in range(3):
        assert torch.equal(codec(wave[b : b + 1].to(DEV))[0], tok[b]), b


def test_keep_pad_and_determinism():
    wave = _case(3, 2960)[0].to(DEV)
    codec = _codec()
    tok = codec(wave)
    assert torch.equal(codec(wave), tok)
    for k in (1, 7, 16):
        kept = codec(wave, keep=k)
        assert kept.shape == (3, k, 2) and kept.is_contiguous() and torch.equal(kept, tok[:, :k])
    padded = codec(wave, pad=483)
    assert padded.shape == (3, 19, 2)
    assert torch.equal(padded, codec(F.pad(wave, (0, 483))))
    assert torch.equal(codec(wave.unsqueeze(1)), tok)                                 # [B, 1, L]


def test_combine_groups():
    shared = _codec(3, True)
    sd = {k: (v.expand(320, 2, 256).clone() if k.endswith("embedding") else v) for k, v in _ref(3, True).state_dict().items()}
    from syncvsr_amd.audio_codec import VqWav2VecCodec

    full = VqWav2VecCodec.from_state_dict(sd).to(DEV)
    wave = _case(3, 2960)[0].to(DEV)
    a, b = shared(wave), full(wave)
    assert torch.equal(a, b) and a.unique().numel() > 8


def test_nan_clip_gives_token_zero():
    wave = _case(3, 2960)[0].clone()
    codec = _codec()
    clean = codec(wave.to(DEV)).cpu()
    wave[1, 1234] = float("nan")
    tok = codec(wave.to(DEV)).cpu()
    assert (tok[1] == 0).all()
    assert torch.equal(tok[0], clean[0]) and torch.equal(tok[2], clean[2])
    assert clean[1].ne(0).any()


def test_assign_nan_in_one_group_zeroes_both_tokens():
    """svsr_vq_assign alone, finite statistics, one row whose projection holds a NaN in group 1 only: the row's tokens are (0, 0), every other
    row keeps its tokens."""
    from syncvsr_amd import ops

    codec, _, lo = _gpu_layers(3, 2960)
    p = codec.packed(DEV)
    B, Fr, _ = lo[8].shape
    ze = lo[8].reshape(B * Fr, 512).clone()
    part = torch.empty(ops.vq_part_floats(B, Fr, 1), dtype=torch.float32, device=DEV)
    ops.vq_project(lo[7].contiguous(), B, Fr, p["pw"], torch.empty_like(ze), part)

    def assign(z):
        tok = torch.full((B * Fr * 2,), -1, dtype=torch.int64, device=DEV)
        ops.vq_assign(z, B, Fr, Fr, p["pg"], p["pb"], 1e-5, part, p["emb"], p["e2"], tok)
        return tok.view(B, Fr, 2).cpu()

    clean = assign(ze)
    assert torch.equal(clean, _gpu_layers(3, 2960)[1].cpu())
    t = int(clean[1].ne(0).all(-1).nonzero()[0])             # a frame of clip 1 whose tokens are both non-zero
    ze[Fr + t, 256 + 17] = float("nan")
    tok = assign(ze)
    assert (tok[1, t] == 0).all()
    tok[1, t] = clean[1, t]
    assert torch.equal(tok, clean)


def test_errors():
    codec = _codec()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec(torch.zeros(2, 2960))
    with pytest.raises(ValueError, match=r"464 samples.*465"):
        codec(torch.zeros(2, 464, device=DEV))
    with pytest.raises(ValueError, match=r"2960 samples.*16 audio frames, need 17 frames \(3025 samples\)"):
        codec(torch.zeros(2, 2960, device=DEV), keep=17)
    assert codec(torch.zeros(1, 464, device=DEV), pad=1).shape == (1, 1, 2)
    assert codec.workspace_bytes(3, 2960) > 2 * 3 * 592 * 512


# ---- integration -----------------------------------------------------------------------------------------------------------------
T_LRW, SIZE = 7, 40
L_LRW = 640 * T_LRW + 305            # exactly the samples of T * A = 28 frames


def _lrw(attach: bool = True, seed: int = 21):
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.init import init_state_dict, synthetic_batch
    from syncvsr_amd.model import Model

    cfg = default_lrw_config(model__bert__num_hidden_layers=2)
    cfg.optim.scheduler.num_warmup_steps = 1
    model = Model(cfg)
    model.load_state_dict(init_state_dict(cfg, seed=seed, perturb_norm=True))
    model.to(DEV)
    if attach:
        model.attach_audio_codec(_codec())
    videos, _, labels, wm = [t.to(DEV) for t in synthetic_batch(cfg, batch=3, frames=T_LRW, size=SIZE, seed=33)]
    wave = R.synthetic_waveform(3, L_LRW + 40, 5).to(DEV)
    return cfg, model, videos, wave, labels, wm


def test_forward_audios_forward_and_validation_step():
    cfg, model, videos, wave, labels, wm = _lrw()
    model.eval()
    tok = model.wav2vec(wave)
    assert tok.shape == (3, 4 * T_LRW, 2)
    assert torch.equal(model.forward_audios(wave), tok)
    out_t = model(videos, tok, labels, wm)
    out_w = model(videos, wave, labels, wm)
    val = model.validation_step((videos, wave.unsqueeze(1), labels, wm))
    test = model.test_step((videos, wave, labels, wm))
    torch.cuda.synchronize()
    for k, v in out_t.items():
        assert torch.equal(out_w[k], v) and torch.equal(val[f"val/{k}"], v) and torch.equal(test[f"test/{k}"], v), k
    assert torch.isfinite(out_t["loss_audio"])
    with pytest.raises(ValueError, match="need 28 frames"):
        model(videos, wave[:, : L_LRW - 1], labels, wm)
    with pytest.raises(RuntimeError):
        model(videos, wave.cpu(), labels, wm)


def test_float_audio_without_codec_is_not_tokenised():
    _, model, videos, wave, labels, wm = _lrw(attach=False)
    assert model._tokenize_waveforms(wave, 28) is wave
    with pytest.raises(ValueError, match="forward_audios needs the vq tokeniser.*VqWav2VecCodec"):
        model.forward_audios(wave)


def test_dctcn_forward_on_waveforms():
    from dctcn_cases import dctcn_subcase
    from syncvsr_amd.dctcn import DCTCNLightningModule

    cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", "nowb_t7")
    m = DCTCNLightningModule(cfg)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    videos, _, labels, word, attention = [t.to(DEV) for t in batch]
    B, T = videos.size(0), videos.size(2)
    wave = R.synthetic_waveform(B, 640 * T + 305, 8).to(DEV)
    with pytest.raises(ValueError, match="pass pre-computed audio tokens"):
        m(videos, wave, labels, word, attention)
    n = sum(p.numel() for p in m.parameters())
    m.attach_audio_codec(_codec())
    assert sum(p.numel() for p in m.parameters()) == n
    tok = m.wav2vec(wave, keep=dims["A"] * T)
    out_t = m(videos, tok, labels, word, attention)
    out_w = m(videos, wave, labels, word, attention)
    torch.cuda.synchronize()
    for k, v in out_t.items():
        assert torch.equal(out_w[k], v), k
    # the codec's buffers are in the state dict and load back; a reference checkpoint's other wav2vec.* keys are still ignored
    sd2 = m.state_dict()
    assert "wav2vec.vector_quantizer.embedding" in sd2
    m2 = DCTCNLightningModule(cfg)
    m2.attach_audio_codec(_codec(5))
    m2.load_state_dict({**sd2, "wav2vec.feature_aggregator.conv_layers.0.0.weight": torch.zeros(3)})
    m2.to(DEV)
    assert torch.equal(m2.wav2vec(wave), m.wav2vec(wave))


def test_cutmix_tokenises_then_splices():
    from syncvsr_amd.augment import CutMix

    _, model, videos, wave, labels, wm = _lrw()
    codec = model.wav2vec
    cm = CutMix(model.word_labels, wav2vec=codec)
    cm.generator = torch.Generator().manual_seed(17)
    a = cm(videos, wave, labels, wm)
    cm.generator = torch.Generator().manual_seed(17)
    b = cm(videos, codec(wave), labels, wm)
    assert a[1].dtype == torch.int64
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    plain = CutMix(model.word_labels)
    plain.generator = torch.Generator().manual_seed(17)
    for x, y in zip(plain(videos, codec(wave), labels, wm), b):
        assert torch.equal(x, y)
    # the codec is borrowed, not a sub-module: it is not listed and not moved by the CutMix that holds it
    assert cm.wav2vec is codec and not cm.state_dict() and not list(cm.children())


def test_codec_stays_out_of_training_state_and_round_trips():
    _, model, _, wave, _, _ = _lrw(attach=False)
    n = sum(p.numel() for p in model.parameters())
    keys0 = set(model.state_dict())
    flat = model.store().flat.numel()
    model.attach_audio_codec(_codec())
    assert sum(p.numel() for p in model.parameters()) == n and model.store().flat.numel() == flat
    assert not any(k.startswith("wav2vec") for k, _ in model.named_parameters())
    sd = model.state_dict()
    new = set(sd) - keys0
    assert new == {"wav2vec." + k for k in _ref().state_dict()}
    _, model2, _, _, _, _ = _lrw(attach=False, seed=8)
    model2.attach_audio_codec(_codec(5))
    assert not torch.equal(model2.wav2vec(wave), model.wav2vec(wave))
    model2.load_state_dict(sd)
    for k, v in model2.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    assert torch.equal(model2.wav2vec(wave), model.wav2vec(wave))
    _, model3, _, _, _, _ = _lrw(attach=False)
    with pytest.raises(RuntimeError):
        model3.load_state_dict(sd)


def test_attach_refuses_the_wrong_kind():
    import w2v_codec_ref as W
    from syncvsr_amd.audio_codec import Wav2Vec2Codec
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.model import Model

    _, model, *_ = _lrw(attach=False)
    with pytest.raises(ValueError, match="'vq' codec"):
        model.attach_audio_codec(Wav2Vec2Codec.from_state_dict(W.seeded_weights("layer", 1), W.hf_config_kwargs("layer")))
    other = Model(default_lrw_config(model__bert__num_hidden_layers=1, model__wav2vec__path="facebook/wav2vec2-large-xlsr-53")).to(DEV)
    with pytest.raises(ValueError, match="'wav2vec2' codec"):
        other.attach_audio_codec(_codec())


def _train(native: bool, on_waveforms: bool, steps: int = 3, reload_after: int = -1):
    from syncvsr_amd.engine import TrainStep

    cfg, model, videos, wave, labels, wm = _lrw()
    model.train()
    ts = TrainStep(model, cfg, native=native)
    losses = []
    for i in range(steps):
        if i == reload_after:
            ts.synchronize()
            ptr = model.wav2vec.packed(DEV)["emb"].data_ptr()
            model.load_state_dict({"wav2vec." + k: v for k, v in _codec(5).state_dict().items()}, strict=False)
            assert model.wav2vec.packed(DEV)["emb"].data_ptr() == ptr                  # updated in place
        audios = wave if on_waveforms else model.wav2vec(wave, keep=4 * T_LRW)
        out = ts.step(videos, audios, labels, wm)
        losses.append(torch.stack([out[k].float().reshape(()) for k in ("loss_total", "loss_category", "loss_audio")]).cpu())
    ts.synchronize()
    torch.cuda.synchronize()
    return losses, model.store().flat.detach().cpu().clone()


def test_trainstep_on_waveforms_eager_native_tokens():
    """Three steps on float audio: eager and native agree bit for bit, and both with the steps on the codec's own tokens."""
    le, pe = _train(False, True)
    ln, pn = _train(True, True)
    lt, pt = _train(True, False)
    for a, b, c in zip(le, ln, lt):
        assert torch.equal(a, b) and torch.equal(a, c), (a, b, c)
    assert torch.equal(pe, pn) and torch.equal(pe, pt)


def test_native_replay_sees_codec_weights_loaded_after_recording():
    l0, _ = _train(True, True, steps=2)
    l1, p1 = _train(True, True, steps=2, reload_after=1)
    e1, pe = _train(False, True, steps=2, reload_after=1)
    assert torch.equal(l0[0], l1[0])
    assert l1[1][2] != l0[1][2]                        # the audio loss of the replayed step moved with the new targets
    assert torch.equal(l1[1], e1[1]) and torch.equal(p1, pe)
