"""Host-side checks of the vq-wav2vec k-means tokeniser: the restatement tests/vq_codec_ref.py (names, shapes, the two forms of the
distance, per-clip statistics) and what syncvsr_amd.audio_codec.VqWav2VecCodec does without a device (loading, refusals, frame counts).

fairseq is not a dependency of this package and the comparison with it at the end is skipped wherever it is not installed: the restatement
is pinned to the specification taken from fairseq's Wav2VecModel / ConvFeatureExtractionModel / KmeansVectorQuantizer sources (the module
docstring of vq_codec_ref.py and syncvsr_amd/audio_codec.py), not to a fairseq run.
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_codec_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def model():
    return R.seeded_model(1)


@pytest.fixture(scope="module")
def case(model):
    wave = R.synthetic_waveform(3, 2960, 12)
    tok, s = R.oracle(model, wave)
    return wave, tok, s


def test_state_dict_names_and_shapes(model):
    sd = model.state_dict()
    want = {f"{R.VQ}.embedding": (320, 2, 256), f"{R.VQ}.projection.0.weight": (512, 256, 1), f"{R.VQ}.projection.1.weight": (512,),
            f"{R.VQ}.projection.1.bias": (512,)}
    cin = 1
    for i, k in enumerate(R.KERNELS):
        want[f"{R.FE}.{i}.0.weight"] = (512, cin, k)
        want[f"{R.FE}.{i}.2.weight"] = want[f"{R.FE}.{i}.2.bias"] = (512,)
        cin = 512
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    from syncvsr_amd.audio_codec import VqWav2VecCodec

    codec = VqWav2VecCodec.from_state_dict(sd, R.fairseq_args())
    got = codec.state_dict()
    assert set(got) == set(want)
    assert all(torch.equal(got[k], sd[k]) for k in want)
    assert not list(codec.parameters())


def test_prefix_and_other_fairseq_keys(model):
    from syncvsr_amd.audio_codec import VqWav2VecCodec

    sd = {"wav2vec." + k: v for k, v in model.state_dict().items()}
    sd["wav2vec.feature_aggregator.conv_layers.0.0.weight"] = torch.zeros(4)
    sd["wav2vec.wav2vec_predictions.project_to_steps.weight"] = torch.zeros(4)
    codec = VqWav2VecCodec.from_state_dict(sd)
    assert not any("aggregator" in k or "predictions" in k for k in codec.state_dict())
    ck = {"model": {k[len("wav2vec."):]: v for k, v in sd.items()}, "args": SimpleNamespace(**R.fairseq_args())}
    assert set(VqWav2VecCodec.from_checkpoint(ck).state_dict()) == set(codec.state_dict())
    ck["args"] = R.fairseq_args(vq_type="gumbel")
    with pytest.raises(NotImplementedError, match="kmeans"):
        VqWav2VecCodec.from_checkpoint(ck)
    ck["args"] = None                                   # (newer checkpoints keep an omegaconf `cfg` instead: the released layout is assumed)
    VqWav2VecCodec.from_checkpoint(ck)
    import argparse

    ck["args"] = argparse.Namespace(**R.fairseq_args(vq_groups=1))
    with pytest.raises(NotImplementedError, match="vq_groups"):
        VqWav2VecCodec.from_checkpoint(ck)

    class NotPlain:                                     # e.g. an omegaconf node: its __dict__ is not its content, so it is not read at all
        def __init__(self):
            self._content = R.fairseq_args(vq_type="gumbel")

    ck["args"] = NotPlain()
    with pytest.raises(NotImplementedError, match="NotPlain"):
        VqWav2VecCodec.from_checkpoint(ck)
    short = dict(ck["model"])
    del short[f"{R.VQ}.embedding"]
    with pytest.raises(KeyError):
        VqWav2VecCodec.from_state_dict(short)


def test_missing_affine_is_identity(model):
    from syncvsr_amd.audio_codec import VqWav2VecCodec

    sd = {k: v for k, v in model.state_dict().items() if not k.endswith((".2.weight", ".2.bias")) and "projection.1" not in k}
    got = VqWav2VecCodec.from_state_dict(sd).state_dict()
    assert torch.equal(got[f"{R.FE}.3.2.weight"], torch.ones(512)) and torch.equal(got[f"{R.VQ}.projection.1.bias"], torch.zeros(512))


@pytest.mark.parametrize("over,word", [
    (dict(vq_type="gumbel"), "vq_type"),
    (dict(conv_feature_layers="[(512, 10, 5), (512, 8, 4), (512, 4, 2), (512, 4, 2), (512, 4, 2), (512, 1, 1), (512, 1, 1)]"), "conv_feature_layers"),
    (dict(conv_feature_layers=[(256, 10, 5)] * 8), "conv_feature_layers"),
    (dict(skip_connections_feat=True), "skip_connections_feat"),
    (dict(log_compression=False), "log_compression"),
    (dict(vq_groups=1), "vq_groups"),
    (dict(vq_vars=640), "vq_vars"),
    (dict(vq_dim=256), "vq_dim"),
])
def test_check_config_refusals(over, word):
    from syncvsr_amd.audio_codec import vq_check_config

    with pytest.raises(NotImplementedError, match=word):
        vq_check_config(R.fairseq_args(**over))
    with pytest.raises(NotImplementedError, match=word):
        vq_check_config(SimpleNamespace(**R.fairseq_args(**over)))


def test_check_config_accepts_the_released_layout():
    from syncvsr_amd.audio_codec import vq_check_config

    assert vq_check_config(None) is False
    assert vq_check_config(R.fairseq_args()) is False
    assert vq_check_config(R.fairseq_args(vq_dim=512, combine_groups=True, conv_feature_layers=[(512, k, s) for k, s in zip(R.KERNELS, R.STRIDES)])) is True


def test_frame_counts():
    from syncvsr_amd.audio_codec import VqWav2VecCodec, vq_frame_counts, vq_min_samples

    assert vq_frame_counts(465) == [92, 22, 10, 4, 1, 1, 1, 1]
    assert vq_frame_counts(464)[-1] == 0
    assert vq_frame_counts(2960) == [591, 146, 72, 35, 16, 16, 16, 16]
    assert vq_frame_counts(18960)[-1] == 116
    assert VqWav2VecCodec.frame_counts(2963) == R.frames(2963)
    for T in (1, 7, 29):                                 # keep = A * T = 4 T needs 640 T + 305 samples, and one fewer is too few
        assert vq_min_samples(4 * T) == 640 * T + 305
        assert vq_frame_counts(640 * T + 305)[-1] == 4 * T and vq_frame_counts(640 * T + 304)[-1] == 4 * T - 1
    assert VqWav2VecCodec._rows(vq_frame_counts(2960)) == [592, 146, 72, 36, 16, 16, 16, 16]


def test_score_form_and_broadcast_norm_form_agree(model, case):
    """|e|^2 - 2 z.e and fairseq's (ze - e).norm() differ by the row's |z|^2 and a square root: the same argmin."""
    wave, tok, s = case
    with torch.no_grad():
        idx = model.vector_quantizer.forward_idx(model.feature_extractor(wave))
    assert tok.shape == idx.shape == (3, 16, 2)
    assert torch.equal(tok, idx)
    assert tok.min() >= 0 and tok.max() < 320 and tok.unique().numel() > 8
    assert 30 < s.std().item() < 50                      # the scale the margins of the GPU test are read against


def test_combine_groups_expansion():
    from syncvsr_amd.audio_codec import VqWav2VecCodec

    shared = R.seeded_model(3, combine_groups=True)
    sd = shared.state_dict()
    assert tuple(sd[f"{R.VQ}.embedding"].shape) == (320, 1, 256)
    codec = VqWav2VecCodec.from_state_dict(sd, R.fairseq_args(combine_groups=True))
    assert tuple(codec.state_dict()[f"{R.VQ}.embedding"].shape) == (320, 1, 256)
    f = codec._forms(torch.device("cpu"))
    assert tuple(f["emb"].shape) == (2, 320, 256) and torch.equal(f["emb"][0], f["emb"][1])
    assert torch.equal(f["emb"][1].float(), sd[f"{R.VQ}.embedding"][:, 0].to(torch.bfloat16).float())
    assert torch.allclose(f["e2"], f["emb"].float().square().sum(-1))
    full = R.seeded_model(3)
    full.load_state_dict({k: (v.expand(320, 2, 256).clone() if k.endswith("embedding") else v) for k, v in sd.items()})
    wave = R.synthetic_waveform(2, 2960, 5)
    assert torch.equal(R.oracle(shared, wave)[0], R.oracle(full, wave)[0])


def test_clips_do_not_see_their_batch_neighbours(model, case):
    """Every GroupNorm takes its statistics per clip: a clip's scores are those it has alone, whatever stands next to it."""
    wave, tok, s = case
    for b in range(3):
        t1, s1 = R.oracle(model, wave[b : b + 1])
        assert torch.equal(t1[0], tok[b])
        assert torch.allclose(s1[0], s[b], atol=1e-3, rtol=1e-5)
    louder = wave.clone()
    louder[0] *= 7.0
    assert torch.equal(R.oracle(model, louder)[0][1:], tok[1:])


def test_replay_stays_near_the_oracle(model, case):
    """The kernels' roundings move scores of standard deviation ~40 by less than 2 (the bound the GPU test scales its EPS from)."""
    wave, tok, s = case
    t2, s2 = R.replay(model, wave)
    assert (s - s2).abs().max().item() < 2.0
    assert (t2 != tok).sum().item() <= 4


def test_cpu_tensor_is_refused(model):
    from syncvsr_amd.audio_codec import VqWav2VecCodec

    codec = VqWav2VecCodec.from_state_dict(model.state_dict())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec(torch.zeros(1, 465))


def test_attach_refuses_the_wrong_kind(model):
    import w2v_codec_ref as W
    from syncvsr_amd.audio_codec import VqWav2VecCodec, Wav2Vec2Codec
    from syncvsr_amd.augment import CutMix
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.model import Model

    vq = VqWav2VecCodec.from_state_dict(model.state_dict())
    w2v = Wav2Vec2Codec.from_state_dict(W.seeded_weights("layer", 1), W.hf_config_kwargs("layer"))
    m_vq = Model(default_lrw_config(model__bert__num_hidden_layers=1))
    with pytest.raises(ValueError, match="'vq' codec"):
        m_vq.attach_audio_codec(w2v)
    m_w2v = Model(default_lrw_config(model__bert__num_hidden_layers=1, model__wav2vec__path="facebook/wav2vec2-large-xlsr-53"))
    with pytest.raises(ValueError, match="'wav2vec2' codec"):
        m_w2v.attach_audio_codec(vq)
    with pytest.raises(TypeError):
        m_vq.attach_audio_codec(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="VqWav2VecCodec"):
        CutMix(500, wav2vec=w2v)
    with pytest.raises(TypeError):
        CutMix(500, wav2vec=torch.nn.Linear(2, 2))
    assert CutMix(500).wav2vec is None
    n = sum(p.numel() for p in m_vq.parameters())
    keys = set(m_vq.state_dict())
    m_vq.attach_audio_codec(vq)
    assert sum(p.numel() for p in m_vq.parameters()) == n
    assert set(m_vq.state_dict()) - keys == {"wav2vec." + k for k in vq.state_dict()}
    assert m_vq.cutmix.wav2vec is vq and not any(k.startswith("cutmix.") for k in m_vq.state_dict())


def test_against_fairseq():
    """Skipped where fairseq is not installed (it is not installable next to this package's torch): see the module docstring."""
    pytest.importorskip("fairseq")
    from fairseq.models.wav2vec import Wav2VecModel

    args = SimpleNamespace(**R.fairseq_args(), prediction_steps=1, sample_distance=None, num_negatives=1, activation="relu", dropout=0.0,
                           dropout_features=0.0, dropout_agg=0.0, conv_aggregator_layers="[(512, 2, 1)]", skip_connections_agg=False,
                           residual_scale=0.5, project_features="none", no_conv_bias=False, agg_zero_pad=False, cross_sample_negatives=0,
                           negative_sampling_seed=None, offset="auto", balanced_classes=False, infonce=False, aggregator="cnn", vq_temp="(2.0, 0.5, 0.999995)",
                           vq_depth=1, vq_gamma=0.25)
    fs = Wav2VecModel.build_model(args, None).eval()
    mine = R.seeded_model(1)
    fs.load_state_dict(mine.state_dict(), strict=False)
    wave = R.synthetic_waveform(2, 2960, 5)
    with torch.no_grad():
        idx = fs.vector_quantizer.forward_idx(fs.feature_extractor(wave))[1]
    assert torch.equal(idx, R.oracle(mine, wave)[0])


def test_sentence_level_model_still_refuses_the_vq_tokeniser(model):
    """Its `audios` slot tokenises with the wav2vec2 codec only; a `vq` model there keeps taking pre-computed tokens."""
    from syncvsr_amd.audio_codec import VqWav2VecCodec
    from syncvsr_amd.lrs_init import default_lrs_args
    from syncvsr_amd.lrs_model import E2E

    args = default_lrs_args(adim=128, aheads=2, eunits=256, elayers=1, ddim=128, dheads=2, dunits=256, dlayers=1, codec="vq")
    e2e = E2E(41, args)
    with pytest.raises(ValueError, match="sentence-level"):
        e2e.attach_audio_codec(VqWav2VecCodec.from_state_dict(model.state_dict()))
    assert e2e._modules.get("wav2vec") is None
