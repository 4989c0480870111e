"""CPU checks of the wav2vec2 audio tokeniser: the fp32 restatement (tests/w2v_codec_ref.py) against the HF golden and against HF transformers
itself, the token layout, the frame-count formula, the refused configurations and the C ABI of csrc/w2v_codec.hip."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import w2v_codec_ref as R  # noqa: E402

from syncvsr_amd import audio_codec as AC  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "w2v_codec.npz")
CASES = {"t12": 12 * 640, "t29": 29 * 640, "odd": 12 * 640 + 3}
PAD = 8000


@pytest.mark.parametrize("mode", ["layer", "group"])
@pytest.mark.parametrize("case", list(CASES))
def test_restatement_matches_golden(mode, case):
    g = np.load(GOLDEN)
    sd = R.seeded_weights(mode, 1)
    wave = R.synthetic_waveform(2, CASES[case], 21)
    layers: list = []
    z = R.logits(sd, R.features(sd, mode, wave, PAD, layers_out=layers))
    tok = R.tokens_from_logits(z)
    ref = torch.from_numpy(g[f"{mode}_{case}_tokens"].astype(np.int64))
    assert tok.shape == ref.shape == (2, R.frames(CASES[case] + PAD)[-1], 2)
    sure = R.margins(z) > 1e-3          # (fp32 summation order may swap exact near-ties between two CPU builds)
    assert torch.equal(tok[sure], ref[sure])
    cs = np.array([[t.sum().item(), t.abs().sum().item()] for t in layers])
    np.testing.assert_allclose(cs[:, 1], g[f"{mode}_{case}_checksums"][:, 1], rtol=1e-4)
    np.testing.assert_allclose(cs[:, 0], g[f"{mode}_{case}_checksums"][:, 0], rtol=1e-3, atol=1e-5 * cs[:, 1].max())      # (a signed sum cancels: bound by sum |x|)
    if f"{mode}_{case}_logits" in g:
        np.testing.assert_allclose(z.numpy(), g[f"{mode}_{case}_logits"].astype(np.float32), atol=5e-3, rtol=2e-3)


@pytest.mark.parametrize("mode", ["layer", "group"])
def test_restatement_matches_hf(mode):
    transformers = pytest.importorskip("transformers")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_golden_w2v_codec import hf_run

    assert transformers is not None
    wave = R.synthetic_waveform(2, 12 * 640 + 3, 5)
    tok_hf, z_hf, _ = hf_run(mode, wave)
    sd = R.seeded_weights(mode, 1)
    tok, z = R.tokenize(sd, mode, wave, pad=PAD)
    torch.testing.assert_close(z, z_hf, atol=1e-4, rtol=1e-4)
    sure = R.margins(z) > 1e-3
    assert torch.equal(tok[sure], tok_hf[sure])


def test_group_offset_and_vocabulary():
    g = np.load(GOLDEN)
    for k in g.files:
        if k.endswith("_tokens"):
            t = g[k]
            assert (t[..., 0] >= 0).all() and (t[..., 0] < 320).all(), k
            assert (t[..., 1] >= 320).all() and (t[..., 1] < 640).all(), k
    z = torch.zeros(1, 640)
    z[0, 7] = 1.0
    z[0, 320 + 5] = 1.0
    assert R.tokens_from_logits(z).tolist() == [[7, 325]]
    z = torch.zeros(1, 640)            # ties go to the lowest index, as torch.argmax
    assert R.tokens_from_logits(z).tolist() == [[0, 320]]


@pytest.mark.parametrize("L", [400, 401, 7680 + 8000, 7683 + 8000, 102400 + 8000])
def test_frame_count_formula(L):
    x = torch.zeros(1, 1, L)
    n = []
    for k, s in zip(AC.KERNELS, AC.STRIDES):
        x = torch.nn.functional.conv1d(x, torch.zeros(1, 1, k), stride=s)
        n.append(x.size(-1))
    assert AC.frame_counts(L) == n == R.frames(L)
    # the reference's clip: 160 video frames + 8000 zeros = 110,400 samples -> 344 frames (>= T * A = 320 tokens)
    assert AC.frame_counts(160 * 640 + 8000)[-1] == 344


def _base(mode="layer"):
    return dict(R.hf_config_kwargs(mode))


@pytest.mark.parametrize("change", [
    dict(conv_dim=(256,) * 7),
    dict(conv_kernel=(10, 3, 3, 3, 3, 3, 2)),
    dict(conv_stride=(5, 2, 2, 2, 2, 2, 1)),
    dict(feat_extract_activation="relu"),
    dict(num_codevector_groups=1),
    dict(num_codevectors_per_group=100),
    dict(feat_extract_norm="batch"),
    dict(conv_bias=False),
])
def test_refused_configs(change):
    cfg = _base()
    cfg.update(change)
    with pytest.raises(NotImplementedError):
        AC.check_config(cfg)


def test_accepted_configs_and_state_dict_names():
    assert AC.check_config(_base("layer")) == "layer"
    assert AC.check_config(_base("group")) == "group"
    for mode in ("layer", "group"):
        sd = R.seeded_weights(mode, 3)
        c = AC.Wav2Vec2Codec.from_state_dict({"wav2vec." + k: v for k, v in sd.items()}, _base(mode))
        assert set(c.state_dict()) == set(sd)
        assert not list(c.parameters())
        for k, v in c.state_dict().items():
            assert torch.equal(v, sd[k])
    with pytest.raises(KeyError):
        AC.Wav2Vec2Codec.from_state_dict({}, _base("group"))


def test_codec_symbols_in_header_and_library():
    from syncvsr_amd import _lib

    names = ("svsr_w2v_conv0", "svsr_w2v_norm_gelu", "svsr_w2v_quantize", "svsr_w2v_stats_floats")
    hdr = _lib.parse_header()
    for n in names:
        assert n in hdr, n
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n
    assert lib.svsr_steplist_knows(b"svsr_w2v_quantize") == 1
    assert lib.svsr_w2v_stats_floats(2, 100) == 2 * 2 * 2 * 512 + 2 * 2 * 512
    assert lib.svsr_w2v_stats_floats(0, 100) < 0
