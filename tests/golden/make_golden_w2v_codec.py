"""Writes tests/golden/w2v_codec.npz: the seeded full-size wav2vec2 tokeniser weights of tests/w2v_codec_ref.py loaded into HF transformers'
Wav2Vec2ForPreTraining (both feat_extract_norm modes), run as the reference's forward_audios runs it (feature_extractor ->
feature_projection -> quantizer with codevectors = arange(640), eval mode).

    python tests/golden/make_golden_w2v_codec.py

Cases (B = 2): LRS clips of T = 12 and T = 29 video frames (640 samples each) with the 8000 appended zeros, and an odd-length row
(12 * 640 + 3 samples + 8000).  Stored per mode and case: eval tokens, per-layer checksums (sum and sum of |x| of every layer output), and for
T = 12 the 640 logits of every frame (float16, to keep the file small).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import w2v_codec_ref as R  # noqa: E402

CASES = {"t12": 12 * 640, "t29": 29 * 640, "odd": 12 * 640 + 3}
PAD = 8000
WAVE_SEED = 21
WEIGHT_SEED = 1


def hf_run(mode: str, wave: torch.Tensor):
    from transformers import Wav2Vec2Config, Wav2Vec2ForPreTraining

    torch.manual_seed(0)
    m = Wav2Vec2ForPreTraining(Wav2Vec2Config(**R.hf_config_kwargs(mode))).eval()
    m.load_state_dict(R.seeded_weights(mode, WEIGHT_SEED), strict=False)
    cv = torch.arange(m.quantizer.codevectors.size(1)).view(1, -1, 1).expand_as(m.quantizer.codevectors)
    m.quantizer.codevectors.data = cv.float()
    x = torch.cat([wave.squeeze(1), torch.zeros(wave.size(0), PAD)], dim=-1)
    layers = []
    with torch.no_grad():
        h = x[:, None]
        for conv in m.wav2vec2.feature_extractor.conv_layers:
            h = conv(h)
            layers.append(h.transpose(1, 2))
        _, f = m.wav2vec2.feature_projection(h.transpose(1, 2))
        tok = m.quantizer(f)[0].unflatten(-1, (2, -1))[..., 0].long()
        z = m.quantizer.weight_proj(f)
    return tok, z, layers


def main() -> None:
    out = {}
    for mode in ("layer", "group"):
        for name, L in CASES.items():
            wave = R.synthetic_waveform(2, L, WAVE_SEED)
            tok, z, layers = hf_run(mode, wave)
            out[f"{mode}_{name}_tokens"] = tok.numpy().astype(np.int16)
            out[f"{mode}_{name}_checksums"] = np.array([[t.sum().item(), t.abs().sum().item()] for t in layers], dtype=np.float64)
            if name == "t12":
                out[f"{mode}_{name}_logits"] = z.numpy().astype(np.float16)
    np.savez_compressed(os.path.join(HERE, "w2v_codec.npz"), **out)


if __name__ == "__main__":
    main()
