"""DC-TCN word-level model, host side (no GPU): the fp64 restatement against the goldens recorded from the reference, the module's
state-dict surface against the reference's own key list, the documented refusals, and the C ABI of the new kernels."""
import os
import re

import pytest
import torch

from dctcn_cases import DCTCN_CASES, audio_rows, dctcn_subcase, dctcn_tags, load_golden, rel_err
from dctcn_restatement import dctcn_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svsr_tconv_fwd", "svsr_tcn_se_fwd", "svsr_tcn_norm_pool_fwd")
CASES = [(n, t) for n in DCTCN_CASES for t in dctcn_tags(n)]


@pytest.mark.parametrize("name,tag", CASES)
def test_restatement_matches_the_reference_golden_in_fp64(name, tag):
    """Large tensors are stored in fp32 (6e-8 relative), scalars and the word logits in fp64."""
    cfg, dims, sd, batch = dctcn_subcase(name, tag)
    gold = load_golden(name)
    keep = {}
    out = dctcn_forward(sd, dims, *batch, lambda_audio=float(cfg.optim.lambda_audio), keep=keep)
    B, C, T = out["last_hidden_states"].shape
    assert rel_err(out["last_hidden_states"], gold[f"{tag}.last_hidden_states"]) < 1e-6
    assert rel_err(out["logits_category"], gold[f"{tag}.logits_category"]) < 1e-9
    assert rel_err(out["logits_audio"].reshape(B * T, -1)[audio_rows(B, T)], gold[f"{tag}.logits_audio"]) < 1e-6
    for k in ("loss_total", "loss_category", "loss_audio", "accuracy_top1", "accuracy_top5"):
        assert abs(float(out[k]) - float(gold[f"{tag}.{k}"])) <= 1e-9 * max(1.0, abs(float(gold[f"{tag}.{k}"]))), k
    assert 0.0 < float(gold[f"{tag}.accuracy_top1"]) < float(gold[f"{tag}.accuracy_top5"])       # the accuracy checks are not vacuous
    if tag == "nowb_t7":
        for k, v in keep.items():
            assert rel_err(v, gold[f"{tag}.{k}"]) < 1e-6, k


@pytest.mark.parametrize("name,tag", CASES)
def test_module_state_dict_has_the_reference_keys_and_shapes(name, tag):
    from syncvsr_amd.dctcn import DCTCNLightningModule

    cfg, dims, sd, _ = dctcn_subcase(name, tag)
    gold = load_golden(name)
    want = {str(k): tuple(int(d) for d in str(s).split(",") if d) for k, s in zip(gold[f"{tag}.state_keys"], gold[f"{tag}.state_shapes"])}
    model = DCTCNLightningModule(cfg)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == want
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    if name == "dctcn_full":
        # Lipreading itself has 752 entries; lightning.py:238-239 moves `model.tcn.tcn_output.{weight,bias}` out to `video_classifier.*`
        assert sum(k.startswith("model.") for k in got) == 750 and "model.tcn.tcn_output.weight" not in got
    model.load_state_dict(dict(sd, **{"wav2vec.feature_extractor.conv_layers.0.0.weight": torch.zeros(3)}))        # codec keys are ignored
    missing = dict(sd)
    del missing["model.tcn.tcn_trunk.features.denseblock1.denselayer1.cbcr0_0.net.0.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        model.load_state_dict(missing)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        model.load_state_dict(dict(sd, extra=torch.zeros(1)))


@pytest.mark.parametrize("path,value,word", [
    ("model.dctcn.backbone_type", "shufflenet", "backbone_type"),
    ("model.dctcn.relu_type", "prelu", "relu_type"),
    ("model.dctcn.width_mult", 0.5, "width_mult"),
    ("model.dctcn.extract_feats", True, "extract_feats"),
    ("model.dctcn.tcn_options", dict(kernel_size=[3], num_layers=4, dropout=0.2, dwpw=False, width_mult=1), "tcn_options"),
    ("model.dctcn.densetcn_options.kernel_size_set", [3, 5, 9], "kernel size 9"),
    ("model.dctcn.densetcn_options.kernel_size_set", [3, 5, 7, 9], "kernel_size_set"),
    ("model.dctcn.densetcn_options.dilation_size_set", [1, 2, 6], "dilation 6"),
    ("model.dctcn.densetcn_options.growth_rate_set", [384, 384, 384, 96], "growth rate 96"),
    ("model.dctcn.densetcn_options.reduced_size", 500, "reduced_size"),
    ("model.dctcn.densetcn_options.squeeze_excitation", False, "squeeze_excitation"),
])
def test_unsupported_options_raise_the_documented_error(path, value, word):
    from syncvsr_amd.dctcn import DCTCNLightningModule
    from syncvsr_amd.dctcn_init import default_dctcn_config

    cfg = default_dctcn_config()
    cfg.set_path(path, value)
    with pytest.raises(NotImplementedError, match=re.escape(word)):
        DCTCNLightningModule(cfg)


def test_every_reason_is_listed_together_and_both_loss_weight_names_are_taken():
    from syncvsr_amd.dctcn import DCTCNLightningModule
    from syncvsr_amd.dctcn_init import default_dctcn_config, tiny_dctcn_config

    cfg = default_dctcn_config(model__dctcn__relu_type="relu", model__dctcn__width_mult=2.0)
    with pytest.raises(NotImplementedError) as e:
        DCTCNLightningModule(cfg)
    assert "relu_type" in str(e.value) and "width_mult" in str(e.value)
    cfg = tiny_dctcn_config()
    assert DCTCNLightningModule(cfg).lambda_audio == 10.0
    del cfg.optim["lambda_audio"]
    cfg.optim["loss_audio_weight"] = 3.0
    m = DCTCNLightningModule(cfg)
    assert m.lambda_audio == 3.0 and m.vq_groups == 2 and m.audio_vocab_size == 320 and m.audio_alignment == 4


def test_training_mode_forward_is_refused_not_run():
    from syncvsr_amd.dctcn import DCTCNLightningModule
    from syncvsr_amd.dctcn_init import dctcn_synthetic_batch, tiny_dctcn_config

    cfg = tiny_dctcn_config()
    m = DCTCNLightningModule(cfg)
    assert not m.training
    m.train()
    videos, tokens, labels, wm, am = dctcn_synthetic_batch(cfg, 2, 7, size=40)
    with pytest.raises(NotImplementedError, match="eval"):
        m(videos, tokens, labels, wm, am)
    with pytest.raises(NotImplementedError, match="eval"):
        m.predict(videos, wm, am)


def test_new_symbols_are_declared_and_exported():
    from syncvsr_amd import _lib

    decl = _lib.parse_header()
    for n in NEW_SYMBOLS:
        assert n in decl, f"{n} is not declared in include/syncvsr_hip.h"
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), f"{n} is not exported"
    src = open(os.path.join(ROOT, "syncvsr_amd", "csrc", "dctcn.hip")).read()
    assert "atomic" not in src.lower().replace("no atomics", ""), "the back-end kernels use no atomics (bit-identical runs)"
