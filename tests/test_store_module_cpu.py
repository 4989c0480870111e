"""model._StoreModule, the base of the three store-backed modules (no GPU): what is hoisted lives in the base alone, the loss seeds are
the fp32 products both models wrote before, and E2E carries the dropout word in its rng_state."""
import pytest
import torch

from dctcn_cases import dctcn_subcase
from golden_cases import build_case, build_lrs_case

HOISTED = ("configure_optimizers", "attach_audio_codec", "_advance_dropout", "reseed_dropout", "rng_state", "load_rng_state",
           "accumulate_into_grads", "direct_constants", "set_loss_scale", "loss_seeds", "state_dict")


def _lrw():
    from syncvsr_amd.model import Model

    cfg, sd, *_ = build_case("lrw_tiny")
    m = Model(cfg)
    m.load_state_dict(sd)
    return m


def _lrs():
    from syncvsr_amd.lrs_model import E2E

    args, odim, sd, *_ = build_lrs_case("lrs_tiny", load_golden=False)
    m = E2E(odim, args, seed=3)
    m.load_state_dict(sd)
    return m


def _dctcn():
    from syncvsr_amd.dctcn import DCTCNLightningModule

    cfg, _, sd, _ = dctcn_subcase("dctcn_tiny", "nowb_t7")
    m = DCTCNLightningModule(cfg)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def models():
    return {"lrw": _lrw(), "lrs": _lrs(), "dctcn": _dctcn()}


def test_hoisted_names_live_in_the_base_only(models):
    from syncvsr_amd.model import _StoreModule

    for which, m in models.items():
        assert isinstance(m, _StoreModule)
        own = type(m).__dict__
        for name in HOISTED:
            assert name not in own, f"{type(m).__name__} defines {name} itself"
            assert name in _StoreModule.__dict__, name
        for name in ("store", "mark_params_dirty"):          # the DC-TCN module wraps them to drop its prepared weights
            assert (name in own) == (which == "dctcn"), (which, name)


@pytest.mark.parametrize("which", ["lrw", "lrs"])
def test_loss_seeds_are_the_fp32_products(models, which):
    m = models[which]
    ws = m._loss_weights()
    assert ws == ((1.0, m.lambda_audio) if which == "lrw" else (m.mtlalpha, 1.0 - m.mtlalpha, m.audio_weight))
    seeds = m.loss_seeds(torch.device("cpu"))
    first = [torch.tensor(w, dtype=torch.float32) for w in ws]
    ptrs = [g.data_ptr() for g in seeds]
    assert len(seeds) == len(ws)
    for g, w in zip(seeds, first):
        assert g.dtype == torch.float32 and g.dim() == 0 and torch.equal(g, w)
    try:
        m.set_loss_scale(1 / 3)
        again = m.loss_seeds(torch.device("cpu"))
        for g, h, p, w in zip(seeds, again, ptrs, first):
            assert h is g and g.data_ptr() == p, "the seeds are rewritten in place: a recorded step list holds their addresses"
            assert torch.equal(g, torch.tensor(1 / 3, dtype=torch.float32) * w)
    finally:
        m.set_loss_scale(1.0)
    for g, p, w in zip(m.loss_seeds(torch.device("cpu")), ptrs, first):
        assert g.data_ptr() == p and torch.equal(g, w)


def test_lrs_rng_state_carries_the_dropout_word(models):
    m = models["lrs"]
    assert m._drop_word is None and m.dropout_seed == 0          # E2E starts its word at 0 whatever `seed` is
    assert m.rng_state() == {"dropout_word": m.dropout_seed}
    m.load_rng_state({"dropout_word": 7})
    assert m.rng_state() == {"dropout_word": 7} and m.dropout_seed == 7
    m.load_rng_state({"dropout_word": 0})


def test_xt_lrw_round_trips_layer_rng():
    from syncvsr_amd.config import xtransformers_lrw_config
    from syncvsr_amd.model import Model

    m = Model(xtransformers_lrw_config(True, model__bert__depth=2, model__bert__layer_dropout=0.4), seed=5)
    m._layer_rng.random()
    state = m.rng_state()
    assert state["dropout_word"] == 5 and state["layer_rng"] == m._layer_rng.getstate()
    draws = [m._layer_rng.random() for _ in range(3)]
    m.load_rng_state(dict(state, dropout_word=9))
    assert m.rng_state() == dict(state, dropout_word=9)
    assert [m._layer_rng.random() for _ in range(3)] == draws
    m.reseed_dropout(5)                                            # the layer-drop draws follow the seed
    import random

    assert m._layer_rng.getstate() == random.Random(5).getstate() and m.dropout_seed == 5


def test_train_step_takes_store_modules_with_a_training_step_only(models):
    from syncvsr_amd.engine import TrainStep

    for model in (models["dctcn"], torch.nn.Linear(2, 2)):          # the DC-TCN module states no loss weights: eval path only
        with pytest.raises(TypeError, match="training step"):
            TrainStep(model)
