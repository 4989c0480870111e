"""dctcn_train.DCTCNTrainStep's data-parallel and accumulation arguments, as far as the host decides them (no device): the per-rank dropout
seed rule, the constructor's refusals (each before any device work: the module sits on the CPU here) and the configuration entry."""
import itertools

import pytest
import torch


def _model(**kw):
    from syncvsr_amd.dctcn import DCTCNLightningModule
    from syncvsr_amd.dctcn_init import tiny_dctcn_config

    return DCTCNLightningModule(tiny_dctcn_config(True, **kw))


def test_dropout_seed_is_injective_over_ranks_and_micro_steps():
    from syncvsr_amd.dctcn_train import dropout_seed

    for total, accumulate, world in ((5, 1, 2), (5, 2, 2), (7, 3, 4), (1, 1, 4), (4, 4, 3)):
        pairs = list(itertools.product(range(world), range(total * accumulate)))
        seeds = [dropout_seed(11, r, total, accumulate, i) for r, i in pairs]
        assert len(set(seeds)) == len(pairs), (total, accumulate, world)
        # a rank's seeds are one contiguous run behind the previous rank's
        assert min(seeds) == 11 and max(seeds) == 11 + world * total * accumulate - 1
    for i in range(9):
        assert dropout_seed(11, 0, 5, 1, i) == 11 + i          # rank 0, accumulate = 1: the single-process step's seed
    assert dropout_seed(3, 1, 5, 2, 4) == 3 + 10 + 4


def test_constructor_refuses_bad_arguments_before_device_work():
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    m = _model()
    with pytest.raises(ValueError, match="accumulate"):
        DCTCNTrainStep(m, 5, accumulate=0)
    with pytest.raises(ValueError, match="grad_comm_dtype"):
        DCTCNTrainStep(m, 5, grad_comm_dtype=torch.float16)
    assert m._store is None, "a refused constructor must not have built the parameter store"


def test_configured_accumulation_needs_the_argument_or_from_config():
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    m = _model(train__accumulate_grad_batches=2)
    with pytest.raises(ValueError, match="accumulate_grad_batches") as e:
        DCTCNTrainStep(m, 5)
    assert "accumulate=" in str(e.value) and "from_config" in str(e.value)          # the message points at the way out
    assert m._store is None
    assert DCTCNTrainStep.from_config(m, 5).window.n == 2          # reads train.accumulate_grad_batches itself
    assert DCTCNTrainStep.from_config(m, 5, accumulate=3).window.n == 3          # an explicit argument wins
    assert DCTCNTrainStep(m, 5, accumulate=1).window.n == 1
    plain = DCTCNTrainStep.from_config(_model(), 5)
    assert plain.window.n == 1 and plain.dp is None and plain.last_reduce is None and plain.micro_steps == 0
