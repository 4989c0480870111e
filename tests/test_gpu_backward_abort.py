"""A backward that aborts on a host exception leaves nothing for the next one (-m gpu).

The hand-written backward passes postpone work: parameter-gradient reductions wait in `model._deferred` for the layer's hand-over to the
side stream, linear weight gradients wait in `model._wg_group` for one grouped launch.  A Python exception between collecting and
handing over leaves closures over the aborted pass's tensors behind; issued by the next backward they would add that pass's reductions
into the new gradient.  `model._begin_backward` drops them.  Each case raises a plain RuntimeError from an `ops` wrapper BEFORE it
launches anything (nothing faults on the device), runs the same batch again and compares the gradient buffer bit for bit with a twin
model that only ever ran the clean pass.  Dropout is 0: the aborted forward would otherwise advance the seed word and the twin would
draw other masks."""
import pytest
import torch

from golden_cases import build_case, build_lrs_case

pytestmark = pytest.mark.gpu


def _lrw():
    from syncvsr_amd.model import Model

    cfg, sd, batch, training, gold = build_case("lrw_tiny")         # 2 clips x 5 frames x 24^2, 2 encoder layers
    return (lambda: Model(cfg)), sd, batch, (lambda out: out["loss_total"]), False


def _lrs():
    from syncvsr_amd.lrs_model import E2E

    args, odim, sd, batch, training, gold = build_lrs_case("lrs_tiny_b3", load_golden=False)      # 3 clips, <= 14 frames, 16^2, 1 + 2 layers
    return (lambda: E2E(odim, args)), sd, batch, (lambda out: out[0]), True


# which wrapper raises: the word-level pass then holds the embeddings' LayerNorm reduction in the deferred list (its grouped weight
# gradients are out already); the sentence-level pass is inside its last decoder layer, with a half-filled group and deferred entries
_CASES = {"lrw": (_lrw, "embed_bwd_scatter"), "lrs": (_lrs, "mha_bwd")}


@pytest.mark.parametrize("which", sorted(_CASES))
def test_backward_after_aborted_backward_equals_clean_backward(which, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import ops

    dev = torch.device("cuda:0")
    make, wrapper = _CASES[which]
    build, sd, batch, loss_of, small = make()
    gb = [t.to(dev) for t in batch]

    def new_model():
        m = build()
        m.load_state_dict(sd)
        m.to(dev).train()
        assert m.drop_p == 0.0 and m.attn_drop_p == 0.0
        m._side.enabled = True                # as engine.TrainStep.__init__ does
        m._side.enabled_small = small
        return m

    def backward(m):
        loss_of(m(*gb)).backward()

    def abort(*a, **k):
        raise RuntimeError("aborted on the host, before any launch")

    model = new_model()
    with monkeypatch.context() as mp:
        mp.setattr(ops, wrapper, abort)
        with pytest.raises(RuntimeError, match="aborted on the host"):
            backward(model)
    backward(model)
    torch.cuda.synchronize()
    twin = new_model()
    backward(twin)
    torch.cuda.synchronize()
    g, r = model.store().grad, twin.store().grad
    assert torch.equal(g, r), f"{int((g != r).sum())} gradient elements differ after an aborted backward (max |diff| {float((g - r).abs().max()):.3e})"
    assert model._wg_group is None and not model._deferred
