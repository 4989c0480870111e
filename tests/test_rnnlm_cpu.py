"""Recurrent language-model scorer without a GPU: the reference's state-dict keys, the float64 restatement pinned to the recorded reference
numbers (tests/golden/lrs_rnnlm_tiny.npz), `load_lm`'s dispatch on `model_module`, the packed weight layout and the row arithmetic of
`select_states`."""
import json

import numpy as np
import pytest
import torch

from lm_cases import lm_case
from rnnlm_cases import RNNLM_CASES, V, load_golden, rnnlm_key_shapes, rnnlm_state_dict
from rnnlm_restatement import RNNLMRestatement, bf16_round


@pytest.fixture(scope="module")
def gold():
    return load_golden()


@pytest.mark.parametrize("case", list(RNNLM_CASES))
def test_state_dict_keys_are_the_references(gold, case):
    from syncvsr_amd.lrs_lm import RNNLM

    conf, seed = RNNLM_CASES[case]
    lm = RNNLM(V, conf)
    sd = lm.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f"{case}.state_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in gold[f"{case}.state_shapes"]]
    assert list(sd.keys()) == [k for k, _ in rnnlm_key_shapes(conf)]
    assert not lm.training and not any(p.requires_grad for p in lm.parameters())
    lm.load_state_dict(rnnlm_state_dict(conf, seed), strict=True)
    if conf["tie_weights"]:
        assert lm.predictor.lo.weight is lm.predictor.embed.weight
    with pytest.raises(RuntimeError, match="inference-only"):
        lm.train(True)
    assert lm.final_score(None) == 0.0 and lm.init_state(None) is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.batch_score(torch.zeros((1, 1), dtype=torch.int64), None, None)


@pytest.mark.parametrize("case", list(RNNLM_CASES))
def test_restatement_matches_the_recorded_reference(gold, case):
    """The bound tests/test_oracle_golden.py pins its restatements to the goldens with: rtol 1e-5, atol 1e-6."""
    conf, seed = RNNLM_CASES[case]
    ref = RNNLMRestatement(rnnlm_state_dict(conf, seed), conf)
    logp, h, c = ref.run(gold[f"{case}.tok"], gold[f"{case}.prev"])
    np.testing.assert_allclose(logp, gold[f"{case}.logp"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(h, gold[f"{case}.h"], rtol=1e-5, atol=1e-6)
    if conf["type"] == "lstm":
        np.testing.assert_allclose(c, gold[f"{case}.c"], rtol=1e-5, atol=1e-6)
    else:
        assert c is None and f"{case}.c" not in gold.files
    np.testing.assert_allclose(np.array(ref.forward(gold[f"{case}.fwd.x"], gold[f"{case}.fwd.t"])), gold[f"{case}.fwd.out"], rtol=1e-5, atol=1e-6)
    assert int(gold[f"{case}.fwd.out"][2]) == int((gold[f"{case}.fwd.x"] != 0).sum())


def test_load_lm_dispatches_on_model_module(tmp_path):
    """lightning.py:255 / lm_interface.py:61-66: no model_module, or "default", is the recurrent LM; "transformer" the transformer LM; seq_rnn
    and foreign modules are refused with the reason."""
    from syncvsr_amd.lrs_lm import RNNLM, TransformerLM, load_lm

    conf, seed = RNNLM_CASES["lstm2"]
    sd = rnnlm_state_dict(conf, seed)
    torch.save(sd, tmp_path / "rnnlm.model.best")
    (tmp_path / "model.json").write_text(json.dumps(dict(conf, backend="pytorch")))                       # no model_module at all
    lm = load_lm(V, str(tmp_path / "rnnlm.model.best"))
    assert isinstance(lm, RNNLM) and not lm.training and lm.typ == "lstm" and (lm.layers, lm.unit, lm.embed_unit) == (2, 96, 64)
    assert all(torch.equal(lm.state_dict()[k], v) for k, v in sd.items())
    for module in ("default", "espnet.nets.pytorch_backend.lm.default:DefaultRNNLM"):
        got = load_lm(V, str(tmp_path / "rnnlm.model.best"), dict(conf, model_module=module))
        assert isinstance(got, RNNLM)
    assert isinstance(TransformerLM.from_files(V, str(tmp_path / "rnnlm.model.best"), dict(conf)), RNNLM)
    torch.save({"model": sd}, tmp_path / "snapshot")
    assert isinstance(load_lm(V, str(tmp_path / "snapshot"), dict(conf)), RNNLM)
    gconf, gseed = RNNLM_CASES["gru1"]
    torch.save(rnnlm_state_dict(gconf, gseed), tmp_path / "gru")
    assert load_lm(V, str(tmp_path / "gru"), dict(gconf, model_module="default")).typ == "gru"
    for module in ("seq_rnn", "somewhere.else:LM"):
        with pytest.raises(NotImplementedError, match=module):
            load_lm(V, str(tmp_path / "rnnlm.model.best"), dict(conf, model_module=module))
    # the reference reads args.type / layer / unit without defaults: a config that lacks one was not written for this module
    with pytest.raises(NotImplementedError, match="lacks type"):
        load_lm(V, str(tmp_path / "rnnlm.model.best"), {k: v for k, v in conf.items() if k != "type"})
    with pytest.raises(NotImplementedError, match="lacks layer, unit"):
        load_lm(V, str(tmp_path / "rnnlm.model.best"), dict(type="lstm", model_module="default"))
    tconf, tV, tsd, _ = lm_case("lrs_lm_tiny")
    torch.save(tsd, tmp_path / "tlm")
    assert isinstance(load_lm(tV, str(tmp_path / "tlm"), dict(tconf)), TransformerLM)                     # model_module="transformer": as before
    assert load_lm(V, lm) is lm
    with pytest.raises(ValueError, match="units"):
        load_lm(V + 1, lm)
    with pytest.raises(NotImplementedError, match="Linear"):
        load_lm(V, torch.nn.Linear(2, 2))


def test_unsupported_configurations_are_named_at_construction():
    from syncvsr_amd.lrs_lm import RNNLM

    with pytest.raises(NotImplementedError, match="unit = 5000.*embed_unit = 4100"):
        RNNLM(V, dict(type="lstm", layer=1, unit=5000, embed_unit=4100))
    with pytest.raises(ValueError, match="rnn"):
        RNNLM(V, dict(type="rnn", layer=1, unit=64))
    with pytest.raises(ValueError, match="Tie Weights"):
        RNNLM(V, dict(type="lstm", layer=1, unit=96, embed_unit=64, tie_weights=True))
    lm = RNNLM(V, dict(type="gru", layer=2, unit=650))
    assert (lm.embed_unit, lm.unit_pad, lm.embed_pad) == (650, 704, 704)
    assert lm.workspace_bytes(40) == 2 * 40 * 704 * (2 * 4 + 2) + 40 * 8


@pytest.mark.parametrize("gru", [False, True])
@pytest.mark.parametrize("E,U", [(64, 64), (64, 96), (650, 650)])
def test_packed_weights_round_trip(E, U, gru):
    """pack_rnn_cell -> unpack_rnn_cell gives back the bf16-rounded matrices and the bias rows, the padding holds zeros only, and single
    entries sit where include/syncvsr_hip.h says lane l of the MFMA B fragment reads them."""
    from syncvsr_amd.lrs_lm import pack_rnn_cell, unpack_rnn_cell

    G = 3 if gru else 4
    g = torch.Generator().manual_seed(E + U + G)
    w_ih, w_hh = torch.randn(G * U, E, generator=g), torch.randn(G * U, U, generator=g)
    b_ih, b_hh = torch.randn(G * U, generator=g), torch.randn(G * U, generator=g)
    wpk, bias = pack_rnn_cell(w_ih, w_hh, b_ih, b_hh, gru)
    Ep, Up = (E + 63) // 64 * 64, (U + 63) // 64 * 64
    assert wpk.shape == (Up // 16, (Ep + Up) // 32, G, 64, 8) and wpk.dtype == torch.bfloat16 and wpk.is_contiguous()
    assert bias.shape == (Up // 16, 4, 16) and bias.dtype == torch.float32
    r_ih, r_hh, b4, rest = unpack_rnn_cell(wpk, bias, E, U, gru)
    assert torch.equal(r_ih, w_ih.bfloat16().float()) and torch.equal(r_hh, w_hh.bfloat16().float())
    assert float(rest.abs().max()) == 0.0
    bi, bh = b_ih.view(G, U), b_hh.view(G, U)
    want = torch.stack((bi[0] + bh[0], bi[1] + bh[1], bi[2], bh[2])) if gru else bi + bh
    assert torch.equal(b4, want)
    for t, s, gate, lane, j in ((0, 0, 0, 0, 0), (Up // 16 - 1, 1, G - 1, 37, 5), (1, Ep // 32, 1, 63, 7), (2, (Ep + Up) // 32 - 1, 2, 16, 3)):
        u, k = 16 * t + (lane & 15), 32 * s + 8 * (lane >> 4) + j
        if u >= U:
            want_v = 0.0
        elif k < Ep:
            want_v = float(w_ih.view(G, U, E)[gate, u, k].bfloat16()) if k < E else 0.0
        else:
            want_v = float(w_hh.view(G, U, U)[gate, u, k - Ep].bfloat16()) if k - Ep < U else 0.0
        assert float(wpk[t, s, gate, lane, j]) == want_v, (t, s, gate, lane, j)


def test_select_states_moves_row_indices_only():
    """Scripted select_states / pruning sequence on the host: the rows a state names are those of the hypotheses' own parents, through a
    permutation, duplicated parents, the search's pruning and a shrinking beam; the state's buffers, side and step stay as they were."""
    from syncvsr_amd.lrs_lm import RNNLM, RNNBuffers, RNNState, select_rows

    lm = RNNLM(V, RNNLM_CASES["gru1"][0])
    bufs = RNNBuffers(layers=1, capacity=8, width=128, lstm=False, device="cpu")
    assert bufs.h.shape == (2, 1, 8, 128) and bufs.c is None and bufs.nbytes() == lm.workspace_bytes(8)
    fresh = RNNState(bufs, None, 1, 0)
    assert select_rows(None, torch.tensor([0, 0])) is None and lm.select_states(fresh, torch.tensor([0, 0]), None).rows is None and len(fresh) == 0
    owner = list(range(5))                                                    # hypothesis -> state row, as a scoring call leaves it
    state = RNNState(bufs, bufs.iota[:5], 0, 1)
    for prev, keep in ((torch.tensor([4, 0, 0, 2, 1]), None), (torch.tensor([1, 1, 3]), torch.tensor([0, 2])), (torch.tensor([1, 0, 1, 1]), torch.tensor([3]))):
        state = lm.select_states(state, prev, torch.zeros_like(prev))
        owner = [owner[int(p)] for p in prev]
        if keep is not None:
            state = state[keep]                                               # BatchBeamSearch._take: ended hypotheses leave
            owner = [owner[int(k)] for k in keep]
        assert state.rows.dtype == torch.int64 and state.rows.tolist() == owner and len(state) == len(owner)
        assert state.bufs is bufs and (state.parity, state.gen) == (0, 1)
    assert lm.select_states(None, torch.tensor([0]), None) is None and lm.select_state(None, 0) is None


def test_bf16_rounding_of_the_restatement_is_torchs():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3
    x[:4] = torch.tensor([0.0, 1.0, 1.00390625, 1.01171875])                    # exact, and two ties (to even: down, up)
    assert np.array_equal(bf16_round(x.numpy()), x.bfloat16().double().numpy())
