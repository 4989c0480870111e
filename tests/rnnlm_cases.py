"""Seeded recurrent-LM cases of the RNN-LM scorer tests (tests/test_rnnlm_cpu.py, tests/test_gpu_rnnlm.py): configuration, weights regenerated
from a seed under the reference's state-dict names (three cases of fp32 weights would not fit the size limit of a committed file), and the
numbers tests/golden/make_golden_rnnlm.py recorded from the reference in tests/golden/lrs_rnnlm_tiny.npz."""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V = 41                            # the vocabulary of the lrs_infer_tiny model the recorded search runs on

# name -> (LM arguments as the reference's model.json holds them, weight seed).  unit 96 pads to 128 (a padded tail), embed_unit 64 != unit.
RNNLM_CASES = {
    "lstm2": (dict(type="lstm", layer=2, unit=96, embed_unit=64, dropout_rate=0.5, emb_dropout_rate=0.0, tie_weights=False), 3),
    "gru1": (dict(type="gru", layer=1, unit=96, embed_unit=64, dropout_rate=0.5, emb_dropout_rate=0.0, tie_weights=False), 4),
    "lstm_tie": (dict(type="lstm", layer=1, unit=96, embed_unit=None, dropout_rate=0.0, emb_dropout_rate=0.0, tie_weights=True), 5),
}
STEPS, ROWS = 6, 5
# the recorded search: (case, beam, ctc_weight, lm_weight) on the lrs_infer_tiny clip.  The weight seed of ITS language model is picked by the
# generator (the first seed whose search has no near-tie at the edge of the beam: make_golden_rnnlm.py) and stored as `search.lm_seed`
SEARCH = ("lstm2", 4, 0.1, 0.3)
SEARCH_FRAMES = 6                 # encoder frames of the clip the search sees (= its length limit)
LOGP_ABS, LOGP_REL = 0.1, 1e-2    # the log-probability bounds of the transformer-LM scorer's tests (tests/test_gpu_lrs_lm.py)


def score_tol(s: float) -> float:
    """Bound on a hypothesis' total score against the reference's: the one tests/test_gpu_lrs_lm.py holds the LM-fused search to."""
    return 2e-2 * abs(s) + 0.05


def rnnlm_key_shapes(conf: dict, n_vocab: int = V) -> list:
    """State-dict keys and shapes of the reference's DefaultRNNLM, in its own order."""
    U = conf["unit"]
    E = U if conf.get("embed_unit") is None else conf["embed_unit"]
    G = 4 if conf["type"] == "lstm" else 3
    out = [("predictor.embed.weight", (n_vocab, E))]
    for i in range(conf["layer"]):
        p = f"predictor.rnn.{i}"
        out += [(f"{p}.weight_ih", (G * U, E if i == 0 else U)), (f"{p}.weight_hh", (G * U, U)), (f"{p}.bias_ih", (G * U,)), (f"{p}.bias_hh", (G * U,))]
    return out + [("predictor.lo.weight", (n_vocab, U)), ("predictor.lo.bias", (n_vocab,))]


def rnnlm_state_dict(conf: dict, seed: int, n_vocab: int = V) -> dict:
    """fp32 weights: cell matrices uniform in +-0.25 (the state matters: gates leave their linear range), cell biases +-0.2, embedding and
    output matrix +-1 (peaked posteriors: log-probabilities span about 10), output bias +-0.1.  tie_weights: lo.weight IS embed.weight."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in rnnlm_key_shapes(conf, n_vocab):
        scale = 1.0 if k in ("predictor.embed.weight", "predictor.lo.weight") else 0.1 if k == "predictor.lo.bias" else 0.2 if "bias" in k else 0.25
        sd[k] = (torch.rand(shape, generator=g) * 2 - 1) * scale
    if conf.get("tie_weights"):
        sd["predictor.lo.weight"] = sd["predictor.embed.weight"]
    return sd


def step_inputs(case: str):
    """tok int64 [STEPS, ROWS] (the token each hypothesis is extended by; a 0 among them) and prev int64 [STEPS, ROWS] (row s: the parent of each
    hypothesis of step s among those of step s - 1: permutations, duplicated parents; row 0 unused)."""
    g = torch.Generator().manual_seed(100 + RNNLM_CASES[case][1])
    tok = torch.randint(1, V - 1, (STEPS, ROWS), generator=g)
    tok[0] = V - 1
    tok[2, 1] = 0
    prev = torch.stack([torch.randperm(ROWS, generator=g) for _ in range(STEPS)])
    prev[1] = 0 * prev[1] + torch.tensor([0, 0, 1, 3, 3])            # duplicated parents
    prev[3, 4] = prev[3, 0]
    return tok, prev


def forward_pair(seed: int = 17, B: int = 3, L: int = 7):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(1, V - 1, (B, L + 1), generator=g)
    seq[:, 0] = V - 1
    x, t = seq[:, :-1].clone(), seq[:, 1:].clone()
    x[1, L - 2 :] = 0                                                 # a padded tail: those positions count for nothing in `count`
    return x, t


def load_golden():
    return np.load(os.path.join(GOLDEN, "lrs_rnnlm_tiny.npz"), allow_pickle=False)


def search_lm(gold) -> tuple:
    """-> (conf, state dict) of the language model of the recorded search."""
    conf = dict(RNNLM_CASES[SEARCH[0]][0])
    return conf, rnnlm_state_dict(conf, int(gold["search.lm_seed"]))
