"""Seeded language-model cases of the LM-scorer tests (tests/test_lrs_lm_cpu.py, tests/test_gpu_lrs_lm.py): configuration, weights
regenerated from a seed under the reference's state-dict names, and the golden numbers tests/golden/make_golden_lrs_lm.py recorded."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (LM arguments, vocabulary units, weight seed, gain of the output layer).  The gain multiplies `decoder.weight` so that the
# random-init posteriors are peaked: the language model then changes what the search finds, and near-ties do not decide the n-best order.
# Tiny case: seed and gain were picked on the REFERENCE alone (make_golden_lrs_lm.py asserts the conditions): margins of 13.2 / 10.2 / 9.0
# between best and runner-up in the three runs, and log-probabilities spanning about [-14, 0] — with a gain of 6 or 12 the span doubles /
# quadruples and the fp64 restatement with weights and layer outputs rounded to bf16 (tests/lm_restatement.py round_to=) already
# deviates from the reference by 0.11-0.17 / 0.21-0.36 absolute at the tails: no bf16 stack could meet the 0.1 absolute bound the decoder
# scorer's test uses; at gain 3 that floor is 0.05.
LM_CASES = {
    "lrs_lm_tiny": (dict(layer=2, unit=256, att_unit=128, embed_unit=64, head=2, pos_enc="sinusoidal", model_module="transformer"), 41, 8, 3.0),
    "lrs_lm_full": (dict(layer=16, unit=2048, att_unit=512, embed_unit=128, head=8, pos_enc="sinusoidal", model_module="transformer"), 5049, 4, 6.0),
}
# (beam, ctc_weight, lm_weight) of the recorded searches on the lrs_infer_tiny clip
LM_RUNS = [(5, 0.1, 0.5), (30, 0.1, 0.5), (30, 0.1, 0.0)]


def lm_key_shapes(conf: dict, n_vocab: int, norms=("norm_ff", "norm_mha")) -> list:
    """State-dict keys and shapes of the reference's TransformerLM, in its own order (encoder_layer.py:59-60 creates norm_ff first)."""
    E, D, U = conf["embed_unit"], conf["att_unit"], conf["unit"]
    out = [("embed.weight", (n_vocab, E)), ("encoder.embed.0.weight", (D, E)), ("encoder.embed.0.bias", (D,)), ("encoder.embed.1.weight", (D,)),
           ("encoder.embed.1.bias", (D,))]
    for i in range(conf["layer"]):
        p = f"encoder.encoders.{i}"
        for k in ("linear_q", "linear_k", "linear_v", "linear_out"):
            out += [(f"{p}.self_attn.{k}.weight", (D, D)), (f"{p}.self_attn.{k}.bias", (D,))]
        out += [(f"{p}.feed_forward.w_1.weight", (U, D)), (f"{p}.feed_forward.w_1.bias", (U,)), (f"{p}.feed_forward.w_2.weight", (D, U)),
                (f"{p}.feed_forward.w_2.bias", (D,))]
        for k in norms:
            out += [(f"{p}.{k}.weight", (D,)), (f"{p}.{k}.bias", (D,))]
    out += [("encoder.after_norm.weight", (D,)), ("encoder.after_norm.bias", (D,)), ("decoder.weight", (n_vocab, D)), ("decoder.bias", (n_vocab,))]
    return out


def lm_state_dict(name: str) -> dict:
    """fp32 weights of case `name`: matrices uniform in +-1.5/sqrt(fan_in), biases +-0.1, norm gains 1 +- 0.1, embeddings N(0, 1)."""
    conf, V, seed, gain = LM_CASES[name]
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in lm_key_shapes(conf, V, norms=("norm_mha", "norm_ff")):          # (the order the values are drawn in; returned in the reference's)
        if k == "embed.weight":
            t = torch.randn(shape, generator=g)
        elif k.endswith(".weight") and len(shape) == 2:
            t = (torch.rand(shape, generator=g) * 2 - 1) * (1.5 / math.sqrt(shape[1]))
        elif k.endswith(".weight"):
            t = 1.0 + 0.1 * (torch.rand(shape, generator=g) * 2 - 1)
        else:
            t = 0.1 * (torch.rand(shape, generator=g) * 2 - 1)
        sd[k] = t
    sd["decoder.weight"] = sd["decoder.weight"] * gain
    return {k: sd[k] for k, _ in lm_key_shapes(conf, V)}


def lm_case(name: str, load_golden: bool = True):
    """-> (conf, n_vocab, state dict, golden npz | None)"""
    conf, V, _, _ = LM_CASES[name]
    gold = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False) if load_golden else None
    return dict(conf), V, lm_state_dict(name), gold


def token0_prefixes(V: int) -> torch.Tensor:
    """Hand-made prefixes [6, 7] with token 0 at interior positions (the `ys != 0` key mask): one row without, rows with one, two, and
    two adjacent zeros, a zero right behind <sos>, and one that ENDS in 0 (its own key is masked too)."""
    s = V - 1
    return torch.tensor([[s, 3, 7, 2, 9, 4, 5],
                         [s, 3, 0, 2, 9, 4, 5],
                         [s, 0, 7, 2, 0, 4, 5],
                         [s, 3, 7, 0, 0, 4, 5],
                         [s, 0, 0, 2, 9, 0, 5],
                         [s, 3, 7, 2, 9, 4, 0]], dtype=torch.int64) % V
