"""fp64 torch restatement of the reference's TransformerLM (LRS/video/espnet/nets/pytorch_backend/lm/transformer.py with
transformer/encoder.py input_layer="linear", encoder_layer.py pre-LN blocks, attention.py MultiHeadedAttention, embedding.py
PositionalEncoding), written from its state dict: what the LM-scorer tests re-score returned hypotheses with, along their own path.
`round_to` (e.g. torch.bfloat16) rounds the weights and every layer output to that format: the noise floor of a bf16 stack."""
from __future__ import annotations

import math

import torch


def _sinusoid(L: int, D: int) -> torch.Tensor:
    pos = torch.arange(L, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, D, 2, dtype=torch.float32) * -(math.log(10000.0) / D))
    pe = torch.zeros(L, D)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
    return pe.double()


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def lm_logits(sd: dict, conf: dict, ys: torch.Tensor, round_to=None) -> torch.Tensor:
    """ys int64 [n, L] -> logits fp64 [n, L, V] of every position (key mask: ys != 0 AND causal)."""
    rnd = (lambda t: t) if round_to is None else (lambda t: t.to(round_to).double())
    W = {k: rnd(v.double()) if k.endswith(".weight") and v.dim() == 2 else v.double() for k, v in sd.items()}
    n, L = ys.shape
    D, H = conf["att_unit"], conf["head"]
    dk = D // H
    x = W["embed.weight"][ys]
    x = rnd(x @ W["encoder.embed.0.weight"].T + W["encoder.embed.0.bias"])
    x = torch.relu(_ln(x, W["encoder.embed.1.weight"], W["encoder.embed.1.bias"], 1e-5))
    x = rnd(x * math.sqrt(D) + _sinusoid(L, D))
    mask = (ys != 0).unsqueeze(1) & torch.tril(torch.ones(L, L, dtype=torch.bool)).unsqueeze(0)          # [n, L(query), L(key)]
    for i in range(conf["layer"]):
        p = f"encoder.encoders.{i}"
        t = rnd(_ln(x, W[f"{p}.norm_mha.weight"], W[f"{p}.norm_mha.bias"], 1e-12))
        q, k, v = (rnd(t @ W[f"{p}.self_attn.linear_{c}.weight"].T + W[f"{p}.self_attn.linear_{c}.bias"]).view(n, L, H, dk).transpose(1, 2)
                   for c in "qkv")
        sc = (q @ k.transpose(-2, -1)) / math.sqrt(dk)
        m = mask.unsqueeze(1)
        att = torch.softmax(sc.masked_fill(~m, -1e300), dim=-1).masked_fill(~m, 0.0)                     # attention.py:81-90
        ctx = rnd((att @ v).transpose(1, 2).reshape(n, L, D))
        x = rnd(x + ctx @ W[f"{p}.self_attn.linear_out.weight"].T + W[f"{p}.self_attn.linear_out.bias"])
        t = rnd(_ln(x, W[f"{p}.norm_ff.weight"], W[f"{p}.norm_ff.bias"], 1e-12))
        h = rnd(torch.relu(t @ W[f"{p}.feed_forward.w_1.weight"].T + W[f"{p}.feed_forward.w_1.bias"]))
        x = rnd(x + h @ W[f"{p}.feed_forward.w_2.weight"].T + W[f"{p}.feed_forward.w_2.bias"])
    x = rnd(_ln(x, W["encoder.after_norm.weight"], W["encoder.after_norm.bias"], 1e-12))
    return x @ W["decoder.weight"].T + W["decoder.bias"]


class LMRestatement:
    """The restatement behind the scorer interface of the search (stateless: every call scores the whole prefix)."""

    def __init__(self, sd: dict, conf: dict, round_to=None):
        self.sd, self.conf, self.round_to = sd, conf, round_to

    def batch_init_state(self, x):
        return None

    def select_states(self, states, prev, tok):
        return None

    def batch_score(self, ys: torch.Tensor, states, xs=None):
        return torch.log_softmax(lm_logits(self.sd, self.conf, ys, self.round_to)[:, -1], dim=-1), None

    def forward(self, x: torch.Tensor, t: torch.Tensor):
        """lm/transformer.py:140-174 -> (nll / count, nll, count)."""
        logp = torch.log_softmax(lm_logits(self.sd, self.conf, x, self.round_to), dim=-1)
        loss = -logp.gather(-1, t.unsqueeze(-1)).squeeze(-1)
        mask = (x != 0).double()
        return (loss * mask).sum() / mask.sum(), (loss * mask).sum(), mask.sum()
