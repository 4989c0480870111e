"""float64 NumPy restatement of the reference's DefaultRNNLM (LRS/video/espnet/nets/pytorch_backend/lm/default.py: nn.Embedding -> stacked
nn.LSTMCell / nn.GRUCell -> nn.Linear -> log_softmax), written from its state dict.  `bf16_weights=True` rounds every matrix to bfloat16 first,
`bf16_inputs=True` also rounds what enters a contraction (the embedding row, the output of the layer below, h_prev): exactly what
svsr_rnn_cell_step does, so that only fp32 accumulation order and the fast sigmoid / tanh separate the kernel from this file."""
from __future__ import annotations

import numpy as np


def bf16_round(a: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even to bfloat16, returned as float64."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def cell_step(typ: str, w_ih, w_hh, b_ih, b_hh, x, h, c=None, bf16_inputs: bool = False):
    """One nn.LSTMCell / nn.GRUCell step in float64: x [n, E], h [n, U] (c [n, U]: LSTM) -> (h', c' | None).  torch's gate orders."""
    rnd = bf16_round if bf16_inputs else (lambda a: np.asarray(a, dtype=np.float64))
    U = w_hh.shape[1]
    gi = rnd(x) @ w_ih.T + b_ih
    gh = rnd(h) @ w_hh.T + b_hh
    if typ == "lstm":
        s = gi + gh
        i, f, g, o = _sig(s[:, :U]), _sig(s[:, U : 2 * U]), np.tanh(s[:, 2 * U : 3 * U]), _sig(s[:, 3 * U :])
        c2 = f * c + i * g
        return o * np.tanh(c2), c2
    r, z = _sig(gi[:, :U] + gh[:, :U]), _sig(gi[:, U : 2 * U] + gh[:, U : 2 * U])
    n = np.tanh(gi[:, 2 * U :] + r * gh[:, 2 * U :])
    return (1.0 - z) * n + z * h, None


def log_softmax(z):
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


class RNNLMRestatement:
    """The restatement behind the scorer interface.  State: (h [layers, n, U], c [layers, n, U] | None), or None: zeros."""

    def __init__(self, sd: dict, conf: dict, bf16_weights: bool = False, bf16_inputs: bool = False):
        self.typ, self.layers, self.U = conf["type"], int(conf["layer"]), int(conf["unit"])
        self.bf16_inputs = bf16_inputs
        w = {k: np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v.detach().double().numpy() for k, v in sd.items()}
        if bf16_weights:
            w = {k: bf16_round(v) if v.ndim == 2 else v for k, v in w.items()}
        self.w = w

    def step(self, tok: np.ndarray, state=None):
        """tok int [n] -> (log-probabilities [n, V], state)."""
        w, n = self.w, len(tok)
        if state is None:
            z = np.zeros((self.layers, n, self.U))
            state = (z, z.copy() if self.typ == "lstm" else None)
        hs, cs = state
        x = w["predictor.embed.weight"][np.asarray(tok)]
        h2, c2 = [], []
        for i in range(self.layers):
            p = f"predictor.rnn.{i}"
            h, c = cell_step(self.typ, w[f"{p}.weight_ih"], w[f"{p}.weight_hh"], w[f"{p}.bias_ih"], w[f"{p}.bias_hh"], x, hs[i],
                             None if cs is None else cs[i], self.bf16_inputs)
            h2.append(h)
            c2.append(c)
            x = h
        top = bf16_round(x) if self.bf16_inputs else x
        logits = top @ w["predictor.lo.weight"].T + w["predictor.lo.bias"]
        return log_softmax(logits), (np.stack(h2), np.stack(c2) if self.typ == "lstm" else None)

    @staticmethod
    def select(state, prev):
        prev = np.asarray(prev)
        return state[0][:, prev], None if state[1] is None else state[1][:, prev]

    def run(self, tok: np.ndarray, prev: np.ndarray):
        """The scripted steps of rnnlm_cases.step_inputs -> (logp [S, n, V], h [S, layers, n, U], c | None)."""
        state, lp, hs, cs = None, [], [], []
        for s in range(tok.shape[0]):
            if s > 0:
                state = self.select(state, prev[s])
            logp, state = self.step(tok[s], state)
            lp.append(logp)
            hs.append(state[0])
            cs.append(state[1])
        return np.stack(lp), np.stack(hs), np.stack(cs) if self.typ == "lstm" else None

    def forward(self, x: np.ndarray, t: np.ndarray):
        """default.py:106-136 -> (loss / batch, loss, count)."""
        B, L = x.shape
        state, loss, count = None, 0.0, 0
        for i in range(L):
            logp, state = self.step(x[:, i], state)
            nz = int((x[:, i] != 0).sum())
            loss += float(-logp[np.arange(B), t[:, i]].mean()) * nz
            count += nz
        return loss / B, loss, count

    # -- what a re-scoring along a path needs (torch in / out, like tests/lm_restatement.py) ---------------------------------------------
    def path_logp(self, yseq: list) -> float:
        """sum over the path of log p(y[i + 1] | y[: i + 1])."""
        state, tot = None, 0.0
        for a, b in zip(yseq[:-1], yseq[1:]):
            logp, state = self.step(np.array([a]), state)
            tot += float(logp[0, b])
        return tot
