"""CTC best-path (greedy) decoding, restated in numpy / torch from its description — the definition svsr_ctc_frame_best and svsr_ctc_collapse
(csrc/lrs_search.hip) are built to:

    per frame        best = argmax of the fp32 logits (torch.argmax: the lowest index on a tie, the first NaN if there is one);
                     best_logp = log_softmax(logits)[best], taken in fp64 and rounded to fp32
    per clip         a run is a maximal stretch of equal `best` over frames 0 .. tlen - 1 (itertools.groupby); every run whose value is not
                     the blank is one token: its id, (first, last) frame, and the mean of best_logp over the run — an fp32 sum in frame
                     order divided by the run length;  score = the fp32 sum of best_logp over the clip's frames in frame order
"""
from __future__ import annotations

import itertools

import numpy as np
import torch


def frame_best(logits):
    """logits fp32 [..., V] -> (best int64 [...], best_logp fp32 [...])."""
    x = torch.as_tensor(logits)
    assert x.dtype == torch.float32
    best = torch.argmax(x, dim=-1)
    lp = torch.log_softmax(x.double(), dim=-1).gather(-1, best.unsqueeze(-1)).squeeze(-1)
    return best.numpy().astype(np.int64), lp.numpy().astype(np.float32)


def margin(logits):
    """logits fp32 [..., V >= 2] -> fp32 [...]: how far the winner of every frame is ahead of the runner-up."""
    top = torch.as_tensor(logits).float().topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]).numpy()


def sum32(v) -> np.float32:
    """The fp32 sum of v in its order (np.cumsum adds one element after the other)."""
    v = np.asarray(v, dtype=np.float32)
    return np.cumsum(v, dtype=np.float32)[-1] if v.size else np.float32(0.0)


def collapse_one(best, best_logp, blank: int = 0):
    """best [T] winners, best_logp fp32 [T] -> (tokens int64 [L], spans int64 [L, 2], token_logp fp32 [L], score fp32)."""
    best = [int(v) for v in best]
    lp = np.asarray(best_logp, dtype=np.float32)
    assert len(best) == lp.shape[0]
    tokens, spans, tlp, t = [], [], [], 0
    for v, run in itertools.groupby(best):
        n = len(list(run))
        if v != blank:
            tokens.append(v)
            spans.append((t, t + n - 1))
            tlp.append(sum32(lp[t : t + n]) / np.float32(n))
        t += n
    return (np.array(tokens, dtype=np.int64), np.array(spans, dtype=np.int64).reshape(-1, 2), np.array(tlp, dtype=np.float32), sum32(lp))


def collapse_batch(best, best_logp, tlen, blank: int = 0, Lcap=None):
    """best int [C, Tmax], best_logp fp32 [C, Tmax], tlen [C] -> (tokens int64 [C, Lcap] -1 behind ntok, spans int32 [C, Lcap, 2] -1 behind
    ntok, token_logp fp32 [C, Lcap] 0 behind ntok, ntok int32 [C], score fp32 [C]): the outputs of svsr_ctc_collapse."""
    best, best_logp = np.asarray(best), np.asarray(best_logp, dtype=np.float32)
    C, Tmax = best.shape
    Lcap = Tmax if Lcap is None else Lcap
    tokens = np.full((C, Lcap), -1, np.int64)
    spans = np.full((C, Lcap, 2), -1, np.int32)
    tlp = np.zeros((C, Lcap), np.float32)
    ntok = np.zeros(C, np.int32)
    score = np.zeros(C, np.float32)
    for c in range(C):
        T = max(0, min(int(tlen[c]), Tmax))
        tk, sp, lp, sc = collapse_one(best[c, :T], best_logp[c, :T], blank)
        n = min(len(tk), Lcap)
        tokens[c, :n], spans[c, :n], tlp[c, :n], ntok[c], score[c] = tk[:n], sp[:n], lp[:n], len(tk), sc
    return tokens, spans, tlp, ntok, score


def greedy_one(logits, blank: int = 0):
    """logits fp32 [T, V] of one clip's live frames -> (tokens, spans, token_logp, frames int64 [T], score fp32)."""
    best, lp = frame_best(logits)
    tokens, spans, tlp, score = collapse_one(best, lp, blank)
    return tokens, spans, tlp, best, score
