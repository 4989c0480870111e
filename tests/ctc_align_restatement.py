"""CTC forced alignment (Viterbi over the CTC lattice), restated in numpy from its description — the definition svsr_ctc_align
(csrc/lrs_search.hip) is built to, result for result, and what the reference's `CTC.forced_align_batch` (ctc.py:246-328) computes for every
clip that has a path (tests/golden/make_golden_ctc_align.py asserts that where the reference is).

    states of a clip     ext = [blank, y1, blank, y2, ..., yL, blank], S = 2L + 1
    frame 0              d[0] = lp[0, blank], d[1] = lp[0, y1], everything else -inf
    frame t >= 1         d'[s] = max(d[s], d[s-1], d[s-2]) + lp[t, ext[s]]        candidates in THAT order, the first maximum wins (strict >);
                         s-2 only for odd s >= 3 with ext[s] != ext[s-2]; one fp32 add per cell, everything in fp32
    end                  the larger of d[S-2] and d[S-1] at frame tlen-1, S-2 on a tie; the back-pointers give one state per frame

A clip without a path — tlen < L + (adjacent equal labels), tlen <= 0, L = 0, a label outside [0, V) or equal to blank, or posteriors whose
best path is -inf — has score -inf and frames = spans = -1 (the reference returns a junk path there)."""
from __future__ import annotations

import numpy as np

NEG = np.float32(-np.inf)


def frames_needed(y) -> int:
    """Fewest frames a transcript can be aligned to: one per label and one blank between two equal neighbours."""
    y = [int(v) for v in y]
    return len(y) + sum(1 for a, b in zip(y, y[1:]) if a == b)


def collapse(frames, blank: int = 0) -> list:
    """The transcript a frame sequence spells: merge runs, drop blanks."""
    out, last = [], None
    for v in (int(f) for f in frames):
        if v != last and v != blank:
            out.append(v)
        last = v
    return out


def align_one(lp: np.ndarray, y, blank: int = 0):
    """lp fp32 [T, V] log-probabilities, y the L labels -> (frames int64 [T], spans int64 [L, 2], score fp32)."""
    lp = np.asarray(lp)
    assert lp.dtype == np.float32 and lp.ndim == 2
    T, V = lp.shape
    y = [int(v) for v in y]
    L = len(y)
    bad = (np.full(T, -1, np.int64), np.full((L, 2), -1, np.int64), NEG)
    if T < 1 or L < 1 or any(v < 0 or v >= V or v == blank for v in y):
        return bad
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = y
    skip = np.zeros(S, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    d = np.full(S, NEG, np.float32)
    d[0], d[1] = lp[0, blank], lp[0, y[0]]
    bp = np.zeros((T, S), np.uint8)
    for t in range(1, T):
        c1 = np.concatenate(([NEG], d[:-1])).astype(np.float32)
        c2 = np.concatenate(([NEG, NEG], d[:-2])).astype(np.float32)
        best, k = d.copy(), np.zeros(S, np.uint8)
        m = c1 > best
        best[m], k[m] = c1[m], 1
        m = skip & (c2 > best)
        best[m], k[m] = c2[m], 2
        d = (best + lp[t, ext]).astype(np.float32)           # one fp32 add per cell
        bp[t] = k
    s = S - 1 if d[S - 1] > d[S - 2] else S - 2
    score = d[s]
    if not score > NEG:                                      # no path (NaN included)
        return bad
    states = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    spans = np.full((L, 2), -1, np.int64)
    for l in range(L):
        at = np.nonzero(states == 2 * l + 1)[0]
        spans[l] = (at[0], at[-1])
    return ext[states], spans, np.float32(score)


def align_batch(logp: np.ndarray, tlen, labels: np.ndarray, blank: int = 0):
    """logp fp32 [B, Tmax, >= V columns are all read as the vocabulary], tlen [B], labels int64 [B, Lmax] padded with -1 at the tail ->
    (frames int32 [B, Tmax], -1 beyond tlen; spans int32 [B, Lmax, 2], -1 beyond L_b; score fp32 [B]): the outputs of svsr_ctc_align."""
    logp, labels = np.asarray(logp), np.asarray(labels)
    B, Tmax, _ = logp.shape
    Lmax = labels.shape[1]
    frames = np.full((B, Tmax), -1, np.int32)
    spans = np.full((B, Lmax, 2), -1, np.int32)
    score = np.full(B, NEG, np.float32)
    for b in range(B):
        L = Lmax
        while L > 0 and labels[b, L - 1] == -1:              # the padding is the run of -1 at the tail; anything else in front of it is a label
            L -= 1
        T = min(int(tlen[b]), Tmax)
        if T < 1:
            continue
        f, sp, sc = align_one(logp[b, :T], labels[b, :L], blank)
        frames[b, :T], spans[b, :L], score[b] = f, sp, sc
    return frames, spans, score
