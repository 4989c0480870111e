"""Host restatement of svsr_edit_distance (include/syncvsr_hip.h): the full table of (cost, S, D, I) cells in plain Python integers, written
from the definition and nothing else.  Row i = the first i hypothesis ids, column j = the first j reference ids.

    cell(0,0) = (0, 0, 0, 0);  cell(i,0) = i insertions;  cell(0,j) = j deletions
    for i, j >= 1 the candidates, in priority order:
        1. cell(i-1,j-1), plus one substitution unless hyp[i-1] == ref[j-1]
        2. cell(i,j-1) plus one deletion
        3. cell(i-1,j) plus one insertion
    the smallest cost wins, a tie goes to the earlier candidate, the counts travel with the chosen predecessor.

Also the host statements of what syncvsr_amd/lrs_eval.py adds up: per-pair rows, sums, and the oracle (per-clip minimum) over an n-best.
"""
from __future__ import annotations

import numpy as np


def edit_one(hyp, ref) -> tuple:
    """(cost, S, D, I) of one pair of id sequences (anything comparable with ==)."""
    hyp, ref = list(hyp), list(ref)
    H, R = len(hyp), len(ref)
    table = [[None] * (R + 1) for _ in range(H + 1)]
    for i in range(H + 1):
        table[i][0] = (i, 0, 0, i)
    for j in range(R + 1):
        table[0][j] = (j, 0, j, 0)
    for i in range(1, H + 1):
        for j in range(1, R + 1):
            c, s, d, n = table[i - 1][j - 1]
            best = (c, s, d, n) if hyp[i - 1] == ref[j - 1] else (c + 1, s + 1, d, n)
            c, s, d, n = table[i][j - 1]
            if c + 1 < best[0]:
                best = (c + 1, s, d + 1, n)
            c, s, d, n = table[i - 1][j]
            if c + 1 < best[0]:
                best = (c + 1, s, d, n + 1)
            table[i][j] = best
    return table[H][R]


def edit_batch(hyp, hyp_len, ref, ref_len) -> np.ndarray:
    """Padded rows and lengths -> int32 [N, 4], as ops.edit_distance returns it.  Only the first hyp_len / ref_len ids of a row are looked at."""
    out = np.zeros((len(hyp_len), 4), np.int32)
    for p in range(len(hyp_len)):
        out[p] = edit_one(np.asarray(hyp[p])[: int(hyp_len[p])].tolist(), np.asarray(ref[p])[: int(ref_len[p])].tolist())
    return out


def levenshtein(a, b) -> int:
    """The textbook two-row distance, independent of the table above: no counts, no priorities."""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
        prev = cur
    return prev[len(b)]


def split(text: str, level: str) -> list:
    """A transcript as the sequence that is scored: words as `compute_word_level_distance` makes them, characters, or space-separated tokens."""
    if level == "word":
        return text.lower().split()
    if level == "char":
        return list(text)
    if level == "token":
        return text.split()
    raise ValueError(level)


def text_errors(hyps, refs, level: str = "word") -> np.ndarray:
    """int64 [5] = summed (errors, S, D, I, reference length) over the pairs of transcripts."""
    tot = np.zeros(5, np.int64)
    for h, r in zip(hyps, refs):
        hs, rs = split(h, level), split(r, level)
        tot[:4] += np.array(edit_one(hs, rs), np.int64)
        tot[4] += len(rs)
    return tot


def oracle_errors(nbests, refs, level: str = "word") -> int:
    """Summed over the clips: the fewest errors any hypothesis of the clip's n-best makes (an empty n-best: the empty transcript)."""
    tot = 0
    for hyps, r in zip(nbests, refs):
        rs = split(r, level)
        tot += min(edit_one(split(h, level), rs)[0] for h in (hyps if len(hyps) else [""]))
    return tot
