"""CTC forced alignment and CTC greedy decoding of the LRS model: which frames the tokens of a transcript occupy — a known transcript
(`align_clips`), or the best path's own (`greedy_clips`).

    alis = align_clips(model, clips, lengths, targets)      # clips [C, Tmax, 1, H, W], lengths [C], targets int64 [C, Lmax] padded with ignore_id
    a = alis[0]                                             # Alignment(frames [T_c], tokens [L_c], spans [L_c, 2], token_logp [L_c], score)

The batched twin of `lrs_infer.decode_clips`: one encoder pass, one ctc_lo + log_softmax over the batch, ONE svsr_ctc_align launch
(csrc/lrs_search.hip k_ctc_align: the Viterbi recursion of the reference's `CTC.forced_align_batch`, ctc.py:246-328, one workgroup per clip)
and one device-to-host copy.  `align_features` is the same from padded encoder outputs, as `forward_clips` is to `decode_clips`.  The
reference-named methods `E2E.ctc.forced_align_batch` / `forced_align` (lrs_model._CtcFacade) run the same kernel.

Everything that has no alignment is refused on the host, from the lengths and the targets alone, before the encoder or any launch
(`check_targets`): the reference returns a path that does not spell the transcript there.

    paths = greedy_clips(model, clips, lengths)              # no transcript needed
    p = paths[0]                                            # GreedyPath(tokens [L_c], spans [L_c, 2], token_logp [L_c], frames [T_c], score)

Best-path decoding (`CTC.argmax`, ctc.py:172, and the `groupby` every recipe applies to it): one encoder pass, one ctc_lo over the batch to
fp32 logits, svsr_ctc_frame_best (the winner of every frame and its log-probability, straight from the logits: the [C, Tmax, odim]
log-softmax is never stored), svsr_ctc_collapse (runs merged, blanks dropped, one workgroup per clip) and one device-to-host copy.
`greedy_features` starts from padded encoder outputs; `E2E.ctc.greedy_batch` returns the transcripts alone.  A clip that decodes to
nothing is an empty `GreedyPath`, not an error.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .model import _require_device


class Alignment(NamedTuple):
    frames: np.ndarray          # int64 [T]: the token of every frame (blank_id between and inside tokens)
    tokens: np.ndarray          # int64 [L]: the transcript
    spans: np.ndarray           # int64 [L, 2]: first and last frame of every token
    token_logp: np.ndarray      # fp32 [L]: mean log-probability of the token over its frames (an fp32 sum in frame order)
    score: float                # log-probability of the path


class GreedyPath(NamedTuple):
    tokens: np.ndarray          # int64 [L]: the collapsed transcript (L = 0: every frame's winner was the blank)
    spans: np.ndarray           # int64 [L, 2]: first and last frame of every token
    token_logp: np.ndarray      # fp32 [L]: mean log-probability of the token over its frames (an fp32 sum in frame order)
    frames: np.ndarray          # int64 [T]: the most probable unit of every frame
    score: float                # log-probability of the best path: the fp32 sum of the winners' log-probabilities in frame order


def frames_needed(y) -> int:
    """Fewest frames the transcript can be aligned to: one per token and one blank between two equal neighbours."""
    return len(y) + sum(1 for a, b in zip(y, y[1:]) if a == b)


def check_targets(targets, lengths, C: int, Tmax: int, odim: int, blank: int, ignore_id: int) -> tuple[torch.Tensor, list]:
    """targets int64 [C, Lmax] padded with ignore_id, lengths [C] -> (labels int64 [C, Lmax] padded with -1 (host), lengths as a list).
    Raises ValueError for whatever has no alignment; nothing has been launched by then."""
    tg = torch.as_tensor(targets).detach().cpu()
    if tg.dim() != 2 or tg.size(0) != C or tg.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"targets must be integer ids [{C}, Lmax], got {tg.dtype} {tuple(tg.shape)}")
    lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(lens) != C:
        raise ValueError(f"{len(lens)} lengths for {C} clips")
    if any(t < 1 or t > Tmax for t in lens):
        raise ValueError(f"lengths must lie in [1, {Tmax}] (the padded frame count), got {lens}")
    if not 0 <= int(blank) < odim:
        raise ValueError(f"blank_id {blank} is outside [0, {odim})")
    if tg.size(1) > ops.CTC_ALIGN_MAX_LABELS:
        raise ValueError(f"transcripts of more than {ops.CTC_ALIGN_MAX_LABELS} tokens are not supported, got Lmax = {tg.size(1)}")
    rows = tg.to(torch.int64).tolist()
    for c, row in enumerate(rows):
        n = len(row)
        while n > 0 and row[n - 1] == ignore_id:
            n -= 1
        y = row[:n]
        if n == 0:
            raise ValueError(f"clip {c}: empty transcript")
        if ignore_id in y:
            raise ValueError(f"clip {c}: ignore_id ({ignore_id}) in front of a live token at position {y.index(ignore_id)}")
        for v in y:
            if v < 0 or v >= odim or v == blank:
                raise ValueError(f"clip {c}: id {v} is outside [0, {odim}) or the blank ({blank})")
        need = frames_needed(y)
        if lens[c] < need:
            raise ValueError(f"clip {c}: infeasible, tlen = {lens[c]} frames but its {n} tokens need {need} (one per token, one blank between equal neighbours)")
    labels = tg.to(torch.int64).clone()
    labels[labels == ignore_id] = -1
    return labels.contiguous(), lens


def align_logp(logp: torch.Tensor, lens: list, labels: torch.Tensor, blank: int):
    """logp fp32 [C, Tmax, odim] on the device, checked lengths and labels (host) -> device (frames int32 [C, Tmax], spans int32 [C, Lmax, 2],
    score fp32 [C]): one launch."""
    dev = logp.device
    tlen = torch.tensor(lens, dtype=torch.int32).to(dev)
    return ops.ctc_align(logp.contiguous(), tlen, labels.to(dev), blank)


def _results(logp: torch.Tensor, lens: list, labels: torch.Tensor, blank: int) -> list:
    C, Tmax, _ = logp.shape
    Lmax = labels.size(1)
    frames, spans, score = align_logp(logp, lens, labels, blank)
    at = logp.gather(2, frames.clamp(min=0).long().unsqueeze(2)).squeeze(2)                # log-probability of each frame's own token
    host = torch.cat([frames.reshape(-1), spans.reshape(-1), score.view(torch.int32), at.contiguous().view(torch.int32).reshape(-1)]).cpu().numpy()
    o = np.cumsum([0, C * Tmax, C * Lmax * 2, C, C * Tmax])
    fr, sp = host[o[0] : o[1]].reshape(C, Tmax), host[o[1] : o[2]].reshape(C, Lmax, 2)
    sc, lp = host[o[2] : o[3]].view(np.float32), host[o[3] : o[4]].view(np.float32).reshape(C, Tmax)
    out = []
    for c in range(C):
        y = labels[c][labels[c] >= 0].numpy()
        L = len(y)
        if not sc[c] > -np.inf:
            raise ValueError(f"clip {c}: no path through its posteriors")
        s = sp[c, :L].astype(np.int64)
        tl = np.array([np.cumsum(lp[c, a : b + 1], dtype=np.float32)[-1] / np.float32(b + 1 - a) for a, b in s], dtype=np.float32)
        out.append(Alignment(frames=fr[c, : lens[c]].astype(np.int64), tokens=y.astype(np.int64), spans=s, token_logp=tl, score=float(sc[c])))
    return out


def align_features(model, enc_feats: torch.Tensor, lengths, targets, blank_id: int = 0) -> list:
    """enc_feats [C, Tmax, adim] padded encoder outputs, lengths [C], targets int64 [C, Lmax] padded with the model's ignore_id -> one
    `Alignment` per clip."""
    from .lrs_infer import CTCPrefixScorer

    if enc_feats.dim() != 3 or enc_feats.size(2) != model.adim:
        raise ValueError(f"enc_feats must be [clips, frames, {model.adim}], got {tuple(enc_feats.shape)}")
    C, Tmax = enc_feats.shape[:2]
    labels, lens = check_targets(targets, lengths, C, Tmax, model.odim, blank_id, model.ignore_id)
    _require_device(enc_feats)
    logp = CTCPrefixScorer(model, model.eos).ctc_log_softmax(enc_feats.detach().reshape(C * Tmax, model.adim)).view(C, Tmax, -1)
    return _results(logp, lens, labels, blank_id)


def align_clips(model, clips: torch.Tensor, lengths, targets, blank_id: int = 0) -> list:
    """clips [C, Tmax, 1, H, W] padded along T, lengths [C], targets int64 [C, Lmax] padded with the model's ignore_id -> one `Alignment`
    per clip, over `model.encoder(clips, masks)` as `decode_clips` runs it (the model is in eval mode)."""
    if clips.dim() != 5 or clips.size(2) != 1:
        raise ValueError("clips must be [C, Tmax, 1, H, W]")
    C, Tmax = clips.shape[:2]
    labels, lens = check_targets(targets, lengths, C, Tmax, model.odim, blank_id, model.ignore_id)        # before the encoder
    lt = torch.tensor(lens, dtype=torch.int64).to(clips.device)
    masks = (torch.arange(Tmax, device=clips.device).unsqueeze(0) < lt.unsqueeze(1)).unsqueeze(1)          # [C, 1, Tmax], make_non_pad_mask
    enc, _ = model.encoder(clips, masks)
    return align_features(model, enc, lens, targets, blank_id)


def check_lengths(lengths, C: int, Tmax: int, odim: int, blank: int) -> list:
    """lengths [C] -> a list, after the checks `check_targets` makes of lengths and blank (the same words).  Nothing has been launched."""
    lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(lens) != C:
        raise ValueError(f"{len(lens)} lengths for {C} clips")
    if any(t < 1 or t > Tmax for t in lens):
        raise ValueError(f"lengths must lie in [1, {Tmax}] (the padded frame count), got {lens}")
    if not 0 <= int(blank) < odim:
        raise ValueError(f"blank_id {blank} is outside [0, {odim})")
    if Tmax > ops.CTC_GREEDY_MAX_FRAMES:
        raise ValueError(f"clips of more than {ops.CTC_GREEDY_MAX_FRAMES} frames are not supported, got Tmax = {Tmax}")
    return lens


def greedy_logits(logits: torch.Tensor, lens: list, V: int, blank: int) -> list:
    """logits fp32 [C * Tmax, ldp >= V] on the device, checked lengths -> one `GreedyPath` per clip: two launches, one device-to-host copy."""
    C = len(lens)
    Tmax = logits.shape[0] // C
    tlen = torch.tensor(lens, dtype=torch.int32).to(logits.device)
    best, best_logp = ops.ctc_frame_best(logits, tlen, Tmax=Tmax, V=V)
    tokens, spans, token_logp, ntok, score = ops.ctc_collapse(best, best_logp, tlen, blank)
    host = torch.cat([tokens.view(torch.int32).reshape(-1), spans.reshape(-1), token_logp.view(torch.int32).reshape(-1), best.reshape(-1),
                      ntok, score.view(torch.int32)]).cpu().numpy()
    n = C * Tmax
    o = np.cumsum([0, 2 * n, 2 * n, n, n, C, C])
    tk, sp = host[o[0] : o[1]].view(np.int64).reshape(C, Tmax), host[o[1] : o[2]].reshape(C, Tmax, 2)
    tl, fr = host[o[2] : o[3]].view(np.float32).reshape(C, Tmax), host[o[3] : o[4]].reshape(C, Tmax)
    nt, sc = host[o[4] : o[5]], host[o[5] : o[6]].view(np.float32)
    return [GreedyPath(tokens=tk[c, : nt[c]].copy(), spans=sp[c, : nt[c]].astype(np.int64), token_logp=tl[c, : nt[c]].copy(),
                       frames=fr[c, : lens[c]].astype(np.int64), score=float(sc[c])) for c in range(C)]


def greedy_features(model, enc_feats: torch.Tensor, lengths, blank_id: int = 0) -> list:
    """enc_feats [C, Tmax, adim] padded encoder outputs, lengths [C] -> one `GreedyPath` per clip: the CTC head's best path."""
    from .lrs_infer import CTCPrefixScorer

    if enc_feats.dim() != 3 or enc_feats.size(2) != model.adim:
        raise ValueError(f"enc_feats must be [clips, frames, {model.adim}], got {tuple(enc_feats.shape)}")
    C, Tmax = enc_feats.shape[:2]
    lens = check_lengths(lengths, C, Tmax, model.odim, blank_id)
    _require_device(enc_feats)
    logits = CTCPrefixScorer(model, model.eos).ctc_logits(enc_feats.detach().reshape(C * Tmax, model.adim))
    return greedy_logits(logits, lens, model.odim, blank_id)


def greedy_clips(model, clips: torch.Tensor, lengths, blank_id: int = 0) -> list:
    """clips [C, Tmax, 1, H, W] padded along T, lengths [C] -> one `GreedyPath` per clip, over `model.encoder(clips, masks)` as
    `align_clips` runs it (the model is in eval mode)."""
    if clips.dim() != 5 or clips.size(2) != 1:
        raise ValueError("clips must be [C, Tmax, 1, H, W]")
    C, Tmax = clips.shape[:2]
    lens = check_lengths(lengths, C, Tmax, model.odim, blank_id)                                           # before the encoder
    _require_device(clips)
    lt = torch.tensor(lens, dtype=torch.int64).to(clips.device)
    masks = (torch.arange(Tmax, device=clips.device).unsqueeze(0) < lt.unsqueeze(1)).unsqueeze(1)          # [C, 1, Tmax], make_non_pad_mask
    enc, _ = model.encoder(clips, masks)
    return greedy_features(model, enc, lens, blank_id)
