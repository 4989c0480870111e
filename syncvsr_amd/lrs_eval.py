"""Scoring of the LRS model's transcripts: word error rate, token error rate and oracle error rate over an n-best list, from ONE kernel
(csrc/lrs_eval.hip k_edit_distance through `ops.edit_distance`: distance, substitutions, deletions and insertions of a batch of id pairs).

    ev = Evaluator(model, token_list, search)                # search: a lrs_infer.BatchBeamSearch, or None for CTC greedy decoding
    for clips, lengths, targets in loader:                    # clips [C, Tmax, 1, H, W], lengths [C], targets int64 [C, Lmax] padded with ignore_id
        ev.update(clips, lengths, targets)
    ev.compute()["wer"]                                       # total_edit_distance / total_length, the reference's names

What the last three lines of the reference's `test_step` and its epoch hooks do (LRS/video/lightning.py:17-20,124-128,224-234:
`compute_word_level_distance` = torchaudio.functional.edit_distance on `.lower().split()`, `total_edit_distance`, `total_length`, `wer`),
for a batch of clips per call.  The transcripts are made as the reference makes them (`ids_to_text`), split into words, characters or tokens
and interned into int64 rows on the host (`sequences`); every pair of an `update` — the 1-best of every clip at the chosen level, the same
1-best as token ids against the target ids, and every hypothesis of every clip's n-best — is scored by one launch, the per-clip minimum over
the n-best is taken on the device, and the counts stay on the device until `compute` copies them, once.

Without texts, for a validation loop: `token_errors` scores transcripts that are already on the device (what `ops.ctc_collapse` leaves
there) against padded targets and returns the summed counts as a device tensor; `greedy_token_errors` chains the encoder, ctc_lo,
svsr_ctc_frame_best, svsr_ctc_collapse and the kernel.  Neither copies anything to the host, so the results of many steps can be added up and
read once.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .model import _require_device

LEVELS = ("word", "char", "token")


def ids_to_text(ids, token_list: Sequence[str]) -> str:
    """Token ids -> the transcript as the reference writes it, for both sides of the comparison: the pieces joined, `<space>` and the
    SentencePiece word mark U+2581 turned into blanks, `<eos>` dropped, blanks at both ends stripped (`TextTransform.post_process` /
    `_ids_to_str`, datamodule/transforms.py:162-170, for the target; `parse_hypothesis` and lightning.py:121-122 for a hypothesis without
    its leading sos).  Negative ids (padding) are skipped."""
    ids = ids.tolist() if hasattr(ids, "tolist") else list(ids)
    text = "".join(token_list[int(i)] for i in ids if int(i) >= 0)
    return text.replace("<space>", " ").replace("▁", " ").replace("<eos>", "").strip()


def _split(text: str, level: str) -> list:
    if level == "word":
        return text.lower().split()                      # compute_word_level_distance, lightning.py:17-20
    if level == "char":
        return list(text)
    if level == "token":
        return text.split()
    raise ValueError(f"level must be one of {LEVELS}, got {level!r}")


def _pad(rows: list) -> tuple[torch.Tensor, torch.Tensor]:
    """Lists of ints -> (int64 [N, max length] padded with -1, int32 [N] lengths), on the host."""
    out = torch.full((len(rows), max([len(r) for r in rows] + [0])), -1, dtype=torch.int64)
    for n, r in enumerate(rows):
        if r:
            out[n, : len(r)] = torch.tensor(r, dtype=torch.int64)
    return out, torch.tensor([len(r) for r in rows], dtype=torch.int32)


def sequences(hyp_texts: Sequence[str], ref_texts: Sequence[str], level: str = "word"):
    """Pairs of transcripts -> (hyp int64 [N, Lh], hyp_len int32 [N], ref int64 [N, Lr], ref_len int32 [N]) on the host, for
    `ops.edit_distance`: each transcript split at `level` — "word": `.lower().split()`, "char": its characters, "token": `.split()` — and
    every distinct item given one id, in order of first appearance over the call.  Rows are padded with -1."""
    if level not in LEVELS:
        raise ValueError(f"level must be one of {LEVELS}, got {level!r}")
    if len(hyp_texts) != len(ref_texts):
        raise ValueError(f"{len(hyp_texts)} hypotheses for {len(ref_texts)} references")
    table: dict = {}
    hyp = [[table.setdefault(w, len(table)) for w in _split(t, level)] for t in hyp_texts]
    ref = [[table.setdefault(w, len(table)) for w in _split(t, level)] for t in ref_texts]
    return _pad(hyp) + _pad(ref)


def _check_width(*widths: int) -> None:
    if max(widths) > ops.EDIT_MAX_LEN:
        raise ValueError(f"sequences of more than {ops.EDIT_MAX_LEN} ids are not supported, got rows of {' and '.join(str(w) for w in widths)}")


def token_errors(hyp_ids: torch.Tensor, hyp_len: torch.Tensor, targets: torch.Tensor, ignore_id: int = -1) -> torch.Tensor:
    """hyp_ids int64 [N, Lh] and hyp_len int32 [N] on the device (the tokens and ntok of `ops.ctc_collapse`), targets int64 [N, Lmax] padded
    with ignore_id at the tail -> int64 [5] on the device: the summed (errors, substitutions, deletions, insertions, target length).  The
    target lengths are counted on the device and nothing is copied to the host."""
    if hyp_ids.dim() != 2 or targets.dim() != 2 or targets.shape[0] != hyp_ids.shape[0] or hyp_ids.dtype != torch.int64:
        raise ValueError(f"hyp_ids int64 [N, Lh] and targets [N, Lmax] are needed, got {hyp_ids.dtype} {tuple(hyp_ids.shape)} and {tuple(targets.shape)}")
    _check_width(hyp_ids.shape[1], targets.shape[1])
    _require_device(hyp_ids)
    tg = targets.to(device=hyp_ids.device, dtype=torch.int64)
    ref_len = (tg != ignore_id).sum(dim=1, dtype=torch.int32)
    out = ops.edit_distance(hyp_ids, hyp_len.to(torch.int32).contiguous(), tg.contiguous(), ref_len)
    return torch.cat([out.sum(dim=0, dtype=torch.int64), ref_len.sum(dtype=torch.int64).view(1)])


def greedy_token_errors(model, clips: torch.Tensor, lengths, targets: torch.Tensor, blank_id: int = 0) -> torch.Tensor:
    """clips [C, Tmax, 1, H, W] padded along T, lengths [C] (host), targets int64 [C, Lmax] padded with the model's ignore_id -> int64 [5] on
    the device: `token_errors` of the CTC head's best path (encoder, ctc_lo, svsr_ctc_frame_best, svsr_ctc_collapse, svsr_edit_distance).
    Nothing is copied to the host: a validation loop adds the results of its steps up and reads the sum once."""
    from .lrs_align import check_lengths
    from .lrs_infer import CTCPrefixScorer

    if clips.dim() != 5 or clips.size(2) != 1:
        raise ValueError("clips must be [C, Tmax, 1, H, W]")
    C, Tmax = clips.shape[:2]
    lens = check_lengths(lengths, C, Tmax, model.odim, blank_id)                                           # before the encoder
    if targets.dim() != 2 or targets.shape[0] != C:
        raise ValueError(f"targets must be integer ids [{C}, Lmax], got {tuple(targets.shape)}")
    _check_width(Tmax, targets.shape[1])                                                                   # a clip has no more tokens than frames
    _require_device(clips)
    tlen = torch.tensor(lens, dtype=torch.int32).to(clips.device)
    masks = (torch.arange(Tmax, device=clips.device).unsqueeze(0) < tlen.unsqueeze(1)).unsqueeze(1)        # [C, 1, Tmax], make_non_pad_mask
    enc, _ = model.encoder(clips, masks)
    logits = CTCPrefixScorer(model, model.eos).ctc_logits(enc.detach().reshape(C * Tmax, model.adim))
    best, best_logp = ops.ctc_frame_best(logits, tlen, Tmax=Tmax, V=model.odim)
    tokens, _, _, ntok, _ = ops.ctc_collapse(best, best_logp, tlen, blank_id)
    return token_errors(tokens, ntok, targets, model.ignore_id)


class Evaluator:
    """Accumulates the reference's `total_edit_distance` and `total_length` over batches of clips, on the device.

    `update(clips, lengths, targets)` decodes the clips — `lrs_infer.decode_clips` with the given `BatchBeamSearch`, `lrs_align.greedy_clips`
    without one — and scores the 1-best of every clip against its target as `test_step` does, at `level` ("word", "char" or "token" of the
    texts) and, as token ids against the target ids, for the token error rate.  When the search returns more than one hypothesis for some
    clip, every hypothesis is scored in the same launch and the fewest errors per clip go into the oracle error rate.  `update_texts(hyps,
    refs)` adds transcripts that were decoded elsewhere.  `compute()` copies the counts once.  A clip that decodes to nothing scores its
    target's length in deletions."""

    # err, sub, del, ins, len at `level`; token err, token len; oracle err and the length it goes with
    _SLOTS = 9

    def __init__(self, model, token_list: Sequence[str], search=None, level: str = "word", blank_id: int = 0):
        if level not in LEVELS:
            raise ValueError(f"level must be one of {LEVELS}, got {level!r}")
        self.model, self.token_list, self.search, self.level, self.blank_id = model, list(token_list), search, level, int(blank_id)
        self._acc: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self._acc = None

    def _device(self) -> torch.device:
        p = next(self.model.parameters(), None) if self.model is not None else None
        if p is None:
            raise RuntimeError("syncvsr_amd runs on an MI355X HIP device only; there is no CPU fallback (the evaluator needs a model on the device)")
        _require_device(p)
        return p.device

    def _score(self, dev, hyps: list, refs: list, token_pairs: Optional[tuple], nbest_texts: Optional[list]) -> None:
        """One launch for every pair of the call; the sums and the per-clip minimum on the device."""
        C = len(refs)
        pairs_h, pairs_r = list(hyps), list(refs)
        rows_of = []                                                        # per clip: the rows of its n-best in the launch
        if nbest_texts is not None:
            for c, texts in enumerate(nbest_texts):
                texts = texts if len(texts) else [""]
                rows_of.append(list(range(len(pairs_h), len(pairs_h) + len(texts))))
                pairs_h += texts
                pairs_r += [refs[c]] * len(texts)
        hyp, hyp_len, ref, ref_len = sequences(pairs_h, pairs_r, self.level)
        if token_pairs is not None:                                         # token ids are ids already: rows C .. 2C - 1 of the launch
            th, thl, tr, trl = _pad(token_pairs[0]) + _pad(token_pairs[1])
            wh, wr = max(hyp.shape[1], th.shape[1]), max(ref.shape[1], tr.shape[1])
            grow = lambda t, w: torch.nn.functional.pad(t, (0, w - t.shape[1]), value=-1)      # noqa: E731
            hyp, ref = torch.cat([grow(hyp[:C], wh), grow(th, wh), grow(hyp[C:], wh)]), torch.cat([grow(ref[:C], wr), grow(tr, wr), grow(ref[C:], wr)])
            hyp_len, ref_len = torch.cat([hyp_len[:C], thl, hyp_len[C:]]), torch.cat([ref_len[:C], trl, ref_len[C:]])
            rows_of = [[r + C for r in rows] for rows in rows_of]
        _check_width(hyp.shape[1], ref.shape[1])
        n = hyp.shape[0]
        out = ops.edit_distance(hyp.to(dev), hyp_len.to(dev), ref.to(dev), ref_len.to(dev)).to(torch.int64)
        rl = ref_len.to(dev).to(torch.int64)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        parts = [out[:C].sum(dim=0), rl[:C].sum().view(1)]
        parts += [out[C : 2 * C, 0].sum().view(1), rl[C : 2 * C].sum().view(1)] if token_pairs is not None else [zero, zero]
        if rows_of:
            width = max(len(r) for r in rows_of)
            idx = torch.tensor([r + [n] * (width - len(r)) for r in rows_of], dtype=torch.int64).to(dev)   # row n: a cost no pair reaches
            cost = torch.cat([out[:, 0], torch.full((1,), 1 << 40, dtype=torch.int64, device=dev)])
            parts += [cost[idx].min(dim=1).values.sum().view(1), rl[:C].sum().view(1)]
        else:
            parts += [zero, zero]
        acc = torch.cat(parts)
        self._acc = acc if self._acc is None else self._acc + acc

    def update_texts(self, hyps: Sequence[str], refs: Sequence[str]) -> None:
        """Transcripts from elsewhere, one hypothesis per reference: scored at `level` (no token ids, no n-best)."""
        if len(hyps) != len(refs):
            raise ValueError(f"{len(hyps)} hypotheses for {len(refs)} references")
        dev = self._device()
        if len(refs):
            self._score(dev, list(hyps), list(refs), None, None)

    def update(self, clips: torch.Tensor, lengths, targets: torch.Tensor) -> None:
        """clips [C, Tmax, 1, H, W] padded along T, lengths [C], targets int64 [C, Lmax] padded with the model's ignore_id."""
        if clips.dim() != 5 or clips.size(2) != 1:
            raise ValueError("clips must be [C, Tmax, 1, H, W]")
        C = clips.shape[0]
        tg = torch.as_tensor(targets).detach().cpu()
        if tg.dim() != 2 or tg.shape[0] != C or tg.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"targets must be integer ids [{C}, Lmax], got {tg.dtype} {tuple(tg.shape)}")
        _require_device(clips)
        ignore, eos = self.model.ignore_id, self.model.eos
        ref_ids = [[v for v in row if v != ignore] for row in tg.tolist()]
        refs = [ids_to_text(r, self.token_list) for r in ref_ids]
        nbest_texts = None
        if self.search is not None:
            from .lrs_infer import decode_clips

            nbests = decode_clips(self.model, self.search, clips, lengths)
            flat = [h.yseq[1:] for nb in nbests for h in nb]                                               # without the leading sos
            host = torch.cat(flat).cpu().tolist() if flat else []                                          # one copy for every hypothesis
            ids, o = [], 0
            for nb in nbests:
                ids.append([])
                for h in nb:
                    k = len(h.yseq) - 1
                    ids[-1].append(host[o : o + k])
                    o += k
            hyp_ids = [[v for v in nb[0] if v != eos] if nb else [] for nb in ids]
            hyps = [ids_to_text(nb[0], self.token_list) if nb else "" for nb in ids]
            if any(len(nb) > 1 for nb in ids):
                nbest_texts = [[ids_to_text(y, self.token_list) for y in nb] for nb in ids]
        else:
            from .lrs_align import greedy_clips

            paths = greedy_clips(self.model, clips, lengths, self.blank_id)
            hyp_ids = [p.tokens.tolist() for p in paths]
            hyps = [ids_to_text(y, self.token_list) for y in hyp_ids]
        self._score(clips.device, hyps, refs, (hyp_ids, ref_ids), nbest_texts)

    def compute(self) -> dict:
        """One copy of the counts -> wer (total_edit_distance / total_length), total_edit_distance, total_length, sub, del, ins,
        token_error_rate and oracle_wer; a rate whose length is 0 (nothing scored for it: no n-best, texts only) is None."""
        v = [0] * self._SLOTS if self._acc is None else self._acc.cpu().tolist()
        rate = lambda e, n: e / n if n else None      # noqa: E731
        return {"wer": rate(v[0], v[4]), "total_edit_distance": v[0], "total_length": v[4], "sub": v[1], "del": v[2], "ins": v[3],
                "token_error_rate": rate(v[5], v[6]), "oracle_wer": rate(v[7], v[8])}
