"""Inference surface of the LRS (sentence-level) model: the scorers and the batch beam search the reference's test loop drives.

    enc_feat, _ = model.encoder(sample.unsqueeze(0), None)          # LRS/video/lightning.py:114-118
    nbest = get_beam_search_decoder(model, token_list)(enc_feat.squeeze(0))        # lightning.py:119,237-279

Mirrors, by name and argument meaning, `E2E.scorers()` (e2e_asr_transformer.py:182-184), `Decoder.forward_one_step / score /
batch_score` (transformer/decoder.py:153-220), `CTCPrefixScorer` (scorers/ctc.py), `LengthBonus` (scorers/length_bonus.py),
`BatchBeamSearch` (batch_beam_search.py, beam_search.py:285-420), `end_detect` (e2e_asr_common.py:19-49) and
`get_beam_search_decoder` (lightning.py:237-279).  Design differences, all result-preserving:

  * the search state is batched tensors from start to end (token matrix, score vector, CTC forward variables [n, T, 2]) — the
    reference converts to and from per-hypothesis Python objects every step (batch_beam_search.py:230-275);
  * the CTC prefix recursion over the T frames runs in ONE HIP kernel per step, one thread per (hypothesis, candidate) pair
    (csrc/lrs_search.hip k_ctc_prefix_score_clips) instead of ~10 small torch kernels per frame (ctc_prefix_score.py:139-146);
  * the decoder scorer recomputes the prefix with the training kernels (one [n * L]-row batch keeps the MFMA tiles full) instead
    of caching per-layer outputs: the decoder's self-attention is causal, so the last row is identical either way.

The search itself is device-agnostic host logic over torch tensors; the two neural scorers need the HIP library.

There is ONE search.  `BatchBeamSearch.forward_clips(xs [C, Tmax, D], lengths)` / `decode_clips` decode C clips in lock step (the reference
decodes its test list clip after clip), and `forward(x [T, D])` is that search with one clip: rows stay grouped by clip, the scorers are
clip-aware (`batch_init_state_clips`, `batch_score_clips` / `batch_score_partial_clips`; a scorer that speaks the reference's single-clip
protocol only, and for CPU tensors one that speaks both, is wrapped in `PerClipScorers`), the selection of a position is one HIP entry
point for all clips (svsr_beam_select; anything but fp32 CUDA tensors: its torch statement `beam_select_reference`), and the host
synchronises once per position.
"""
from __future__ import annotations

import math
from typing import Any, NamedTuple, Optional

import torch

from . import ops
from .model import _require_device

LOGZERO = -1.0e10          # ctc_prefix_score.py:33
BF16 = torch.bfloat16


class Hypothesis(NamedTuple):
    """beam_search.py:17-33."""

    yseq: torch.Tensor
    score: float = 0.0
    scores: dict = {}
    states: dict = {}

    def asdict(self) -> dict:
        return dict(yseq=self.yseq.tolist(), score=float(self.score), scores={k: float(v) for k, v in self.scores.items()})


def end_detect(ended_hyps: list, i: int, M: int = 3, D_end: float = math.log(1 * math.exp(-10))) -> bool:
    """Eq. (50) of Watanabe et al. (e2e_asr_common.py:19-49): stop when, for each of the last M lengths, the best hypothesis that
    ended with that length scores more than |D_end| below the best ended hypothesis."""
    if not ended_hyps:
        return False
    best = max(float(h["score"]) for h in ended_hyps)
    count = 0
    for m in range(M):
        same = [float(h["score"]) for h in ended_hyps if len(h["yseq"]) == i - m]
        if same and max(same) - best < D_end:
            count += 1
    return count == M


# ----------------------------------------------------------------------------------------------------
# scorers
# ----------------------------------------------------------------------------------------------------
class LengthBonus:
    """scorers/length_bonus.py: +1 per emitted token (weighted by `penalty`)."""

    def __init__(self, n_vocab: int):
        self.n = int(n_vocab)

    def select_states(self, states, prev, tok):
        return None

    # -- clip-aware protocol: the bonus does not look at the clip
    def batch_init_state_clips(self, xs, lengths):
        self._like = xs
        return None

    def batch_score_clips(self, ys, states, clip_of):
        return torch.ones((ys.shape[0], self.n), dtype=self._like.dtype, device=self._like.device), None


class DecoderScorer:
    """The attention decoder as a full-vocabulary scorer (transformer/decoder.py:153-220), incremental like the reference's
    `forward_one_step(..., cache)` (decoder.py:153-186 + decoder_layer.py:67-103): a step computes ONE new row per hypothesis.

    State / cache: one tensor per decoder layer, [n, L, 3*ddim] = (layer output | self-attention key | self-attention value) of the
    L positions scored so far — a list of per-layer [n, L, .] tensors exactly like the reference's cache, so generic scorer plumbing
    (stack / index by hypothesis) works on it unchanged.  The reference caches the layer outputs only and re-projects keys and
    values of the whole prefix every step; keeping them too makes a step O(L) in the attention alone.  The source-attention keys /
    values of `memory` (recomputed per step in the reference, decoder_layer.py:106-113) are projected once per clip and layer."""

    def __init__(self, model):
        self.model = model
        self._mem = None          # (memory tensor, version, per-layer [T, 2D] of ONE row when all rows alias it | None, {n: [per-layer [n*T, 2D]]})

    # -- ScorerInterface / BatchScorerInterface ---------------------------------------------------
    def init_state(self, x):
        return None

    def batch_init_state(self, x):
        return None

    def select_state(self, state, i, new_id=None):
        return None if state is None else [c[i] for c in state]

    def select_states(self, states, prev, tok):
        return None if states is None else tuple(c[prev] for c in states)

    # -- source-attention keys / values -----------------------------------------------------------
    def _src_kv(self, st, mem, rows: int):
        """Per layer, the fused source-attention k | v projection of `rows` memory rows: bf16 [rows, 2 * ddim]."""
        from .lrs_model import _lin

        m = self.model
        return [_lin(st, mem, f"decoder.decoders.{i}.src_attn.linear_k", rows, m.ddim, 2 * m.ddim) for i in range(m.dlayers)]

    def _memory_kv(self, st, memory: torch.Tensor, n: int, T: int):
        m = self.model
        D = m.ddim
        c = self._mem
        try:                       # inference tensors (torch.inference_mode) carry no version counter: identity + weights generation decide alone
            ver = memory._version
        except RuntimeError:
            ver = -1
        gen = getattr(st, "generation", 0)          # bumped by every optimiser step / shadow refresh: cached keys / values follow the weights
        same = (c is not None and c["ptr"] == memory.data_ptr() and c["ver"] == ver and c["gen"] == gen and c["T"] == T and c["stride"] == memory.stride()
                and c["base"] is memory._base)
        if not same:
            c = self._mem = dict(ptr=memory.data_ptr(), ver=ver, gen=gen, T=T, stride=memory.stride(), base=memory._base, keep=memory, row=None, by_n={})
        if n in c["by_n"]:
            return c["by_n"][n]
        aliased = n > 1 and memory.stride(0) == 0           # x.unsqueeze(0).expand(n, T, D): every hypothesis attends to the same clip
        if aliased or n == 1:
            if c["row"] is None:
                mem = memory[0].to(BF16).contiguous()
                c["row"] = self._src_kv(st, mem, T)
            kv = [r.unsqueeze(0).expand(n, T, 2 * D).reshape(n * T, 2 * D).contiguous() if n > 1 else r for r in c["row"]]
        else:
            mem = memory.to(BF16).reshape(n * T, D).contiguous()
            kv = self._src_kv(st, mem, n * T)
        c["by_n"] = {n: kv}                                  # (the beam only shrinks or stays: one width at a time is enough)
        return kv

    def forward_one_step(self, tgt: torch.Tensor, tgt_mask, memory: torch.Tensor, memory_mask=None, cache=None):
        """tgt int64 [n, L], memory [n, T, ddim], cache: None or per-layer [n, L-1, 3*ddim] from the previous step ->
        (log-probabilities of the next token [n, odim], new cache: per-layer [n, L, 3*ddim]).  `tgt_mask` is the causal mask by
        construction (decoder.py:189,216).  Without a cache the whole prefix is computed (and the cache built); with one, only
        position L-1."""
        from .lrs_model import LrsTargets, _decoder_fwd

        m = self.model
        if m.training:
            raise RuntimeError("forward_one_step is an inference entry point: call model.eval() first")
        if memory.size(-1) != m.ddim:
            raise ValueError(f"memory is {memory.size(-1)} wide, the decoder expects ddim = {m.ddim} (the reference feeds the encoder "
                             "output to the decoder directly at inference, lightning.py:114-119, which needs adim == ddim)")
        st = _fresh_store(m, self)
        n, L = tgt.shape
        T, D = memory.size(1), m.ddim
        if memory_mask is not None:
            ilen = memory_mask.reshape(n, -1).sum(-1).to(torch.int32).contiguous()
        else:
            ilen = torch.full((n,), T, dtype=torch.int32, device=memory.device)
        if cache is not None and (len(cache) != m.dlayers or any(c is None for c in cache)):
            cache = None
        if cache is not None and (cache[0].shape[0] != n or cache[0].shape[1] != L - 1 or cache[0].shape[2] != 3 * D):
            raise ValueError(f"cache entries are {tuple(cache[0].shape)}, expected ({n}, {L - 1}, {3 * D}): the cache must come from the "
                             "previous forward_one_step call for the same hypotheses")
        with torch.no_grad():
            if cache is None or L == 1:
                tg = LrsTargets(None, tgt.contiguous(), None)
                mem = memory.to(BF16).reshape(n * T, D).contiguous()
                tape: dict[str, Any] = {}
                pred = _decoder_fwd(m, st, tape, tg, mem, ilen, n, T)                # fp32 [n * L, odim padded to 64]
                logits = pred.view(n, L, -1)[:, -1, : m.odim]
                new_cache = tuple(torch.cat((tape[f"decoder.decoders.{i}"]["out"].view(n, L, D),
                                             tape[f"decoder.decoders.{i}"]["self"]["qkv"].view(n, L, 3 * D)[:, :, D:]), dim=2) for i in range(m.dlayers))
            else:
                logits, new_cache = self._step_cached(st, tgt, memory, ilen, cache, n, L, T)
        return torch.log_softmax(logits.float(), dim=-1), new_cache

    def _step_cached(self, st, tgt, memory, ilen, cache, n: int, L: int, T: int):
        """Position L-1 of every hypothesis on top of `cache`, every row attending to its own `memory` row."""
        D, H = self.model.ddim, self.model.dheads
        memkv = self._memory_kv(st, memory, n, T)
        return self._step(st, tgt, cache, lambda i, q: ops.mha_fwd(q, D, memkv[i], memkv[i][:, D:], 2 * D, B=n, H=H, Lq=1, Lk=T, klen=ilen)[0])

    def _step(self, st, ys, cache, src_attn):
        """Position L-1 of every hypothesis on top of `cache` (decoder_layer.py:67-127 with tgt_q = tgt[:, -1:]): ys int64 [n, L], cache
        per-layer [n, L-1, 3*ddim], src_attn(layer index, q bf16 [n, ddim]) -> the source-attention context of that layer ->
        (logits fp32 [n, odim], new cache)."""
        from .lrs_model import _ffn_fwd, _lin, _ln

        m = self.model
        D, U, H = m.ddim, m.dunits, m.dheads
        n, L = ys.shape
        pe = m._pos_table("abs", L, ys.device)
        x = ops.embed_pos_fwd(ys[:, -1:].contiguous(), st.p32("decoder.embed.0.weight"), pe[L - 1 : L].contiguous(), 1, D, math.sqrt(D))   # [n, D]
        new_cache = []
        for i in range(m.dlayers):
            p = f"decoder.decoders.{i}"
            c = cache[i]
            t1, _, _ = _ln(st, x, f"{p}.norm1")
            qkv = _lin(st, t1, f"{p}.self_attn.linear_q", n, D, 3 * D)                                     # this position's q | k | v
            kv = torch.cat((c[:, :, D:], qkv[:, D:].unsqueeze(1)), dim=1).view(n * L, 2 * D)               # keys / values 0..L-1
            ctx, _ = ops.mha_fwd(qkv, 3 * D, kv, kv[:, D:], 2 * D, B=n, H=H, Lq=1, Lk=L)                     # the last query sees every key
            x1 = _lin(st, ctx, f"{p}.self_attn.linear_out", n, D, D, addend=x)
            t2, _, _ = _ln(st, x1, f"{p}.norm2")
            ctx2 = src_attn(i, _lin(st, t2, f"{p}.src_attn.linear_q", n, D, D))
            x2 = _lin(st, ctx2, f"{p}.src_attn.linear_out", n, D, D, addend=x1)
            x = _ffn_fwd(m, st, {}, "ff", x2, f"{p}.feed_forward", n, D, U, 1.0, f"{p}.norm3", f"dec.{i}.ff")
            new_cache.append(torch.cat((c, torch.cat((x, qkv[:, D:]), dim=1).unsqueeze(1)), dim=1))
        tn, _, _ = _ln(st, x, "decoder.after_norm")
        V = m.odim
        pred = ops.linear_fwd(tn, st.s16("decoder.output_layer.weight"), st.p32("decoder.output_layer.bias"), rows=n, K=D, N=V, x_pitch=D,
                              out_f32=True, out_pitch=(V + 63) // 64 * 64)[0]
        return pred[:, :V], tuple(new_cache)

    # -- clip-aware protocol (BatchBeamSearch.forward_clips) ---------------------------------------
    def batch_init_state_clips(self, xs: torch.Tensor, lengths):
        """xs [C, Tmax, ddim] padded encoder outputs, lengths [C]: projects the source keys / values of every clip and layer in ONE
        [C * Tmax]-row GEMM per layer; a step's query rows find their clip's block through `clip_of` (svsr_mha_src_step_fwd), so no
        per-hypothesis copy of them is ever made.  Rows beyond a clip's length are projected but never read."""
        m = self.model
        if m.training:
            raise RuntimeError("batch_init_state_clips is an inference entry point: call model.eval() first")
        if xs.dim() != 3 or xs.size(-1) != m.ddim:
            raise ValueError(f"xs is {tuple(xs.shape)}, the decoder expects [clips, frames, ddim = {m.ddim}] (the reference feeds the encoder "
                             "output to the decoder directly at inference, lightning.py:114-119, which needs adim == ddim)")
        _require_device(xs)
        st = _fresh_store(m, self)
        C, Tmax, D = xs.shape
        tlen = torch.as_tensor(lengths, dtype=torch.int32).to(xs.device).contiguous()
        with torch.no_grad():
            kv = self._src_kv(st, xs.to(BF16).reshape(C * Tmax, D).contiguous(), C * Tmax)
        self._clips = dict(kv=kv, tlen=tlen, C=C, Tmax=Tmax, dev=xs.device)
        return None

    def batch_score_clips(self, ys: torch.Tensor, states, clip_of: torch.Tensor):
        """ys int64 [n, L], states: None (first position) or the batched cache (per-layer [n, L-1, 3*ddim]), clip_of int32 [n] ->
        (log-probabilities of the next token [n, odim], new cache).  Every position, the first included, goes through the one-row step:
        the cache of the first position is empty."""
        m, ck = self.model, self._clips
        D, H = m.ddim, m.dheads
        n, L = ys.shape
        st = m.store()
        if states is None:
            if L != 1:
                raise ValueError("the decoder scorer of a multi-clip search starts from the <sos> column: states may be None at the first position only")
            states = tuple(torch.empty((n, 0, 3 * D), dtype=BF16, device=ys.device) for _ in range(m.dlayers))
        if len(states) != m.dlayers or states[0].shape != (n, L - 1, 3 * D):
            raise ValueError(f"cache entries are {tuple(states[0].shape)}, expected ({n}, {L - 1}, {3 * D}): the cache must come from the "
                             "previous scoring call for the same hypotheses")
        with torch.no_grad():
            logits, new_cache = self._step(st, ys, states, lambda i, q: ops.mha_src_step_fwd(q, ck["kv"][i], clip_of, ck["tlen"], Tmax=ck["Tmax"], H=H))
            return torch.log_softmax(logits.float(), dim=-1), new_cache

    def score(self, ys: torch.Tensor, state, x: torch.Tensor):
        logp, cache = self.forward_one_step(ys.unsqueeze(0), None, x.unsqueeze(0), cache=None if state is None else [c.unsqueeze(0) for c in state])
        return logp.squeeze(0), [c.squeeze(0) for c in cache]

    def batch_score(self, ys: torch.Tensor, states, xs: torch.Tensor):
        """states: None (first step) or the batched cache (per-layer [n, L-1, 3*ddim], as select_states returns it); a list of
        per-hypothesis states (the reference's calling convention, batch_beam_search.py) is stacked first."""
        if isinstance(states, list) and states and isinstance(states[0], (list, tuple)):
            states = [torch.stack([s[i] for s in states]) for i in range(len(states[0]))]
        elif isinstance(states, list):                      # [None] * n
            states = None
        return self.forward_one_step(ys, None, xs, cache=states)


def _fresh_store(model, scorer=None):
    """What every inference entry point does first: join the side stream (a TrainStep may have left the tail of its optimiser step there)
    and bring the bf16 shadows up to date; a decoder scorer then drops the source keys / values it projected with the old weights."""
    st = model.store()
    model._side.join()
    if not st.shadow_fresh:
        st.refresh_shadows()
        if scorer is not None:
            scorer._mem = None
    return st


class CTCPrefixScorer:
    """CTC prefix scores of the candidate extensions (scorers/ctc.py:87-127 + ctc_prefix_score.py:11-165).  State of the running
    hypotheses: (r [n, T, 2] forward log-probabilities ending in non-blank / blank, s [n] log prefix probability)."""

    blank = 0

    def __init__(self, model, eos: int):
        self.model, self.eos = model, int(eos)
        self.logp: Optional[torch.Tensor] = None

    def ctc_logits(self, x: torch.Tensor) -> torch.Tensor:
        """ctc_lo alone: x [T, adim] -> fp32 LOGITS [T, odim rounded up to 64] (the first odim columns are the units; the rest is padding)."""
        m = self.model
        st = _fresh_store(m)
        T = x.size(0)
        with torch.no_grad():
            return ops.linear_fwd(x.to(BF16).contiguous(), st.s16("ctc.ctc_lo.weight"), st.p32("ctc.ctc_lo.bias"), rows=T, K=m.adim, N=m.odim,
                                  x_pitch=m.adim, out_f32=True, out_pitch=(m.odim + 63) // 64 * 64)[0]

    def ctc_log_softmax(self, x: torch.Tensor) -> torch.Tensor:
        """`CTC.log_softmax` (ctc.py:163-170): x [T, adim] -> fp32 [T, odim]."""
        return torch.log_softmax(self.ctc_logits(x)[:, : self.model.odim].float(), dim=-1).contiguous()

    def batch_init_state(self, x: torch.Tensor):
        self.logp = self.ctc_log_softmax(x)
        return None

    def _prefix(self, logp, r_prev, last, ids, out_len):
        return ops.ctc_prefix_score(logp, r_prev, last, ids, out_len, self.blank, self.eos)

    def batch_score_partial(self, y: torch.Tensor, ids: Optional[torch.Tensor], state, x: torch.Tensor):
        """y int64 [n, L] (with <sos>), ids int64 [n, S] or None -> (scores [n, odim]: log psi(prefix + c) - log psi(prefix), with
        -1e10 for labels outside ids and for blank, pending state for select_states)."""
        logp = self.logp
        T, V = logp.shape
        n = y.shape[0]
        if state is None:
            r_prev = torch.full((T, 2), LOGZERO, dtype=logp.dtype, device=logp.device)
            r_prev[:, 1] = torch.cumsum(logp[:, self.blank], 0)
            r_prev = r_prev.unsqueeze(0).expand(n, T, 2).contiguous()
            s_prev = torch.zeros(n, dtype=logp.dtype, device=logp.device)
        else:
            r_prev, s_prev = state
        return self._score_partial(y, ids, r_prev, s_prev, V, r_prev[:, T - 1],
                                   lambda r, last, ids_c, out_len: self._prefix(logp, r, last, ids_c, out_len))

    def _score_partial(self, y, ids, r_prev, s_prev, V: int, end, prefix):
        """The part both protocols share.  prefix(r_prev, last label, ids, labels in the prefix) -> (r_new, psi) is the recursion; end [n, 2]
        is r_prev at the last frame of each hypothesis' clip, which gives <eos> its score."""
        ids_c = None if ids is None else ids.contiguous()
        r_new, psi = prefix(r_prev.contiguous(), y[:, -1].contiguous(), ids_c, y.shape[1] - 1)
        if ids_c is None:
            full = psi.clone()
        else:
            full = torch.full((y.shape[0], V), LOGZERO, dtype=psi.dtype, device=psi.device).scatter_(1, ids_c, psi)
        full[:, self.eos] = torch.logaddexp(end[:, 0], end[:, 1])
        full[:, self.blank] = LOGZERO
        return full - s_prev.unsqueeze(1), (r_new, full, ids_c)

    # -- clip-aware protocol -------------------------------------------------------------------------
    def batch_init_state_clips(self, xs: torch.Tensor, lengths):
        """xs [C, Tmax, adim]: the posteriors of every clip in one GEMM + one log-softmax -> self.logp_clips fp32 [C, Tmax, odim]."""
        C, Tmax = xs.shape[:2]
        self.logp_clips = self.ctc_log_softmax(xs.reshape(C * Tmax, xs.shape[2])).view(C, Tmax, -1)
        self.tlen = torch.as_tensor(lengths, dtype=torch.int32).to(xs.device).contiguous()
        return None

    def _prefix_clips(self, logp, tlen, r_prev, last, ids, clip_of, out_len):
        return ops.ctc_prefix_score_clips(logp, tlen, r_prev, last, ids, clip_of, out_len, self.blank, self.eos)

    def batch_score_partial_clips(self, y: torch.Tensor, ids: Optional[torch.Tensor], state, clip_of: torch.Tensor):
        """`batch_score_partial` with hypothesis r scored against the tlen[clip_of[r]] frames of its own clip.  State: (r [n, Tmax, 2] with
        -1e10 beyond the clip's length, s [n])."""
        logp, tlen = self.logp_clips, self.tlen
        C, Tmax, V = logp.shape
        n = y.shape[0]
        cl = clip_of.long()
        if state is None:
            live = torch.arange(Tmax, device=logp.device).unsqueeze(0) < tlen.unsqueeze(1)                  # [C, Tmax]
            r0 = torch.full((C, Tmax, 2), LOGZERO, dtype=logp.dtype, device=logp.device)
            r0[:, :, 1] = torch.where(live, torch.cumsum(logp[:, :, self.blank], 1), r0[:, :, 1])
            r_prev = r0[cl].contiguous()
            s_prev = torch.zeros(n, dtype=logp.dtype, device=logp.device)
        else:
            r_prev, s_prev = state
        end = r_prev[torch.arange(n, device=logp.device), tlen.long()[cl] - 1]                                  # [n, 2]: the clip's last frame
        return self._score_partial(y, ids, r_prev, s_prev, V, end,
                                   lambda r, last, ids_c, out_len: self._prefix_clips(logp, tlen, r, last, ids_c, clip_of, out_len))

    def select_states(self, pending, prev: torch.Tensor, tok: torch.Tensor):
        """State of the extensions (prev[i], tok[i])."""
        r_new, full, ids = pending
        if ids is None:
            j = tok
        else:
            idmap = torch.full(full.shape, 0, dtype=torch.int64, device=full.device).scatter_(
                1, ids, torch.arange(ids.shape[1], device=full.device).expand_as(ids))
            j = idmap[prev, tok]
        return r_new[prev, j].contiguous(), full[prev, tok].contiguous()


# ----------------------------------------------------------------------------------------------------
# the adapter for single-clip scorers, and the torch statement of the selection step
# ----------------------------------------------------------------------------------------------------
def _ranges(clip_of) -> dict:
    """{clip: (first row, end row)} of a non-decreasing row -> clip map (host side)."""
    out: dict = {}
    for r, c in enumerate(clip_of.tolist() if isinstance(clip_of, torch.Tensor) else clip_of):
        lo, _ = out.get(c, (r, r))
        out[c] = (lo, r + 1)
    return out


class _ClipStates:
    """State of a PerClipScorers: {clip: (first row, end row, that clip's batched state)}.  Indexing by a tensor of rows (the search's
    `keep` gather) splits the rows by clip and indexes every clip's state with its local rows."""

    def __init__(self, per: dict):
        self.per = per

    def split(self, rows: torch.Tensor):
        """rows (global, grouped by clip in clip order) -> [(clip, positions lo, hi in `rows`, local rows)]."""
        host = rows.tolist()
        out, pos = [], 0
        for c, (lo, hi, _) in self.per.items():
            start = pos
            while pos < len(host) and lo <= host[pos] < hi:
                pos += 1
            if pos > start:
                out.append((c, start, pos, rows[start:pos] - lo))
        if pos != len(host):
            raise ValueError("rows of a multi-clip search must stay grouped by clip, in clip order")
        return out

    def __getitem__(self, keep: torch.Tensor) -> "_ClipStates":
        return _ClipStates({c: (a, b, BatchBeamSearch._take(self.per[c][2], loc)) for c, a, b, loc in self.split(keep)})


class PerClipScorers:
    """Adapter: any scorer that speaks the single-clip protocol (`batch_init_state(x)`, `batch_score(ys, states, xs)` or
    `batch_score_partial(y, ids, state, x)`, `select_states`) as a clip-aware scorer of `BatchBeamSearch`.  Rows are split by clip, the
    wrapped scorer is called once per clip with that clip's unpadded encoder output, and the answers are concatenated: correct for every
    scorer, and as slow as one search per clip for this scorer's share of a step.  The single-clip protocol lets a scorer keep data of its
    clip on itself (CTCPrefixScorer.logp), so every clip gets its own shallow copy of the wrapped scorer: attributes that
    `batch_init_state` sets land on the copy.  `copies=False` (one clip only) hands the clip to the wrapped scorer itself, which is what
    the reference's search does and how `BatchBeamSearch.forward` wraps."""

    def __init__(self, scorer, copies: bool = True):
        self.scorer, self.copies = scorer, copies
        self._per: dict = {}
        if hasattr(scorer, "batch_score_partial"):           # (the attribute marks a partial scorer for BatchBeamSearch's constructor)
            self.batch_score_partial_clips = self._batch_score_partial_clips

    def batch_init_state_clips(self, xs: torch.Tensor, lengths):
        import copy

        if not self.copies and len(lengths) != 1:
            raise ValueError("PerClipScorers(copies=False) serves one clip")
        self._per = {}
        per = {}
        for c, T in enumerate(int(v) for v in lengths):
            d = copy.copy(self.scorer) if self.copies else self.scorer
            x = xs[c, :T]
            self._per[c] = (d, x)
            per[c] = (c, c + 1, d.batch_init_state(x))
        return _ClipStates(per)

    def _each(self, ys, states, clip_of, call):
        rng = _ranges(clip_of)
        scores, per = [], {}
        for c, (lo, hi) in rng.items():
            d, x = self._per[c]
            st = states.per[c][2] if isinstance(states, _ClipStates) and c in states.per else None
            sc, new = call(d, x, lo, hi, st)
            scores.append(sc)
            per[c] = (lo, hi, new)
        return torch.cat(scores, dim=0), _ClipStates(per)

    def batch_score_clips(self, ys, states, clip_of):
        return self._each(ys, states, clip_of, lambda d, x, lo, hi, st: d.batch_score(ys[lo:hi], st, x.unsqueeze(0).expand(hi - lo, *x.shape)))

    def _batch_score_partial_clips(self, ys, ids, states, clip_of):
        return self._each(ys, states, clip_of,
                          lambda d, x, lo, hi, st: d.batch_score_partial(ys[lo:hi], None if ids is None else ids[lo:hi], st, x))

    def select_states(self, states: _ClipStates, prev: torch.Tensor, tok: torch.Tensor):
        return _ClipStates({c: (a, b, self._per[c][0].select_states(states.per[c][2], loc, tok[a:b])) for c, a, b, loc in states.split(prev)})


def beam_select_reference(planes, weights, run: torch.Tensor, row_lo, beam: int, V: int):
    """The torch statement of the selection step — what svsr_beam_select computes, and the path of everything but fp32 CUDA tensors.
    planes [n, >= V] with their weights, in order; run [n]; row_lo: host list [C + 1] of the clips' row ranges.  weighted = zeros;
    weighted += w_k * s_k for every plane; weighted += run[:, None]; per clip the min(beam, rows * V) best (row, token), higher first,
    ties to the lower (row, token) -> (prev [m] global rows, tok [m], total [m], vals [P, m]: each plane at the winners, count: list [C])."""
    n = run.numel()
    weighted = torch.zeros((n, V), dtype=run.dtype, device=run.device)
    for w, sc in zip(weights, planes):
        weighted += w * sc[:, :V].to(run.dtype)
    weighted += run.unsqueeze(1)
    prev, tok, count = [], [], []
    for c in range(len(row_lo) - 1):
        lo, hi = int(row_lo[c]), int(row_lo[c + 1])
        k = min(int(beam), max(hi - lo, 0) * V)
        count.append(k)
        if k == 0:
            continue
        order = torch.sort(weighted[lo:hi].reshape(-1), descending=True, stable=True)[1][:k]
        prev.append(lo + torch.div(order, V, rounding_mode="trunc"))
        tok.append(order % V)
    if not prev:
        e = torch.empty(0, dtype=torch.int64, device=run.device)
        return e, e, weighted.new_empty(0), weighted.new_empty((len(planes), 0)), count
    prev, tok = torch.cat(prev), torch.cat(tok)
    return prev, tok, weighted[prev, tok], torch.stack([sc[prev, tok].to(run.dtype) for sc in planes]), count


# ----------------------------------------------------------------------------------------------------
# batch beam search
# ----------------------------------------------------------------------------------------------------
class BatchBeamSearch:
    """beam_search.py:36-113 (constructor contract) + batch_beam_search.py (one vectorised step per output position)."""

    def __init__(self, beam_size: int, vocab_size: int, weights: dict, scorers: dict, sos: int, eos: int, token_list=None,
                 pre_beam_ratio: float = 1.5, pre_beam_score_key: Optional[str] = None):
        self.weights = weights
        self.scorers, self.full_scorers, self.part_scorers = {}, {}, {}
        for k, v in scorers.items():
            if weights.get(k, 0) == 0 or v is None:          # beam_search.py:73-76
                continue
            self.scorers[k] = v
            partial = hasattr(v, "batch_score_partial") or hasattr(v, "batch_score_partial_clips")
            (self.part_scorers if partial else self.full_scorers)[k] = v
        self.sos, self.eos, self.token_list = int(sos), int(eos), token_list
        self.beam_size, self.n_vocab = int(beam_size), int(vocab_size)
        self.pre_beam_size = int(pre_beam_ratio * beam_size)
        if pre_beam_score_key is not None and pre_beam_score_key != "full" and pre_beam_score_key not in self.full_scorers:
            raise KeyError(f"{pre_beam_score_key} is not found in {self.full_scorers}")
        self.pre_beam_score_key = pre_beam_score_key
        self.do_pre_beam = pre_beam_score_key is not None and self.pre_beam_size < self.n_vocab and len(self.part_scorers) > 0

    @staticmethod
    def _take(states, keep: torch.Tensor):
        if states is None:
            return None
        if isinstance(states, tuple):
            return tuple(s[keep] for s in states)
        return states[keep]

    def forward(self, x: torch.Tensor, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> list:
        """x: encoder output of ONE clip [T, D] -> ended hypotheses, best first (beam_search.py:333-405): the search below with one clip."""
        if x.dim() != 2:
            raise ValueError(f"x must be the encoder output of one clip [frames, D], got {tuple(x.shape)}")
        if x.shape[0] == 0:
            return []
        return self._forward_group(x.unsqueeze(0), [x.shape[0]], maxlenratio, minlenratio, copies=False)[0]

    __call__ = forward

    # ------------------------------------------------------------------------------------------------
    # the search: C clips advance in lock step
    # ------------------------------------------------------------------------------------------------
    # Device bytes the CTC scorer's pending state [rows, candidates, Tmax, 2] fp32 of one step may take.  A batch whose C * beam rows
    # would exceed it is decoded in groups of consecutive clips that fit (full-vocabulary partial scoring, ctc_weight == 1.0, at beam 40
    # over 5,049 units and 150 frames is 242 MB per clip: 8 clips per group; with the pre-beam of 60 candidates it is 2.9 MB per clip).
    clip_workspace_bytes = 2 << 30

    def clips_per_group(self, Tmax: int) -> int:
        """Clips `forward_clips` decodes together at `Tmax` padded frames under `clip_workspace_bytes` (at least 1)."""
        if not self.part_scorers:
            return 1 << 30
        cand = self.pre_beam_size if self.do_pre_beam else self.n_vocab
        return max(1, int(self.clip_workspace_bytes) // (self.beam_size * cand * int(Tmax) * 2 * 4))

    def _clip_scorers(self, dev, copies: bool = True) -> dict:
        """The scorers as the search speaks to them.  The clip-aware methods of this package's scorers are HIP launches, while their
        single-clip protocol is the reference's and runs wherever its hooks do (a subclass that restates `CTCPrefixScorer._prefix` in torch
        scores CPU tensors): a scorer that speaks both is driven clip-aware for device tensors and through `PerClipScorers` otherwise."""
        out = {}
        for k, d in self.scorers.items():
            single = hasattr(d, "batch_init_state") and hasattr(d, "batch_score_partial" if k in self.part_scorers else "batch_score")
            clips = hasattr(d, "batch_init_state_clips") and hasattr(d, "batch_score_partial_clips" if k in self.part_scorers else "batch_score_clips")
            if isinstance(d, PerClipScorers) or (clips and (dev.type == "cuda" or not single)):
                out[k] = d
            else:
                out[k] = PerClipScorers(d, copies)
        return out

    def _select(self, planes, weights, run_score, clip_of, rows, meta):
        """-> (prev, tok, total, vals [P, m], clip_of of the winners).  rows: host list of rows per clip; meta: int32 device tensor
        row_lo [C + 1] | out_off [C] (made where the host last synchronised), None on CPU.  The kernel adds fp32 planes; every other
        dtype, and CPU tensors, take the torch statement."""
        V, beam = self.n_vocab, self.beam_size
        if run_score.device.type == "cuda" and run_score.dtype == torch.float32:
            C = len(rows)
            prev, tok, total, vals, clip_out, _ = ops.beam_select(
                [s.to(torch.float32) for s in planes], weights, run_score.contiguous(), clip_of, meta[: C + 1], meta[C + 1 :], beam=beam, V=V,
                max_rows=max(rows), out_rows=sum(min(beam, r * V) for r in rows))
            return prev, tok, total, vals, clip_out
        row_lo = [0]
        for r in rows:
            row_lo.append(row_lo[-1] + r)
        prev, tok, total, vals, _ = beam_select_reference(planes, weights, run_score, row_lo, beam, V)
        return prev, tok, total, vals, clip_of[prev]

    def _search_clips(self, run: dict, scorers: dict, rows: list, dtype) -> dict:
        """One position of every live clip (batch_beam_search.py:180-275): run = dict(yseq [n, L], score [n], scores {k: [n]}, states
        {k: batched state}, clip_of [n], meta); full scorers, the pre-beam, partial scorers, then the per-clip selection."""
        yseq, clip_of = run["yseq"], run["clip_of"]
        sc, st = {}, {}
        for k in self.full_scorers:
            sc[k], st[k] = scorers[k].batch_score_clips(yseq, run["states"][k], clip_of)
        part_ids = None
        if self.do_pre_beam:
            if self.pre_beam_score_key == "full":
                pre = torch.zeros((yseq.shape[0], self.n_vocab), dtype=dtype, device=yseq.device)
                for k in self.full_scorers:
                    pre += self.weights[k] * sc[k].to(dtype)
            else:
                pre = sc[self.pre_beam_score_key]
            part_ids = torch.topk(pre, self.pre_beam_size, dim=-1)[1]          # per row: the clips do not meet here
        for k in self.part_scorers:
            sc[k], st[k] = scorers[k].batch_score_partial_clips(yseq, part_ids, run["states"][k], clip_of)
        order = list(self.full_scorers) + list(self.part_scorers)              # the order the planes are added up in
        prev, tok, total, vals, new_clip = self._select([sc[k].to(dtype) for k in order], [self.weights[k] for k in order], run["score"], clip_of,
                                                        rows, run["meta"])
        return dict(
            yseq=torch.cat((yseq[prev], tok.unsqueeze(1)), dim=1),
            score=total,
            scores={k: run["scores"][k][prev] + vals[j] for j, k in enumerate(order)},
            states={k: scorers[k].select_states(st[k], prev, tok) for k in order},
            clip_of=new_clip,
        )

    def forward_clips(self, xs: torch.Tensor, lengths, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> list:
        """xs: padded encoder outputs of C clips [C, Tmax, D], lengths [C] (int tensor or list) -> per clip the ended hypotheses, best
        first: element c is what `forward(xs[c, :lengths[c]])`, the same search with that clip alone, returns.  All clips start
        together, so every live hypothesis has the same prefix length at every position; each clip keeps its own length limit, end detection and ended list, and a clip that has finished
        simply stops contributing rows.  One host synchronisation per position for all clips together.  Scorers without the clip-aware
        methods are wrapped in `PerClipScorers`.  Batches beyond `clips_per_group(Tmax)` clips are decoded in groups of consecutive
        clips (`clip_workspace_bytes`)."""
        if xs.dim() != 3:
            raise ValueError(f"xs must be [clips, frames, D], got {tuple(xs.shape)}")
        lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        C, Tmax = xs.shape[:2]
        if len(lens) != C:
            raise ValueError(f"{len(lens)} lengths for {C} clips")
        if any(t < 1 or t > Tmax for t in lens):
            raise ValueError(f"lengths must lie in [1, {Tmax}] (the padded frame count), got {lens}")
        G = self.clips_per_group(Tmax)
        out: list = []
        for g0 in range(0, C, G):
            ls = lens[g0 : g0 + G]
            out += self._forward_group(xs[g0 : g0 + G, : max(ls)], ls, maxlenratio, minlenratio)
        return out

    def _forward_group(self, xs: torch.Tensor, lens: list, maxlenratio: float, minlenratio: float, copies: bool = True) -> list:
        C, dev, dt = xs.shape[0], xs.device, xs.dtype
        V, beam = self.n_vocab, self.beam_size
        if maxlenratio == 0:
            maxlen = list(lens)
        elif maxlenratio < 0:
            maxlen = [-1 * int(maxlenratio)] * C
        else:
            maxlen = [max(1, int(maxlenratio * t)) for t in lens]
        scorers = self._clip_scorers(dev, copies)
        rows = [1 if maxlen[c] > 0 else 0 for c in range(C)]                      # live hypotheses per clip (host bookkeeping)
        first = [c for c in range(C) if rows[c]]
        run = dict(yseq=torch.full((len(first), 1), self.sos, dtype=torch.int64, device=dev), score=torch.zeros(len(first), dtype=dt, device=dev),
                   scores={k: torch.zeros(len(first), dtype=dt, device=dev) for k in self.scorers},
                   states={k: d.batch_init_state_clips(xs, lens) for k, d in scorers.items()},
                   clip_of=torch.tensor(first, dtype=torch.int32, device=dev), meta=self._meta(rows, dev))
        ended: list[list] = [[] for _ in range(C)]
        wide = torch.float64 if dt == torch.float64 else torch.float32          # holds tokens (< 2^24) and narrower scores exactly
        i = 0
        while sum(rows) > 0:
            run = self._search_clips(run, scorers, rows, dt)
            rows = [min(beam, r * V) for r in rows]
            names = list(run["scores"])
            host = torch.stack([run["yseq"][:, -1].to(wide), run["score"].to(wide)] + [run["scores"][k].to(wide) for k in names]).cpu()
            last, score, parts = host[0].tolist(), host[1].tolist(), [h.tolist() for h in host[2:]]
            keep, b = [], 0
            for c in range(C):
                n_c, limit, kept = rows[c], i == maxlen[c] - 1, 0
                for r in range(b, b + n_c):
                    if limit or int(last[r]) == self.eos:      # batch_beam_search.py:318-334: the length limit closes every running hypothesis
                        y = run["yseq"][r]
                        if limit:
                            y = torch.cat((y, y.new_full((1,), self.eos)))
                        ended[c].append(Hypothesis(yseq=y, score=score[r], scores={k: parts[j][r] for j, k in enumerate(names)}))
                    else:
                        keep.append(r)
                        kept += 1
                if kept and maxlenratio == 0.0 and end_detect([dict(score=h.score, yseq=h.yseq) for h in ended[c]], i):
                    del keep[len(keep) - kept :]
                    kept = 0
                b += n_c
                rows[c] = kept
            if len(keep) != b:                                   # rows of ended hypotheses and of finished clips leave together
                kt = torch.tensor(keep, dtype=torch.int64, device=dev)
                run = dict(yseq=run["yseq"][kt], score=run["score"][kt], scores={k: v[kt] for k, v in run["scores"].items()},
                           states={k: self._take(v, kt) for k, v in run["states"].items()}, clip_of=run["clip_of"][kt])
            run["meta"] = self._meta(rows, dev)
            i += 1
        out = []
        for c in range(C):
            nbest = sorted(ended[c], key=lambda h: h.score, reverse=True)
            if not nbest and minlenratio >= 0.1:                 # beam_search.py:383-392
                nbest = self._forward_group(xs[c : c + 1, : lens[c]], lens[c : c + 1], maxlenratio, max(0.0, minlenratio - 0.1), copies)[0]
            out.append(nbest)
        return out

    def _meta(self, rows: list, dev):
        """row_lo [C + 1] | out_off [C] of the next selection as one int32 device tensor (CPU tensors: not needed)."""
        if dev.type != "cuda":
            return None
        lo, off = [0], [0]
        for r in rows:
            lo.append(lo[-1] + r)
            off.append(off[-1] + min(self.beam_size, r * self.n_vocab))
        return torch.tensor(lo + off[:-1], dtype=torch.int32, device=dev)


def get_beam_search_decoder(model, token_list, rnnlm=None, rnnlm_conf=None, penalty=0, ctc_weight: float = 0.1, lm_weight: float = 0.0,
                            beam_size: int = 40, scorers: Optional[dict] = None) -> BatchBeamSearch:
    """LRS/video/lightning.py:237-279.  `rnnlm`: a `lrs_lm.TransformerLM` or `lrs_lm.RNNLM`, or the path of such a model's state dict with
    `rnnlm_conf` the path of its model.json (default: next to it) or a mapping of its arguments — its `model_module` picks the class as in
    the reference: absent or "default" is the recurrent LM, "transformer" the transformer LM.  It scores under "lm" with weight `lm_weight`
    (and is dropped when that is 0, beam_search.py:73-76).  The reference's sequential RNN LM (seq_rnn) is not part of this package."""
    sos = eos = model.odim - 1
    scorers = dict(scorers) if scorers is not None else model.scorers()
    if not rnnlm:
        lm = None
    else:
        from .lrs_lm import load_lm

        lm = load_lm(len(token_list), rnnlm, rnnlm_conf)
        lm.beam_hint = int(beam_size)
    scorers["lm"] = lm
    scorers["length_bonus"] = LengthBonus(len(token_list))
    weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": lm_weight, "length_bonus": penalty}
    return BatchBeamSearch(beam_size=beam_size, vocab_size=len(token_list), weights=weights, scorers=scorers, sos=sos, eos=eos,
                           token_list=token_list, pre_beam_score_key=None if ctc_weight == 1.0 else "decoder")


def decode_clips(model, search: BatchBeamSearch, clips: torch.Tensor, lengths) -> list:
    """The batched twin of `ModelModule.forward` (LRS/video/lightning.py:98-106) up to the token ids: clips [C, Tmax, 1, H, W] padded
    along T, lengths [C] -> per clip the n-best list of `search.forward_clips` over `model.encoder(clips, masks)`."""
    if clips.dim() != 5 or clips.size(2) != 1:
        raise ValueError("clips must be [C, Tmax, 1, H, W]")
    C, Tmax = clips.shape[:2]
    lens = torch.as_tensor(lengths, dtype=torch.int64).to(clips.device)
    if lens.numel() != C or int(lens.min()) < 1 or int(lens.max()) > Tmax:
        raise ValueError(f"lengths must be {C} values in [1, {Tmax}]")
    masks = (torch.arange(Tmax, device=clips.device).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1)          # [C, 1, Tmax], make_non_pad_mask
    enc, _ = model.encoder(clips, masks)
    return search.forward_clips(enc, lens.tolist())
