"""Transformer language model as a beam-search scorer (shallow fusion): the `rnnlm=` / `lm_weight=` arguments of
`get_beam_search_decoder` (LRS/video/lightning.py:237-279).

Restates `TransformerLM` of the reference (LRS/video/espnet/nets/pytorch_backend/lm/transformer.py): `nn.Embedding(n_vocab, embed_unit)`
-> `Encoder(input_layer="linear")` (transformer/encoder.py:143-150: Linear -> torch LayerNorm (eps 1e-5) -> ReLU -> x * sqrt(att_unit) + pe)
-> N pre-LN blocks (norm_mha -> MultiHeadedAttention -> + ; norm_ff -> ReLU feed-forward -> +; encoder_layer.py:98-137) -> after_norm
-> `Linear(att_unit, n_vocab)`, with the key mask `ys != 0` AND causal (lm/transformer.py:135-138).  Frozen and inference only, in the
style of `Wav2Vec2Codec`: weights are buffers under the reference's state-dict names, their device forms (bf16 matrices, fused q|k|v)
are made once per device.

State of a running search — what makes a beam step O(1) in copied bytes:

  * one POOL per layer: bf16 rows `q | k | v` [capacity, 3 * att_unit], append-only, shared by every hypothesis of the search.  The
    fused q|k|v projection of a step writes its n new rows straight behind the used part; no row is written twice;
  * one ROW TABLE int32 [n, L] for the hypothesis set: entry (b, p) names the pool row that holds position p of hypothesis b (the
    same row index in every layer's pool).  A token 0 is stored as -row - 2: still a query, never a key (include/syncvsr_hip.h).

`select_states(states, prev, tok)` gathers the table only (n * L ints).  Attention reads keys and values through the table
(svsr_mha_table_fwd), so neither they nor any layer output are copied again — the reference re-stacks per-hypothesis caches of all
layer outputs and re-projects keys / values of the whole prefix every step (lm/transformer.py:224-250, encoder.py:311-316).
"""
from __future__ import annotations

import json
import math
from typing import Any, Mapping, Optional

import torch
import torch.nn as nn

from . import ops
from .audio_codec import _Buffers
from .lrs_model import LN_EPS, _sinusoid

BF16 = torch.bfloat16
EMBED_LN_EPS = 1e-5              # torch.nn.LayerNorm of the input layer (encoder.py:146); the blocks use ESPnet's LayerNorm (1e-12)
TRANSFORMER_LM_MODULES = ("transformer", "espnet.nets.pytorch_backend.lm.transformer:TransformerLM")      # lm_interface.py:61-66


def _arg(args: Any, key: str, default=None):
    if isinstance(args, Mapping):
        return args.get(key, default)
    return getattr(args, key, default)


class LMPool:
    """The per-layer q | k | v row pools of ONE search.  `reserve(rows)` hands out the next rows (same indices in every layer); the
    capacity doubles (one copy of the used part) when a caller outruns what `batch_init_state` sized."""

    def __init__(self, layers: int, width: int, capacity: int, device):
        self.width, self.used = int(width), 0
        self.bufs = [torch.empty((max(int(capacity), 1), self.width), dtype=BF16, device=device) for _ in range(layers)]
        self.grown = 0

    @property
    def capacity(self) -> int:
        return self.bufs[0].shape[0]

    def reserve(self, rows: int) -> int:
        base = self.used
        if base + rows > self.capacity:
            cap = self.capacity
            while cap < base + rows:
                cap *= 2
            for i, old in enumerate(self.bufs):
                new = torch.empty((cap, self.width), dtype=BF16, device=old.device)
                new[:base].copy_(old[:base])
                self.bufs[i] = new
            self.grown += 1
        self.used = base + rows
        return base

    def nbytes(self) -> int:
        return sum(b.numel() * 2 for b in self.bufs)


class LMState:
    """Batched scorer state: the shared pool + the row table [n, L] of the n hypotheses (or [L]: one hypothesis).  Indexing gathers
    table rows — that is all `select_states` and the search's own pruning ever move."""

    __slots__ = ("pool", "table")

    def __init__(self, pool: LMPool, table: torch.Tensor):
        self.pool, self.table = pool, table

    def __getitem__(self, idx) -> "LMState":
        return LMState(self.pool, self.table[idx])

    def __len__(self) -> int:
        return self.table.shape[0]


def table_entries(rows: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """Row-table entries (int32) of pool rows `rows` holding `tokens`: the row, or -row - 2 for token 0 (a query, never a key)."""
    rows = rows.to(torch.int32)
    return torch.where(tokens != 0, rows, -rows - 2)


def extend_table(table: Optional[torch.Tensor], ys: torch.Tensor, base: int) -> torch.Tensor:
    """The bookkeeping of one scoring call, device-agnostic: ys int64 [n, L]; table None -> prefix pass, rows base + b * L + p for
    every position; table int32 [n, L - 1] -> step, rows base + b for the last position, appended as a new column."""
    n, L = ys.shape
    if table is None:
        rows = base + torch.arange(n * L, device=ys.device).view(n, L)
        return table_entries(rows, ys).contiguous()
    if table.shape != (n, L - 1):
        raise ValueError(f"the language-model state holds a row table of shape {tuple(table.shape)}, expected ({n}, {L - 1}): the state must come "
                         "from the previous scoring call (through select_states) for the same hypotheses")
    rows = base + torch.arange(n, device=ys.device)
    return torch.cat((table, table_entries(rows, ys[:, -1]).unsqueeze(1)), dim=1).contiguous()


class TransformerLM(nn.Module):
    """`TransformerLM(n_vocab, args)` of the reference: args.layer / unit / att_unit / embed_unit / head / pos_enc (+ dropout rates, accepted
    and ignored: evaluation only; tie_weights).  `args` is a Namespace or a mapping."""

    def __init__(self, n_vocab: int, args: Any):
        super().__init__()
        self.n_vocab = int(n_vocab)
        self.layers, self.unit = int(_arg(args, "layer", 4)), int(_arg(args, "unit", 1024))
        self.att_unit, self.embed_unit = int(_arg(args, "att_unit", 256)), int(_arg(args, "embed_unit", 128))
        self.head = int(_arg(args, "head", 2))
        pos_enc = _arg(args, "pos_enc", "sinusoidal")
        self.tie_weights = bool(_arg(args, "tie_weights", False))
        if pos_enc == "none":
            raise NotImplementedError("pos_enc='none' is not supported: the scorer adds the sinusoidal table in its input-layer kernel")
        if pos_enc != "sinusoidal":
            raise ValueError(f"unknown pos-enc option: {pos_enc}")
        if self.head < 1 or self.att_unit != self.head * 64:
            raise NotImplementedError(f"att_unit / head must be 64 (the attention kernels of this package are 64 wide per head), got "
                                      f"{self.att_unit} / {self.head}")
        if self.embed_unit % 64 != 0 or self.unit % 64 != 0 or self.embed_unit < 64 or self.unit < 64:
            raise NotImplementedError(f"embed_unit and unit must be multiples of 64 (the contraction kernels read 64 channels per step), got "
                                      f"{self.embed_unit} and {self.unit}")
        if self.att_unit > 2048:
            raise NotImplementedError("att_unit above 2048 is not supported by the LayerNorm kernels")
        if self.tie_weights and self.att_unit != self.embed_unit:
            raise ValueError("Tie Weights: True need embedding and final dimensions to match")
        if self.layers < 1 or self.n_vocab < 2:
            raise ValueError("the language model needs at least one layer and two vocabulary units")
        V, E, D, U = self.n_vocab, self.embed_unit, self.att_unit, self.unit
        g = torch.Generator().manual_seed(0)

        def lin(n_out: int, n_in: int) -> _Buffers:
            b = 1.0 / math.sqrt(n_in)
            return _Buffers(weight=(torch.rand(n_out, n_in, generator=g) * 2 - 1) * b, bias=(torch.rand(n_out, generator=g) * 2 - 1) * b)

        def norm() -> _Buffers:
            return _Buffers(weight=torch.ones(D), bias=torch.zeros(D))

        self.embed = _Buffers(weight=torch.randn(V, E, generator=g))
        self.encoder = nn.Module()
        self.encoder.embed = nn.ModuleList([lin(D, E), norm()])          # Sequential(Linear, LayerNorm, Dropout, ReLU, PositionalEncoding): entries 0, 1 hold tensors
        blocks = []
        for _ in range(self.layers):
            blk = nn.Module()
            blk.self_attn = nn.Module()
            for k in ("linear_q", "linear_k", "linear_v", "linear_out"):
                setattr(blk.self_attn, k, lin(D, D))
            blk.feed_forward = nn.Module()
            blk.feed_forward.w_1, blk.feed_forward.w_2 = lin(U, D), lin(D, U)
            blk.norm_ff, blk.norm_mha = norm(), norm()            # (the reference registers norm_ff first: state-dict order)
            blocks.append(blk)
        self.encoder.encoders = nn.ModuleList(blocks)
        self.encoder.after_norm = norm()
        self.decoder = lin(V, D)
        if self.tie_weights:
            self.decoder.weight = self.embed.weight
        self.encoder._register_load_state_dict_pre_hook(_rename_legacy_keys)
        self._packed: Optional[dict] = None
        self.beam_hint = 40                        # hypotheses batch_init_state sizes the pools for (lightning.py:245 default beam)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())
        self.requires_grad_(False)
        self.eval()

    # -- construction from files ------------------------------------------------------------------------------------------
    @classmethod
    def from_files(cls, n_vocab: int, rnnlm: str, rnnlm_conf: Any = None) -> "TransformerLM | RNNLM":
        """The language model of a state-dict file and its model.json: `lm_from_files`, which picks the class by the config's `model_module`
        as the reference does (a config without one names the recurrent LM)."""
        return lm_from_files(n_vocab, rnnlm, rnnlm_conf)

    # -- device forms -----------------------------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("TransformerLM is a frozen, inference-only scorer: training the language model is outside this package")
        return super().train(False)

    def _invalidate(self) -> None:
        self._packed = None

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._packed = None
        return out

    def packed(self, dev: torch.device) -> dict:
        """bf16 matrices ([N, K], nn.Linear layout; q|k|v fused to [3D, D]) and fp32 vectors on `dev`, made once."""
        p = self._packed
        if p is not None and p["dev"] == dev:
            return p

        def w16(t):
            return t.detach().to(dev, torch.float32).to(BF16).contiguous()

        def f32(t):
            return t.detach().to(dev, torch.float32).contiguous()

        with torch.no_grad():
            e = self.encoder
            p = dict(dev=dev, emb=w16(self.embed.weight), w_in=w16(e.embed[0].weight), b_in=f32(e.embed[0].bias), g_in=f32(e.embed[1].weight),
                     be_in=f32(e.embed[1].bias), g_out=f32(e.after_norm.weight), be_out=f32(e.after_norm.bias), w_dec=w16(self.decoder.weight),
                     b_dec=f32(self.decoder.bias), layers=[], pe=None)
            for blk in e.encoders:
                a, ff = blk.self_attn, blk.feed_forward
                p["layers"].append(dict(
                    g1=f32(blk.norm_mha.weight), be1=f32(blk.norm_mha.bias), g2=f32(blk.norm_ff.weight), be2=f32(blk.norm_ff.bias),
                    wqkv=w16(torch.cat((a.linear_q.weight, a.linear_k.weight, a.linear_v.weight), 0)),
                    bqkv=f32(torch.cat((a.linear_q.bias, a.linear_k.bias, a.linear_v.bias), 0)),
                    wo=w16(a.linear_out.weight), bo=f32(a.linear_out.bias), w1=w16(ff.w_1.weight), b1=f32(ff.w_1.bias), w2=w16(ff.w_2.weight),
                    b2=f32(ff.w_2.bias)))
        self._packed = p
        return p

    def _pe(self, p: dict, L: int) -> torch.Tensor:
        if p["pe"] is None or p["pe"].shape[0] < L:
            rows = max(256, 2 * L)
            p["pe"] = _sinusoid(torch.arange(rows), self.att_unit).to(p["dev"]).contiguous()
        return p["pe"]

    # -- the network over R new rows --------------------------------------------------------------------------------------
    def _rows(self, p: dict, pool: LMPool, base: int, table: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, n: int, Lq: int, L: int) -> torch.Tensor:
        """tok int64 [R], pos int32 [R] (R = n * Lq new rows, pool rows base .. base + R - 1 already reserved) -> block-stack output bf16 [R, D]."""
        D, E, U, H = self.att_unit, self.embed_unit, self.unit, self.head
        R = n * Lq
        e = p["emb"].index_select(0, tok)
        lin = ops.linear_fwd(e, p["w_in"], p["b_in"], rows=R, K=E, N=D, x_pitch=E)[0]
        x = ops.lm_embed_fwd(lin, p["g_in"], p["be_in"], self._pe(p, L), pos, D, EMBED_LN_EPS, math.sqrt(D))
        for i, w in enumerate(p["layers"]):
            t1 = ops.add_ln_fwd(x, None, w["g1"], w["be1"], LN_EPS)[0]
            buf = pool.bufs[i]
            ops.linear_fwd(t1, w["wqkv"], w["bqkv"], rows=R, K=D, N=3 * D, x_pitch=D, out=buf[base : base + R], out_pitch=3 * D)      # straight into the pool
            ctx = ops.mha_table_fwd(buf, table, n=n, Lq=Lq, L=L, H=H, scale=1.0 / 8.0, pool_rows=pool.used)
            x1 = ops.linear_fwd(ctx, w["wo"], w["bo"], rows=R, K=D, N=D, x_pitch=D, addend=x)[0]
            t2 = ops.add_ln_fwd(x1, None, w["g2"], w["be2"], LN_EPS)[0]
            h = ops.linear_fwd(t2, w["w1"], w["b1"], rows=R, K=D, N=U, x_pitch=D, relu=True)[0]
            x = ops.linear_fwd(h, w["w2"], w["b2"], rows=R, K=U, N=D, x_pitch=U, addend=x1)[0]
        return x

    def _logits(self, p: dict, x: torch.Tensor, R: int) -> torch.Tensor:
        """after_norm + output layer over R rows -> fp32 [R, n_vocab]."""
        D, V = self.att_unit, self.n_vocab
        tn = ops.add_ln_fwd(x, None, p["g_out"], p["be_out"], LN_EPS)[0]
        Vp = (V + 63) // 64 * 64
        return ops.linear_fwd(tn, p["w_dec"], p["b_dec"], rows=R, K=D, N=V, x_pitch=D, out_f32=True, out_pitch=Vp)[0][:, :V]

    def _check(self, ys: torch.Tensor) -> dict:
        if self.training:
            raise RuntimeError("TransformerLM scores in eval mode only")
        if ys.device.type != "cuda":
            raise RuntimeError("syncvsr_amd runs on an MI355X HIP device only; there is no CPU fallback (tests/lm_restatement.py is the fp64 restatement)")
        return self.packed(ys.device)

    # -- scorer interface (scorer_interface.py; lm/transformer.py:176-250) ----------------------------------------------------
    def init_state(self, x):
        return None

    def batch_init_state(self, x, beam: Optional[int] = None, maxlen: Optional[int] = None):
        """A fresh pool sized for `beam` hypotheses (default: `self.beam_hint`, which get_beam_search_decoder sets to its beam size) over
        `maxlen` positions (default: the clip's frames, the search's length limit, beam_search.py:351-356) — returned inside an empty
        state so that the first `batch_score` appends to it.  A search that outruns it grows the pool by doubling."""
        beam = self.beam_hint if beam is None else int(beam)
        maxlen = int(x.shape[0]) if maxlen is None else int(maxlen)
        pool = LMPool(self.layers, 3 * self.att_unit, beam * (maxlen + 1), x.device)
        return LMState(pool, torch.empty((0, 0), dtype=torch.int32, device=x.device))

    # -- clip-aware protocol (BatchBeamSearch.forward_clips): the language model does not look at the clip; rows are rows ---------------
    def batch_init_state_clips(self, xs, lengths):
        """One pool for the C clips of a multi-clip search: `beam_hint` rows per clip over the longest clip's positions."""
        lens = [int(v) for v in lengths]
        return self.batch_init_state(xs[0], beam=self.beam_hint * len(lens), maxlen=max(lens))

    def batch_score_clips(self, ys: torch.Tensor, states, clip_of: torch.Tensor = None):
        return self.batch_score(ys, states, None)

    def workspace_bytes(self, beam: int, maxlen: int) -> int:
        """Device bytes of the state of one search: the pools `batch_init_state(beam=, maxlen=)` sizes + the row table."""
        return self.layers * beam * (maxlen + 1) * 3 * self.att_unit * 2 + beam * (maxlen + 1) * 4

    def select_state(self, state, i, new_id=None):
        return None if state is None else state[i]

    def select_states(self, states, prev: torch.Tensor, tok: torch.Tensor):
        return None if states is None else states[prev]

    def _merge(self, states, n: int, L: int, dev):
        """-> (pool, table [n, L-1] | None).  Accepts None, [None] * n, an empty state from batch_init_state, the batched state, or a list of
        per-hypothesis states of one pool (the reference's calling convention)."""
        if isinstance(states, (list, tuple)):
            if not states or any(s is None for s in states):
                return None, None
            pool = states[0].pool
            if any(s.pool is not pool for s in states) or any(s.table.dim() != 1 or s.table.numel() != L - 1 for s in states):
                return None, None                      # states of different searches cannot share rows: score the prefixes again
            return pool, torch.stack([s.table for s in states])
        if states is None:
            return None, None
        if states.table.numel() == 0 and states.table.shape[0] == 0:
            return states.pool, None                   # fresh from batch_init_state
        return states.pool, states.table

    def batch_score(self, ys: torch.Tensor, states, xs: torch.Tensor = None):
        """ys int64 [n, L] prefixes (with <sos>) -> (log-probabilities of the next token fp32 [n, n_vocab], state)."""
        p = self._check(ys)
        n, L = ys.shape
        pool, table = self._merge(states, n, L, ys.device)
        if pool is None:
            pool = LMPool(self.layers, 3 * self.att_unit, max(n * L * 2, 64), ys.device)
        with torch.no_grad():
            if table is None:
                base = pool.reserve(n * L)
                table = extend_table(None, ys, base)
                pos = torch.arange(L, dtype=torch.int32, device=ys.device).repeat(n)
                x = self._rows(p, pool, base, table, ys.reshape(-1), pos, n, L, L)
                x = x.view(n, L, self.att_unit)[:, -1].contiguous()
            else:
                base = pool.reserve(n)
                table = extend_table(table, ys, base)
                pos = torch.full((n,), L - 1, dtype=torch.int32, device=ys.device)
                x = self._rows(p, pool, base, table, ys[:, -1].contiguous(), pos, n, 1, L)
            logp = torch.log_softmax(self._logits(p, x, n).float(), dim=-1)
        return logp, LMState(pool, table)

    def score(self, y: torch.Tensor, state, x: torch.Tensor = None):
        logp, st = self.batch_score(y.unsqueeze(0), None if state is None else [state], None)
        return logp.squeeze(0), st[0]

    # -- perplexity evaluation (lm/transformer.py:140-174) ----------------------------------------------------------------------
    def forward(self, x: torch.Tensor, t: torch.Tensor):
        """x, t int64 [B, L] -> (nll / count, nll, count) with nll = -sum log p(t | x) over positions where x != 0.  Forward only."""
        p = self._check(x)
        B, L = x.shape
        with torch.no_grad():
            pool = LMPool(self.layers, 3 * self.att_unit, B * L, x.device)
            base = pool.reserve(B * L)
            table = extend_table(None, x, base)
            pos = torch.arange(L, dtype=torch.int32, device=x.device).repeat(B)
            h = self._rows(p, pool, base, table, x.reshape(-1), pos, B, L, L)
            logp = torch.log_softmax(self._logits(p, h, B * L).float(), dim=-1)
            loss = -logp.gather(1, t.reshape(-1, 1)).squeeze(1)
            mask = (x != 0).reshape(-1).to(loss.dtype)
            nll, count = (loss * mask).sum(), mask.sum()
        return nll / count, nll, count


def _rename_legacy_keys(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    """transformer/encoder.py:47-59: checkpoints older than ESPnet 0.5 name the input layer `input_layer.` and the final norm `norm.`."""
    for old, new in ((prefix + "input_layer.", prefix + "embed."), (prefix + "norm.", prefix + "after_norm.")):
        for k in [k for k in state_dict if k.startswith(old)]:
            state_dict[new + k[len(old):]] = state_dict.pop(k)


# ======================================================================================================================
# Recurrent language model: the reference's default (lm_interface.py: model_module "default" -> lm/default.py DefaultRNNLM)
# ======================================================================================================================
RNN_PAD = 64                     # embed_unit and unit are zero-padded to this at pack time (svsr_rnn_cell_step's K / N step)
RNN_MAX_DIM = 4096               # padded width svsr_rnn_cell_step takes


def _pad_to(n: int, m: int = RNN_PAD) -> int:
    return (int(n) + m - 1) // m * m


def pack_rnn_cell(w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor, gru: bool):
    """nn.LSTMCell / nn.GRUCell tensors (w_ih [G U, E], w_hh [G U, U], biases [G U]; G = 4: i, f, g, o | 3: r, z, n) -> what
    svsr_rnn_cell_step reads: wpk bf16 [Up / 16, (Ep + Up) / 32, G, 64, 8] — per 16-unit tile and 32-wide k-step the MFMA B fragment of EVERY
    gate, lane l holding W_g[16 t + (l & 15)][32 s + 8 (l >> 4) + j] of W_g = [W_ih,g | W_hh,g] zero-padded to [Up, Ep + Up] — and bias fp32
    [Up / 16, 4, 16]: LSTM b_ih + b_hh per gate; GRU r, z summed, then b_in and b_hn apart (b_hn sits inside r * (.))."""
    G = 3 if gru else 4
    U, E = int(w_hh.shape[1]), int(w_ih.shape[1])
    if w_ih.shape[0] != G * U or w_hh.shape[0] != G * U or b_ih.numel() != G * U or b_hh.numel() != G * U:
        raise ValueError(f"cell tensors of shapes {tuple(w_ih.shape)}, {tuple(w_hh.shape)} are not those of a {'GRU' if gru else 'LSTM'} cell")
    Ep, Up = _pad_to(E), _pad_to(U)
    W = torch.zeros((G, Up, Ep + Up), dtype=torch.float32, device=w_ih.device)
    W[:, :U, :E] = w_ih.detach().float().view(G, U, E)
    W[:, :U, Ep : Ep + U] = w_hh.detach().float().view(G, U, U)
    T, KS = Up // 16, (Ep + Up) // 32
    wpk = W.to(BF16).view(G, T, 16, KS, 4, 8).permute(1, 3, 0, 4, 2, 5).reshape(T, KS, G, 64, 8).contiguous()
    bi, bh = b_ih.detach().float().view(G, U), b_hh.detach().float().view(G, U)
    b4 = torch.zeros((4, Up), dtype=torch.float32, device=w_ih.device)
    if gru:
        b4[0, :U], b4[1, :U], b4[2, :U], b4[3, :U] = bi[0] + bh[0], bi[1] + bh[1], bi[2], bh[2]
    else:
        b4[:, :U] = bi + bh
    return wpk, b4.view(4, T, 16).permute(1, 0, 2).contiguous()


def unpack_rnn_cell(wpk: torch.Tensor, bias: torch.Tensor, E: int, U: int, gru: bool):
    """Inverse of pack_rnn_cell -> (w_ih [G U, E], w_hh [G U, U] as fp32 of the bf16 values, the four bias rows [4, U], the padding [G, Up, Ep + Up]
    with the real entries zeroed: all zeros for a well-formed pack)."""
    G = 3 if gru else 4
    Ep, Up = _pad_to(E), _pad_to(U)
    T, KS = Up // 16, (Ep + Up) // 32
    W = wpk.float().view(T, KS, G, 4, 16, 8).permute(2, 0, 4, 1, 3, 5).reshape(G, Up, Ep + Up)
    w_ih, w_hh = W[:, :U, :E].reshape(G * U, E).clone(), W[:, :U, Ep : Ep + U].reshape(G * U, U).clone()
    rest = W.clone()
    rest[:, :U, :E] = 0
    rest[:, :U, Ep : Ep + U] = 0
    return w_ih, w_hh, bias.view(T, 4, 16).permute(1, 0, 2).reshape(4, Up)[:, :U].clone(), rest


class RNNBuffers:
    """The state rows of ONE search: fp32 h (and c: LSTM) as a ping-pong pair [2, layers, capacity, Up], plus the bf16 copy of the step's h
    [layers, capacity, Up] that the layer above and the output projection read.  A step reads side `parity` through the parent rows of the
    last selection and writes the other side; `gen` counts the steps written here."""

    def __init__(self, layers: int, capacity: int, width: int, lstm: bool, device):
        self.capacity = max(int(capacity), 1)
        self.h = torch.empty((2, layers, self.capacity, width), dtype=torch.float32, device=device)
        self.c = torch.empty_like(self.h) if lstm else None
        self.h16 = torch.empty((layers, self.capacity, width), dtype=BF16, device=device)
        self.iota = torch.arange(self.capacity, dtype=torch.int64, device=device)
        self.parity, self.gen = 1, 0

    def nbytes(self) -> int:
        return (self.h.numel() * (2 if self.c is not None else 1)) * 4 + self.h16.numel() * 2 + self.iota.numel() * 8


class RNNState:
    """Batched scorer state: the buffers of the search + the int64 rows [n] (or one row, 0-dim) that hold the n hypotheses' states on side
    `parity`, as written by step `gen`.  rows None: no step yet (zero state).  Indexing gathers the rows — n integers are all that
    `select_states` and the search's pruning move; the next step's kernels read the state rows through them."""

    __slots__ = ("bufs", "rows", "parity", "gen")

    def __init__(self, bufs: RNNBuffers, rows: Optional[torch.Tensor], parity: int, gen: int):
        self.bufs, self.rows, self.parity, self.gen = bufs, rows, parity, gen

    def __getitem__(self, idx) -> "RNNState":
        return RNNState(self.bufs, None if self.rows is None else self.rows[idx], self.parity, self.gen)

    def __len__(self) -> int:
        return 0 if self.rows is None else self.rows.shape[0]


def select_rows(rows: Optional[torch.Tensor], prev: torch.Tensor) -> Optional[torch.Tensor]:
    """Index arithmetic of `select_states`, device-agnostic: rows [n] name the state rows of the n scored hypotheses, prev [m] the parent of
    each survivor -> rows [m] of the survivors' states (None stays None: nothing was scored yet)."""
    return None if rows is None else rows[prev]


class RNNLM(nn.Module):
    """`DefaultRNNLM(n_vocab, args)` of the reference (lm/default.py): args.type ("lstm" | "gru"), layer, unit, embed_unit (None: unit),
    tie_weights (+ dropout_rate / emb_dropout_rate, accepted and ignored: evaluation only).  nn.Embedding -> `layer` nn.LSTMCell / nn.GRUCell
    -> nn.Linear(unit, n_vocab), weights as frozen buffers under the reference's state-dict names (`predictor.*`).  A step is one
    svsr_rnn_cell_step launch per layer + the output projection + log-softmax; the state of a search lives in `RNNBuffers`."""

    def __init__(self, n_vocab: int, args: Any):
        super().__init__()
        self.n_vocab = int(n_vocab)
        self.typ = str(_arg(args, "type", "lstm"))
        self.layers, self.unit = int(_arg(args, "layer", 2)), int(_arg(args, "unit", 650))
        eu = _arg(args, "embed_unit", None)
        self.embed_unit = self.unit if eu is None else int(eu)
        self.tie_weights = bool(_arg(args, "tie_weights", False))
        if self.typ not in ("lstm", "gru"):
            raise ValueError(f"unknown RNN type: {self.typ!r} (lstm or gru)")
        if self.layers < 1 or self.n_vocab < 2 or self.unit < 1 or self.embed_unit < 1:
            raise ValueError("the language model needs at least one layer, one unit and two vocabulary units")
        if self.tie_weights and self.unit != self.embed_unit:
            raise ValueError("Tie Weights: True need embedding and final dimensions to match")
        bad = [f"{k} = {v} pads to {_pad_to(v)}" for k, v in (("unit", self.unit), ("embed_unit", self.embed_unit)) if _pad_to(v) > RNN_MAX_DIM]
        if bad:
            raise NotImplementedError(f"the recurrent-cell kernel takes widths up to {RNN_MAX_DIM} after padding to multiples of {RNN_PAD}: " + "; ".join(bad))
        V, E, U, G = self.n_vocab, self.embed_unit, self.unit, (4 if self.typ == "lstm" else 3)
        g = torch.Generator().manual_seed(0)

        def uni(*shape) -> torch.Tensor:                       # default.py:388-389: every parameter uniform in [-0.1, 0.1]
            return (torch.rand(*shape, generator=g) * 2 - 1) * 0.1

        self.predictor = nn.Module()
        self.predictor.embed = _Buffers(weight=uni(V, E))
        self.predictor.rnn = nn.ModuleList([_Buffers(weight_ih=uni(G * U, E if i == 0 else U), weight_hh=uni(G * U, U), bias_ih=uni(G * U), bias_hh=uni(G * U))
                                            for i in range(self.layers)])
        self.predictor.lo = _Buffers(weight=uni(V, U), bias=uni(V))
        if self.tie_weights:
            self.predictor.lo.weight = self.predictor.embed.weight
        self._packed: Optional[dict] = None
        self.beam_hint = 40
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())
        self.requires_grad_(False)
        self.eval()

    @property
    def lstm(self) -> bool:
        return self.typ == "lstm"

    @property
    def unit_pad(self) -> int:
        return _pad_to(self.unit)

    @property
    def embed_pad(self) -> int:
        return _pad_to(self.embed_unit)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("RNNLM is a frozen, inference-only scorer: training the language model is outside this package")
        return super().train(False)

    def _invalidate(self) -> None:
        self._packed = None

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._packed = None
        if self.tie_weights:                                   # (nn.Module._apply maps the shared tensor twice)
            self.predictor.lo.weight = self.predictor.embed.weight
        return out

    def packed(self, dev: torch.device) -> dict:
        """Device forms, made once: the embedding table bf16 [V, Ep] and the output matrix bf16 [V, Up] (zero-padded columns), per layer
        the gate-interleaved fragments of pack_rnn_cell."""
        p = self._packed
        if p is not None and p["dev"] == dev:
            return p
        V, E, U, Ep, Up = self.n_vocab, self.embed_unit, self.unit, self.embed_pad, self.unit_pad
        pr = self.predictor
        with torch.no_grad():
            emb = torch.zeros((V, Ep), dtype=BF16, device=dev)
            emb[:, :E] = pr.embed.weight.detach().to(dev, torch.float32).to(BF16)
            w_lo = torch.zeros((V, Up), dtype=BF16, device=dev)
            w_lo[:, :U] = pr.lo.weight.detach().to(dev, torch.float32).to(BF16)
            p = dict(dev=dev, emb=emb, w_lo=w_lo, b_lo=pr.lo.bias.detach().to(dev, torch.float32).contiguous(), layers=[])
            for cell in pr.rnn:
                p["layers"].append(pack_rnn_cell(cell.weight_ih.to(dev), cell.weight_hh.to(dev), cell.bias_ih.to(dev), cell.bias_hh.to(dev), not self.lstm))
        self._packed = p
        return p

    def _check(self, ys: torch.Tensor) -> dict:
        if self.training:
            raise RuntimeError("RNNLM scores in eval mode only")
        if ys.device.type != "cuda":
            raise RuntimeError("syncvsr_amd runs on an MI355X HIP device only; there is no CPU fallback (tests/rnnlm_restatement.py is the fp64 restatement)")
        return self.packed(ys.device)

    # -- one step over n rows --------------------------------------------------------------------------------------------------
    def _new_bufs(self, capacity: int, dev) -> RNNBuffers:
        return RNNBuffers(self.layers, capacity, self.unit_pad, self.lstm, dev)

    def _step(self, p: dict, tok: torch.Tensor, state: Optional[RNNState], n: int):
        """tok int64 [n] (any stride), state: where the parents' rows are (None / rows None: zero state) -> (logits fp32 [n, V], new state).
        Writes the other side of the state's own buffers when `state` is their latest step and they are large enough (the search's
        path: nothing is allocated or copied); otherwise fresh buffers take the result and the state's are only read."""
        Ep, Up, U, V = self.embed_pad, self.unit_pad, self.unit, self.n_vocab
        rb = state.bufs if state is not None else None
        src = state.rows if state is not None else None
        if src is not None:
            if rb.gen - state.gen > 1 or (rb.gen != state.gen and rb.parity == state.parity):
                raise ValueError("the language-model state was overwritten: it is older than the last two scoring calls of its search (a state "
                                 "is good for the scoring call after the one that made it; select_state() detaches a hypothesis for longer)")
            if src.dim() == 0:
                src = src.view(1)
            if src.numel() != n:
                raise ValueError(f"the language-model state holds {src.numel()} rows for {n} hypotheses: it must come from the previous scoring "
                                 "call (through select_states) for the same hypotheses")
            src = src.contiguous()
        if rb is not None and rb.gen == state.gen and n <= rb.capacity:
            wb, side = rb, 1 - state.parity
        else:
            wb, side = self._new_bufs(n, tok.device), 0
        rs = state.parity if state is not None else 0
        gru = not self.lstm
        for i, (wpk, bias) in enumerate(p["layers"]):
            ops.rnn_cell_step(gru, wpk, bias, p["emb"] if i == 0 else wb.h16[i - 1], tok if i == 0 else None,
                              rb.h[rs, i] if src is not None else None, rb.c[rs, i] if src is not None and self.lstm else None, src,
                              wb.h[side, i], wb.c[side, i] if self.lstm else None, wb.h16[i], R=n, Ep=Ep if i == 0 else Up, Up=Up, U=U)
        wb.parity, wb.gen = side, wb.gen + 1
        Vp = (V + 63) // 64 * 64
        logits = ops.linear_fwd(wb.h16[self.layers - 1], p["w_lo"], p["b_lo"], rows=n, K=Up, N=V, x_pitch=Up, out_f32=True, out_pitch=Vp)[0][:, :V]
        return logits, RNNState(wb, wb.iota[:n], side, wb.gen)

    # -- scorer interface (scorer_interface.py; lm/default.py:138-213) -------------------------------------------------------------
    def init_state(self, x):
        return None

    def batch_init_state(self, x, beam: Optional[int] = None, maxlen: Optional[int] = None):
        """Buffers for `beam` hypotheses (default: `self.beam_hint`, which get_beam_search_decoder sets to its beam size), inside a state
        without rows: the first `batch_score` starts from the zero state (default.py:398-406).  `maxlen` is accepted for the signature
        the transformer LM has: a recurrent state does not grow with the prefix."""
        beam = self.beam_hint if beam is None else int(beam)
        return RNNState(self._new_bufs(beam, x.device), None, 1, 0)

    def batch_init_state_clips(self, xs, lengths):
        """One pair of buffers for the C clips of a multi-clip search: `beam_hint` rows per clip."""
        return self.batch_init_state(xs[0], beam=self.beam_hint * len(list(lengths)))

    def batch_score_clips(self, ys: torch.Tensor, states, clip_of: torch.Tensor = None):
        return self.batch_score(ys, states, None)

    def workspace_bytes(self, beam: int, maxlen: int = 0) -> int:
        """Device bytes of the state of one search: what `batch_init_state(beam=)` allocates (independent of the prefix length)."""
        Up = self.unit_pad
        return self.layers * beam * Up * (2 * 4 * (2 if self.lstm else 1) + 2) + beam * 8

    def final_score(self, state) -> float:
        return 0.0                                             # default.py:316-322: the predictor has no `final`

    def select_state(self, state, i, new_id=None):
        """One hypothesis' state, detached from the search's buffers (layers * Up numbers are copied): it stays valid however many steps
        the search takes afterwards — the per-hypothesis protocol of the reference's BeamSearch keeps states for as long as it likes."""
        if state is None or state.rows is None:
            return None
        row = state.rows.reshape(-1)[i] if state.rows.dim() else state.rows
        src, own = state.bufs, self._new_bufs(1, state.bufs.h.device)
        own.h[0, :, 0] = src.h[state.parity, :, row]
        if self.lstm:
            own.c[0, :, 0] = src.c[state.parity, :, row]
        own.parity, own.gen = 0, 1
        return RNNState(own, own.iota[0], 0, 1)

    def select_states(self, states, prev: torch.Tensor, tok: torch.Tensor):
        return None if states is None else RNNState(states.bufs, select_rows(states.rows, prev), states.parity, states.gen)

    def _merge(self, states, n: int, dev) -> Optional[RNNState]:
        """Accepts None, [None] * n, the batched state, or a list of per-hypothesis states (the reference's calling convention): states of
        one step of one search share their rows' buffers; anything else is gathered into fresh buffers first."""
        if states is None:
            return None
        if isinstance(states, RNNState):
            return states
        if not states or any(s is None or s.rows is None for s in states):
            return None                                        # default.py:193: states[0] is None -> zero state
        if len(states) != n:
            raise ValueError(f"{len(states)} language-model states for {n} hypotheses")
        s0 = states[0]
        if all(s.bufs is s0.bufs and s.parity == s0.parity and s.gen == s0.gen for s in states):
            return RNNState(s0.bufs, torch.cat([s.rows.reshape(-1) for s in states]), s0.parity, s0.gen)
        own = self._new_bufs(n, dev)
        own.h[0] = torch.stack([s.bufs.h[s.parity][:, s.rows.reshape(-1)[0]] for s in states], dim=1)
        if self.lstm:
            own.c[0] = torch.stack([s.bufs.c[s.parity][:, s.rows.reshape(-1)[0]] for s in states], dim=1)
        own.parity, own.gen = 0, 1
        return RNNState(own, own.iota[:n], 0, 1)

    def batch_score(self, ys: torch.Tensor, states, xs: torch.Tensor = None):
        """ys int64 [n, L] prefixes (with <sos>) -> (log-probabilities of the next token fp32 [n, n_vocab], state).  As in the reference
        (default.py:204) only the LAST token of each prefix is read: the rest of the prefix is what the state stands for, and without a
        state the step starts from zeros."""
        p = self._check(ys)
        n = ys.shape[0]
        with torch.no_grad():
            logits, state = self._step(p, ys[:, -1], self._merge(states, n, ys.device), n)
            logp = torch.log_softmax(logits.float(), dim=-1)
        return logp, state

    def score(self, y: torch.Tensor, state, x: torch.Tensor = None):
        logp, st = self.batch_score(y.unsqueeze(0), None if state is None else [state], None)
        return logp.squeeze(0), st[0]

    # -- perplexity evaluation (default.py:106-136) ---------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, t: torch.Tensor):
        """x, t int64 [B, L] -> the reference's triple (loss / B, loss, count): loss = sum over positions i of mean_b(-log p(t[b, i])) times the
        number of rows with x[b, i] != 0, count = that number summed.  Forward only."""
        p = self._check(x)
        B, L = x.shape
        with torch.no_grad():
            state = None
            loss = torch.zeros((), dtype=torch.float32, device=x.device)
            count = torch.zeros((), dtype=torch.int64, device=x.device)
            for i in range(L):
                logits, state = self._step(p, x[:, i], state, B)
                nll = -torch.log_softmax(logits.float(), dim=-1).gather(1, t[:, i : i + 1]).squeeze(1)
                non_zeros = (x[:, i] != 0).sum()
                loss = loss + nll.mean() * non_zeros.to(nll.dtype)
                count = count + non_zeros
        return loss / B, loss, count

    @classmethod
    def from_files(cls, n_vocab: int, rnnlm: str, rnnlm_conf: Any = None):
        return load_lm(n_vocab, rnnlm, rnnlm_conf)


RNN_LM_MODULES = ("default", "espnet.nets.pytorch_backend.lm.default:DefaultRNNLM")                          # lm_interface.py:61-66
RNN_LM_REQUIRED = ("type", "layer", "unit")                      # what DefaultRNNLM.__init__ reads as args.<name>: no getattr default


def _read_conf(rnnlm: Any, rnnlm_conf: Any) -> dict:
    import os

    if rnnlm_conf is None:
        rnnlm_conf = os.path.join(os.path.dirname(str(rnnlm)), "model.json")
    if isinstance(rnnlm_conf, (str, os.PathLike)):
        with open(rnnlm_conf, "rb") as f:
            conf = json.load(f)
        if not isinstance(conf, dict):
            raise ValueError(f"{rnnlm_conf} is not a language-model config (a JSON object of arguments)")
        return conf
    return dict(rnnlm_conf) if isinstance(rnnlm_conf, Mapping) else dict(vars(rnnlm_conf))


def lm_from_files(n_vocab: int, rnnlm: str, rnnlm_conf: Any = None) -> "TransformerLM | RNNLM":
    """`rnnlm`: path of a state dict (or of a snapshot holding it under "model", asr_utils.py torch_load); `rnnlm_conf`: path of the
    reference's model.json (default: next to `rnnlm`, asr_utils.py:678-703), or a mapping / Namespace of the arguments.  The class follows
    `model_module` as in the reference (lightning.py:255, lm_interface.py:61-66): absent or "default" is the recurrent LM, "transformer" the
    transformer LM; "seq_rnn" and foreign modules are not part of this package, and a recurrent-LM config must carry `type`, `layer` and
    `unit` as the reference's does."""
    conf = _read_conf(rnnlm, rnnlm_conf)
    module = conf.get("model_module", "default")
    if module in TRANSFORMER_LM_MODULES:
        lm = TransformerLM(n_vocab, conf)
    elif module in RNN_LM_MODULES:
        # default.py:85-96 reads args.type, args.layer and args.unit without defaults, and the trainer writes every argument into model.json: a
        # config without them was not written for this module (a transformer-LM config whose model_module was lost, say) and is refused
        # here, by name, rather than by the key mismatch of the strict load below
        missing = [k for k in RNN_LM_REQUIRED if k not in conf]
        if missing:
            raise NotImplementedError(f"language model module {module!r} (the reference's recurrent LM, also what a config without model_module means) "
                                      f"cannot be built from this config: it lacks {', '.join(missing)}, which the reference's DefaultRNNLM reads "
                                      f"without defaults; a transformer LM config must say model_module={TRANSFORMER_LM_MODULES[0]!r}")
        lm = RNNLM(n_vocab, conf)
    else:
        raise NotImplementedError(f"language model module {module!r} is not part of this package: the transformer LM ({TRANSFORMER_LM_MODULES[0]!r}) and "
                                  f"the default recurrent LM ({RNN_LM_MODULES[0]!r}, also meant by a config without model_module) are; the reference's "
                                  "sequential RNN LM (seq_rnn: cuDNN-style nn.LSTM / nn.GRU / nn.RNN stacks under other state-dict names) stays outside")
    sd = torch.load(rnnlm, map_location="cpu", weights_only=True)
    if isinstance(sd, Mapping) and "model" in sd and isinstance(sd["model"], Mapping):
        sd = sd["model"]
    lm.load_state_dict(sd, strict=True)
    return lm


def load_lm(n_vocab: int, rnnlm: Any, rnnlm_conf: Any = None) -> "TransformerLM | RNNLM":
    """What `get_beam_search_decoder(rnnlm=, rnnlm_conf=)` accepts -> an eval-mode TransformerLM or RNNLM."""
    if isinstance(rnnlm, (TransformerLM, RNNLM)):
        if rnnlm.n_vocab != n_vocab:
            raise ValueError(f"the language model scores {rnnlm.n_vocab} units, the token list has {n_vocab}")
        return rnnlm
    if isinstance(rnnlm, nn.Module) or hasattr(rnnlm, "batch_score"):
        raise NotImplementedError(f"language-model scorer {type(rnnlm).__name__} is not part of this package: pass a syncvsr_amd.lrs_lm.TransformerLM "
                                  "or RNNLM, or the path of such a model's state dict")
    return lm_from_files(n_vocab, rnnlm, rnnlm_conf)
