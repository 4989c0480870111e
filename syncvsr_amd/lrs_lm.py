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
    def from_files(cls, n_vocab: int, rnnlm: str, rnnlm_conf: Any = None) -> "TransformerLM":
        """`rnnlm`: path of a state dict (or of a snapshot holding it under "model", asr_utils.py torch_load); `rnnlm_conf`: path of the
        reference's model.json (default: next to `rnnlm`, asr_utils.py:678-703), or a mapping / Namespace of the arguments."""
        import os

        if rnnlm_conf is None:
            rnnlm_conf = os.path.join(os.path.dirname(str(rnnlm)), "model.json")
        if isinstance(rnnlm_conf, (str, os.PathLike)):
            with open(rnnlm_conf, "rb") as f:
                conf = json.load(f)
            if not isinstance(conf, dict):
                raise ValueError(f"{rnnlm_conf} is not a language-model config (a JSON object of arguments)")
        else:
            conf = dict(rnnlm_conf) if isinstance(rnnlm_conf, Mapping) else dict(vars(rnnlm_conf))
        module = conf.get("model_module", "default")                 # lightning.py:255
        if module not in TRANSFORMER_LM_MODULES:
            raise NotImplementedError(f"language model module {module!r} is not part of this package: only the transformer LM "
                                      f"({TRANSFORMER_LM_MODULES[0]!r}) is; the reference's RNN language models stay outside")
        lm = cls(n_vocab, conf)
        sd = torch.load(rnnlm, map_location="cpu", weights_only=True)
        if isinstance(sd, Mapping) and "model" in sd and isinstance(sd["model"], Mapping):
            sd = sd["model"]
        lm.load_state_dict(sd, strict=True)
        return lm

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


def load_lm(n_vocab: int, rnnlm: Any, rnnlm_conf: Any = None) -> TransformerLM:
    """What `get_beam_search_decoder(rnnlm=, rnnlm_conf=)` accepts -> an eval-mode TransformerLM."""
    if isinstance(rnnlm, TransformerLM):
        if rnnlm.n_vocab != n_vocab:
            raise ValueError(f"the language model scores {rnnlm.n_vocab} units, the token list has {n_vocab}")
        return rnnlm
    if isinstance(rnnlm, nn.Module) or hasattr(rnnlm, "batch_score"):
        raise NotImplementedError(f"language-model scorer {type(rnnlm).__name__} is not part of this package: pass a syncvsr_amd.lrs_lm.TransformerLM, "
                                  "or the path of a transformer-LM state dict")
    return TransformerLM.from_files(n_vocab, rnnlm, rnnlm_conf)
