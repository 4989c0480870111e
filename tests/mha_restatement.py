"""Plain-torch float64 restatement of the attention kernels of syncvsr_amd/csrc/mha.hip (mha_coop.h per tile, mha_flash.h streamed keys), the
cases tests/test_gpu_mha_edges.py runs them at, and the per-row error metric with its tolerances.

The function follows oracle/lrs_oracle.py (_attend, rel_mha): scores[i,j] = ((q_i+u)·k_j + (q_i+v)·pe[T-1+j-i]) / 8, masked positions set to
-1e10 before the softmax and to 0 after it — a query with no live key therefore gets a zero ctx row (and zero gradients).

rounded=False is the reference: float64 throughout, gradients by autograd.  rounded=True restates where the kernels round to bf16 (nothing
else: not their fp32 accumulation order, not __expf / __logf, not the online-softmax rescaling), with the backward written out by hand:
  q+u, q+v                      add_bias_frag (forward, query pass) and the pack8 of the key / table passes: fp32 sum -> bf16
  P before P·V                  f32row_frag (per tile), mf_pack_swap (flash); the stored probabilities the key pass reads are the same bf16
  ctx                           output; the flash backward reads it back for D_i = dctx_i·ctx_i
  dS                            per tile: bf16(P) ∘ (dP - rowsum(bf16(P) ∘ dP)) / 8;  flash: P ∘ (dP - dctx·bf16(ctx)) / 8 with P in fp32;
                                rounded to bf16 before dS·K, dS_skewed·PE, dS^T·(q+u) and the table pass
  dq, dq_ac, dq_bd, dk, dv, dpe outputs (dq = bf16(dq_ac + dq_bd) from the unrounded summands)
The flash forward rounds exp(s - running max) rather than the normalised probability; both are one bf16 rounding of P's numerator, and the
restatement rounds the normalised one.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import torch

BF = torch.bfloat16
F64 = torch.float64
NEG = -1e10
DH = 64
H = 2
TENSORS = ("ctx", "probs", "lse", "dq", "dk", "dv", "dq_ac", "dq_bd", "dpe")


def _bf(x: torch.Tensor) -> torch.Tensor:
    """fp32 value -> bf16, as the kernels' f2bf does, back in float64"""
    return x.float().to(BF).to(F64)


def live_mask(B: int, Lq: int, Lk: int, klen, causal: bool) -> torch.Tensor:
    """[B, 1, Lq, Lk] bool: key j is live for query i of clip b"""
    m = torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    if klen is not None:
        m = m & (torch.arange(Lk).view(1, 1, 1, Lk) < torch.as_tensor(klen).view(B, 1, 1, 1))
    if causal:
        m = m & torch.tril(torch.ones(Lq, Lk, dtype=torch.bool)).view(1, 1, Lq, Lk)
    return m


def _skew_index(T: int) -> torch.Tensor:
    return (T - 1) + torch.arange(T).view(1, T) - torch.arange(T).view(T, 1)


def scores_of(qu, qv, k, pe, scale):
    """qu, qv [B, Lq, H, 64] (qv, pe None: no relative-position term), k [B, Lk, H, 64], pe [2T-1, H, 64] -> [B, H, Lq, Lk]"""
    ac = torch.matmul(qu.transpose(1, 2), k.permute(0, 2, 3, 1))
    if pe is None:
        return ac * scale
    B, T = qu.shape[0], qu.shape[1]
    bd_full = torch.matmul(qv.transpose(1, 2), pe.permute(1, 2, 0))                 # [B, H, T, 2T-1]
    bd = bd_full.gather(-1, _skew_index(T).expand(B, qu.shape[2], T, T))
    return (ac + bd) * scale


def _softmax(scores, mask):
    dead = ~mask
    p = torch.softmax(scores.masked_fill(dead, NEG), -1).masked_fill(dead, 0.0)
    lse = torch.logsumexp(scores.masked_fill(dead, -float("inf")), -1)
    lse = torch.where(mask.any(-1).expand_as(lse), lse, torch.full_like(lse, float("inf")))      # the flash forward's record of "no live key"
    return p, lse


def attention(q, k, v, *, pe=None, bias_u=None, bias_v=None, klen=None, causal: bool = False, scale: float = 0.125, dctx=None,
              rounded: bool = False, flash: bool = False, round_bias: bool = False) -> dict:
    """q [B, Lq, H, 64], k / v [B, Lk, H, 64], pe [2 Lq - 1, H, 64] with bias_u / bias_v [H, 64], klen [B] or None, dctx [B, Lq, H, 64] or None.
    -> ctx [B, Lq, H, 64], probs [B, H, Lq, Lk], lse [B, H, Lq] (+inf: no live key); with dctx: dq, dk, dv (shaped like q, k, v), and with pe:
    dq_ac, dq_bd (the gradients with respect to q+u and q+v) and dpe.  flash selects which kernel's dS the rounded mode restates.  round_bias
    (reference mode): q+u and q+v alone are rounded to bf16, gradient passed through — the reference of tests/test_gpu_lrs_kernels.py."""
    rel = pe is not None
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    mask = live_mask(B, Lq, Lk, klen, causal)
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    if rel:
        pe, bias_u, bias_v = pe.to(F64), bias_u.to(F64), bias_v.to(F64)
    if dctx is not None:
        dctx = dctx.to(F64)
    if not rounded:
        leaves = [t.detach().clone().requires_grad_(True) for t in ((q, k, v, pe) if rel else (q, k, v))]
        ql, kl, vl = leaves[:3]
        qu = ql + bias_u if rel else ql
        qv = ql + bias_v if rel else None
        if rel and round_bias:
            qu, qv = qu + (_bf(qu.detach()) - qu.detach()), qv + (_bf(qv.detach()) - qv.detach())
        if rel:
            qu.retain_grad(); qv.retain_grad()
        p, lse = _softmax(scores_of(qu, qv, kl, leaves[3] if rel else None, scale), mask)
        ctx = torch.matmul(p, vl.transpose(1, 2)).transpose(1, 2)
        out = {"ctx": ctx.detach(), "probs": p.detach(), "lse": lse.detach()}
        if dctx is not None:
            ctx.backward(dctx)
            out.update(dq=ql.grad, dk=kl.grad, dv=vl.grad)
            if rel:
                out.update(dq_ac=qu.grad, dq_bd=qv.grad, dpe=leaves[3].grad)
        return out

    qu = _bf(q + bias_u) if rel else q
    qv = _bf(q + bias_v) if rel else None
    p, lse = _softmax(scores_of(qu, qv, k, pe, scale), mask)
    pr = _bf(p)
    ctx = _bf(torch.matmul(pr, v.transpose(1, 2)).transpose(1, 2))
    out = {"ctx": ctx, "probs": pr, "lse": lse}
    if dctx is None:
        return out
    dp = torch.matmul(dctx.transpose(1, 2), v.permute(0, 2, 3, 1))                  # [B, H, Lq, Lk]
    if flash:
        ds = p * (dp - (dctx * ctx).sum(-1).transpose(1, 2).unsqueeze(-1)) * scale
    else:
        ds = pr * (dp - (pr * dp).sum(-1, keepdim=True)) * scale
    ds = _bf(ds)
    dq_ac = torch.matmul(ds, k.transpose(1, 2)).transpose(1, 2)
    out["dk"] = _bf(torch.matmul(ds.transpose(-2, -1), qu.transpose(1, 2)).transpose(1, 2))
    out["dv"] = _bf(torch.matmul(pr.transpose(-2, -1), dctx.transpose(1, 2)).transpose(1, 2))
    if not rel:
        out["dq"] = _bf(dq_ac)
        return out
    T = Lq
    ds_full = torch.zeros(B, q.shape[2], T, 2 * T - 1, dtype=F64).scatter_(-1, _skew_index(T).expand(B, q.shape[2], T, T), ds)
    dq_bd = torch.matmul(ds_full, pe.transpose(0, 1)).transpose(1, 2)
    dpe = torch.matmul(ds_full.transpose(-2, -1), qv.transpose(1, 2)).sum(0).transpose(0, 1)
    out.update(dq=_bf(dq_ac + dq_bd), dq_ac=_bf(dq_ac), dq_bd=_bf(dq_bd), dpe=_bf(dpe))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the per-row metric
# ------------------------------------------------------------------------------------------------------------------------------------
def as_rows(name: str, t: torch.Tensor) -> torch.Tensor:
    """The rows of the metric: the last dimension is the row (one value for lse), the leading ones are its indices:
    ctx / dq / dq_ac / dq_bd (clip, query, head); dk / dv (clip, key, head); dpe (table row, head); lse (clip, head, query); probs (clip, head, query)"""
    return t.unsqueeze(-1) if name == "lse" else t


class RowCheck(NamedTuple):
    worst: float            # max over rows of |got - ref| / max(|ref|, 0.05 median |ref| over ref's non-zero rows)
    where: tuple            # indices of that row
    nonzero: int            # rows that are exactly zero (or infinite, lse) in ref and are not the same in got
    nonzero_where: Optional[tuple]
    whole: float            # |got - ref| / |ref| over the whole tensor (0 where ref is all zero)


def row_check(name: str, got: torch.Tensor, ref: torch.Tensor) -> RowCheck:
    got, ref = as_rows(name, got.to(F64)), as_rows(name, ref.to(F64))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    inf = torch.isinf(ref).any(-1)
    fin_ref = torch.where(inf.unsqueeze(-1), torch.zeros_like(ref), ref)
    fin_got = torch.where(inf.unsqueeze(-1), torch.zeros_like(got), got)
    rn = fin_ref.norm(dim=-1)
    zero = (rn == 0) & ~inf
    bad = (zero & (got != 0).any(-1)) | (inf & (got != ref).any(-1)) | torch.isnan(got).any(-1)
    live = rn[rn > 0]
    floor = 0.05 * float(live.median()) if live.numel() else 0.0
    err = (fin_got - fin_ref).norm(dim=-1) / rn.clamp_min(max(floor, 1e-300))
    if floor == 0.0:                                   # nothing in ref is non-zero: there is no scale, the rule of exact zeros is all there is
        err = torch.zeros_like(err)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    flat = int(err.argmax())
    where = tuple(int(x) for x in torch.unravel_index(torch.tensor(flat), err.shape))
    nb = int(bad.sum())
    bw = tuple(int(x) for x in torch.unravel_index(bad.flatten().int().argmax(), bad.shape)) if nb else None
    tot = float(fin_ref.norm())
    return RowCheck(float(err.flatten()[flat]), where, nb, bw, float((fin_got - fin_ref).norm() / tot) if tot > 0 else 0.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases, smallest first within each family
# ------------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    rel: bool
    causal: bool
    Lq: int
    Lk: int
    klen: Optional[tuple]      # per clip
    B: int


def _rel(T, klen=None, B=None):
    if klen is None and B is None:
        klen = (T, 33) if T >= 257 else (T, 1, min(32, T), max(1, T - 1))
    B = len(klen) if klen is not None else B
    return Case(f"rel-T{T}" + ("" if klen is not None else "-nolen") + ("-short" if klen is not None and max(klen) < T else ""), True, False, T, T, klen, B)


def _src(Lq, Lk, klen=None):
    klen = klen if klen is not None else tuple(min(max(x, 1), Lk) for x in (Lk, 1, 32, Lk - 1))
    return Case(f"src-{Lq}x{Lk}" + ("-dead" if min(klen) == 0 else ""), False, False, Lq, Lk, klen, len(klen))


REL_CASES = sorted([_rel(T) for T in (1, 31, 32, 33, 64, 65, 129, 161, 192, 193, 225, 256, 257, 512, 513)]
                   + [_rel(96, (40, 33, 1)), _rel(64, None, 2)], key=lambda c: (c.Lq, c.name))
CAUSAL_CASES = sorted([Case(f"causal-T{T}", False, True, T, T, None, 2) for T in (1, 32, 33, 64, 257)]
                      + [Case("causal-T65-klen", False, True, 65, 65, (65, 32, 1), 3)], key=lambda c: c.Lq)
SRC_CASES = [_src(1, 1), _src(1, 300), _src(33, 32), _src(32, 33), _src(70, 256), _src(257, 64)]
DEAD_CASE = _src(33, 64, (64, 0))
CASES = REL_CASES + CAUSAL_CASES + SRC_CASES + [DEAD_CASE]
GUARD_CASES = ("rel-T33", "rel-T257", "src-32x33")
DETERMINISM_CASES = ("rel-T256", "rel-T513")


def case(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


def _r(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def make_inputs(c: Case) -> dict:
    """Seeded randn rounded to bf16, biases scaled 0.5 (fp32), laid out as the kernels take them: rel: qkv [B*T, 3D], pe [2T-1, D], u / v [H, 64],
    dctx [B*T, D]; otherwise q [B*Lq, D], kv [B*Lk, 2D], dctx [B*Lq, D]"""
    D = H * DH
    if c.rel:
        return dict(qkv=_r(c.B * c.Lq, 3 * D, seed=1).to(BF), pe=_r(2 * c.Lq - 1, D, seed=2).to(BF), u=_r(H, DH, seed=3, scale=0.5),
                    v=_r(H, DH, seed=4, scale=0.5), dctx=_r(c.B * c.Lq, D, seed=5).to(BF))
    return dict(q=_r(c.B * c.Lq, D, seed=1).to(BF), kv=_r(c.B * c.Lk, 2 * D, seed=2).to(BF), dctx=_r(c.B * c.Lq, D, seed=3).to(BF))


def restate(c: Case, x: dict, **kw) -> dict:
    if c.rel:
        qkv = x["qkv"].view(c.B, c.Lq, 3, H, DH)
        return attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], pe=x["pe"].view(-1, H, DH), bias_u=x["u"], bias_v=x["v"], klen=c.klen,
                         dctx=x["dctx"].view(c.B, c.Lq, H, DH), **kw)
    kv = x["kv"].view(c.B, c.Lk, 2, H, DH)
    return attention(x["q"].view(c.B, c.Lq, H, DH), kv[:, :, 0], kv[:, :, 1], klen=c.klen, causal=c.causal, dctx=x["dctx"].view(c.B, c.Lq, H, DH), **kw)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """The float64 reference of a case, computed once and shared; callers do not modify it."""
    c = case(name)
    return restate(c, make_inputs(c))


# ------------------------------------------------------------------------------------------------------------------------------------
# tolerances
# ------------------------------------------------------------------------------------------------------------------------------------
# The largest per-row error (row_check) of rounded=True against rounded=False over every case above and both forms of dS, as
# tests/test_mha_restatement_cpu.py measures it (recorded 2 % above the measurement: a float64 BLAS that sums in another order moves a
# rounding here and there).  The maxima sit at rows whose gradient is a small difference of large terms: dS = P ∘ (dP - D) where dP is
# close to D, so the 2^-9 of one bf16 rounding of P, ctx or q+u is a large fraction of what is left — they are far above the whole-tensor
# figures (3e-3 to 4e-3), which is why the whole-tensor bounds of tests/test_gpu_lrs_kernels.py are asserted beside them.
ROUNDING = {
    "ctx": 1.19e-2,       # rel-T225, per-tile dS, clip 3 (klen 224) query 34 head 1
    "probs": 1.07e-2,     # rel-T225, the same row
    "lse": 5.36e-2,       # rel-T1: the one score of clip 0 head 0 is close to zero, q+u is rounded
    "dq": 6.76e-2,        # rel-T31, flash dS, clip 0 query 6 head 1
    "dk": 1.174e-1,       # src-1x300, flash dS, clip 2 (klen 32) key 23 head 0: one query, dP - dctx·bf16(ctx) of a key with dP close to D
    "dv": 1.28e-2,        # rel-T225, per-tile dS, clip 3 key 197 head 1
    "dq_ac": 5.70e-2,     # rel-T31, flash dS, clip 0 query 6 head 1
    "dq_bd": 8.33e-2,     # rel-T31, the same row
    "dpe": 1.84e-2,       # rel-T193, flash dS, table row 84 head 1
}
# what the rounded restatement cannot reproduce — fp32 accumulation order, __expf / __logf, the online-softmax rescaling — is covered by a factor
FACTOR = {n: 4.0 for n in TENSORS}
# the whole-tensor bounds of tests/test_gpu_lrs_kernels.py (probs: that of ctx; dq_ac, dq_bd: that of the gradients)
WHOLE_BOUND = dict(ctx=1.5e-2, probs=1.5e-2, lse=2e-3, dq=2.5e-2, dk=2.5e-2, dv=2.5e-2, dq_ac=2.5e-2, dq_bd=2.5e-2, dpe=2.5e-2)


def tolerance(name: str) -> float:
    return FACTOR[name] * ROUNDING[name]
