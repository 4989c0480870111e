"""Plain float64 restatement of the non-contraction kernels of the sentence-level training step (syncvsr_amd/csrc/lrs_misc.hip), the cases
tests/test_gpu_lrs_loss_edges.py runs them at, and the tolerances of that comparison.

  ctc            k_row_lse, k_ctc_lattice, k_ctc_grad: torch.nn.CTCLoss(reduction="sum", zero_infinity=True) / B on log_softmax, blank 0,
                 written out as the alpha / beta recursions over the extended target (blank, y0, blank, y1, ..., blank); an item whose
                 ilen is outside [1, T] contributes 0 and gets zero gradient rows
  ls_loss        k_ls_loss_fwd / bwd: ESPnet's label-smoothing KL loss, the argmax counts (a tie goes to the lowest index), the gradient; a
                 target >= V poisons the loss with NaN and leaves the gradient finite (no entry of the row is the target)
  glu_dwconv     k_glu_dwconv_fwd / bwd, k_dw_reduce: GLU, depthwise Conv1d(K, pad (K-1)/2), the BatchNorm partial rows per (clip, 32-frame
                 tile), and the backward by hand
  embed_pos_bwd  k_embed_pos_bwd: demb[tok[r]] += scale * dx[r]

Each takes `brk`, a deliberate mistake of the kind the edge cases exist to catch (BREAKS): the GPU tests must fail against a restatement that
makes it, and the older mid-sized cases of tests/test_gpu_lrs_kernels.py must not notice.  tests/test_lrs_loss_restatement_cpu.py checks both
halves of that on the host.

The per-row metric is mha_restatement.row_check: |got - ref| / max(|ref|, 0.05 median |ref| over the non-zero rows), rows that are exactly
zero in the reference exactly zero in the output.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from mha_restatement import RowCheck, row_check  # noqa: F401  (the metric; re-exported)

BF = torch.bfloat16
F64 = torch.float64
U32 = 2.0 ** -24              # unit roundoff of fp32
DW_TT = 32                    # frames per tile of the depthwise kernels (lrs_misc.hip)
DW_SPLITS = 96                # ops.DW_SPLITS
EMB_LIST_CAP = 4096 - 32      # rows of one token the list path of k_embed_pos_bwd is sure to hold
EMB_MAX_ROWS = 16384
BREAKS = ("drop_states_256", "skip_equal_256", "one_tile_per_split", "list_cap_rows")


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(BF).to(F64)


# ------------------------------------------------------------------------------------------------------------------------------------
# CTC
# ------------------------------------------------------------------------------------------------------------------------------------
def target_of(row) -> list:
    """labels of a -1 padded row: everything in front of the first negative entry (a full row has no terminator)"""
    out = []
    for v in row:
        if int(v) < 0:
            break
        out.append(int(v))
    return out


def ctc(z, labels, ilen, B: int, T: int, V: int, gout: float = 1.0, brk: Optional[str] = None) -> dict:
    """z [B*T, >= V] (columns V.. and rows t >= ilen[b] are never looked at), labels int64 [B, Lmax] padded with -1, ilen [B].
    -> nll [B] (after zero_infinity), loss = sum(nll) / B, dz [B*T, V] = gout * dloss/dz, feasible [B] bool"""
    zz = np.asarray(torch.as_tensor(z).to(F64))[:, :V].reshape(B, T, V)
    nll = np.zeros(B)
    feas = np.zeros(B, dtype=bool)
    dz = np.zeros((B, T, V))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            Tb = int(ilen[b])
            if Tb < 1 or Tb > T:
                continue
            y = target_of(labels[b])
            S = 2 * len(y) + 1
            x = zz[b, :Tb]
            m = x.max(1, keepdims=True)
            lp = x - (m + np.log(np.exp(x - m).sum(1, keepdims=True)))          # log_softmax of the live frames
            ext = np.zeros(S, dtype=np.int64)
            ext[1::2] = y
            skip = np.zeros(S, dtype=bool)                                        # s-2 -> s: odd s whose label differs from the one before
            skip[2:] = (np.arange(2, S) % 2 == 1) & (ext[2:] != ext[:-2])
            dead = np.zeros(S, dtype=bool)
            if brk == "skip_equal_256":
                skip[2:] |= (np.arange(2, S) % 2 == 1) & (np.arange(2, S) >= 256)
            if brk == "drop_states_256":
                dead[256:] = True
            NEG = -np.inf
            e = lp[:, ext]                                                        # [Tb, S] emission of every state
            alpha = np.full((Tb, S), NEG)
            alpha[0, 0] = e[0, 0]
            if S > 1:
                alpha[0, 1] = e[0, 1]
            alpha[0, dead] = NEG
            for t in range(1, Tb):
                a = alpha[t - 1]
                v = a.copy()
                v[1:] = np.logaddexp(v[1:], a[:-1])
                v[2:] = np.where(skip[2:], np.logaddexp(v[2:], a[:-2]), v[2:])
                alpha[t] = v + e[t]
                alpha[t, dead] = NEG
            ll = np.logaddexp(alpha[Tb - 1, S - 1], alpha[Tb - 1, S - 2] if S > 1 else NEG)
            if not np.isfinite(ll):
                continue                                                          # zero_infinity: no loss, no gradient
            feas[b] = True
            nll[b] = -ll
            beta = np.full((Tb, S), NEG)                                          # includes the emission at t
            beta[Tb - 1, S - 1] = e[Tb - 1, S - 1]
            if S > 1:
                beta[Tb - 1, S - 2] = e[Tb - 1, S - 2]
            beta[Tb - 1, dead] = NEG
            for t in range(Tb - 2, -1, -1):
                n = beta[t + 1]
                v = n.copy()
                v[:-1] = np.logaddexp(v[:-1], n[1:])
                v[:-2] = np.where(skip[2:], np.logaddexp(v[:-2], n[2:]), v[:-2])
                beta[t] = v + e[t]
                beta[t, dead] = NEG
            occ = np.exp(alpha + beta - e - ll)                                   # posterior of being in state s at frame t
            occ[~np.isfinite(alpha + beta)] = 0.0
            acc = np.zeros((Tb, V))
            np.add.at(acc, (np.arange(Tb)[:, None], ext[None, :]), occ)
            dz[b, :Tb] = (np.exp(lp) - acc) * (gout / B)
    return dict(nll=torch.from_numpy(nll), loss=torch.tensor(nll.sum() / B, dtype=F64), dz=torch.from_numpy(dz.reshape(B * T, V)),
                feasible=torch.from_numpy(feas))


class CtcCase(NamedTuple):
    name: str
    T: int
    V: int
    targets: tuple            # per item, a tuple of labels
    ilen: tuple
    Lmax: int
    scale: float = 1.0        # of the logits
    gout: float = 1.0
    ldo_extra: int = 0        # ldo = ld + this

    @property
    def B(self) -> int:
        return len(self.targets)

    @property
    def ld(self) -> int:
        return (self.V + 63) // 64 * 64


def frames_needed(y) -> int:
    """the shortest input that can emit y: one frame per label and a blank between equal neighbours"""
    return len(y) + sum(1 for a, b in zip(y, y[1:]) if a == b)


def _long_target(n: int, V: int, seed: int) -> tuple:
    """n labels with equal neighbours early, in the middle, past label 128 (lattice state 257: the second pass of the state loops) and at the
    very end"""
    g = torch.Generator().manual_seed(seed)
    y = [int(v) for v in torch.randint(1, V, (n,), generator=g)]
    for i in (1, n // 2, n - 1) + ((130, 200) if n > 201 else ()):
        if 0 < i < n:
            y[i] = y[i - 1]
    return tuple(y)


def _ctc_cases() -> list:
    C = CtcCase
    same = (7,) * 6
    out = [
        C("T1-one-label", 1, 11, ((4,), (2, 5)), (1, 1), 2),                                     # the second item is infeasible
        C("B1", 7, 11, ((3, 4),), (7,), 2),
        C("empty-target", 5, 11, ((), (3, 3), (1, 2, 3)), (5, 3, 5), 3),                          # S = 1; (3, 3) at exactly 2n - 1 frames
        C("V2", 6, 2, ((1, 1), (1,), ()), (6, 4, 2), 2),
        C("full-row", 9, 11, ((1, 2, 2, 3), (5,), (6, 6, 6, 6)), (9, 4, 6), 4),                   # no -1 terminator; the third is infeasible
        C("all-same", 12, 11, (same, same, same), (11, 10, 12), 6),                               # 2n - 1 frames, 2n - 2 (infeasible), slack
        C("distinct-exact", 10, 11, (tuple(range(1, 11)), (3, 1, 4), (2, 9)), (10, 3, 1), 10),    # ilen == len: softmax - one-hot; ilen < len
        C("gout-ldo", 8, 11, ((1, 2, 2), (4,)), (8, 5), 3, 1.0, 0.3, 64),
        C("scaled-20", 12, 11, ((1, 2, 3), (2, 2), (5,)), (12, 7, 1), 3, 20.0),
        C("V5049", 20, 5049, ((17, 5048, 5048, 1, 2500, 9), (4000, 3, 3)), (20, 13), 6),
        C("T600", 600, 11, ((1, 2, 2, 5, 3), (4,)), (600, 377), 5),
    ]
    ys = tuple(_long_target(n, 70, 40 + n) for n in (127, 128, 129))                              # S = 255, 257, 259
    need = [frames_needed(y) for y in ys]
    T = max(need) + 3
    out.append(C("len-127-128-129", T, 70, ys, (need[0] + 1, T, need[2]), 129))
    ys = tuple(_long_target(n, 70, 40 + n) for n in (256, 257))                                   # S = 513, 515: a third pass
    need = [frames_needed(y) for y in ys]
    T = max(need) + 2
    out.append(C("len-256-257", T, 70, ys, (need[0] + 2, T), 257))
    return out


CTC_CASES = _ctc_cases()
# items whose ilen is outside [1, T], first, in the middle and last; CTC_BAD_ILEN_KEPT are the others, run alone with gout / 2 (B = 8 -> 4: the
# same gout / B to the bit)
CTC_BAD_ILEN = CtcCase("bad-ilen", 6, 11, ((1, 2), (3,), (4, 4), (5, 6), (1,), (2, 3), (7,), (8, 9)), (0, 6, 4, 9, -2, 5, 2, 7), 2)
CTC_BAD_ILEN_KEPT = (1, 2, 5, 6)


def ctc_case(name: str) -> CtcCase:
    return next(c for c in CTC_CASES + [CTC_BAD_ILEN] if c.name == name)


def ctc_labels(c: CtcCase) -> torch.Tensor:
    lab = torch.full((c.B, c.Lmax), -1, dtype=torch.int64)
    for b, y in enumerate(c.targets):
        lab[b, :len(y)] = torch.tensor(y, dtype=torch.int64)
    return lab


def ctc_logits(c: CtcCase, nan_pad: bool) -> torch.Tensor:
    """fp32 [B*T, ld].  nan_pad: the pad columns V..ld, the rows t >= ilen[b] and every row of an item whose ilen is outside [1, T] are NaN —
    nothing may read them; otherwise they hold ordinary values"""
    z = torch.randn(c.B * c.T, c.ld, generator=torch.Generator().manual_seed(11)) * c.scale
    if nan_pad:
        z[:, c.V:] = float("nan")
        zv = z.view(c.B, c.T, c.ld)
        for b, n in enumerate(c.ilen):
            zv[b, (n if 1 <= n <= c.T else 0):] = float("nan")
    return z


@functools.lru_cache(maxsize=None)
def ctc_reference(name: str) -> dict:
    c = ctc_case(name)
    return ctc(ctc_logits(c, False), ctc_labels(c), c.ilen, c.B, c.T, c.V, c.gout)


# ------------------------------------------------------------------------------------------------------------------------------------
# label smoothing
# ------------------------------------------------------------------------------------------------------------------------------------
def ls_loss(z, target, V: int, smoothing: float, inv_denom: float, gout: float = 1.0) -> dict:
    """z [R, >= V], target int64 [R] (negative: the row is ignored) -> loss, correct, live, lse [R], dz [R, V]"""
    x = torch.as_tensor(z).to(F64)[:, :V]
    t = torch.as_tensor(target)
    R = x.shape[0]
    live, bad = t >= 0, t >= V
    lsm = torch.log_softmax(x, 1)
    true = torch.full_like(x, smoothing / (V - 1))
    ok = live & ~bad
    true[ok, t[ok]] = 1.0 - smoothing
    rows = (torch.xlogy(true, true) - true * lsm).sum(1) * inv_denom
    rows = torch.where(live, rows, torch.zeros_like(rows))
    rows = torch.where(bad, torch.full_like(rows, float("nan")), rows)
    cols = torch.arange(V).expand(R, V)
    am = torch.where(x == x.max(1, keepdim=True).values, cols, torch.full_like(cols, V)).min(1).values      # a tie: the lowest index
    dz = gout * inv_denom * (torch.softmax(x, 1) - true) * live.unsqueeze(1)
    return dict(loss=rows.sum(), correct=int(((am == t) & live).sum()), live=int(live.sum()), lse=torch.logsumexp(x, 1), dz=dz)


class LsCase(NamedTuple):
    name: str
    R: int
    V: int
    smoothing: float
    norm_len: bool
    kind: str = "mixed"       # mixed | all-ignored | bad-target
    ldo_extra: int = 0

    @property
    def ld(self) -> int:
        return (self.V + 63) // 64 * 64


LS_CASES = ([LsCase(f"R{R}-V{V}-s{s}-{'len' if nl else 'batch'}", R, V, s, nl, ldo_extra=64 if R == 5 else 0)
             for V in (2, 63, 64, 65) for R in (1, 5, 27) for s in (0.0, 0.1) for nl in (False, True)]
            + [LsCase(f"R5-V5049-s{s}-{'len' if nl else 'batch'}", 5, 5049, s, nl) for s in (0.0, 0.1) for nl in (False, True)]
            + [LsCase("all-ignored", 5, 11, 0.1, False, "all-ignored"), LsCase("bad-target", 6, 11, 0.1, False, "bad-target", 64)])
LS_BATCH = 3                  # the denominator of the batch normalisation


def ls_case(name: str) -> LsCase:
    return next(c for c in LS_CASES if c.name == name)


def ls_inputs(c: LsCase, nan_pad: bool):
    """-> z fp32 [R, ld], target int64 [R], inv_denom.  Row 0's target is V - 1; rows 0 and 1 hold a constructed argmax tie between columns 0
    and V - 1 (row 0: the target is the higher index, so the row is NOT counted correct; row 1: the target is column 0, counted); every
    third row from row 2 is ignored."""
    g = torch.Generator().manual_seed(13)
    z = torch.randn(c.R, c.ld, generator=g)
    t = torch.randint(0, c.V, (c.R,), generator=g)
    t[0] = c.V - 1
    z[0, 0] = z[0, c.V - 1] = 6.0
    if c.R > 1:
        t[1] = 0
        z[1, 0] = z[1, c.V - 1] = 6.0
        t[2::3] = -1
    if c.kind == "all-ignored":
        t[:] = -1
    if c.kind == "bad-target":
        t[3], t[4] = c.V, c.V + 100
    if nan_pad:
        z[:, c.V:] = float("nan")
    live = int((t >= 0).sum())
    return z, t, (1.0 / max(live, 1) if c.norm_len else 1.0 / LS_BATCH)


@functools.lru_cache(maxsize=None)
def ls_reference(name: str) -> dict:
    c = ls_case(name)
    z, t, inv = ls_inputs(c, False)
    return ls_loss(z, t, c.V, c.smoothing, inv)


# ------------------------------------------------------------------------------------------------------------------------------------
# GLU + depthwise conv
# ------------------------------------------------------------------------------------------------------------------------------------
def glu_dwconv(u, w, bias, dc, B: int, T: int, D: int, K: int, brk: Optional[str] = None) -> dict:
    """u [B*T, 2D] (value | gate), w [D, K], bias [D], dc [B*T, D] -> c [B*T, D], stats [B * ceil(T / 32), 2, D] (sum and sum of squares of c over
    the frames of one (clip, tile)), du [B*T, 2D], dw [D, K], dbias [D]; c_abs, stats_abs, dw_abs, dbias_abs: the same sums over absolute
    values (what an fp32 summation error is proportional to)"""
    u, w, bias, dc = (torch.as_tensor(t).to(F64) for t in (u, w, bias, dc))
    pad = (K - 1) // 2
    uv = u.view(B, T, 2 * D)
    a, sg = uv[..., :D], torch.sigmoid(uv[..., D:])
    g = a * sg
    gp = torch.zeros(B, T + K - 1, D, dtype=F64)
    gp[:, pad:pad + T] = g
    win = gp.unfold(1, K, 1)                                                      # [B, T, D, K]: g[t + k - pad]
    c = (win * w).sum(-1) + bias
    c_abs = (win.abs() * w.abs()).sum(-1) + bias.abs()
    ntt = (T + DW_TT - 1) // DW_TT
    tile_of = torch.arange(B).view(B, 1) * ntt + (torch.arange(T) // DW_TT).view(1, T)       # [B, T] -> row of the partials
    rows = tile_of.flatten()
    stats = torch.zeros(B * ntt, 2, D, dtype=F64)
    stats[:, 0].index_add_(0, rows, c.reshape(B * T, D))
    stats[:, 1].index_add_(0, rows, (c * c).reshape(B * T, D))
    stats_abs = torch.zeros_like(stats)
    stats_abs[:, 0].index_add_(0, rows, c_abs.reshape(B * T, D))
    stats_abs[:, 1].index_add_(0, rows, (c_abs * c_abs).reshape(B * T, D))
    dcv = dc.view(B, T, D)
    seen = torch.ones(B, T, 1, dtype=F64)
    if brk == "one_tile_per_split":                                               # a workgroup that stops after its first tile
        seen = (tile_of < DW_SPLITS).to(F64).unsqueeze(-1)
    dcp = torch.zeros(B, T + K - 1, D, dtype=F64)
    dcp[:, pad:pad + T] = dcv
    dg = (dcp.unfold(1, K, 1) * w.flip(-1)).sum(-1) * seen                        # dg[t] = sum_k dc[t - k + pad] w[k]
    du = torch.cat([dg * sg, dg * a * sg * (1.0 - sg)], -1).reshape(B * T, 2 * D)
    dcs = dcv * seen
    return dict(c=c.reshape(B * T, D), c_abs=c_abs.reshape(B * T, D), stats=stats, stats_abs=stats_abs, du=du,
                dw=torch.einsum("btd,btdk->dk", dcs, win), dw_abs=torch.einsum("btd,btdk->dk", dcs.abs(), win.abs()),
                dbias=dcs.sum((0, 1)), dbias_abs=dcs.abs().sum((0, 1)))


class DwCase(NamedTuple):
    B: int
    T: int
    D: int
    K: int

    @property
    def name(self) -> str:
        return f"B{self.B}-T{self.T}-D{self.D}-K{self.K}"


DW_CASES = [DwCase(2, T, D, K) for T in (1, 31, 32, 33, 65) for D in (64, 192) for K in (1, 3, 15, 31)]
DW_MANY_TILES = [DwCase(13, 250, 64, 31), DwCase(13, 250, 64, 7)]                 # 13 * 8 = 104 tiles > 96 splits: eight workgroups take two
DW_START = 0.75               # dw and dbias start at this value (exact in fp32) instead of zero


def dw_case(name: str) -> DwCase:
    return next(c for c in DW_CASES + DW_MANY_TILES if c.name == name)


def _r(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dw_inputs(c: DwCase) -> dict:
    return dict(u=_r(c.B * c.T, 2 * c.D, seed=1).to(BF), w=_r(c.D, c.K, seed=2, scale=1 / math.sqrt(c.K)), bias=_r(c.D, seed=3, scale=0.1),
                dc=_r(c.B * c.T, c.D, seed=4).to(BF))


@functools.lru_cache(maxsize=None)
def dw_reference(name: str) -> dict:
    c = dw_case(name)
    return glu_dwconv(**dw_inputs(c), B=c.B, T=c.T, D=c.D, K=c.K)


# ------------------------------------------------------------------------------------------------------------------------------------
# decoder embedding backward
# ------------------------------------------------------------------------------------------------------------------------------------
def embed_pos_bwd(tok, dx, V: int, scale: float, start=None, brk: Optional[str] = None) -> dict:
    """tok int64 [R], dx [R, D] -> demb [V, D] = start + scale * (sum of the rows of each token), demb_abs (over absolute values), rows [V]"""
    tok = torch.as_tensor(tok).flatten()
    x = torch.as_tensor(dx).to(F64) * scale
    if brk == "list_cap_rows":                                                    # only as many rows of a token as the list path holds
        nth = torch.zeros_like(tok)
        for v in tok.unique():
            sel = tok == v
            nth[sel] = torch.arange(int(sel.sum()))
        x = x * (nth < EMB_LIST_CAP).unsqueeze(1)
    D = x.shape[1]
    s0 = torch.zeros(V, D, dtype=F64) if start is None else torch.as_tensor(start).to(F64)
    return dict(demb=s0.clone().index_add_(0, tok, x), demb_abs=s0.abs().index_add_(0, tok, x.abs()),
                rows=torch.bincount(tok, minlength=V))


class EmbCase(NamedTuple):
    n_big: int                # rows of token EMB_BIG (0: none, random tokens only)
    R: int
    D: int

    @property
    def name(self) -> str:
        return f"big{self.n_big}-R{self.R}-D{self.D}"


EMB_V, EMB_BIG = 50, 7
EMB_CASES = [EmbCase(n, n + 300, D) for D in (8, 264) for n in (4064, 4065, 4200)] + [EmbCase(0, 27, 8), EmbCase(0, EMB_MAX_ROWS, 8)]


def emb_inputs(c: EmbCase, exact: bool):
    """-> tok int64 [R] (token EMB_BIG on n_big rows spread among the others), dx bf16 [R, D], scale.  exact: dx holds small integers and the
    scale is 4, so every partial sum is an integer below 2^24 — fp32 adds them without rounding in any order"""
    g = torch.Generator().manual_seed(17)
    others = torch.randint(0, EMB_V - 1, (c.R - c.n_big,), generator=g)
    others = others + (others >= EMB_BIG).long()
    tok = torch.cat([torch.full((c.n_big,), EMB_BIG, dtype=torch.int64), others])[torch.randperm(c.R, generator=g)]
    if exact:
        return tok, torch.randint(-8, 9, (c.R, c.D), generator=g).to(BF), 4.0
    return tok, torch.randn(c.R, c.D, generator=g).to(BF), math.sqrt(c.D)


# ------------------------------------------------------------------------------------------------------------------------------------
# tolerances
# ------------------------------------------------------------------------------------------------------------------------------------
# dz, c and du are stored as bf16: one rounding per element.  bf16 keeps 8 significant bits, so a rounding is at most 2^-9 of the element's
# binade, which is up to 2^-8 = 3.9e-3 of the element itself, and a row's error is at most 2^-8 of its norm.  ROUNDING is the largest per-row
# error (row_check) of the reference rounded to bf16 against itself over every case above, as tests/test_lrs_loss_restatement_cpu.py measures
# it (recorded 2 % above the measurement: short rows whose elements sit low in their binades come close to the 2^-8); the bound is 4 x that — the margin is for __expf / __logf / the fast reciprocal of the
# sigmoid and for fp32 accumulation, which are not restated — and never more than the whole-tensor bound of tests/test_gpu_lrs_kernels.py,
# which the whole tensors are held to as well.  (4 x ROUNDING is above 6e-3 for all four, so 6e-3 is the bound of every row.)
ROUNDING = {
    "ctc_dz": 3.41e-3,    # T600, clip 0 frame 490
    "ls_dz": 3.49e-3,     # R1-V2-s0.1-batch: a row of two elements, both rounded the same way
    "c": 2.58e-3,         # B13-T250-D64-K31, row 1660
    "du": 2.70e-3,        # B2-T31-D64-K1, row 46
}
MEASURED = {
    # worst figures of the kernels on an MI355X against the float64 reference over every case (tests/test_gpu_lrs_loss_edges.py prints them)
    "ctc_dz": 4.73e-3,        # per row: T600, clip 0 frame 103 (bound 6e-3); whole tensor 1.90e-3 (distinct-exact)
    "ls_dz": 3.42e-3,         # per row: R1-V2-s0.1-batch — the bf16 rounding alone; whole tensor the same (one row)
    "c": 2.53e-3,             # per row: B13-T250-D64-K31, clip 6 frame 160; whole tensor 1.79e-3 (B2-T1-D64-K15)
    "du": 2.64e-3,            # per row: B2-T31-D64-K1, clip 1 frame 15; whole tensor 1.81e-3 (B2-T1-D64-K15)
    "ctc_nll": 5.8e-7,        # relative, len-256-257 item 1 (bound 2e-4); closest to its bound: T1-one-label, 1.8e-8 of 5.3e-6
    "ls_loss": 3.5e-7,        # relative, R1-V65-s0.1-len (bound 5.7e-6)
    "lse": 1.2e-7,            # relative, R27-V2-s0.0-batch row 11 (bound 5.3e-6)
    "stats": 9.3e-3,          # of sum_bound: B2-T1-D64-K1, sum of squares
    "dw": 2.1e-2,             # of sum_bound: B2-T1-D64-K1; whole tensor 2.1e-7 (B13-T250-D64-K31)
    "dbias": 1.6e-6,          # of sum_bound; whole tensor 6.1e-8
    "demb": 7.3e-2,           # of its bound: big0-R27-D8, a token on one row; exact (integer-valued) inputs: equal
}
WHOLE_BOUND = dict(ctc_dz=6e-3, ls_dz=6e-3, c=6e-3, du=6e-3, ctc_loss=2e-4, ls_loss=2e-5, dw=5e-3, dbias=5e-3)


def tolerance(name: str) -> float:
    return min(4.0 * ROUNDING[name], WHOLE_BOUND[name])


# fp32 results (losses, log-sum-exps, partial sums, parameter gradients) carry no bf16 rounding; what bounds them is fp32 summation: a sum of n
# terms, in any order, is off by at most n 2^-24 sum |terms|.  FAST_OPS stands for the relative error of one __expf / __logf / reciprocal chain
# (a few units in the last place each), counted as 16 more roundings; the factor 4 is the same margin as above.
FAST_OPS = 16


def sum_bound(n_terms: int, abs_sum: torch.Tensor) -> torch.Tensor:
    """element-wise bound on |fp32 result - exact| for a result built from n_terms fp32 operations over terms whose absolute values add up to abs_sum"""
    return 4.0 * (n_terms + FAST_OPS) * U32 * abs_sum


def bound_check(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor):
    """rows = the last dimension: -> (worst |got - ref| / |bound| over the rows, its indices); NaN in got is infinitely wrong"""
    got, ref, bound = (t.to(F64).reshape(-1, t.shape[-1]) if t.dim() > 1 else t.to(F64).reshape(-1, 1) for t in (got, ref, bound))
    err = (got - ref).norm(dim=-1) / bound.norm(dim=-1).clamp_min(1e-300)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    i = int(err.argmax())
    return float(err[i]), i


def ctc_nll_tolerance(T: int, V: int) -> float:
    """relative to max(1, |nll|): the running log-probability is rounded once per frame and each frame's log-softmax is a sum of V terms by 64
    lanes (V / 64 + 6 additions) plus one __expf / __logf chain per step; never more than the 2e-4 of tests/test_gpu_lrs_kernels.py"""
    return min(WHOLE_BOUND["ctc_loss"], 4.0 * T * (V / 64 + 6 + FAST_OPS) * U32)


def ls_loss_tolerance(R: int, V: int) -> float:
    """relative to max(1, |loss|): per row two sums of V terms by 64 lanes, then the fixed-order sum of R rows; never more than 2e-5"""
    return min(WHOLE_BOUND["ls_loss"], 4.0 * (R + V / 64 + 6 + FAST_OPS) * U32)


def lse_tolerance(V: int) -> float:
    """relative to max(1, |lse|)"""
    return 4.0 * (V / 64 + 6 + FAST_OPS) * U32
