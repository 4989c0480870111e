"""Plain-torch float64 restatement of the stem front-end kernels — syncvsr_amd/csrc/stem.hip (Conv3d 1 -> 64, 5x7x7, stride 1x2x2, pad 2x3x3:
forward with BatchNorm partial sums, weight gradient) and the stem passes of syncvsr_amd/csrc/norm_act.hip (BatchNorm + GELU / Swish + 3x3
stride-2 max-pool, forward and backward) — the cases tests/test_gpu_stem_edges.py runs them at, each with the path it is meant to take
(tests/test_stem_restatement_cpu.py asserts the paths with the library's host queries), and the metrics with their tolerances.

The convolution is written as a gather of the 245 taps followed by one matrix product (nothing of torch's conv3d), the pool as nine strided
slices of a padded frame.  rounded=False is the reference: float64 throughout.  rounded=True restates where the kernels round to bf16 and
nothing else (not their fp32 summation order, not the erf / exp approximations of common.h):
  clip, weights                 both forward kernels and the weight gradient read them as bf16 (both modes: it is the kernels' definition)
  conv output                   bf16; the BatchNorm partial sums are taken from the unrounded accumulators
  y                             bf16 of the window maximum
  gpool (winner form only)      g = dpool * act'(z of the winner), bf16, before it is summed and routed (k_stem_bwd_reduce_win)
  dx                            bf16
The backward takes the KERNEL's arg-max (window slot 0..8, i * 3 + j) as an input, so routing is fully determined and no element of dx is
exempt from the comparison; certify_amax judges that arg-max on its own.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch

from mha_restatement import row_check  # noqa: F401  (the per-position metric: the last dimension, 64 channels, is the row)

BF = torch.bfloat16
F64 = torch.float64
ACT_GELU, ACT_SWISH = 1, 2
ACTS = (ACT_GELU, ACT_SWISH)
C_OUT, TAPS = 64, 245
FWD_CAP, WGRAD_CAP = 768, 512          # persistent workgroups of the forward / of the weight gradients (stem.hip stem_fwd_grid, stem_wgrad_grid)
SW_RB, STEM_GP, STEM_GPW, STEM_BR = 4, 4, 24, 8


def _bf(x: torch.Tensor) -> torch.Tensor:
    """fp32 value -> bf16 (round to nearest even, the kernels' f2bf), back in float64"""
    return x.float().to(BF).to(F64)


# ------------------------------------------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------------------------------------------
def patches(vid: torch.Tensor) -> torch.Tensor:
    """vid [B, T, H, W] -> the 245 taps of every output position [B*T, Ho, Wo, 245] (float64, zero outside the frame and outside the CLIP),
    tap index (kt * 7 + kh) * 7 + kw, pixel (t + kt - 2, 2y + kh - 3, 2x + kw - 3)"""
    B, T, H, W = vid.shape
    Ho, Wo = H // 2, W // 2
    vp = torch.zeros(B, T + 4, H + 6, W + 6, dtype=F64)
    vp[:, 2:2 + T, 3:3 + H, 3:3 + W] = _bf(vid)
    taps = [vp[:, kt:kt + T, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kt in range(5) for kh in range(7) for kw in range(7)]
    return torch.stack(taps, -1).reshape(B * T, Ho, Wo, TAPS)


def stem_conv_fwd(vid: torch.Tensor, w: torch.Tensor, rounded: bool = False, pat: torch.Tensor | None = None):
    """vid [B, T, H, W], w [64, 5, 7, 7] -> out [B*T, Ho, Wo, 64], per-channel sum [64] and sum of squares [64] of the unrounded output"""
    pat = patches(vid) if pat is None else pat
    out = pat @ _bf(w).reshape(C_OUT, TAPS).t()
    s, q = out.sum((0, 1, 2)), (out * out).sum((0, 1, 2))
    return (_bf(out) if rounded else out), s, q


def stem_conv_wgrad(vid: torch.Tensor, dy: torch.Tensor, pat: torch.Tensor | None = None) -> torch.Tensor:
    """vid [B, T, H, W], dy [B*T, Ho, Wo, 64] -> dw [64, 5, 7, 7]"""
    pat = patches(vid) if pat is None else pat
    return (dy.to(F64).reshape(-1, C_OUT).t() @ pat.reshape(-1, TAPS)).reshape(C_OUT, 5, 7, 7)


# ------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + activation + max-pool
# ------------------------------------------------------------------------------------------------------------------------------------
def act_fn(z: torch.Tensor, act: int) -> torch.Tensor:
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0))) if act == ACT_GELU else z * torch.sigmoid(z)


def act_grad(z: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def pooled_hw(Hc: int, Wc: int) -> tuple:
    return (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


def windows(t: torch.Tensor, fill: float) -> torch.Tensor:
    """t [N, Hc, Wc, C] -> [9, N, Hp, Wp, C]: slot i * 3 + j of pooled (ph, pw) is t[2ph - 1 + i, 2pw - 1 + j], `fill` outside the frame"""
    N, Hc, Wc, C = t.shape
    Hp, Wp = pooled_hw(Hc, Wc)
    pad = torch.full((N, 2 * Hp + 1, 2 * Wp + 1, C), fill, dtype=t.dtype)
    pad[:, 1:1 + Hc, 1:1 + Wc] = t
    return torch.stack([pad[:, i:i + 2 * Hp:2, j:j + 2 * Wp:2] for i in range(3) for j in range(3)])


def _at_slot(win: torch.Tensor, amax: torch.Tensor) -> torch.Tensor:
    return torch.gather(win, 0, amax.long().unsqueeze(0)).squeeze(0)


def _bn(x, mean, rstd, gamma, beta):
    xh = (x.to(F64) - mean.to(F64)) * rstd.to(F64)
    return xh, xh * gamma.to(F64) + beta.to(F64)


def pool_fwd(x, mean, rstd, gamma, beta, act: int, rounded: bool = False):
    """x [N, Hc, Wc, C] (bf16 values) -> z [N, Hc, Wc, C], a = act(z), and the per-window maximum of a [N, Hp, Wp, C]"""
    _, z = _bn(x, mean, rstd, gamma, beta)
    a = act_fn(z, act)
    y = windows(a, -math.inf).max(0).values
    return z, a, (_bf(y) if rounded else y)


class PoolBwd(NamedTuple):
    dx: torch.Tensor          # [N, Hc, Wc, C]
    dgamma: torch.Tensor      # [C]
    dbeta: torch.Tensor       # [C]
    abs_gx: torch.Tensor      # [C] sum |g * xhat|: the terms of dgamma
    abs_g: torch.Tensor       # [C] sum |g|
    rss_gx: torch.Tensor      # [C] sqrt(sum (g * xhat)^2) over the pooled outputs: the scale of the bf16 rounding of g in the winner form
    rss_g: torch.Tensor       # [C]


def pool_bwd(dpool, amax, x, mean, rstd, gamma, beta, act: int, rounded: bool = False, win: bool = False) -> PoolBwd:
    """dpool [N, Hp, Wp, C], amax [N, Hp, Wp, C] (uint8 window slot: the kernel's) -> dx, dgamma, dbeta.  The gradient of a pooled output goes
    to the element its slot names and nowhere else.  win (rounded mode): the winner form, which keeps g per pooled output in bf16."""
    N, Hc, Wc, C = x.shape
    Hp, Wp = pooled_hw(Hc, Wc)
    xh, z = _bn(x, mean, rstd, gamma, beta)
    g_out = dpool.to(F64) * act_grad(_at_slot(windows(z, 0.0), amax), act)          # per pooled output
    if rounded and win:
        g_out = _bf(g_out)
    xh_out = _at_slot(windows(xh, 0.0), amax)
    pad = torch.zeros(N, 2 * Hp + 1, 2 * Wp + 1, C, dtype=F64)
    for s in range(9):
        i, j = divmod(s, 3)
        pad[:, i:i + 2 * Hp:2, j:j + 2 * Wp:2] += torch.where(amax == s, g_out, torch.zeros_like(g_out))
    g = pad[:, 1:1 + Hc, 1:1 + Wc].clone()
    pad[:, 1:1 + Hc, 1:1 + Wc] = 0
    assert not bool(pad.any()), "an arg-max slot outside the frame: certify_amax comes first"
    n = N * Hc * Wc
    dbeta, dgamma = g.sum((0, 1, 2)), (g * xh).sum((0, 1, 2))
    dx = gamma.to(F64) * rstd.to(F64) * (g - dbeta / n - xh * (dgamma / n))
    t = g_out * xh_out
    return PoolBwd(_bf(dx) if rounded else dx, dgamma, dbeta, t.abs().sum((0, 1, 2)), g_out.abs().sum((0, 1, 2)),
                   (t * t).sum((0, 1, 2)).sqrt(), (g_out * g_out).sum((0, 1, 2)).sqrt())


def certify_amax(amax, y, xwin, x, a, eps: float) -> list:
    """The forward's arg-max judged on its own, for every pooled output: the slot lies inside the frame; a at the slot is within eps of the
    window maximum; y is a at the slot to one bf16 rounding (of a value eps away); xwin (or None) is bit-equal to x at the slot.
    x [N, Hc, Wc, C] bf16, a = pool_fwd(...)[1].  -> list of failures"""
    fails = []
    N, Hc, Wc, C = x.shape
    Hp, Wp = pooled_hw(Hc, Wc)
    am = amax.long()
    if int(am.max()) > 8:
        return [f"arg-max slot {int(am.max())} > 8"]
    h = 2 * torch.arange(Hp).view(1, Hp, 1, 1) - 1 + am // 3
    w = 2 * torch.arange(Wp).view(1, 1, Wp, 1) - 1 + am % 3
    inside = (h >= 0) & (h < Hc) & (w >= 0) & (w < Wc)
    if not bool(inside.all()):
        k = [int(v) for v in torch.nonzero(~inside)[0]]
        return [f"{int((~inside).sum())} arg-max slots lie outside the frame, first at (frame, ph, pw, channel) {k} slot {int(am[tuple(k)])}"]
    win = windows(a, -math.inf)
    at, top = _at_slot(win, amax), win.max(0).values
    short = top - at
    if not bool((short <= eps).all()):
        k = [int(v) for v in torch.nonzero(short > eps)[0]]
        fails.append(f"{int((short > eps).sum())} arg-max slots are not a window maximum, worst short by {float(short.max()):.3e} (eps {eps:.1e}), first {k}")
    off = (y.to(F64) - at).abs() - (2.0 ** -8 * (at.abs() + eps) + eps)          # half a unit in the last of 8 bits
    if not bool((off <= 0).all()):
        k = [int(v) for v in torch.nonzero(off > 0)[0]]
        fails.append(f"{int((off > 0).sum())} values of y are not act(z) at their slot to one bf16 rounding, worst over by {float(off.max()):.3e}, first {k}")
    if xwin is not None:
        want = _at_slot(windows(x.to(F64), 0.0), amax)
        if not torch.equal(xwin.to(F64), want):
            fails.append(f"xwin differs from x at the arg-max in {int((xwin.to(F64) != want).sum())} places")
    return fails


# ------------------------------------------------------------------------------------------------------------------------------------
# the activation formulas of csrc/common.h in fp32 (numpy), to measure the tie epsilon of the arg-max certificate
# ------------------------------------------------------------------------------------------------------------------------------------
def _expf(x):
    """__expf: exp2 of the fp32-rounded x * log2(e)"""
    f = np.float32
    return np.exp2((x.astype(f) * f(1.4426950408889634)).astype(f)).astype(f)


def act_f32(z, act: int):
    """gelu_erf (Abramowitz & Stegun 7.1.26 on |x|, mirrored) / swish of common.h, every operation rounded to fp32"""
    f = np.float32
    z = z.astype(f)
    if act == ACT_SWISH:
        return (z * (f(1.0) / (f(1.0) + _expf(-z))).astype(f)).astype(f)
    u = (np.abs(z) * f(0.70710678118654752440)).astype(f)
    t = (f(1.0) / (f(0.3275911) * u + f(1.0)).astype(f)).astype(f)
    ex = _expf(-(u * u).astype(f))
    poly = (t * f(1.061405429) + f(-1.453152027)).astype(f)
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = (t * poly + f(c)).astype(f)
    hp = (f(0.5) * (t * poly).astype(f)).astype(f)
    cdf = np.where(z >= 0, (f(1.0) - (hp * ex).astype(f)).astype(f), (hp * ex).astype(f))
    return (z * cdf).astype(f)


Z_RANGE = 8.0        # |z| of every pool case stays below this (asserted by the CPU test)


def measure_act_error(act: int) -> float:
    """max |formula in fp32 - float64 activation| over a dense grid of fp32 z in [-Z_RANGE, Z_RANGE]"""
    z = np.linspace(-Z_RANGE, Z_RANGE, 2_000_001).astype(np.float32)
    ref = act_fn(torch.from_numpy(z.astype(np.float64)), act).numpy()
    return float(np.abs(act_f32(z, act).astype(np.float64) - ref).max())


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases.  Every case names the edge it crosses and, as data, the kernels it is meant to reach.
# ------------------------------------------------------------------------------------------------------------------------------------
class ConvCase(NamedTuple):
    name: str
    B: int
    T: int
    H: int
    W: int
    fwd: tuple          # forward kernels to run: "dma" (k_stem_conv_fwd_dma: W % 8 == 0, workspace given), "f4" (k_stem_conv_fwd, 16-byte fill:
                        # W % 4 == 0, at W % 8 == 0 with the workspace withheld), "scalar" (k_stem_conv_fwd, scalar fill: W % 4 == 2)
    wgrad: str          # what use_tr=True reaches: "pipe" (k_stem_conv_wgrad_pipe) or "tr" (k_stem_conv_wgrad<true>); use_tr=False is always
                        # k_stem_conv_wgrad<false>
    crosses: tuple      # of "fwd_cap" (more than 768 tiles), "wgrad_cap" (more than 512 row groups), "partial_tile" (HoWo % 128 != 0),
                        # "partial_group" (Ho % 4 != 0), "wop_pad" (Wo % 16 != 0), "short_T" (T < 5)
    edge: str


def _cc(name, B, T, H, W, fwd, wgrad, crosses, edge):
    return ConvCase(name, B, T, H, W, tuple(fwd.split("+")), wgrad, tuple(crosses.split("+")) if crosses else (), edge)


CONV_CASES = [
    # forward DMA path (and the direct kernel's 16-byte fill with the workspace withheld)
    _cc("dma-24x24", 2, 5, 24, 24, "dma+f4", "pipe", "partial_tile+wop_pad", "two tiles a frame, the second of 16 positions; both clips' frames 0, 1, T-2, T-1"),
    _cc("dma-8x8", 1, 1, 8, 8, "dma+f4", "pipe", "partial_tile+wop_pad+short_T", "the smallest frame: one tile of 16 positions, one frame, Wo = 4"),
    _cc("dma-16x40", 2, 2, 16, 40, "dma+f4", "pipe", "partial_tile+wop_pad+short_T", "a 32-position tail tile, Wo = 20 padded to 32"),
    _cc("dma-22x24", 1, 3, 22, 24, "dma+f4", "pipe", "partial_tile+partial_group+wop_pad+short_T", "HoWo = 132: a 4-position last tile that starts mid-row; Ho = 11"),
    # forward direct path, 16-byte fill
    _cc("f4-12x12", 2, 3, 12, 12, "f4", "pipe", "partial_tile+partial_group+wop_pad+short_T", "W % 8 == 4"),
    _cc("f4-22x44", 1, 4, 22, 44, "f4", "pipe", "partial_tile+partial_group+wop_pad+short_T", "W % 8 == 4, two tiles a frame (242 positions), rows split across tiles"),
    # forward direct path, scalar fill
    _cc("sc-10x14", 2, 3, 10, 14, "scalar", "tr", "partial_tile+partial_group+wop_pad+short_T", "W % 4 == 2"),
    _cc("sc-18x22", 1, 5, 18, 22, "scalar", "tr", "partial_tile+partial_group+wop_pad", "W % 4 == 2, T = 5: every frame sees temporal padding but the middle one"),
    # T below the temporal kernel: B*T = 2, 4, 6 (and 8) frames that all see both clips' zero padding
    _cc("T1-8x8", 2, 1, 8, 8, "dma+f4", "pipe", "partial_tile+wop_pad+short_T", "T = 1: each frame is a clip"),
    _cc("T2-8x8", 2, 2, 8, 8, "dma+f4", "pipe", "partial_tile+wop_pad+short_T", "T = 2"),
    _cc("T3-8x8", 2, 3, 8, 8, "dma+f4", "pipe", "partial_tile+wop_pad+short_T", "T = 3"),
    _cc("T4-8x8", 2, 4, 8, 8, "dma+f4", "pipe", "partial_tile+wop_pad+short_T", "T = 4"),
    _cc("T1-8x10", 2, 1, 8, 10, "scalar", "tr", "partial_tile+wop_pad+short_T", "T = 1, scalar fill"),
    _cc("T3-8x10", 2, 3, 8, 10, "scalar", "tr", "partial_tile+wop_pad+short_T", "T = 3, scalar fill"),
    # the persistent-grid caps: 785 one-tile frames (768 + a ragged trip of 17), 1,570 row groups (512 x 3 + 34) of which every second is partial
    _cc("cap-12x8", 5, 157, 12, 8, "dma+f4", "pipe", "fwd_cap+wgrad_cap+partial_tile+partial_group+wop_pad", "both grid caps; Ho = 6"),
    # the boundary of the register-pipelined weight gradient (PW / 2 <= 32: W <= 96)
    _cc("pipe-96", 1, 3, 12, 96, "dma+f4", "pipe", "partial_tile+partial_group+short_T", "W = 96: the last piped shape, Wo = WoP = 48"),
    _cc("pipe-100", 1, 3, 12, 100, "f4", "tr", "partial_tile+partial_group+wop_pad+short_T", "W = 100: the first not piped (PW / 2 = 36)"),
    _cc("pipe-98", 1, 3, 12, 98, "scalar", "tr", "partial_tile+partial_group+wop_pad+short_T", "W = 98: W % 4 != 0"),
    # Wo against WoP (Wo = 4 is the 8-wide cases above)
    _cc("wop-15", 1, 2, 8, 30, "scalar", "tr", "partial_tile+wop_pad+short_T", "Wo = 15: one short of WoP = 16"),
    _cc("wop-16", 1, 2, 8, 32, "dma+f4", "pipe", "partial_tile+short_T", "Wo = 16 = WoP"),
    _cc("wop-17", 1, 2, 8, 34, "scalar", "tr", "partial_tile+wop_pad+short_T", "Wo = 17: WoP = 32, fifteen pad columns"),
]
ISOLATION_CASES = ("T3-8x8", "dma-24x24", "sc-10x14")       # clip isolation of the forward: every kernel, T below and at the temporal kernel


def conv_case(name: str) -> ConvCase:
    return next(c for c in CONV_CASES if c.name == name)


class FusedCase(NamedTuple):
    name: str
    B: int
    T: int
    H: int
    W: int
    act: int
    variant: str        # the instantiation of k_stem_bwd_wgrad: "6,6" or "6,8"
    edge: str


FUSED_CASES = [
    FusedCase("fused-T1", 2, 1, 12, 16, ACT_GELU, "6,6", "T = 1: every tap but kt = 2 is temporal padding"),
    FusedCase("fused-cap", 5, 157, 12, 8, ACT_SWISH, "6,6", "Ho % 4 != 0 together with 1,570 row groups on 512 workgroups"),
    FusedCase("fused-92", 1, 3, 12, 92, ACT_GELU, "6,6", "W = 92: the last shape of <6,6>"),
    FusedCase("fused-96", 1, 3, 12, 96, ACT_SWISH, "6,8", "W = 96: <6,8>, the last shape the fused pass takes"),
]


class PoolCase(NamedTuple):
    name: str
    N: int
    Hc: int
    Wc: int
    C: int
    form: str           # svsr_stem_bn_act_pool_bwd's form: "gather" (k_stem_bwd_reduce_gather, or k_stem_bwd_reduce_win when the forward's winners are
                        # passed; apply by k_stem_bwd_lds: C = 64, Wc <= 56), "lds" (k_stem_bwd_lds for both passes: Wc <= 128), "plain"
                        # (k_stem_pool_bwd_reduce / _apply)
    edge: str


POOL_CASES = [
    PoolCase("g-8x8", 2, 8, 8, 64, "gather", "even Hc and Wc: the last row and column are in one window only"),
    PoolCase("g-11x9", 3, 11, 9, 64, "gather", "odd Hc and Wc: the last pooled row and column hang over the frame"),
    PoolCase("g-50x12", 2, 50, 12, 64, "gather", "Hp = 25: two winner groups (STEM_GPW = 24), the second holding one row; seven gather groups, the last of one row"),
    PoolCase("g-9x56", 2, 9, 56, 64, "gather", "Wc = 56: the last gather width"),
    PoolCase("g-1x9", 2, 1, 9, 64, "gather", "Hc = 1: windows of one row"),
    PoolCase("g-2x8", 2, 2, 8, 64, "gather", "Hc = 2"),
    PoolCase("l-9x58", 2, 9, 58, 64, "lds", "Wc = 58: the first width past the gather form; two row blocks (STEM_BR = 8), the second of one row"),
    PoolCase("l-17x128", 1, 17, 128, 64, "lds", "Wc = 128: the last LDS width (60 KiB of pooled rows); three row blocks"),
    PoolCase("l-2x59", 2, 2, 59, 64, "lds", "Hc = 2 and odd Wc"),
    PoolCase("l-12x12-c128", 2, 12, 12, 128, "lds", "C = 128: not the gather form whatever the width; 16 channel groups"),
    PoolCase("p-9x130", 2, 9, 130, 64, "plain", "Wc = 130: the first plain width, one row per workgroup (rpb = 1)"),
    PoolCase("p-5x132", 1, 5, 132, 64, "plain", "Wc = 132, one frame"),
    PoolCase("p-1x131", 2, 1, 131, 64, "plain", "Hc = 1 and odd Wc"),
]


def pool_case(name: str) -> PoolCase:
    return next(c for c in POOL_CASES if c.name == name)


def pool_forms(c: PoolCase) -> tuple:
    """the backward runs of a case: (label, winners passed)"""
    return (("gather", False), ("win", True)) if c.form == "gather" else ((c.form, False),)


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs and shared references (computed once; callers do not modify them)
# ------------------------------------------------------------------------------------------------------------------------------------
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100000


@functools.lru_cache(maxsize=None)
def conv_inputs(name: str, kind: str) -> dict:
    """kind "int": clip and weights from {-1, 0, 1} (every output an integer of at most 245: exact in bf16 and in every fp32 partial sum);
    "random": a normal clip (fp32, NOT rounded: the kernels round), weights uniform in +-0.1, dy normal in bf16"""
    c = conv_case(name)
    g = _gen(_seed(c.name) + (7 if kind == "int" else 0))
    if kind == "int":
        vid = torch.randint(-1, 2, (c.B, c.T, c.H, c.W), generator=g).float()
        w = torch.randint(-1, 2, (C_OUT, 5, 7, 7), generator=g).float()
        return dict(vid=vid, w=w)
    vid = torch.randn(c.B, c.T, c.H, c.W, generator=g)
    w = (torch.rand(C_OUT, 5, 7, 7, generator=g) - 0.5) * 0.2
    dy = torch.randn(c.B * c.T, c.H // 2, c.W // 2, C_OUT, generator=g).to(BF)
    return dict(vid=vid, w=w, dy=dy)


@functools.lru_cache(maxsize=None)
def conv_reference(name: str, kind: str) -> dict:
    """out / sum / sumsq of the forward and, for "random", dw with the fp32 summation bounds of the sums and of dw"""
    c, x = conv_case(name), conv_inputs(name, kind)
    pat = patches(x["vid"])
    out, s, q = stem_conv_fwd(x["vid"], x["w"], pat=pat)
    ref = dict(out=out, sum=s, sumsq=q)
    n = out.shape[0] * out.shape[1] * out.shape[2]
    # a position's accumulator is off by at most 245 * 2^-24 * sum |w x| of its own terms; the row sums add n of them
    mag = pat.abs() @ _bf(x["w"]).reshape(C_OUT, TAPS).abs().t()
    ref["sum_bound"] = (TAPS + n) * 2.0 ** -24 * mag.sum((0, 1, 2))
    ref["sumsq_bound"] = (2 * TAPS + n + 1) * 2.0 ** -24 * (mag * mag).sum((0, 1, 2))
    if kind == "random":
        ref["dw"] = stem_conv_wgrad(x["vid"], x["dy"], pat=pat)
        ref["dw_bound"] = n * 2.0 ** -24 * stem_conv_wgrad(x["vid"].abs(), x["dy"].float().abs(), pat=pat.abs())
    return ref


def impulse_positions(c: ConvCase) -> list:
    """Up to 64 output positions (clip, frame, row, column), one per channel: the frame corners, the first row of the last (partial) 4-row
    group, the last column, at frames 0, 1, T-2, T-1 of the first and the last clip; past the grid cap also frames whose row groups a second,
    third and fourth persistent trip own"""
    Ho, Wo = c.H // 2, c.W // 2
    ts = sorted({0, 1, c.T - 2, c.T - 1} & set(range(c.T)))
    bs = sorted({0, c.B - 1})
    ys = sorted({0, (Ho - 1) // SW_RB * SW_RB, Ho - 1})
    xs = sorted({0, Wo // 2, Wo - 1})
    cand = [(b, t, y, x) for b in bs for t in ts for y in ys for x in xs]
    first = []
    gpf = (Ho + SW_RB - 1) // SW_RB
    if gpf * c.B * c.T > WGRAD_CAP:
        for grp in (WGRAD_CAP - 1, WGRAD_CAP, 2 * WGRAD_CAP + 1, gpf * c.B * c.T - 1):
            f = grp // gpf
            first += [(f // c.T, f % c.T, min(Ho - 1, (grp % gpf) * SW_RB + 1), Wo - 1)]
    cand = [p for p in cand if p not in first]
    room = C_OUT - len(first)
    if len(cand) > room:
        cand = [cand[round(i * (len(cand) - 1) / (room - 1))] for i in range(room)]
    return first + cand


def impulse_case(name: str) -> tuple:
    """-> (clip [B, T, H, W] fp32 with no zero in it, dy [B*T, Ho, Wo, 64] bf16 of one 1.0 per channel, dw [64, 5, 7, 7] float64: the clip's bf16
    pixels under each impulse, 0 outside the frame and the clip)"""
    c = conv_case(name)
    vid = conv_inputs(name, "random")["vid"]
    Ho, Wo = c.H // 2, c.W // 2
    vp = torch.zeros(c.B, c.T + 4, c.H + 6, c.W + 6, dtype=F64)
    vp[:, 2:2 + c.T, 3:3 + c.H, 3:3 + c.W] = _bf(vid)
    dy = torch.zeros(c.B * c.T, Ho, Wo, C_OUT, dtype=BF)
    dw = torch.zeros(C_OUT, 5, 7, 7, dtype=F64)
    for ch, (b, t, y, x) in enumerate(impulse_positions(c)):
        dy[b * c.T + t, y, x, ch] = 1.0
        dw[ch] = vp[b, t:t + 5, 2 * y:2 * y + 7, 2 * x:2 * x + 7]
    return vid, dy, dw


@functools.lru_cache(maxsize=None)
def pool_inputs(name: str) -> dict:
    """x = 1.5 * normal in bf16, mean / rstd its batch statistics (fp32), gamma = 1 + 0.2 normal, beta = 0.2 normal, dpool normal in bf16"""
    c = pool_case(name)
    g = _gen(_seed(c.name))
    x = (1.5 * torch.randn(c.N, c.Hc, c.Wc, c.C, generator=g)).to(BF)
    gamma, beta = 1 + 0.2 * torch.randn(c.C, generator=g), 0.2 * torch.randn(c.C, generator=g)
    xf = x.float()
    mean, rstd = xf.mean((0, 1, 2)), torch.rsqrt(xf.var((0, 1, 2), unbiased=False) + 1e-5)
    Hp, Wp = pooled_hw(c.Hc, c.Wc)
    dpool = torch.randn(c.N, Hp, Wp, c.C, generator=g).to(BF)
    return dict(x=x, mean=mean, rstd=rstd, gamma=gamma, beta=beta, dpool=dpool)


@functools.lru_cache(maxsize=None)
def pool_reference(name: str, act: int) -> tuple:
    x = pool_inputs(name)
    return pool_fwd(x["x"], x["mean"], x["rstd"], x["gamma"], x["beta"], act)


def reference_amax(a: torch.Tensor) -> torch.Tensor:
    """the first maximum in window order (torch's max_pool rule), for the CPU tests, which have no kernel arg-max"""
    return windows(a, -math.inf).max(0).indices.to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------------------------
# tolerances
# ------------------------------------------------------------------------------------------------------------------------------------
# bf16 outputs, per position (row_check over the 64 channels of a pixel): the worst error of rounded=True against rounded=False over the
# case lists above (both activations, both backward forms), as tests/test_stem_restatement_cpu.py measures it — recorded up to 2 % above
# the measurement.  What the rounded restatement does not reproduce (fp32 summation order, the erf / exp formulas) is covered by FACTOR.
ROUNDING = {
    "out": 2.49e-3,      # cap-12x8, frame 646 row 5 column 0: one bf16 rounding of each channel (at most 2^-8 of it)
    "y": 2.36e-3,        # p-1x131, Swish, frame 0 pooled column 65
    "dx": 6.63e-3,       # g-50x12, Swish, winner form (g and dx both rounded), frame 1 row 17 column 6
}
FACTOR = 4.0
# ... capped at the whole-tensor max-abs bound tests/test_gpu_kernels.py uses for the same tensor (check()'s default for the convolution output
# and y, 2e-2 for a BatchNorm dx); the relative L2 bounds of the same calls (6e-3, 6e-3, 8e-3) are asserted over the whole tensor beside it
CAP = {"out": 1.5e-2, "y": 1.5e-2, "dx": 2e-2}
WHOLE_BOUND = {"out": 6e-3, "y": 6e-3, "dx": 8e-3}
# the effect of keeping g in bf16 on dgamma / dbeta (winner form), as a multiple of sqrt(sum of squared terms) of the channel: worst over the
# gather cases and both activations, measured and recorded as above
G_ROUNDING = 5.87e-3       # g-11x9, GELU
# |fp32 formula of common.h - float64 activation| over |z| <= Z_RANGE (measure_act_error; the erf formula's own bound is 1.5e-7 on the CDF,
# times |z| in the GELU), recorded as above; Swish: one rounding of 1 + exp(-z) and one of the reciprocal, times |z|
ACT_ERROR = {ACT_GELU: 4.27e-7, ACT_SWISH: 9.29e-7}
# z itself is x * (gamma * rstd) + (beta - mean * gamma * rstd) in fp32: four roundings of terms below Z_TERMS (asserted by the CPU test), and
# both activations have |act'| <= 1.13
Z_TERMS = 8.0
Z_ERROR = 1.13 * 4 * 2.0 ** -24 * Z_TERMS


def tolerance(name: str) -> float:
    return min(FACTOR * ROUNDING[name], CAP[name])


def tie_eps(act: int) -> float:
    """two window candidates whose activations are closer than this may resolve either way (both carry the formula's error)"""
    return 2.0 * (ACT_ERROR[act] + Z_ERROR)


def sum_tolerance(bound: torch.Tensor) -> torch.Tensor:
    """fp32 sums (dw, the BatchNorm partial sums, dgamma, dbeta): FACTOR x the summation bound n * 2^-24 * sum |terms| of each element"""
    return FACTOR * bound


def pool_sum_tolerance(c: PoolCase, r: PoolBwd, win: bool) -> tuple:
    """-> (tolerance of dgamma [C], of dbeta [C])"""
    n = c.N * c.Hc * c.Wc
    k = FACTOR * G_ROUNDING if win else 0.0
    return FACTOR * n * 2.0 ** -24 * r.abs_gx + k * r.rss_gx, FACTOR * n * 2.0 ** -24 * r.abs_g + k * r.rss_g


def bound_check(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> tuple:
    """-> (worst |got - ref| / tol, flat index); an element whose tolerance is 0 must be equal"""
    err = (got.to(F64) - ref.to(F64)).abs().flatten()
    tol = tol.to(F64).flatten()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    i = int(ratio.argmax())
    return float(ratio[i]), i
