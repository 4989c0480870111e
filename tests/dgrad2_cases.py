"""Cases, operands, float64 restatement and plan census of the merged downsample-block data gradient (svsr_igemm_dgrad2 / svsr_igemm_dgrad2_bn,
svsr_conv_plan mode 3): shared by tests/test_dgrad2_restatement_cpu.py and tests/test_gpu_dgrad2_edges.py.  The exact method, the comparison
helpers and the guard bands are those of tests/contraction_restatement.py.

The contraction runs over `planes` (the block's output channels), the launch writes `ci_in` (its input channels).  The kernels contract in
64-channel steps, so — as the dense layers of the library do for a width that is no multiple of 64 — planes = 16 and 136 travel zero-padded to
64 and 192 channels: dy, dy2 and both transposed weights are allocated with `kp` channels and hold zeros behind `planes`."""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass, field

import contraction_cases as cc
import contraction_restatement as R

GLDS = cc.GLDS
TAP2 = 9                       # IGEMM_TAP2 of csrc/igemm_fwd.h: the tap word of the second operand pair
CHANNELS = ((16, 8), (128, 64), (136, 72), (256, 128))          # planes -> ci_in: Co <= 64, > 64, and no multiple of the 64-wide column group
MAPS = ((4, 4), (5, 5), (6, 7), (7, 6), (2, 2))
EPILOGUES = ("plain", "relu", "swish")
# every instantiation svsr_igemm_dgrad2 can launch (igemm_fwd.hip igemm_fwd_run)
REQUIRED = (f"{GLDS}<64,64,4>", f"{GLDS}<64,64,4,2>", f"{GLDS}<64,64,3>", f"{GLDS}<128,64,2>", f"{GLDS}<128,128,2>",
            f"{GLDS}<64,64,4>+bn", f"{GLDS}<64,64,3>+bn", f"{GLDS}<128,64,2>+bn", f"{GLDS}<128,128,2>+bn")


@dataclass(frozen=True)
class Case:
    name: str
    N: int
    H: int
    W: int
    planes: int
    ci_in: int
    epi: str                      # plain | relu (mask read from y) | swish (residual input r)
    knobs: dict = field(default_factory=dict)
    label: str = ""               # "" = the small default: 64 x 64 tiles
    floats: bool = False          # N(0,1) operands: the error comparison, not the bit comparison

    @property
    def id(self) -> str:
        return self.name

    @property
    def kp(self) -> int:
        return -(-self.planes // 64) * 64

    @property
    def hw_out(self):
        return R.out_size(self.H, 3, 2, 1), R.out_size(self.W, 3, 2, 1)


def _cases() -> list:
    C = []
    for (H, W) in MAPS:
        for N in (1, 3):
            for planes, ci in CHANNELS:
                for epi in EPILOGUES:
                    C.append(Case(f"{H}x{W}_n{N}_{planes}to{ci}_{epi}", N, H, W, planes, ci, epi))
    # class row counts around a 128-row tile: a 2 x 256 map has column classes of 128 (even), 127 (odd, interior) and 1 (the last odd column)
    # pixels per row class, a 2 x 258 map 129, 128 and 1 — one below, at and one above the tile edge between them
    for W in (256, 258):
        for (planes, ci), knobs, lab in (((128, 64), {"igemm_tile": 128}, "<128,64,2>"), ((256, 128), cc.T128, "<128,128,2>")):
            for epi in EPILOGUES:
                C.append(Case(f"tile128_2x{W}_{planes}to{ci}_{epi}", 1, 2, W, planes, ci, epi, knobs, GLDS + lab + ("+bn" if epi != "plain" else "")))
    # more than 2.5 x 256 tiles of 64 rows: the 3-deep ring of the 64 x 64 tile
    for epi in ("plain", "relu"):
        C.append(Case(f"ns3_118x118_n3_64to8_{epi}", 3, 118, 118, 64, 8, epi, {"igemm_tile": 64}, f"{GLDS}<64,64,3>" + ("+bn" if epi != "plain" else "")))
    for epi in EPILOGUES:
        C.append(Case(f"float_12x12_n4_128to64_{epi}", 4, 12, 12, 128, 64, epi, floats=True))
    return C


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def expected_label(c: Case) -> str:
    if c.label:
        return c.label
    if c.epi == "plain" and 4 * (c.kp // 64) >= 12 and min(c.H, c.W) > 2:          # four-tap classes, K steps >= 12: the in-workgroup K split
        return f"{GLDS}<64,64,4,2>"
    return f"{GLDS}<64,64,4>" + ("+bn" if c.epi != "plain" else "")


def plan_words(mode: int, N: int, H: int, W: int, co_launch: int):
    """host-only: (words, meta) of svsr_conv_plan(mode, 3x3 / stride 2 / pad 1)"""
    lib = cc._lib()
    meta = (ctypes.c_int * 8)()
    n = lib.svsr_conv_plan(mode, N, H, W, co_launch, 3, 2, 1, None, 0, meta)
    assert n > 0, n
    words = (ctypes.c_int * n)()
    assert lib.svsr_conv_plan(mode, N, H, W, co_launch, 3, 2, 1, words, n, meta) == n
    return list(words), [int(v) for v in meta]


def plan_classes(words):
    """-> [(tap words, deltas, pixels per image, first tile, [(src, dst)])] in the plan's order"""
    ncls, pos0 = words[0] & 0xFFFF, words[1]
    out = []
    for c in range(ncls):
        w = words[2 + 24 * c: 2 + 24 * (c + 1)]
        nt, P, off, tile0 = w[0], w[1], w[2], w[3]
        pos = words[pos0 + 2 * off: pos0 + 2 * (off + P)]
        out.append((tuple(w[13:13 + nt]), tuple(w[4:4 + nt]), P, tile0, list(zip(pos[0::2], pos[1::2]))))
    return out


def census(H: int, W: int, merged: bool = True) -> dict:
    """Independent restatement: {tap words of a pixel of dx, in (kh, kw) order, TAP2 right behind the centre tap: [pixel indices]} of the 3x3 /
    stride 2 / pad 1 data gradient (+ the 1x1 / stride 2 branch, which reaches pixel (y, x) iff both are even)."""
    Ho, Wo = R.out_size(H, 3, 2, 1), R.out_size(W, 3, 2, 1)
    assert (Ho, Wo) == (R.out_size(H, 1, 2, 0), R.out_size(W, 1, 2, 0)), "both branches have the same output grid"
    cls: dict = {}
    for y in range(H):
        for x in range(W):
            key = []
            for kh in range(3):
                for kw in range(3):
                    if (y + 1 - kh) % 2 or (x + 1 - kw) % 2 or not (0 <= (y + 1 - kh) // 2 < Ho and 0 <= (x + 1 - kw) // 2 < Wo):
                        continue
                    key.append(kh * 3 + kw)
                    if merged and (kh, kw) == (1, 1):
                        assert y % 2 == 0 and x % 2 == 0
                        key.append(TAP2)
            if merged and y % 2 == 0 and x % 2 == 0:
                assert TAP2 in key, "the centre tap of an (even, even) pixel is always inside the grid"
            cls.setdefault(tuple(key), []).append(y * W + x)
    return cls


def build(c: Case) -> dict:
    """-> operands as the kernels take them (zero-padded to kp channels), the float64 references and the sums of |products|"""
    import torch

    seed = zlib.crc32(c.name.encode()) & 0xFFFF
    N, H, W, K, Kp, Ci = c.N, c.H, c.W, c.planes, c.kp, c.ci_in
    Ho, Wo = c.hw_out
    if c.floats:
        rn = lambda shape, k, s=1.0: (torch.randn(shape, generator=torch.Generator().manual_seed(seed + k)) * s).to(R.BF)
        dy, dy2, w3, w1 = rn((N, Ho, Wo, K), 1), rn((N, Ho, Wo, K), 3), rn((K, 3, 3, Ci), 2), rn((K, 1, 1, Ci), 4)
    else:
        dy, dy2 = R.exact((N, Ho, Wo, K), seed + 1), R.exact((N, Ho, Wo, K), seed + 3)
        w3, w1 = R.exact((K, 3, 3, Ci), seed + 2), R.exact((K, 1, 1, Ci), seed + 4)
    pad = lambda t: torch.cat([t, torch.zeros(*t.shape[:-1], Kp - K, dtype=t.dtype)], -1).contiguous() if Kp > K else t.contiguous()
    I = dict(dy=pad(dy), dy2=pad(dy2), wt=pad(w3.permute(3, 1, 2, 0)), wt2=pad(w1.permute(3, 1, 2, 0)).reshape(Ci, Kp))
    d3, d1 = R.conv_dgrad(dy, w3, 2, 1, (H, W)), R.conv_dgrad(dy2, w1, 2, 0, (H, W))
    d = {"in": I, "ref": {}, "abs": {}, "dxd": d1, "d": d3 + d1}
    dabs = R.conv_dgrad(dy.abs(), w3.abs(), 2, 1, (H, W)) + R.conv_dgrad(dy2.abs(), w1.abs(), 2, 0, (H, W))
    ref, ab = d["ref"], d["abs"]
    if c.epi == "plain":
        ref["out"], ab["out"] = d["d"], dabs
        return d
    ints = lambda shape, k, lo, hi: torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed + k)).float()
    pow2 = lambda shape, k: 2.0 ** torch.randint(-1, 2, shape, generator=torch.Generator().manual_seed(seed + k)).float()
    shape = (N, H, W, Ci)
    I["x"] = ints(shape, 11, -2, 2).to(R.BF)
    I["mean"], I["rstd"] = ints((Ci,), 12, -1, 1), pow2((Ci,), 13)
    I["gamma"], I["beta"] = pow2((Ci,), 14) * (1 - 2 * (torch.arange(Ci) % 3 == 0).float()), ints((Ci,), 15, -1, 1)
    I["y"] = ints(shape, 16, -1, 1).to(R.BF)          # ReLU: the block-below output (the mask); Swish: its residual input r
    ab["g"] = dabs
    if c.epi == "swish":
        ref["g_swish"], ref["gb"], ref["z"] = R.dgrad_bn_swish(d["d"], I["x"], I["mean"], I["rstd"], I["gamma"], I["beta"], I["y"])
        if c.floats:          # the unrounded value: bf16(d) inside dgrad_bn_swish is already one of the kernel's roundings
            sc = I["gamma"].double() * I["rstd"].double()
            z = I["x"].double() * sc + (I["beta"].double() - I["mean"].double() * sc) + I["y"].double()
            ref["g_float"] = d["d"] * R.swish_grad(z)
    else:
        mask = I["y"].double() > 0
        ref["g"], ref["sums"] = R.dgrad_bn_relu(d["d"], mask, I["x"], I["mean"], I["rstd"])
        ga = R.rne_bf16(dabs) if not c.floats else dabs
        xh = ((I["x"].double() - I["mean"].double()) * I["rstd"].double()).abs()
        ab["sum_g"], ab["sum_g_xhat"] = ga.reshape(-1, Ci).sum(0), (ga * xh).reshape(-1, Ci).sum(0)
        if c.floats:
            ref["g_float"] = torch.where(mask, d["d"], torch.zeros_like(d["d"]))
    return d
