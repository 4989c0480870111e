"""Float64 restatements of the contraction kernels (igemm_fwd.hip, igemm_p8.hip, conv3x3_c64.hip, igemm_wgrad.hip, wgrad3x3.hip) on EXACT
operands, and the comparison helpers of tests/test_gpu_contraction_edges.py.  CPU only.

The exact method.  The contraction is linear.  Operands are small integers stored as bf16; `exact_budget` bounds, per output kind, the sum of
|products| behind any output element.  While that stays below 2^24 every fp32 partial sum — in the MFMA's order, the ring order, K groups,
split-K slabs, unit lists, chained reduces — is an integer fp32 represents exactly, so an fp32 output must equal the integer reference bit
for bit and a bf16 output its round-to-nearest-even (common.h f2bf is RNE, which is torch's cast).  Scales (alpha, gscale, rstd, gamma) are
powers of two and bias / addend / mean / beta small integers, so the epilogues stay exact too.  `assert_bits` is the only check of every
linear output.

The two non-linear epilogues (`assert_close_rows`), bounds counted from the code.  A bf16 rounding (RNE to 8 significant bits) moves a value
by at most half an ulp of its binade, halfulp(v) = 2^(floor(log2|v|) - 8): 2^-9 relative at the top of the binade, 2^-8 at its bottom.  The
checks use the half ulp of the element's own binade, never the looser 2^-8 * |v|.

* GELU `out` (igemm_fwd.hip igemm_epilogue, act == 1): v = acc + bias is exact; out = bf16(gelu_erf(v)) — ONE bf16 rounding at the output.
  gelu_erf(v) = v * Phi(v) in fp32 (common.h normal_cdf_exp): the A&S 7.1.26 erfc has |error| <= 1.5e-7, i.e. 0.75e-7 in Phi; v_rcp_f32, v_exp_f32, five fmas, three multiplies and the mirror subtraction cost at most 16 fp32 half-ulps of values <= 1
  (16 * 2^-24 = 0.95e-6).  So with e = |v| * (0.75e-7 + 16 * 2^-24):  |out - gelu(v)| <= halfulp(|gelu(v)| + e) + e.
  At |v| <= 64 that is at most 3.9e-3 * |ref| + 6.6e-5: 3.8x tighter than the 1.5e-2 * max|ref| of tests/test_gpu_kernels.py, and relative to
  the element instead of the tensor's maximum.  `out_pre` = bf16(v) stays on assert_bits.
* Swish BatchNorm-backward (igemm_epilogue, bnb_act == 2): g = bf16(bf16(d) * swish_grad(z)), d = dgrad + addend exact, z = fma(x, sc, sh)
  (+ r) exact for integer x, r, mean, beta and power-of-two gamma, rstd.  bf16(d) is the RNE of an integer: restated exactly (gb).  Then ONE
  more bf16 rounding of gb * swish_grad(z); swish_grad = s * (1 + z * (1 - s)), s = rcp(1 + exp(-z)): v_exp_f32 and
  v_rcp_f32 (<= 2 ulp together in s, |s| <= 1), then four fp32 operations whose operands are bounded by 1 + |z|: absolute error
  <= (2 + |z|) * 8 * 2^-24.  So with e = |gb| * (2 + |z|) * 8 * 2^-24:  |g - gb * swish'(z)| <= halfulp(|ref| + e) + e.
  Its two column sums add non-integer bf16 values in fp32: against the float64 sums of the kernel's OWN g (and g * (x - mean) * rstd, exact
  per term) the sequential-summation bound rows * 2^-24 * sum|terms| holds per column, whatever the order.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

BF = torch.bfloat16
F64 = torch.float64
LIMIT = float(1 << 24)
SENT16 = 0x7F5B                 # bf16 NaN pattern no kernel produces from finite operands
SENT32 = 0x7FC5A5A5             # fp32 NaN pattern
SPARE_ROWS = 3
STAT_SPARE = 1024               # floats watched behind the last statistics row


# ---------------------------------------------------------------------------------------------------------------------
# exact operands
# ---------------------------------------------------------------------------------------------------------------------
def exact(shape, seed: int, values=(-1, 1), zero: float = 0.5) -> torch.Tensor:
    """bf16 tensor of small integers: 0 with probability `zero`, else uniform over `values`."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(values, dtype=torch.float32)
    pick = vals[torch.randint(0, len(values), shape, generator=g)]
    keep = torch.rand(shape, generator=g) >= zero
    return (pick * keep).to(BF)


def rne_bf16(t: torch.Tensor) -> torch.Tensor:
    """float64 integers (< 2^24: exact in fp32) -> the bf16 the kernels store, back in float64"""
    return t.float().to(BF).to(F64)


def _nchw(t):
    return t.to(F64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def out_size(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


# ---------------------------------------------------------------------------------------------------------------------
# restatements (float64 in, float64 out; NHWC activations, weights [Co][k][k][Ci])
# ---------------------------------------------------------------------------------------------------------------------
def conv_fwd(x, w, s: int, p: int):
    return _nhwc(F.conv2d(_nchw(x), w.to(F64).permute(0, 3, 1, 2), stride=s, padding=p))


def fwd_stats(acc):
    """BatchNorm partials of a forward: column sums of the fp32 accumulators and of their squares (NOT of the rounded output)"""
    a = acc.reshape(-1, acc.shape[-1])
    return torch.stack([a.sum(0), (a * a).sum(0)])


def epilogue(acc, bias=None, act: str = "none", alpha: float = 1.0, addend=None):
    """-> (out, pre): out = alpha * act(acc + bias) + addend; pre = acc + bias (what GELU launches also store)"""
    v = acc if bias is None else acc + bias.to(F64)
    pre = v
    if act == "relu":
        v = v.clamp_min(0)
    elif act == "gelu":
        v = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))
    v = v * alpha
    if addend is not None:
        v = v + addend.to(F64)
    return v, pre


def seq_rows(B: int, S: int, s0: int, n: int) -> torch.Tensor:
    """row indices b * S + s0 + j (j < n) of a [B * S, .] tensor, in dense [B * n] order"""
    return (torch.arange(B)[:, None] * S + s0 + torch.arange(n)[None, :]).reshape(-1)


def linear(x, w, seq=None):
    """x [R, K] @ w[N, K]^T; seq = (S, s0, n): gathers rows s0..s0+n-1 of every length-S sequence"""
    x = x.to(F64)
    if seq is not None:
        S, s0, n = seq
        x = x[seq_rows(x.shape[0] // S, S, s0, n)]
    return x @ w.to(F64).t()


def conv_dgrad(dy, w, s: int, p: int, hw):
    H, W = hw
    k = w.shape[1]
    Ho, Wo = dy.shape[1:3]
    oph, opw = H - ((Ho - 1) * s - 2 * p + k), W - ((Wo - 1) * s - 2 * p + k)
    return _nhwc(F.conv_transpose2d(_nchw(dy), w.to(F64).permute(0, 3, 1, 2), stride=s, padding=p, output_padding=(oph, opw)))


def dgrad_reach(k: int, s: int, p: int, hw) -> torch.Tensor:
    """[H, W] bool: the pixels of dx some tap reaches (the others: 0 + addend in mode 1, untouched in mode 2)"""
    H, W = hw
    one = torch.ones(1, out_size(H, k, s, p), out_size(W, k, s, p), 1, dtype=F64)
    return conv_dgrad(one, torch.ones(1, k, k, 1, dtype=F64), s, p, hw)[0, :, :, 0] > 0


def bn_mask(x, mean, rstd, gamma, beta):
    sc = gamma.to(F64) * rstd.to(F64)
    return x.to(F64) * sc + (beta.to(F64) - mean.to(F64) * sc) > 0


def dgrad_bn_relu(d, mask, x, mean, rstd, scale: float = 1.0):
    """d = dgrad (+ addend), exact.  -> g = mask ? bf16(bf16(d) * scale) : 0 (g is rounded BEFORE it enters the sums), sum g, sum g * xhat"""
    g = torch.where(mask, rne_bf16(rne_bf16(d) * scale), torch.zeros_like(d))
    xh = (x.to(F64) - mean.to(F64)) * rstd.to(F64)
    C = d.shape[-1]
    return g, torch.stack([g.reshape(-1, C).sum(0), (g * xh).reshape(-1, C).sum(0)])


def swish_grad(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def dgrad_bn_swish(d, x, mean, rstd, gamma, beta, res=None):
    """-> (g unrounded = bf16(d) * swish'(z), gb, z)"""
    sc = gamma.to(F64) * rstd.to(F64)
    z = x.to(F64) * sc + (beta.to(F64) - mean.to(F64) * sc)
    if res is not None:
        z = z + res.to(F64)
    gb = rne_bf16(d)
    return gb * swish_grad(z), gb, z


def conv_wgrad(x, dy, k: int, s: int, p: int):
    """dw [Co][k][k][Ci] = sum dy[n,a,b,co] * x[n, a*s+kh-p, b*s+kw-p, ci], tap by tap"""
    x, dy = x.to(F64), dy.to(F64)
    N, H, W, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    xp = F.pad(x, (0, 0, p, p, p, p))
    dw = torch.zeros(Co, k, k, Ci, dtype=F64)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
            dw[:, kh, kw] = torch.einsum("nabo,nabi->oi", dy, xs)
    return dw


def linear_wgrad(x, dy, seq=None):
    x = x.to(F64)
    if seq is not None:
        S, s0, n = seq
        x = x[seq_rows(x.shape[0] // S, S, s0, n)]
    dy = dy.to(F64)
    return dy.t() @ x, dy.sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# the 2^24 condition
# ---------------------------------------------------------------------------------------------------------------------
def exact_budget(case) -> dict:
    """{output kind: largest sum of |products| behind one of its elements} of a case of tests/contraction_cases.py — the statistics count as
    kinds (sum(out^2) per column); the table is valid only while every value is below 2^24 (LIMIT)"""
    import contraction_cases

    return budget_of(contraction_cases.build(case)["abs"])


def budget_of(kind_to_abs: dict) -> dict:
    """{output kind: tensor of sum-of-|products| per element} -> {kind: its maximum}"""
    return {k: float(v.abs().max()) if v.numel() else 0.0 for k, v in kind_to_abs.items()}


# ---------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    if t.dtype == BF:
        b = t.view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(b == 0x8000, torch.zeros_like(b), b)          # -0 == +0
    assert t.dtype == torch.float32, t.dtype
    b = t.view(torch.int32)
    return torch.where(b == -(1 << 31), torch.zeros_like(b), b)


def as_dtype(ref: torch.Tensor, dtype) -> torch.Tensor:
    """float64 exact reference -> the stored format (RNE)"""
    return ref.float().to(dtype)


def assert_bits(got: torch.Tensor, ref: torch.Tensor, what: str, where=None) -> None:
    """Element-wise bit equality of a [rows, columns] (or [..., columns]) tensor with the reference in the same dtype (a float64 reference is
    cast RNE first).  `where(row, col) -> str` names the tile / tap class / split a wrong element falls in."""
    got = got.detach().cpu()
    if ref.dtype == F64:
        ref = as_dtype(ref, got.dtype)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = (_bits(got) != _bits(ref)).reshape(-1, got.shape[-1]) if got.ndim > 1 else (_bits(got) != _bits(ref)).reshape(1, -1)
    n = int(bad.sum())
    if n:
        r, c = (int(v) for v in bad.nonzero()[0])
        g2, r2 = got.reshape(bad.shape), ref.reshape(bad.shape)
        rows_hit = int(bad.any(1).sum())
        place = f" [{where(r, c)}]" if where is not None else ""
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ in bits ({rows_hit} rows); first at (row {r}, column {c}){place}: "
                             f"got {float(g2[r, c])!r}, want {float(r2[r, c])!r}")


def assert_close_rows(got: torch.Tensor, ref: torch.Tensor, slack: torch.Tensor, what: str) -> None:
    """|got - ref| <= half a bf16 ulp of (|ref| + slack) + slack per element: one bf16 rounding of a value the fp32 path knows to within
    `slack` (module docstring).  ref, slack float64."""
    g = got.detach().cpu().to(F64)
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite values"
    err = (g - ref).abs()
    mag = (ref.abs() + slack).clamp_min(2.0 ** -126)
    tol = 2.0 ** (torch.floor(torch.log2(mag)) - 8) + slack          # half a bf16 ulp of the element's binade (8 significant bits)
    bad = (err > tol).reshape(-1, g.shape[-1])
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the derived bound; first at (row {r}, column {c}): got "
                             f"{float(g.reshape(bad.shape)[r, c])!r}, want {float(ref.reshape(bad.shape)[r, c])!r}, bound {float(tol.reshape(bad.shape)[r, c]):.3e}")


def gelu_slack(pre: torch.Tensor) -> torch.Tensor:
    return pre.abs() * (0.75e-7 + 16 * 2.0 ** -24)


def swish_slack(gb: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    return gb.abs() * (2 + z.abs()) * 8 * 2.0 ** -24


def assert_sum_rows(got_sum: torch.Tensor, terms: torch.Tensor, what: str) -> None:
    """fp32 column sums of non-integer terms [rows, C] (float64, exact per term) in any order: |sum - sum64| <= rows * 2^-24 * sum|terms|"""
    ref = terms.sum(0)
    tol = terms.shape[0] * 2.0 ** -24 * terms.abs().sum(0) + 1e-30
    err = (got_sum.detach().cpu().to(F64) - ref).abs()
    assert bool((err <= tol).all()), f"{what}: column {int((err > tol).nonzero()[0])} off by {float(err.max()):.3e} (bound {float(tol.min()):.3e})"


# ---------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------
def guarded(rows: int, cols: int, pitch: int, dtype, dev, fill=None):
    """-> (buffer [rows + SPARE_ROWS, pitch] full of sentinels, its [rows, cols] corner).  The kernel gets the buffer's address and `pitch`."""
    assert pitch >= cols
    if dtype == BF:
        buf = torch.full((rows + SPARE_ROWS, pitch), SENT16, dtype=torch.int16, device=dev).view(BF)
    else:
        buf = torch.full((rows + SPARE_ROWS, pitch), SENT32, dtype=torch.int32, device=dev).view(torch.float32)
    if fill is not None:
        buf[:rows, :cols] = fill.to(dev).to(dtype)
    return buf, buf[:rows, :cols]


def sentinel_mask(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu()
    return (t.view(torch.int16) == SENT16) if t.dtype == BF else (t.view(torch.int32) == SENT32)


def assert_guard(buf: torch.Tensor, rows: int, cols: int, what: str) -> None:
    m = sentinel_mask(buf)
    assert bool(m[rows:].all()), f"{what}: {int((~m[rows:]).sum())} elements of the spare rows behind row {rows - 1} were written"
    assert bool(m[:, cols:].all()), f"{what}: {int((~m[:, cols:]).sum())} elements of the spare columns behind column {cols - 1} were written"


def assert_untouched(t: torch.Tensor, what: str) -> None:
    m = sentinel_mask(t)
    assert bool(m.all()), f"{what}: {int((~m).sum())} sentinel elements were written, first at flat index {int((~m).reshape(-1).nonzero()[0])}"
