"""The stem front-end kernels (syncvsr_amd/csrc/stem.hip: both forward kernels, the three weight-gradient kernels, the fused backward; the
stem passes of syncvsr_amd/csrc/norm_act.hip: pool forward, the four forms of the pool backward) against the float64 restatement of
tests/stem_restatement.py, at every path and edge of its case tables (tests/test_stem_restatement_cpu.py proves each case takes the path it
names):

  * exact, zero tolerance: the forward on clips and weights from {-1, 0, 1} (every output and every per-workgroup BatchNorm partial row an
    integer below 2^24) on the DMA-fed and on the direct kernel; the weight gradient of one 1.0 per channel at the frame corners, the last
    partial row group, the last column, the first and last two frames of the first and last clip and in row groups of the second to fourth
    persistent trip (dw is the clip's bf16 pixels under the impulse and exact zeros outside frame and clip) on <false>, <true> and _pipe;
    clip 0's output bits with clip 1 replaced and the reverse; the fused backward against the two-launch route at T = 1, past the grid cap
    with Ho % 4 != 0, W = 92 (<6,6>) and W = 96 (<6,8>); every entry point twice, same bits;
  * random data: the convolution output, y and dx per output position (the 64 channels of a pixel against that pixel's own norm:
    mha_restatement.row_check), dw per (channel, tap) and the BatchNorm sums, dgamma, dbeta per channel against their fp32 summation bounds;
    the forward's arg-max is certified on its own (stem_restatement.certify_amax) and dx is compared with the restatement fed that arg-max:
    no share of elements is exempt;
  * outputs are carved out of sentinel-filled buffers: nothing in front of the first element or past position Ho * Wo of the last frame
    is written;
  * refusals: odd or small H / W from every entry point, the LDS limits of the forward (W = 1394 direct, 1392 DMA-fed) and of the weight
    gradient (W = 290) one step past the last accepted shape, pooled sizes that do not belong to the frame, want_dx=False outside the gather form.

Tolerances (stem_restatement: ROUNDING measured on the CPU, x 4, capped at the whole-tensor bound tests/test_gpu_kernels.py uses):
  out 9.96e-3, y 9.44e-3, dx 2e-2 per position; whole-tensor 6e-3, 6e-3, 8e-3; sums 4 x n * 2^-24 * sum |terms| (+ 4 x 5.87e-3 of the root sum
  of squares for the bf16 g of the winner form); arg-max tie epsilon see stem_restatement.tie_eps.
Constants measured on the CPU: rounding per position out 2.458e-3, y 2.327e-3, dx 6.537e-3; bf16 g on dgamma / dbeta 5.789e-3 of the root sum
  of squares; activation formulas over |z| <= 8: GELU 4.21e-7, Swish 9.15e-7, plus 2.16e-6 for the fp32 z: tie epsilon 5.2e-6 / 6.2e-6.
Worst values seen on an MI355X (144 tests, 3.7 s; every exact case exact):
  out 2.458e-3 per position (cap-12x8, direct kernel, frame 646) and 1.68e-3 whole; y 2.33e-3; gpool 2.20e-3; dx 6.535e-3 per position (g-50x12,
  Swish, winner form) and 2.69e-3 whole; dw 1.6 % of its tolerance, the BatchNorm sums 0.03 %, dgamma 24 % and dbeta 23 % (g-11x9, winner form).

What the assertions were seen to catch (each mistake built once into a copy of the library, this module and the stem tests of
tests/test_gpu_kernels.py and tests/test_gpu_bench_shapes.py run once against it):
  * k_stem_conv_fwd bounds the temporal taps by the global frame index instead of the clip: 25 cases here (integer and random forward of every
    B = 2 shape on the direct kernel, the cap shape, all three clip-isolation cases); the existing tests pass - none of them runs that kernel.
  * the same in k_stem_conv_fwd_dma: 16 cases here; test_stem_conv (2 of 3) and test_stem_at_benchmark_batch fail as well.
  * k_stem_conv_wgrad skips the last partial row group: 18 cases here (impulses and random data of every Ho % 4 != 0 shape, on <false> and,
    where it is what use_tr reaches, <true>); the existing tests pass.
  * kw shifted by one in k_stem_conv_wgrad_pipe: 30 cases here (impulses, random data, all four fused-backward cases: the fused pass is
    compared with the piped route); the existing test_stem_conv, the fused test and the benchmark-batch test fail as well.
  * k_stem_bwd_reduce_win counts one pooled row too few in its second group: both g-50x12 backward cases here; the existing tests pass.
  * the right-edge window read twice in k_stem_pool_bwd_apply: p-9x130 and p-5x132, both activations; the existing tests pass.
  * forward loop stride gridDim.x - 1: 39 cases here, first at the partial row of workgroup 0; test_stem_conv fails as well."""
import math

import pytest
import torch

import stem_restatement as sr
from stem_restatement import BF, F64, bound_check, row_check

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B            # bf16 bit pattern of the guard elements (a finite value no kernel writes by accident)
GUARD = 4096                 # elements in front of and behind every carved output
F_SENTINEL = 12345.0


def _dev():
    return torch.device("cuda:0")


def _guarded(shape):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=_dev())
    return buf, buf[GUARD:GUARD + n].view(BF).view(shape)


def _assert_guard(buf, what: str):
    raw = buf.cpu()
    assert (raw[:GUARD] == SENTINEL).all(), f"{what}: elements in front of the first were written"
    assert (raw[-GUARD:] == SENTINEL).all(), f"{what}: elements past the last position of the last frame were written"


def _bits(t):
    return t.reshape(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == BF else t.dtype)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _per_position(tag, what, got, ref, fails):
    chk = row_check(what, got, ref)
    tol, whole = sr.tolerance(what), sr.WHOLE_BOUND[what]
    print(f"STEM-EDGE {tag} {what}: worst position {chk.worst:.3e} at {chk.where} (tol {tol:.3e}), whole {chk.whole:.3e} (bound {whole:.1e})")
    if not torch.isfinite(got.float()).all():
        fails.append(f"{tag} {what} holds NaN or infinity")
    if not chk.worst < tol:
        fails.append(f"{tag} {what}: position {chk.where} is off by {chk.worst:.3e} (tolerance {tol:.3e})")
    if not chk.whole < whole:
        fails.append(f"{tag} {what}: the whole tensor is off by {chk.whole:.3e} (bound {whole:.1e})")
    if chk.nonzero:
        fails.append(f"{tag} {what}: {chk.nonzero} positions are zero in the reference and not in the output (or hold NaN), first {chk.nonzero_where}")


def _bounded(tag, what, got, ref, tol, fails):
    worst, i = bound_check(got, ref, tol)
    print(f"STEM-EDGE {tag} {what}: worst element {worst:.3e} of its tolerance, flat index {i}")
    if not worst < 1.0:
        fails.append(f"{tag} {what}: element {i} is off by {worst:.3e} of its tolerance ({float(got.flatten()[i]):.6g} against {float(ref.flatten()[i]):.6g})")


# ------------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------------
def _fwd(c, path: str, vid, w):
    """-> out [B*T, Ho, Wo, 64] (CPU), the BatchNorm partial rows [rows, 2, 64] (CPU, float64); guards checked"""
    from syncvsr_amd import ops
    dev = _dev()
    buf, out = _guarded((c.B * c.T, c.H // 2, c.W // 2, 64))
    o, st = ops.stem_conv_fwd(vid.view(c.B, 1, c.T, c.H, c.W).to(dev), w.reshape(-1).to(dev), want_stats=True, use_ws=(path == "dma"), out=out)
    part, rows = st
    rows_t = part[: rows * 128].view(rows, 2, 64).cpu().to(F64)
    assert o.data_ptr() == out.data_ptr()
    _assert_guard(buf, f"{c.name} {path} out")
    tiles = (c.H // 2 * (c.W // 2) + 127) // 128 * c.B * c.T
    assert rows == min(tiles, sr.FWD_CAP)
    return out.cpu(), rows_t


def _tile_sums(c, ref_out, rows: int):
    """the reference's sum and sum of squares over the tiles each persistent workgroup owns: [rows, 2, 64]"""
    F_, Ho, Wo, C = ref_out.shape
    tpf = (Ho * Wo + 127) // 128
    flat = torch.zeros(F_, tpf * 128, C, dtype=F64)
    flat[:, : Ho * Wo] = ref_out.reshape(F_, Ho * Wo, C)
    t = flat.view(F_ * tpf, 128, C)
    per_tile = torch.stack([t.sum(1), (t * t).sum(1)], 1)
    return torch.stack([per_tile[r::rows].sum(0) for r in range(rows)])


@pytest.mark.parametrize("name", [c.name for c in sr.CONV_CASES])
def test_forward_on_integer_data_is_exact(name):
    """Every output element, every workgroup's partial row and the totals equal the reference exactly, on every forward kernel of the case; a
    second launch gives the same bits."""
    c, x, ref = sr.conv_case(name), sr.conv_inputs(name, "int"), sr.conv_reference(name, "int")
    fails = []
    for path in c.fwd:
        out, rows = _fwd(c, path, x["vid"], x["w"])
        out2, rows2 = _fwd(c, path, x["vid"], x["w"])
        bad = out.to(F64) != ref["out"]
        if bad.any():
            k = [int(v) for v in torch.nonzero(bad)[0]]
            fails.append(f"{path}: {int(bad.sum())} output elements differ, first (frame, y, x, channel) {k}: {float(out[tuple(k)])} against {float(ref['out'][tuple(k)])}")
        want = _tile_sums(c, ref["out"], rows.shape[0])
        if not torch.equal(rows, want):
            r = int(torch.nonzero((rows != want).flatten(1).any(1))[0])
            fails.append(f"{path}: the partial row of workgroup {r} (of {rows.shape[0]}) differs: sum off by {float((rows[r, 0] - want[r, 0]).abs().max())}, "
                         f"sum of squares by {float((rows[r, 1] - want[r, 1]).abs().max())}")
        if not (torch.equal(rows.sum(0)[0], ref["sum"]) and torch.equal(rows.sum(0)[1], ref["sumsq"])):
            fails.append(f"{path}: the per-channel totals differ")
        if not (_same(out, out2) and torch.equal(rows, rows2)):
            fails.append(f"{path}: two launches differ")
    assert not fails, f"{name}: " + "; ".join(fails)


@pytest.mark.parametrize("name", [c.name for c in sr.CONV_CASES])
def test_forward_on_random_data_every_position(name):
    c, x, ref = sr.conv_case(name), sr.conv_inputs(name, "random"), sr.conv_reference(name, "random")
    fails = []
    for path in c.fwd:
        out, rows = _fwd(c, path, x["vid"], x["w"])
        tag = f"{name} {path}"
        _per_position(tag, "out", out, ref["out"], fails)
        _bounded(tag, "stats.sum", rows.sum(0)[0], ref["sum"], sr.sum_tolerance(ref["sum_bound"]), fails)
        _bounded(tag, "stats.sumsq", rows.sum(0)[1], ref["sumsq"], sr.sum_tolerance(ref["sumsq_bound"]), fails)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("name", sr.ISOLATION_CASES)
def test_forward_clips_do_not_see_each_other(name):
    """B = 2: clip 0's output bits do not change when clip 1 holds other data, and the reverse"""
    c, x = sr.conv_case(name), sr.conv_inputs(name, "random")
    other = 3.0 * torch.randn(c.T, c.H, c.W, generator=torch.Generator().manual_seed(99)) + 1.0
    fails = []
    for path in c.fwd:
        base, _ = _fwd(c, path, x["vid"], x["w"])
        for clip in (0, 1):
            vid = x["vid"].clone()
            vid[clip] = other
            out, _ = _fwd(c, path, vid, x["w"])
            keep = slice((1 - clip) * c.T, (2 - clip) * c.T)
            if not _same(out[keep], base[keep]):
                bad = (_bits(out[keep]) != _bits(base[keep])).view(c.T, -1).any(1)
                fails.append(f"{path}: clip {1 - clip} changed with clip {clip}'s data, frames {[int(i) for i in torch.nonzero(bad).flatten()]}")
            if _same(out, base):
                fails.append(f"{path}: replacing clip {clip} changed nothing")
    assert not fails, f"{name}: " + "; ".join(fails)


# ------------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------------------------
def _wgrad(c, vid, dy, use_tr: bool):
    from syncvsr_amd import ops
    dev = _dev()
    n = 64 * 245
    buf = torch.full((n + 2 * GUARD,), F_SENTINEL, device=dev)
    dw = buf[GUARD:GUARD + n]
    dw.zero_()
    ops.stem_conv_wgrad(vid.view(c.B, 1, c.T, c.H, c.W).to(dev), dy.to(dev), dw, use_tr=use_tr)
    raw = buf.cpu()
    assert (raw[:GUARD] == F_SENTINEL).all() and (raw[-GUARD:] == F_SENTINEL).all(), f"{c.name} dw: written outside [64][245]"
    return raw[GUARD:GUARD + n].view(64, 5, 7, 7).clone()


def _wgrad_paths(c):
    return (("<false>", False), (c.wgrad, True))


@pytest.mark.parametrize("name", [c.name for c in sr.CONV_CASES])
def test_weight_gradient_of_impulses_is_the_clip_under_them(name):
    c = sr.conv_case(name)
    vid, dy, want = sr.impulse_case(name)
    pos = sr.impulse_positions(c)
    fails = []
    for label, use_tr in _wgrad_paths(c):
        dw = _wgrad(c, vid, dy, use_tr)
        bad = dw.to(F64) != want
        if bad.any():
            ch, kt, kh, kw = [int(v) for v in torch.nonzero(bad)[0]]
            where = pos[ch] if ch < len(pos) else None
            fails.append(f"{label}: {int(bad.sum())} taps differ in channels {sorted({int(v) for v in torch.nonzero(bad)[:, 0]})[:8]}, first channel {ch} "
                         f"(impulse at clip, frame, row, column {where}) tap ({kt}, {kh}, {kw}): {float(dw[ch, kt, kh, kw])} against {float(want[ch, kt, kh, kw])}")
        if not _same(dw, _wgrad(c, vid, dy, use_tr)):
            fails.append(f"{label}: two launches differ")
    assert not fails, f"{name}: " + "; ".join(fails)


@pytest.mark.parametrize("name", [c.name for c in sr.CONV_CASES])
def test_weight_gradient_on_random_data_every_tap(name):
    c, x, ref = sr.conv_case(name), sr.conv_inputs(name, "random"), sr.conv_reference(name, "random")
    fails = []
    for label, use_tr in _wgrad_paths(c):
        dw = _wgrad(c, x["vid"], x["dy"], use_tr)
        _bounded(f"{name} {label}", "dw", dw, ref["dw"], sr.sum_tolerance(ref["dw_bound"]), fails)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("name", [c.name for c in sr.FUSED_CASES])
def test_fused_backward_is_the_two_launch_route_bit_for_bit(name):
    from syncvsr_amd import ops
    c = next(k for k in sr.FUSED_CASES if k.name == name)
    dev, C, Ho, Wo = _dev(), 64, c.H // 2, c.W // 2
    g = torch.Generator().manual_seed(4321 + c.H + c.W)
    vid = torch.randn((c.B, 1, c.T, c.H, c.W), generator=g).to(dev)
    x = (1.5 * torch.randn((c.B * c.T, Ho, Wo, C), generator=g)).to(BF).to(dev)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(dev)
    beta = (0.2 * torch.randn(C, generator=g)).to(dev)
    xf = x.float()
    m, r = xf.mean((0, 1, 2)), torch.rsqrt(xf.var((0, 1, 2), unbiased=False) + 1e-5)
    y, amax, xwin = ops.stem_bn_gelu_pool_fwd(x, m, r, gamma, beta, act=c.act, want_win=True)
    dpool = torch.randn(tuple(y.shape), generator=g).to(BF).to(dev)
    assert ops.stem_bwd_wgrad_ok(vid)

    def two_launches():
        coef = torch.empty(3 * C, device=dev); dg = torch.zeros(C, device=dev); db = torch.zeros(C, device=dev)
        dx = ops.stem_bn_gelu_pool_bwd(dpool, amax, x, m, r, gamma, beta, coef, dg, db, act=c.act, xwin=xwin)
        dw = torch.zeros(64 * 245, device=dev)
        ops.stem_conv_wgrad(vid, dx, dw, use_tr=True)
        return coef, dg, db, dw

    def fused():
        coef = torch.empty(3 * C, device=dev); dg = torch.zeros(C, device=dev); db = torch.zeros(C, device=dev)
        gpool = ops.stem_bn_gelu_pool_bwd(dpool, amax, x, m, r, gamma, beta, coef, dg, db, act=c.act, xwin=xwin, want_dx=False)
        dw = torch.zeros(64 * 245, device=dev)
        ops.stem_bwd_wgrad(vid, gpool, amax, x, m, r, coef, dw)
        return coef, dg, db, dw

    a, b, b2 = two_launches(), fused(), fused()
    assert a[3].abs().max().item() > 0
    for n, u, v, v2 in zip(("coef", "dgamma", "dbeta", "dw"), a, b, b2):
        assert _same(u, v), f"{name}: {n} of the fused backward differs from the two-launch route, max |diff| {(u - v).abs().max().item():.3e} of {u.abs().max().item():.3e}"
        assert _same(v, v2), f"{name}: {n} differs between two fused launches"


# ------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + activation + max-pool
# ------------------------------------------------------------------------------------------------------------------------------------
def _pool_fwd(name: str, act: int):
    from syncvsr_amd import ops
    dev = _dev()
    c, x = sr.pool_case(name), sr.pool_inputs(name)
    d = {k: v.to(dev) for k, v in x.items()}
    Hp, Wp = sr.pooled_hw(c.Hc, c.Wc)
    buf, yout = _guarded((c.N, Hp, Wp, c.C))
    y, amax, xwin = ops.stem_bn_gelu_pool_fwd(d["x"], d["mean"], d["rstd"], d["gamma"], d["beta"], act=act, want_win=True, out=yout)
    torch.cuda.synchronize()
    _assert_guard(buf, f"{name} y")
    return d, y, amax, xwin


@pytest.mark.parametrize("act", sr.ACTS)
@pytest.mark.parametrize("name", [c.name for c in sr.POOL_CASES])
def test_pool_forward_every_position_and_its_argmax(name, act):
    from syncvsr_amd import ops
    x = sr.pool_inputs(name)
    d, y, amax, xwin = _pool_fwd(name, act)
    z, a, yref = sr.pool_reference(name, act)
    fails = sr.certify_amax(amax.cpu(), y.cpu(), xwin.cpu(), x["x"], a, sr.tie_eps(act))
    _per_position(f"{name} act{act}", "y", y.cpu(), yref, fails)
    y2, amax2 = ops.stem_bn_gelu_pool_fwd(d["x"], d["mean"], d["rstd"], d["gamma"], d["beta"], act=act)
    if not (_same(y, y2) and torch.equal(amax, amax2)):
        fails.append("the launch without xwin gives other bits")
    assert not fails, f"{name} act {act}: " + "; ".join(fails)


@pytest.mark.parametrize("act", sr.ACTS)
@pytest.mark.parametrize("name", [c.name for c in sr.POOL_CASES])
def test_pool_backward_every_position_with_the_kernels_argmax(name, act):
    """dx of every form against the restatement fed the kernel's (certified) arg-max, dgamma and dbeta per channel; the gather form is the one
    that accepts want_dx=False, every other form refuses it."""
    from syncvsr_amd import _lib, ops
    dev = _dev()
    c, x = sr.pool_case(name), sr.pool_inputs(name)
    d, y, amax, xwin = _pool_fwd(name, act)
    _, a, _ = sr.pool_reference(name, act)
    fails = sr.certify_amax(amax.cpu(), y.cpu(), xwin.cpu(), x["x"], a, sr.tie_eps(act))
    assert not fails, f"{name} act {act}: " + "; ".join(fails)
    ref = sr.pool_bwd(x["dpool"], amax.cpu(), x["x"], x["mean"], x["rstd"], x["gamma"], x["beta"], act)

    def run(win: bool, want_dx: bool = True):
        coef = torch.empty(3 * c.C, device=dev); dg = torch.zeros(c.C, device=dev); db = torch.zeros(c.C, device=dev)
        buf, dxout = _guarded(tuple(d["x"].shape))
        out = ops.stem_bn_gelu_pool_bwd(d["dpool"], amax, d["x"], d["mean"], d["rstd"], d["gamma"], d["beta"], coef, dg, db, act=act,
                                        xwin=xwin if win else None, want_dx=want_dx, out=dxout if want_dx else None)
        torch.cuda.synchronize()
        _assert_guard(buf, f"{name} dx")
        return out.cpu(), dg.cpu(), db.cpu(), coef.cpu()

    for label, win in sr.pool_forms(c):
        tag = f"{name} act{act} {label}"
        dx, dg, db, coef = run(win)
        _per_position(tag, "dx", dx, ref.dx, fails)
        tg, tb = sr.pool_sum_tolerance(c, ref, win)
        _bounded(tag, "dgamma", dg, ref.dgamma, tg, fails)
        _bounded(tag, "dbeta", db, ref.dbeta, tb, fails)
        again = run(win)
        if not all(_same(u, v) for u, v in zip((dx, dg, db, coef), again)):
            fails.append(f"{tag}: two launches differ")
    if c.form == "gather":
        gpool, dg, db, _ = run(True, want_dx=False)
        zw = sr._at_slot(sr.windows(sr._bn(x["x"], x["mean"], x["rstd"], x["gamma"], x["beta"])[1], 0.0), amax.cpu())
        _per_position(f"{name} act{act} win", "y", gpool, x["dpool"].to(F64) * sr.act_grad(zw, act), fails)      # (one bf16 rounding, like y)
    else:
        with pytest.raises(_lib.SvsrError):
            run(True, want_dx=False)
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from syncvsr_amd import _lib, ops
    dev, lib = _dev(), _lib.load()
    big = torch.full((1 << 20,), F_SENTINEL, device=dev)          # behind every pointer, should a refusal be missing
    p, s, ERR = big.data_ptr(), ops._stream(), 1001
    for B, T, H, W in ((1, 2, 9, 16), (1, 2, 16, 9), (1, 2, 6, 16), (1, 2, 16, 6)):
        assert lib.svsr_stem_conv_fwd(p, p, p, p, B, T, H, W, None, 0, s) == ERR
        assert lib.svsr_stem_conv_fwd(p, p, p, p, B, T, H, W, p, 1 << 22, s) == ERR
        assert lib.svsr_stem_conv_wgrad_plan(B, T, H, W, None, None) == ERR
        for use_tr in (0, 1):
            assert lib.svsr_stem_conv_wgrad(p, p, p, B, T, H, W, use_tr, p, 1 << 20, s) == ERR
        assert lib.svsr_stem_bwd_wgrad_ok(B, T, H, W) == 0
        assert lib.svsr_stem_bwd_wgrad(p, p, p, p, p, p, p, p, B, T, H, W, p, 1 << 20, s) == ERR
    assert lib.svsr_stem_bwd_wgrad(p, p, p, p, p, p, p, p, 1, 2, 12, 100, p, 1 << 20, s) == ERR          # W > 96: the two launches
    assert lib.svsr_stem_conv_wgrad(p, p, p, 1, 2, 12, 16, 1, p, 64 * 245 - 1, s) == ERR                 # a slab short of one workgroup
    # pooled sizes that are not the frame's, a channel count the passes do not take
    for Hp, Wp, C in ((4, 5, 64), (5, 4, 64), (6, 5, 64), (5, 5, 24)):
        assert lib.svsr_stem_bn_act_pool_fwd(p, p, p, p, p, p, p, 2, 9, 9, Hp, Wp, C, 1, None, s) == ERR
        assert lib.svsr_stem_bn_act_pool_bwd(p, p, p, p, p, p, p, p, p, p, p, p, 2, 9, 9, Hp, Wp, C, 1, None, None, s) == ERR
    assert lib.svsr_stem_bn_act_pool_fwd(p, p, p, p, p, p, p, 2, 9, 9, 5, 5, 64, 3, None, s) == ERR      # no such activation
    torch.cuda.synchronize()
    assert bool((big == F_SENTINEL).all()), "a refused call wrote something"

    # the LDS limits, from the launchers' formulas: 64 * 296 * 2 + 5 * 9 * (W + 6) * 2 <= 160 KiB (direct: W <= 1392),
    # 2368 * 16 + ceil(45 * (W + 8) / 8 / 64) * 64 * 16 <= 160 KiB (DMA-fed: W <= 1384); 1028 * WoP + 2080 <= 160 KiB (weight gradient: W <= 288)
    g = torch.Generator().manual_seed(8)
    w = torch.randint(-1, 2, (64, 5, 7, 7), generator=g).float()
    for W, use_ws, ok in ((1394, False, False), (1392, True, False), (1392, False, True), (1384, True, True)):
        vid = torch.randint(-1, 2, (1, 1, 8, W), generator=g).float()
        if not ok:
            with pytest.raises(_lib.SvsrError):
                ops.stem_conv_fwd(vid.view(1, 1, 1, 8, W).to(dev), w.reshape(-1).to(dev), use_ws=use_ws)
            continue
        out, _ = ops.stem_conv_fwd(vid.view(1, 1, 1, 8, W).to(dev), w.reshape(-1).to(dev), use_ws=use_ws)
        assert torch.equal(out.cpu().to(F64), sr.stem_conv_fwd(vid, w)[0]), f"forward at the LDS limit, W = {W}"
    for W, ok in ((290, False), (288, True)):
        vid = torch.randn(1, 1, 8, W, generator=g)
        dy = torch.zeros(1, 4, W // 2, 64, dtype=BF)
        for ch in range(64):
            dy[0, ch % 4, (ch * 37) % (W // 2) if ch > 1 else ch * (W // 2 - 1), ch] = 1.0
        for use_tr in (False, True):
            dw = torch.zeros(64 * 245, device=dev)
            if not ok:
                with pytest.raises(_lib.SvsrError):
                    ops.stem_conv_wgrad(vid.view(1, 1, 1, 8, W).to(dev), dy.to(dev), dw, use_tr=use_tr)
                assert not bool(dw.any())
                continue
            ops.stem_conv_wgrad(vid.view(1, 1, 1, 8, W).to(dev), dy.to(dev), dw, use_tr=use_tr)
            assert torch.equal(dw.cpu().view(64, 5, 7, 7).to(F64), sr.stem_conv_wgrad(vid, dy)), f"weight gradient at the LDS limit, W = {W}, use_tr {use_tr}"
