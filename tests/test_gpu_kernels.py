"""Kernel-level parity (-m gpu): every C-ABI entry point against a plain torch-fp32 CPU restatement of the same op,
fed the same bf16-rounded inputs.  Tolerances are stated per class of tensor:
  * bf16 activations / activation-gradients: max-abs error <= 1.5e-2 * max|ref| and relative L2 error <= 6e-3
    (one bf16 rounding of the output = 2^-9 relative, plus fp32 accumulation-order noise)
  * fp32 outputs (weight gradients, statistics, losses): relative L2 error <= 2e-3 (inputs are bf16-exact, products are
    accumulated in fp32 on both sides).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF)


def check(got, ref, name, max_tol=1.5e-2, l2_tol=6e-3):
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    l2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    assert err <= max_tol * scale and l2 <= l2_tol, f"{name}: max err {err:.3e} (scale {scale:.3e}), rel L2 {l2:.3e}"


def stat_sums(stats, C):
    """(buffer, rows) BatchNorm partials -> [2][C] column sums on the CPU"""
    buf, rows = stats
    return buf[: rows * 2 * C].view(rows, 2, C).double().sum(0).float().cpu()


def nhwc(t):  # [N,C,H,W] fp32 -> [N,H,W,C]
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


CONV_CASES = [
    # N, H, W, Ci, Co, k, stride, pad
    (3, 11, 11, 64, 64, 3, 1, 1),
    (2, 12, 12, 64, 128, 3, 2, 1),
    (2, 11, 11, 64, 128, 3, 2, 1),
    (3, 6, 6, 128, 256, 1, 2, 0),
    (5, 3, 3, 256, 512, 3, 1, 1),
    (40, 22, 22, 64, 64, 3, 1, 1),      # M = 19360 -> 128x64 tiles
    (70, 11, 11, 128, 128, 3, 1, 1),    # M = 8470  -> 128x128 tiles
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_stats(dev, case):
    from syncvsr_amd import ops

    N, H, W, Ci, Co, k, s, p = case
    x = rnd((N, H, W, Ci), 1)
    w = rnd((Co, k, k, Ci), 2, 1.0 / math.sqrt(k * k * Ci))
    out, stats = ops.conv2d_fwd(x.to(dev), w.to(dev), k, s, p, want_stats=True)
    ref = F.conv2d(nchw(x.float()), w.float().permute(0, 3, 1, 2), stride=s, padding=p)
    check(out, nhwc(ref), "conv_fwd")
    st = stat_sums(stats, Co)
    count = ref.numel() // Co
    sum_err = (st[0] - ref.sum((0, 2, 3))).abs()
    assert bool((sum_err <= 2e-3 * torch.sqrt(count * (ref * ref).sum((0, 2, 3)))).all()), "stats.sum"
    check(st[1], (ref * ref).sum((0, 2, 3)), "stats.sumsq", 3e-3, 2e-3)


@pytest.mark.parametrize("case", CONV_CASES[:6])
def test_conv_dgrad(dev, case):
    from syncvsr_amd import ops

    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
    dy = rnd((N, Ho, Wo, Co), 3)
    w = rnd((Co, k, k, Ci), 4, 1.0 / math.sqrt(k * k * Co))
    wt = w.permute(3, 1, 2, 0).contiguous()                # [Ci][k][k][Co]
    xs = torch.zeros(N, Ci, H, W, requires_grad=True)
    F.conv2d(xs, w.float().permute(0, 3, 1, 2), stride=s, padding=p).backward(nchw(dy.float()))
    dx = ops.conv2d_dgrad(dy.to(dev), wt.to(dev), k, s, p, (H, W))
    check(dx, nhwc(xs.grad), "conv_dgrad")
    add = rnd((N, H, W, Ci), 5)
    dx2 = ops.conv2d_dgrad(dy.to(dev), wt.to(dev), k, s, p, (H, W), addend=add.to(dev).clone())
    check(dx2, nhwc(xs.grad) + add.float(), "conv_dgrad+addend")


@pytest.mark.parametrize("use_tr", [False, True])
@pytest.mark.parametrize("case", CONV_CASES[:6])
def test_conv_wgrad(dev, case, use_tr):
    from syncvsr_amd import ops

    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
    x = rnd((N, H, W, Ci), 6)
    dy = rnd((N, Ho, Wo, Co), 7)
    ws = torch.zeros(Co, Ci, k, k, requires_grad=True)
    F.conv2d(nchw(x.float()), ws, stride=s, padding=p).backward(nchw(dy.float()))
    dw = torch.zeros(Co, k, k, Ci, device=dev)
    ops.conv2d_wgrad(x.to(dev), dy.to(dev), dw, k, s, p, use_tr=use_tr)
    check(dw, ws.grad.permute(0, 2, 3, 1), f"conv_wgrad tr={use_tr}", 3e-3, 2e-3)


def test_linear_variants(dev):
    from syncvsr_amd import ops

    B, S, K, N = 3, 7, 512, 192
    x = rnd((B * S, K), 8)
    w = rnd((N, K), 9, 1 / math.sqrt(K))
    b = torch.randn(N, generator=torch.Generator().manual_seed(10))
    ref = F.linear(x.float(), w.float(), b)
    out, _ = ops.linear_fwd(x.to(dev), w.to(dev), b.to(dev), rows=B * S, K=K, N=N, x_pitch=K)
    check(out, ref, "linear")
    out, pre = ops.linear_fwd(x.to(dev), w.to(dev), b.to(dev), rows=B * S, K=K, N=N, x_pitch=K, gelu=True)
    check(pre, ref, "linear.pre")
    check(out, F.gelu(ref), "linear.gelu")
    out, _ = ops.linear_fwd(x.to(dev), w.to(dev), b.to(dev), rows=B * (S - 1), K=K, N=N, x_pitch=K, seq=(S, 1, S - 1), out_f32=True)
    check(out, ref.view(B, S, N)[:, 1:].reshape(-1, N), "linear.seq f32", 2e-3, 1e-3)
    # odd N (classifier-like) with fp32 output, rows s = 0
    N2 = 100
    w2 = rnd((N2, K), 11, 1 / math.sqrt(K))
    out, _ = ops.linear_fwd(x.to(dev), w2.to(dev), None, rows=B, K=K, N=N2, x_pitch=K, seq=(S, 0, 1), out_f32=True)
    check(out, F.linear(x.float(), w2.float()).view(B, S, N2)[:, 0], "linear.cls", 2e-3, 1e-3)
    # dgrad with scatter + addend, wgrad with gather
    dy = rnd((B * (S - 1), N), 12)
    wt = torch.zeros(K, 1, N, dtype=BF)
    wt[:, 0, :] = w.t()
    dx = torch.zeros(B * S, K, dtype=BF, device=dev)
    ops.linear_dgrad(dy.to(dev), wt.to(dev), rows=B * (S - 1), N=N, K=K, dy_pitch=N, out=dx, seq=(S, 1, S - 1))
    ref_dx = torch.zeros(B, S, K)
    ref_dx[:, 1:] = (dy.float() @ w.float()).view(B, S - 1, K)
    check(dx, ref_dx.view(-1, K), "linear.dgrad.scatter")
    dw = torch.zeros(N, K, device=dev)
    ops.linear_wgrad(x.to(dev), dy.to(dev), dw, rows=B * (S - 1), K=K, N=N, x_pitch=K, dy_pitch=N, seq=(S, 1, S - 1))
    ref_dw = dy.float().t() @ x.float().view(B, S, K)[:, 1:].reshape(-1, K)
    check(dw, ref_dw, "linear.wgrad", 3e-3, 2e-3)
    db = torch.zeros(N, device=dev)
    z = rnd((B * (S - 1), N), 13)
    dz = ops.bias_act_bwd(dy.to(dev), z.to(dev), db, R=B * (S - 1), N=N, n_valid=N - 3, ld=N)
    zz = z.float().requires_grad_(True)
    F.gelu(zz).backward(dy.float())
    check(dz, zz.grad, "gelu_bwd")
    ref_db = zz.grad.to(BF).float().sum(0)
    ref_db[N - 3:] = 0
    check(db, ref_db, "bias_grad", 1e-2, 6e-3)


STEM_CASES = [(2, 5, 24, 24), (1, 3, 88, 88), (2, 2, 16, 40)]


@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_conv(dev, case):
    from syncvsr_amd import ops

    B, T, H, W = case
    g = torch.Generator().manual_seed(20)
    vid = torch.randn(B, 1, T, H, W, generator=g)
    w = (torch.rand(64, 1, 5, 7, 7, generator=g) - 0.5) * 0.2
    out, stats = ops.stem_conv_fwd(vid.to(dev), w.to(dev).reshape(-1), want_stats=True)
    ref = F.conv3d(vid.to(BF).float(), w.to(BF).float(), stride=(1, 2, 2), padding=(2, 3, 3))      # [B,64,T,Ho,Wo]
    ref_nhwc = ref.permute(0, 2, 3, 4, 1).reshape(B * T, H // 2, W // 2, 64)
    check(out, ref_nhwc, "stem_conv_fwd")
    st = stat_sums(stats, 64)
    check(st[1], (ref * ref).sum((0, 2, 3, 4)), "stem.stats.sumsq", 3e-3, 2e-3)
    dy = rnd((B * T, H // 2, W // 2, 64), 21)
    ws = w.to(BF).float().clone().requires_grad_(True)
    F.conv3d(vid.to(BF).float(), ws, stride=(1, 2, 2), padding=(2, 3, 3)).backward(
        dy.float().view(B, T, H // 2, W // 2, 64).permute(0, 4, 1, 2, 3))
    for use_tr in (False, True):
        dw = torch.zeros(64 * 245, device=dev)
        ops.stem_conv_wgrad(vid.to(dev), dy.to(dev), dw, use_tr=use_tr)
        check(dw.view(64, 1, 5, 7, 7), ws.grad, f"stem_conv_wgrad tr={use_tr}", 4e-3, 3e-3)


def _bn_ref(x, gamma, beta, res, act):
    dims = (0, 1, 2)
    mean = x.mean(dims)
    var = x.var(dims, unbiased=False)
    y = (x - mean) * torch.rsqrt(var + 1e-5) * gamma + beta
    if res is not None:
        y = y + res
    if act:
        y = torch.relu(y)
    return y, mean, var


@pytest.mark.parametrize("C,act,use_res", [(64, 1, False), (128, 1, True), (512, 0, False), (256, 1, True)])
def test_bn_act(dev, C, act, use_res):
    from syncvsr_amd import ops

    N, H, W = 5, 7, 6
    x = rnd((N, H, W, C), 30, 2.0) + 0.3
    res = rnd((N, H, W, C), 31) if use_res else None
    g = torch.Generator().manual_seed(32)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    dy = rnd((N, H, W, C), 33)
    xf = x.float().requires_grad_(True)
    rf = res.float().requires_grad_(True) if use_res else None
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yref, mean, var = _bn_ref(xf, gm, bt, rf, act)
    yref.backward(dy.float())
    # statistics through the partial-row protocol: 135 rows (more than the 128 one reduction sweep covers), split unevenly
    nrows = 135
    wgt = torch.rand(nrows, 1, generator=torch.Generator().manual_seed(34)) + 0.1
    wgt = wgt / wgt.sum()
    part = torch.zeros(nrows, 2, C)
    part[:, 0] = wgt * x.float().sum((0, 1, 2))
    part[:, 1] = wgt * (x.float() ** 2).sum((0, 1, 2))
    part = part.reshape(-1).to(dev)
    m = torch.empty(C, device=dev); r = torch.empty(C, device=dev)
    rm = torch.zeros(C, device=dev); rv = torch.ones(C, device=dev); nbt = torch.zeros((), dtype=torch.long, device=dev)
    count = N * H * W
    ops.bn_finalize((part, nrows), C, count, m, r, rm, rv, nbt)
    check(m, mean, "bn.mean", 1e-3, 1e-3)
    check(r, torch.rsqrt(var + 1e-5), "bn.rstd", 1e-3, 1e-3)
    check(rm, 0.1 * mean, "bn.running_mean", 1e-3, 1e-3)
    check(rv, 0.9 + 0.1 * var * count / (count - 1), "bn.running_var", 1e-3, 1e-3)
    assert int(nbt.item()) == 1
    y = ops.bn_act_fwd(x.to(dev), None if res is None else res.to(dev), m, r, gamma.to(dev), beta.to(dev), act)
    check(y, yref, "bn_act_fwd")
    coef = torch.empty(3 * C, device=dev)
    dg = torch.zeros(C, device=dev); db = torch.zeros(C, device=dev)
    dx, dres = ops.bn_act_bwd(dy.to(dev), y if act else None, x.to(dev), m, r, gamma.to(dev), coef, dg, db, act, use_res)
    check(dx, xf.grad, "bn_act_bwd.dx", 2e-2, 8e-3)
    check(dg, gm.grad, "bn.dgamma", 1e-2, 6e-3)
    check(db, bt.grad, "bn.dbeta", 1e-2, 6e-3)
    if use_res:
        check(dres, rf.grad, "bn.dres")


DGRAD_BN_CASES = [
    # N, H, W, Ci, Co, k, stride, pad, addend          (H, W, Ci: geometry of the RESULT = the BatchNorm output being differentiated)
    (40, 22, 22, 64, 64, 3, 1, 1, True),       # persistent 64 -> 64 kernel, several chunks per workgroup
    (3, 11, 11, 64, 64, 3, 1, 1, False),       # the same kernel with fewer chunks than workgroups
    (70, 11, 11, 128, 128, 3, 1, 1, True),     # 128x128 tiles
    (70, 11, 11, 128, 128, 3, 1, 1, False),
    (9, 12, 12, 64, 128, 3, 2, 1, True),       # stride-2 data gradient: four parity classes in one launch
    (150, 6, 6, 256, 256, 3, 1, 1, True),      # 128x64 tiles (few tiles)
    (5, 3, 3, 512, 512, 3, 1, 1, False),       # 64x64 tiles
]


@pytest.mark.parametrize("case", DGRAD_BN_CASES)
def test_conv_dgrad_with_bn_backward_epilogue(dev, case):
    """svsr_igemm_dgrad_bn / svsr_conv3x3_c64_dgrad_bn + svsr_bn_bwd_from_stats == data gradient, then BatchNorm+ReLU backward
    (torch fp32), and the masked gradient is bit-identical to the one the separate passes produce."""
    from syncvsr_amd import ops

    N, H, W, Ci, Co, k, s, p, use_add = case
    Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
    dy = rnd((N, Ho, Wo, Co), 3)
    w = rnd((Co, k, k, Ci), 4, 1.0 / math.sqrt(k * k * Co))
    wt = w.permute(3, 1, 2, 0).contiguous()
    add = rnd((N, H, W, Ci), 5) if use_add else None
    xb = rnd((N, H, W, Ci), 6, 2.0) + 0.3                  # the BatchNorm input whose output the result differentiates
    res = rnd((N, H, W, Ci), 7) if use_add else None       # residual branch of that output (only its effect on the mask matters)
    g_ = torch.Generator().manual_seed(8)
    gamma = 1 + 0.2 * torch.randn(Ci, generator=g_)
    beta = 0.2 * torch.randn(Ci, generator=g_)
    xs = torch.zeros(N, Ci, H, W, requires_grad=True)
    F.conv2d(xs, w.float().permute(0, 3, 1, 2), stride=s, padding=p).backward(nchw(dy.float()))
    dout = nhwc(xs.grad) + (add.float() if use_add else 0.0)
    xf = xb.float().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yref, mean, var = _bn_ref(xf, gm, bt, None if res is None else res.float(), 1)
    mean, var = mean.detach(), var.detach()
    # the forward output the backward sees is the HIP forward's (its ReLU mask is what the mask-from-x variant must reproduce bit for bit)
    y_dev = ops.bn_act_fwd(xb.to(dev), None if res is None else res.to(dev), mean.to(dev), torch.rsqrt(var + 1e-5).to(dev),
                           gamma.to(dev), beta.to(dev), 1)
    check(y_dev, yref.detach(), "bn_act_fwd")
    ybf = y_dev.cpu()
    # reference backward with the mask of the bf16 output the kernels see, and the gradient rounded as the launch stores it
    gref = torch.where(ybf.float() > 0, dout.to(BF).float(), torch.zeros(()))
    rstd = torch.rsqrt(var + 1e-5)
    xhat = (xb.float() - mean) * rstd
    cnt = N * H * W
    s1, s2 = gref.sum((0, 1, 2)), (gref * xhat).sum((0, 1, 2))
    dxb_ref = gamma * rstd * (gref - s1 / cnt - xhat * s2 / cnt)

    m, r = mean.to(dev), rstd.to(dev)
    g, stats = ops.conv2d_dgrad_bn(dy.to(dev), wt.to(dev), k, s, p, (H, W), None if add is None else add.to(dev).clone(), ybf.to(dev),
                                   xb.to(dev), m, r)
    check(g, gref, "dgrad_bn.g")
    sums = stat_sums(stats, Ci)
    check(sums[0], s1, "dgrad_bn.sum_g", 1e-2, 6e-3)
    check(sums[1], s2, "dgrad_bn.sum_g_xhat", 1e-2, 6e-3)
    coef = torch.empty(3 * Ci, device=dev)
    dg = torch.zeros(Ci, device=dev); db = torch.zeros(Ci, device=dev)
    dxb = ops.bn_bwd_from_stats(g, xb.to(dev), m, r, gamma.to(dev), stats, coef, dg, db)
    check(dxb, dxb_ref, "dgrad_bn.dx", 2e-2, 8e-3)
    check(dg, s2, "dgrad_bn.dgamma", 1e-2, 6e-3)
    check(db, s1, "dgrad_bn.dbeta", 1e-2, 6e-3)
    # the separate passes on the same inputs: same masked gradient bit for bit, same BatchNorm input gradient up to summation order
    do = ops.conv2d_dgrad(dy.to(dev), wt.to(dev), k, s, p, (H, W), addend=None if add is None else add.to(dev).clone())
    dg2 = torch.zeros(Ci, device=dev); db2 = torch.zeros(Ci, device=dev)
    dxb2, dres2 = ops.bn_act_bwd(do, ybf.to(dev), xb.to(dev), m, r, gamma.to(dev), coef, dg2, db2, 1, True)
    if s == 1 and Ci == 64 or ops.conv_plan(1, N, H, W, Ci, k, s, p).bm == 128:
        assert torch.equal(g, dres2), "masked gradient differs from the separate pass"
    else:       # few 64x64 tiles: the plain launch splits K inside the workgroup (another summation order), the fused one does not
        check(g, dres2.float().cpu(), "dgrad_bn.g vs separate passes", 1e-2, 3e-3)
    check(dxb, dxb2.float().cpu(), "dgrad_bn.dx vs separate passes", 1e-2, 3e-3)
    check(dg, dg2.cpu(), "dgrad_bn.dgamma vs separate passes", 1e-3, 1e-3)
    if res is None:     # no residual branch: the mask recomputed from x equals the mask read from y
        gx, statsx = ops.conv2d_dgrad_bn(dy.to(dev), wt.to(dev), k, s, p, (H, W), None, None, xb.to(dev), m, r, gamma.to(dev), beta.to(dev))
        assert torch.equal(gx, g) and torch.equal(stat_sums(statsx, Ci), sums), "mask recomputed from x differs from the stored one"
    # reproducible
    g3, stats3 = ops.conv2d_dgrad_bn(dy.to(dev), wt.to(dev), k, s, p, (H, W), None if add is None else add.to(dev).clone(), ybf.to(dev),
                                     xb.to(dev), m, r)
    assert torch.equal(g3, g) and torch.equal(stat_sums(stats3, Ci), sums)


@pytest.mark.parametrize("case", [DGRAD_BN_CASES[0], DGRAD_BN_CASES[1], DGRAD_BN_CASES[2], DGRAD_BN_CASES[3], DGRAD_BN_CASES[5]])
def test_conv_dgrad_with_swish_bn_backward_epilogue(dev, case):
    """The Swish variant (LRS trunk): g = (dgrad + addend) * swish'(bn(x) + residual), sums of g and g * xhat, then the apply pass ==
    data gradient followed by BatchNorm+Swish backward in fp32; and == the separate passes up to one bf16 rounding of g."""
    from syncvsr_amd import ops

    N, H, W, Ci, Co, k, s, p, use_add = case
    Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
    dy = rnd((N, Ho, Wo, Co), 3)
    w = rnd((Co, k, k, Ci), 4, 1.0 / math.sqrt(k * k * Co))
    wt = w.permute(3, 1, 2, 0).contiguous()
    add = rnd((N, H, W, Ci), 5) if use_add else None
    xb = rnd((N, H, W, Ci), 6, 2.0) + 0.3
    res = rnd((N, H, W, Ci), 7) if use_add else None
    g_ = torch.Generator().manual_seed(8)
    gamma = 1 + 0.2 * torch.randn(Ci, generator=g_)
    beta = 0.2 * torch.randn(Ci, generator=g_)
    xs = torch.zeros(N, Ci, H, W, requires_grad=True)
    F.conv2d(xs, w.float().permute(0, 3, 1, 2), stride=s, padding=p).backward(nchw(dy.float()))
    dout = (nhwc(xs.grad) + (add.float() if use_add else 0.0)).to(BF).float()
    xf = xb.float()
    mean, var = xf.mean((0, 1, 2)), xf.var((0, 1, 2), unbiased=False)
    rstd = torch.rsqrt(var + 1e-5)
    xhat = (xf - mean) * rstd
    z = (xhat * gamma + beta + (res.float() if res is not None else 0.0)).requires_grad_(True)
    (z * torch.sigmoid(z)).sum().backward()
    gref = dout * z.grad
    cnt = N * H * W
    s1, s2 = gref.sum((0, 1, 2)), (gref * xhat).sum((0, 1, 2))
    dxb_ref = gamma * rstd * (gref - s1 / cnt - xhat * s2 / cnt)
    m, r = mean.to(dev), rstd.to(dev)
    g, stats = ops.conv2d_dgrad_bn(dy.to(dev), wt.to(dev), k, s, p, (H, W), None if add is None else add.to(dev).clone(),
                                   None if res is None else res.to(dev), xb.to(dev), m, r, gamma.to(dev), beta.to(dev), act=2)
    check(g, gref, "dgrad_bn_swish.g", 2e-2, 8e-3)
    sums = stat_sums(stats, Ci)
    check(sums[0], s1, "dgrad_bn_swish.sum_g", 1e-2, 6e-3)
    check(sums[1], s2, "dgrad_bn_swish.sum_g_xhat", 1e-2, 6e-3)
    coef = torch.empty(3 * Ci, device=dev)
    dg = torch.zeros(Ci, device=dev); db = torch.zeros(Ci, device=dev)
    dxb = ops.bn_bwd_from_stats(g, xb.to(dev), m, r, gamma.to(dev), stats, coef, dg, db)
    check(dxb, dxb_ref, "dgrad_bn_swish.dx", 2e-2, 8e-3)
    check(dg, s2, "dgrad_bn_swish.dgamma", 1e-2, 6e-3)
    check(db, s1, "dgrad_bn_swish.dbeta", 1e-2, 6e-3)
    # the separate passes on the same inputs
    do = ops.conv2d_dgrad(dy.to(dev), wt.to(dev), k, s, p, (H, W), addend=None if add is None else add.to(dev).clone())
    y_dev = ops.bn_act_fwd(xb.to(dev), None if res is None else res.to(dev), m, r, gamma.to(dev), beta.to(dev), 2)
    dg2 = torch.zeros(Ci, device=dev); db2 = torch.zeros(Ci, device=dev)
    dxb2, dres2 = ops.bn_act_bwd(do, y_dev, xb.to(dev), m, r, gamma.to(dev), coef, dg2, db2, 2, True, beta=beta.to(dev),
                                 res=None if res is None else res.to(dev))
    check(g, dres2.float().cpu(), "dgrad_bn_swish.g vs separate passes", 1e-2, 4e-3)
    check(dxb, dxb2.float().cpu(), "dgrad_bn_swish.dx vs separate passes", 1.5e-2, 5e-3)
    check(dg, dg2.cpu(), "dgrad_bn_swish.dgamma vs separate passes", 3e-3, 3e-3)
    g3, stats3 = ops.conv2d_dgrad_bn(dy.to(dev), wt.to(dev), k, s, p, (H, W), None if add is None else add.to(dev).clone(),
                                     None if res is None else res.to(dev), xb.to(dev), m, r, gamma.to(dev), beta.to(dev), act=2)
    assert torch.equal(g3, g) and torch.equal(stat_sums(stats3, Ci), sums)


def test_linear_dgrad_with_swish_bn_backward_epilogue(dev):
    """ops.linear_dgrad_bn (Conformer convolution module: pointwise_conv2's data gradient -> BatchNorm1d + Swish backward)."""
    from syncvsr_amd import ops

    R, D = 2400, 768
    dy = rnd((R, D), 3)
    w = rnd((D, D), 4, 1.0 / math.sqrt(D))            # [N out][K in]
    wt = w.t().contiguous().view(D, 1, D)             # transposed shadow [K][1][N]
    xb = rnd((R, D), 6, 2.0) + 0.3
    g_ = torch.Generator().manual_seed(8)
    gamma = 1 + 0.2 * torch.randn(D, generator=g_)
    beta = 0.2 * torch.randn(D, generator=g_)
    dout = (dy.float() @ w.float()).to(BF).float()
    xf = xb.float()
    mean, var = xf.mean(0), xf.var(0, unbiased=False)
    rstd = torch.rsqrt(var + 1e-5)
    xhat = (xf - mean) * rstd
    z = (xhat * gamma + beta).requires_grad_(True)
    (z * torch.sigmoid(z)).sum().backward()
    gref = dout * z.grad
    s1, s2 = gref.sum(0), (gref * xhat).sum(0)
    dxb_ref = gamma * rstd * (gref - s1 / R - xhat * s2 / R)
    m, r = mean.to(dev), rstd.to(dev)
    g, stats = ops.linear_dgrad_bn(dy.to(dev), wt.to(dev), rows=R, N=D, K=D, dy_pitch=D, x=xb.to(dev), mean=m, rstd=r,
                                   gamma=gamma.to(dev), beta=beta.to(dev), act=2)
    check(g, gref, "linear_dgrad_bn.g", 2e-2, 8e-3)
    coef = torch.empty(3 * D, device=dev)
    dg = torch.zeros(D, device=dev); db = torch.zeros(D, device=dev)
    dxb = ops.bn_bwd_from_stats(g, xb.to(dev), m, r, gamma.to(dev), stats, coef, dg, db)
    check(dxb, dxb_ref, "linear_dgrad_bn.dx", 2e-2, 8e-3)
    check(dg, s2, "linear_dgrad_bn.dgamma", 1e-2, 6e-3)
    check(db, s1, "linear_dgrad_bn.dbeta", 1e-2, 6e-3)


@pytest.mark.parametrize("R,D,U,pdrop", [(2400, 768, 2048, 0.1), (704, 768, 2048, 0.0), (130, 256, 512, 0.25)])
def test_linear_dgrad_with_relu_dropout_epilogue(dev, R, D, U, pdrop):
    """ops.linear_dgrad_relu (feed-forward block: w_2's data gradient through dropout(relu(z)), positionwise_feed_forward.py:28-30) against
    autograd in fp32 and against the two launches it replaces (linear_dgrad + bias_act_bwd)."""
    from syncvsr_amd import ops

    dy = rnd((R, D), 3)
    w2 = rnd((D, U), 4, 1.0 / math.sqrt(U))           # [N out = D][K in = U]
    wt = w2.t().contiguous().view(U, 1, D)            # transposed shadow [K][1][N]
    g_ = torch.Generator().manual_seed(11)
    z = torch.randn(R, U, generator=g_)
    keep = (torch.rand(R, U, generator=g_) >= pdrop).float()
    gs = 1.0 / (1.0 - pdrop)
    h = (torch.relu(z) * keep * gs).to(BF)            # the saved activation: zero where ReLU or the mask cut
    dref = (dy.float() @ w2.float()) * (h.float() > 0).float() * gs
    dz, (part, tiles) = ops.linear_dgrad_relu(dy.to(dev), wt.to(dev), rows=R, N=D, K=U, dy_pitch=D, y=h.to(dev), gscale=gs)
    check(dz, dref, "linear_dgrad_relu.dz", 2e-2, 8e-3)
    db = torch.zeros(U, device=dev)
    ops.colsum_rows(part, tiles, 2 * U, db, U)
    check(db, dref.sum(0), "linear_dgrad_relu.dbias", 1e-2, 2e-2)
    # the pair of launches it replaces: same dz bit for bit (both round the data gradient to bf16, then the product)
    dh = ops.linear_dgrad(dy.to(dev), wt.to(dev), rows=R, N=D, K=U, dy_pitch=D)
    db2 = torch.zeros(U, device=dev)
    dz2 = ops.bias_act_bwd(dh, h.to(dev), db2, R=R, N=U, n_valid=U, ld=U, relu=True, gscale=gs)
    assert torch.equal(dz, dz2)
    check(db, db2.float().cpu(), "linear_dgrad_relu.dbias vs bias_act_bwd", 4e-3, 4e-3)      # (sums of the rounded values here, of the unrounded products there)


@pytest.mark.parametrize("Hc,Wc", [(12, 12), (11, 9), (44, 44)])
def test_stem_bn_gelu_pool(dev, Hc, Wc):
    from syncvsr_amd import ops

    N, C = 3, 64
    x = rnd((N, Hc, Wc, C), 40, 1.5)
    g = torch.Generator().manual_seed(41)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    xf = nchw(x.float()).requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    mean = xf.mean((0, 2, 3)); var = xf.var((0, 2, 3), unbiased=False)
    z = (xf - mean.view(1, -1, 1, 1)) * torch.rsqrt(var.view(1, -1, 1, 1) + 1e-5) * gm.view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)
    yref = F.max_pool2d(F.gelu(z), 3, 2, 1)
    dpool = rnd(tuple(nhwc(yref).shape), 42)
    yref.backward(nchw(dpool.float()))
    m = mean.detach().to(dev); r = torch.rsqrt(var.detach() + 1e-5).to(dev)
    y, amax = ops.stem_bn_gelu_pool_fwd(x.to(dev), m, r, gamma.to(dev), beta.to(dev))
    check(y, nhwc(yref), "stem_pool_fwd")
    coef = torch.empty(3 * C, device=dev)
    dg = torch.zeros(C, device=dev); db = torch.zeros(C, device=dev)
    dx = ops.stem_bn_gelu_pool_bwd(dpool.to(dev), amax, x.to(dev), m, r, gamma.to(dev), beta.to(dev), coef, dg, db)
    # Max-pool routing: two window candidates whose GELU values differ by less than the erf approximation error (1.5e-7,
    # Abramowitz-Stegun 7.1.26 in common.h) may resolve to a different argmax than torch's erf does; the gradient then
    # lands on the other (numerically tied) pixel.  Such flips are allowed for <= 0.1 % of the elements.
    got, ref_dx = dx.float().cpu(), nhwc(xf.grad)
    bad = ((got - ref_dx).abs() > 2e-2 * ref_dx.abs().max()).sum().item()
    assert bad <= max(4, 1e-3 * ref_dx.numel()), f"stem_pool_bwd.dx: {bad} elements off"
    assert ((got - ref_dx).norm() / ref_dx.norm()).item() <= 3e-2
    check(dg, gm.grad, "stem.dgamma", 1e-2, 6e-3)
    check(db, bt.grad, "stem.dbeta", 1e-2, 6e-3)
    # the same through the winners the forward keeps (xwin: the convolution output at every window's arg-max; reduce pass over pooled
    # outputs, apply pass without activation derivatives): same outputs, and xwin IS the bf16 value at the arg-max
    y2, amax2, xwin = ops.stem_bn_gelu_pool_fwd(x.to(dev), m, r, gamma.to(dev), beta.to(dev), want_win=True)
    assert torch.equal(y2, y) and torch.equal(amax2, amax)
    Hp, Wp = y.shape[1], y.shape[2]
    xpad = F.pad(nchw(x.float()), (1, 1, 1, 1))
    win = F.unfold(xpad, 3, stride=2).view(N, C, 9, Hp, Wp)                     # [N, C, 9, Hp, Wp]
    want_win = torch.gather(win, 2, nchw(amax.cpu().long()).unsqueeze(2)).squeeze(2)
    assert torch.equal(nchw(xwin.float().cpu()), want_win), "xwin must be the stored convolution output at the arg-max"
    dg2 = torch.zeros(C, device=dev); db2 = torch.zeros(C, device=dev)
    dx2 = ops.stem_bn_gelu_pool_bwd(dpool.to(dev), amax, x.to(dev), m, r, gamma.to(dev), beta.to(dev), coef, dg2, db2, xwin=xwin)
    got2 = dx2.float().cpu()
    assert ((got2 - got).norm() / got.norm()).item() <= 4e-3, "winner form vs gather form (g rounded to bf16 once more)"
    bad2 = ((got2 - ref_dx).abs() > 2e-2 * ref_dx.abs().max()).sum().item()
    assert bad2 <= max(4, 1e-3 * ref_dx.numel()) and ((got2 - ref_dx).norm() / ref_dx.norm()).item() <= 3e-2
    check(dg2, gm.grad, "stem.dgamma (winners)", 1e-2, 6e-3)
    check(db2, bt.grad, "stem.dbeta (winners)", 1e-2, 6e-3)


@pytest.mark.parametrize("B,T,H,W,act", [(2, 5, 88, 88, 1), (1, 3, 44, 72, 2), (1, 2, 42, 40, 1), (3, 7, 96, 96, 2)])
def test_stem_backward_apply_inside_the_weight_gradient(dev, B, T, H, W, act):
    """svsr_stem_bwd_wgrad (BatchNorm / activation / max-pool backward apply pass fused into the stem convolution's weight gradient):
    dW bit-identical to svsr_stem_bn_act_pool_bwd -> svsr_stem_conv_wgrad, dgamma / dbeta likewise; frame heights that leave a short
    last tile (H/2 = 22, 21) and pooled rows past the frame, both activations."""
    from syncvsr_amd import ops

    C, Ho, Wo = 64, H // 2, W // 2
    g = torch.Generator().manual_seed(1234 + H + W)
    vid = torch.randn((B, 1, T, H, W), generator=g).to(dev)
    x = (1.5 * torch.randn((B * T, Ho, Wo, C), generator=g)).to(torch.bfloat16).to(dev)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(dev); beta = (0.2 * torch.randn(C, generator=g)).to(dev)
    xf = x.float()
    m = xf.mean((0, 1, 2)); r = torch.rsqrt(xf.var((0, 1, 2), unbiased=False) + 1e-5)
    y, amax, xwin = ops.stem_bn_gelu_pool_fwd(x, m, r, gamma, beta, act=act, want_win=True)
    dpool = torch.randn(tuple(y.shape), generator=g).to(torch.bfloat16).to(dev)
    assert ops.stem_bwd_wgrad_ok(vid)
    coef = torch.empty(3 * C, device=dev); dg = torch.zeros(C, device=dev); db = torch.zeros(C, device=dev)
    dx = ops.stem_bn_gelu_pool_bwd(dpool, amax, x, m, r, gamma, beta, coef, dg, db, act=act, xwin=xwin)
    dw = torch.zeros(64 * 245, device=dev)
    ops.stem_conv_wgrad(vid, dx, dw, use_tr=True)
    coef2 = torch.empty(3 * C, device=dev); dg2 = torch.zeros(C, device=dev); db2 = torch.zeros(C, device=dev)
    gpool = ops.stem_bn_gelu_pool_bwd(dpool, amax, x, m, r, gamma, beta, coef2, dg2, db2, act=act, xwin=xwin, want_dx=False)
    dw2 = torch.zeros(64 * 245, device=dev)
    ops.stem_bwd_wgrad(vid, gpool, amax, x, m, r, coef2, dw2)
    assert torch.equal(coef, coef2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    assert dw.abs().max().item() > 0
    assert torch.equal(dw, dw2), f"fused stem backward: max |diff| {(dw - dw2).abs().max().item():.3e} of {dw.abs().max().item():.3e}"


def test_avgpool(dev):
    from syncvsr_amd import ops

    x = rnd((7, 3, 3, 512), 50)
    y = ops.avgpool_fwd(x.to(dev))
    check(y, x.float().mean((1, 2)), "avgpool_fwd")
    dy = rnd((7, 512), 51)
    dx = ops.avgpool_bwd(dy.to(dev), (7, 3, 3, 512))
    check(dx, (dy.float() / 9).view(7, 1, 1, 512).expand(7, 3, 3, 512), "avgpool_bwd")


def test_add_ln_and_embed(dev):
    from syncvsr_amd import ops

    B, S, D = 3, 6, 512
    R = B * S
    a, r = rnd((R, D), 60), rnd((R, D), 61)
    g = torch.Generator().manual_seed(62)
    gamma = 1 + 0.2 * torch.randn(D, generator=g); beta = 0.2 * torch.randn(D, generator=g)
    dy = rnd((R, D), 63)
    af, rf = a.float().requires_grad_(True), r.float().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yref = F.layer_norm(af + rf, (D,), gm, bt, 1e-12)
    yref.backward(dy.float())
    y, mean, rstd = ops.add_ln_fwd(a.to(dev), r.to(dev), gamma.to(dev), beta.to(dev), 1e-12)
    check(y, yref, "add_ln_fwd")
    dg = torch.zeros(D, device=dev); db = torch.zeros(D, device=dev)
    ds = ops.add_ln_bwd(dy.to(dev), a.to(dev), r.to(dev), gamma.to(dev), mean, rstd, dg, db)
    check(ds, af.grad, "add_ln_bwd.ds", 2e-2, 8e-3)
    check(dg, gm.grad, "ln.dgamma", 1e-2, 6e-3)
    check(db, bt.grad, "ln.dbeta", 1e-2, 6e-3)
    # embeddings
    feats = rnd((B * (S - 1), D), 64)
    cls = torch.randn(D, generator=g); pos = 0.02 * torch.randn(16, D, generator=g); typ = 0.02 * torch.randn(2, D, generator=g)
    e = torch.cat((cls.to(BF).float().view(1, 1, D).expand(B, 1, D), feats.float().view(B, S - 1, D)), 1) + pos[:S] + typ[0]
    yref = F.layer_norm(e, (D,), gamma, beta, 1e-12)
    s0, y0, m0, r0 = ops.embed_ln_fwd(feats.to(dev), cls.to(dev), pos.to(dev).reshape(-1), typ.to(dev).reshape(-1), gamma.to(dev), beta.to(dev), B, S, D, 1e-12)
    check(s0, e.view(R, D), "embed.sum")
    check(y0, yref.view(R, D), "embed.ln", 2e-2, 8e-3)
    ds0 = rnd((R, D), 65)
    dcls = torch.zeros(D, device=dev); dpos = torch.zeros(16 * D, device=dev); dtyp = torch.zeros(2 * D, device=dev)
    dfe = ops.embed_bwd_scatter(ds0.to(dev), dcls, dpos, dtyp, B, S, D)
    d3 = ds0.float().view(B, S, D)
    check(dfe, d3[:, 1:].reshape(-1, D), "embed.dfeats", 1e-6, 1e-6)
    check(dcls, d3[:, 0].sum(0), "embed.dcls", 1e-3, 1e-3)
    check(dpos.view(16, D)[:S], d3.sum(0), "embed.dpos", 1e-3, 1e-3)
    check(dtyp.view(2, D)[0], d3.sum((0, 1)), "embed.dtype", 1e-3, 1e-3)


@pytest.mark.parametrize("S", [30, 6, 64])
def test_attention(dev, S):
    from syncvsr_amd import ops

    B, H, dh = 2, 8, 64
    D = H * dh
    qkv = rnd((B * S, 3 * D), 70)
    dctx = rnd((B * S, D), 71)
    q = qkv.float().requires_grad_(True)
    qq, kk, vv = (t.reshape(B, S, H, dh).transpose(1, 2) for t in q.view(B * S, 3, D).unbind(1))
    pr = torch.softmax(qq @ kk.transpose(-1, -2) / math.sqrt(dh), -1)
    ctx_ref = (pr @ vv).transpose(1, 2).reshape(B * S, D)
    ctx_ref.backward(dctx.float())
    qd = qkv.to(dev)
    ctx, probs = ops.mha_fwd(qd, 3 * D, qd[:, D:], qd[:, 2 * D:], 3 * D, B=B, H=H, Lq=S, Lk=S)
    check(ctx, ctx_ref, "attn_fwd")
    check(probs.view(B, H, S, -1)[..., :S], pr, "attn_probs")
    dqkv = torch.empty_like(qd)
    ops.mha_bwd(dctx.to(dev), qd, 3 * D, qd[:, D:], qd[:, 2 * D:], 3 * D, probs, B=B, H=H, Lq=S, Lk=S, dq=dqkv, dq_pitch=3 * D,
                dk=dqkv[:, D:], dv=dqkv[:, 2 * D:], dkv_pitch=3 * D)
    check(dqkv, q.grad, "attn_bwd", 2e-2, 1e-2)


def test_cross_entropy_and_topk(dev):
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(80)
    R, V = 50, 320
    logits = (torch.randn(R, V, generator=g) * 2).to(BF)
    tgt = torch.randint(0, V, (R,), generator=g)
    lf = logits.float().requires_grad_(True)
    ref = F.cross_entropy(lf, tgt)
    (ref * 3.0).backward()
    loss, lse = ops.ce_fwd(logits.to(dev), V, tgt.to(dev), None, R, V, 0.0)
    check(loss, ref, "ce.hard", 1e-5, 1e-5)
    dl = torch.empty(R, V, dtype=BF, device=dev)
    ops.ce_bwd(logits.to(dev), V, tgt.to(dev), None, R, V, 0.0, lse, torch.tensor(3.0, device=dev), dl, V)
    check(dl, lf.grad, "ce.hard.bwd")
    # fp32 logits, odd class count, label smoothing, hard + soft targets
    B, C = 9, 500
    lg = torch.randn(B, C, generator=g) * 3
    hard = torch.randint(0, C, (B,), generator=g)
    soft = torch.zeros(B, C); soft[torch.arange(B), hard] = 0.7; soft[torch.arange(B), (hard + 5) % C] += 0.3
    for tgt_i, tgt_p in ((hard, None), (None, soft)):
        lf = lg.clone().requires_grad_(True)
        ref = F.cross_entropy(lf, tgt_i if tgt_i is not None else tgt_p, label_smoothing=0.1)
        ref.backward()
        loss, lse = ops.ce_fwd(lg.to(dev), C, None if tgt_i is None else tgt_i.to(dev), None if tgt_p is None else tgt_p.to(dev), B, C, 0.1)
        check(loss, ref, "ce.ls", 1e-5, 1e-5)
        dl = torch.zeros(B, 512, dtype=BF, device=dev)
        ops.ce_bwd(lg.to(dev), C, None if tgt_i is None else tgt_i.to(dev), None if tgt_p is None else tgt_p.to(dev), B, C, 0.1, lse,
                   torch.tensor(1.0, device=dev), dl, 512)
        check(dl[:, :C], lf.grad, "ce.ls.bwd")
        assert float(dl[:, C:].abs().max()) == 0.0
        acc = ops.topk_acc(lg.to(dev), None if tgt_i is None else tgt_i.to(dev), None if tgt_p is None else tgt_p.to(dev)).cpu()
        corr = lg.topk(5, dim=1)[1] == hard.unsqueeze(1)
        assert abs(acc[0].item() - corr[:, 0].float().mean().item()) < 1e-6
        assert abs(acc[1].item() - corr.float().amax(1).mean().item()) < 1e-6


@pytest.mark.parametrize("R,K,G,V,seq", [(58, 512, 8, 320, (30, 1, 29)), (301, 576, 4, 640, None), (928, 512, 8, 320, (30, 1, 29)), (128, 64, 1, 320, None)])
def test_fused_audio_head(dev, R, K, G, V, seq):
    """svsr_linear_ce_fwd / _bwd (projection + per-frame cross-entropy in one contraction, logits never stored) against
    F.cross_entropy((h W^T + b).reshape(-1, V), tok) in fp32 on the same bf16 inputs: loss and log-sum-exp to fp32 accuracy, dlogits to one
    bf16 rounding; rows gathered like the model's (S, s0, T) view of the encoder output; a target outside [0, V) poisons the loss."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(R + V)
    rows_h = R if seq is None else (R // seq[2]) * seq[0]
    h = (torch.randn(rows_h, K, generator=g) * 0.8).to(BF)
    w = (torch.randn(G * V, K, generator=g) / math.sqrt(K) * 2.0).to(BF)
    b = torch.randn(G * V, generator=g) * 0.5
    tok = torch.randint(0, V, (R * G,), generator=g)
    gout = torch.tensor(0.37)
    assert ops.linear_ce_ok(R, K, G, V)
    hs = h.float() if seq is None else h.float().view(-1, seq[0], K)[:, seq[1]:seq[1] + seq[2]].reshape(R, K)
    z = (hs @ w.float().t() + b).reshape(R * G, V).requires_grad_(True)
    ref = F.cross_entropy(z, tok)
    (ref * gout).backward()
    loss, lse = ops.linear_ce_fwd(h.to(dev), w.to(dev), b.to(dev), tok.to(dev), R, K, G, V, seq=seq)
    assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item()), (loss.item(), ref.item())
    check(lse, torch.logsumexp(z.detach(), dim=1), "lse", max_tol=2e-5, l2_tol=1e-5)
    dl = torch.full((R, G * V), float("nan"), dtype=BF, device=dev)
    ops.linear_ce_bwd(h.to(dev), w.to(dev), b.to(dev), tok.to(dev), R, K, G, V, lse, gout.to(dev), dl, seq=seq)
    check(dl.view(R * G, V), z.grad, "dlogits", max_tol=6e-3, l2_tol=4e-3)
    bad = tok.clone()
    bad[3] = V
    loss_bad, _ = ops.linear_ce_fwd(h.to(dev), w.to(dev), b.to(dev), bad.to(dev), R, K, G, V, seq=seq)
    assert torch.isnan(loss_bad).item()
    assert not ops.linear_ce_ok(R, K, G, 100) and not ops.linear_ce_ok(R, 72, G, V)


def test_adamw_clip_schedule(dev):
    from oracle import lrw_oracle as O
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(90)
    n, decay_end = 10007, 6000
    p = torch.randn(n, generator=g); grads = [torch.randn(n, generator=g) * s for s in (3.0, 0.01, 1.0)]
    m = torch.zeros(n); v = torch.zeros(n)
    pd, md, vd = p.to(dev), m.to(dev), v.to(dev)
    shadow = torch.zeros(n, dtype=BF, device=dev)
    state = torch.zeros(4 + 1024, dtype=torch.int32, device=dev)
    lr, betas, eps, wd, max_norm, warm, total = 1e-2, (0.9, 0.999), 1e-6, 0.01, 1.0, 2, 10
    # oracle: two "parameters" (decayed 2-D, undecayed 1-D)
    pa, pb = p[:decay_end].clone().view(-1, 1), p[decay_end:].clone()
    ma, mb, va, vb = torch.zeros_like(pa), torch.zeros_like(pb), torch.zeros_like(pa), torch.zeros_like(pb)
    for step, gr in enumerate(grads):
        gd = gr.to(dev)
        ops.grad_sumsq(gd, state)
        ops.adamw_step(pd, gd, md, vd, shadow, decay_end, lr, betas, eps, wd, max_norm, warm, total, state)
        ga, gb = gr[:decay_end].clone().view(-1, 1), gr[decay_end:].clone()
        O.clip_grad_norm([ga, gb], max_norm)
        O.adamw_step([pa, pb], [ga, gb], [ma, mb], [va, vb], step + 1, O.cosine_lr(step, lr, warm, total), betas, eps, wd)
    ref = torch.cat((pa.view(-1), pb))
    check(pd, ref, "adamw.p", 1e-5, 1e-5)
    check(shadow, ref, "adamw.shadow", 8e-3, 4e-3)
    st = state.cpu()
    assert int(st[0]) == 3


def test_colsum_rows_multi_equals_separate_launches(dev):
    """svsr_colsum_rows_multi: a layer's postponed parameter-gradient reductions (LayerNorm weight / bias, linear biases: autograd's accumulation
    into .grad) as one launch — every shape class of svsr_colsum_rows in one batch, 19 problems (two launches), accumulating into non-zero
    outputs: bit-identical to separate launches.  Two contributions to the same output stay separate launches, in order."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(17)
    shapes = [(512, 1536, 768, 768), (5, 70000, 70000, 0), (40, 3072, 3000, 0), (300, 9000, 9000, 0), (700, 6, 3, 3), (64, 768, 768, 0), (9, 40, 40, 0)]
    shapes = shapes + shapes + shapes[:5]
    fns_a, fns_b, outs_a, outs_b = [], [], [], []
    for rows, ld, n0, n1 in shapes:
        part = torch.randn(rows * ld, generator=g).to(dev)
        base0, base1 = torch.randn(n0, generator=g), (torch.randn(n1, generator=g) if n1 else None)
        for fns, outs in ((fns_a, outs_a), (fns_b, outs_b)):
            o0, o1 = base0.clone().to(dev), (base1.clone().to(dev) if n1 else None)
            fns.append(ops._deferred_colsum(part, rows, ld, o0, n0, o1, n1))
            outs.append((o0, o1))
    # a second contribution to the first problem's outputs
    extra = torch.randn(512 * 1536, generator=g).to(dev)
    fns_a.append(ops._deferred_colsum(extra, 512, 1536, outs_a[0][0], 768, outs_a[0][1], 768))
    fns_b.append(ops._deferred_colsum(extra, 512, 1536, outs_b[0][0], 768, outs_b[0][1], 768))
    ops.run_deferred(fns_a)
    for f in fns_b:
        f()
    torch.cuda.synchronize()
    for (a0, a1), (b0, b1) in zip(outs_a, outs_b):
        assert torch.equal(a0, b0) and (a1 is None or torch.equal(a1, b1))


def test_grad_sumsq_in_ranges(dev):
    """svsr_grad_sumsq_parts: the clip's sum of squares (Lightning's gradient_clip_val, lightning.py:216-223 via the Trainer) over two
    ranges into disjoint partial sums — what engine.TrainStep runs (everything behind the stem weight early, the stem weight last).  The
    norm AdamW then reads equals the fp64 norm of the whole buffer; a range with a ragged tail, partial sums of an earlier step overwritten."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(91)
    n, head = 1_000_003, 15680
    grad = (torch.randn(n, generator=g) * 0.3).to(dev)
    state = torch.zeros(4 + 1024, dtype=torch.int32, device=dev)
    state[4:] = torch.randn(1024, device=dev).view(torch.int32)           # stale partial sums
    ops.grad_sumsq_parts(grad, head, n - head, state, 0, ops.SUMSQ_PARTS - 1)
    ops.grad_sumsq_parts(grad, 0, head, state, ops.SUMSQ_PARTS - 1, 1)
    parts = state[4:].view(torch.float32).double().cpu()
    ref_tail = float((grad[head:].double() ** 2).sum()); ref_head = float((grad[:head].double() ** 2).sum())
    assert abs(float(parts[:-1].sum()) - ref_tail) <= 2e-6 * ref_tail
    assert abs(float(parts[-1]) - ref_head) <= 2e-6 * ref_head
    # through AdamW: one step with a clip that bites; the update equals the single-launch form's up to the norm's last bits
    p0 = torch.randn(n, generator=g).to(dev)
    outs = []
    for split in (True, False):
        pd = p0.clone(); md = torch.zeros(n, device=dev); vd = torch.zeros(n, device=dev); sh = torch.zeros(n, dtype=BF, device=dev)
        st = torch.zeros(4 + 1024, dtype=torch.int32, device=dev)
        if split:
            ops.grad_sumsq_parts(grad, head, n - head, st, 0, ops.SUMSQ_PARTS - 1)
            ops.grad_sumsq_parts(grad, 0, head, st, ops.SUMSQ_PARTS - 1, 1)
        else:
            ops.grad_sumsq(grad, st)
        ops.adamw_step(pd, grad, md, vd, sh, n, 1e-2, (0.9, 0.98), 1e-6, 0.03, 1.0, 0, 0, st)
        outs.append(pd)
    assert ((outs[0] - outs[1]).abs().max() / outs[1].abs().max()).item() <= 1e-6
    with pytest.raises(Exception):
        ops.grad_sumsq_parts(grad, 0, n, state, 1000, 100)                  # partial sums past the 1,024


def test_grouped_linear_weight_gradients_equal_separate_launches(dev):
    """svsr_igemm_wgrad_group: the encoder's / heads' nn.Linear weight gradients of a backward pass as ONE launch (reference
    lightning.py:82,92,107 via autograd).  Same workgroup code, one writer per element: the results must EQUAL those of separate
    svsr_igemm_wgrad launches bit for bit, bias gradients and sequence-sliced rows (the two heads) included."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(7)
    B, S, D = 4, 30, 512

    def mk(shape, scale=1.0):
        return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(dev)

    R = B * S
    shapes = [dict(rows=R, K=D, N=3 * D, bias=True), dict(rows=R, K=D, N=D, bias=True), dict(rows=R, K=D, N=2048, bias=False),
              dict(rows=R, K=2048, N=D, bias=True), dict(rows=B * (S - 1), K=D, N=1280, bias=True, seq=(S, 1, S - 1)),
              dict(rows=B, K=D, N=500, bias=True, seq=(S, 0, 1), dy_pitch=512)]
    problems, singles = [], []
    for sh in shapes:
        x = mk((R, sh["K"]))
        dyp = sh.get("dy_pitch", sh["N"])
        dy = mk((sh["rows"], dyp), 0.1)
        if dyp != sh["N"]:
            dy[:, sh["N"]:] = 0
        for store in (problems, singles):
            dw = torch.zeros((sh["N"], sh["K"]), dtype=torch.float32, device=dev)
            db = torch.zeros(sh["N"], dtype=torch.float32, device=dev) if sh["bias"] else None
            store.append(dict(x=x, dy=dy, dw=dw, db=db, rows=sh["rows"], K=sh["K"], N=sh["N"], x_pitch=sh["K"], dy_pitch=dyp, seq=sh.get("seq")))
    ops.linear_wgrad_group(problems)
    for q in singles:
        ops.linear_wgrad(q["x"], q["dy"], q["dw"], rows=q["rows"], K=q["K"], N=q["N"], x_pitch=q["x_pitch"], dy_pitch=q["dy_pitch"], seq=q["seq"], db=q["db"])
    torch.cuda.synchronize()
    for a, b, sh in zip(problems, singles, shapes):
        assert torch.equal(a["dw"], b["dw"]), sh
        assert float(a["dw"].abs().max()) > 0
        if sh["bias"]:
            assert torch.equal(a["db"], b["db"]), sh
    # and against torch on the first problem
    q = problems[0]
    ref = q["dy"].float().t() @ q["x"].float()
    assert ((q["dw"] - ref).norm() / ref.norm()).item() < 2e-3


@pytest.mark.parametrize("imgmajor", [1, 0])
@pytest.mark.parametrize("case", [(70, 6, 6, 72, 40, 3, 1, 1), (130, 5, 7, 64, 136, 3, 2, 1), (64, 4, 4, 128, 128, 1, 2, 0), (200, 3, 3, 136, 72, 3, 1, 1)])
def test_conv_wgrad_image_block_enumeration(dev, case, imgmajor):
    """svsr_igemm_wgrad's two row enumerations (plan word 0 bit 16; tune key wg_imgmajor): with >= 64 images a 64-row chunk is one
    output position of 64 consecutive images (wave-uniform DMA bases).  Cases: a last block with 6 / 2 / 8 images only, exactly one
    block, stride 2, a 1x1 stride-2 projection, channel counts that overhang the 64/128-wide tile (zero-page selects)."""
    from syncvsr_amd import ops

    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
    x = rnd((N, H, W, Ci), 16)
    dy = rnd((N, Ho, Wo, Co), 17, 0.25)
    ws = torch.zeros(Co, Ci, k, k, requires_grad=True)
    F.conv2d(nchw(x.float()), ws, stride=s, padding=p).backward(nchw(dy.float()))
    ops.tune("wg_imgmajor", imgmajor)
    try:
        plan = ops.wgrad_conv_plan(N, H, W, Ci, Co, k, s, p)
        assert (int(plan.words[0].item()) >> 16) & 1 == imgmajor
        dw = torch.zeros(Co, k, k, Ci, device=dev)
        ops.conv2d_wgrad(x.to(dev), dy.to(dev), dw, k, s, p, use_tr=False)
        dw2 = torch.zeros(Co, k, k, Ci, device=dev)
        ops.conv2d_wgrad(x.to(dev), dy.to(dev), dw2, k, s, p, use_tr=False)
        torch.cuda.synchronize()
    finally:
        ops.tune("wg_imgmajor", 1)
    assert torch.equal(dw, dw2)
    check(dw, ws.grad.permute(0, 2, 3, 1), f"conv_wgrad imgmajor={imgmajor}", 3e-3, 2e-3)


def test_grouped_weight_gradients_replay_from_a_hip_graph(dev):
    """svsr_igemm_wgrad_group inside a captured HIP graph: the problem table travels as kernel arguments (by value in the graph's
    nodes), so a replay long after the host-side problem list is gone still computes the same thing — 20 problems = two table
    chunks.  (A host-to-device copy node of the table kept a pointer into freed host memory: the replay aborted.)"""
    import os

    from syncvsr_amd import ops

    if os.environ.get("SVSR_REDZONE") == "1":
        # the red-zone allocator (tests/conftest.py) is a plain hipMalloc per tensor: an allocation inside a stream capture invalidates the
        # capture (torch's caching allocator serves captures from a private pool instead).  The launch itself is covered under red zones by
        # test_grouped_linear_weight_gradients_equal_separate_launches.
        pytest.skip("HIP graph capture needs torch's caching allocator")
    g = torch.Generator().manual_seed(11)
    R, K, N = 928, 512, 2048
    xs = [(torch.randn((R, K), generator=g)).to(torch.bfloat16).to(dev) for _ in range(20)]
    dys = [(torch.randn((R, N), generator=g) * 0.1).to(torch.bfloat16).to(dev) for _ in range(20)]
    dws = [torch.zeros((N, K), dtype=torch.float32, device=dev) for _ in range(20)]
    dbs = [torch.zeros(N, dtype=torch.float32, device=dev) for _ in range(20)]

    def problems():
        return [dict(x=x, dy=dy, dw=dw, db=db, rows=R, K=K, N=N, x_pitch=K, dy_pitch=N) for x, dy, dw, db in zip(xs, dys, dws, dbs)]

    plan = ops.wgrad_rows_plan(R, 1, 0, 0, K, N, True)
    assert plan.bc == 64 and plan.splits == 1 and int(plan.meta[1]) == 3, "the case must take the grouped launch"
    ops.linear_wgrad_group(problems())           # eager (also builds the plans outside the capture)
    torch.cuda.synchronize()
    want = [(dw.clone(), db.clone()) for dw, db in zip(dws, dbs)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            ops.linear_wgrad_group(problems())
    torch.cuda.current_stream().wait_stream(side)
    junk = [bytearray(1 << 16) for _ in range(64)]          # churn the host heap
    del junk
    for t in dws + dbs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for (dw, db), (wdw, wdb) in zip(zip(dws, dbs), want):
        assert torch.equal(dw, wdw) and torch.equal(db, wdb)
    assert float(dws[0].abs().max()) > 0
