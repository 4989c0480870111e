"""The batch-statistic kernels of the DC-TCN back-end (csrc/dctcn.hip: svsr_tconv_fwd_ext, svsr_tcn_colstats, svsr_tconv_apply,
svsr_tconv_epi_bwd_bs, svsr_tconv_bn_bwd, svsr_tconv_dgrad_ext, svsr_tconv_wgrad_ext, svsr_tcn_norm_pool_bwd_bs), each against an fp64 torch
restatement of its own inputs.

Bounds (nothing here is tuned to a result):
  * an fp32 accumulator of n bf16 x bf16 products lies within n * 2^-24 * sum |x| |w| of the exact sum (n = n_in * k <= 1344);
  * a bf16 result lies within one bf16 ulp of the fp64 one (2^-8 relative: the rounding's half ulp and the fp32 arithmetic in front of it,
    whose fast sigmoid is good to ~2^-20) plus 2^-16 of the magnitudes that were added on the way;
  * an fp32 sum of N terms in a fixed order lies within N * 2^-24 * sum |terms|.
Shapes: B = 3; T in {7, 29, 32, 33}; (k, d) from {(3, 1), (7, 5), (5, 8)} and their multi-branch sets — h = 16 = TC_HALO, h > T, an extent that
crosses a 32-row tile boundary the interior does not (T = 29, h >= 2), a trailing odd slot (B * tiles odd)."""
import pytest
import torch
import torch.nn.functional as F

from syncvsr_amd import dropout, ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
B, CO = 3, 64
# (kernel sizes of the launch, dilation, n_in, gated)
SETS = [((3,), 1, 64, False), ((3, 5, 7), 5, 192, True), ((5,), 8, 64, True), ((3, 5), 8, 192, False), ((7,), 5, 64, False)]
TS = (7, 29, 32, 33)
IDS = [f"k{'_'.join(map(str, ks))}-d{d}-n{n}-{'gated' if g else 'plain'}" for ks, d, n, g in SETS]


def _dev():
    return torch.device("cuda:0")


def _case(ks, d, n_in, gated, T, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * d + len(ks) + seed)
    x = torch.randn(B * T, n_in, generator=g).to(BF16)
    ws = [(torch.randn(CO, k, n_in, generator=g) / (n_in * k) ** 0.5).to(BF16) for k in ks]
    gates = [torch.rand(B, n_in, generator=g) if gated else None for _ in ks]
    return x, ws, gates


def _ref_acc(x, ws, gates, ks, d, T):
    """fp64 accumulators at every position of the full-padding convolution: [(B, CO, T + 2 h)] per branch, and sum |x| |w| beside them."""
    out = []
    for w, gt, k in zip(ws, gates, ks):
        xs = x.view(B, T, -1)
        if gt is not None:
            xs = (xs.float() * gt.unsqueeze(1)).to(BF16)
        xs = xs.double().transpose(1, 2)
        w64 = w.double().permute(0, 2, 1)
        out.append((F.conv1d(xs, w64, padding=(k - 1) * d, dilation=d), F.conv1d(xs.abs(), w64.abs(), padding=(k - 1) * d, dilation=d)))
    return out


def _run_fwd(x, ws, gates, ks, d, T):
    dev = _dev()
    brs = [dict(k=k, w=w.to(dev), gate=None if gt is None else gt.to(dev)) for k, w, gt in zip(ks, ws, gates)]
    acc = torch.full((B * (T + 2 * max(ops.tconv_halos(ks, d))), len(ks) * CO), float("nan"), dtype=torch.float32, device=dev)
    return ops.tconv_fwd_ext(x.to(dev), B=B, T=T, n_in=x.shape[1], d=d, branches=brs, co=CO, acc=acc)


def _own(acc, T, hmax, h, j):
    """Branch j's own rows of the extended buffer -> [B, T + 2 h, CO]"""
    return acc.view(B, T + 2 * hmax, -1)[:, hmax - h: hmax + h + T, j * CO: (j + 1) * CO]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ks,d,n_in,gated", SETS, ids=IDS)
def test_fwd_ext_and_colstats(ks, d, n_in, gated, T):
    x, ws, gates = _case(ks, d, n_in, gated, T)
    acc, hmax, hs = _run_fwd(x, ws, gates, ks, d, T)
    acc2, _, _ = _run_fwd(x, ws, gates, ks, d, T)
    stats = ops.tcn_colstats(acc, B=B, T=T, co=CO, hmax=hmax, hs=hs)
    stats2 = ops.tcn_colstats(acc2, B=B, T=T, co=CO, hmax=hmax, hs=hs)
    a, a2 = acc.cpu(), acc2.cpu()
    assert torch.equal(stats.cpu(), stats2.cpu())
    ext = a.view(B, T + 2 * hmax, -1)
    for j, ((ref, mag), h, k) in enumerate(zip(_ref_acc(x, ws, gates, ks, d, T), hs, ks)):
        got, got2 = _own(a, T, hmax, h, j), _own(a2, T, hmax, h, j)
        assert torch.equal(got, got2)
        err = (got.double() - ref.transpose(1, 2)).abs()
        assert bool((err <= n_in * k * 2.0 ** -24 * mag.transpose(1, 2) + 1e-30).all()), float(err.max())
        # rows outside the branch's own extent are not written
        outside = torch.cat([ext[:, : hmax - h, j * CO: (j + 1) * CO], ext[:, hmax + h + T:, j * CO: (j + 1) * CO]], 1)
        assert bool(torch.isnan(outside).all())
        own = got.double().reshape(-1, CO)
        N = own.shape[0]
        mean, m2 = own.mean(0), ((own - own.mean(0)) ** 2).sum(0)
        s = stats.cpu().double()[:, j * CO: (j + 1) * CO]
        assert bool(((s[0] - mean).abs() <= N * 2.0 ** -23 * own.abs().mean(0)).all())
        assert bool(((s[1] - m2).abs() <= N * 2.0 ** -21 * m2).all())


def _act(z, act, slope=None):
    if act == ops.ACT_SWISH:
        return z * torch.sigmoid(z)
    if act == ops.ACT_PRELU:
        return torch.where(z >= 0, z, z * slope)
    return z


def _epi_setup(ks, d, T, seed, with_res, act):
    """Extended accumulators with a fixed fill, BatchNorm vectors from their own statistics, dy, res, and the fp64 chain."""
    hs = ops.tconv_halos(ks, d)
    hmax, C = max(hs), len(ks) * CO
    g = torch.Generator().manual_seed(seed)
    acc = torch.randn(B * (T + 2 * hmax), C, generator=g) * 1.5 + 0.3
    dy = torch.randn(B * T, C, generator=g).to(BF16)
    res = torch.randn(B * T, C, generator=g).to(BF16) if with_res else None
    weight, bias = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    slope = torch.rand(C, generator=g) * 0.5 if act == ops.ACT_PRELU else None
    return hs, hmax, C, acc, dy, res, weight, bias, slope


def _chain64(acc, dy, res, weight, bias, slope, hs, hmax, T, act, res_act, keep, p):
    """autograd in fp64 of the stage from the extended accumulators on: -> out [B*T, C], dacc_ext, dres, d weight, d bias, d slope, and the
    batch vectors (mean, invstd)."""
    C = acc.shape[1]
    a = acc.double().view(B, T + 2 * hmax, C).clone().requires_grad_(True)
    w, b_ = weight.double().clone().requires_grad_(True), bias.double().clone().requires_grad_(True)
    sl = None if slope is None else slope.double().clone().requires_grad_(True)
    r = None if res is None else res.double().clone().requires_grad_(True)
    cols, means, istds = [], [], []
    for j, h in enumerate(hs):
        own = a[:, hmax - h: hmax + h + T, j * CO: (j + 1) * CO]
        mean, var = own.mean((0, 1)), own.var((0, 1), unbiased=False)
        istd = 1.0 / torch.sqrt(var + ops.BN_EPS)
        z = (own - mean) * istd * w[j * CO: (j + 1) * CO] + b_[j * CO: (j + 1) * CO]
        cols.append(z[:, h: h + T])
        means.append(mean.detach()); istds.append(istd.detach())
    z = torch.cat(cols, 2).reshape(B * T, C)
    y = _act(z, act, sl)
    if keep is not None:
        y = y * keep / (1.0 - p)
    if r is not None:
        y = y + r
        if res_act == ops.ACT_SWISH:
            y = _act(y, ops.ACT_SWISH)
    y.backward(dy.double())
    return (y.detach(), a.grad.view(-1, C), None if r is None else r.grad, w.grad, b_.grad, None if sl is None else sl.grad, torch.cat(means),
            torch.cat(istds))


EPI = [((3, 5, 7), 5, ops.ACT_SWISH, True, 0.2), ((5,), 8, ops.ACT_SWISH, False, 0.2), ((1,), 1, ops.ACT_PRELU, False, 0.0),
       ((3, 5), 8, ops.ACT_SWISH, True, 0.0)]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ks,d,act,with_res,p", EPI, ids=[f"k{'_'.join(map(str, e[0]))}-d{e[1]}-act{e[2]}-res{int(e[3])}-p{e[4]}" for e in EPI])
def test_apply_and_epilogue_backward(ks, d, act, with_res, p, T):
    dev = _dev()
    hs, hmax, C, acc, dy, res, weight, bias, slope = _epi_setup(ks, d, T, 77 + T, with_res, act)
    res_act = ops.ACT_SWISH if with_res else ops.ACT_NONE
    seed, site = 9, 4
    drop = (dropout.site_key(seed, site), p) if p else None
    keep = torch.from_numpy(dropout.keep_mask(seed, site, p, B * T * C)).view(B * T, C).double() if p else None
    ref_out, ref_dacc, ref_dres, ref_dw, ref_db, ref_dsl, mean64, istd64 = _chain64(acc, dy, res, weight, bias, slope, hs, hmax, T, act, res_act, keep, p)
    to = lambda t: None if t is None else t.to(dev)          # noqa: E731
    acc_d, dy_d, res_d, slope_d = to(acc), to(dy), to(res), to(slope)
    stats = ops.tcn_colstats(acc_d, B=B, T=T, co=CO, hmax=hmax, hs=hs)
    n = torch.tensor([float(B * (T + 2 * h)) for h in hs], device=dev).repeat_interleave(CO)
    scale, shift, mean, invstd, _ = ops.bn_batch_affine(stats, n, to(weight), to(bias))
    assert bool(((mean.cpu().double() - mean64).abs() <= 1e-5 * (1 + mean64.abs())).all())
    geo = dict(B=B, T=T, co=CO, hmax=hmax, hs=hs, act=act, slope=slope_d, res=res_d, res_act=res_act, drop=drop)
    out = torch.zeros((B * T, C + 64), dtype=BF16, device=dev)
    ops.tconv_apply(acc_d, scale, shift, out=out[:, 64:], **geo)
    got = out[:, 64:].cpu().double()
    mag = 1.0 + (res.double().abs() if res is not None else 0.0)
    # 2^-8 of the result, 2^-16 of what was added, and the fp32 statistics' own error in z (1e-5 of 1 + |z|, z = O(5)) through act' <= 1.1
    assert bool(((got - ref_out).abs() <= 2.0 ** -8 * ref_out.abs() + 2.0 ** -16 * mag + 1e-4 / (1.0 - p)).all()), float((got - ref_out).abs().max())
    assert float(out[:, :64].abs().max()) == 0.0
    if p:
        assert bool(((got == 0) | (keep > 0) | (res is not None)).all())
    # pass 1
    dres, sums = ops.tconv_epi_bwd_bs(dy_d, acc_d, scale, shift, **geo)
    dres2, sums2 = ops.tconv_epi_bwd_bs(dy_d, acc_d, scale, shift, **geo)
    assert torch.equal(sums, sums2) and (dres is None or torch.equal(dres, dres2))
    dw, db, ca, cb = ops.bn_batch_param_grads(sums[0], sums[1], mean, invstd, n)
    tol = lambda ref: 4e-3 * ref.abs() + 4e-3 * ref.abs().mean()          # noqa: E731  sums of B*T <= 99 bf16-input terms: 2^-8 per term
    assert bool(((db.cpu().double() - ref_db).abs() <= tol(ref_db)).all())
    assert bool(((dw.cpu().double() - ref_dw).abs() <= tol(ref_dw)).all())
    if with_res:
        e = (dres.cpu().double() - ref_dres).abs()
        assert bool((e <= 2.0 ** -8 * ref_dres.abs() + 1e-4).all()), float(e.max())
    if act == ops.ACT_PRELU:
        assert bool(((sums[2].cpu().double() - ref_dsl).abs() <= tol(ref_dsl)).all())
    # pass 2
    dacc = ops.tconv_bn_bwd(dy_d, acc_d, scale, shift, mean, invstd, ca, cb, **geo)
    dacc2 = ops.tconv_bn_bwd(dy_d, acc_d, scale, shift, mean, invstd, ca, cb, **geo)
    assert torch.equal(dacc, dacc2)
    got = dacc.cpu().double()
    e = (got - ref_dacc).abs()
    # one bf16 rounding of the result; the terms ca, cb carry pass 1's sum error (4e-3 relative) scaled by scale = O(1)
    bound = 2.0 ** -8 * ref_dacc.abs() + 4e-3 * (ca.cpu().double().abs() + cb.cpu().double().abs() * 4.0) * scale.cpu().double().abs() + 1e-5
    assert bool((e <= bound).all()), float((e - bound).max())
    ext = got.view(B, T + 2 * hmax, C)
    for j, h in enumerate(hs):          # zeros outside a branch's own rows
        assert float(ext[:, : hmax - h, j * CO: (j + 1) * CO].abs().max() if hmax > h else 0.0) == 0.0
        assert float(ext[:, hmax + h + T:, j * CO: (j + 1) * CO].abs().max() if hmax > h else 0.0) == 0.0


@pytest.mark.parametrize("T", (7, 33))
def test_pass1_without_dropout_and_halo_keeps_the_bits_of_epi_bwd(T):
    """hmax = 0, p = 0: the sums and dres of svsr_tconv_epi_bwd, bit for bit."""
    dev = _dev()
    for act, with_res in ((ops.ACT_SWISH, True), (ops.ACT_PRELU, False), (ops.ACT_SWISH, False)):
        hs, hmax, C, acc, dy, res, weight, bias, slope = _epi_setup((1,), 1, T, 5 + T, with_res, act)
        to = lambda t: None if t is None else t.to(dev)          # noqa: E731
        res_act = ops.ACT_SWISH if with_res else ops.ACT_NONE
        _, dres0, sums0 = ops.tconv_epi_bwd(to(dy), to(acc), to(weight), to(bias), rows=B * T, C=C, act=act, slope=to(slope), res=to(res), res_act=res_act)
        dres1, sums1 = ops.tconv_epi_bwd_bs(to(dy), to(acc), to(weight), to(bias), B=B, T=T, co=CO, hmax=0, hs=[0], act=act, slope=to(slope),
                                            res=to(res), res_act=res_act)
        assert torch.equal(sums0, sums1)
        assert dres0 is None and dres1 is None or torch.equal(dres0, dres1)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ks,d,n_in,gated", SETS, ids=IDS)
def test_dgrad_and_wgrad_over_extended_rows(ks, d, n_in, gated, T):
    dev = _dev()
    x, ws, gates = _case(ks, d, n_in, gated, T, seed=3)
    hs = ops.tconv_halos(ks, d)
    hmax, nb = max(hs), len(ks)
    g = torch.Generator().manual_seed(T + d)
    dacc = torch.randn(B, T + 2 * hmax, nb * CO, generator=g)
    for j, h in enumerate(hs):          # zeros outside a branch's own rows, as svsr_tconv_bn_bwd writes them
        dacc[:, : hmax - h, j * CO: (j + 1) * CO] = 0
        dacc[:, hmax + h + T:, j * CO: (j + 1) * CO] = 0
    dacc = dacc.reshape(-1, nb * CO).to(BF16)
    # fp64: autograd of sum_j <conv_full(bf16(x * gate_j), w_j), dacc_j>
    x64 = x.double().view(B, T, n_in)
    dx_ref, dw_ref, dgate_ref, mag = torch.zeros(B, T, n_in, dtype=torch.float64), [], [], torch.zeros(B, T, n_in, dtype=torch.float64)
    for j, (w, gt, k, h) in enumerate(zip(ws, gates, ks, hs)):
        xg = (x.view(B, T, n_in).float() * gt.unsqueeze(1)).to(BF16).double() if gt is not None else x64
        xg = xg.clone().requires_grad_(True)
        w64 = w.double().permute(0, 2, 1).clone().requires_grad_(True)
        full = F.conv1d(xg.transpose(1, 2), w64, padding=(k - 1) * d, dilation=d)                # [B, CO, T + 2 h]
        dj = dacc.double().view(B, T + 2 * hmax, -1)[:, hmax - h: hmax + h + T, j * CO: (j + 1) * CO].transpose(1, 2)
        (full * dj).sum().backward()
        dxg = xg.grad
        mag += F.conv_transpose1d(dj.abs(), w64.detach().abs(), padding=(k - 1) * d, dilation=d).transpose(1, 2) * (1.0 if gt is None else gt.double().unsqueeze(1))
        dx_ref += dxg * (gt.double().unsqueeze(1) if gt is not None else 1.0)
        dgate_ref.append(None if gt is None else (dxg * x64).sum(1))
        dw_ref.append(w64.grad.permute(0, 1, 2))                                                 # [CO, n_in, k]: the parameter's layout
    xd, dd = x.to(dev), dacc.to(dev)
    brs = [dict(k=k, wt=ops.tconv_wt(w.permute(0, 2, 1).contiguous()).to(dev), dy_off=j * CO, gate=None if gt is None else gt.to(dev))
           for j, (k, w, gt) in enumerate(zip(ks, ws, gates))]
    out = torch.zeros((B * T, n_in), dtype=BF16, device=dev)
    gpart = ops.tconv_dgrad(dd, B=B, T=T, co=CO, d=d, n_out=n_in, out=out, x=xd if gated else None, branches=brs, hmax=hmax)
    out2 = torch.zeros_like(out)
    gpart2 = ops.tconv_dgrad(dd, B=B, T=T, co=CO, d=d, n_out=n_in, out=out2, x=xd if gated else None, branches=brs, hmax=hmax)
    assert torch.equal(out, out2) and (gpart is None or torch.equal(gpart, gpart2))
    e = (out.cpu().double().view(B, T, n_in) - dx_ref).abs()
    assert bool((e <= 2.0 ** -8 * dx_ref.abs() + CO * 7 * len(ks) * 2.0 ** -24 * mag + 1e-30).all()), float(e.max())
    if gated:
        gp = gpart.cpu().double().sum(2)
        for j in range(nb):
            ref = dgate_ref[j]
            assert bool(((gp[j] - ref).abs() <= 1e-4 * ref.abs() + 1e-4 * ref.abs().mean()).all())
    # with zero rows around the interior the extended data gradient is the plain one, bit for bit (the same MFMA sequence over the same values)
    inner = torch.zeros(B, T + 2 * hmax, nb * CO, dtype=BF16)
    inner[:, hmax: hmax + T] = dacc.view(B, T + 2 * hmax, -1)[:, hmax: hmax + T]
    o_ext, o_plain = torch.zeros_like(out), torch.zeros_like(out)
    ops.tconv_dgrad(inner.reshape(-1, nb * CO).to(dev), B=B, T=T, co=CO, d=d, n_out=n_in, out=o_ext, x=xd if gated else None, branches=brs, hmax=hmax)
    ops.tconv_dgrad(inner[:, hmax: hmax + T].reshape(-1, nb * CO).contiguous().to(dev), B=B, T=T, co=CO, d=d, n_out=n_in, out=o_plain,
                    x=xd if gated else None, branches=brs)
    assert torch.equal(o_ext, o_plain)
    o_zero = torch.zeros_like(out)          # shift 0 through the generalised entry: the existing entry point's bits
    ops.tconv_dgrad(inner[:, hmax: hmax + T].reshape(-1, nb * CO).contiguous().to(dev), B=B, T=T, co=CO, d=d, n_out=n_in, out=o_zero,
                    x=xd if gated else None, branches=brs, hmax=0)
    assert torch.equal(o_zero, o_plain)
    for j, (k, gt, ref) in enumerate(zip(ks, gates, dw_ref)):
        dw = torch.zeros((CO, n_in, k), dtype=torch.float32, device=dev)
        kw = dict(B=B, T=T, n_in=n_in, co=CO, k=k, d=d, gate=None if gt is None else gt.to(dev))
        ops.tconv_wgrad(xd, dd[:, j * CO: (j + 1) * CO], dw, hmax=hmax, **kw)
        dw2 = torch.zeros_like(dw)
        ops.tconv_wgrad(xd, dd[:, j * CO: (j + 1) * CO], dw2, hmax=hmax, **kw)
        assert torch.equal(dw, dw2)
        e = (dw.cpu().double() - ref).abs()
        n_terms = B * (T + 2 * hmax)
        assert bool((e <= n_terms * 2.0 ** -24 * 64.0 + 1e-6 * ref.abs()).all()), float(e.max())          # |x| |dy| <= 64 per term (4 sigma each)
        # hmax = 0 through the generalised entry: the existing entry point's bits
        plain = dd.view(B, T + 2 * hmax, -1)[:, hmax: hmax + T, j * CO: (j + 1) * CO].reshape(B * T, CO).contiguous()
        d0, d1 = torch.zeros_like(dw), torch.zeros_like(dw)
        ops.tconv_wgrad(xd, plain, d0, **kw)
        ops.tconv_wgrad(xd, plain, d1, hmax=0, **kw)
        assert torch.equal(d0, d1)


@pytest.mark.parametrize("T", (7, 29))
def test_norm5_batch_statistics(T):
    dev = _dev()
    C = 320
    g = torch.Generator().manual_seed(T)
    x = (torch.randn(B * T, C, generator=g) * 2 + 1).to(BF16)
    dh, dp = torch.randn(B * T, C, generator=g).to(BF16), torch.randn(B, C, generator=g).to(BF16)
    mask = (torch.rand(B, T, generator=g) > 0.3).float()
    weight, bias = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    xd = x.to(dev)
    stats = ops.tcn_colstats(xd, B=B, T=T, co=C)
    x64 = x.double().clone().requires_grad_(True)
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    assert bool(((stats[0].cpu().double() - mean.detach()).abs() <= 1e-5 * (1 + mean.detach().abs())).all())
    assert bool(((stats[1].cpu().double() - var.detach() * B * T).abs() <= 1e-4 * var.detach() * B * T).all())
    hn = (x64 - mean) / torch.sqrt(var + ops.BN_EPS) * weight.double() + bias.double()
    gsum = dh.double() + (dp.double().unsqueeze(1) * (mask.double() / (mask.double().sum(1, keepdim=True) + 1e-6)).unsqueeze(2)).reshape(B * T, C)
    hn.backward(gsum)
    n = torch.full((C,), float(B * T), device=dev)
    scale, shift, mu, istd, _ = ops.bn_batch_affine(stats, n, weight.to(dev), bias.to(dev))
    out = torch.zeros((B * T, C), dtype=BF16, device=dev)
    _, sums = ops.tcn_norm_pool_bwd(dh.to(dev), dp.to(dev), xd, scale, mask.to(dev).contiguous(), B=B, T=T, C=C, out=out)
    dw, db, ca, cb = ops.bn_batch_param_grads(sums[0], sums[1], mu, istd, n)
    ops.tcn_norm_pool_bwd_bs(dh.to(dev), dp.to(dev), xd, scale, mu, istd, ca, cb, mask.to(dev).contiguous(), B=B, T=T, C=C, out=out)
    e = (out.cpu().double() - x64.grad).abs()
    assert bool((e <= 2.0 ** -8 * x64.grad.abs() + 1e-4 * (1 + gsum.abs())).all()), float(e.max())
