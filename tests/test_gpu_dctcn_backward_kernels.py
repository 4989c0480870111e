"""GPU parity of the DC-TCN backward kernels (csrc/dctcn.hip), each alone, against fp32 torch on the same bf16-rounded operands.  Bound: the
one tests/test_gpu_dctcn_kernels.py applies to svsr_tconv_fwd (fp32 accumulation order and one bf16 store are the only differences); fp32
outputs (weight gradients, sums) have no bf16 store and stay far inside it.  Every output is a view into a sentinel-filled buffer."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_dctcn_kernels import LINEAR_BOUND, _r, _rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"
SENT = 7.0


def _conv(x, w, k, d):          # x [B, T, ci] fp32, w [co, ci, k] -> [B, T, co]
    return F.conv1d(x.transpose(1, 2), w, None, padding=(k - 1) * d // 2, dilation=d).transpose(1, 2)


def _dgrad_case(B, T, n_in, co, ks, d, gated, addend, cadd, seed, change_clip=None, off=0):
    from syncvsr_amd import ops

    nb, pitch = len(ks), off + n_in + 64          # the output is the view [:, off: off + n_in] of a wider sentinel-filled buffer
    dy = (_r(B * T, nb * co + 8, seed=seed) * 0.5).to(BF)
    x = _r(B * T, n_in + 8, seed=seed + 1).to(BF)
    if change_clip is not None:
        dy[change_clip * T: (change_clip + 1) * T] += 1.0
        x[change_clip * T: (change_clip + 1) * T] += 1.0
    out = torch.full((B * T + 2, pitch), SENT, dtype=BF)
    add = _r(B * T, n_in, seed=seed + 2).to(BF)
    if addend:
        out[: B * T, off: off + n_in] = add
    ca = _r(B, n_in, seed=seed + 3) if cadd else None
    ref = add.float().view(B, T, n_in).clone() if addend else torch.zeros(B, T, n_in)
    if cadd:
        ref += ca.unsqueeze(1) / T
    branches, gref = [], []
    for i, k in enumerate(ks):
        w = (_r(co, n_in, k, seed=seed + 10 + i) / (co * k) ** 0.5).to(BF)
        gate = torch.sigmoid(_r(B, n_in, seed=seed + 20 + i)) if gated else None
        dyi = dy[:, i * co: (i + 1) * co].float().view(B, T, co)
        xi = torch.zeros(B, T, n_in, requires_grad=True)
        (_conv(xi, w.float(), k, d) * dyi).sum().backward()
        dxg = xi.grad
        ref += dxg * gate.unsqueeze(1) if gated else dxg
        if gated:
            gref.append((x[:, :n_in].float().view(B, T, n_in) * dxg).sum(1))
        br = dict(k=k, wt=ops.tconv_wt(w).to(DEV), dy_off=i * co)
        if gated:
            br["gate"] = gate.to(DEV).contiguous()
        branches.append(br)
    full = out.to(DEV)
    o = full[:, off: off + n_in]
    gp = ops.tconv_dgrad(dy.to(DEV), B=B, T=T, co=co, d=d, n_out=n_in, out=o, branches=branches, x=x.to(DEV) if gated else None,
                         addend=o if addend else None, cadd=None if ca is None else ca.to(DEV), cadd_scale=1.0 / T)
    torch.cuda.synchronize()
    got = full.cpu()
    assert bool((got[: B * T, off + n_in:].float() == SENT).all()) and bool((got[B * T:].float() == SENT).all()), "guard band overwritten"
    assert bool((got[:, :off].float() == SENT).all()), "guard band in front of the written channels overwritten"
    got = got[:, off:]
    err = _rel_err(got[: B * T, :n_in].float(), ref.reshape(B * T, n_in))
    print(f"dgrad B={B} T={T} n_in={n_in} co={co} ks={ks} d={d} gated={gated} add={addend}: rel err {err:.3e}")
    assert err < LINEAR_BOUND
    if gated:
        assert tuple(gp.shape) == (nb, B, (T + 31) // 32, n_in)
        gsum = gp.sum(2).cpu()
        for i in range(nb):
            e = _rel_err(gsum[i], gref[i])
            print(f"   gate partials branch {i}: rel err {e:.3e}")
            assert e < LINEAR_BOUND
    return got[: B * T, :n_in].clone(), (None if gp is None else gp.cpu())


@pytest.mark.parametrize("T", [1, 2, 29, 32, 33, 65])
@pytest.mark.parametrize("k,d", [(1, 1), (3, 1), (5, 2), (7, 5)])
def test_dgrad_every_length_and_tap_reach(T, k, d):
    B = {1: 3, 2: 2, 29: 3, 32: 1, 33: 2, 65: 3}[T]
    _dgrad_case(B, T, 64 if k == 7 else 192, 64, (k,), d, k != 1, T % 2 == 1, T in (29, 33), seed=T * 10 + k)


@pytest.mark.parametrize("nb,n_in,co", [(1, 576, 128), (2, 192, 64), (3, 576, 64), (3, 64, 128)])
def test_dgrad_branch_counts_and_widths(nb, n_in, co):
    _dgrad_case(3, 33, n_in, co, (3, 5, 7)[:nb], 2, True, True, True, seed=500 + nb + n_in)
    _dgrad_case(2, 29, n_in, co, (3, 5, 7)[:nb], 5 if nb < 3 else 2, False, False, False, seed=600 + nb + n_in)


@pytest.mark.parametrize("gated", [False, True])
def test_dgrad_written_at_a_channel_offset_in_place(gated):
    """out, addend (the same view) and, gated, the gate partials with the output view starting at channel 128 of a wider buffer."""
    _dgrad_case(3, 33, 192, 64, (3, 5, 7), 2, gated, True, True, seed=650 + gated, off=128)
    _dgrad_case(2, 29, 64, 128, (7,), 5, gated, True, False, seed=660 + gated, off=64)


def test_dgrad_clip_isolation_and_determinism():
    a, ga = _dgrad_case(3, 33, 192, 64, (3, 7), 5, True, True, True, seed=700)
    b, gb = _dgrad_case(3, 33, 192, 64, (3, 7), 5, True, True, True, seed=700)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(ga, gb)
    c, gc = _dgrad_case(3, 33, 192, 64, (3, 7), 5, True, True, True, seed=700, change_clip=1)
    for clip in (0, 2):
        assert torch.equal(a[clip * 33: (clip + 1) * 33].view(torch.int16), c[clip * 33: (clip + 1) * 33].view(torch.int16))
        assert torch.equal(ga[:, clip], gc[:, clip])
    assert not torch.equal(a[33:66], c[33:66])


@pytest.mark.parametrize("B,T", [(1, 1), (2, 2), (3, 29), (1, 32), (2, 33), (3, 65)])
@pytest.mark.parametrize("k,d", [(1, 1), (3, 1), (5, 2), (7, 5)])
def test_wgrad_every_length_and_tap_reach(B, T, k, d):
    from syncvsr_amd import ops

    n_in, co, n_valid = {1: (576, 128, 513), 3: (192, 64, 192), 5: (64, 128, 64), 7: (64, 64, 64)}[k]
    gated = k != 1
    seed = B * 100 + T + k
    x = _r(B * T, n_in + 8, seed=seed).to(BF)
    dy = (_r(B * T, co + 16, seed=seed + 1) * 0.5).to(BF)
    gate = torch.sigmoid(_r(B, n_in, seed=seed + 2)) if gated else None
    xin = x[:, :n_in].float().view(B, T, n_in)
    if gated:
        xin = (xin * gate.unsqueeze(1)).to(BF).float()
    w = torch.zeros(co, n_in, k, requires_grad=True)
    (_conv(xin, w, k, d) * dy[:, 8: 8 + co].float().view(B, T, co)).sum().backward()
    ref = w.grad[:, :n_valid]
    buf = torch.full((co * n_valid * k + 64,), SENT).to(DEV)
    dw = buf[32: 32 + co * n_valid * k].view(co, n_valid, k)
    args = dict(B=B, T=T, n_in=n_in, co=co, k=k, d=d, gate=None if gate is None else gate.to(DEV).contiguous())
    xd, dyd = x.to(DEV), dy.to(DEV)[:, 8: 8 + co]
    ops.tconv_wgrad(xd, dyd, dw, **args)
    torch.cuda.synchronize()
    first = dw.cpu().clone()
    err = _rel_err(first, ref)
    print(f"wgrad B={B} T={T} k={k} d={d} gated={gated}: rel err {err:.3e}")
    assert err < LINEAR_BOUND
    assert bool((buf[:32] == SENT).all()) and bool((buf[32 + co * n_valid * k:] == SENT).all()), "guard band overwritten"
    ops.tconv_wgrad(xd, dyd, dw, **args)                                     # determinism, then add
    assert torch.equal(dw.cpu(), first)
    ops.tconv_wgrad(xd, dyd, dw, add=True, **args)
    assert torch.equal(dw.cpu(), first + first)
    if B * ((T + 31) // 32) >= 4:                                            # another split of the rows: same sum, another order
        ops.tconv_wgrad(xd, dyd, dw, splits=2, **args)
        assert _rel_err(dw.cpu(), ref) < LINEAR_BOUND


@pytest.mark.parametrize("rows,C,act,residual", [(1, 64, 2, False), (65, 192, 2, True), (87, 128, 3, False), (130, 64, 0, False), (64, 576, 2, True)])
def test_epilogue_backward(rows, C, act, residual):
    from syncvsr_amd import ops

    seed = rows + C
    dyw = torch.full((rows, C + 72), SENT, dtype=BF)
    dyw[:, 8: 8 + C] = _r(rows, C, seed=seed).to(BF)
    acc = _r(rows, C, seed=seed + 1)
    scale, shift, slope = 1 + 0.2 * _r(C, seed=seed + 2), 0.1 * _r(C, seed=seed + 3), 0.25 + 0.05 * _r(C, seed=seed + 4)
    scale[3] = 0.0                                                           # BatchNorm weight exactly 0
    res = _r(rows, C, seed=seed + 5).to(BF) if residual else None
    a = acc.clone().requires_grad_(True)
    r = res.float().clone().requires_grad_(True) if residual else None
    z = a * scale + shift
    z.retain_grad()
    y = z * torch.sigmoid(z) if act == 2 else torch.where(z >= 0, z, z * slope) if act == 3 else z
    if residual:
        y = y + r
        y = y * torch.sigmoid(y)
    dy = dyw[:, 8: 8 + C].float()
    (y * dy).sum().backward()
    dacc_buf = torch.full((rows + 1, C + 16), SENT, dtype=BF).to(DEV)
    dres_buf = torch.full((rows + 1, C + 16), SENT, dtype=BF).to(DEV)
    dacc, dres, sums = ops.tconv_epi_bwd(dyw.to(DEV)[:, 8: 8 + C], acc.to(DEV), scale.to(DEV), shift.to(DEV), rows=rows, C=C, act=act,
                                         slope=slope.to(DEV) if act == 3 else None, res=None if res is None else res.to(DEV),
                                         res_act=2 if residual else 0, dacc=dacc_buf[:rows, 8: 8 + C], dres=dres_buf[:rows, 8: 8 + C] if residual else None)
    torch.cuda.synchronize()
    sums = sums.cpu()
    g_ref = z.grad                                                           # dL/dz from autograd: no division by scale, channel 3 included
    assert _rel_err(dacc.float().cpu(), a.grad) < LINEAR_BOUND and bool(torch.isfinite(sums).all())
    assert float(dacc.float().cpu()[:, 3].abs().max()) == 0.0
    assert _rel_err(sums[0], g_ref.sum(0)) < LINEAR_BOUND and _rel_err(sums[1], (g_ref * acc).sum(0)) < LINEAR_BOUND
    assert _rel_err(sums[0][3], g_ref.sum(0)[3]) < LINEAR_BOUND and _rel_err(sums[1][3], (g_ref * acc).sum(0)[3]) < LINEAR_BOUND
    assert float(sums[1][3].abs()) > 0                                       # d bn.weight is not zero exactly where the weight is
    if act == 3:
        zz = (acc * scale + shift)
        assert _rel_err(sums[2], (dy * zz.clamp(max=0)).sum(0)) < LINEAR_BOUND
    if residual:
        assert _rel_err(dres.float().cpu(), r.grad) < LINEAR_BOUND and _rel_err(sums[3], r.grad.sum(0)) < LINEAR_BOUND
    again = ops.tconv_epi_bwd(dyw.to(DEV)[:, 8: 8 + C], acc.to(DEV), scale.to(DEV), shift.to(DEV), rows=rows, C=C, act=act,
                              slope=slope.to(DEV) if act == 3 else None, res=None if res is None else res.to(DEV), res_act=2 if residual else 0)
    assert torch.equal(again[0].view(torch.int16), dacc.contiguous().view(torch.int16)) and torch.equal(again[2].cpu(), sums)      # same bits twice
    assert not residual or torch.equal(again[1].view(torch.int16), dres.contiguous().view(torch.int16))
    for buf in (dacc_buf, dres_buf) if residual else (dacc_buf,):
        b = buf.float().cpu()
        assert bool((b[:, :8] == SENT).all()) and bool((b[:, 8 + C:] == SENT).all()) and bool((b[rows:] == SENT).all()), "guard band overwritten"


@pytest.mark.parametrize("B,T,n_in", [(1, 1, 64), (2, 33, 192), (3, 29, 576), (3, 65, 192)])
def test_se_backward(B, T, n_in):
    from syncvsr_amd import ops

    nb, Rr = 3, n_in // 16
    x = _r(B * T, n_in + 64, seed=1).to(BF)
    w1 = (_r(nb, Rr, n_in, seed=2) / n_in ** 0.5).to(BF)
    w2 = (_r(nb, n_in, Rr, seed=3) / Rr ** 0.5).to(BF)
    n_tt = (T + 31) // 32
    gpart = _r(nb, B, n_tt, n_in, seed=4)
    gate = ops.tcn_se_fwd(x.to(DEV), w1.to(DEV), w2.to(DEV), B=B, T=T, n_in=n_in)
    m = x[:, :n_in].float().view(B, T, n_in).mean(1).requires_grad_(True)
    a, b = w1.float().requires_grad_(True), w2.float().requires_grad_(True)
    tot = 0
    for i in range(nb):
        hid = m @ a[i].T
        tot = tot + (torch.sigmoid((hid * torch.sigmoid(hid)) @ b[i].T) * gpart[i].sum(1)).sum()
    tot.backward()
    buf = torch.full((2 * nb * Rr * n_in + 64,), SENT).to(DEV)
    dw1 = [buf[32 + i * Rr * n_in: 32 + (i + 1) * Rr * n_in].view(Rr, n_in) for i in range(nb)]
    dw2 = [buf[32 + (nb + i) * Rr * n_in: 32 + (nb + i + 1) * Rr * n_in].view(n_in, Rr) for i in range(nb)]
    dm = ops.tcn_se_bwd(x.to(DEV), w1.to(DEV), w2.to(DEV), gate, gpart.to(DEV), dw1, dw2, B=B, T=T, n_in=n_in)
    torch.cuda.synchronize()
    first = buf.cpu().clone()
    assert _rel_err(dm.cpu(), m.grad) < LINEAR_BOUND                         # (fp32 throughout: far inside the shared bound)
    for i in range(nb):
        assert _rel_err(dw1[i].cpu(), a.grad[i]) < LINEAR_BOUND and _rel_err(dw2[i].cpu(), b.grad[i]) < LINEAR_BOUND
    assert bool((first[:32] == SENT).all()) and bool((first[-32:] == SENT).all()), "guard band overwritten"
    dm2 = ops.tcn_se_bwd(x.to(DEV), w1.to(DEV), w2.to(DEV), gate, gpart.to(DEV), dw1, dw2, B=B, T=T, n_in=n_in)
    assert torch.equal(dm2, dm) and torch.equal(buf.cpu(), first)


def test_norm_pool_backward_and_saved_accumulators():
    from syncvsr_amd import ops

    B, T, C = 3, 29, 320
    x = _r(B * T, C + 64, seed=1).to(BF)
    dh, dp = _r(B * T, C, seed=2).to(BF), _r(B, C, seed=3).to(BF)
    scale = 1 + 0.1 * _r(C, seed=4)
    mask = torch.ones(B, T)
    mask[1, 1:] = 0
    mask[2, 11:] = 0
    out = torch.full((B * T + 1, C + 64), SENT, dtype=BF).to(DEV)
    _, sums = ops.tcn_norm_pool_bwd(dh.to(DEV), dp.to(DEV), x.to(DEV), scale.to(DEV), mask.to(DEV), B=B, T=T, C=C, out=out)
    torch.cuda.synchronize()
    g = dh.float().view(B, T, C) + dp.float().unsqueeze(1) * (mask / (mask.sum(1, keepdim=True) + 1e-6)).unsqueeze(2)
    o = out.float().cpu()
    assert _rel_err(o[: B * T, :C], (g * scale).reshape(B * T, C)) < LINEAR_BOUND
    assert bool((o[:, C:] == SENT).all()) and bool((o[B * T:] == SENT).all())
    assert _rel_err(sums[0].cpu(), g.sum((0, 1))) < LINEAR_BOUND and _rel_err(sums[1].cpu(), (g * x[:, :C].float().view(B, T, C)).sum((0, 1))) < LINEAR_BOUND
    out2 = torch.full((B * T + 1, C + 64), SENT, dtype=BF).to(DEV)
    _, sums2 = ops.tcn_norm_pool_bwd(dh.to(DEV), dp.to(DEV), x.to(DEV), scale.to(DEV), mask.to(DEV), B=B, T=T, C=C, out=out2)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(sums2, sums)                         # same bits twice
    # the saving forward: the same output bits as svsr_tconv_fwd, and z = scale * acc + shift reproduces them
    n_in, co, k, d = 192, 64, 5, 2
    w = (_r(co, k, n_in, seed=5) / (n_in * k) ** 0.5).to(BF).to(DEV)
    sc, sh = (1 + 0.1 * _r(co, seed=6)).to(DEV), (0.1 * _r(co, seed=7)).to(DEV)
    xs = x[:, :n_in].contiguous().to(DEV)
    br = [dict(k=k, w=w, scale=sc, shift=sh, out_off=0)]
    o1 = ops.tconv_fwd(xs, B=B, T=T, n_in=n_in, d=d, branches=br, co=co, act=2, out=torch.empty(B * T, co, dtype=BF, device=DEV))
    accb = torch.full((B * T + 1, co + 8), SENT, device=DEV)
    o2 = ops.tconv_fwd(xs, B=B, T=T, n_in=n_in, d=d, branches=br, co=co, act=2, out=torch.empty(B * T, co, dtype=BF, device=DEV), acc=accb)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    z = accb[: B * T, :co] * sc + sh
    assert _rel_err((z * torch.sigmoid(z)).cpu(), o1.float().cpu()) < LINEAR_BOUND
    assert bool((accb[:, co:] == SENT).all()) and bool((accb[B * T:] == SENT).all())


def test_out_of_domain_arguments_return_err_arg_and_write_nothing():
    from syncvsr_amd import _lib

    lib = _lib.load()
    B, T, n_in, co = 2, 9, 128, 64
    x = torch.zeros(B * T, n_in, dtype=BF, device=DEV)
    dy = torch.zeros(B * T, co, dtype=BF, device=DEV)
    out = torch.full((B * T, n_in), SENT, dtype=BF, device=DEV)
    wt = torch.zeros(n_in, 7, co, dtype=BF, device=DEV)
    f = torch.full((co * n_in * 7 * 4,), SENT, device=DEV)
    tabs = {k: torch.tensor([[k, wt.data_ptr(), 0, 0]], dtype=torch.int64) for k in (3, 4, 7, 9)}          # host tables, alive during the calls
    tab = tabs.__getitem__
    dg = lambda k, d, c, n, t=T: lib.svsr_tconv_dgrad(dy.data_ptr(), co, B, t, c, d, 1, tab(k).data_ptr(), n, None, 0, None, 0, None, 1.0,  # noqa: E731
                                                     out.data_ptr(), n_in, None, None)
    assert dg(3, 1, co, n_in) == 0
    out.fill_(SENT)
    for bad in (dg(9, 1, co, n_in), dg(4, 1, co, n_in), dg(7, 6, co, n_in), dg(3, 0, co, n_in), dg(3, 1, 32, n_in), dg(3, 1, co, 96), dg(3, 1, co, n_in, 0)):
        assert bad == 1001
    wg = lambda k, d, n, c, s=1, t=T: lib.svsr_tconv_wgrad(x.data_ptr(), n_in, None, dy.data_ptr(), co, B, t, n, c, k, d, s, f.data_ptr(),  # noqa: E731
                                                          f.data_ptr() + 4 * co * n_in * 7 * 2, n, 0, None)
    for bad in (wg(9, 1, n_in, co), wg(2, 1, n_in, co), wg(7, 6, n_in, co), wg(3, 1, 96, co), wg(3, 1, n_in, 32), wg(3, 1, n_in, co, 0), wg(3, 1, n_in, co, 99),
                wg(3, 1, n_in, co, 1, 0)):
        assert bad == 1001
    assert lib.svsr_tconv_epi_bwd(dy.data_ptr(), co, f.data_ptr(), co, B * T, 96, 2, f.data_ptr(), f.data_ptr(), None, None, 0, 0, out.data_ptr(), n_in,
                                  None, 0, f.data_ptr(), f.data_ptr(), None) == 1001
    assert lib.svsr_tconv_epi_bwd(dy.data_ptr(), co, f.data_ptr(), co, B * T, co, 3, f.data_ptr(), f.data_ptr(), None, None, 0, 0, out.data_ptr(), n_in,
                                  None, 0, f.data_ptr(), f.data_ptr(), None) == 1001           # PReLU without slopes
    assert lib.svsr_tcn_norm_pool_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), n_in, B, T, 100, f.data_ptr(), f.data_ptr(), out.data_ptr(), n_in,
                                      f.data_ptr(), f.data_ptr(), None) == 1001
    assert lib.svsr_tcn_se_bwd(x.data_ptr(), n_in, B, T, 96, 8, 3, x.data_ptr(), x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(),
                               tab(3).data_ptr(), 0, None) == 1001
    one = torch.ones(co, device=DEV)
    ftab = torch.tensor([[3, wt.data_ptr(), 0, one.data_ptr(), one.data_ptr(), 0, 0, 0]], dtype=torch.int64)
    sv = lambda acc, pitch: lib.svsr_tconv_fwd_save(x.data_ptr(), n_in, B, T, n_in, 1, 1, ftab.data_ptr(), co, 2, out.data_ptr(), n_in, None, 0, 0,  # noqa: E731
                                                    acc, pitch, None)
    assert sv(None, co) == 1001 and sv(f.data_ptr(), co - 1) == 1001         # no accumulator buffer; acc_pitch < nb * co
    assert lib.svsr_tcn_fold(None, 1, 8, f.data_ptr(), 0, None) == 1001 and lib.svsr_tcn_fold(f.data_ptr(), 0, 8, f.data_ptr(), 0, None) == 1001
    assert lib.svsr_tcn_fold(f.data_ptr(), 1, 0, f.data_ptr(), 0, None) == 1001
    torch.cuda.synchronize()
    assert bool((out.float() == SENT).all()) and bool((f == SENT).all())


def _table_passing_sequence(ops, t, B, T, n_in, co):
    """svsr_tconv_fwd_save -> svsr_tconv_dgrad (gated) -> svsr_tcn_se_bwd on the tensors of t, each launch with a host table.
    -> (gate partials, dm): what the wrappers allocate themselves."""
    ops.tconv_fwd(t["x"], B=B, T=T, n_in=n_in, d=2, co=co, act=2, out=t["y"], acc=t["acc"],
                  branches=[dict(k=3, w=t["w"], gate=t["gate"][0], scale=t["scale"], shift=t["shift"], out_off=0)])
    gp = ops.tconv_dgrad(t["dy"], B=B, T=T, co=co, d=2, n_out=n_in, out=t["dx"], x=t["x"], branches=[dict(k=3, wt=t["wt"], dy_off=0, gate=t["gate"][0])])
    dm = ops.tcn_se_bwd(t["x"], t["w1"], t["w2"], t["gate"], gp, [t["dw1"]], [t["dw2"]], B=B, T=T, n_in=n_in)
    return gp, dm


def test_recorded_replay_owns_its_host_tables():
    """A step list records the three table-passing launches; every Python reference to what the wrappers made is dropped, host memory is
    churned and the inputs are refilled in place: the replay equals an eager run on the new inputs bit for bit (the recorder keeps the tables)."""
    import gc

    from syncvsr_amd import ops

    B, T, n_in, co, Rr = 2, 5, 128, 64, 8
    inputs = dict(x=(B * T, n_in), dy=(B * T, co), w=(co, 3, n_in), wt=(n_in, 3, co), w1=(1, Rr, n_in), w2=(1, n_in, Rr))

    def fill(t, seed):
        for i, (n, shape) in enumerate(inputs.items()):
            t[n].copy_((_r(*shape, seed=seed + i) * (0.1 if n[0] == "w" else 1.0)).to(BF))
        t["gate"].copy_(torch.sigmoid(_r(1, B, n_in, seed=seed + 10)))
        t["scale"].copy_(1 + 0.1 * _r(co, seed=seed + 11))
        t["shift"].copy_(0.1 * _r(co, seed=seed + 12))

    def tensors():
        t = {n: torch.empty(shape, dtype=BF, device=DEV) for n, shape in inputs.items()}
        t.update(gate=torch.empty(1, B, n_in, device=DEV), scale=torch.empty(co, device=DEV), shift=torch.empty(co, device=DEV))
        t.update(y=torch.full((B * T, co), SENT, dtype=BF, device=DEV), acc=torch.full((B * T, co), SENT, device=DEV),
                 dx=torch.full((B * T, n_in), SENT, dtype=BF, device=DEV), dw1=torch.full((Rr, n_in), SENT, device=DEV),
                 dw2=torch.full((n_in, Rr), SENT, device=DEV))
        return t

    outs = ("y", "acc", "dx", "dw1", "dw2")
    t = tensors()
    fill(t, 1000)
    rec = ops.StepRecorder()
    with ops.recording(rec):
        gp, dm = _table_passing_sequence(ops, t, B, T, n_in, co)
    torch.cuda.synchronize()
    first = [t[n].clone() for n in outs]
    gc.collect()
    churn = [torch.zeros(n, dtype=torch.int64) for n in (2, 4, 8, 16, 2, 4, 8, 16)]          # zeros: a table read from re-used memory is refused, not followed
    del churn
    fill(t, 2000)
    rec.run()
    torch.cuda.synchronize()
    e = tensors()
    fill(e, 2000)
    egp, edm = _table_passing_sequence(ops, e, B, T, n_in, co)
    torch.cuda.synchronize()
    for n, before in zip(outs, first):
        view = torch.int16 if t[n].dtype == BF else torch.int32
        assert torch.equal(t[n].view(view), e[n].view(view)), f"{n}: the replay differs from an eager run on the same inputs"
        assert not torch.equal(t[n].view(view), before.view(view)), f"{n}: the replay did not see the refilled inputs"
    assert torch.equal(gp.view(torch.int32), egp.view(torch.int32)) and torch.equal(dm.view(torch.int32), edm.view(torch.int32))
    assert sum(1 for k in rec.keep if torch.is_tensor(k) and k.dtype == torch.int64 and not k.is_cuda) == 3
