"""GPU parity of the DC-TCN back-end kernels (csrc/dctcn.hip) against plain torch in fp32 on bf16-rounded operands."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LINEAR_BOUND = 5e-3       # the bound tests/test_gpu_lrs_kernels.py applies to svsr_linear_fwd (bf16 in, fp32 accumulate, bf16 out) at K = 768


def _dev():
    return torch.device("cuda:0")


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _rel_err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _act(v, act, slope=None):
    if act == 2:
        return v * torch.sigmoid(v)
    if act == 3:
        return torch.where(v >= 0, v, v * slope)
    if act == 1:
        return torch.relu(v)
    return v


def _tconv_case(B, T, n_in, d, ks, co, gated, residual, act, pitch_extra, out_off, seed):
    from syncvsr_amd import ops

    dev = _dev()
    pitch = n_in + pitch_extra
    x = _r(B * T, pitch, seed=seed).to(BF)
    width = out_off + len(ks) * co + 8
    out = torch.full((B * T, width), 7.0, dtype=BF)
    res = _r(B * T, len(ks) * co + 16, seed=seed + 1).to(BF) if residual else None
    branches, ref = [], torch.full((B * T, width), 7.0)
    for i, k in enumerate(ks):
        w = (_r(co, n_in, k, seed=seed + 10 + i) / (n_in * k) ** 0.5).to(BF)              # torch layout [co, ci, k]
        gate = torch.sigmoid(_r(B, n_in, seed=seed + 20 + i)) if gated else None
        scale, shift = 1 + 0.1 * _r(co, seed=seed + 30 + i), 0.1 * _r(co, seed=seed + 40 + i)
        slope = 0.25 + 0.05 * _r(co, seed=seed + 50 + i)
        xin = x[:, :n_in].float().view(B, T, n_in)
        if gated:
            xin = (xin * gate.unsqueeze(1)).to(BF).float()                                # the MFMA operand is bf16(x * gate)
        y = F.conv1d(xin.transpose(1, 2), w.float(), None, padding=(k - 1) * d // 2, dilation=d).transpose(1, 2).reshape(B * T, co)
        y = _act(y * scale + shift, act, slope)
        if residual:
            y = y + res[:, 8 + i * co: 8 + (i + 1) * co].float()
            y = y * torch.sigmoid(y)
        ref[:, out_off + i * co: out_off + (i + 1) * co] = y
        br = dict(k=k, w=w.permute(0, 2, 1).contiguous().to(dev), scale=scale.to(dev), shift=shift.to(dev), out_off=out_off + i * co, res_off=8 + i * co)
        if gated:
            br["gate"] = gate.to(dev).contiguous()
        if act == 3:
            br["slope"] = slope.to(dev)
        branches.append(br)
    got = ops.tconv_fwd(x.to(dev), B=B, T=T, n_in=n_in, d=d, branches=branches, co=co, act=act, out=out.to(dev),
                        res=None if res is None else res.to(dev), res_act=2 if residual else 0)
    torch.cuda.synchronize()
    got = got.float().cpu()
    lo, hi = out_off, out_off + len(ks) * co
    err = _rel_err(got[:, lo:hi], ref[:, lo:hi])
    print(f"tconv B={B} T={T} n_in={n_in} d={d} ks={ks} gated={gated} res={residual} act={act}: rel err {err:.3e} (bound {LINEAR_BOUND})")
    assert err < LINEAR_BOUND
    assert bool((got[:, :lo] == 7.0).all()) and bool((got[:, hi:] == 7.0).all()), "sentinels beside the written channels were overwritten"


@pytest.mark.parametrize("T", [1, 5, 29, 40])
@pytest.mark.parametrize("n_in", [64, 384, 512, 896, 1280])
def test_tconv_three_branches_gated_every_length_and_width(T, n_in):
    d = {1: 1, 5: 2, 29: 5, 40: 5}[T]
    _tconv_case(3, T, n_in, d, (3, 5, 7), 128, True, False, 2, 64, 64, seed=T * 7 + n_in)


@pytest.mark.parametrize("d", [1, 2, 5])
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("gated,residual", [(False, False), (True, True), (False, True), (True, False)])
def test_tconv_every_kernel_size_dilation_gate_and_residual(d, k, gated, residual):
    _tconv_case(2, 29, 384, d, (k,), 64, gated, residual, 2, 0, 0, seed=100 + 10 * d + k)
    _tconv_case(5, 40, 512, d, (k,), 128, gated, residual, 2, 128, 192, seed=200 + 10 * d + k)


def test_tconv_pointwise_prelu_and_plain_bias_modes():
    """k = 1, ungated: transition0 (576-wide padded input, PReLU), a transition (Swish) and downsample (no activation)."""
    _tconv_case(3, 29, 576, 1, (1,), 512, False, False, 3, 0, 0, seed=301)
    _tconv_case(3, 7, 1664, 1, (1,), 512, False, False, 2, 0, 0, seed=302)
    _tconv_case(3, 29, 896, 1, (1,), 384, False, False, 0, 768, 0, seed=303)
    _tconv_case(2, 33, 128, 1, (1,), 64, False, False, 1, 0, 64, seed=304)


def test_tconv_in_place_on_the_feature_stack_is_bit_identical_run_to_run():
    """A layer's second stage writes behind the channels the next layer reads: out aliases x.  Two runs give the same bits."""
    from syncvsr_amd import ops

    dev = _dev()
    B, T, n_in, co = 4, 29, 512, 128
    outs = []
    for _ in range(2):
        stack = torch.zeros(B * T, n_in + 3 * co, dtype=BF)
        stack[:, :n_in] = _r(B * T, n_in, seed=5).to(BF)
        stack = stack.to(dev)
        brs = [dict(k=k, w=(_r(co, k, n_in, seed=6 + i) / (n_in * k) ** 0.5).to(BF).to(dev), scale=torch.ones(co, device=dev),
                    shift=torch.zeros(co, device=dev), out_off=n_in + i * co) for i, k in enumerate((3, 5, 7))]
        ops.tconv_fwd(stack, B=B, T=T, n_in=n_in, d=2, branches=brs, co=co, act=2, out=stack)
        torch.cuda.synchronize()
        outs.append(stack.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert torch.equal(outs[0][:, :n_in].view(torch.int16), _r(B * T, n_in, seed=5).to(BF).view(torch.int16))
    assert float(outs[0][:, n_in:].float().abs().sum()) > 0


@pytest.mark.parametrize("B,T,n_in", [(1, 1, 64), (3, 29, 512), (5, 7, 896), (2, 40, 1280)])
def test_se_gates_against_torch(B, T, n_in):
    from syncvsr_amd import ops

    dev = _dev()
    R, pitch = n_in // 16, n_in + 64
    x = _r(B * T, pitch, seed=1).to(BF)
    w1 = (_r(3, R, n_in, seed=2) / n_in ** 0.5).to(BF)
    w2 = (_r(3, n_in, R, seed=3) / R ** 0.5).to(BF)
    gate = ops.tcn_se_fwd(x.to(dev), w1.to(dev), w2.to(dev), B=B, T=T, n_in=n_in)
    torch.cuda.synchronize()
    m = x[:, :n_in].float().view(B, T, n_in).mean(1)
    for i in range(3):
        hid = m @ w1[i].float().T
        ref = torch.sigmoid((hid * torch.sigmoid(hid)) @ w2[i].float().T)
        err = _rel_err(gate[i].cpu(), ref)
        print(f"se B={B} T={T} n_in={n_in} branch {i}: rel err {err:.3e}")
        assert err < 1e-4            # fp32 throughout (v_exp / v_rcp sigmoid: ~1e-6 relative); nothing is stored in bf16


def test_norm_pool_tail_with_an_all_zero_mask():
    from syncvsr_amd import ops

    dev = _dev()
    B, T, C = 4, 29, 1664
    x = _r(B * T, C + 64, seed=1).to(BF)
    scale, shift = 1 + 0.1 * _r(C, seed=2), 0.1 * _r(C, seed=3)
    mask = torch.ones(B, T)
    mask[1, 11:] = 0
    mask[2] = 0                    # a clip without a single valid frame: 0 / 1e-6 = 0, finite
    mask[3, :5] = 0
    h, pooled = ops.tcn_norm_pool_fwd(x.to(dev), scale.to(dev), shift.to(dev), mask.to(dev), B=B, T=T, C=C)
    torch.cuda.synchronize()
    href = (x[:, :C].float() * scale + shift)
    assert _rel_err(h.float().cpu(), href) < 4e-3                      # one bf16 rounding
    hb = h.float().cpu().view(B, T, C)
    pref = (hb * mask.unsqueeze(2)).sum(1) / (mask.sum(1, keepdim=True) + 1e-6)
    assert bool(torch.isfinite(pooled.float()).all())
    assert _rel_err(pooled.float().cpu(), pref) < 4e-3
    assert float(pooled[2].float().abs().max()) == 0.0


def test_rejected_arguments_raise():
    from syncvsr_amd import ops
    from syncvsr_amd._lib import SvsrError

    dev = _dev()
    B, T, n_in, co = 2, 9, 128, 64
    x = torch.zeros(B * T, n_in, dtype=BF, device=dev)
    out = torch.zeros(B * T, co, dtype=BF, device=dev)
    one, zero = torch.ones(co, device=dev), torch.zeros(co, device=dev)

    def br(k, n=n_in, **kw):
        return dict(dict(k=k, w=torch.zeros(co, k, n, dtype=BF, device=dev), scale=one, shift=zero, out_off=0), **kw)

    ops.tconv_fwd(x, B=B, T=T, n_in=n_in, d=1, branches=[br(3)], co=co, act=2, out=out)                      # the accepted baseline
    with pytest.raises(SvsrError):
        ops.tconv_fwd(x, B=B, T=T, n_in=n_in, d=6, branches=[br(7)], co=co, act=2, out=out)                  # (k - 1) * d / 2 = 18 > 16
    with pytest.raises(SvsrError):
        ops.tconv_fwd(x, B=B, T=T, n_in=n_in, d=1, branches=[br(9)], co=co, act=2, out=out)                  # k > 7
    with pytest.raises(SvsrError):
        ops.tconv_fwd(x, B=B, T=T, n_in=n_in, d=0, branches=[br(3)], co=co, act=2, out=out)                  # d < 1
    with pytest.raises(SvsrError):
        ops.tconv_fwd(x, B=B, T=T, n_in=n_in, d=1, branches=[br(3)], co=co, act=3, out=out)                  # PReLU without slopes
    with pytest.raises(SvsrError):
        ops.tconv_fwd(x, B=B, T=T, n_in=n_in, d=1, branches=[br(3)], co=co, act=5, out=out)                  # unknown activation
    lib = __import__("syncvsr_amd._lib", fromlist=["load"]).load()
    tab = torch.tensor([[3, br(3)["w"].data_ptr(), 0, one.data_ptr(), zero.data_ptr(), 0, 0, 0]], dtype=torch.int64)
    args = lambda n, c, t: (x.data_ptr(), n_in, B, t, n, 1, 1, tab.data_ptr(), c, 2, out.data_ptr(), co, None, 0, 0, None)      # noqa: E731
    assert lib.svsr_tconv_fwd(*args(96, co, T)) == 1001            # n_in not a multiple of 64
    assert lib.svsr_tconv_fwd(*args(n_in, 32, T)) == 1001          # co not a multiple of 64
    assert lib.svsr_tconv_fwd(*args(n_in, co, 0)) == 1001          # T < 1
    g = torch.zeros(3, B, n_in, device=dev)
    assert lib.svsr_tcn_se_fwd(x.data_ptr(), n_in, B, T, 96, 6, 3, x.data_ptr(), x.data_ptr(), g.data_ptr(), None) == 1001
    assert lib.svsr_tcn_se_fwd(x.data_ptr(), n_in, B, T, n_in, 6, 3, x.data_ptr(), x.data_ptr(), g.data_ptr(), None) == 1001     # R % 4
    assert lib.svsr_tcn_norm_pool_fwd(x.data_ptr(), n_in, B, T, 100, one.data_ptr(), zero.data_ptr(), g.data_ptr(), out.data_ptr(), out.data_ptr(), None) == 1001
    torch.cuda.synchronize()
