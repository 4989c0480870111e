"""The merged downsample-block data gradient on the GPU (-m gpu): svsr_igemm_dgrad2 / svsr_igemm_dgrad2_bn against the float64 restatement and
against the two-launch form (1x1 data gradient, then the 3x3 one adding to it).  Cases and method: tests/dgrad2_cases.py,
tests/contraction_restatement.py.  Exact operands: the merged launch, the two launches and the restatement must agree bit for bit (the 1x1
gradient is itself a bf16 number, so the two-launch form's intermediate rounding loses nothing).  N(0,1) operands: the merged sum is rounded
once, the two-launch form twice — its error against float64 may not be smaller."""
import pytest
import torch

import contraction_cases as cc
import contraction_restatement as R
import dgrad2_cases as dc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _stats_begin():
    from syncvsr_amd import ops

    buf = ops.scratch(1)
    buf[: 1 << 20].view(torch.int32).fill_(R.SENT32)
    return buf


def _stats_rows(buf, rows: int, C: int, what: str):
    n = rows * 2 * C
    R.assert_untouched(buf[n: n + R.STAT_SPARE], f"{what}: statistics rows behind row {rows - 1}")
    part = buf[:n].cpu()
    assert not bool(R.sentinel_mask(part).any()), f"{what}: a statistics row below {rows} was not written"
    return part.view(rows, 2, C)


def _bn(c, t):
    """(y, x, mean, rstd, gamma, beta, act) of the epilogue"""
    return (t["y"], t["x"], t["mean"], t["rstd"], t["gamma"], t["beta"], 2 if c.epi == "swish" else 1)


def _merged(c, t, dev):
    """one merged launch into a sentinel-guarded buffer -> {out | g, sums rows}"""
    from syncvsr_amd import ops
    from syncvsr_amd.ops import _p

    N, H, W, Kp, Ci = c.N, c.H, c.W, c.kp, c.ci_in
    Ho, Wo = c.hw_out
    plan = ops.conv_plan(3, N, H, W, Ci, 3, 2, 1)
    assert cc._glds_label(plan.meta, Kp, Ci, c.epi != "plain") == dc.expected_label(c)
    rows = N * H * W
    buf, view = R.guarded(rows, Ci, Ci, BF, dev)
    head = (_p(t["dy"]), _p(t["wt"]), _p(t["dy2"]), _p(t["wt2"]), _p(buf))
    out = {}
    if c.epi == "plain":
        ops._call("svsr_igemm_dgrad2", *head, None, None, None, plan.words.data_ptr(), plan.meta, N, Ho * Wo, Kp, Kp, Ci, H * W, Ci, 9, 0, 0, 1.0,
                  None, 0, 0.0, ops._stream())
        torch.cuda.synchronize()
    else:
        sbuf = _stats_begin()
        y, x, mean, rstd, gamma, beta, act = _bn(c, t)
        ops._call("svsr_igemm_dgrad2_bn", *head, _p(sbuf), plan.words.data_ptr(), plan.meta, N, Ho * Wo, Kp, Kp, Ci, H * W, Ci, 9, _p(y), _p(x),
                  _p(mean), _p(rstd), _p(gamma), _p(beta), act, ops._stream())
        torch.cuda.synchronize()
        out["rows"] = _stats_rows(sbuf, plan.tiles, Ci, c.name)
    R.assert_guard(buf, rows, Ci, c.name)
    out["out" if c.epi == "plain" else "g"] = view.cpu().reshape(N, H, W, Ci)
    return out


def _two_launches(c, t):
    """the form the merged launch replaces, through the wrappers model.py used"""
    from syncvsr_amd import ops

    hw = (c.H, c.W)
    dxd = ops.conv2d_dgrad(t["dy2"], t["wt2"].view(c.ci_in, 1, 1, c.kp), 1, 2, 0, hw)
    if c.epi == "plain":
        out = ops.conv2d_dgrad(t["dy"], t["wt"], 3, 2, 1, hw, addend=dxd)
        torch.cuda.synchronize()
        return {"out": out.cpu()}
    y, x, mean, rstd, gamma, beta, act = _bn(c, t)
    g, (stats, rows) = ops.conv2d_dgrad_bn(t["dy"], t["wt"], 3, 2, 1, hw, dxd, y, x, mean, rstd, gamma, beta, act)
    torch.cuda.synchronize()
    return {"g": g.cpu(), "rows": stats[: rows * 2 * c.ci_in].cpu().view(rows, 2, c.ci_in)}


def _through_ops(c, t):
    """the wrapper model.py calls"""
    from syncvsr_amd import ops

    r = ops.conv2d_dgrad2(t["dy"], t["wt"], t["dy2"], t["wt2"], (c.H, c.W), bn=None if c.epi == "plain" else _bn(c, t))
    torch.cuda.synchronize()
    return r.cpu() if c.epi == "plain" else r[0].cpu()


@pytest.mark.parametrize("case", [c for c in dc.CASES if not c.floats], ids=lambda c: c.name)
def test_merged_launch_is_bit_exact(dev, case):
    c = case
    d = dc.build(c)
    assert max(R.budget_of(d["abs"]).values()) < R.LIMIT
    assert torch.equal(R.rne_bf16(d["dxd"]), d["dxd"])
    t = {k: v.to(dev) for k, v in d["in"].items()}
    ref, Ci = d["ref"], c.ci_in
    kind = "out" if c.epi == "plain" else "g"
    with cc.knobs(c.knobs):
        got = _merged(c, t, dev)
        again = _merged(c, t, dev)
        two = _two_launches(c, t)
        wrapped = _through_ops(c, t)
    what = f"{c.name} [{dc.expected_label(c)}]"
    xh = None if c.epi == "plain" else ((d["in"]["x"].double() - d["in"]["mean"].double()) * d["in"]["rstd"].double()).reshape(-1, Ci)
    if c.epi == "plain":
        R.assert_bits(got["out"], ref["out"], what + " out")
    elif c.epi == "relu":
        R.assert_bits(got["g"], ref["g"], what + " g")
        R.assert_bits(got["rows"].double().sum(0).float(), ref["sums"], what + " column sums of the partial rows")
    else:
        R.assert_close_rows(got["g"], ref["g_swish"], R.swish_slack(ref["gb"], ref["z"]), what + " g")
        g64 = got["g"].double().reshape(-1, Ci)
        sums = got["rows"].double().sum(0)
        R.assert_sum_rows(sums[0], g64, what + " sum g")
        R.assert_sum_rows(sums[1], g64 * xh, what + " sum g*xhat")
    # the two-launch form: the same bits, in the gradient and (ReLU: exact integers) in the sums; the wrapper: the merged launch's bits
    R.assert_bits(got[kind], two[kind], what + " against the two-launch form")
    if c.epi == "relu":
        R.assert_bits(got["rows"].double().sum(0).float(), two["rows"].double().sum(0).float(), what + " sums against the two-launch form")
    R.assert_bits(wrapped, got[kind], what + " through ops.conv2d_dgrad2")
    for k, v in got.items():
        assert torch.equal(v.contiguous().view(torch.uint8), again[k].contiguous().view(torch.uint8)), f"{c.name}: {k} differs between two launches"


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.floats], ids=lambda c: c.name)
def test_merged_launch_is_no_further_from_float64_than_two_launches(dev, case):
    c = case
    d = dc.build(c)
    t = {k: v.to(dev) for k, v in d["in"].items()}
    kind = "out" if c.epi == "plain" else "g"
    ref = d["ref"]["out"] if c.epi == "plain" else d["ref"]["g_float"]
    got, two = _merged(c, t, dev), _two_launches(c, t)
    again = _merged(c, t, dev)
    assert torch.equal(got[kind].view(torch.int16), again[kind].view(torch.int16))
    e1, e2 = (got[kind].double() - ref).abs(), (two[kind].double() - ref).abs()
    ee = torch.zeros(c.H, c.W, dtype=torch.bool)
    ee[0::2, 0::2] = True
    print(f"{c.name}: merged sum|err| {float(e1.sum()):.6f} max {float(e1.max()):.6f}; two launches sum|err| {float(e2.sum()):.6f} max {float(e2.max()):.6f}; "
          f"on the (even, even) pixels {float(e1[:, ee].sum()):.6f} against {float(e2[:, ee].sum()):.6f}")
    # pixels the 1x1 branch does not reach: the same contraction, the same bits
    assert torch.equal(got[kind][:, ~ee].view(torch.int16), two[kind][:, ~ee].view(torch.int16))
    assert float(e1.sum()) <= float(e2.sum()) and float(e1[:, ee].sum()) <= float(e2[:, ee].sum())
    if c.epi != "swish":
        # plain / ReLU: a merged element is the bf16 number NEAREST to its fp32 sum, so it can be further from float64 than the two-launch element
        # only by that sum's own error — at most (terms) * 2^-24 * sum|products| with 10 * planes terms.  (Swish rounds a product afterwards:
        # there only the totals above are compared.)
        slack = 10 * c.planes * 2.0 ** -24 * float(d["abs"][kind].max())
        assert bool((e1 <= e2 + slack).all()) and float(e1.max()) <= float(e2.max()) + slack
