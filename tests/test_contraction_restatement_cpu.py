"""The three conditions the exact contraction suite (tests/test_gpu_contraction_edges.py) rests on, proved without a GPU: the float64
restatements equal independent torch autograd computations on every case, every case is inside the 2^24 budget for every output kind, and the
case table reaches every instantiation and plan format listed in tests/contraction_cases.py; plus: assert_bits reports the errors it is for."""
import pytest
import torch
import torch.nn.functional as F

import contraction_cases as cc
import contraction_restatement as R

F64 = torch.float64


@pytest.fixture(scope="module")
def built():
    return {c.name: cc.build(c) for c in cc.CASES}


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _conv_geo(c, q=None):
    q = dict(q or c.shape)
    if c.op in ("c64", "wgrad3", "chain"):
        q = dict(dict(Ci=64, Co=64), **q, k=3, s=1, p=1)
    return q


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_restatement_equals_autograd(built, case):
    """independent route: forward by unfold + matmul, every gradient by autograd of F.conv2d / matmul in float64"""
    d, o = built[case.name], case.opts
    I, ref = d["in"], d["ref"]
    if case.op == "group":
        for i, q in enumerate(case.shape["problems"]):
            x = I[f"x{i}"].double()
            if q.get("seq"):
                x = x.view(-1, q["seq"][0], q["K"])[:, q["seq"][1]: q["seq"][1] + q["seq"][2]].reshape(-1, q["K"])
            w = torch.zeros(q["N"], q["K"], dtype=F64, requires_grad=True)
            b = torch.zeros(q["N"], dtype=F64, requires_grad=True)
            (x @ w.t() + b).backward(I[f"dy{i}"].double())
            assert torch.equal(ref[f"dw{i}"], w.grad + (I[f"dw0{i}"].double() if f"dw0{i}" in I else 0))
            if q.get("db"):
                assert torch.equal(ref[f"db{i}"], b.grad + (I[f"db0{i}"].double() if f"db0{i}" in I else 0))
        return
    if "R" in case.shape:
        s = case.shape
        K, N, seq = s["K"], s["N"], s.get("seq")
        pick = (lambda t: t) if seq is None else (lambda t: t.view(-1, seq[0], t.shape[-1])[:, seq[1]: seq[1] + seq[2]].reshape(-1, t.shape[-1]))
        if case.op == "linear":
            acc = (pick(I["x"].double())[:, None, :] * I["w"].double()[None]).sum(-1)
            v = acc + (I["bias"].double() if "bias" in I else 0)
            assert torch.equal(ref["pre"], v)
            if o.get("act") == "gelu":
                assert torch.allclose(ref["out"], F.gelu(v), rtol=0, atol=1e-12)
            else:
                v = v.clamp_min(0) if o.get("act") == "relu" else v
                assert torch.equal(ref["out"], v * o.get("alpha", 1.0) + (I["addend"].double() if "addend" in I else 0))
            return
        if case.op == "lin_wgrad":
            w = torch.zeros(N, K, dtype=F64, requires_grad=True)
            b = torch.zeros(N, dtype=F64, requires_grad=True)
            (pick(I["x"].double()) @ w.t() + b).backward(I["dy"].double())
            assert torch.equal(ref["dw"], w.grad + (I["dw0"].double() if "dw0" in I else 0))
            if "db" in ref:
                assert torch.equal(ref["db"], b.grad + (I["db0"].double() if "db0" in I else 0))
            return
        # data gradients of out = x W^T: autograd with respect to x
        w = I["wt"][:, :N].double().t()
        x = torch.zeros(s["R"], K, dtype=F64, requires_grad=True)
        (x @ w.t()).backward(I["dy"][:, :N].double())
        dd = x.grad
        if case.op == "lin_dgrad":
            dd = dd * o.get("alpha", 1.0)
            if "addend" in I:
                dd = dd + pick(I["addend"].double())
            assert torch.equal(ref["out"], dd)
            return
        _check_bn(case, d, dd, K)
        return
    links = case.shape["links"] if case.op == "chain" else [case.shape]
    for li, q in enumerate(links):
        q = _conv_geo(case, q)
        k, st, p = q["k"], q["s"], q["p"]
        sfx = str(li) if case.op == "chain" else ""
        if "out" in ref and "x" in I and "w" in I:          # forward: unfold + matmul
            cols = F.unfold(_nchw(I["x"]), k, padding=p, stride=st)                         # [N, Ci*k*k, L]
            wm = I["w"].double().permute(0, 3, 1, 2).reshape(q["Co"], -1)
            acc = (wm @ cols).permute(0, 2, 1).reshape(ref["out"].shape)
            assert torch.equal(ref["out"], acc)
            a2 = acc.reshape(-1, q["Co"])
            assert torch.equal(ref["stats"], torch.stack([a2.sum(0), (a2 * a2).sum(0)]))
        elif "wt" in I:
            w = I["wt"].double().permute(3, 0, 1, 2)                                        # [Co][Ci][k][k]
            x = torch.zeros(q["N"], q["Ci"], q["H"], q["W"], dtype=F64, requires_grad=True)
            F.conv2d(x, w, stride=st, padding=p).backward(_nchw(I["dy"]))
            dd = x.grad.permute(0, 2, 3, 1)
            reach = d["reach"]
            probe = torch.zeros(1, 1, q["H"], q["W"], dtype=F64, requires_grad=True)
            F.conv2d(probe, torch.ones(1, 1, k, k, dtype=F64), stride=st, padding=p).sum().backward()
            assert torch.equal(reach, probe.grad[0, 0] > 0)
            assert bool((dd[:, ~reach] == 0).all())
            if "addend" in I:
                dd = dd + I["addend"].double()
            if "out" in ref:
                assert torch.equal(ref["out"], dd)
            else:
                _check_bn(case, d, dd, q["Ci"])
        else:
            w = torch.zeros(q["Co"], q["Ci"], k, k, dtype=F64, requires_grad=True)
            F.conv2d(_nchw(I["x" + sfx]), w, stride=st, padding=p).backward(_nchw(I["dy" + sfx]))
            want = w.grad.permute(0, 2, 3, 1) + (I["dw0" + sfx].double() if "dw0" + sfx in I else 0)
            assert torch.equal(ref["dw" + sfx], want)


def _check_bn(case, d, dd, C):
    """BatchNorm-backward epilogues: the mask / activation derivative by autograd of relu / silu on bn(x) [+ r], g rounded to bf16 before the sums"""
    I, ref, o = d["in"], d["ref"], case.opts
    gb = dd.float().to(torch.bfloat16).double()
    if case.op == "lin_dgrad_relu":
        g = torch.where(I["y"].double() > 0, (gb * o["gscale"]).float().to(torch.bfloat16).double(), torch.zeros_like(gb))
        assert torch.equal(ref["g"], g) and torch.equal(ref["sums"][0], g.sum(0))
        return
    x = I["x"].double()
    z = ((x - I["mean"].double()) * I["rstd"].double() * I["gamma"].double() + I["beta"].double()).requires_grad_(True)
    if "g_swish" in ref:
        zz = z + (I["y"].double() if "y" in I else 0)
        F.silu(zz).sum().backward()
        assert torch.allclose(ref["g_swish"], gb * z.grad, rtol=1e-13, atol=1e-13) and torch.equal(ref["z"], zz.detach()) and torch.equal(ref["gb"], gb)
        return
    if "y" in I:
        mask = I["y"].double() > 0
    else:
        torch.relu(z).sum().backward()
        mask = z.grad > 0
    g = torch.where(mask, gb, torch.zeros_like(gb))
    xh = (x - I["mean"].double()) * I["rstd"].double()
    assert torch.equal(ref["g"], g)
    assert torch.equal(ref["sums"], torch.stack([g.reshape(-1, C).sum(0), (g * xh).reshape(-1, C).sum(0)]))


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_every_output_kind_is_inside_the_exact_budget(built, case):
    b = R.exact_budget(case)
    assert b == R.budget_of(built[case.name]["abs"])
    assert b and all(v < R.LIMIT / 4 for v in b.values()), b          # (a condition with room to spare, not a measurement: 2^22)
    for k, v in built[case.name]["in"].items():
        if v.dtype == torch.bfloat16:
            assert torch.equal(v.float(), v.float().round()) and float(v.float().abs().max()) <= 4, k


def test_census_every_listed_instantiation_is_reached():
    from syncvsr_amd import ops

    names = ("igemm_tile", "igemm_m128", "wg_blocks", "w3_blocks", "igemm_bn64_below", "wg_short_k", "igemm_ksplit", "igemm_lin_bn64", "p8", "p8_grid",
             "p8_min_items", "p8_stagger", "wg_imgmajor", "wg_units", "wg_unit_max", "wg_unit_min", "igemm_ksplit128", "w3_waves", "reduce_cus", "w3_dense")
    before = {k: ops.tune_value(k) for k in names}
    reached, per_label = set(), {}
    for c in cc.CASES:
        assert set(c.knobs) <= set(names), c.name
        with cc.knobs(c):
            pr = cc.probe(c)
        assert pr["label"] == c.label, (c.name, pr)
        for k, v in c.expect.items():
            assert pr[k] == v, (c.name, k, pr)
        if c.label.endswith("+bn") and c.label.startswith(cc.GLDS):          # the BatchNorm-backward epilogue turns the K-group split off
            assert pr["label"].count(",") == 2, pr
        if c.op in ("wgrad", "lin_wgrad") and "/units" in c.label:
            assert pr["units"] >= pr["tasks"] and pr["slots"] <= pr["units"] and pr["part"] > 0
        if c.op in ("wgrad", "lin_wgrad") and "/split" in c.label:
            assert (pr["part"] > 0) == (pr["splits"] > 1)
        reached.add(c.label)
        per_label[c.label] = per_label.get(c.label, 0) + 1
        assert {k: ops.tune_value(k) for k in names} == before, f"{c.name} left a knob changed"
    assert reached == set(cc.REQUIRED_LABELS), (set(cc.REQUIRED_LABELS) - reached, reached - set(cc.REQUIRED_LABELS))
    # plan formats the table must hold: unit lists cut into 1, 2 and >= 3 units per task and longer than one round; split counts 1, 2, > chunks
    by = {c.name: c for c in cc.CASES}
    with cc.knobs(by["wgu64_flat_2_units"]):
        pr = cc.probe(by["wgu64_flat_2_units"])
        assert pr["units_per_task"] == [2] and pr["units"] > ops.tune_value("wg_blocks")
    with cc.knobs(by["wgu64_conv_s2_1_2_3_units"]):          # from the plan's own unit table: tasks WITH work cut into 1, 2 and 3 units, more than one round
        pr = cc.probe(by["wgu64_conv_s2_1_2_3_units"])
        assert pr["units_per_task"] == [1, 2, 3] and pr["empty_tasks"] == 0 and pr["units"] > ops.tune_value("wg_blocks")
    with cc.knobs(by["wgu64_reduce_many_units"]):
        pr = cc.probe(by["wgu64_reduce_many_units"])
        assert pr["units"] >= 3 * pr["tasks"] and pr["slots"] > 8 * pr["tasks"]
    with cc.knobs(by["wgu64_conv_unreached_tap"]):
        pr = cc.probe(by["wgu64_conv_unreached_tap"])
        assert pr["slots"] < pr["units"] and pr["empty_tasks"] == 6, "the taps no position reaches are single empty units without a slab"
    with cc.knobs(by["wgu64_conv_s2_eight_queues"]):
        assert cc.probe(by["wgu64_conv_s2_eight_queues"])["taps"] == 9
    for c in (c for c in cc.CASES if c.op == "wgrad3" and "direct" in c.name):
        with cc.knobs(c):
            assert cc.probe(c)["splits"] == [1], c.name
    assert len(cc.CASES) == sum(per_label.values())


def test_assert_bits_is_sharp():
    c = next(c for c in cc.CASES if c.name == "conv_3x3_s1_classes")
    d = cc.build(c)
    ref = d["ref"]["out"].reshape(-1, c.shape["Co"])
    good = R.as_dtype(ref, torch.bfloat16)
    R.assert_bits(good, ref, "identity")
    R.assert_bits(-0.0 * torch.ones(2, 2).to(torch.bfloat16), torch.zeros(2, 2, dtype=F64), "-0 == +0")
    # one element one ulp off
    off = good.clone()
    r, col = (int(v) for v in (good.float().abs() > 0).nonzero()[7])
    off.view(torch.int16)[r, col] += 1
    with pytest.raises(AssertionError, match=rf"1 of .* first at \(row {r}, column {col}\)"):
        R.assert_bits(off, ref, "ulp", lambda rr, cc_: f"tile {rr // 64}")
    f32 = ref.float()
    off32 = f32.clone()
    off32.view(torch.int32)[r, col] += 1
    with pytest.raises(AssertionError, match="1 of"):
        R.assert_bits(off32, ref, "ulp fp32")
    # one row zeroed
    z = good.clone()
    rz = int((good.float().abs().sum(1) > 0).nonzero()[3])
    z[rz] = 0
    with pytest.raises(AssertionError, match=rf"\(1 rows\); first at \(row {rz},"):
        R.assert_bits(z, ref, "row")
    # one tap dropped for one border class: the top-left corner pixel loses its (kh, kw) = (1, 1) tap
    x, w = d["in"]["x"].double(), d["in"]["w"].double()
    drop = d["ref"]["out"].clone()
    drop[:, 0, 0, :] -= x[:, 0, 0, :] @ w[:, 1, 1, :].t()
    assert not torch.equal(drop, d["ref"]["out"])
    with pytest.raises(AssertionError, match="differ in bits"):
        R.assert_bits(R.as_dtype(drop, torch.bfloat16).reshape(-1, c.shape["Co"]), ref, "tap")
    # one statistics row omitted: the column sums lose one M tile's share
    acc = d["ref"]["out"].reshape(-1, c.shape["Co"])
    part = torch.stack([R.fwd_stats(acc[i: i + 64]) for i in range(0, acc.shape[0], 64)])
    R.assert_bits(part.sum(0).float(), d["ref"]["stats"], "stats")
    with pytest.raises(AssertionError, match="differ in bits"):
        R.assert_bits(part[:-1].sum(0).float(), d["ref"]["stats"], "stats row")
    # a touched guard element
    for dtype in (torch.bfloat16, torch.float32):
        buf, view = R.guarded(5, 6, 8, dtype, "cpu")
        R.assert_guard(buf, 5, 6, "clean")
        view.zero_()
        R.assert_guard(buf, 5, 6, "clean")
        buf[2, 7] = 0
        with pytest.raises(AssertionError, match="spare columns"):
            R.assert_guard(buf, 5, 6, "col")
        buf, _ = R.guarded(5, 6, 8, dtype, "cpu")
        buf[5, 0] = 1
        with pytest.raises(AssertionError, match="spare rows"):
            R.assert_guard(buf, 5, 6, "row")
    with pytest.raises(AssertionError, match="sentinel elements were written"):
        R.assert_untouched(torch.zeros(4), "flat")
    # the derived bounds are tighter than the aggregate tolerance they replace
    v = torch.tensor([[64.0]], dtype=F64)
    assert float(2.0 ** -8 * (v + R.gelu_slack(v)) + R.gelu_slack(v)) < 1.5e-2 * 64 / 3
    with pytest.raises(AssertionError, match="outside the derived bound"):
        R.assert_close_rows(torch.tensor([[1.01]]), torch.tensor([[1.0]], dtype=F64), torch.zeros(1, 1, dtype=F64), "close")


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_every_output_element_can_be_located(built, case):
    """the text assert_bits adds to a report: tap class and row tile for convolutions, tap / task tile / splits for weight gradients — and the tap
    classes restated here are the plan's own (count, and row tiles adding up to the plan's tile count)"""
    with cc.knobs(case):
        plan = cc.probe(case)
    for kind, ref in built[case.name]["ref"].items():
        if kind in ("pre", "gb", "z"):
            continue
        kind = "g" if kind == "g_swish" else kind
        flat = ref.reshape(-1, ref.shape[-1]) if ref.ndim > 1 else ref.reshape(1, -1)
        where = cc.where_of(case, kind, plan)
        for r, col in ((0, 0), (flat.shape[0] - 1, flat.shape[1] - 1), (flat.shape[0] // 2, flat.shape[1] // 3)):
            assert isinstance(where(r, col), str) and where(r, col)
    if case.op in ("conv_fwd", "dgrad", "dgrad_bn"):
        _, sizes, _ = cc.tap_classes(case)
        if plan["mode"] == 2:
            sizes = {k: v for k, v in sizes.items() if k}          # in place: pixels no tap reaches are not visited
        bm = cc._tile_edges(case.label)[0]
        assert len(sizes) == plan["classes"] and max(len(k) for k in sizes) == plan["max_taps"]
        assert sum(-(-case.shape["N"] * v // bm) for v in sizes.values()) == plan["tiles"]


def test_a_dropped_tap_is_reported_with_its_tap_class():
    c = next(c for c in cc.CASES if c.name == "conv_3x3_s1_classes")
    d = cc.build(c)
    x, w = d["in"]["x"].double(), d["in"]["w"].double()
    drop = d["ref"]["out"].clone()
    drop[:, 0, 0, :] -= x[:, 0, 0, :] @ w[:, 1, 1, :].t()          # the top-left corner class loses its centre tap
    with cc.knobs(c):
        where = cc.where_of(c, "out", cc.probe(c))
    with pytest.raises(AssertionError, match=r"pixel \(0, 0\), tap class \[\(1, 1\), \(1, 2\), \(2, 1\), \(2, 2\)\] \(4 taps"):
        R.assert_bits(R.as_dtype(drop, torch.bfloat16), d["ref"]["out"], "tap", where)
