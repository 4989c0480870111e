"""Bit-exact parity of the contraction kernels at every tile edge and instantiation (-m gpu): tests/contraction_cases.py lists the cases,
tests/contraction_restatement.py says why equality of bits is the right check (exact operands under the 2^24 budget) and holds the float64
restatements.  Every test: set the case's knobs, assert the label about to launch, run into sentinel-guarded buffers, compare bits (the derived
bound for the GELU / Swish epilogues), check the guards, run again and require the same bits."""
import pytest
import torch

import contraction_cases as cc
import contraction_restatement as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _plan_label(plan, Ci, Co, bn_epi):
    return cc._glds_label(plan.meta, Ci, Co, bn_epi)


def _stats_begin(dev):
    """the per-stream scratch the wrappers take statistics rows from, filled with sentinels"""
    from syncvsr_amd import ops

    buf = ops.scratch(1)
    head = buf[: 1 << 20]
    head.view(torch.int32).fill_(R.SENT32)
    return buf


def _stats_sums(buf, rows: int, C: int, what: str):
    """float64 column sums of the partial rows; everything behind the last row must still be sentinels"""
    n = rows * 2 * C
    R.assert_untouched(buf[n: n + R.STAT_SPARE], f"{what}: statistics rows behind row {rows - 1}")
    part = buf[:n].cpu()
    assert not bool(R.sentinel_mask(part).any()), f"{what}: a statistics row below {rows} was not written"
    return part.view(rows, 2, C).double().sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# one launch of each operation -> {kind: host tensor}
# ---------------------------------------------------------------------------------------------------------------------
def _bn_args(I, dev):
    from syncvsr_amd.ops import _p

    t = {k: I[k].to(dev) for k in ("x", "mean", "rstd", "gamma", "beta", "y") if k in I}
    return t, (_p(t.get("y")), _p(t["x"]), _p(t["mean"]), _p(t["rstd"]), _p(t["gamma"]), _p(t["beta"]))


def _run_conv(c, d, dev):
    from syncvsr_amd import ops

    s, o, I = c.shape, c.opts, d["in"]
    N, H, W, Ci, Co, k, st, p = (s[n] for n in ("N", "H", "W", "Ci", "Co", "k", "s", "p"))
    Ho, Wo = R.out_size(H, k, st, p), R.out_size(W, k, st, p)
    out = {}
    if c.op == "conv_fwd":
        plan = ops.conv_plan(0, N, H, W, Co, k, st, p)
        assert _plan_label(plan, Ci, Co, False) == c.label
        pitch = o.get("pitch", Co)
        buf, view = R.guarded(N * Ho * Wo, Co, pitch, BF, dev)
        sbuf = _stats_begin(dev)
        stt = ops.igemm_fwd(plan, I["x"].to(dev), I["w"].to(dev), buf, Nimg=N, in_pix=H * W, Ci=Ci, in_pitch=Ci, Co=Co, out_pix=Ho * Wo,
                            out_pitch=pitch, wt_taps=k * k, want_stats=True)
        torch.cuda.synchronize()
        assert stt[1] == plan.tiles
        out["stats"] = _stats_sums(sbuf, plan.tiles, Co, c.name)
        R.assert_guard(buf, N * Ho * Wo, Co, c.name)
        out["out"] = view.cpu().reshape(N, Ho, Wo, Co)
        return out
    # data gradients: the launch contracts over the forward's Co and writes the forward's Ci
    mode = 2 if (c.op == "dgrad" and o.get("addend") == "inplace") else 1
    plan = ops.conv_plan(mode, N, H, W, Ci, k, st, p)
    assert _plan_label(plan, Co, Ci, c.op == "dgrad_bn") == c.label
    rows = N * H * W
    add = I.get("addend")
    reach = d["reach"].reshape(1, H * W, 1).expand(N, H * W, Ci).reshape(rows, Ci)
    if c.op == "dgrad":
        fill = add.reshape(rows, Ci) if o.get("addend") == "inplace" else None
        buf, view = R.guarded(rows, Ci, Ci, BF, dev, fill)
        if mode == 2:          # pixels no tap reaches must be left alone: they hold sentinels, not the addend
            view.view(torch.int16)[~reach.to(dev)] = R.SENT16
        addend = buf if mode == 2 else (add.to(dev) if add is not None else None)
        ops.igemm_fwd(plan, I["dy"].to(dev), I["wt"].to(dev), buf, Nimg=N, in_pix=Ho * Wo, Ci=Co, in_pitch=Co, Co=Ci, out_pix=H * W, out_pitch=Ci,
                      wt_taps=k * k, addend=addend)
        torch.cuda.synchronize()
        R.assert_guard(buf, rows, Ci, c.name)
        got = view.cpu()
        if mode == 2:
            R.assert_untouched(got[~reach], f"{c.name}: pixels no tap reaches (mode 2)")
            got = torch.where(reach, got, add.reshape(rows, Ci))
        out["out"] = got.reshape(N, H, W, Ci)
        return out
    fill = add.reshape(rows, Ci) if add is not None else None
    buf, view = R.guarded(rows, Ci, Ci, BF, dev, fill)
    t, bn = _bn_args(I, dev)
    sbuf = _stats_begin(dev)
    dy, wt = I["dy"].to(dev), I["wt"].to(dev)          # (held until the synchronize: a temporary's memory would go to the next allocation)
    ops._call("svsr_igemm_dgrad_bn", ops._p(dy), ops._p(wt), ops._p(buf), ops._p(buf) if add is not None else None, ops._p(sbuf),
              plan.words.data_ptr(), plan.meta, N, Ho * Wo, Co, Co, Ci, H * W, Ci, k * k, *bn, o.get("act", 1), ops._stream())
    torch.cuda.synchronize()
    out["sums"] = _stats_sums(sbuf, plan.tiles, Ci, c.name)
    R.assert_guard(buf, rows, Ci, c.name)
    out["g"] = view.cpu().reshape(N, H, W, Ci)
    return out


def _run_c64(c, d, dev):
    from syncvsr_amd import ops

    s, I, form = c.shape, d["in"], c.opts["form"]
    N, H, W = s["N"], s["H"], s["W"]
    assert ops._c64_ok(64, 64, 3, 1, 1, W) and cc.probe(c)["label"] == c.label
    rows, srows = N * H * W, int(ops._query("svsr_conv3x3_c64_stat_rows", N, H, W)[0])
    assert srows == cc.probe(c)["rows"] and (srows <= 2 or "reduce_cus" not in c.knobs)
    out = {}
    fill = I["addend"].reshape(rows, 64) if "addend" in I else None
    buf, view = R.guarded(rows, 64, 64, BF, dev, fill)
    img = buf[:rows].view(N, H, W, 64)
    sbuf = _stats_begin(dev)
    if form == "fwd":
        st = ops.conv3x3_c64(I["x"].to(dev), I["w"].to(dev), img, None, True, ops._conv_taps(3, 1))
        assert st[1] == srows
    else:
        taps = tuple((1 - kh, 1 - kw, kh * 3 + kw) for kh in range(3) for kw in range(3))
        if form == "dgrad":
            ops.conv3x3_c64(I["dy"].to(dev), I["wt"].to(dev), img, img, False, taps)
        else:
            tdy, tdx, tw = zip(*taps)
            t, bn = _bn_args(I, dev)
            dy, wt = I["dy"].to(dev), I["wt"].to(dev)          # (held until the synchronize: a temporary's memory would go to the next allocation)
            ops._call("svsr_conv3x3_c64_dgrad_bn", ops._p(dy), ops._p(wt), ops._p(buf), None, ops._p(sbuf), N, H, W,
                      ops._ints(tdy), ops._ints(tdx), ops._ints(tw), *bn, 1, ops._p(ops.c64_pixtab(N, H, W, dev)), ops._stream())
    torch.cuda.synchronize()
    if form != "dgrad":
        out["stats" if form == "fwd" else "sums"] = _stats_sums(sbuf, srows, 64, c.name)
    R.assert_guard(buf, rows, 64, c.name)
    out["out" if form != "dgrad_bn" else "g"] = view.cpu().reshape(N, H, W, 64)
    return out


def _run_linear(c, d, dev):
    from syncvsr_amd import ops

    s, o, I = c.shape, c.opts, d["in"]
    Rr, K, N, seq = s["R"], s["K"], s["N"], s.get("seq")
    out = {}
    if c.op == "linear":
        geo, _ = cc.rows_geo(s)
        plan = ops.rows_plan(*geo, N)
        assert _plan_label(plan, K, N, False) == c.label
        pitch, f32 = o.get("pitch", N), bool(o.get("f32"))
        alias = o.get("addend") == "alias"
        buf, view = R.guarded(Rr, N, pitch, torch.float32 if f32 else BF, dev, I["addend"] if alias else None)
        addend = None
        if alias:
            addend = buf
        elif o.get("addend"):
            addend, av = R.guarded(Rr, N, pitch, BF, dev, I["addend"])
        bias = I["bias"].to(dev) if "bias" in I else None
        res, pre = ops.linear_fwd(I["x"].to(dev), I["w"].to(dev), bias, rows=Rr, K=K, N=N, x_pitch=K, out=buf, out_pitch=pitch,
                                  gelu=o.get("act") == "gelu", out_f32=f32, addend=addend, seq=seq, relu=o.get("act") == "relu", alpha=o.get("alpha", 1.0))
        torch.cuda.synchronize()
        R.assert_guard(buf, Rr, N, c.name)
        out["out"] = view.cpu()
        if pre is not None:
            out["pre"] = pre[:Rr, :N].cpu()
        return out
    Np = I["wt"].shape[-1]
    geo, _ = cc.rows_geo(s, scatter=True)
    plan = ops.rows_plan(*geo, K)
    assert _plan_label(plan, Np, K, c.op != "lin_dgrad") == c.label
    if c.op == "lin_dgrad":
        rows_all = Rr if seq is None else (Rr // seq[2]) * seq[0]
        fill = I.get("addend")
        buf, view = R.guarded(rows_all, K, K, BF, dev, fill)
        ops.linear_dgrad(I["dy"].to(dev), I["wt"].to(dev), rows=Rr, N=N, K=K, dy_pitch=Np, out=buf, addend=buf if fill is not None else None, seq=seq,
                         alpha=o.get("alpha", 1.0))
        torch.cuda.synchronize()
        R.assert_guard(buf, rows_all, K, c.name)
        got = view.cpu()
        if seq is not None:
            tgt = R.seq_rows(Rr // seq[2], *seq)
            rest = torch.ones(rows_all, dtype=torch.bool)
            rest[tgt] = False
            if fill is None:
                R.assert_untouched(got[rest], f"{c.name}: rows outside the scattered slice")
            else:
                R.assert_bits(got[rest], fill[rest], f"{c.name}: rows outside the scattered slice")
            got = got[tgt]
        out["out"] = got
        return out
    buf, view = R.guarded(Rr, K, K, BF, dev)
    stats = torch.full((plan.tiles * 2 * K + R.STAT_SPARE,), R.SENT32, dtype=torch.int32, device=dev).view(torch.float32)
    dy, wt = I["dy"].to(dev), I["wt"].to(dev)
    if c.op == "lin_dgrad_relu":
        y, zeros, ones = I["y"].to(dev), torch.zeros(K, device=dev), torch.ones(K, device=dev)
        ops._call("svsr_igemm_dgrad_relu", ops._p(dy), ops._p(wt), ops._p(buf), ops._p(stats), plan.words.data_ptr(), plan.meta, Rr, 1, Np, Np, K, 1, K, 1,
                  ops._p(y), ops._p(zeros), ops._p(ones), float(o["gscale"]), ops._stream())
    else:
        t, bn = _bn_args(I, dev)
        ops._call("svsr_igemm_dgrad_bn", ops._p(dy), ops._p(wt), ops._p(buf), None, ops._p(stats), plan.words.data_ptr(), plan.meta, Rr, 1, Np, Np, K,
                  1, K, 1, *bn, o.get("act", 1), ops._stream())
    torch.cuda.synchronize()
    out["sums"] = _stats_sums(stats, plan.tiles, K, c.name)
    R.assert_guard(buf, Rr, K, c.name)
    out["g"] = view.cpu()
    return out


def _dw_buffer(shape, pre, dev):
    """fp32 dw carved out of a sentinel-filled flat buffer (pre: the values an add-mode launch adds to)"""
    n = int(torch.tensor(shape).prod())
    flat = torch.full((n + 256,), R.SENT32, dtype=torch.int32, device=dev).view(torch.float32)
    if pre is not None:
        flat[:n] = pre.to(dev).reshape(-1)
    return flat, flat[:n].view(*shape)


def _run_wgrad(c, d, dev):
    from syncvsr_amd import ops

    s, o, I = c.shape, c.opts, d["in"]
    assert cc.probe(c)["label"] == c.label
    out = {}
    if c.op == "group":
        probs, keep = [], []
        for i, q in enumerate(s["problems"]):
            K, N = q["K"], q["N"]
            flat, dw = _dw_buffer((N, K), I.get(f"dw0{i}"), dev)
            if f"dw0{i}" not in I:
                dw.zero_()
            db = None
            if q.get("db"):
                dflat, db = _dw_buffer((N,), I.get(f"db0{i}"), dev)
                if f"db0{i}" not in I:
                    db.zero_()
                keep.append((f"db{i}", dflat, db))
            keep.append((f"dw{i}", flat, dw))
            probs.append(dict(x=I[f"x{i}"].to(dev), dy=I[f"dy{i}"].to(dev), dw=dw, rows=q["R"], K=K, N=N, x_pitch=K, dy_pitch=N, seq=q.get("seq"), db=db))
        ops.linear_wgrad_group(probs, tile=o["tile"])
        torch.cuda.synchronize()
        for name, flat, view in keep:
            R.assert_untouched(flat[view.numel():], f"{c.name}: behind {name}")
            out[name] = view.cpu()
        return out
    mode, pre = o["mode"], I.get("dw0")
    if c.op == "lin_wgrad":
        K, N = s["K"], s["N"]
        flat, dw = _dw_buffer((N, K), pre if mode & 1 else None, dev)
        db = dflat = None
        if o.get("db"):
            dflat, db = _dw_buffer((N,), I.get("db0") if mode & 2 else None, dev)
        assert (pre is not None) == bool(mode & 1), "add modes run into pre-filled buffers, store modes into sentinels"
        ops.linear_wgrad(I["x"].to(dev), I["dy"].to(dev), dw, rows=s["R"], K=K, N=N, x_pitch=K, dy_pitch=N, seq=s.get("seq"), db=db, mode=mode)
        torch.cuda.synchronize()
        if db is not None:
            R.assert_untouched(dflat[N:], f"{c.name}: behind db")
            out["db"] = db.cpu()
    else:
        N, H, W, Ci, Co, k, st, p = (s[n] for n in ("N", "H", "W", "Ci", "Co", "k", "s", "p"))
        flat, dw = _dw_buffer((Co, k, k, Ci), pre if mode & 1 else None, dev)
        ops.conv2d_wgrad(I["x"].to(dev), I["dy"].to(dev), dw, k, st, p, use_tr=False, mode=mode)
        torch.cuda.synchronize()
    R.assert_untouched(flat[dw.numel():], f"{c.name}: behind dw")
    out["dw"] = dw.cpu()
    return out


def _run_w3(c, d, dev):
    from syncvsr_amd import ops

    s, o, I = c.shape, c.opts, d["in"]
    pr = cc.probe(c)
    assert pr["label"] == c.label
    out = {}
    if c.op == "wgrad3":
        x, dy = I["x"].to(dev), I["dy"].to(dev)
        assert ops.halo_wgrad_ok(x, dy, 3, 1, 1)
        flat, dw = _dw_buffer((s["Co"], 3, 3, s["Ci"]), I.get("dw0") if o["mode"] else None, dev)
        ops.conv2d_wgrad(x, dy, dw, 3, 1, 1, mode=o["mode"])
        torch.cuda.synchronize()
        R.assert_untouched(flat[dw.numel():], f"{c.name}: behind dw")
        out["dw"] = dw.cpu()
        return out
    # two links of different geometry + flush, against the stand-alone launches
    assert all(sp > 1 for sp in pr["splits"]), "both links must leave slabs"
    pending, bufs = None, []
    for i, q in enumerate(s["links"]):
        flat, dw = _dw_buffer((q["Co"], 3, 3, q["Ci"]), None, dev)
        pending = ops.conv3x3_wgrad_chain(I[f"x{i}"].to(dev), I[f"dy{i}"].to(dev), dw, pending, mode=0)
        bufs.append((flat, dw))
    ops.conv3x3_wgrad_flush(pending)
    torch.cuda.synchronize()
    for i, (flat, dw) in enumerate(bufs):
        R.assert_untouched(flat[dw.numel():], f"{c.name}: behind dw of link {i}")
        out[f"dw{i}"] = dw.cpu()
        alone = torch.empty_like(dw)
        ops.conv2d_wgrad(I[f"x{i}"].to(dev), I[f"dy{i}"].to(dev), alone, 3, 1, 1, mode=0)
        R.assert_bits(out[f"dw{i}"], alone.cpu(), f"{c.name}: link {i} against the stand-alone launch")
    return out


RUNNERS = {"conv_fwd": _run_conv, "dgrad": _run_conv, "dgrad_bn": _run_conv, "c64": _run_c64, "linear": _run_linear, "lin_dgrad": _run_linear,
           "lin_dgrad_relu": _run_linear, "lin_dgrad_bn": _run_linear, "wgrad": _run_wgrad, "lin_wgrad": _run_wgrad, "group": _run_wgrad,
           "wgrad3": _run_w3, "chain": _run_w3}


def _compare(c, d, got):
    ref, o = d["ref"], c.opts
    plan = cc.probe(c)          # (under the case's knobs: the caller holds them)
    for kind, g in sorted(got.items()):
        what = f"{c.name} [{c.label}] {kind}"
        if kind == "out" and o.get("act") == "gelu":
            R.assert_close_rows(g, ref["out"], R.gelu_slack(ref["pre"]), what)
        elif kind == "g" and "g_swish" in ref:
            R.assert_close_rows(g, ref["g_swish"], R.swish_slack(ref["gb"], ref["z"]), what)
        elif kind == "sums" and "g_swish" in ref:
            g64 = got["g"].double().reshape(-1, g.shape[-1])
            I = d["in"]
            xh = ((I["x"].double() - I["mean"].double()) * I["rstd"].double()).reshape(-1, g.shape[-1])
            R.assert_sum_rows(g[0], g64, what + " sum g")
            R.assert_sum_rows(g[1], g64 * xh, what + " sum g*xhat")
        elif kind == "sums" and c.op == "lin_dgrad_relu":
            R.assert_bits(g[0].float(), ref["sums"][0], what, cc.where_of(c, kind, plan))          # (the second half of a row is scratch there)
        elif kind in ("stats", "sums"):
            R.assert_bits(g.float(), ref[kind], what, cc.where_of(c, kind, plan))                  # float64 sum of the partial rows == the exact integers
        else:
            R.assert_bits(g, ref[kind], what, cc.where_of(c, kind, plan))


@pytest.mark.parametrize("case", cc.ordered(), ids=lambda c: c.name)
def test_contraction_is_bit_exact(dev, case):
    d = cc.build(case)
    assert max(R.budget_of(d["abs"]).values()) < R.LIMIT
    with cc.knobs(case):
        got = RUNNERS[case.op](case, d, dev)
        _compare(case, d, got)
        again = RUNNERS[case.op](case, d, dev)
    for kind, g in got.items():
        assert torch.equal(g.contiguous().view(torch.uint8), again[kind].contiguous().view(torch.uint8)), f"{case.name}: {kind} differs between two launches"
