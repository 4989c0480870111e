"""CPU-only: the float64 restatement of the stem kernels (tests/stem_restatement.py) against torch's own conv3d / max_pool2d / gelu with
autograd and against oracle/lrw_oracle.py's stem3d; the path every case of tests/test_gpu_stem_edges.py claims against the library's host
queries; which instantiations of k_stem_bwd_wgrad the accepted shapes reach; and the measured constants behind the GPU module's tolerances
(printed with -s, asserted against the recorded values)."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

import stem_restatement as sr
from stem_restatement import ACT_GELU, ACT_SWISH, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from syncvsr_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement is the operation
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dma-22x24", "sc-10x14", "T1-8x8", "T3-8x10", "wop-17"])
def test_convolution_and_weight_gradient_against_torch(name):
    c, x = sr.conv_case(name), sr.conv_inputs(name, "random")
    v = x["vid"].to(torch.bfloat16).to(F64).view(c.B, 1, c.T, c.H, c.W)
    w = x["w"].to(torch.bfloat16).to(F64).view(64, 1, 5, 7, 7).requires_grad_(True)
    ref = F.conv3d(v, w, stride=(1, 2, 2), padding=(2, 3, 3))                       # [B, 64, T, Ho, Wo]
    ref.backward(x["dy"].to(F64).view(c.B, c.T, c.H // 2, c.W // 2, 64).permute(0, 4, 1, 2, 3))
    want = ref.detach().permute(0, 2, 3, 4, 1).reshape(c.B * c.T, c.H // 2, c.W // 2, 64)
    out, s, q = sr.stem_conv_fwd(x["vid"], x["w"])
    assert _close(out, want) and _close(s, want.sum((0, 1, 2))) and _close(q, (want * want).sum((0, 1, 2)))
    assert _close(sr.stem_conv_wgrad(x["vid"], x["dy"]), w.grad.view(64, 5, 7, 7))
    r = sr.conv_reference(name, "random")
    assert _close(r["dw"], w.grad.view(64, 5, 7, 7))
    assert bool((r["dw"][r["dw_bound"] == 0] == 0).all()) and bool((r["dw_bound"] > 0).any())       # (a tap that only ever meets padding has no terms)


@pytest.mark.parametrize("act", sr.ACTS)
@pytest.mark.parametrize("Hc,Wc", [(8, 8), (11, 9), (1, 9), (2, 5)])
def test_pool_forward_and_backward_with_a_given_argmax_against_autograd(Hc, Wc, act):
    """float64 normal inputs (no two equal values in a window): the first-maximum arg-max is torch's, and the backward fed with it is autograd's"""
    g = torch.Generator().manual_seed(5 + Hc)
    N, C = 2, 16
    x = torch.randn(N, Hc, Wc, C, generator=g, dtype=F64).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    mean = x.mean((0, 1, 2))
    var = x.var((0, 1, 2), unbiased=False)
    z = (x - mean) * torch.rsqrt(var + 1e-5) * gamma + beta
    a = F.gelu(z) if act == ACT_GELU else F.silu(z)
    y = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    dpool = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dpool)
    m, r = mean.detach(), torch.rsqrt(var.detach() + 1e-5)
    z2, a2, y2 = sr.pool_fwd(x.detach(), m, r, gamma.detach(), beta.detach(), act)
    assert _close(z2, z.detach()) and _close(a2, a.detach()) and _close(y2, y.detach())
    amax = sr.reference_amax(a2)
    assert sr.certify_amax(amax, y2, None, x.detach(), a2, 0.0) == []
    got = sr.pool_bwd(dpool, amax, x.detach(), m, r, gamma.detach(), beta.detach(), act)
    assert _close(got.dx, x.grad, 1e-10) and _close(got.dgamma, gamma.grad, 1e-10) and _close(got.dbeta, beta.grad, 1e-10)
    # a slot moved to a neighbour is a different gradient: the given arg-max is what routes
    moved = amax.clone()
    moved[0, 0, 0, 0] = 8 if int(amax[0, 0, 0, 0]) != 8 else 4
    if Hc > 1 and Wc > 1:
        assert not _close(sr.pool_bwd(dpool, moved, x.detach(), m, r, gamma.detach(), beta.detach(), act).dx, x.grad, 1e-6)


def test_chain_against_the_oracles_stem3d():
    from oracle import lrw_oracle as O

    c, x = sr.conv_case("dma-22x24"), sr.conv_inputs("dma-22x24", "random")
    g = torch.Generator().manual_seed(3)
    gamma, beta = 1 + 0.2 * torch.randn(64, generator=g, dtype=F64), 0.2 * torch.randn(64, generator=g, dtype=F64)
    sd = {"stem3d.0.weight": x["w"].to(torch.bfloat16).to(F64).view(64, 1, 5, 7, 7), "stem3d.1.weight": gamma, "stem3d.1.bias": beta,
          "stem3d.1.running_mean": torch.zeros(64, dtype=F64), "stem3d.1.running_var": torch.ones(64, dtype=F64),
          "stem3d.1.num_batches_tracked": torch.zeros((), dtype=torch.long)}
    vid = x["vid"].to(torch.bfloat16).to(F64).view(c.B, 1, c.T, c.H, c.W)
    out, s, q = sr.stem_conv_fwd(x["vid"], x["w"])
    n = out.shape[0] * out.shape[1] * out.shape[2]
    mean = s / n
    rstd = torch.rsqrt(q / n - mean * mean + O.BN_EPS)
    for act, fn in ((ACT_GELU, None), (ACT_SWISH, F.silu)):
        want = O.stem3d(vid, sd, True, act=fn)                                    # [B, 64, T, Hp, Wp]
        y = sr.pool_fwd(out, mean, rstd, gamma, beta, act)[2]
        assert _close(y, want.permute(0, 2, 3, 4, 1).flatten(0, 1), 1e-9)


def test_the_certificate_refuses_a_wrong_argmax():
    x = sr.pool_inputs("g-11x9")
    z, a, y = sr.pool_fwd(x["x"], x["mean"], x["rstd"], x["gamma"], x["beta"], ACT_GELU)
    amax = sr.reference_amax(a)
    xwin = sr._at_slot(sr.windows(x["x"].to(F64), 0.0), amax).to(torch.bfloat16)
    yb = y.to(torch.bfloat16)
    assert sr.certify_amax(amax, yb, xwin, x["x"], a, sr.tie_eps(ACT_GELU)) == []
    bad = amax.clone()
    bad[1, 5, 4, 7] = 8                      # the last pooled row and column of an 11 x 9 frame: slot (2, 2) is outside
    assert "outside the frame" in sr.certify_amax(bad, yb, xwin, x["x"], a, sr.tie_eps(ACT_GELU))[0]
    bad = amax.clone()
    bad[0, 2, 2, 3] = (int(amax[0, 2, 2, 3]) + 1) % 9
    assert sr.certify_amax(bad, yb, xwin, x["x"], a, sr.tie_eps(ACT_GELU))
    y2 = yb.clone()
    y2[2, 1, 1, 0] = y2[2, 1, 1, 0] * 1.02
    assert any("one bf16 rounding" in f for f in sr.certify_amax(amax, y2, xwin, x["x"], a, sr.tie_eps(ACT_GELU)))


def test_integer_cases_are_exact_in_bf16_and_in_fp32_sums():
    for c in sr.CONV_CASES:
        r = sr.conv_reference(c.name, "int")
        assert float(r["out"].abs().max()) <= 245 and bool((r["out"] == r["out"].round()).all())
        assert float(r["out"].abs().sum((0, 1, 2)).max()) < 2 ** 24, c.name
        assert float(r["sumsq"].max()) < 2 ** 24, c.name
        assert float(r["sumsq"].min()) > 0, c.name


def test_impulses_are_one_per_channel_and_reach_the_edges():
    for c in sr.CONV_CASES:
        pos = sr.impulse_positions(c)
        Ho, Wo = c.H // 2, c.W // 2
        assert 1 <= len(pos) <= 64 and len(set(pos)) == len(pos), c.name
        assert all(0 <= b < c.B and 0 <= t < c.T and 0 <= y < Ho and 0 <= x < Wo for b, t, y, x in pos)
        ts, bs = {t for _, t, _, _ in pos}, {b for b, _, _, _ in pos}
        assert {0, c.T - 1} <= ts and {0, c.B - 1} <= bs, c.name
        assert {(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1)} <= {(y, x) for _, _, y, x in pos}, c.name
        if "partial_group" in c.crosses:
            assert any(y >= Ho // 4 * 4 for _, _, y, _ in pos)
        if "wgrad_cap" in c.crosses:
            gpf = (Ho + 3) // 4
            trips = {((b * c.T + t) * gpf + y // 4) // sr.WGRAD_CAP for b, t, y, _ in pos}
            assert {0, 1, 2, 3} <= trips, (c.name, trips)
        vid, dy, dw = sr.impulse_case(c.name)
        assert bool((vid != 0).all()) and float(dy.float().sum()) == len(pos)
        assert _close(sr.stem_conv_wgrad(vid, dy), dw, 0.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# every case takes the path it claims
# ------------------------------------------------------------------------------------------------------------------------------------
def _wgrad_pipe(W: int) -> bool:
    """the `pipe` condition of svsr_stem_conv_wgrad with use_tr"""
    WoP = (W // 2 + 15) // 16 * 16
    return W % 4 == 0 and (WoP + 8) // 2 <= 32 and sr.SW_RB * WoP * 8 <= 8 * 256


@pytest.mark.parametrize("name", [c.name for c in sr.CONV_CASES])
def test_convolution_cases_take_the_path_they_claim(lib, name):
    c = sr.conv_case(name)
    Ho, Wo = c.H // 2, c.W // 2
    ws = lib.svsr_stem_conv_fwd_ws_bytes(c.B, c.T, c.H, c.W)
    assert ("dma" in c.fwd) == (ws > 0), "the DMA kernel runs where the workspace query is non-zero"
    if ws:
        assert ws == 2 * (c.B * c.T * c.H * (c.W + 8) + 64 * 296) and "f4" in c.fwd and c.W % 8 == 0
    assert ("f4" in c.fwd) == (c.W % 4 == 0) and ("scalar" in c.fwd) == (c.W % 4 == 2)
    tiles = (Ho * Wo + 127) // 128 * c.B * c.T
    assert lib.svsr_stem_conv_fwd_stat_rows(c.B, c.T, c.H, c.W) == min(tiles, sr.FWD_CAP)
    splits, floats = ctypes.c_int(0), ctypes.c_int64(0)
    assert lib.svsr_stem_conv_wgrad_plan(c.B, c.T, c.H, c.W, ctypes.byref(splits), ctypes.byref(floats)) == 0
    groups = (Ho + 3) // 4 * c.B * c.T
    assert splits.value == min(groups, sr.WGRAD_CAP) and floats.value == splits.value * 64 * 245
    assert (c.wgrad == "pipe") == _wgrad_pipe(c.W) and c.wgrad in ("pipe", "tr")
    crosses = {"fwd_cap": tiles > sr.FWD_CAP, "wgrad_cap": groups > sr.WGRAD_CAP, "partial_tile": Ho * Wo % 128 != 0,
               "partial_group": Ho % 4 != 0, "wop_pad": Wo % 16 != 0, "short_T": c.T < 5}
    assert set(c.crosses) == {k for k, v in crosses.items() if v}, crosses


def test_the_edge_list_is_covered():
    names = {c.name: c for c in sr.CONV_CASES}
    assert {k for c in sr.CONV_CASES for k in c.crosses} == {"fwd_cap", "wgrad_cap", "partial_tile", "partial_group", "wop_pad", "short_T"}
    assert {k for c in sr.CONV_CASES for k in c.fwd} == {"dma", "f4", "scalar"} and {c.wgrad for c in sr.CONV_CASES} == {"pipe", "tr"}
    for T in (1, 2, 3, 4):
        assert any(c.B == 2 and c.T == T and "dma" in c.fwd for c in sr.CONV_CASES)
    assert {c.W // 2 for c in sr.CONV_CASES} >= {4, 15, 16, 17}
    assert _wgrad_pipe(96) and not _wgrad_pipe(100) and not _wgrad_pipe(98) and {"pipe-96", "pipe-100", "pipe-98"} <= set(names)
    c = names["dma-22x24"]
    assert (c.H // 2) * (c.W // 2) == 132 and 128 % (c.W // 2) != 0
    c = names["cap-12x8"]
    assert c.B * c.T == 785 and (c.H // 2 + 3) // 4 * c.B * c.T == 1570 and c.H // 2 == 6
    for n in sr.ISOLATION_CASES:
        assert names[n].B == 2
    assert {k for n in sr.ISOLATION_CASES for k in names[n].fwd} == {"dma", "f4", "scalar"}
    assert {c.form for c in sr.POOL_CASES} == {"gather", "lds", "plain"}
    for form in ("gather", "lds", "plain"):
        cs = [c for c in sr.POOL_CASES if c.form == form]
        assert any(c.Hc % 2 for c in cs) and any(c.Wc % 2 for c in cs) and any(c.Hc <= 2 for c in cs), form


def _pool_form(Wc: int, C: int) -> str:
    """svsr_stem_bn_act_pool_bwd's choice, restated from stem_bwd_uses_lds / stem_gather_lds / stem_bwd_gathers"""
    Wp = (Wc - 1) // 2 + 1
    lds = (sr.STEM_BR // 2 + 1) * Wp * C * 3 <= 60 * 1024
    gather_bytes = max(((2 * sr.STEM_GP + 1) * Wc * 8 + 255) // 256 * 256 * 16, 16384)
    return "gather" if C == 64 and lds and gather_bytes <= 64 * 1024 else "lds" if lds else "plain"


@pytest.mark.parametrize("name", [c.name for c in sr.POOL_CASES])
def test_pool_cases_take_the_form_they_claim(lib, name):
    """svsr_stem_bn_act_pool_bwd_rows tells the plain form from the two LDS-tiled ones; the gather form and the LDS form need the same number
    of partial rows at every height (ceil(ceil(Hc / 2) / 4) == ceil(Hc / 8)), so those two are told apart by the restated thresholds here and,
    on the GPU, by the refusal of want_dx=False outside the gather form (tests/test_gpu_stem_edges.py)."""
    c = sr.pool_case(name)
    Hp, _ = sr.pooled_hw(c.Hc, c.Wc)
    cv = c.C // 8
    rpb = max(1, min(c.Hc, 1024 // (c.Wc * cv)))
    rows = {"gather": c.N * ((Hp + 3) // 4), "lds": c.N * ((c.Hc + 7) // 8), "plain": c.N * ((c.Hc + rpb - 1) // rpb)}
    assert rows["gather"] == rows["lds"]
    assert _pool_form(c.Wc, c.C) == c.form
    assert lib.svsr_stem_bn_act_pool_bwd_rows(c.N, c.Hc, c.Wc, c.C) == rows[c.form]


def test_pool_form_thresholds(lib):
    assert [_pool_form(w, 64) for w in (56, 57, 58, 128, 129, 130)] == ["gather", "lds", "lds", "lds", "plain", "plain"]
    assert _pool_form(12, 128) == "lds" and _pool_form(64, 128) == "lds" and _pool_form(65, 128) == "plain"
    # 40 rows: the LDS forms need 5 partial rows a frame, the plain form (one row per workgroup from Wc = 129 on) 40
    assert [lib.svsr_stem_bn_act_pool_bwd_rows(1, 40, w, 64) for w in (56, 58, 128, 129, 130)] == [5, 5, 5, 40, 40]
    assert lib.svsr_stem_bn_act_pool_bwd_rows(1, 1, 9, 64) == 1 and lib.svsr_stem_bn_act_pool_bwd_rows(1, 2, 8, 64) == 1      # Hc = 1, 2 are accepted
    assert lib.svsr_stem_bn_act_pool_bwd_rows(1, 8, 8, 24) == 0                                                                # C = 24 is not


def _fused_variant(W: int) -> str:
    """the instantiation svsr_stem_bwd_wgrad picks (the <8,8> of the first version needed SW_RB * WoP * 8 > 6 * 256)"""
    WoP = (W // 2 + 15) // 16 * 16
    if sr.SW_RB * WoP * 8 > 6 * 256:
        return "8,8"
    return "6,6" if 5 * (2 * sr.SW_RB + 5) * (W // 4) <= 6 * 256 else "6,8"


def test_which_fused_backward_instantiations_the_accepted_shapes_reach(lib):
    seen, widths = {}, {}
    for H in range(8, 257, 2):
        for W in range(8, 257, 4):
            if lib.svsr_stem_bwd_wgrad_ok(1, 3, H, W):
                v = _fused_variant(W)
                seen[v] = seen.get(v, 0) + 1
                widths.setdefault(v, set()).add(W)
    print("STEM-CPU fused backward instantiations over even H in 8..256, W in 8..256 step 4:", seen,
          {v: (min(w), max(w)) for v, w in widths.items()})
    assert set(seen) == {"6,6", "6,8"}, "k_stem_bwd_wgrad<8,8> is unreachable: WoP >= 64 needs PW / 2 = 36 > 32"
    assert widths["6,6"] == set(range(8, 93, 4)) and widths["6,8"] == {96}
    assert not lib.svsr_stem_bwd_wgrad_ok(1, 3, 12, 100) and not lib.svsr_stem_bwd_wgrad_ok(1, 3, 12, 98) and not lib.svsr_stem_bwd_wgrad_ok(1, 3, 11, 96)
    for c in sr.FUSED_CASES:
        assert lib.svsr_stem_bwd_wgrad_ok(c.B, c.T, c.H, c.W) and _fused_variant(c.W) == c.variant, c.name
    blob = open(lib._name, "rb").read()
    assert b"k_stem_bwd_wgradILi6ELi6EE" in blob and b"k_stem_bwd_wgradILi6ELi8EE" in blob, "the two live instantiations are in the library"
    assert b"k_stem_bwd_wgradILi8ELi8EE" not in blob, "the unreachable one is gone"


def test_host_refusals(lib):
    """what the host queries refuse (the launchers' refusals are exercised on the GPU, with real buffers behind every pointer)"""
    for B, T, H, W in ((1, 1, 7, 8), (1, 1, 8, 7), (1, 1, 6, 8), (1, 1, 8, 6), (1, 1, 9, 16), (1, 1, 16, 9)):
        assert lib.svsr_stem_conv_wgrad_plan(B, T, H, W, None, None) != 0
        assert lib.svsr_stem_conv_fwd_ws_bytes(B, T, H, W) == 0 and not lib.svsr_stem_bwd_wgrad_ok(B, T, H, W)


# ------------------------------------------------------------------------------------------------------------------------------------
# the constants behind the GPU module's tolerances
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    m = {"out": (0.0, None), "y": (0.0, None), "dx": (0.0, None), "g": (0.0, None), "z": 0.0, "zterms": 0.0}

    def worst(key, val, where):
        if val > m[key][0]:
            m[key] = (val, where)

    for c in sr.CONV_CASES:
        x, ref = sr.conv_inputs(c.name, "random"), sr.conv_reference(c.name, "random")
        chk = sr.row_check("out", sr._bf(ref["out"]), ref["out"])
        worst("out", chk.worst, (c.name,) + chk.where)
    for c in sr.POOL_CASES:
        x = sr.pool_inputs(c.name)
        sc = (x["gamma"] * x["rstd"]).to(F64)
        m["zterms"] = max(m["zterms"], float(((x["x"].to(F64) * sc).abs() + (x["mean"].to(F64) * sc).abs() + x["beta"].to(F64).abs()).max()))
        for act in sr.ACTS:
            z, a, y = sr.pool_reference(c.name, act)
            m["z"] = max(m["z"], float(z.abs().max()))
            chk = sr.row_check("y", sr._bf(y), y)
            worst("y", chk.worst, (c.name, act) + chk.where)
            amax = sr.reference_amax(a)
            ref = sr.pool_bwd(x["dpool"], amax, x["x"], x["mean"], x["rstd"], x["gamma"], x["beta"], act)
            for label, win in sr.pool_forms(c):
                r = sr.pool_bwd(x["dpool"], amax, x["x"], x["mean"], x["rstd"], x["gamma"], x["beta"], act, rounded=True, win=win)
                chk = sr.row_check("dx", r.dx, ref.dx)
                worst("dx", chk.worst, (c.name, act, label) + chk.where)
                if win:
                    k = max(float(((r.dgamma - ref.dgamma).abs() / ref.rss_gx).max()), float(((r.dbeta - ref.dbeta).abs() / ref.rss_g).max()))
                    worst("g", k, (c.name, act))
    m["act"] = {act: sr.measure_act_error(act) for act in sr.ACTS}
    return m


@pytest.mark.parametrize("name", ["out", "y", "dx"])
def test_the_recorded_rounding_errors_are_what_the_restatement_gives(name, measured):
    got, recorded = measured[name], sr.ROUNDING[name]
    print(f"STEM-CPU rounding {name}: measured {got[0]:.4e} at {got[1]}, recorded {recorded:.4e}, tolerance {sr.tolerance(name):.4e} "
          f"(cap {sr.CAP[name]:.1e}), whole-tensor bound {sr.WHOLE_BOUND[name]:.1e}")
    assert 0.9 * recorded <= got[0] <= recorded, (name, got, recorded)
    assert sr.tolerance(name) == min(4 * recorded, sr.CAP[name])


def test_the_recorded_sum_and_tie_constants(measured):
    got = measured["g"]
    print(f"STEM-CPU bf16 g on dgamma / dbeta: measured {got[0]:.4e} of the root sum of squares at {got[1]}, recorded {sr.G_ROUNDING:.4e}")
    assert 0.9 * sr.G_ROUNDING <= got[0] <= sr.G_ROUNDING
    for act in sr.ACTS:
        e = measured["act"][act]
        print(f"STEM-CPU activation {act}: fp32 formula against float64 over |z| <= {sr.Z_RANGE}: {e:.4e}, recorded {sr.ACT_ERROR[act]:.4e}, "
              f"z error {sr.Z_ERROR:.3e}, tie epsilon {sr.tie_eps(act):.4e}")
        assert 0.9 * sr.ACT_ERROR[act] <= e <= sr.ACT_ERROR[act]
        assert sr.tie_eps(act) == 2 * (sr.ACT_ERROR[act] + sr.Z_ERROR)
    print(f"STEM-CPU pool cases: max |z| {measured['z']:.3f} (range {sr.Z_RANGE}), max terms of z {measured['zterms']:.3f} (bound {sr.Z_TERMS})")
    assert measured["z"] < sr.Z_RANGE and measured["zterms"] < sr.Z_TERMS
    # the erf formula's stated bound: 1.5e-7 on the CDF, so |z| * 1.5e-7 on the GELU, plus fp32 rounding of the product
    assert sr.ACT_ERROR[ACT_GELU] <= sr.Z_RANGE * 1.5e-7 + sr.Z_RANGE * 2.0 ** -23
    assert sr.ACT_ERROR[ACT_SWISH] <= sr.Z_RANGE * 3 * 2.0 ** -24 + 1e-7
