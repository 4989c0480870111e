"""The float64 restatements of tests/lrs_loss_restatement.py, host side (no GPU): the CTC recursions against torch's CTCLoss and its autograd,
the label-smoothing loss against the oracle, the GLU + depthwise conv against F.conv1d's autograd, the deliberate breaks (each must change a
new case by more than the GPU tolerance and leave the shapes of tests/test_gpu_lrs_kernels.py alone), and the recorded rounding sizes that
set the tolerances of tests/test_gpu_lrs_loss_edges.py."""
import math

import pytest
import torch
import torch.nn.functional as F

import lrs_loss_restatement as lr
from lrs_loss_restatement import BF, F64, row_check


# ------------------------------------------------------------------------------------------------------------------------------------
# CTC
# ------------------------------------------------------------------------------------------------------------------------------------
def _torch_ctc(c: lr.CtcCase, z: torch.Tensor):
    zf = z[:, :c.V].to(F64).view(c.B, c.T, c.V).clone().requires_grad_(True)
    lp = zf.transpose(0, 1).log_softmax(2)
    tgt = lr.ctc_labels(c).clamp_min(1)                            # (the padding is never read: target_lengths says where a row ends)
    nll = F.ctc_loss(lp, tgt, torch.tensor(c.ilen), torch.tensor([len(y) for y in c.targets]), blank=0, reduction="none", zero_infinity=True)
    (nll.sum() / c.B * c.gout).backward()
    return nll.detach(), zf.grad.reshape(c.B * c.T, c.V)


@pytest.mark.parametrize("name", [c.name for c in lr.CTC_CASES])
def test_the_ctc_recursions_equal_torch_ctc_loss_and_its_autograd(name):
    c = lr.ctc_case(name)
    ref = lr.ctc_reference(name)
    nll, grad = _torch_ctc(c, lr.ctc_logits(c, False))
    assert torch.allclose(ref["nll"], nll, rtol=1e-12, atol=1e-12), (ref["nll"], nll)
    assert float(ref["loss"]) == pytest.approx(float(nll.sum()) / c.B, rel=1e-12, abs=1e-12)
    assert float((ref["dz"] - grad).abs().max()) < 1e-12 * max(1.0, float(grad.abs().max()))
    dz = ref["dz"].view(c.B, c.T, c.V)
    for b, n in enumerate(c.ilen):
        assert (dz[b, n:] == 0).all()
        if not ref["feasible"][b]:
            assert ref["nll"][b] == 0 and (dz[b] == 0).all()
    # what the NaN-filled inputs hide is never looked at
    nan = lr.ctc(lr.ctc_logits(c, True), lr.ctc_labels(c), c.ilen, c.B, c.T, c.V, c.gout)
    assert torch.equal(nan["dz"], ref["dz"]) and torch.equal(nan["nll"], ref["nll"])


def test_the_ctc_cases_are_those_the_issue_names():
    by = {c.name: c for c in lr.CTC_CASES}
    feas = lambda n: lr.ctc_reference(n)["feasible"].tolist()
    assert len(by) == len(lr.CTC_CASES)
    for c in lr.CTC_CASES + [lr.CTC_BAD_ILEN]:
        assert len(c.ilen) == c.B and all(len(y) <= c.Lmax and all(1 <= v < c.V for v in y) for y in c.targets)
        assert any(len(y) == c.Lmax for y in c.targets)
    assert by["empty-target"].targets[0] == () and feas("empty-target") == [True, True, True]
    assert by["T1-one-label"].T == 1 and feas("T1-one-label") == [True, False]
    assert feas("full-row") == [True, True, False] and len(by["full-row"].targets[0]) == by["full-row"].Lmax
    n = len(by["all-same"].targets[0])
    assert by["all-same"].ilen[:2] == (2 * n - 1, 2 * n - 2) and feas("all-same") == [True, False, True]
    d = by["distinct-exact"]
    assert len(set(d.targets[0])) == len(d.targets[0]) == d.ilen[0] and feas("distinct-exact") == [True, True, False]
    assert by["V2"].V == 2 and by["B1"].B == 1 and by["gout-ldo"].gout == 0.3 and by["gout-ldo"].ldo_extra == 64 and by["scaled-20"].scale == 20.0
    assert [len(y) for y in by["len-127-128-129"].targets] == [127, 128, 129] and [len(y) for y in by["len-256-257"].targets] == [256, 257]
    for n in ("len-127-128-129", "len-256-257"):
        c = by[n]
        assert all(feas(n)) and min(c.ilen) < c.T and c.T <= max(lr.frames_needed(y) for y in c.targets) + 3
        assert all(lr.frames_needed(y) <= t for y, t in zip(c.targets, c.ilen))
    y = by["len-256-257"].targets[1]
    assert y[130] == y[129] and y[-1] == y[-2]                      # equal neighbours past lattice state 256
    assert by["T600"].T == 600 and len(by["T600"].targets[0]) == 5 and by["V5049"].V == 5049


def test_an_input_as_long_as_its_distinct_target_has_the_gradient_softmax_minus_one_hot():
    c = lr.ctc_case("distinct-exact")
    ref = lr.ctc_reference(c.name)
    z = lr.ctc_logits(c, False)[:, :c.V].to(F64).view(c.B, c.T, c.V)
    for b in (0, 1):
        y = c.targets[b]
        want = torch.softmax(z[b, :len(y)], 1) - F.one_hot(torch.tensor(y), c.V)
        got = ref["dz"].view(c.B, c.T, c.V)[b, :len(y)] * c.B
        assert torch.allclose(got, want, rtol=0, atol=1e-13)


def test_an_item_whose_ilen_is_outside_1_to_T_is_no_item():
    c = lr.CTC_BAD_ILEN
    ref = lr.ctc_reference(c.name)
    bad = [b for b, n in enumerate(c.ilen) if n < 1 or n > c.T]
    assert bad == [0, 3, 4, 7] and sorted(bad + list(lr.CTC_BAD_ILEN_KEPT)) == list(range(c.B))
    dz = ref["dz"].view(c.B, c.T, c.V)
    for b in bad:
        assert ref["nll"][b] == 0 and (dz[b] == 0).all()
    k = list(lr.CTC_BAD_ILEN_KEPT)
    z = lr.ctc_logits(c, False).view(c.B, c.T, -1)[k].reshape(len(k) * c.T, -1)
    alone = lr.ctc(z, lr.ctc_labels(c)[k], [c.ilen[b] for b in k], len(k), c.T, c.V, c.gout * len(k) / c.B)
    assert torch.equal(alone["nll"], ref["nll"][k]) and torch.equal(alone["dz"].view(len(k), c.T, c.V), dz[k])
    assert (ref["nll"][k] > 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# label smoothing
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in lr.LS_CASES if c.kind != "bad-target"])
def test_the_label_smoothing_restatement_equals_the_oracle(name):
    from oracle import lrs_oracle as O
    c = lr.ls_case(name)
    z, t, inv = lr.ls_inputs(c, False)
    ref = lr.ls_reference(name)
    zf = z[:, :c.V].to(F64).view(1, c.R, c.V).clone().requires_grad_(True)
    loss = O.label_smoothing_loss(zf, t.view(1, c.R), c.smoothing, False) * inv            # (one "clip": the oracle's sum over the live rows)
    loss.backward()
    assert float(ref["loss"]) == pytest.approx(float(loss.detach()), rel=1e-12, abs=1e-13)
    assert float((ref["dz"] - zf.grad[0]).abs().max()) < 1e-13
    assert ref["live"] == int((t >= 0).sum())
    if ref["live"]:
        assert ref["correct"] / ref["live"] == pytest.approx(O.th_accuracy(zf.detach(), t.view(1, c.R)), abs=1e-12)
    else:
        assert ref["correct"] == 0 and float(ref["loss"]) == 0.0 and (ref["dz"] == 0).all()
    # the constructed ties: row 0 (target V - 1, the higher of the two tied columns) is not correct, row 1 (target 0) is
    if c.kind == "mixed":
        z2, t2 = z.clone(), t.clone()
        z2[0, 0] -= 1.0
        assert lr.ls_loss(z2, t2, c.V, c.smoothing, inv)["correct"] == ref["correct"] + 1


def test_a_target_past_the_vocabulary_poisons_the_loss_and_not_the_gradient():
    c = lr.ls_case("bad-target")
    ref = lr.ls_reference(c.name)
    assert math.isnan(float(ref["loss"])) and torch.isfinite(ref["dz"]).all() and ref["live"] == 4


def test_the_label_smoothing_cases_are_those_the_issue_names():
    assert {(c.R, c.V) for c in lr.LS_CASES if c.kind == "mixed"} >= {(R, V) for R in (1, 5, 27) for V in (2, 63, 64, 65)} | {(5, 5049)}
    assert {(c.smoothing, c.norm_len) for c in lr.LS_CASES if c.V == 65 and c.R == 27} == {(s, n) for s in (0.0, 0.1) for n in (False, True)}
    assert len({c.name for c in lr.LS_CASES}) == len(lr.LS_CASES) and any(c.ldo_extra for c in lr.LS_CASES)


# ------------------------------------------------------------------------------------------------------------------------------------
# GLU + depthwise conv
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in lr.DW_CASES if c.D == 64] + [lr.DW_MANY_TILES[1].name])
def test_the_glu_dwconv_restatement_equals_conv1d_and_its_autograd(name):
    c = lr.dw_case(name)
    x = lr.dw_inputs(c)
    ref = lr.dw_reference(name)
    B, T, D, K = c
    uf = x["u"].to(F64).view(B, T, 2 * D).clone().requires_grad_(True)
    wf, bf_ = x["w"].to(F64).clone().requires_grad_(True), x["bias"].to(F64).clone().requires_grad_(True)
    g = uf[..., :D] * torch.sigmoid(uf[..., D:])
    cr = F.conv1d(g.transpose(1, 2), wf.view(D, 1, K), bf_, padding=(K - 1) // 2, groups=D).transpose(1, 2).reshape(B * T, D)
    cr.backward(x["dc"].to(F64))
    for n, want in (("c", cr.detach()), ("du", uf.grad.reshape(B * T, 2 * D)), ("dw", wf.grad), ("dbias", bf_.grad)):
        assert float((ref[n] - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max())), n
    ntt = (T + 31) // 32
    assert ref["stats"].shape == (B * ntt, 2, D)
    cv = cr.detach().view(B, T, D)
    for b in range(B):
        for i in range(ntt):
            blk = cv[b, 32 * i:32 * i + 32]
            assert torch.allclose(ref["stats"][b * ntt + i, 0], blk.sum(0), rtol=0, atol=1e-11)
            assert torch.allclose(ref["stats"][b * ntt + i, 1], (blk * blk).sum(0), rtol=0, atol=1e-11)


def test_the_glu_dwconv_cases_are_those_the_issue_names():
    assert {(c.T, c.K, c.D) for c in lr.DW_CASES} == {(T, K, D) for T in (1, 31, 32, 33, 65) for K in (1, 3, 15, 31) for D in (64, 192)}
    for c in lr.DW_MANY_TILES:
        assert c.B * ((c.T + 31) // 32) > lr.DW_SPLITS
    from syncvsr_amd import ops
    assert ops.DW_SPLITS == lr.DW_SPLITS


# ------------------------------------------------------------------------------------------------------------------------------------
# embedding backward
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_embedding_backward_restatement_is_a_loop_over_rows():
    c = lr.EmbCase(0, 27, 8)
    tok, dx, scale = lr.emb_inputs(c, False)
    start = torch.full((lr.EMB_V, c.D), 0.5)
    ref = lr.embed_pos_bwd(tok, dx, lr.EMB_V, scale, start)
    want = start.to(F64).clone()
    for r in range(c.R):
        want[tok[r]] += dx[r].to(F64) * scale
    assert torch.allclose(ref["demb"], want, rtol=0, atol=1e-13) and int(ref["rows"].sum()) == c.R


def test_the_embedding_cases_are_those_the_issue_names():
    assert {(c.n_big, c.D) for c in lr.EMB_CASES if c.n_big} == {(n, D) for n in (4064, 4065, 4200) for D in (8, 264)}
    assert lr.EMB_LIST_CAP == 4064 and any(c.R == lr.EMB_MAX_ROWS for c in lr.EMB_CASES)
    for c in lr.EMB_CASES:
        tok, dx, scale = lr.emb_inputs(c, True)
        assert int((tok == lr.EMB_BIG).sum()) == c.n_big and tok.numel() == c.R <= lr.EMB_MAX_ROWS
        ref = lr.embed_pos_bwd(tok, dx, lr.EMB_V, scale)
        assert float(ref["demb_abs"].max()) < 2 ** 24 and (ref["demb"] == ref["demb"].round()).all()      # exact in fp32, whatever the order


# ------------------------------------------------------------------------------------------------------------------------------------
# the deliberate breaks
# ------------------------------------------------------------------------------------------------------------------------------------
def _old_ctc_case():
    """tests/test_gpu_lrs_kernels.py::test_ctc at its largest target (40 labels, S = 81)"""
    g = torch.Generator().manual_seed(7)
    ys = tuple(tuple(int(v) for v in torch.randint(1, 41, (n,), generator=g)) for n in (40, 12, 25))
    return lr.CtcCase("old", 90, 41, ys, (90, 50, 70), 40)


@pytest.mark.parametrize("brk", ["drop_states_256", "skip_equal_256"])
def test_a_broken_ctc_lattice_fails_the_long_targets_only(brk):
    caught = []
    for c in lr.CTC_CASES:
        if max(len(y) for y in c.targets) < 128 and c.name != "T600":
            continue
        ref = lr.ctc_reference(c.name)
        out = lr.ctc(lr.ctc_logits(c, False), lr.ctc_labels(c), c.ilen, c.B, c.T, c.V, c.gout, brk=brk)
        chk = row_check("dz", _bf(out["dz"]), ref["dz"])
        if chk.worst > lr.tolerance("ctc_dz") or chk.nonzero or not torch.allclose(out["nll"], ref["nll"], rtol=2e-4, atol=0):
            caught.append(c.name)
    assert caught == ["len-127-128-129", "len-256-257"], caught
    c = _old_ctc_case()
    z, lab = lr.ctc_logits(c, False), lr.ctc_labels(c)
    a, b = lr.ctc(z, lab, c.ilen, c.B, c.T, c.V), lr.ctc(z, lab, c.ilen, c.B, c.T, c.V, brk=brk)
    assert torch.equal(a["dz"], b["dz"]) and torch.equal(a["nll"], b["nll"])


def _bf(x):
    return x.float().to(BF).to(F64)


def test_a_backward_that_takes_one_tile_per_split_fails_the_many_tile_cases_only():
    for c in lr.DW_MANY_TILES:
        ref = lr.dw_reference(c.name)
        out = lr.glu_dwconv(**lr.dw_inputs(c), B=c.B, T=c.T, D=c.D, K=c.K, brk="one_tile_per_split")
        assert row_check("du", _bf(out["du"]), ref["du"]).worst > lr.tolerance("du")
        assert lr.bound_check(out["dw"], ref["dw"], lr.sum_bound(c.B * c.T + 2, ref["dw_abs"]))[0] > 1
        assert lr.bound_check(out["dbias"], ref["dbias"], lr.sum_bound(c.B * c.T + 2, ref["dbias_abs"]))[0] > 1
    for c in lr.DW_CASES[:3] + [lr.DwCase(3, 70, 128, 7), lr.DwCase(2, 150, 64, 31)]:      # the latter: shapes of test_glu_dwconv
        x = lr.dw_inputs(c)
        a, b = lr.glu_dwconv(**x, B=c.B, T=c.T, D=c.D, K=c.K), lr.glu_dwconv(**x, B=c.B, T=c.T, D=c.D, K=c.K, brk="one_tile_per_split")
        assert all(torch.equal(a[n], b[n]) for n in a)


def test_an_embedding_backward_that_stops_at_the_list_cap_fails_past_4064_rows_only():
    for c in lr.EMB_CASES:
        tok, dx, scale = lr.emb_inputs(c, True)
        a, b = lr.embed_pos_bwd(tok, dx, lr.EMB_V, scale), lr.embed_pos_bwd(tok, dx, lr.EMB_V, scale, brk="list_cap_rows")
        assert torch.equal(a["demb"], b["demb"]) == (c.n_big <= lr.EMB_LIST_CAP), c.name


# ------------------------------------------------------------------------------------------------------------------------------------
# the rounding constants
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounding():
    worst = {}

    def see(key, case, t):
        chk = row_check(key, _bf(t), t)
        assert chk.nonzero == 0
        if chk.worst > worst.get(key, (0.0,))[0]:
            worst[key] = (chk.worst, case, chk.where)

    for c in lr.CTC_CASES + [lr.CTC_BAD_ILEN]:
        see("ctc_dz", c.name, lr.ctc_reference(c.name)["dz"])
    for c in lr.LS_CASES:
        see("ls_dz", c.name, lr.ls_reference(c.name)["dz"])
    for c in lr.DW_CASES + lr.DW_MANY_TILES:
        ref = lr.dw_reference(c.name)
        see("c", c.name, ref["c"])
        see("du", c.name, ref["du"])
    return worst


@pytest.mark.parametrize("name", sorted(lr.ROUNDING))
def test_the_recorded_rounding_errors_are_what_the_restatement_gives(name, rounding):
    got, recorded = rounding[name], lr.ROUNDING[name]
    print(name, got, recorded)
    assert 0.9 * recorded <= got[0] <= recorded, (name, got, recorded)
    assert got[0] <= 2.0 ** -8                                         # one bf16 rounding per element
    assert lr.tolerance(name) == min(4 * recorded, lr.WHOLE_BOUND[name]) <= 6e-3
