"""The references of the beam-search kernel tests, on the CPU (tests/search_cases.py): the fp64 statement of source attention against
plain `torch.softmax` attention on each clip's unpadded tensors; the fp32 restatement of the kernel's chunked online softmax inside the
bound the GPU test applies, and two wrong variants of it (no rescale of the earlier chunks; the last key of a partial chunk dropped)
outside it — the inputs can tell a wrong kernel from a right one; and the order `beam_select_reference` gives on the selection's edge cases."""
import pytest
import torch

import search_cases as SC


@pytest.mark.parametrize("name", list(SC.SRC_STEP_SHAPES))
def test_src_step_reference_equals_softmax_attention_per_clip(name):
    case, want, A = SC.src_step_shape(name)
    H, Tmax, D = case["H"], case["Tmax"], case["H"] * 64
    q = case["q_wide"][:, D : 2 * D].double()
    live = 0
    for r, c in enumerate(case["clip_of"]):
        if not 0 <= c < len(case["tlens"]) or case["tlens"][c] < 1:
            assert not want[r].any() and not A[r].any()
            continue
        T = min(case["tlens"][c], Tmax)
        clip = case["kv"][c * Tmax : c * Tmax + T, : 2 * D].double()                       # the clip alone, unpadded
        assert bool(torch.isfinite(clip).all())
        k, v = clip[:, :D].view(T, H, 64).transpose(0, 1), clip[:, D:].view(T, H, 64).transpose(0, 1)      # [H, T, 64]
        p = torch.softmax(torch.einsum("hd,htd->ht", q[r].view(H, 64), k) * case["scale"], dim=-1)
        assert float((torch.einsum("ht,htd->hd", p, v).reshape(D) - want[r]).abs().max()) <= 1e-12
        assert float((torch.einsum("ht,htd->hd", p, v.abs()).reshape(D) - A[r]).abs().max()) <= 1e-12
        if r in case["peaks"] and T > 1:                                                    # the peak key holds the weight (bf16 inputs: about 12)
            assert float(p[:, case["peaks"][r]].min()) > 0.95, (r, float(p[:, case["peaks"][r]].min()))
        live += 1
    assert live >= 1 and bool(torch.isfinite(want).all())
    # the padding is NaN and was never read
    assert bool(torch.isnan(case["kv"][:, 2 * D :].float()).all())


def _restated(name, **kw):
    case, want, A = SC.src_step_shape(name)
    D = case["H"] * 64
    got = SC.src_step_chunked_fp32(case["q_wide"][:, D : 2 * D], case["kv"], case["clip_of"], case["tlens"], case["Tmax"], case["H"], case["scale"], **kw)
    return SC.src_step_ratio(got, want, A), got, case


@pytest.mark.parametrize("name", list(SC.SRC_STEP_SHAPES))
def test_fp32_chunked_restatement_stays_within_the_bound(name):
    ratio, got, case = _restated(name)
    print(f"{name}: fp32 chunked restatement, max error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    for r in SC.src_step_dead_rows(case):
        assert not got[r].any()


@pytest.mark.parametrize("name", ["t150", "t130"])
@pytest.mark.parametrize("mutant", ["skip_rescale", "drop_partial_tail"])
def test_wrong_restatements_leave_the_bound(name, mutant):
    ratio, _, _ = _restated(name, **{mutant: True})
    print(f"{name}: {mutant}, max error / bound = {ratio:.3g}")
    assert ratio > 1.0


def test_src_step_ratio_counts_any_error_in_a_dead_row_and_nan():
    want, A = torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64)
    got = torch.zeros(2, 4)
    assert SC.src_step_ratio(got, want, A) == 0.0
    got[1, 2] = 1e-30
    assert SC.src_step_ratio(got, want, A) == float("inf")
    got[1, 2] = float("nan")
    assert SC.src_step_ratio(got, want + 1, A + 1) == float("inf")


@pytest.mark.parametrize("name", list(SC.BEAM_EDGE_CASES))
def test_beam_select_reference_orders_the_edge_cases(name):
    """Per clip: totals non-increasing under the documented order (NaN above everything), strictly so or tied with increasing flat index."""
    planes, weights, run, rows, V, beam, (prev, tok, total, vals, count) = SC.beam_edge_case(name)
    row_lo, out_off, o = SC.beam_layout(rows, V, beam)
    assert count == [min(beam, r * V) for r in rows] and total.numel() == o and vals.shape == (len(planes), o)
    assert int(tok.max()) < V                                                               # columns V .. of a wide pitch never win
    key = SC.beam_rank_key(total)
    ties = 0
    for c, k in enumerate(count):
        s = slice(out_off[c], out_off[c] + k)
        assert bool(((prev[s] >= row_lo[c]) & (prev[s] < row_lo[c + 1])).all())
        flat = (prev[s] - row_lo[c]) * V + tok[s]
        kk = key[s]
        assert bool(((kk[:-1] > kk[1:]) | ((kk[:-1] == kk[1:]) & (flat[:-1] < flat[1:]))).all()), (name, c)
        ties += int((kk[:-1] == kk[1:]).sum())
    assert ties > 0
    for i, p in enumerate(planes):
        got, want = vals[i], p[prev, tok]
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])


def test_beam_select_reference_special_values_come_out_as_documented():
    planes, weights, run, rows, V, beam, (prev, tok, total, vals, count) = SC.beam_edge_case("special_all")
    p = planes[0]
    for lo, hi, off in ((0, 3, 0), (3, 5, 123)):
        blk = p[lo:hi].reshape(-1)
        n_nan, n_pinf, n_ninf = int(torch.isnan(blk).sum()), int((blk == float("inf")).sum()), int((blk == -float("inf")).sum())
        assert min(n_nan, n_pinf, n_ninf) >= 1
        t = total[off : off + blk.numel()]
        flat = (prev[off : off + blk.numel()] - lo) * V + tok[off : off + blk.numel()]
        assert bool(torch.isnan(t[:n_nan]).all()) and flat[:n_nan].tolist() == torch.nonzero(torch.isnan(blk)).view(-1).tolist()
        assert bool((t[n_nan : n_nan + n_pinf] == float("inf")).all()) and bool((t[-n_ninf:] == -float("inf")).all())
        assert bool(torch.isfinite(t[n_nan + n_pinf : -n_ninf]).all())
    planes, weights, run, rows, V, beam, (prev, tok, total, vals, count) = SC.beam_edge_case("special_wide")
    assert int(torch.isnan(total).sum()) == 3 and int((total == float("inf")).sum()) == 2 and bool(torch.isfinite(total[5:]).all())
    assert (prev * V + tok)[:5].tolist() == [2047, 17 * V + 100, 39 * V + 5048, 2048, 25 * V]


def test_beam_boundary_cases_put_the_winners_where_they_say():
    for which in ("straddle", "tail", "head"):
        planes, weights, run, rows, V, beam, flats = SC.beam_boundary_case(which)
        prev, tok, total, vals, count = SC.beam_edge_case(which)[6]
        assert sorted((prev * V + tok).tolist()) == sorted(flats) and count[0] == 40
        slices = sorted({f // 2048 for f in flats})
        assert slices == {"straddle": [0, 1, 2], "tail": [98], "head": [0]}[which]
        if which == "straddle":
            assert (prev * V + tok).tolist() == flats and int(total.view(torch.int32).unique().numel()) == 1
        if which == "head":
            assert count == [40, 0]
