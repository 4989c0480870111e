"""The beam search on the GPU (-m gpu): the three entry points of csrc/lrs_search.hip against their statements, the clip-aware
decoder step against the single-clip one, `BatchBeamSearch.forward_clips` under the criteria tests/test_gpu_lrs_infer.py and
tests/test_gpu_lrs_lm.py apply to `forward`, per clip, and `forward` as the one-clip group of the same search that it is."""
import numpy as np
import pytest
import torch

import search_cases as SC
from golden_cases import build_lrs_infer_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------------------------------
# svsr_beam_select
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,V,beam", [([1], 41, 40), ([1, 5, 2, 3], 300, 7), ([40] * 16, 5049, 40), ([40, 0, 17], 5049, 40), ([3, 2], 41, 256)])
def test_beam_select_kernel_equals_its_torch_statement(dev, rows, V, beam):
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_infer import LOGZERO, beam_select_reference

    g = torch.Generator().manual_seed(V + len(rows))
    n, C = sum(rows), len(rows)
    row_lo = [0]
    for r in rows:
        row_lo.append(row_lo[-1] + r)
    out_off, o = [], 0
    for r in rows:
        out_off.append(o)
        o += min(beam, r * V)
    # log-probability-like planes on a coarse grid (exact ties among the best), a CTC-like plane that is LOGZERO outside a few candidates
    planes = [(-torch.randint(0, 40, (n, V), generator=g).float() * 0.25), torch.full((n, V), LOGZERO), -torch.rand(n, V, generator=g) * 8]
    live = torch.rand(n, V, generator=g) < (0.9 if V < 100 else 0.01)
    planes[1][live] = -torch.randint(0, 16, (int(live.sum()),), generator=g).float() * 0.5
    planes[2] = (planes[2] * 4).round() / 4
    weights = [0.9, 0.1, 0.3]
    run = -torch.randint(0, 6, (n,), generator=g).float() * 0.5
    planes = [p.to(dev) for p in planes]
    run = run.to(dev)
    clip_of = torch.tensor([c for c, r in enumerate(rows) for _ in range(r)], dtype=torch.int32, device=dev)
    w_prev, w_tok, w_total, w_vals, w_count = beam_select_reference(planes, weights, run, row_lo, beam, V)
    got = []
    for _ in range(2):
        got.append(ops.beam_select(planes, weights, run, clip_of, torch.tensor(row_lo, dtype=torch.int32, device=dev),
                                   torch.tensor(out_off, dtype=torch.int32, device=dev), beam=beam, V=V, max_rows=max(rows), out_rows=o))
    prev, tok, total, vals, clip_out, count = got[0]
    torch.cuda.synchronize()
    assert count.tolist() == w_count
    assert torch.equal(prev, w_prev) and torch.equal(tok, w_tok)
    assert torch.equal(total.view(torch.int32), w_total.view(torch.int32))                  # bit for bit
    assert torch.equal(vals, w_vals) and torch.equal(clip_out, clip_of[w_prev])
    assert all(torch.equal(a, b) for a, b in zip(got[0], got[1]))                            # run to run
    t = w_total.cpu()
    ties = sum(int((t[row_lo_c : row_lo_c + k][1:] == t[row_lo_c : row_lo_c + k][:-1]).sum()) for row_lo_c, k in zip(out_off, w_count))
    print(f"rows {rows[:4]}.. V {V} beam {beam}: {o} winners, {ties} exact ties among neighbours, {int((t < -1e8).sum())} LOGZERO winners")
    assert ties > 0



def _bits(t):
    return t.view(torch.int32) if t.is_floating_point() else t


def _same_but_nan(got, want):
    """NaN where the reference has NaN, and the reference's bits everywhere else"""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got[~nan]), _bits(want[~nan]))


@pytest.mark.parametrize("name", list(SC.BEAM_EDGE_CASES))
def test_beam_select_kernel_at_its_documented_edges(dev, name):
    """tests/search_cases.py BEAM_EDGE_CASES against `beam_select_reference` (tests/test_search_cases_cpu.py checks the reference's own order
    on the same inputs): 1, 2 and 4 planes (the fourth with a negative weight); a row pitch wider than V whose extra columns hold NaN and
    +inf; NaN (above everything, by index), +inf and -inf among the totals of one plane; the 40 winners tied across two slice boundaries,
    all inside the last partial slice, and all inside slice 0 beside a clip without rows.  Indices exact, totals and values bit for bit
    where not NaN, two launches bit for bit."""
    from syncvsr_amd import ops

    planes, weights, run, rows, V, beam, (w_prev, w_tok, w_total, w_vals, w_count) = SC.beam_edge_case(name)
    row_lo, out_off, o = SC.beam_layout(rows, V, beam)
    i32 = dict(dtype=torch.int32, device=dev)
    d_planes, d_run = [p.to(dev) for p in planes], run.to(dev)
    assert all(p.stride(0) == planes[0].shape[1] for p in d_planes)
    clip_of = torch.tensor([c for c, r in enumerate(rows) for _ in range(r)], **i32)
    got = [ops.beam_select(d_planes, weights, d_run, clip_of, torch.tensor(row_lo, **i32), torch.tensor(out_off, **i32), beam=beam, V=V,
                           max_rows=max(rows), out_rows=o) for _ in range(2)]
    torch.cuda.synchronize()
    prev, tok, total, vals, clip_out, count = [t.cpu() for t in got[0]]
    assert count.tolist() == w_count
    assert torch.equal(prev, w_prev) and torch.equal(tok, w_tok)
    assert _same_but_nan(total, w_total) and _same_but_nan(vals, w_vals)
    assert torch.equal(clip_out, clip_of.cpu()[w_prev])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got[0], got[1]))              # run to run
    print(f"{name}: rows {rows} V {V} pitch {planes[0].shape[1]} beam {beam} planes {len(planes)}: {o} winners, {int(torch.isnan(w_total).sum())} NaN, "
          f"{int(torch.isinf(w_total).sum())} inf")


def test_beam_select_rejects_what_it_cannot_rank(dev):
    from syncvsr_amd import ops

    assert ops.beam_select_slices(5049, 40, 40) == 99 and ops.beam_select_slices(5049, 40, 82) > 0
    assert ops.beam_select_slices(5049, 40, 83) == 0 and ops.beam_select_slices(41, 257, 1) == 0 and ops.beam_select_slices(5049, 1, 208) == 0
    z = torch.zeros(83, 5049, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="cannot rank"):
        ops.beam_select([z], [1.0], z[:, 0].contiguous(), torch.zeros(83, **i32), torch.tensor([0, 83], **i32), torch.tensor([0], **i32), beam=40, V=5049,
                        max_rows=83, out_rows=40)
    with pytest.raises(ValueError, match="planes"):
        ops.beam_select([z] * 5, [1.0] * 5, z[:, 0].contiguous(), torch.zeros(83, **i32), torch.tensor([0, 83], **i32), torch.tensor([0], **i32), beam=4,
                        V=5049, max_rows=83, out_rows=4)


# ----------------------------------------------------------------------------------------------------------------------
# svsr_ctc_prefix_score_clips
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tlens,V,per,S", [([16, 9, 5], 41, 3, 7), ([150, 37, 88, 4], 5049, 10, 60), ([37, 20], 300, 2, None)])
def test_ctc_prefix_clips_kernel_matches_restatement_per_clip(dev, tlens, V, per, S):
    """Tolerances of test_ctc_prefix_kernel_matches_restatement_over_several_steps; the padding of logp and r_prev is NaN throughout: a
    read of it would surface in the outputs."""
    from oracle import lrs_oracle as O
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(sum(tlens) + V)
    C, Tmax, eos = len(tlens), max(tlens), V - 1
    logp = torch.full((C, Tmax, V), float("nan"))
    for c, T in enumerate(tlens):
        logp[c, :T] = torch.log_softmax(2.0 * torch.randn(T, V, generator=g), dim=-1)
    n = C * per
    clip_of = torch.arange(C).repeat_interleave(per)
    r_prev = torch.full((n, Tmax, 2), float("nan"))
    for r in range(n):
        T = tlens[clip_of[r]]
        r_prev[r, :T, 0] = O.CTC_LOGZERO
        r_prev[r, :T, 1] = torch.cumsum(logp[clip_of[r], :T, 0], 0)
    last = torch.full((n,), eos, dtype=torch.int64)
    tl = torch.tensor(tlens, dtype=torch.int32, device=dev)
    for step in range(4):
        ids = None if S is None else torch.stack([torch.randperm(V, generator=g)[:S] for _ in range(n)])
        if ids is not None and step > 0:
            ids[:, 0] = last
            ids[0, 1], ids[1, 1] = eos, 0
        r_new, psi = ops.ctc_prefix_score_clips(logp.to(dev), tl, r_prev.to(dev).contiguous(), last.to(dev), None if ids is None else ids.to(dev),
                                                clip_of.to(dev, torch.int32), step, 0, eos)
        torch.cuda.synchronize()
        r_new, psi = r_new.cpu(), psi.cpu()
        assert bool(torch.isfinite(r_new).all()) and bool(torch.isfinite(psi).all())
        nxt = torch.full((n, Tmax, 2), float("nan"))
        j = torch.randint(1 if S is None else 2, (S or V) - 1, (n,), generator=g)
        for r in range(n):
            c, T = int(clip_of[r]), tlens[clip_of[r]]
            r_ref, psi_ref = O.ctc_prefix_score(logp[c, :T].double(), r_prev[r : r + 1, :T].double(), last[r : r + 1], None if ids is None else ids[r : r + 1],
                                                step, 0, eos)
            live = psi_ref[0] > -1e9
            assert torch.equal(live, psi[r] > -1e9), (step, r)
            np.testing.assert_allclose(psi[r].numpy()[live.numpy()], psi_ref[0].numpy()[live.numpy()], atol=2e-4, rtol=1e-5)
            rl = r_ref[0] > -1e9
            np.testing.assert_allclose(r_new[r, :, :T].numpy()[rl.numpy()], r_ref[0].numpy()[rl.numpy()], atol=5e-4, rtol=1e-5)
            assert bool((r_new[r, :, :T][~rl] < -1e9).all()) and bool((r_new[r, :, T:] == O.CTC_LOGZERO).all())
            nxt[r, :T] = r_ref[0, j[r]].float()
        r_prev = nxt
        last = (j if ids is None else ids[torch.arange(n), j]).long()


@pytest.mark.parametrize("T,V,n,S", [(1, 41, 2, None), (9, 41, 3, 7), (9, 41, 3, None)])
def test_ctc_prefix_clips_one_clip_equals_the_single_clip_entry_point(dev, T, V, n, S):
    """svsr_ctc_prefix_score launches the kernel without its two tables (every hypothesis in clip 0, Tmax frames); the same rows as one clip
    padded to T + 5 frames with NaN, through clip_of and tlen, must give the same bits, and -1e10 in the padding of the new state."""
    from oracle import lrs_oracle as O
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(1000 * T + V + n)
    Tmax, eos = T + 5, V - 1
    logp = torch.full((1, Tmax, V), float("nan"))
    logp[0, :T] = torch.log_softmax(2.0 * torch.randn(T, V, generator=g), dim=-1)
    r_prev = torch.full((n, Tmax, 2), float("nan"))
    r_prev[:, :T, 0] = O.CTC_LOGZERO
    r_prev[:, :T, 1] = torch.cumsum(logp[0, :T, 0], 0)
    last = torch.randint(1, V - 1, (n,), generator=g)
    ids = None if S is None else torch.stack([torch.randperm(V, generator=g)[:S] for _ in range(n)])
    if ids is not None:
        ids[0, 0] = last[0]                                  # (with S = None every row meets its own last label among the V candidates)
    ids_d = None if ids is None else ids.to(dev)
    tl = torch.tensor([T], dtype=torch.int32, device=dev)
    clip_of = torch.zeros(n, dtype=torch.int32, device=dev)
    for out_len in (0, 1, 3):
        r_one, psi_one = ops.ctc_prefix_score(logp[0, :T].to(dev).contiguous(), r_prev[:, :T].to(dev).contiguous(), last.to(dev), ids_d, out_len, 0, eos)
        r_pad, psi_pad = ops.ctc_prefix_score_clips(logp.to(dev), tl, r_prev.to(dev), last.to(dev), ids_d, clip_of, out_len, 0, eos)
        torch.cuda.synchronize()
        assert r_one.shape == (n, S or V, T, 2) and r_pad.shape == (n, S or V, Tmax, 2)
        assert torch.equal(psi_one, psi_pad), out_len
        assert torch.equal(r_one, r_pad[:, :, :T]), out_len
        assert bool((r_pad[:, :, T:] == O.CTC_LOGZERO).all()), out_len



def _ctc_clip_inputs(g, tlens, V, clip_of, Tmax=None, out_len=0):
    """logp [C, Tmax, V] and r_prev [n, Tmax, 2] with NaN wherever a clip has no frame (and in every row without a clip); the state of a live
    row is finite in both columns — so the "same label" branch (phi = r_b) differs from the other (phi = logaddexp(r_n, r_b)) — and -1e10
    before frame out_len - 1, as a prefix of out_len labels leaves it."""
    from oracle import lrs_oracle as O

    C, Tmax = len(tlens), Tmax or max(tlens)
    logp = torch.full((C, Tmax, V), float("nan"))
    for c, T in enumerate(tlens):
        logp[c, :T] = torch.log_softmax(2.0 * torch.randn(T, V, generator=g), dim=-1)
    r_prev = torch.full((len(clip_of), Tmax, 2), float("nan"))
    for r, c in enumerate(clip_of):
        if 0 <= c < C:
            r_prev[r, : tlens[c]] = -5.0 * torch.rand(tlens[c], 2, generator=g) - 0.1 * torch.arange(tlens[c]).view(-1, 1)
            r_prev[r, : min(max(out_len - 1, 0), tlens[c])] = O.CTC_LOGZERO
    return logp, r_prev


def _ctc_row_matches_oracle(r_new_r, psi_r, logp_c, r_prev_r, last_r, ids_r, out_len, eos, T, where):
    """one hypothesis (r_new_r [S, Tmax, 2], psi_r [S]) under the criteria of test_ctc_prefix_clips_kernel_matches_restatement_per_clip"""
    from oracle import lrs_oracle as O

    r_ref, psi_ref = O.ctc_prefix_score(logp_c[:T].double(), r_prev_r[None, :T].double(), torch.tensor([int(last_r)]), None if ids_r is None else ids_r[None],
                                        out_len, 0, eos)
    live = psi_ref[0] > -1e9
    assert torch.equal(live, psi_r > -1e9), where
    np.testing.assert_allclose(psi_r.numpy()[live.numpy()], psi_ref[0].numpy()[live.numpy()], atol=2e-4, rtol=1e-5, err_msg=str(where))
    rl = r_ref[0] > -1e9
    np.testing.assert_allclose(r_new_r[:, :T].numpy()[rl.numpy()], r_ref[0].numpy()[rl.numpy()], atol=5e-4, rtol=1e-5, err_msg=str(where))
    assert bool((r_new_r[:, :T][~rl] < -1e9).all()) and bool((r_new_r[:, T:] == O.CTC_LOGZERO).all()), where
    return psi_ref[0]


@pytest.mark.parametrize("S", [None, 7])
def test_ctc_prefix_clips_rows_without_frames_and_a_length_above_tmax(dev, S):
    """Clips of 9, 0 and 5 frames, two rows each, one row of clip -1 and one of clip C: the rows of the empty clip and the two stray rows are
    -1e10 throughout (their logp and r_prev are NaN), the others match the oracle; the same launch with tlen[0] = Tmax + 3 gives the same bits."""
    from oracle import lrs_oracle as O
    from syncvsr_amd import ops

    tlens, V, eos = (9, 0, 5), 41, 40
    clip_of = [0, 0, 1, 1, 2, 2, -1, 3]
    n, Tmax = len(clip_of), 9
    for out_len in (0, 2):
        g = torch.Generator().manual_seed(500 + out_len + (S or 0))
        logp, r_prev = _ctc_clip_inputs(g, tlens, V, clip_of, out_len=out_len)
        last = torch.randint(1, V - 1, (n,), generator=g)
        ids = None if S is None else torch.stack([torch.randperm(V, generator=g)[:S] for _ in range(n)])
        if ids is not None:
            ids[:, 0] = last
            ids[0, 1], ids[4, 1] = eos, 0
        ids_d = None if ids is None else ids.to(dev)
        out = []
        for t0 in (Tmax, Tmax + 3):
            tl = torch.tensor([t0, 0, 5], dtype=torch.int32, device=dev)
            out.append(ops.ctc_prefix_score_clips(logp.to(dev), tl, r_prev.to(dev), last.to(dev), ids_d, torch.tensor(clip_of, dtype=torch.int32, device=dev),
                                                  out_len, 0, eos))
        torch.cuda.synchronize()
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), "tlen = Tmax + 3 must behave as Tmax"
        r_new, psi = out[1][0].cpu(), out[1][1].cpu()
        assert r_new.shape == (n, S or V, Tmax, 2)
        for r, c in enumerate(clip_of):
            if not 0 <= c < 3 or tlens[c] == 0:
                assert bool((r_new[r] == O.CTC_LOGZERO).all()) and bool((psi[r] == O.CTC_LOGZERO).all()), (out_len, r)
            else:
                _ctc_row_matches_oracle(r_new[r], psi[r], logp[c], r_prev[r], last[r], None if ids is None else ids[r], out_len, eos, tlens[c], (out_len, r))


def test_ctc_prefix_clips_candidate_ids_and_last_labels_outside_the_vocabulary(dev):
    """-1, V, 2^31 and 2^32 + 5 as candidates are impossible extensions (-1e10, nothing read), whatever their low 32 bits say; the other
    columns keep the bits of a launch with valid ids in those places.  A last label of 2^32 + 7 is not label 7: the row scores candidate 7
    as any other label (the oracle with last = -1)."""
    from oracle import lrs_oracle as O
    from syncvsr_amd import ops

    tlens, V, eos, S = (9, 5), 41, 40, 7
    clip_of = [0, 0, 1, 1]
    n = len(clip_of)
    for out_len in (0, 2):
        g = torch.Generator().manual_seed(600 + out_len)
        logp, r_prev = _ctc_clip_inputs(g, tlens, V, clip_of, out_len=out_len)
        last = torch.randint(1, V - 1, (n,), generator=g)
        ids = torch.stack([torch.randperm(V, generator=g)[:S] for _ in range(n)])
        ids[1, 4] = last[1]                                    # a true "same label" pair stays one
        ids[2, 5] = 7
        last[2] = 2 ** 32 + 7
        bad = ids.clone()
        bad[:, :4] = torch.tensor([-1, V, 2 ** 31, 2 ** 32 + 5])
        tl = torch.tensor(tlens, dtype=torch.int32, device=dev)
        cl = torch.tensor(clip_of, dtype=torch.int32, device=dev)
        r_ok, psi_ok = ops.ctc_prefix_score_clips(logp.to(dev), tl, r_prev.to(dev), last.to(dev), ids.to(dev), cl, out_len, 0, eos)
        r_bad, psi_bad = ops.ctc_prefix_score_clips(logp.to(dev), tl, r_prev.to(dev), last.to(dev), bad.to(dev), cl, out_len, 0, eos)
        torch.cuda.synchronize()
        r_ok, psi_ok, r_bad, psi_bad = r_ok.cpu(), psi_ok.cpu(), r_bad.cpu(), psi_bad.cpu()
        for j in range(4):
            assert bool((psi_bad[:, j] == O.CTC_LOGZERO).all()) and bool((r_bad[:, j] == O.CTC_LOGZERO).all()), (out_len, int(bad[0, j]))
        assert torch.equal(_bits(psi_bad[:, 4:]), _bits(psi_ok[:, 4:])) and torch.equal(_bits(r_bad[:, 4:]), _bits(r_ok[:, 4:]))
        ref_last = last.clone()
        ref_last[2] = -1
        for r, c in enumerate(clip_of):
            psi_ref = _ctc_row_matches_oracle(r_ok[r], psi_ok[r], logp[c], r_prev[r], ref_last[r], ids[r], out_len, eos, tlens[c], (out_len, r))
            if r == 2:                                         # the inputs can tell the two branches apart at candidate 7
                other = O.ctc_prefix_score(logp[c, : tlens[c]].double(), r_prev[r : r + 1, : tlens[c]].double(), torch.tensor([7]), ids[r : r + 1], out_len, 0, eos)[1][0]
                assert abs(float(other[5] - psi_ref[5])) > 1e-2


@pytest.mark.parametrize("T,out_len", [(5, 4), (5, 5), (1, 0), (1, 1)])
@pytest.mark.parametrize("S", [None, 7])
def test_ctc_prefix_clips_prefix_as_long_as_the_clip(dev, T, out_len, S):
    """out_len = T - 1 and T: the frame loop runs once or not at all.  Against the oracle; with out_len = T every label but eos is -1e10 and
    eos is logaddexp of r_prev at the last frame."""
    from oracle import lrs_oracle as O
    from syncvsr_amd import ops

    V, eos, n, Tmax = 41, 40, 3, T + 2
    g = torch.Generator().manual_seed(700 + 10 * T + out_len + (S or 0))
    logp, r_prev = _ctc_clip_inputs(g, (T,), V, [0] * n, Tmax=Tmax, out_len=out_len)
    last = torch.randint(1, V - 1, (n,), generator=g)
    ids = None if S is None else torch.stack([torch.randperm(V - 1, generator=g)[:S] for _ in range(n)])
    if ids is not None:
        ids[:, 0] = last
        ids[0, 1], ids[1, 2] = eos, 0
    r_new, psi = ops.ctc_prefix_score_clips(logp.to(dev), torch.tensor([T], dtype=torch.int32, device=dev), r_prev.to(dev), last.to(dev),
                                            None if ids is None else ids.to(dev), torch.zeros(n, dtype=torch.int32, device=dev), out_len, 0, eos)
    torch.cuda.synchronize()
    r_new, psi = r_new.cpu(), psi.cpu()
    assert bool(torch.isfinite(r_new).all()) and bool(torch.isfinite(psi).all())
    for r in range(n):
        _ctc_row_matches_oracle(r_new[r], psi[r], logp[0], r_prev[r], last[r], None if ids is None else ids[r], out_len, eos, T, (T, out_len, r))
        if out_len == T:
            lab = torch.arange(V) if ids is None else ids[r]
            assert bool((psi[r][lab != eos] == O.CTC_LOGZERO).all())
            want = float(torch.logaddexp(r_prev[r, T - 1, 0].double(), r_prev[r, T - 1, 1].double()))
            assert bool(((psi[r][lab == eos] - want).abs() <= 2e-4 + 1e-5 * abs(want)).all())
    assert out_len != T or S is not None or int((psi > -1e9).sum()) == n                       # (every row met eos among the V candidates)



# ----------------------------------------------------------------------------------------------------------------------
# svsr_mha_src_step_fwd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.SRC_STEP_SHAPES))
def test_mha_src_step_kernel_equals_its_fp64_statement(dev, name):
    """tests/search_cases.py SRC_STEP_SHAPES: clips of 1 to 150 frames (one to three chunks of 64 keys, partial last chunks of 1, 2 and 22
    keys), peak keys at the first and last frame and on both sides of the first chunk boundary, rows without a clip, a clip without frames, a
    length above Tmax, 45 waves (the last workgroup holds one), q a column slice of a [n, 3D] tensor, kv rows of 2D + 8 with NaN in every
    frame and column that is not the clip's.  Elementwise |got - want| <= 2^-8 |want| + 2^-10 A against the fp64 statement (A = sum_k p_k
    |v_k|): two half-ulps of the bf16 result, and the fp32 error of scores and exp; tests/test_search_cases_cpu.py shows an fp32 restatement
    of the kernel at 0.68 / 0.71 of this bound (t150 / t130) and two wrong ones hundreds of times above it.  Rows without keys are exact
    zeros.  Written into a column slice of a wider tensor, the same bits arrive and the columns beside them keep theirs."""
    from syncvsr_amd import ops

    case, want, A = SC.src_step_shape(name)
    H, Tmax, D, n = case["H"], case["Tmax"], case["H"] * 64, len(case["clip_of"])
    q = case["q_wide"].to(dev)[:, D : 2 * D]
    kv = case["kv"].to(dev)
    assert q.stride(0) == 3 * D and kv.stride(0) == 2 * D + 8
    clip_of = torch.tensor(case["clip_of"], dtype=torch.int32, device=dev)
    tlen = torch.tensor(case["tlens"], dtype=torch.int32, device=dev)
    got = ops.mha_src_step_fwd(q, kv, clip_of, tlen, Tmax=Tmax, H=H, scale=case["scale"])
    wide = torch.full((n, D + 24), 7.0, dtype=torch.bfloat16, device=dev)
    ret = ops.mha_src_step_fwd(q, kv, clip_of, tlen, Tmax=Tmax, H=H, scale=case["scale"], out=wide[:, 8 : 8 + D])
    torch.cuda.synchronize()
    assert got.shape == (n, D) and got.dtype == torch.bfloat16 and ret.data_ptr() == wide[:, 8:].data_ptr()
    got, wide = got.cpu(), wide.cpu()
    assert bool(torch.isfinite(got.float()).all())
    for r in SC.src_step_dead_rows(case):
        assert not got[r].any(), r
    ratio = SC.src_step_ratio(got, want, A)
    print(f"{name}: H {H} Tmax {Tmax} rows {n}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(_bits(wide[:, 8 : 8 + D].contiguous()), _bits(got))
    assert bool((wide[:, :8] == 7.0).all()) and bool((wide[:, 8 + D :] == 7.0).all())


def test_mha_src_step_rejects_pitches_and_alignment_it_cannot_load(dev):
    from syncvsr_amd import _lib, ops

    H, D, Tmax, n = 1, 64, 4, 2
    i32 = dict(dtype=torch.int32, device=dev)
    clip_of, tlen = torch.zeros(n, **i32), torch.tensor([Tmax], **i32)
    bf = dict(dtype=torch.bfloat16, device=dev)
    q, kv = torch.zeros(n, 3 * D, **bf), torch.zeros(Tmax, 2 * D, **bf)
    ops.mha_src_step_fwd(q[:, :D], kv, clip_of, tlen, Tmax=Tmax, H=H)                       # (the well-formed call is taken)
    with pytest.raises(_lib.SvsrError):
        ops.mha_src_step_fwd(torch.zeros(n, 3 * D + 4, **bf)[:, :D], kv, clip_of, tlen, Tmax=Tmax, H=H)        # q_pitch % 8 != 0
    with pytest.raises(_lib.SvsrError):
        ops.mha_src_step_fwd(q[:, :D], torch.zeros(Tmax, 2 * D - 8, **bf), clip_of, tlen, Tmax=Tmax, H=H)       # kv_pitch < 2 * H * 64
    with pytest.raises(_lib.SvsrError):
        ops.mha_src_step_fwd(q[:, 4 : 4 + D], kv, clip_of, tlen, Tmax=Tmax, H=H)                                # q 8 bytes off a 16-byte boundary
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# the searches
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dev):
    from syncvsr_amd.lrs_model import E2E

    args, odim, sd, clip, runs, gold = build_lrs_infer_case("lrs_infer_tiny")
    model = E2E(odim, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    return model, args, odim, sd, clip, runs, gold


def _derived(enc, seed=17):
    """The clips of tests/test_lrs_search_clips_cpu.py: the golden encoder output, a truncation, two seeded perturbations (one truncated)."""
    g = torch.Generator().manual_seed(seed)
    T = enc.shape[0]
    a = enc + 0.5 * torch.randn(enc.shape, generator=g, dtype=torch.float64).to(enc.dtype)
    b = enc.flip(0) + 0.8 * torch.randn(enc.shape, generator=g, dtype=torch.float64).to(enc.dtype)
    return [enc, enc[: (9 * T) // 16], a, b[: (5 * T) // 16]]


def _pad(clips):
    lens = [c.shape[0] for c in clips]
    xs = torch.full((len(clips), max(lens), clips[0].shape[1]), 3.0, dtype=clips[0].dtype)         # (padding that would show if it were read)
    for i, c in enumerate(clips):
        xs[i, : lens[i]] = c
    return xs, lens


def test_decoder_step_with_per_row_clips_equals_the_single_clip_step(dev, tiny):
    """Seven positions, rows re-ordered and dropped like the search does: the clip-aware step against `forward_one_step` on each clip's own
    rows and unpadded memory, within the 3e-2 test_decoder_cache_steps_equal_prefix_recomputation allows between batch shapes."""
    model, args, odim, sd, clip, runs, gold = tiny
    sc = model.decoder._scorer()
    clips = _derived(torch.from_numpy(gold["enc_feat"]))
    xs, lens = _pad(clips)
    sc.batch_init_state_clips(xs.to(dev), lens)
    g = torch.Generator().manual_seed(2)
    clip_of = torch.tensor([0, 0, 0, 1, 2, 2, 3, 3, 3, 3], dtype=torch.int32, device=dev)
    n = clip_of.numel()
    ys = torch.full((n, 1), odim - 1, dtype=torch.int64, device=dev)
    states = None
    for step in range(7):
        logp, states = sc.batch_score_clips(ys, states, clip_of)
        assert logp.shape == (n, odim) and states[0].shape == (n, ys.shape[1], 3 * model.ddim)
        for c in range(4):
            rows = torch.nonzero(clip_of == c).view(-1)
            if rows.numel() == 0:
                continue
            mem = clips[c].to(dev).unsqueeze(0).expand(rows.numel(), -1, -1)
            want, _ = sc.forward_one_step(ys[rows], None, mem, cache=None)
            err = float((logp[rows] - want).abs().max())
            assert err <= 3e-2, (step, c, err)
        tok = torch.where(torch.arange(n, device=dev) % 2 == 0, logp.argmax(-1), torch.randint(0, odim - 1, (n,), generator=g).to(dev))
        prev = torch.arange(n, device=dev)
        if step == 2:
            prev = torch.tensor([1, 0, 0, 4, 5, 8, 6], device=dev)              # clip 1 leaves, rows of the others are re-ordered inside their clip
        ys = torch.cat((ys[prev], tok[prev].unsqueeze(1)), dim=1)
        states = sc.select_states(states, prev, tok[prev])
        clip_of = clip_of[prev].contiguous()
        n = prev.numel()
    with pytest.raises(ValueError, match="ddim"):
        sc.batch_init_state_clips(xs[:, :, :-1].to(dev), lens)


def _rescore(sd, args, odim, enc, yseq, ctcw, maxlen, lm_ref=None, lmw=0.0):
    """Scores of one hypothesis under the fp64 scorers, accumulated along its own path (tests/test_gpu_lrs_infer.py, test_gpu_lrs_lm.py)."""
    from oracle import lrs_oracle as O

    dec, ctc = O.OracleDecoderScorer(sd, args), O.make_oracle_ctc_scorer(sd, odim - 1)
    ctc.batch_init_state(enc)
    y = torch.tensor([yseq[:1]])
    state, tot = None, dict(decoder=0.0, ctc=0.0, lm=0.0)
    for tok in yseq[1 : 1 + maxlen]:                      # a closing <eos> forced at the length limit is not scored
        d, _ = dec.batch_score(y, [None], enc.unsqueeze(0))
        c, pend = ctc.batch_score_partial(y, None, state, enc)
        tot["decoder"] += float(d[0, tok])
        tot["ctc"] += float(c[0, tok])
        if lmw != 0:
            tot["lm"] += float(lm_ref.batch_score(y, None, None)[0][0, tok])
        state = ctc.select_states(pend, torch.tensor([0]), torch.tensor([tok]))
        y = torch.cat((y, torch.tensor([[tok]])), dim=1)
    return (1 - ctcw) * tot["decoder"] + ctcw * tot["ctc"] + lmw * tot["lm"], tot


def _reference_search(sd64, args, odim, x64, beam, ctcw, lm_ref=None, lmw=0.0):
    """The single-clip statement of the search (tests/search_cases.py) under the fp64 scorers (tests/test_lrs_search_clips_cpu.py ties it to
    the reference's own n-best)."""
    from oracle import lrs_oracle as O
    from syncvsr_amd.lrs_infer import get_beam_search_decoder

    class _M:
        pass

    m = _M()
    m.odim = odim
    bs = get_beam_search_decoder(m, [f"t{i}" for i in range(odim)], ctc_weight=ctcw, beam_size=beam,
                                 scorers=dict(decoder=O.OracleDecoderScorer(sd64, args), ctc=O.make_oracle_ctc_scorer(sd64, odim - 1)))
    return SC.single_clip_search(bs, x64)


def _check_clip(nbest, ref, sd64, args, odim, x64, beam, ctcw, where, margin=0.05, lm_ref=None, lmw=0.0):
    """The per-clip criteria of test_beam_search_on_the_gpu_finds_the_reference_hypotheses."""
    want, gs = ref[0].yseq.tolist(), [h.score for h in ref]
    second = gs[1] if len(gs) > 1 else -1e30
    print(f"{where}: hip best {nbest[0].yseq.tolist()} {nbest[0].score:.4f} | reference {want} {gs[0]:.4f} (2nd {second:.4f})")
    if gs[0] - second > 0.2 and beam >= 5:
        assert nbest[0].yseq.tolist() == want, (where, nbest[0].yseq.tolist(), want)
        assert abs(nbest[0].score - gs[0]) <= 2e-2 * abs(gs[0]) + 0.05
    else:
        assert nbest[0].score >= gs[0] - margin * abs(gs[0])
    for h in nbest[:3]:
        tot, parts = _rescore(sd64, args, odim, x64, h.yseq.tolist(), ctcw, x64.shape[0], lm_ref, lmw)
        d = h.asdict()
        assert abs(d["score"] - tot) <= 2e-2 * abs(tot) + 0.05, (where, d, tot)
        for k in ("decoder", "ctc") + (("lm",) if lmw != 0 else ()):
            assert abs(d["scores"][k] - parts[k]) <= 2e-2 * abs(parts[k]) + 0.05, (where, k, d, parts)
    assert all(nbest[i].score >= nbest[i + 1].score for i in range(len(nbest) - 1))
    assert all(h.yseq[0] == odim - 1 and h.yseq[-1] == odim - 1 for h in nbest)


def _no_boundary_ties(monkeypatch):
    """torch.topk stays for the pre-beam: only the SET of candidates reaches the search (the CTC scorer scatters them into a full plane),
    so its tie order could change a result only through a tie between the last candidate kept and the first one left out."""
    inner = torch.topk
    seen = []

    def topk(x, k, dim=-1, *a, **kw):
        if x.dim() == 2 and k < x.shape[-1]:
            v = inner(x, k + 1, dim=dim)[0]
            assert bool((v[:, k - 1] > v[:, k]).all()), "a tie at the pre-beam boundary: torch.topk's tie order would matter on these inputs"
            seen.append(x.shape[0])
        return inner(x, k, dim, *a, **kw)

    monkeypatch.setattr(torch, "topk", topk)
    return seen


def test_forward_clips_tiny_model_four_clips(dev, tiny, monkeypatch):
    from syncvsr_amd.lrs_infer import get_beam_search_decoder

    model, args, odim, sd, clip, runs, gold = tiny
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    tokens = [f"t{i}" for i in range(odim)]
    clips = _derived(torch.from_numpy(gold["enc_feat"]))
    xs, lens = _pad(clips)
    seen = _no_boundary_ties(monkeypatch)
    for r, (beam, ctcw) in enumerate(runs):
        bs = get_beam_search_decoder(model, tokens, ctc_weight=ctcw, beam_size=beam)
        got = bs.forward_clips(xs.to(dev), torch.tensor(lens))
        again = bs.forward_clips(xs.to(dev), lens)
        assert len(got) == 4
        for c in range(4):
            ref = _reference_search(sd64, args, odim, clips[c].double(), beam, ctcw)
            _check_clip(got[c], ref, sd64, args, odim, clips[c].double(), beam, ctcw, f"run{r} clip{c}")
            assert [h.asdict() for h in got[c]] == [h.asdict() for h in again[c]]                  # run to run
        gy = gold[f"run{r}.yseq"]                                                                    # clip 0 is the reference's own clip
        if gold[f"run{r}.score"][0] - gold[f"run{r}.score"][1] > 0.2 and beam >= 5:
            assert got[0][0].yseq.tolist() == gy[0][gy[0] >= 0].tolist()
        # one clip through forward_clips is the search `forward` runs: same hypotheses, scores within the bound between batch shapes
        one = bs.forward_clips(clips[1].unsqueeze(0).to(dev), [lens[1]])[0]
        single = bs.forward(clips[1].to(dev))
        assert one[0].yseq.tolist() == single[0].yseq.tolist() and abs(one[0].score - single[0].score) <= 2e-2 * abs(single[0].score) + 0.05
    assert seen, "the pre-beam never ran"
    with pytest.raises(ValueError, match="lengths"):
        bs.forward_clips(xs.to(dev), [lens[0] + 1] + lens[1:])
    # clips -> encoder -> search (decode_clips), against the search on the encoder output of the clip alone
    from syncvsr_amd.lrs_infer import decode_clips

    bs = get_beam_search_decoder(model, tokens, ctc_weight=0.1, beam_size=30)
    T = clip.shape[0]
    batch = torch.zeros(2, T, *clip.shape[1:])
    batch[0], batch[1, : T - 5] = clip, clip[: T - 5]
    out = decode_clips(model, bs, batch.to(dev), [T, T - 5])
    gy = gold["run1.yseq"]
    assert out[0][0].yseq.tolist() == gy[0][gy[0] >= 0].tolist()
    assert abs(out[0][0].score - gold["run1.score"][0]) <= 0.05 * abs(gold["run1.score"][0])
    enc1, _ = model.encoder(clip[: T - 5].unsqueeze(0).to(dev), None)
    alone = bs.forward(enc1.squeeze(0))
    assert abs(out[1][0].score - alone[0].score) <= 0.05 * abs(alone[0].score) and len(out[1][0].yseq) <= T - 5 + 2


def test_forward_clips_shipped_model_beside_two_shorter_clips(dev):
    """The 252 M-parameter model, 5,049 units, beam 40, CTC weight 0.1: the golden clip as clip 0 beside two shorter derived clips.  Clip 0
    under test_shipped_model_with_the_reference_search_settings' criteria; every clip's reported scores equal the fp64 re-scoring."""
    from syncvsr_amd.lrs_infer import get_beam_search_decoder
    from syncvsr_amd.lrs_model import E2E

    args, odim, sd, clip, runs, gold = build_lrs_infer_case("lrs_infer_full")
    model = E2E(odim, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    g_enc = torch.from_numpy(gold["enc_feat"])
    d = _derived(g_enc, seed=23)
    clips = [g_enc, d[1], d[3]]
    xs, lens = _pad(clips)
    beam, ctcw = runs[0]
    bs = get_beam_search_decoder(model, [f"t{i}" for i in range(odim)], ctc_weight=ctcw, beam_size=beam)
    got = bs.forward_clips(xs.to(dev), lens)
    gs = gold["run0.score"]
    print(f"clip 0: hip best {got[0][0].score:.4f} ({len(got[0][0].yseq)} tokens) | reference {gs[0]:.4f} (2nd {gs[1]:.4f})")
    assert got[0][0].score >= gs[0] - 0.02 * abs(gs[0])
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    for c in range(3):
        tot, parts = _rescore(sd64, args, odim, clips[c].double(), got[c][0].yseq.tolist(), ctcw, lens[c])
        h = got[c][0].asdict()
        print(f"clip {c}: {h['score']:.4f} (fp64 {tot:.4f})")
        assert abs(h["score"] - tot) <= 2e-2 * abs(tot) + 0.05, (c, h["score"], tot)
        assert abs(h["scores"]["decoder"] - parts["decoder"]) <= 2e-2 * abs(parts["decoder"]) + 0.05
        assert abs(h["scores"]["ctc"] - parts["ctc"]) <= 2e-2 * abs(parts["ctc"]) + 0.05
        single = bs.forward(clips[c].to(dev))
        assert got[c][0].score >= single[0].score - 0.02 * abs(single[0].score)


def test_forward_clips_with_the_language_model(dev, tiny):
    """`lrs_lm_tiny`, lm_weight > 0, three clips: per clip the criteria of test_lm_fused_beam_search_finds_the_reference_hypotheses against the
    fp64 single-clip search, and the pool sized for C x beam rows never had to grow."""
    from lm_cases import LM_RUNS, lm_case
    from lm_restatement import LMRestatement
    from syncvsr_amd.lrs_infer import get_beam_search_decoder
    from syncvsr_amd.lrs_lm import LMPool, TransformerLM

    model, args, odim, sd, clip, runs, _ = tiny
    conf, V, lsd, gold = lm_case("lrs_lm_tiny")
    lm = TransformerLM(V, conf)
    lm.load_state_dict(lsd, strict=True)
    lm.to(dev)
    lm_ref = LMRestatement(lsd, conf)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    clips = _derived(torch.from_numpy(gold["enc_feat"]))[:3]
    xs, lens = _pad(clips)
    tokens = [f"t{i}" for i in range(odim)]
    pools = []
    inner = LMPool.__init__

    def spy(self, *a, **k):
        inner(self, *a, **k)
        pools.append(self)

    LMPool.__init__ = spy
    try:
        ran = 0
        for r, (beam, ctcw, lmw) in enumerate(LM_RUNS):
            if lmw == 0:
                continue
            ran += 1
            bs = get_beam_search_decoder(model, tokens, rnnlm=lm, ctc_weight=ctcw, lm_weight=lmw, beam_size=beam)
            del pools[:]
            got = bs.forward_clips(xs.to(dev), lens)
            assert len(pools) == 1 and pools[0].grown == 0 and pools[0].capacity == 3 * beam * (max(lens) + 1), (len(pools), pools[0].grown)
            for c in range(3):
                from oracle import lrs_oracle as O
                from syncvsr_amd.lrs_infer import BatchBeamSearch, LengthBonus

                ref = BatchBeamSearch(beam_size=beam, vocab_size=odim, weights={"decoder": 1 - ctcw, "ctc": ctcw, "lm": lmw, "length_bonus": 0},
                                      scorers=dict(decoder=O.OracleDecoderScorer(sd64, args), ctc=O.make_oracle_ctc_scorer(sd64, odim - 1), lm=lm_ref,
                                                   length_bonus=LengthBonus(odim)), sos=odim - 1, eos=odim - 1, pre_beam_score_key="decoder")
                _check_clip(got[c], SC.single_clip_search(ref, clips[c].double()), sd64, args, odim, clips[c].double(), beam, ctcw, f"lm run{r} clip{c}",
                            lm_ref=lm_ref, lmw=lmw)
                assert "lm" in got[c][0].scores
        assert ran >= 1
    finally:
        LMPool.__init__ = inner


def _to(v, dev):
    if isinstance(v, torch.Tensor):
        return v.to(dev)
    return type(v)(_to(e, dev) for e in v) if isinstance(v, (list, tuple)) else v


class _HostScorer:
    """A CPU scorer of the single-clip protocol behind device tensors: arguments go to the host, scores and states come back to `dev`."""

    def __init__(self, inner, dev):
        self.inner, self.dev = inner, dev

    def batch_init_state(self, x):
        return _to(self.inner.batch_init_state(x.cpu()), self.dev)

    def batch_score(self, ys, states, xs):
        return _to(self.inner.batch_score(ys.cpu(), _to(states, "cpu"), xs.cpu()), self.dev)

    def select_states(self, states, prev, tok):
        return _to(self.inner.select_states(_to(states, "cpu"), prev.cpu(), tok.cpu()), self.dev)


class _HostPartialScorer(_HostScorer):
    def batch_score_partial(self, y, ids, state, x):
        return _to(self.inner.batch_score_partial(y.cpu(), _to(ids, "cpu"), _to(state, "cpu"), x.cpu()), self.dev)


def test_forward_equals_a_one_clip_forward_clips(dev, tiny):
    """`forward(x)` and `forward_clips(x[None], [T])[0]` are the same launches on the same inputs: equal hypotheses, bit-equal scores.  And
    an encoder output that is not fp32 (fp64 on the device, the oracle's scorers behind PerClipScorers) is selected by the torch statement
    instead of being refused, and gives what the single-clip statement of the search gives, to 1e-9."""
    from oracle import lrs_oracle as O
    from syncvsr_amd.lrs_infer import PerClipScorers, get_beam_search_decoder

    model, args, odim, sd, clip, runs, gold = tiny
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    tokens = [f"t{i}" for i in range(odim)]
    x = torch.from_numpy(gold["enc_feat"]).to(dev)
    T = x.shape[0]
    for beam in (4, 5):
        bs = get_beam_search_decoder(model, tokens, ctc_weight=0.1, beam_size=beam)
        one, group = bs(x), bs.forward_clips(x.unsqueeze(0), [T])[0]
        assert one and len(one) == len(group)
        for a, b in zip(one, group):
            assert a.yseq.tolist() == b.yseq.tolist()
            assert a.score == b.score and a.scores == b.scores, (beam, a.asdict(), b.asdict())      # floats compared exactly: the same bits

        class _M:
            pass

        m = _M()
        m.odim = odim
        raw = dict(decoder=_HostScorer(O.OracleDecoderScorer(sd64, args), dev), ctc=_HostPartialScorer(O.make_oracle_ctc_scorer(sd64, odim - 1), dev))
        statement = get_beam_search_decoder(m, tokens, ctc_weight=0.1, beam_size=beam, scorers=raw)
        wrapped = get_beam_search_decoder(m, tokens, ctc_weight=0.1, beam_size=beam, scorers={k: PerClipScorers(v) for k, v in raw.items()})
        assert list(wrapped.part_scorers) == ["ctc"]
        x64 = x.double()
        want = SC.single_clip_search(statement, x64)
        assert want
        for got in (wrapped.forward(x64), statement.forward(x64), wrapped.forward_clips(x64.unsqueeze(0), [T])[0]):
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.yseq.is_cuda and g.yseq.tolist() == w.yseq.tolist()
                assert abs(g.score - w.score) <= 1e-9 and set(g.scores) == set(w.scores)
                assert all(abs(g.scores[k] - w.scores[k]) <= 1e-9 for k in w.scores), (beam, g.asdict(), w.asdict())
