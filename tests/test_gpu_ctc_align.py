"""CTC forced alignment on the GPU (-m gpu): svsr_ctc_align against the reference's own outputs (tests/golden/ctc_align.npz) and against the
numpy restatement (tests/ctc_align_restatement.py), then the surface built on it (E2E.ctc.forced_align_batch / forced_align,
lrs_align.align_clips).  Every comparison is exact: frames and spans equal, scores equal bit for bit — the kernel does the reference's
comparisons in the reference's order and one fp32 add per cell, so there is nothing to be close about."""
import os

import numpy as np
import pytest
import torch

from ctc_align_restatement import align_batch, collapse, frames_needed
from golden_cases import build_lrs_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ctc_align.npz")
NEG = -np.inf


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _logp(seed, B, T, V, gain=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, V, generator=g) * gain, dim=-1).contiguous()


def _labels(rows, Lmax=None):
    Lmax = Lmax or max(len(r) for r in rows)
    out = torch.full((len(rows), Lmax), -1, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, : len(r)] = torch.tensor(r, dtype=torch.int64)
    return out


def _check(dev, logp, tlen, labels, blank=0, V=None):
    """One launch against the restatement on the same numbers: frames, spans equal, scores bit-equal.  -> the expectation."""
    from syncvsr_amd import ops

    lp = logp if V is None else logp[..., :V]
    want = align_batch(lp.numpy(), tlen, labels.numpy(), blank)
    got = ops.ctc_align(logp.to(dev), torch.tensor(tlen, dtype=torch.int32, device=dev), labels.to(dev), blank, V=V)
    frames, spans, score = (t.cpu().numpy() for t in got)
    assert frames.dtype == np.int32 and spans.dtype == np.int32 and score.dtype == np.float32
    assert np.array_equal(frames, want[0]), (frames, want[0])
    assert np.array_equal(spans, want[1]), (spans, want[1])
    assert np.array_equal(score.view(np.int32), want[2].view(np.int32)), (score, want[2])
    return want


def _infeasible(want, b):
    return want[2][b] == NEG and (want[0][b] == -1).all() and (want[1][b] == -1).all()


def _spells(want, b, tlen, y, blank=0):
    return np.isfinite(want[2][b]) and collapse(want[0][b, : tlen[b]], blank) == list(y) and (want[0][b, tlen[b] :] == -1).all()


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------
def test_kernel_equals_the_reference_on_every_recorded_clip(dev):
    """V = 41, ragged batches of 1-4 clips, Tmax 3-39, Lmax 1-6, labels from five units (repeats are frequent): what the reference's
    forced_align_batch returned for the torch fp32 log_softmax of the stored activations."""
    gold = np.load(GOLD, allow_pickle=False)
    clips = 0
    for i in range(int(gold["n_batches"])):
        hs, ys, ilens, ali = (gold[f"b{i}.{k}"] for k in ("hs", "ys", "ilens", "ali"))
        lp = torch.log_softmax(torch.from_numpy(hs), dim=-1).transpose(0, 1).contiguous()
        want = _check(dev, lp, [int(t) for t in ilens], torch.from_numpy(ys))
        for b in gold[f"b{i}.clips"]:
            assert np.array_equal(want[0][b], ali[b]), (i, b)                   # (both -1 beyond ilens[b])
            clips += 1
    assert clips >= 40


def test_kernel_more_states_than_threads(dev):
    """L = 130: S = 261 states over 256 threads, T = 160; the batch-mate has one label."""
    g = torch.Generator().manual_seed(5)
    y = torch.randint(1, 41, (130,), generator=g).tolist()
    y[40], y[99] = y[39], y[98]                                                  # (two repeats for certain)
    assert frames_needed(y) <= 160
    tlen = [160, 97]
    want = _check(dev, _logp(6, 2, 160, 41), tlen, _labels([y, [17]]))
    assert _spells(want, 0, tlen, y) and _spells(want, 1, tlen, [17])
    assert (want[1][1, 1:] == -1).all() and want[1][0, 129, 1] >= 129


def test_kernel_tight_cases(dev):
    """T = 1 with L = 1; T exactly L + repeats (one path); one frame less (none): -inf, -1 everywhere, the neighbours untouched."""
    y = [3, 3, 7, 9, 9, 9]
    need = frames_needed(y)
    assert need == 9
    rows = [[5], y, y, [4, 8], y]
    tlen = [1, need, need - 1, need + 2, need + 1]
    want = _check(dev, _logp(7, 5, need + 2, 41), tlen, _labels(rows))
    assert want[0][0].tolist() == [5] + [-1] * (need + 1) and want[1][0, 0].tolist() == [0, 0]
    assert want[0][1, :need].tolist() == [3, 0, 3, 7, 9, 0, 9, 0, 9]
    assert _infeasible(want, 2)
    assert _spells(want, 3, tlen, [4, 8]) and _spells(want, 4, tlen, y)
    alone = _check(dev, _logp(7, 5, need + 2, 41)[3:4].contiguous(), tlen[3:4], _labels(rows)[3:4])
    assert np.array_equal(alone[0][0], want[0][3]) and alone[2][0] == want[2][3]


def test_kernel_all_equal_posteriors_every_comparison_a_tie(dev):
    """Every candidate ties: 'stay' wins every cell that has a finite 'stay', and S - 2 the end."""
    V, T = 41, 12
    logp = torch.full((4, T, V), float(-np.log(np.float32(V))), dtype=torch.float32)
    rows = [[3, 3, 7], [3, 3, 3], [5], [2, 4, 6, 8]]
    tlen = [12, 9, 12, 4]
    want = _check(dev, logp, tlen, _labels(rows))
    for b, y in enumerate(rows):
        assert _spells(want, b, tlen, y)
    assert want[0][2, :12].tolist() == [5] * 12                                  # starts in the label (1 beats nothing, stays), ends in S - 2
    assert want[0][0, :12].tolist() == [3, 0, 3] + [7] * 9                       # a state is entered the first frame it can be, then kept
    assert want[0][3, :4].tolist() == [2, 4, 6, 8]


def test_kernel_repeated_labels_aab_and_aaa(dev):
    rows = [[4, 4, 9], [4, 4, 4], [4, 4, 9], [4, 4, 4]]
    tlen = [11, 11, 4, 5]
    want = _check(dev, _logp(8, 4, 11, 41, gain=1.0), tlen, _labels(rows))
    for b, y in enumerate(rows):
        assert _spells(want, b, tlen, y)
        sp = want[1][b]
        assert (sp[1:, 0] > sp[:-1, 1] + (np.array(y[1:]) == np.array(y[:-1]))).all()          # a blank between equal neighbours


def test_kernel_columns_at_minus_infinity(dev):
    """Whole columns of -inf: a transcript label's (no path: infeasible, not NaN), the blank's (a path only without repeats and without
    spare frames), and columns the transcript does not use (nothing changes)."""
    logp = _logp(9, 4, 8, 41)
    logp[0, :, 6] = NEG                       # a label of clip 0
    logp[1, :, 0] = NEG                       # the blank: [5, 6, 7] over 8 frames still has paths without blanks
    logp[2, :, 0] = NEG                       # the blank, and the transcript needs one
    logp[3, :, 10:30] = NEG                   # nobody's
    rows = [[5, 6, 7], [5, 6, 7], [5, 5, 7], [5, 6, 7]]
    tlen = [8, 8, 8, 7]
    want = _check(dev, logp, tlen, _labels(rows))
    assert _infeasible(want, 0) and _infeasible(want, 2)
    assert _spells(want, 1, tlen, rows[1]) and 0 not in want[0][1, :8]
    assert _spells(want, 3, tlen, rows[3])
    assert not np.isnan(want[2]).any()


def test_kernel_blank_is_the_last_unit(dev):
    rows = [[0, 0, 7], [12], [3, 39, 3]]
    tlen = [10, 6, 10]
    want = _check(dev, _logp(10, 3, 10, 41), tlen, _labels(rows), blank=40)
    for b, y in enumerate(rows):
        assert _spells(want, b, tlen, y, blank=40)
    bad = _check(dev, _logp(10, 3, 10, 41), tlen, _labels([[0, 0, 7], [40], [3, 39, 3]]), blank=40)        # the blank as a label
    assert _infeasible(bad, 1) and np.array_equal(bad[0][0], want[0][0]) and np.array_equal(bad[0][2], want[0][2])


def test_kernel_pitch_padding_and_frames_beyond_the_length_are_never_read(dev):
    """ldp = 64 for V = 41 with NaN in the padding columns, and NaN rows beyond every clip's length."""
    V = 41
    logp = torch.full((3, 14, 64), float("nan"))
    logp[..., :V] = _logp(11, 3, 14, V)
    tlen = [14, 9, 5]
    for b, t in enumerate(tlen):
        logp[b, t:] = float("nan")
    rows = [[3, 3, 40], [8, 1], [2]]
    want = _check(dev, logp, tlen, _labels(rows), V=V)
    for b, y in enumerate(rows):
        assert _spells(want, b, tlen, y)
    tight = _check(dev, logp[..., :V].contiguous(), tlen, _labels(rows))
    assert all(np.array_equal(a, b) for a, b in zip(tight, want))


def test_kernel_ids_outside_the_vocabulary(dev):
    """V, -7 and 2^32 + 5 (label 5 after a careless narrowing): infeasible, nothing read through them; the neighbours are aligned."""
    V = 41
    rows = [[3, V, 4], [3, -7, 4], [2 ** 32 + 5], [3, 5, 4], [3, -1, 4], []]
    tlen = [9] * 6
    want = _check(dev, _logp(12, 6, 9, V), tlen, _labels(rows))
    for b in (0, 1, 2, 4, 5):
        assert _infeasible(want, b), b
    assert _spells(want, 3, tlen, [3, 5, 4])
    zero = _check(dev, _logp(12, 6, 9, V), [9, 9, 9, 0, -3, 9], _labels([[3, 5, 4]] * 6))                  # clips without a frame
    assert _infeasible(zero, 3) and _infeasible(zero, 4) and all(_spells(zero, b, tlen, [3, 5, 4]) for b in (0, 1, 2, 5))


def test_kernel_full_vocabulary(dev):
    """5,049 units, 37 frames: the gather's whole index range."""
    V = 5049
    rows = [[5048, 1, 2500, 2500, 17], [4095, 4096], [5048]]
    tlen = [37, 20, 3]
    want = _check(dev, _logp(13, 3, 37, V, gain=4.0), tlen, _labels(rows))
    for b, y in enumerate(rows):
        assert _spells(want, b, tlen, y)


def test_kernel_refuses_shapes_it_cannot_hold(dev):
    from syncvsr_amd import _lib, ops

    with pytest.raises(_lib.SvsrError):                                          # 2 L + 1 > 2048 states
        ops.ctc_align(_logp(1, 1, 4, 41).to(dev), torch.tensor([4], dtype=torch.int32, device=dev), torch.full((1, 1024), -1, dtype=torch.int64, device=dev))
    with pytest.raises(_lib.SvsrError):                                          # blank outside the vocabulary
        ops.ctc_align(_logp(1, 1, 4, 41).to(dev), torch.tensor([4], dtype=torch.int32, device=dev), _labels([[3]]).to(dev), blank=41)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dev):
    from syncvsr_amd.lrs_model import E2E

    args, odim, sd, _, _, _ = build_lrs_case("lrs_tiny_eval", load_golden=False)
    model = E2E(odim, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    return model, odim


def test_surface_forced_align_batch_equals_the_restatement(dev, tiny):
    model, odim = tiny
    g = torch.Generator().manual_seed(21)
    hs = (torch.randn(13, 3, odim, generator=g) * 3.0).to(dev)
    ys = _labels([[4, 4, 9, 2], [7], [5, 6]])
    ilens = torch.tensor([13, 6, 2])
    got = model.ctc.forced_align_batch(hs, ys.to(dev), ilens.to(dev))
    lp = torch.log_softmax(hs, dim=-1).transpose(0, 1).contiguous().cpu()        # the same activations, as the device normalises them
    want = align_batch(lp.numpy(), ilens.tolist(), ys.numpy(), 0)
    assert len(got) == 3
    for b in range(3):
        assert isinstance(got[b], np.ndarray) and got[b].dtype == np.int64 and got[b].shape == (int(ilens[b]),)
        assert np.array_equal(got[b], want[0][b, : int(ilens[b])])
        assert collapse(got[b]) == ys[b][ys[b] >= 0].tolist()
    again = model.ctc.forced_align_batch(hs, ys, ilens.tolist())
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    with pytest.raises(ValueError, match="clip 1: infeasible"):
        model.ctc.forced_align_batch(hs, _labels([[4], [7, 7], [5]]).to(dev), torch.tensor([13, 2, 2]))


def test_surface_forced_align_is_the_batch_routine_on_one_clip_after_ctc_lo(dev, tiny):
    model, odim = tiny
    g = torch.Generator().manual_seed(22)
    h = torch.randn(11, model.adim, generator=g).to(dev)
    y = [6, 6, 30, 2]
    got = model.ctc.forced_align(h, y)
    assert isinstance(got, list) and len(got) == 11 and all(isinstance(v, int) for v in got) and collapse(got) == y
    assert model.ctc.forced_align(h.unsqueeze(0), torch.tensor(y)) == got
    lp = model.ctc.log_softmax(h.unsqueeze(0))[0]                                # [T, odim] after ctc_lo
    want = align_batch(lp.cpu().numpy()[None], [11], np.array([y]), 0)
    assert got == want[0][0].tolist()
    batch = model.ctc.forced_align_batch(lp.unsqueeze(1), torch.tensor([y]), torch.tensor([11]))
    assert batch[0].tolist() == got


def test_surface_align_clips_three_clips_of_different_lengths(dev, tiny):
    from syncvsr_amd.lrs_align import Alignment, align_clips, align_features

    model, odim = tiny
    g = torch.Generator().manual_seed(23)
    lens = [14, 9, 6]
    clips = torch.zeros(3, 14, 1, 24, 24)
    for c, t in enumerate(lens):
        clips[c, :t] = torch.randn(t, 1, 24, 24, generator=g)
    rows = [[5, 5, 17, 3, 39], [22, 8], [9, 9, 9]]
    targets = _labels(rows)
    alis = align_clips(model, clips.to(dev), lens, targets)
    masks = (torch.arange(14).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).unsqueeze(1).to(dev)
    enc, _ = model.encoder(clips.to(dev), masks)
    assert len(alis) == 3
    for c, (a, y, T) in enumerate(zip(alis, rows, lens)):
        assert isinstance(a, Alignment)
        lp = model.ctc.log_softmax(enc[c : c + 1, :T])[0].cpu()                  # this clip's own encoder output, as the GPU produced it
        f, s, sc = align_batch(lp.numpy()[None], [T], np.array([y]), 0)
        assert a.frames.dtype == np.int64 and np.array_equal(a.frames, f[0]), (c, a.frames, f[0])
        assert a.spans.dtype == np.int64 and np.array_equal(a.spans, s[0]), (c, a.spans, s[0])
        assert np.float32(a.score).view(np.int32) == sc[0].view(np.int32), (c, a.score, sc[0])
        assert a.tokens.tolist() == y and collapse(a.frames) == y
        assert (a.spans[:, 0] <= a.spans[:, 1]).all() and (a.spans[1:, 0] > a.spans[:-1, 1]).all() and a.spans.min() >= 0 and a.spans.max() < T
        assert all((a.frames[s0 : s1 + 1] == y[l]).all() for l, (s0, s1) in enumerate(a.spans))
        ref = torch.stack([lp[s0 : s1 + 1, y[l]].mean() for l, (s0, s1) in enumerate(a.spans)]).numpy()
        assert a.token_logp.dtype == np.float32 and np.allclose(a.token_logp, ref, rtol=1e-6, atol=0.0), (c, a.token_logp, ref)
    again = align_clips(model, clips.to(dev), torch.tensor(lens), targets.to(dev))
    feats = align_features(model, enc, lens, targets)
    for a, b, f in zip(alis, again, feats):
        for x, y_, z in zip(a[:4], b[:4], f[:4]):
            assert np.array_equal(x, y_) and np.array_equal(x, z)
        assert a.score == b.score == f.score
