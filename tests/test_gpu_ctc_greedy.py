"""CTC greedy decoding on the GPU (-m gpu): svsr_ctc_frame_best against torch on the same fp32 logits, svsr_ctc_collapse against the
restatement (tests/ctc_greedy_restatement.py) value for value, then the surface built on them (lrs_align.greedy_clips / greedy_features,
E2E.ctc.greedy_batch) on the `lrs_infer_tiny` model, and forced alignment of the greedy transcripts."""
import numpy as np
import pytest
import torch

from ctc_greedy_restatement import collapse_batch, frame_best, greedy_one, margin
from golden_cases import build_lrs_infer_case
from test_ctc_greedy_cpu import HAND, HAND_V, plant

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _tlens(C, Tmax, seed):
    """Ragged lengths: the first clip full, one clip of a single frame where there is room for it."""
    g = torch.Generator().manual_seed(seed)
    t = [Tmax] + [int(torch.randint(1, Tmax + 1, (1,), generator=g)) for _ in range(C - 1)]
    if C > 1:
        t[-1] = 1
    return t


def _logits(seed, C, Tmax, V, ldp, gain=3.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(C * Tmax, ldp)
    x[:, :V] = torch.randn(C * Tmax, V, generator=g) * gain
    return x


def _live(tlen, Tmax):
    return (torch.arange(Tmax).unsqueeze(0) < torch.tensor(tlen).unsqueeze(1)).reshape(-1).numpy()


def _frame_best(dev, x, tlen, Tmax, V):
    from syncvsr_amd import ops

    best, lp = ops.ctc_frame_best(x.to(dev), torch.tensor(tlen, dtype=torch.int32, device=dev), Tmax=Tmax, V=V)
    assert best.dtype == torch.int32 and lp.dtype == torch.float32 and best.shape == lp.shape == (len(tlen), Tmax)
    return best.cpu().numpy().reshape(-1), lp.cpu().numpy().reshape(-1)


def _check_frames(dev, x, tlen, Tmax, V, nan_rows=()):
    """One launch against torch on the same numbers: winners equal, log-probabilities within 1e-5 of the fp64 log_softmax, padding (-1, 0)."""
    best, lp = _frame_best(dev, x, tlen, Tmax, V)
    live = _live(tlen, Tmax)
    want_best, want_lp = frame_best(x[:, :V].contiguous().numpy())
    assert np.array_equal(best[live], want_best[live]), (best[live], want_best[live])
    ok = live.copy()
    ok[list(nan_rows)] = False
    err = np.abs(lp[ok].astype(np.float64) - want_lp[ok]).max() if ok.any() else 0.0
    print(f"C*Tmax={x.shape[0]} V={V} ldp={x.shape[1]}: max |best_logp - fp64 log_softmax| = {err:.3e}")
    assert err <= 1e-5, err
    for r in nan_rows:
        assert live[r] and np.isnan(lp[r]) and np.isnan(want_lp[r])
    assert (best[~live] == -1).all() and (lp[~live] == 0).all()
    return best, lp


# ----------------------------------------------------------------------------------------------------------------------
# the frame kernel
# ----------------------------------------------------------------------------------------------------------------------
# (C, Tmax, V, ldp): one column; below, one short of, and one past a 64-lane sweep of single columns; the shipped vocabulary (its pitch a
# multiple of 64: 16-byte loads, one column left for the single loads); V % 4 == 3 over four full unrolled sweeps; and two pitches that are
# no multiple of four (every column a single load)
FRAME_SHAPES = [(1, 1, 1, 1), (2, 5, 41, 64), (3, 7, 63, 64), (2, 9, 65, 128), (2, 6, 5049, 5056), (1, 3, 8191, 8192), (2, 3, 41, 41), (1, 2, 300, 301)]


@pytest.mark.parametrize("C,Tmax,V,ldp", FRAME_SHAPES)
def test_frame_kernel_equals_torch(dev, C, Tmax, V, ldp):
    _check_frames(dev, _logits(31 + V, C, Tmax, V, ldp), _tlens(C, Tmax, V), Tmax, V)


def test_frame_kernel_flat_and_peaked_rows(dev):
    """Rows whose log-probability is far from 0 and rows where it is 0 to the last bit; a row of equal logits (every comparison a tie)."""
    C, Tmax, V, ldp = 1, 4, 5049, 5056
    x = _logits(5, C, Tmax, V, ldp, gain=0.01)
    x[1, :V] = 2.5
    x[2, :V] *= 3000.0
    x[3, :V] = -60.0
    x[3, 4097] = 60.0
    best, lp = _check_frames(dev, x, [4], Tmax, V)
    assert best[1] == 0 and abs(lp[1] + np.log(V)) < 1e-5 and best[3] == 4097 and lp[3] == 0.0


def test_frame_kernel_ties_and_nan_follow_torch(dev):
    C, Tmax, V, ldp = 2, 9, 65, 128
    x = _logits(7, C, Tmax, V, ldp)
    top = float(x.max()) + 1.0
    x[0, 40] = x[0, 7] = top                      # two lanes of the 16-byte sweep
    x[1, 64] = x[1, 63] = top                     # the last column of the sweep and the single column behind it
    x[2, 3] = x[2, 0] = x[2, 64] = top            # three ways
    x[4, 50] = x[4, 13] = float("nan")            # two NaN: the first wins, whatever else the row holds
    x[5, 64] = float("nan")
    x[5, 2] = float("inf")
    tlen = [9, 8]
    best, _ = _check_frames(dev, x, tlen, Tmax, V, nan_rows=(4, 5))
    assert best[:6].tolist()[:3] == [7, 63, 0] and best[4] == 13 and best[5] == 64
    y = _logits(8, 2, 3, 41, 41)                  # the same through single loads
    y[1, 40] = y[1, 5] = float(y.max()) + 1.0
    y[2, 30] = y[2, 9] = float("nan")
    best, _ = _check_frames(dev, y, [3, 1], 3, 41, nan_rows=(2,))
    assert best[1] == 5 and best[2] == 9


def test_frame_kernel_never_reads_pitch_padding_or_frames_behind_the_length(dev):
    """NaN, inf and huge values in columns V .. ldp - 1 and in every row behind tlen: not a bit of the outputs changes."""
    for C, Tmax, V, ldp in ((2, 5, 41, 64), (2, 6, 5049, 5056), (1, 3, 8191, 8192)):
        x = _logits(9, C, Tmax, V, ldp)
        tlen = _tlens(C, Tmax, 3)
        clean = _check_frames(dev, x, tlen, Tmax, V)
        live = _live(tlen, Tmax)
        for junk in (float("nan"), float("inf"), 3.0e38):
            y = x.clone()
            y[:, V:] = junk
            y[torch.from_numpy(~live)] = junk
            got = _frame_best(dev, y, tlen, Tmax, V)
            assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1].view(np.int32), clean[1].view(np.int32)), (V, junk)


# ----------------------------------------------------------------------------------------------------------------------
# the collapse kernel
# ----------------------------------------------------------------------------------------------------------------------
def _check_collapse(dev, best, lp, tlen, blank, Lcap=None):
    """One launch against the restatement: tokens, spans, ntok equal, token_logp and score bit-equal, the fill behind ntok."""
    from syncvsr_amd import ops

    want = collapse_batch(best, lp, tlen, blank, Lcap)
    got = ops.ctc_collapse(torch.from_numpy(best.astype(np.int32)).to(dev), torch.from_numpy(lp).to(dev),
                           torch.tensor(tlen, dtype=torch.int32, device=dev), blank, Lcap)
    tokens, spans, tlp, ntok, score = (t.cpu().numpy() for t in got)
    assert tokens.dtype == np.int64 and spans.dtype == np.int32 and tlp.dtype == np.float32 and ntok.dtype == np.int32 and score.dtype == np.float32
    assert np.array_equal(ntok, want[3]), (ntok, want[3])
    assert np.array_equal(tokens, want[0]), (tokens, want[0])
    assert np.array_equal(spans, want[1]), (spans, want[1])
    assert np.array_equal(tlp.view(np.int32), want[2].view(np.int32)), (tlp, want[2])
    assert np.array_equal(score.view(np.int32), want[4].view(np.int32)), (score, want[4])
    for c, n in enumerate(ntok):
        assert (tokens[c, n:] == -1).all() and (spans[c, n:] == -1).all() and (tlp[c, n:] == 0).all()
    return want


@pytest.mark.parametrize("name,winners,tlen,blank,tokens,spans", HAND, ids=[h[0] for h in HAND])
def test_collapse_kernel_on_the_hand_made_cases(dev, name, winners, tlen, blank, tokens, spans):
    best, lp = frame_best(plant(winners).numpy())
    want = _check_collapse(dev, best[None], lp[None], [tlen], blank)
    L = len(tokens)
    assert want[3].tolist() == [L] and want[0][0, :L].tolist() == tokens and [tuple(s) for s in want[1][0, :L].tolist()] == spans


def test_both_kernels_on_the_hand_made_cases_in_one_batch(dev):
    """The cases that share blank 0 as ONE padded batch through both kernels: what a clip decodes to does not depend on its batch-mates."""
    from syncvsr_amd import ops

    cases = [h for h in HAND if h[3] == 0]
    Tmax = max(len(h[1]) for h in cases)
    x = torch.zeros(len(cases), Tmax, 64)
    for c, h in enumerate(cases):
        x[c, : len(h[1]), :HAND_V] = plant(h[1])
    tlen = torch.tensor([h[2] for h in cases], dtype=torch.int32, device=dev)
    best, lp = ops.ctc_frame_best(x.reshape(-1, 64).to(dev), tlen, Tmax=Tmax, V=HAND_V)
    tokens, spans, _, ntok, _ = (t.cpu().numpy() for t in ops.ctc_collapse(best, lp, tlen, 0))
    for c, h in enumerate(cases):
        L = len(h[4])
        assert ntok[c] == L and tokens[c, :L].tolist() == h[4] and [tuple(s) for s in spans[c, :L].tolist()] == h[5], h[0]


def _runs(seed, C, Tmax, units):
    """Winner sequences drawn with long runs (a new unit with probability 1/4 per frame) and random log-probabilities."""
    g = torch.Generator().manual_seed(seed)
    new = torch.rand(C, Tmax, generator=g) < 0.25
    draw = torch.tensor(units)[torch.randint(0, len(units), (C, Tmax), generator=g)]
    best = torch.zeros(C, Tmax, dtype=torch.int64)
    for t in range(Tmax):
        best[:, t] = torch.where(new[:, t] | (t == 0), draw[:, t], best[:, max(t - 1, 0)])
    lp = -torch.rand(C, Tmax, generator=g) * 4.0
    return best.numpy(), lp.numpy().astype(np.float32)


@pytest.mark.parametrize("C,Tmax", [(1, 1), (3, 7), (2, 64), (2, 65), (1, 300), (1, 2048)])
@pytest.mark.parametrize("blank", [0, 3])
def test_collapse_kernel_equals_the_restatement_on_long_runs(dev, C, Tmax, blank):
    best, lp = _runs(100 + Tmax, C, Tmax, [0, 3, 3, 5, 4096, 0])
    tlen = _tlens(C, Tmax, Tmax) if Tmax > 1 else [1]
    want = _check_collapse(dev, best, lp, tlen, blank)
    if Tmax >= 64:
        assert 0 < want[3][0] < Tmax // 2                                          # collapses happened, and tokens are left
    full = np.full_like(lp, -1.0)                                                  # every frame another unit: as many tokens as frames
    _check_collapse(dev, np.arange(1, C * Tmax + 1).reshape(C, Tmax), full, tlen, 0)
    _check_collapse(dev, np.full((C, Tmax), blank), full, tlen, blank)             # nothing but blanks: ntok = 0


def test_collapse_kernel_clips_without_frames_and_a_short_capacity(dev):
    best, lp = _runs(7, 3, 40, [0, 2, 9])
    want = _check_collapse(dev, best, lp, [40, 0, -3], 0)
    assert want[3][1] == want[3][2] == 0 and want[4][1] == want[4][2] == 0
    cut = _check_collapse(dev, best, lp, [40, 17, 1], 0, Lcap=2)                   # ntok counts every token, rows >= Lcap are not written
    assert cut[3][0] > 2 and cut[0].shape == (3, 2)


def test_kernels_refuse_what_they_cannot_hold(dev):
    from syncvsr_amd import _lib, ops

    tl = torch.tensor([2], dtype=torch.int32, device=dev)
    x = torch.zeros(2, 32, device=dev)
    with pytest.raises(_lib.SvsrError):                                            # ldp < V
        ops.ctc_frame_best(x, tl, Tmax=2, V=41)
    with pytest.raises(_lib.SvsrError):                                            # V = 0
        ops.ctc_frame_best(x, tl, Tmax=2, V=0)
    T = ops.CTC_GREEDY_MAX_FRAMES + 1
    best, lp = torch.zeros(1, T, dtype=torch.int32, device=dev), torch.zeros(1, T, device=dev)
    with pytest.raises(_lib.SvsrError):                                            # more frames than the LDS plan holds
        ops.ctc_collapse(best, lp, tl, 0)
    with pytest.raises(_lib.SvsrError):                                            # Lcap = 0
        ops.ctc_collapse(best[:, :8].contiguous(), lp[:, :8].contiguous(), tl, 0, Lcap=0)
    ops.ctc_collapse(best[:, : T - 1].contiguous(), lp[:, : T - 1].contiguous(), tl, 0)       # the bound itself is taken
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------------------------------------------------
LENS = [16, 11, 5]


@pytest.fixture(scope="module")
def tiny(dev):
    from syncvsr_amd.lrs_model import E2E

    args, odim, sd, clip, _, _ = build_lrs_infer_case("lrs_infer_tiny", load_golden=False)
    model = E2E(odim, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    clips = torch.zeros(len(LENS), max(LENS), *clip.shape[1:])
    for c, t in enumerate(LENS):
        clips[c, :t] = clip[:t]
    return model, clips.to(dev)


def test_surface_greedy_clips_features_alignment_and_facade_agree(dev, tiny):
    from syncvsr_amd.lrs_align import GreedyPath, align_clips, greedy_clips, greedy_features
    from syncvsr_amd.lrs_infer import CTCPrefixScorer

    model, clips = tiny
    Tmax = max(LENS)
    paths = greedy_clips(model, clips, LENS)
    masks = (torch.arange(Tmax).unsqueeze(0) < torch.tensor(LENS).unsqueeze(1)).unsqueeze(1).to(dev)
    enc, _ = model.encoder(clips, masks)
    feats = greedy_features(model, enc, torch.tensor(LENS))
    assert len(paths) == len(feats) == len(LENS)
    excluded = frames_seen = 0
    sure = []                                                                      # clips whose every frame has a clear winner
    for c, (p, f, T) in enumerate(zip(paths, feats, LENS)):
        assert isinstance(p, GreedyPath) and isinstance(f, GreedyPath)
        assert p.tokens.dtype == np.int64 and p.spans.dtype == np.int64 and p.token_logp.dtype == np.float32 and p.frames.dtype == np.int64
        assert p.frames.shape == (T,) and p.spans.shape == (len(p.tokens), 2) and p.token_logp.shape == p.tokens.shape and isinstance(p.score, float)
        for a, b in zip(p[:4], f[:4]):                                             # the same encoder output, the same kernels: the same bits
            assert np.array_equal(a, b)
        assert p.score == f.score
        logp = CTCPrefixScorer(model, model.eos).ctc_log_softmax(enc[c, :T]).cpu().numpy()      # this clip's posteriors as the search sees them
        tokens, spans, tlp, frames, score = greedy_one(logp, 0)
        clear = margin(logp) > 1e-3
        excluded += int((~clear).sum())
        frames_seen += T
        assert np.array_equal(p.frames[clear], frames[clear]), (c, p.frames, frames)
        assert abs(p.score - float(score)) <= 1e-5 * T, (c, p.score, score)
        if clear.all():
            sure.append(c)
            assert np.array_equal(p.tokens, tokens) and np.array_equal(p.spans, spans), (c, p.tokens, tokens)
            assert np.allclose(p.token_logp, tlp, rtol=0, atol=1e-5)
    print(f"{excluded} of {frames_seen} frames have a top-two margin of 1e-3 or less and were left out of the exact comparison")
    assert 4 * excluded <= frames_seen, (excluded, frames_seen)
    assert sum(len(p.tokens) for p in paths) >= 3
    # forced alignment of the greedy transcripts finds the greedy paths
    live = [c for c, p in enumerate(paths) if len(p.tokens) > 0]
    targets = torch.full((len(live), max(len(paths[c].tokens) for c in live)), -1, dtype=torch.int64)
    for i, c in enumerate(live):
        targets[i, : len(paths[c].tokens)] = torch.from_numpy(paths[c].tokens)
    alis = align_clips(model, clips[live], [LENS[c] for c in live], targets)
    for a, c in zip(alis, live):
        assert abs(a.score - paths[c].score) <= 1e-5 * LENS[c], (c, a.score, paths[c].score)
        if c in sure:
            assert np.array_equal(a.spans, paths[c].spans) and np.array_equal(a.frames, paths[c].frames), (c, a.spans, paths[c].spans)
    # the reference-named facade returns the transcripts
    batch = model.ctc.greedy_batch(enc, LENS)
    assert len(batch) == len(LENS)
    for b, p in zip(batch, paths):
        assert isinstance(b, np.ndarray) and b.dtype == np.int64 and np.array_equal(b, p.tokens)
    other = greedy_features(model, enc, LENS, blank_id=int(paths[0].tokens[0]))   # another blank: that unit is gone, the frames are the same
    assert int(paths[0].tokens[0]) not in other[0].tokens and np.array_equal(other[0].frames, paths[0].frames)


def test_surface_two_runs_are_bit_identical(dev, tiny):
    from syncvsr_amd.lrs_align import greedy_features

    model, clips = tiny
    g = torch.Generator().manual_seed(41)
    enc = torch.randn(3, 37, model.adim, generator=g).to(dev)
    lens = [37, 20, 1]
    one, two = greedy_features(model, enc, lens), greedy_features(model, enc, lens)
    for a, b in zip(one, two):
        for x, y in zip(a[:4], b[:4]):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        assert np.float32(a.score).tobytes() == np.float32(b.score).tobytes()
