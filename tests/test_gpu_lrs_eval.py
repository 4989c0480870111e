"""Scoring of transcripts on the GPU (-m gpu): svsr_edit_distance against the restatement (tests/edit_distance_restatement.py), every output
compared as integers, exactly; then the surface built on it (lrs_eval.token_errors / greedy_token_errors / Evaluator) on the `lrs_infer_tiny`
model.  Behind its length every row holds the OTHER sequence's ids, so a read past a length would change the answer."""
import itertools

import numpy as np
import pytest
import torch

from ctc_greedy_restatement import collapse_batch
from edit_distance_restatement import edit_batch, edit_one, oracle_errors, text_errors
from golden_cases import build_lrs_infer_case

pytestmark = pytest.mark.gpu

EDGE = [0, 1, 2, 63, 64, 65, 127, 128, 129]
GRID = list(itertools.product(EDGE, EDGE)) + [(1024, 1024), (1024, 0), (0, 1024), (1, 1024)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rows(seqs, others, width):
    """int64 [N, width]: row n = seqs[n], then the ids of others[n] (and of seqs[n] again) over and over up to the width."""
    out = np.zeros((len(seqs), width), np.int64)
    for n, (s, o) in enumerate(zip(seqs, others)):
        fill = list(o) + list(s) + [7]
        row = list(s) + [fill[k % len(fill)] for k in range(width - len(s))]
        out[n] = row[:width]
    return out


def _pairs(rng, lens, alphabet):
    return ([rng.integers(0, alphabet, size=h).tolist() for h, _ in lens], [rng.integers(0, alphabet, size=r).tolist() for _, r in lens])


def _launch(dev, hyps, refs, wh=None, wr=None, pitch=0):
    """One launch over the pairs -> int32 [N, 4] on the host.  pitch > 0: the rows are views of rows `pitch` ids wider."""
    from syncvsr_amd import ops

    wh = max(len(h) for h in hyps) if wh is None else wh
    wr = max(len(r) for r in refs) if wr is None else wr
    hyp, ref = _rows(hyps, refs, wh + pitch), _rows(refs, hyps, wr + pitch)
    ht, rt = torch.from_numpy(hyp).to(dev)[:, :wh], torch.from_numpy(ref).to(dev)[:, :wr]
    assert pitch == 0 or (ht.stride(0) == wh + pitch and not ht.is_contiguous()) or wh == 0
    hl = torch.tensor([len(h) for h in hyps], dtype=torch.int32, device=dev)
    rl = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev)
    out = ops.edit_distance(ht, hl, rt, rl)
    assert out.dtype == torch.int32 and out.shape == (len(hyps), 4)
    return out.cpu().numpy()


def _check(dev, hyps, refs, **kw):
    got = _launch(dev, hyps, refs, **kw)
    want = np.array([edit_one(h, r) for h, r in zip(hyps, refs)], np.int32).reshape(len(hyps), 4)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(len(hyps[n]), len(refs[n]), got[n].tolist(), want[n].tolist()) for n in bad[:5]]
    assert (got[:, 1:].sum(axis=1) == got[:, 0]).all()
    assert (np.array([len(h) for h in hyps]) == np.array([len(r) for r in refs]) - got[:, 2] + got[:, 3]).all()
    return got


@pytest.mark.parametrize("alphabet", [3, 5000])
def test_kernel_equals_the_restatement_on_the_length_grid(dev, alphabet):
    """Every pair of edge lengths and the four pairs at the cap in ONE launch (rows of 1024 ids on both sides, so the short rows carry up to
    1024 ids of the other sequence behind their length); three ids: almost every cell is a tie."""
    hyps, refs = _pairs(np.random.default_rng(alphabet), GRID, alphabet)
    got = _check(dev, hyps, refs)
    assert got[GRID.index((1024, 0))].tolist() == [1024, 0, 0, 1024] and got[GRID.index((0, 1024))].tolist() == [1024, 0, 1024, 0]
    assert got[GRID.index((0, 0))].tolist() == [0, 0, 0, 0]


def test_kernel_one_pair_per_launch(dev):
    rng = np.random.default_rng(5)
    for lens in ((65, 129), (0, 0), (1, 1), (0, 3), (130, 64)):
        _check(dev, *_pairs(rng, [lens], 3))


def test_kernel_three_hundred_mixed_pairs_equal_disjoint_and_wide_ids(dev):
    """One launch of 306 pairs: random lengths over both alphabets, equal sequences (0), disjoint alphabets (max of the lengths, all
    substitutions and the rest one kind), and ids that differ above bit 32 only (different).  Then the same rows as views of wider rows."""
    rng = np.random.default_rng(17)
    lens = [(int(rng.integers(0, 90)), int(rng.integers(0, 90))) for _ in range(150)]
    h3, r3 = _pairs(rng, lens, 3)
    h5, r5 = _pairs(rng, lens, 5000)
    same = [rng.integers(0, 3, size=n).tolist() for n in (1, 64, 200)]
    dis_h = [rng.integers(0, 50, size=n).tolist() for n in (40, 70)]
    dis_r = [rng.integers(50, 100, size=n).tolist() for n in (70, 40)]
    low = rng.integers(0, 1 << 31, size=30).tolist()
    high = [v + (1 << 32) for v in low]
    neg = [v - (1 << 63) for v in low]                                       # the same low words under the sign bit
    hyps = h3 + h5 + same + dis_h + [low]
    refs = r3 + r5 + same + dis_r + [high]
    assert len(hyps) == 306
    got = _check(dev, hyps, refs)
    assert (got[300:303] == 0).all()
    assert got[303].tolist() == [70, 40, 30, 0] and got[304].tolist() == [70, 40, 0, 30]
    assert got[305].tolist() == [30, 30, 0, 0]
    assert _check(dev, [low, neg, low], [neg, neg, low])[:, 0].tolist() == [30, 0, 0]
    wide = _check(dev, hyps, refs, pitch=5)                                  # row strides wider than the longest row
    assert np.array_equal(wide, got)
    assert np.array_equal(_check(dev, hyps[:40], refs[:40], wh=120, wr=97, pitch=3), got[:40])


def test_rows_wider_than_the_cap_are_refused_with_nothing_launched(dev, monkeypatch):
    from syncvsr_amd import ops

    W = ops.EDIT_MAX_LEN + 1
    wide, ok = torch.zeros(2, W, dtype=torch.int64, device=dev), torch.zeros(2, 8, dtype=torch.int64, device=dev)
    ln = torch.ones(2, dtype=torch.int32, device=dev)
    assert ops.edit_distance(wide[:, : W - 1], ln, ok, ln).cpu().tolist() == [[0, 0, 0, 0]] * 2          # the cap itself is taken (a view of wider rows)
    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a launch preceded the check"))
    for hyp, ref in ((wide, ok), (ok, wide)):
        with pytest.raises(ValueError, match=f"more than {ops.EDIT_MAX_LEN} ids"):
            ops.edit_distance(hyp, ln, ref, ln)
    assert ops.edit_distance(ok[:0], ln[:0], ok[:0], ln[:0]).shape == (0, 4)                             # no pairs: nothing to launch


# ----------------------------------------------------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------------------------------------------------
def _runs(seed, C, Tmax, units):
    g = torch.Generator().manual_seed(seed)
    new = torch.rand(C, Tmax, generator=g) < 0.4
    draw = torch.tensor(units)[torch.randint(0, len(units), (C, Tmax), generator=g)]
    best = torch.zeros(C, Tmax, dtype=torch.int64)
    for t in range(Tmax):
        best[:, t] = torch.where(new[:, t] | (t == 0), draw[:, t], best[:, max(t - 1, 0)])
    return best.numpy(), (-torch.rand(C, Tmax, generator=g)).numpy().astype(np.float32)


def test_token_errors_straight_from_the_collapse_kernel(dev):
    """Random winners -> ops.ctc_collapse -> token_errors, everything on the device; the host copies through the two restatements."""
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_eval import token_errors

    C, Tmax, blank, ignore = 6, 70, 0, -1
    best, lp = _runs(3, C, Tmax, [0, 2, 2, 5, 9, 0])
    tlen = [70, 33, 1, 64, 65, 12]
    best[2, 0] = 0                                                           # a clip that decodes to nothing
    rng = np.random.default_rng(4)
    targets = np.full((C, 40), ignore, np.int64)
    tl = [40, 0, 3, 17, 25, 9]                                               # one full row, one empty target
    for c, n in enumerate(tl):
        targets[c, :n] = rng.choice([2, 5, 9], size=n)
    tokens, _, _, ntok, _ = ops.ctc_collapse(torch.from_numpy(best.astype(np.int32)).to(dev), torch.from_numpy(lp).to(dev),
                                             torch.tensor(tlen, dtype=torch.int32, device=dev), blank)
    got = token_errors(tokens, ntok, torch.from_numpy(targets).to(dev), ignore)
    assert got.device.type == "cuda" and got.dtype == torch.int64 and got.shape == (5,)
    wt, _, _, wn, _ = collapse_batch(best, lp, tlen, blank)
    assert wn[2] == 0 and wn.max() > 10
    want = edit_batch(wt, wn, targets, tl).astype(np.int64).sum(axis=0).tolist() + [sum(tl)]
    assert got.cpu().tolist() == want
    other = np.where(targets == ignore, -7, targets)                         # another ignore_id, targets on the host
    assert token_errors(tokens, ntok, torch.from_numpy(other), -7).cpu().tolist() == want


LENS = [16, 11, 5]
ODIM_TOKENS = lambda odim: ["<blank>"] + [("▁" if i % 3 == 0 else "") + "abcdefghij"[i % 10] for i in range(1, odim - 1)] + ["<eos>"]      # noqa: E731


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
    rng = np.random.default_rng(8)
    targets = np.full((len(LENS), 9), model.ignore_id, np.int64)
    for c, n in enumerate((9, 4, 6)):
        targets[c, :n] = rng.integers(1, odim - 1, size=n)
    return model, clips.to(dev), torch.from_numpy(targets), ODIM_TOKENS(odim)


def _want(hyps, hyp_ids, refs, ref_ids, nbests=None, level="word"):
    e = text_errors(hyps, refs, level)
    tok = edit_batch(hyp_ids, [len(h) for h in hyp_ids], ref_ids, [len(r) for r in ref_ids])[:, 0].sum() if hyp_ids is not None else 0
    ntok = sum(len(r) for r in ref_ids) if hyp_ids is not None else 0
    return {"wer": e[0] / e[4] if e[4] else None, "total_edit_distance": int(e[0]), "total_length": int(e[4]), "sub": int(e[1]), "del": int(e[2]),
            "ins": int(e[3]), "token_error_rate": tok / ntok if ntok else None,
            "oracle_wer": None if nbests is None else oracle_errors(nbests, refs, level) / e[4]}


def _refs(model, targets, tokens):
    from syncvsr_amd.lrs_eval import ids_to_text

    ids = [[v for v in row if v != model.ignore_id] for row in targets.tolist()]
    return ids, [ids_to_text(r, tokens) for r in ids]


def _add(a, b):
    keys = ("total_edit_distance", "total_length", "sub", "del", "ins")
    return {k: a[k] + b[k] for k in keys}


@pytest.mark.parametrize("level", ["word", "char"])
def test_evaluator_greedy_equals_the_restatement_on_the_decoded_texts(dev, tiny, level):
    from syncvsr_amd.lrs_align import greedy_clips
    from syncvsr_amd.lrs_eval import Evaluator, greedy_token_errors, ids_to_text

    model, clips, targets, tokens = tiny
    ref_ids, refs = _refs(model, targets, tokens)
    paths = greedy_clips(model, clips, LENS)
    hyp_ids = [p.tokens.tolist() for p in paths]
    hyps = [ids_to_text(y, tokens) for y in hyp_ids]
    assert sum(len(y) for y in hyp_ids) >= 3 and all(len(r.split()) >= 1 for r in refs)
    want = _want(hyps, hyp_ids, refs, ref_ids, level=level)
    ev = Evaluator(model, tokens, level=level)
    ev.update(clips, LENS, targets)
    assert ev.compute() == want
    ev.update(clips, LENS, targets.to(dev))                                  # accumulates: the same batch again doubles every count
    twice = ev.compute()
    assert _add(want, want) == {k: twice[k] for k in _add(want, want)} and twice["wer"] == want["wer"] and twice["oracle_wer"] is None
    ev.reset()
    assert ev.compute()["total_length"] == 0
    # two updates over the halves of the batch: the counts of what each half decodes to
    head, tail = clips[:2].contiguous(), clips[2:, : LENS[2]].contiguous()
    a, b = greedy_clips(model, head, LENS[:2]), greedy_clips(model, tail, LENS[2:])
    ev.update(head, LENS[:2], targets[:2])
    ev.update(tail, LENS[2:], targets[2:])
    ids2 = [p.tokens.tolist() for p in a + b]
    assert ev.compute() == _want([ids_to_text(y, tokens) for y in ids2], ids2, refs, ref_ids, level=level)
    # the device-only path of a validation loop: the same token counts, nothing copied
    got = greedy_token_errors(model, clips, LENS, targets.to(dev))
    assert got.device.type == "cuda" and got.dtype == torch.int64
    tok = edit_batch(hyp_ids, [len(h) for h in hyp_ids], ref_ids, [len(r) for r in ref_ids]).astype(np.int64).sum(axis=0).tolist()
    assert got.cpu().tolist() == tok + [sum(len(r) for r in ref_ids)]


def test_evaluator_texts_accumulate_like_one_update_of_the_concatenation(dev, tiny):
    from syncvsr_amd.lrs_eval import Evaluator

    model, _, _, tokens = tiny
    hyps = ["the cat sat", "", "on a mat it is", "Hello  there"]
    refs = ["the cat sat down", "a b c", "on the mat", "hello there"]
    one, two = Evaluator(model, tokens), Evaluator(model, tokens)
    one.update_texts(hyps, refs)
    two.update_texts(hyps[:1], refs[:1])
    two.update_texts(hyps[1:], refs[1:])
    assert one.compute() == two.compute() == _want(hyps, None, refs, None)
    nothing = Evaluator(model, tokens)
    nothing.update_texts([""], ["a b c"])                                    # a transcript of nothing: the reference's words are all deleted
    out = nothing.compute()
    assert (out["total_edit_distance"], out["sub"], out["del"], out["ins"], out["total_length"], out["wer"]) == (3, 0, 3, 0, 3, 1.0)


def test_evaluator_clip_that_decodes_to_nothing_scores_deletions(dev, tiny):
    from syncvsr_amd.lrs_align import greedy_clips
    from syncvsr_amd.lrs_eval import Evaluator

    model, clips, targets, tokens = tiny
    one = clips[:1, :1].contiguous()
    winner = int(greedy_clips(model, one, [1])[0].frames[0])
    ev = Evaluator(model, tokens, blank_id=winner)                           # the only frame's winner is the blank: an empty transcript
    ev.update(one, [1], targets[:1])
    ref_ids, refs = _refs(model, targets[:1], tokens)
    n = len(refs[0].split())
    out = ev.compute()
    assert n >= 1 and (out["total_edit_distance"], out["sub"], out["del"], out["ins"], out["total_length"]) == (n, 0, n, 0, n)
    assert out["token_error_rate"] == 1.0


def test_evaluator_beam_search_scores_the_one_best_and_the_oracle(dev, tiny):
    from syncvsr_amd.lrs_eval import Evaluator, ids_to_text
    from syncvsr_amd.lrs_infer import decode_clips, get_beam_search_decoder

    model, clips, targets, tokens = tiny
    ref_ids, refs = _refs(model, targets, tokens)
    search = get_beam_search_decoder(model, tokens, ctc_weight=0.1, beam_size=4)
    nbests = decode_clips(model, search, clips, LENS)
    assert max(len(nb) for nb in nbests) > 1, [len(nb) for nb in nbests]
    texts = [[ids_to_text(h.yseq[1:].cpu(), tokens) for h in nb] for nb in nbests]
    best_ids = [[v for v in nb[0].yseq[1:].tolist() if v != model.eos] if nb else [] for nb in nbests]
    hyps = [t[0] if t else "" for t in texts]
    want = _want(hyps, best_ids, refs, ref_ids, nbests=texts)
    ev = Evaluator(model, tokens, search)
    ev.update(clips, LENS, targets)
    got = ev.compute()
    assert got == want
    assert got["oracle_wer"] is not None and got["oracle_wer"] <= got["wer"]
    ev.update(clips, LENS, targets)
    assert ev.compute()["oracle_wer"] == want["oracle_wer"] and ev.compute()["total_length"] == 2 * want["total_length"]
