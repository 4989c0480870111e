"""CTC forced alignment, host side (no GPU): the numpy restatement against what the reference's own `CTC.forced_align_batch` returned
(tests/golden/ctc_align.npz), the C ABI of the new kernel, and the errors the surface raises before it launches anything."""
import os

import numpy as np
import pytest
import torch

from ctc_align_restatement import align_batch, align_one, collapse, frames_needed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ctc_align.npz")
TINY = dict(adim=128, aheads=2, eunits=256, elayers=2, ddim=128, dheads=2, dunits=256, dlayers=1)


def test_restatement_equals_the_reference_on_every_recorded_clip():
    gold = np.load(GOLD, allow_pickle=False)
    seen = dict(clips=0, B=set(), T=set(), L=set(), repeats=0)
    for i in range(int(gold["n_batches"])):
        hs, ys, ilens, ali = (gold[f"b{i}.{k}"] for k in ("hs", "ys", "ilens", "ali"))
        assert hs.dtype == np.float32 and hs.shape[2] == int(gold["V"])
        lp = torch.log_softmax(torch.from_numpy(hs), dim=-1).transpose(0, 1).contiguous().numpy()
        frames, spans, score = align_batch(lp, ilens, ys, 0)
        for b in gold[f"b{i}.clips"]:
            T, y = int(ilens[b]), ys[b][ys[b] != -1]
            assert np.array_equal(frames[b, :T], ali[b, :T]) and (frames[b, T:] == -1).all() and (ali[b, T:] == -1).all(), (i, b)
            assert collapse(ali[b, :T]) == y.tolist()
            assert np.isfinite(score[b])
            for l, (a, z) in enumerate(spans[b, : len(y)]):
                assert 0 <= a <= z < T and (frames[b, a : z + 1] == y[l]).all()
            seen["clips"] += 1
            seen["repeats"] += frames_needed(y) - len(y)
            seen["L"].add(len(y))
        seen["B"].add(hs.shape[1])
        seen["T"].add(hs.shape[0])
    assert seen["clips"] >= 40 and seen["B"] == {1, 2, 3, 4} and {3, 39} <= seen["T"] and seen["L"] == {1, 2, 3, 4, 5, 6} and seen["repeats"] >= 10


def test_restatement_marks_what_has_no_path():
    lp = torch.log_softmax(torch.randn(6, 7, generator=torch.Generator().manual_seed(3)), -1).numpy()
    for y, T in (([2, 2, 3], 3), ([1], 0), ([], 4), ([7], 4), ([-7], 4), ([2 ** 32 + 5], 4), ([0, 2], 5)):
        f, s, sc = align_one(lp[:T], y, 0)
        assert sc == -np.inf and (f == -1).all() and (s == -1).all(), (y, T)
    f, s, sc = align_one(lp[:4], [2, 2, 3], 0)                                        # exactly enough frames: the one path
    assert f.tolist() == [2, 0, 2, 3] and s.tolist() == [[0, 0], [2, 2], [3, 3]]
    assert sc == np.float32(np.float32(np.float32(lp[0, 2] + lp[1, 0]) + lp[2, 2]) + lp[3, 3])
    fr, sp, sc = align_batch(lp[None], [6], np.array([[3, -1, 4, -1]]), 0)             # a -1 in front of a live label is no padding
    assert sc[0] == -np.inf and (fr == -1).all() and (sp == -1).all()


def test_new_symbol_is_declared_and_exported():
    from syncvsr_amd import _lib

    decl = _lib.parse_header()
    assert "svsr_ctc_align" in decl, "svsr_ctc_align is not declared in include/syncvsr_hip.h"
    assert [n for _, n in decl["svsr_ctc_align"]] == ["logp", "ldp", "tlen", "labels", "Lmax", "B", "Tmax", "V", "blank", "bp", "frames", "spans",
                                                      "score", "stream"]
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert hasattr(lib, "svsr_ctc_align"), "svsr_ctc_align is not exported"
    assert lib.svsr_steplist_knows(b"svsr_ctc_align")
    src = open(os.path.join(ROOT, "syncvsr_amd", "csrc", "lrs_search.hip")).read()
    body = src[src.index("void k_ctc_align(") : src.index("// Source attention of a beam step")]
    assert "atomic" not in body.lower(), "the alignment kernel uses no atomics"


@pytest.fixture(scope="module")
def model():
    from syncvsr_amd.lrs_init import default_lrs_args
    from syncvsr_amd.lrs_model import E2E

    return E2E(41, default_lrs_args(**TINY), seed=3).eval()


BAD = [
    # (ys_pad, ilens, words the message must hold)
    ([[3, 3, 4], [5, -1, -1]], [3, 6], ("clip 0", "infeasible", "tlen = 3", "need 4")),
    ([[3, 4, -1], [7, 7, 7]], [6, 4], ("clip 1", "infeasible", "tlen = 4", "need 5")),
    ([[3, 4, -1], [-1, -1, -1]], [6, 6], ("clip 1", "empty transcript")),
    ([[3, 41, -1], [5, -1, -1]], [6, 6], ("clip 0", "id 41")),
    ([[3, 4, -1], [5, -7, 2]], [6, 6], ("clip 1", "id -7")),
    ([[3, 4, -1], [2 ** 32 + 5, -1, -1]], [6, 6], ("clip 1", f"id {2 ** 32 + 5}")),
    ([[3, 0, 4], [5, -1, -1]], [6, 6], ("clip 0", "blank")),
    ([[3, -1, 4], [5, -1, -1]], [6, 6], ("clip 0", "ignore_id", "in front of a live token")),
    ([[3, 4, -1], [5, -1, -1]], [6, 0], ("lengths", "[1, 6]")),
    ([[3, 4, -1], [5, -1, -1]], [7, 6], ("lengths", "[1, 6]")),
    ([[3, 4, -1], [5, -1, -1]], [6], ("1 lengths for 2 clips",)),
]


@pytest.mark.parametrize("ys,ilens,words", BAD)
def test_forced_align_batch_refuses_what_has_no_alignment_before_any_launch(model, monkeypatch, ys, ilens, words):
    from syncvsr_amd import ops

    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a launch preceded the check"))
    hs = torch.zeros(6, 2, 41)                                                   # on the CPU: a launch could not even start
    with pytest.raises(ValueError) as e:
        model.ctc.forced_align_batch(hs, torch.tensor(ys), torch.tensor(ilens))
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_the_other_entry_points_share_the_contract(model, monkeypatch):
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_align import align_clips, align_features

    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a launch preceded the check"))
    h = torch.zeros(4, 128)
    for y, word in (([3, 3, 4, 5], "infeasible"), ([], "empty transcript"), ([41], "id 41"), ([0], "blank"), ([3, -1, 4], "ignore_id")):
        with pytest.raises(ValueError, match=word):
            model.ctc.forced_align(h, y)
        with pytest.raises(ValueError, match=word):
            model.ctc.forced_align(h.unsqueeze(0), torch.tensor(y, dtype=torch.int64))
    with pytest.raises(ValueError, match="clip 0.*id 9"):
        model.ctc.forced_align(h, [9], blank_id=9)
    with pytest.raises(ValueError, match="must be"):
        model.ctc.forced_align(torch.zeros(4, 64), [3])
    with pytest.raises(ValueError, match="must be"):
        model.ctc.forced_align_batch(torch.zeros(6, 2, 40), torch.tensor([[3], [4]]), [6, 6])
    tg = torch.tensor([[3, 4, 4], [5, -1, -1]])
    with pytest.raises(ValueError, match=r"clip 0: infeasible, tlen = 3 .* need 4"):
        align_features(model, torch.zeros(2, 5, 128), [3, 5], tg)
    with pytest.raises(ValueError, match=r"clip 0: infeasible, tlen = 3 .* need 4"):
        align_clips(model, torch.zeros(2, 5, 1, 24, 24), [3, 5], tg)             # from the lengths and targets alone, before the encoder
    with pytest.raises(ValueError, match="lengths"):
        align_clips(model, torch.zeros(2, 5, 1, 24, 24), [5, 6], tg)
    with pytest.raises(ValueError, match="clips must be"):
        align_clips(model, torch.zeros(2, 5, 24, 24), [5, 5], tg)
    with pytest.raises(RuntimeError, match="HIP device"):                        # well-formed, but on the CPU: no fallback
        align_features(model, torch.zeros(2, 5, 128), [5, 5], tg)
