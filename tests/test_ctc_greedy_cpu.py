"""CTC greedy decoding, host side (no GPU): the numpy / torch restatement (tests/ctc_greedy_restatement.py) against hand-written expectations and
against forced alignment on the recorded posteriors of tests/golden/ctc_align.npz, the C ABI of the two kernels, and the errors the surface
raises before it launches anything."""
import os

import numpy as np
import pytest
import torch

from ctc_align_restatement import align_one
from ctc_greedy_restatement import collapse_batch, frame_best, greedy_one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ctc_align.npz")
TINY = dict(adim=128, aheads=2, eunits=256, elayers=2, ddim=128, dheads=2, dunits=256, dlayers=1)

# (name, the dominant unit of each of the Tmax frames — a pair: two units planted at exactly the same value —, tlen, blank, tokens, spans):
# the expectations are written by hand, nothing is run to get them
HAND = [
    ("a a _ a b", [5, 5, 0, 5, 7], 5, 0, [5, 5, 7], [(0, 1), (3, 3), (4, 4)]),
    ("all blank", [0, 0, 0, 0], 4, 0, [], []),
    ("one frame, a token", [3], 1, 0, [3], [(0, 0)]),
    ("one frame, a blank", [0], 1, 0, [], []),
    ("a run up to the last live frame, other winners behind it", [2, 4, 4, 4, 6, 1, 6], 4, 0, [2, 4], [(0, 0), (1, 3)]),
    ("the same run with a blank that is unit 8", [0, 0, 8, 0, 3, 8, 8, 5, 5], 7, 8, [0, 0, 3], [(0, 1), (3, 3), (4, 4)]),
    ("exact two-way ties: the lower id wins", [(2, 6), 2, 6, (7, 6), (0, 3), 3], 6, 0, [2, 6, 3], [(0, 1), (2, 3), (5, 5)]),
]
HAND_V = 9


def plant(winners, V=HAND_V, seed=0):
    """fp32 logits [Tmax, V]: noise in [-1, 1) and 8.0 at the dominant unit(s) of every frame."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(len(winners), V, generator=g) * 2.0 - 1.0
    for t, w in enumerate(winners):
        for v in (w if isinstance(w, tuple) else (w,)):
            x[t, v] = 8.0
    return x


@pytest.mark.parametrize("name,winners,tlen,blank,tokens,spans", HAND, ids=[h[0] for h in HAND])
def test_restatement_reproduces_the_hand_made_cases(name, winners, tlen, blank, tokens, spans):
    x = plant(winners)
    tk, sp, tlp, frames, score = greedy_one(x[:tlen].numpy(), blank)
    assert tk.dtype == np.int64 and tk.tolist() == tokens
    assert sp.dtype == np.int64 and sp.shape == (len(tokens), 2) and [tuple(s) for s in sp.tolist()] == spans
    assert frames.tolist() == [min(w) if isinstance(w, tuple) else w for w in winners[:tlen]]
    lp = torch.log_softmax(x[:tlen].double(), -1)                              # an independent statement of the two sums
    at = torch.stack([lp[t, f] for t, f in enumerate(frames.tolist())])
    assert tlp.dtype == np.float32 and tlp.shape == (len(tokens),)
    assert np.allclose(tlp, [float(at[a : b + 1].mean()) for a, b in spans], rtol=0, atol=1e-6)
    assert score.dtype == np.float32 and abs(float(score) - float(at.sum())) <= 1e-6 * tlen
    # the batch form: the same clip padded, rows behind ntok filled
    best, blp = frame_best(x.numpy())
    bt, bs, bl, nt, sc = collapse_batch(best[None], blp[None], [tlen], blank)
    L = len(tokens)
    assert nt.tolist() == [L] and bt[0, :L].tolist() == tokens and (bt[0, L:] == -1).all() and (bs[0, L:] == -1).all() and (bl[0, L:] == 0).all()
    assert np.array_equal(bl[0, :L].view(np.int32), tlp.view(np.int32)) and sc[0].view(np.int32) == score.view(np.int32)


def test_greedy_path_is_its_own_best_alignment_on_the_recorded_posteriors():
    """The best unconstrained path is also the best path constrained to its own transcript: the forced alignment (host restatement) of the
    greedy transcript has the greedy score, on every recorded clip that does not decode to nothing."""
    gold = np.load(GOLD, allow_pickle=False)
    done = skipped = 0
    for i in range(int(gold["n_batches"])):
        hs, ilens = gold[f"b{i}.hs"], gold[f"b{i}.ilens"]
        lp = torch.log_softmax(torch.from_numpy(hs), dim=-1).transpose(0, 1).contiguous().numpy()
        for b in gold[f"b{i}.clips"]:
            T = int(ilens[b])
            tokens, spans, _, frames, score = greedy_one(lp[b, :T], 0)
            if len(tokens) == 0:
                skipped += 1
                continue
            f, s, sc = align_one(lp[b, :T], tokens, 0)
            assert np.isfinite(sc) and abs(float(sc) - float(score)) <= 1e-5 * T, (i, b, sc, score)
            assert np.array_equal(f, frames) and np.array_equal(s, spans), (i, b)
            done += 1
    assert done >= 1, (done, skipped)


def test_the_tiny_inference_case_decodes_to_tokens_without_a_gain():
    """What the end-to-end GPU test relies on: the oracle's encoder features of `lrs_infer_tiny` decode to at least three tokens under the
    case's own ctc_lo weights."""
    from golden_cases import build_lrs_infer_case

    _, odim, sd, _, _, gold = build_lrs_infer_case("lrs_infer_tiny")
    logits = torch.from_numpy(gold["enc_feat"]).float() @ sd["ctc.ctc_lo.weight"].float().T + sd["ctc.ctc_lo.bias"].float()
    assert logits.shape[1] == odim
    tokens = greedy_one(logits.numpy(), 0)[0]
    assert len(tokens) >= 3, tokens


def test_new_symbols_are_declared_and_exported():
    from syncvsr_amd import _lib, ops

    decl = _lib.parse_header()
    assert [n for _, n in decl["svsr_ctc_frame_best"]] == ["logits", "ldp", "tlen", "C", "Tmax", "V", "best", "best_logp", "stream"]
    assert [n for _, n in decl["svsr_ctc_collapse"]] == ["best", "best_logp", "tlen", "C", "Tmax", "Lcap", "blank", "tokens", "spans", "token_logp",
                                                         "ntok", "score", "stream"]
    assert dict((n, t) for t, n in decl["svsr_ctc_frame_best"])["ldp"] == "int64_t"
    assert ops.CTC_GREEDY_MAX_FRAMES >= 2048
    src = open(os.path.join(ROOT, "syncvsr_amd", "csrc", "lrs_search.hip")).read()
    assert f"#define CG_MAX_T {ops.CTC_GREEDY_MAX_FRAMES}\n" in src
    body = src[src.index("// CTC best-path (greedy) decoding, two launches") : src.index("// Source attention of a beam step")]
    assert "void k_ctc_frame_best(" in body and "void k_ctc_collapse(" in body
    assert "atomic" not in body.lower(), "the greedy kernels use no atomics"
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    for name in ("svsr_ctc_frame_best", "svsr_ctc_collapse"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert lib.svsr_steplist_knows(name.encode())


@pytest.fixture(scope="module")
def model():
    from syncvsr_amd.lrs_init import default_lrs_args
    from syncvsr_amd.lrs_model import E2E

    return E2E(41, default_lrs_args(**TINY), seed=3).eval()


BAD = [
    # (lengths, blank_id, words the message must hold)
    ([5], 0, ("1 lengths for 2 clips",)),
    ([5, 5, 5], 0, ("3 lengths for 2 clips",)),
    ([5, 0], 0, ("lengths", "[1, 5]")),
    ([6, 5], 0, ("lengths", "[1, 5]")),
    ([5, 5], 41, ("blank_id 41", "[0, 41)")),
    ([5, 5], -1, ("blank_id -1", "[0, 41)")),
]


@pytest.mark.parametrize("lengths,blank,words", BAD)
def test_greedy_refuses_bad_lengths_and_blanks_before_any_launch(model, monkeypatch, lengths, blank, words):
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_align import greedy_clips, greedy_features

    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a launch preceded the check"))
    calls = (lambda ln: greedy_features(model, torch.zeros(2, 5, 128), ln, blank),
             lambda ln: greedy_clips(model, torch.zeros(2, 5, 1, 24, 24), ln, blank),
             lambda ln: model.ctc.greedy_batch(torch.zeros(2, 5, 128), ln, blank))
    for call in calls:
        for ln in (lengths, torch.tensor(lengths)):
            with pytest.raises(ValueError) as e:
                call(ln)
            for w in words:
                assert w in str(e.value), (w, str(e.value))


def test_greedy_refuses_wrong_shapes_and_the_cpu(model, monkeypatch):
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_align import greedy_clips, greedy_features

    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a launch preceded the check"))
    with pytest.raises(ValueError, match=r"enc_feats must be \[clips, frames, 128\]"):
        greedy_features(model, torch.zeros(2, 5, 64), [5, 5])
    with pytest.raises(ValueError, match="enc_feats must be"):
        greedy_features(model, torch.zeros(5, 128), [5])
    with pytest.raises(ValueError, match="enc_feats must be"):
        model.ctc.greedy_batch(torch.zeros(2, 5, 41), [5, 5])
    with pytest.raises(ValueError, match="clips must be"):
        greedy_clips(model, torch.zeros(2, 5, 24, 24), [5, 5])
    with pytest.raises(ValueError, match="clips must be"):
        greedy_clips(model, torch.zeros(2, 5, 3, 24, 24), [5, 5])
    with pytest.raises(ValueError, match=f"more than {ops.CTC_GREEDY_MAX_FRAMES} frames"):
        greedy_features(model, torch.zeros(1, ops.CTC_GREEDY_MAX_FRAMES + 1, 128), [7])
    for call in (lambda: greedy_features(model, torch.zeros(2, 5, 128), [5, 3]),      # well-formed, but on the CPU: no fallback
                 lambda: greedy_clips(model, torch.zeros(2, 5, 1, 24, 24), [5, 3]),
                 lambda: model.ctc.greedy_batch(torch.zeros(2, 5, 128), torch.tensor([5, 3]), 40)):
        with pytest.raises(RuntimeError, match="HIP device.*no CPU fallback"):
            call()
