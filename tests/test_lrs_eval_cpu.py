"""Scoring of transcripts, host side (no GPU): the restatement of svsr_edit_distance (tests/edit_distance_restatement.py) against an independent
textbook Levenshtein and hand-worked cases, `lrs_eval.ids_to_text` against strings recorded from the reference (tests/golden/lrs_eval_text.npz,
written by tests/golden/make_golden_lrs_eval.py), `lrs_eval.sequences` at its three levels, the C ABI of the kernel, and the errors the surface
raises before it launches anything."""
import os

import numpy as np
import pytest
import torch

from edit_distance_restatement import edit_batch, edit_one, levenshtein, oracle_errors, text_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lrs_eval_text.npz")
TINY = dict(adim=128, aheads=2, eunits=256, elayers=2, ddim=128, dheads=2, dunits=256, dlayers=1)

# (hyp, ref, (cost, S, D, I)): worked by hand from the definition, nothing is run to get them
HAND = [
    ("kitten", "sitting", (3, 2, 1, 0)),             # k->s, e->i, and the g has no partner: one deletion
    ("sitting", "kitten", (3, 2, 0, 1)),
    ("", "abc", (3, 0, 3, 0)),                       # the border cells
    ("abc", "", (3, 0, 0, 3)),
    ("", "", (0, 0, 0, 0)),
    ("abcabc", "abcabc", (0, 0, 0, 0)),
    ("abc", "xyz", (3, 3, 0, 0)),
    ("b", "ab", (1, 0, 1, 0)),
    ("ab", "b", (1, 0, 0, 1)),
]

# The tie-break, over the alphabet {a, b}.
# "ab" / "ba": cell(1,1) = one substitution; cell(1,2) = (1, D=1) (a matches the second a); cell(2,1) = (1, I=1); in cell(2,2) b meets a:
# the diagonal gives 1 + 1 substitution = (2, S=2), the deletion from cell(2,1) gives (2, D=1, I=1), the insertion from cell(1,2) the same
# cost: a three-way tie, and the diagonal wins.
# "aaba" / "bbbaab": in the last cell a meets b: the diagonal cell(3,5) = (4, S=2, D=2) plus a substitution costs 5; the deletion from
# cell(4,5) = (3, S=2, D=1) and the insertion from cell(3,6) = (3, D=3) both cost 4: the deletion wins, (4, 2, 2, 0), not (4, 0, 3, 1).
TIES = [("ab", "ba", (2, 2, 0, 0)), ("aaba", "bbbaab", (4, 2, 2, 0))]


@pytest.mark.parametrize("hyp,ref,want", HAND + TIES, ids=[f"{h or '-'}/{r or '-'}" for h, r, _ in HAND + TIES])
def test_restatement_reproduces_the_hand_made_cases(hyp, ref, want):
    got = edit_one(hyp, ref)
    assert got == want
    assert got[0] == levenshtein(hyp, ref)


def _properties(hyp, ref, cell):
    cost, S, D, I = (int(v) for v in cell)
    assert cost == levenshtein(hyp, ref), (hyp, ref, cell)
    assert S + D + I == cost and min(S, D, I) >= 0, (hyp, ref, cell)
    assert len(hyp) == len(ref) - D + I, (hyp, ref, cell)


def test_restatement_equals_the_textbook_distance_and_keeps_its_properties_on_random_pairs():
    rng = np.random.default_rng(11)
    n = 0
    for alphabet in (2, 3, 50):
        for _ in range(120):
            hyp = rng.integers(0, alphabet, size=int(rng.integers(0, 13))).tolist()
            ref = rng.integers(0, alphabet, size=int(rng.integers(0, 13))).tolist()
            _properties(hyp, ref, edit_one(hyp, ref))
            n += 1
    for hyp, ref, want in HAND + TIES:
        _properties(hyp, ref, want)
    assert n == 360


def test_restatement_batch_form_looks_at_live_ids_only():
    hyp = np.array([[1, 2, 3, 9, 9], [4, 4, 9, 9, 9]])
    ref = np.array([[1, 3, 9], [9, 9, 9]])
    got = edit_batch(hyp, [3, 2], ref, [2, 0])
    assert got.dtype == np.int32 and got.tolist() == [[1, 0, 0, 1], [2, 0, 0, 2]]


def test_ids_to_text_equals_the_reference_strings():
    """Targets: `TextTransform.post_process` of the padded row.  Hypotheses: `parse_hypothesis` of [sos] + ids + [eos], then the three
    calls of lightning.py:122 in their order; that order leaves a blank in front of a trailing <eos> in place, `ids_to_text` strips last, so
    the two are compared up to blanks at the ends — `.split()`, which every level but "char" applies, does not see the difference."""
    from syncvsr_amd.lrs_eval import ids_to_text

    gold = np.load(GOLD, allow_pickle=False)
    tokens = [str(t) for t in gold["tokens"]]
    eos = len(tokens) - 1
    assert tokens[eos] == "<eos>" and len(gold["ids"]) >= 30
    seen = set()
    for row, target, raw in zip(gold["ids"], gold["target_text"], gold["hyp_raw"]):
        live = row[row >= 0]
        assert ids_to_text(row, tokens) == str(target)                                   # padded: the -1 are skipped
        assert ids_to_text(torch.from_numpy(live), tokens) == str(target)
        said = str(raw).replace("▁", " ").strip().replace("<eos>", "")
        got = ids_to_text(live.tolist() + [eos], tokens)
        assert got == said.strip() and got.split() == said.split()
        assert got == str(target)                                                        # both sides of a pair are written alike
        seen.add(got)
    assert "" in seen and "the cats SAT on the Mat" in seen and "it's" in seen and "a b" in seen


def test_sequences_at_the_three_levels():
    from syncvsr_amd.lrs_eval import sequences

    hyps, refs = ["The cat  sat", "", "a b"], ["the CAT sat down", "on it", "a b"]
    for level, hl, rl in (("word", [3, 0, 2], [4, 2, 2]), ("char", [12, 0, 3], [16, 5, 3]), ("token", [3, 0, 2], [4, 2, 2])):
        hyp, hyp_len, ref, ref_len = sequences(hyps, refs, level)
        assert hyp.dtype == ref.dtype == torch.int64 and hyp_len.dtype == ref_len.dtype == torch.int32
        assert hyp_len.tolist() == hl and ref_len.tolist() == rl and hyp.shape == (3, max(hl)) and ref.shape == (3, max(rl))
        for n in range(3):
            assert (hyp[n, hl[n]:] == -1).all() and (ref[n, rl[n]:] == -1).all()
        got = edit_batch(hyp.numpy(), hyp_len.numpy(), ref.numpy(), ref_len.numpy())
        want = [edit_one(*pair) for pair in zip(*[[_split(t, level) for t in side] for side in (hyps, refs)])]
        assert got.tolist() == [list(w) for w in want], level
        assert got[:, 0].sum() == text_errors(hyps, refs, level)[0] and sum(rl) == text_errors(hyps, refs, level)[4]
    word = sequences(hyps, refs, "word")
    assert word[0][0, :3].tolist() == word[2][0, :3].tolist()                            # lowered: "The" == "the", "CAT" == "cat"
    token = sequences(hyps, refs, "token")
    assert token[0][0, 0] != token[2][0, 0] and token[0][0, 2] == token[2][0, 2]         # not lowered
    assert edit_batch(*[t.numpy() for t in (word[0], word[1], word[2], word[3])])[0].tolist() == [1, 0, 1, 0]
    empty = sequences([""], [""], "word")
    assert empty[0].shape == (1, 0) and empty[1].tolist() == [0]
    with pytest.raises(ValueError, match="level"):
        sequences(hyps, refs, "phone")
    with pytest.raises(ValueError, match="2 hypotheses for 3 references"):
        sequences(hyps[:2], refs, "word")
    assert oracle_errors([["the cat", "a cat sat"], []], ["the cat sat", "on"], "word") == 1 + 1


def _split(text, level):
    from edit_distance_restatement import split

    return split(text, level)


def test_new_symbol_is_declared_and_exported():
    from syncvsr_amd import _lib, ops

    decl = _lib.parse_header()
    assert [n for _, n in decl["svsr_edit_distance"]] == ["hyp", "ldh", "hyp_len", "ref", "ldr", "ref_len", "N", "out", "stream"]
    types = dict((n, t) for t, n in decl["svsr_edit_distance"])
    assert types["hyp"] == types["ref"] == "const int64_t*" and types["ldh"] == types["ldr"] == "int64_t" and types["out"] == "int*"
    assert ops.EDIT_MAX_LEN >= 1024 and ops.EDIT_MAX_LEN >= ops.CTC_ALIGN_MAX_LABELS
    src = open(os.path.join(ROOT, "syncvsr_amd", "csrc", "lrs_eval.hip")).read()
    assert f"#define ED_MAX_LEN {ops.EDIT_MAX_LEN}\n" in src and "void k_edit_distance(" in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.lower() and "float" not in code and "__shared__" not in code, "integers only, no atomics, no LDS"
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert hasattr(lib, "svsr_edit_distance"), "svsr_edit_distance is not exported"
    assert lib.svsr_steplist_knows(b"svsr_edit_distance")


@pytest.fixture(scope="module")
def model():
    from syncvsr_amd.lrs_init import default_lrs_args
    from syncvsr_amd.lrs_model import E2E

    return E2E(41, default_lrs_args(**TINY), seed=3).eval()


def test_too_wide_rows_are_refused_before_any_launch(model, monkeypatch):
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_eval import Evaluator, greedy_token_errors, token_errors

    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a launch preceded the check"))
    W = ops.EDIT_MAX_LEN + 1
    ln = torch.ones(2, dtype=torch.int32)
    wide, ok = torch.zeros(2, W, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int64)
    for hyp, ref in ((wide, ok), (ok, wide)):
        with pytest.raises(ValueError, match=f"more than {ops.EDIT_MAX_LEN} ids"):
            ops.edit_distance(hyp, ln, ref, ln)
        with pytest.raises(ValueError, match=f"more than {ops.EDIT_MAX_LEN} ids"):
            token_errors(hyp, ln, ref)
    with pytest.raises(ValueError, match=f"more than {ops.EDIT_MAX_LEN} ids"):
        greedy_token_errors(model, torch.zeros(1, W, 1, 24, 24), [W], torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="1 lengths for 2 clips"):
        greedy_token_errors(model, torch.zeros(2, 5, 1, 24, 24), [5], ok)
    with pytest.raises(ValueError, match="clips must be"):
        greedy_token_errors(model, torch.zeros(2, 5, 24, 24), [5, 5], ok)
    with pytest.raises(ValueError, match="level"):
        Evaluator(model, ["a"] * 41, level="phone")


def test_the_surface_refuses_the_cpu(model, monkeypatch):
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_eval import Evaluator, greedy_token_errors, token_errors

    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a launch preceded the check"))
    ok, ln = torch.zeros(2, 8, dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    ev = Evaluator(model, [f"t{i}" for i in range(41)])
    for call in (lambda: token_errors(ok, ln, ok),
                 lambda: greedy_token_errors(model, torch.zeros(2, 5, 1, 24, 24), [5, 3], ok),
                 lambda: ev.update(torch.zeros(2, 5, 1, 24, 24), [5, 3], ok),
                 lambda: ev.update_texts(["a"], ["b"])):
        with pytest.raises(RuntimeError, match="HIP device.*no CPU fallback"):
            call()
    out = ev.compute()                                                                   # nothing scored: counts of zero, rates None
    assert out["total_edit_distance"] == out["total_length"] == 0 and out["wer"] is None and out["oracle_wer"] is None
