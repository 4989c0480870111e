"""CPU checks of the DC-TCN training-mode restatement (tests/dctcn_train_restatement.py) against the numbers
tests/golden/make_golden_dctcn_train.py recorded from the reference's own DenseTemporalConvNet in .train() (fp64), and of the dropout sites."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dctcn_train_restatement as TR  # noqa: E402
from dctcn_cases import GOLDEN, dctcn_subcase, rel_err  # noqa: E402
from dctcn_train_restatement import GRADS, ROWS, RUNS, STATS, sub  # noqa: E402
from syncvsr_amd import dropout  # noqa: E402
from syncvsr_amd.dctcn_init import default_dctcn_config, tiny_dctcn_config  # noqa: E402

CASES = [(tag, r) for tag in ("wb_t29", "nowb_t7") for r in RUNS]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dctcn_train_tiny.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def runs():
    """{(tag, run, stats): train_grads(...)}, computed once."""
    out = {}
    for tag, r in CASES:
        cfg, dims, sd, batch = dctcn_subcase("dctcn_tiny", tag)
        for stats in ("all", "kept"):
            out[(tag, r, stats)] = TR.train_grads(cfg, dims, sd, batch, float(cfg.optim.lambda_audio), None, stats=stats, **RUNS[r])
    return out


def _hidden(h):
    return h[:, ::7, [t for t in ROWS if t < h.size(2)]]


@pytest.mark.parametrize("tag,r", CASES)
def test_restatement_matches_reference(golden, runs, tag, r):
    out, grads, gf, new_stats = runs[(tag, r, "all")]
    grads = dict(grads, grad_features=gf)
    for k in ("loss_total", "loss_category", "loss_audio"):
        assert rel_err(out[k], golden[f"{tag}.{r}.{k}"]) < 1e-9, k
    assert rel_err(_hidden(out["last_hidden_states"]), golden[f"{tag}.{r}.hidden"]) < 1e-9
    for bn in STATS:
        for b in ("running_mean", "running_var"):
            assert rel_err(new_stats[f"{bn}.{b}"], golden[f"{tag}.{r}.stat.{bn}.{b}"]) < 1e-9, (bn, b)
    for n in GRADS:
        want, got = torch.from_numpy(golden[f"{tag}.{r}.grad.{n}"]), torch.from_numpy(sub(grads[n]))
        if n.endswith(".net.0.bias"):          # a cbcr* conv bias cancels under batch statistics: rounding noise around zero on both sides
            assert float(want.abs().max()) < 1e-10 and float(got.abs().max()) < 1e-10, n
        else:
            assert rel_err(got, want) < 1e-9, n


@pytest.mark.parametrize("tag,r", CASES)
def test_statistics_over_kept_rows_are_wrong(golden, runs, tag, r):
    """The chomp fact: BatchNorm1d sits BEFORE Chomp1d, so statistics over the T kept rows alone are a different network.  The gap is
    three orders above the bf16 floor of a gradient (profiles/dctcn_train.json): 1e-2 is asserted, 0.17 .. 0.48 were measured."""
    out, grads, gf, new_stats = runs[(tag, r, "kept")]
    assert rel_err(_hidden(out["last_hidden_states"]), golden[f"{tag}.{r}.hidden"]) > 1e-2
    bn = STATS[2]          # a k = 7, d = 5 branch: 59 positions of which 30 are chomped
    assert rel_err(new_stats[f"{bn}.running_var"], golden[f"{tag}.{r}.stat.{bn}.running_var"]) > 1e-2
    n = GRADS[3]
    assert rel_err(sub(grads[n]), golden[f"{tag}.{r}.grad.{n}"]) > 1e-2
    # the 1x1 transition0 has no halo: its statistics are the same either way
    assert rel_err(new_stats[f"{STATS[0]}.running_var"], golden[f"{tag}.{r}.stat.{STATS[0]}.running_var"]) < 1e-9


def test_dropout_reaches_the_output(runs):
    a, b = runs[("wb_t29", "plain", "all")][0], runs[("wb_t29", "mix", "all")][0]
    assert rel_err(a["last_hidden_states"], b["last_hidden_states"]) > 1e-2


def test_dctcn_sites_are_stable():
    tiny = dropout.dctcn_sites(tiny_dctcn_config())
    assert list(tiny.items())[:3] == [("block1.layer1.drop0", 1), ("block1.layer1.drop1", 2), ("block1.layer2.drop0", 3)]
    assert tiny["block2.layer1.drop1"] == 8 and len(tiny) == 8
    full = dropout.dctcn_sites(default_dctcn_config())
    assert len(full) == 24 and full["block4.layer3.drop1"] == 24 and sorted(full.values()) == list(range(1, 25))
    assert {k: v for k, v in full.items() if k in tiny and k.startswith("block1")} == {k: v for k, v in tiny.items() if k.startswith("block1")}


def test_site_key_is_the_mask_key():
    k = dropout.site_key(5, 3)
    assert 0 <= k < 2 ** 32 and k == dropout.site_key(5, 3) != dropout.site_key(5, 4)
    m = dropout.keep_mask(5, 3, 0.2, 4096)
    assert 0.74 < m.mean() < 0.86
