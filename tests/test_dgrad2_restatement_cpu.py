"""CPU side of the merged downsample-block data gradient (tests/dgrad2_cases.py): the float64 restatement against autograd, the census of the
merged launch plan (svsr_conv_plan mode 3, host only) and its meta record, and the conditions the bit comparison of
tests/test_gpu_dgrad2_edges.py rests on."""
import pytest
import torch
import torch.nn.functional as F

import contraction_cases as cc
import contraction_restatement as R
import dgrad2_cases as dc

SIZES = sorted(set(dc.MAPS) | {(1, 1), (1, 2), (2, 1), (1, 5), (5, 1), (2, 5), (12, 12), (22, 22), (11, 11), (6, 6), (2, 256), (2, 258)})


@pytest.mark.parametrize("hw", [(4, 4), (5, 5), (6, 7), (7, 6), (2, 2), (1, 1), (1, 4)])
def test_restatement_is_the_gradient_of_two_summed_convolutions(hw):
    H, W = hw
    g = torch.Generator().manual_seed(H * 31 + W)
    N, K, Ci = 2, 5, 3
    x = torch.randn(N, Ci, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    w3 = torch.randn(K, 3, 3, Ci, dtype=torch.float64, generator=g)
    w1 = torch.randn(K, 1, 1, Ci, dtype=torch.float64, generator=g)
    y3 = F.conv2d(x, w3.permute(0, 3, 1, 2), stride=2, padding=1)
    y1 = F.conv2d(x, w1.permute(0, 3, 1, 2), stride=2, padding=0)
    assert y3.shape == y1.shape
    dy, dy2 = torch.randn(y3.shape, dtype=torch.float64, generator=g), torch.randn(y3.shape, dtype=torch.float64, generator=g)
    ((y3 * dy).sum() + (y1 * dy2).sum()).backward()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    got = R.conv_dgrad(nhwc(dy), w3, 2, 1, hw) + R.conv_dgrad(nhwc(dy2), w1, 2, 0, hw)
    assert torch.allclose(got, nhwc(x.grad), rtol=1e-12, atol=1e-12)
    # the 1x1 branch reaches exactly the (even, even) pixels
    reach = R.dgrad_reach(1, 2, 0, hw)
    want = torch.zeros(H, W, dtype=torch.bool)
    want[0::2, 0::2] = True
    assert torch.equal(reach, want)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_census_of_the_merged_plan(hw):
    H, W = hw
    N, co = 3, 64
    words, meta = dc.plan_words(3, N, H, W, co)
    words1, meta1 = dc.plan_words(1, N, H, W, co)
    got, got1 = dc.plan_classes(words), dc.plan_classes(words1)
    want, want1 = dc.census(H, W, True), dc.census(H, W, False)
    Wo = R.out_size(W, 3, 2, 1)
    # classes: the restatement's, each pixel once, decreasing tap count
    assert sorted((tw, sorted(d for _, d in pos)) for tw, _, _, _, pos in got) == sorted((k, v) for k, v in want.items())
    assert sorted((tw, sorted(d for _, d in pos)) for tw, _, _, _, pos in got1) == sorted((k, v) for k, v in want1.items())
    assert [len(c[0]) for c in got] == sorted((len(c[0]) for c in got), reverse=True)
    assert sorted(d for c in got for _, d in c[4]) == list(range(H * W))
    # the extra tap: exactly once in the plan, right behind the centre tap (word 4) with the centre tap's delta, in the class of the (even, even) pixels
    with2 = [c for c in got if dc.TAP2 in c[0]]
    assert len(with2) == 1 and sum(c[0].count(dc.TAP2) for c in got) == 1
    tw, delta, P, _, pos = with2[0]
    assert tw == (4, dc.TAP2) and delta[0] == delta[1] == 0
    assert P == -(-H // 2) * -(-W // 2) and all((d // W) % 2 == 0 and (d % W) % 2 == 0 and s == (d // W // 2) * Wo + d % W // 2 for s, d in pos)
    # every other class is the plain plan's, and the plain plan's centre class is the one-tap class (4,)
    strip = lambda cl: sorted((c[0], c[1], c[2], tuple(c[4])) for c in cl if dc.TAP2 not in c[0] and c[0] != (4,))
    assert strip(got) == strip(got1) and sum(1 for c in got1 if c[0] == (4,)) == 1
    # tap counts of the parity classes.  Odd sizes have no border: exactly the four classes 4 / 2 / 2 / 2.  An even size has a last odd row or
    # column that loses one tap row / column and forms border classes next to the four interior ones.
    counts = sorted(len(k) for k in want)
    if H % 2 and W % 2 and H >= 3 and W >= 3:
        assert counts == [2, 2, 2, 4]
    if H >= 4 and W >= 4:
        interior = {(y % 2, x % 2): len(k) for k, v in want.items() for d in v for y, x in [divmod(d, W)] if y < H - 1 and x < W - 1}
        assert interior == {(0, 0): 2, (0, 1): 2, (1, 0): 2, (1, 1): 4}
        assert len(want) == (3 if H % 2 == 0 else 2) * (3 if W % 2 == 0 else 2)
    if (H, W) == (1, 1):
        assert list(want) == [(4, dc.TAP2)]
    if (H, W) == (2, 2):
        assert sorted(want) == [(4, dc.TAP2), (5,), (7,), (8,)]
    if (H, W) == (1, 2):
        assert sorted(want) == [(4, dc.TAP2), (5,)]
    # meta = {bm, bn, ns, tiles, grid_y, classes, max taps, rows} of the MERGED plan
    bm, bn, ns, tiles, gy, ncls, max_taps, rows = meta
    assert ncls == len(want) and max_taps == max(counts) and rows == N * H * W and gy == -(-co // bn)
    assert tiles == sum(-(-N * c[2] // bm) for c in got)
    t0 = 0
    for c in got:
        assert c[3] == t0
        t0 += -(-N * c[2] // bm)
    assert max_taps <= 4 and (bm, bn) in ((64, 64), (128, 64), (128, 128))


def test_class_count_by_parity_of_the_size():
    """four classes at odd sizes; an even height or width adds the border classes of its last odd row / column"""
    n = lambda H, W: len(dc.census(H, W))
    assert n(5, 5) == 4 and n(11, 11) == 4 and n(7, 5) == 4
    assert n(6, 7) == 6 and n(7, 6) == 6          # + (last odd row, even) and (last odd row, odd) — or the column twins
    assert n(4, 4) == 9 and n(22, 22) == 9 and n(6, 6) == 9
    assert sorted(len(k) for k in dc.census(4, 4)) == [1, 1, 1, 2, 2, 2, 2, 2, 4]


def test_benchmark_shapes_keep_their_instantiation():
    """the merged plan of the three downsample blocks at 928 frames launches the tile the 3x3 plan launched: max taps is 4 in both"""
    for (H, co), want in (((22, 64), (128, 64, 2)), ((11, 128), (128, 128, 2)), ((6, 256), (128, 128, 2))):
        _, m3 = dc.plan_words(3, 928, H, H, co)
        _, m1 = dc.plan_words(1, 928, H, H, co)
        assert tuple(m3[:3]) == tuple(m1[:3]) == want and m3[6] == m1[6] == 4 and m3[7] == m1[7]
        assert m3[3] >= m1[3] - 8 and m3[5] == m1[5]


def test_mode_3_is_the_3x3_stride_2_plan_only():
    import ctypes

    lib, meta = cc._lib(), (ctypes.c_int * 8)()
    for k, s, p in ((3, 1, 1), (1, 2, 0), (3, 2, 0), (2, 2, 1)):
        assert lib.svsr_conv_plan(3, 2, 6, 6, 64, k, s, p, None, 0, meta) < 0
    assert lib.svsr_conv_plan(4, 2, 6, 6, 64, 3, 2, 1, None, 0, meta) < 0


def test_symbols_are_declared_bound_and_registered():
    from syncvsr_amd import _lib

    decl, lib = _lib.parse_header(), _lib.load()
    for name, nargs in (("svsr_igemm_dgrad2", 25), ("svsr_igemm_dgrad2_bn", 24)):
        assert len(decl[name]) == nargs and len(getattr(lib, name).argtypes) == nargs
        assert lib.svsr_steplist_knows(name.encode())


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_conditions(case):
    """what the GPU file relies on: the label, the 2^24 budget, and that the two-launch form loses nothing (dxd is a bf16 number)"""
    with cc.knobs(case.knobs):
        _, meta = dc.plan_words(3, case.N, case.H, case.W, case.ci_in)
        import ctypes

        m = (ctypes.c_int * 8)(*meta)
        assert cc._glds_label(m, case.kp, case.ci_in, case.epi != "plain") == dc.expected_label(case)
    if case.floats or case.H > 100:          # (the large map's operands come from the same generator; its references are built on the GPU side once)
        return
    d = dc.build(case)
    assert max(R.budget_of(d["abs"]).values()) < R.LIMIT
    assert torch.equal(R.rne_bf16(d["dxd"]), d["dxd"]), "the generator must keep the 1x1 gradient exactly representable in bf16"
    assert d["in"]["dy"].shape[-1] == case.kp and not bool(d["in"]["dy"][..., case.planes:].any()) and not bool(d["in"]["wt2"][:, case.planes:].any())


def test_cases_reach_every_instantiation_and_every_issue_shape():
    labels = {dc.expected_label(c) for c in dc.CASES}
    assert not set(dc.REQUIRED) - labels, set(dc.REQUIRED) - labels
    small = {(c.N, c.H, c.W, c.planes, c.ci_in, c.epi) for c in dc.CASES}
    for hw in ((4, 4), (5, 5), (6, 7), (7, 6), (2, 2)):
        for N in (1, 3):
            for ch in ((16, 8), (128, 64), (136, 72), (256, 128)):
                for epi in dc.EPILOGUES:
                    assert (N, *hw, *ch, epi) in small
    assert {e for c in dc.CASES if c.floats for e in [c.epi]} == set(dc.EPILOGUES)
