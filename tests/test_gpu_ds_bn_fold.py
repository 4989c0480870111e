"""The downsample blocks' folded BatchNorm passes against the launch chains they replace, bit for bit (-m gpu).

Forward: svsr_bn_act_fwd2 = relu(bn2(c2) + bf16(bn_d(c_d))) against svsr_bn_act_fwd(c2, res = svsr_bn_act_fwd(c_d, act 0), act 1)
(reference tcn/models/resnet.py:65-72: out = bn2(conv2(.)); out += downsample(x); relu).
Backward: svsr_bn_bwd_from_stats_ds (bn2's apply pass, which also leaves the partial rows of the 1x1 branch's BatchNorm backward) followed by
svsr_bn_bwd_from_stats on those rows, against svsr_bn_bwd_from_stats followed by svsr_bn_act_bwd(g, NULL, c_d, ..., act 0): dc2, dcd, the
partial rows themselves, the dgamma / dbeta accumulators (pre-filled: both paths add into them) and the coef words.

Nothing here has a tolerance: both sides run the same arithmetic in the same order, so every word must be equal.

Shapes, per channel width C = 64 / 128 / 512 (cv = C / 8 = 8 / 16 / 64 channel groups); nvec = positions x cv 16-byte vectors:
  * 1 position: nvec = cv, one workgroup of which 256 - cv threads own no element — they must still reach the row reduction's barrier;
  * 256 x 768 -/+ cv vectors (768 workgroups: the reduction grid's cap): the last threads of the sweep idle / the first cv threads take a second trip;
  * 2 x 3 x 3 positions: an odd count, a partly filled workgroup (C = 64, 128) or several (C = 512).
g has about half its entries exactly zero (what a ReLU mask leaves); one channel of each BatchNorm has gamma = 0.
The same cases run once more in a child process under the red-zone allocator of tests/test_gpu_redzone.py; the partial rows are handed over in a
tensor of exactly the advertised size there, so a row too many lands in a red zone."""
import functools
import os

import pytest
import torch

import test_gpu_redzone as RZ

pytestmark = pytest.mark.gpu

GRID_CAP = 768            # norm_act.hip bn_bwd_grid: workgroups of the reduction passes
WIDTHS = (64, 128, 512)


def _positions(C):
    cv = C // 8
    sweep = 256 * GRID_CAP // cv
    return [(1, 1, 1), (sweep - 1, 1, 1), (sweep + 1, 1, 1), (2, 3, 3)]


CASES = [(C, shape) for C in WIDTHS for shape in _positions(C)]
IDS = [f"C{C}-{n}x{h}x{w}" for C, (n, h, w) in CASES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(C, shape):
    """Host tensors of one case (made once, never written)."""
    g = torch.Generator().manual_seed(1000 * C + shape[0])
    full = (*shape, C)
    I = {k: torch.randn(full, generator=g).to(torch.bfloat16) for k in ("c2", "cd")}
    I["g"] = (torch.randn(full, generator=g) * (torch.rand(full, generator=g) < 0.5)).to(torch.bfloat16)
    for b in ("2", "d"):
        I["mean" + b] = torch.randn(C, generator=g) * 0.1
        I["rstd" + b] = torch.rand(C, generator=g) * 1.5 + 0.5
        I["gamma" + b] = torch.randn(C, generator=g) + 1.0
        I["beta" + b] = torch.randn(C, generator=g) * 0.5
        I["dgamma" + b] = torch.randn(C, generator=g)           # what earlier micro-steps left in the accumulators
        I["dbeta" + b] = torch.randn(C, generator=g)
    I["gamma2"][3] = 0.0
    I["gammad"][5] = 0.0
    I["nrows"] = 5                                               # the data-gradient epilogue's partial rows of bn2, as given
    I["stats"] = torch.randn(I["nrows"] * 2 * C, generator=g)
    return I


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    ints = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    diff = int((a.contiguous().view(ints) != b.contiguous().view(ints)).sum())
    assert diff == 0, f"{what}: {diff} of {a.numel()} words differ"


@pytest.mark.parametrize("C,shape", CASES, ids=IDS)
def test_fwd2_has_the_bits_of_the_two_launches(dev, C, shape):
    from syncvsr_amd import ops

    D = {k: v.to(dev) for k, v in _inputs(C, shape).items() if torch.is_tensor(v)}
    idt = ops.bn_act_fwd(D["cd"], None, D["meand"], D["rstdd"], D["gammad"], D["betad"], 0)
    ref = ops.bn_act_fwd(D["c2"], idt, D["mean2"], D["rstd2"], D["gamma2"], D["beta2"], 1)
    y = ops.bn_act_fwd2(D["c2"], D["cd"], D["mean2"], D["rstd2"], D["gamma2"], D["beta2"], D["meand"], D["rstdd"], D["gammad"], D["betad"])
    torch.cuda.synchronize()
    _same(y, ref, "y")
    assert float(ref.float().abs().sum()) > 0 and float((ref == 0).float().mean()) > 0.2          # the ReLU cut something and kept something


@pytest.mark.parametrize("C,shape", CASES, ids=IDS)
def test_bwd_ds_has_the_bits_of_the_launch_chain(dev, C, shape):
    from syncvsr_amd import ops

    I = _inputs(C, shape)
    D = {k: v.to(dev) for k, v in I.items() if torch.is_tensor(v)}
    npix = shape[0] * shape[1] * shape[2]
    cv = C // 8
    rows = ops._query("svsr_bn_act_bwd_rows", npix, C)[0]
    assert rows == min((npix * cv + 255) // 256, GRID_CAP)
    stats = (D["stats"], I["nrows"])

    def fresh():
        return {k: D[k].clone() for k in ("dgamma2", "dbeta2", "dgammad", "dbetad")} | {
            "coef2": torch.full((3 * C,), float("nan"), device=dev), "coefd": torch.full((3 * C,), float("nan"), device=dev)}

    # the chain: bn2 from the given rows, then the 1x1 branch's BatchNorm the long way (reduce, finalise, apply)
    R = fresh()
    dc2_ref = ops.bn_bwd_from_stats(D["g"], D["c2"], D["mean2"], D["rstd2"], D["gamma2"], stats, R["coef2"], R["dgamma2"], R["dbeta2"])
    dcd_ref, _ = ops.bn_act_bwd(D["g"], None, D["cd"], D["meand"], D["rstdd"], D["gammad"], R["coefd"], R["dgammad"], R["dbetad"], 0, False)
    rows_ref = ops.scratch(rows * 2 * C)[: rows * 2 * C].clone()        # what its reduce pass left in this stream's workspace

    # the fold, through the C entry with a row buffer of exactly the advertised size
    N = fresh()
    dc2 = torch.empty_like(D["c2"])
    rows_d = torch.full((rows * 2 * C,), float("nan"), device=dev)
    ops._call("svsr_bn_bwd_from_stats_ds", D["g"].data_ptr(), D["c2"].data_ptr(), D["mean2"].data_ptr(), D["rstd2"].data_ptr(),
              D["gamma2"].data_ptr(), D["stats"].data_ptr(), I["nrows"], N["coef2"].data_ptr(), N["dgamma2"].data_ptr(), N["dbeta2"].data_ptr(),
              dc2.data_ptr(), D["cd"].data_ptr(), D["meand"].data_ptr(), D["rstdd"].data_ptr(), rows_d.data_ptr(), npix, C, ops._stream())
    dcd = ops.bn_bwd_from_stats(D["g"], D["cd"], D["meand"], D["rstdd"], D["gammad"], (rows_d, rows), N["coefd"], N["dgammad"], N["dbetad"])

    # and as the model calls it (rows in the stream's workspace)
    W = fresh()
    dc2_w, d_stats = ops.bn_bwd_from_stats_ds(D["g"], D["c2"], D["mean2"], D["rstd2"], D["gamma2"], stats, W["coef2"], W["dgamma2"], W["dbeta2"],
                                              D["cd"], D["meand"], D["rstdd"])
    dcd_w = ops.bn_bwd_from_stats(D["g"], D["cd"], D["meand"], D["rstdd"], D["gammad"], d_stats, W["coefd"], W["dgammad"], W["dbetad"])
    torch.cuda.synchronize()

    assert d_stats[1] == rows
    _same(rows_d, rows_ref, "partial rows of the 1x1 branch")
    for name, got, got_w, ref in (("dc2", dc2, dc2_w, dc2_ref), ("dcd", dcd, dcd_w, dcd_ref)):
        _same(got, ref, name)
        _same(got_w, ref, name + " (ops wrapper)")
    for k in R:
        _same(N[k], R[k], k)
        _same(W[k], R[k], k + " (ops wrapper)")
        assert bool(torch.isfinite(R[k]).all()), k
    assert not torch.equal(R["dgammad"], D["dgammad"])           # the accumulators were added into, not left alone


def test_null_arguments_are_refused(dev):
    from syncvsr_amd import ops
    from syncvsr_amd._lib import SvsrError

    C = 64
    D = {k: v.to(dev) for k, v in _inputs(C, (2, 3, 3)).items() if torch.is_tensor(v)}
    v, coef = D["mean2"], torch.zeros(3 * C, device=dev)
    with pytest.raises(SvsrError, match="1001"):
        ops.bn_act_fwd2(D["c2"], None, v, v, v, v, v, v, v, v)
    with pytest.raises(SvsrError, match="1001"):
        ops.bn_bwd_from_stats_ds(D["g"], D["c2"], v, v, v, (D["stats"], 5), coef, D["dgamma2"].clone(), D["dbeta2"].clone(), None, v, v)
    with pytest.raises(SvsrError, match="1001"):
        ops.bn_bwd_from_stats_ds(D["g"], D["c2"], v, v, v, (D["stats"], 5), coef, D["dgamma2"].clone(), D["dbeta2"].clone(), D["cd"], None, v)
    torch.cuda.synchronize()


def test_the_cases_pass_with_red_zones_around_every_tensor(dev, monkeypatch):
    """tests/test_gpu_redzone.py's red-zone pass, pointed at this file."""
    if os.environ.get("SVSR_REDZONE") == "1":         # this IS that child process: the cases above have just run under the allocator
        return
    monkeypatch.setattr(RZ, "FILES", [os.path.basename(__file__)])
    RZ.test_kernel_tests_pass_with_red_zones_around_every_tensor()
