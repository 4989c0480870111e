"""-m gpu: the row-wise and element-wise passes past every grid cap and at every width their guards accept.

Every launch below caps, rounds or splits its grid and walks the rest in a stride loop.  Each gets one case just past the cap (the later
trips ragged, the last workgroup partial) with two kinds of assertion: parity with an fp64 torch restatement fed the same bf16-rounded
inputs (tolerance = the one the small-shape test of the same entry point uses, cited where it is applied), and, for outputs that depend on
their own row only, bit equality between the rows a later trip wrote and a second launch on just those rows (a slice that starts on a
16-byte boundary) — no tolerance, so a stride, offset or channel-group slip shows outright.  A column sum over thousands of rows is
additionally allowed 4x the error of a plain fp32 torch sum of the same terms against the fp64 one (another fp32 addition order is as
valid); both figures are printed.

entry point (file)                                   | grid as launched                      | smallest crossing shape       | covered by
-----------------------------------------------------+---------------------------------------+-------------------------------+---------------------------------------
svsr_add_ln_fwd (bert)                               | ceil(R/4), cap 2048, wave per row     | R > 8192                      | test_add_ln_past_the_caps
svsr_add_ln_bwd / _partials / _branch (bert)         | ceil(R/16), cap 512; 8*D*4 B dyn. LDS | R > 8192 (5 trips at 8197)    | test_add_ln_past_the_caps, test_ln_widths (D=2048: 64 KiB)
svsr_embed_ln_fwd (bert)                             | ceil(B*S/4), cap 2048                 | B*S > 8192                    | test_embed_ln_past_the_cap
svsr_embed_bwd_scatter (bert)                        | ceil(S*D/8/256), no cap, loop over B  | -                             | test_embed_ln_past_the_cap (B = 283)
svsr_bias_act_bwd / _partials (bert)                 | col_blocks x splits, splits halved    | N=2048 R>4096; N=5056 R=2400  | test_bias_act_bwd_past_the_split_cap
                                                     |   while the product exceeds 2048      |                               |
svsr_bn_act_fwd (norm_act, ew_grid_for)              | ceil(nvec/256), cap 2048, rounded up  | rows*C/8 > 524,288            | test_bn_act_past_the_caps, test_bn_widths
                                                     |   to a multiple of cv/gcd(cv,256)     |                               |
svsr_bn_act_bwd reduce pass (bn_bwd_grid)            | same, cap 768                         | rows*C/8 > 196,608            | test_bn_act_past_the_caps, test_bn_widths
svsr_bn_act_bwd apply pass, svsr_bn_bwd_from_stats   | same, cap 2048                        | rows*C/8 > 524,288            | test_bn_act_past_the_caps, test_bn_bwd_from_stats_past_the_cap
svsr_bn_finalize / k_bn_bwd_finalize (norm_act)      | C/4 blocks, 64 row lanes walk nrows   | nrows > 64 (> 512: 8-unroll)  | test_bn_act_past_the_caps (768 rows), tests/test_gpu_kernels.py::test_bn_act (135)
svsr_avgpool_fwd / _bwd (norm_act, ew_grid)          | ceil(nvec/256), cap 2048              | N*C/8 > 524,288               | test_avgpool
svsr_ce_fwd / svsr_ce_bwd (loss_optim)               | ceil(R/4), cap 1024 / 2048            | R > 4096 / R > 8192           | test_cross_entropy_past_the_caps
svsr_topk_acc (loss_optim)                           | ceil(B/4), cap 256                    | B > 1024                      | test_topk_past_the_cap_and_ties
svsr_adamw_step / _range, svsr_cast_bf16,            | ceil(n/256), cap 4096 (grid_for)      | n > 1,048,576                 | test_adamw_and_cast_past_the_cap, test_fill_and_clip_prep_past_the_cap
  svsr_fill_f32, svsr_clip_prep (loss_optim)         |                                       |                               |
svsr_grad_sumsq (loss_optim)                         | 1024 blocks fixed, float4 stride loop | n > 1,048,576                 | test_adamw_and_cast_past_the_cap (its clip factor)
svsr_grad_sumsq_parts (loss_optim)                   | nparts blocks                         | n > 1024 * nparts             | tests/test_gpu_kernels.py::test_grad_sumsq_in_ranges
svsr_transpose_cast_multi (loss_optim)               | 128 x entries, tile loop              | > 128 tiles of 32 x 32        | tests/test_gpu_misc.py::test_transpose_cast_multi (1536 x 512: 768 tiles)
svsr_transpose_bf16_multi (loss_optim)               | 128 x entries, tile loop              | > 128 tiles of 64 x 64        | test_transpose_bf16_multi_past_the_tile_cap (192 and 180 tiles, both paths)
svsr_fill_ranges (loss_optim)                        | ceil(longest/4/256), cap 2048         | a range > 2,097,152 floats    | test_fill_ranges_past_the_cap
k_mha_pe_reduce in svsr_mha_bwd and                  | ceil(n/256), cap 1024                 | (2*Lq-1)*H*64 > 262,144       | test_mha_position_gradient_past_the_cap (H=12, T=172; both launch sites)
  svsr_mha_flash_bwd_parts (mha)                     |                                       |                               |
k_row_lse in svsr_ctc_fwd (lrs_misc, grid1d)         | ceil(B*T/4), cap 2048                 | B*T > 8192                    | test_ctc_row_lse_past_the_cap
svsr_ls_loss_fwd / _bwd (lrs_misc, grid1d)           | ceil(R/4), cap 2048                   | R > 8192                      | test_ls_loss_past_the_cap
svsr_embed_pos_fwd (lrs_misc, grid1d)                | ceil(R*D/8/256), cap 2048             | R*D/8 > 524,288               | test_embed_pos_fwd_past_the_cap
svsr_scale_bf16 (lrs_misc, grid1d)                   | ceil(n/8/256), cap 2048               | n > 4,194,304                 | test_scale_bf16_past_the_cap, test_add_ln_past_the_caps (mask, 6.3 M elements)
k_dw_reduce in svsr_glu_dwconv_bwd (lrs_misc)        | ceil(D*(K+1)/256), cap 256            | D*(K+1) > 65,536: D >= 2112   | test_glu_dwconv_bwd_past_the_reduce_cap (the width is the model's, not the batch's:
                                                     |                                       |   at K = 31                   |   no data-loader change gets there, the case only pins the loop)
svsr_colsum_rows / _multi (runtime)                  | ceil(n/CL) blocks, CL = 256/32/8/1    | nrows > 8 * (256/CL): 8-way   | through its callers here: CE mean (8197 rows, 1 column), top-k (1029 x 2), ls_loss
                                                     |   picked from nrows and n; 256/CL row |   unrolled trip, then 4-way   |   (8197 x 3), LN / bias / embed partial rows (512 x 1536, 129 x 2048, 30 x 512);
                                                     |   lanes walk the rows, no cap         |   and single-row tails        |   shape classes: tests/test_gpu_kernels.py::test_colsum_rows_multi_equals_separate_launches
svsr_rmsnorm_bwd (xt)                                | ceil(R/16) blocks, ceil(R/32) from    | R >= 4096 (rows-per-block     | tests/test_gpu_xt.py::test_rmsnorm_forward_backward[513-576-4100]
                                                     |   R = 4096 on; rows walked in a loop  |   switch; no cap)             |
svsr_stem_conv_fwd, svsr_stem_conv_wgrad,            | ceil(Ho*Wo/128)*B*T tiles, cap 768;   | B*T > 768 one-tile frames;    | tests/test_gpu_stem_edges.py (5 x 157 frames of 12 x 8: 785 tiles, 1,570 row groups;
  svsr_stem_bwd_wgrad (stem)                         |   ceil(Ho/4)*B*T row groups, cap 512  |   B*T*ceil(Ho/4) > 512        |   exact integer / impulse cases, every workgroup's partial row)
persistent GEMM-class kernels (conv3x3_c64,          | one workgroup per CU-slot, tile loop  | more tiles than workgroups    | tests/test_gpu_bench_shapes.py, tests/test_gpu_kernels.py (out of scope here:
  wgrad3x3, igemm_p8)                                |                                       |                               |   the contraction kernels have their own shape tests)
the other launches of xt and runtime; w2v_codec,     | ceil(n/block) or one block per item:  | -                             | nothing to cross
  audio_head, lrs_lm, lrs_search, dctcn, enc_fused,  |   no cap, no stride loop              |                               |
  steplist                                           |                                       |                               |

What the assertions were seen to catch (each mistake built once into a copy of the library, this module run once against it):
  * LayerNorm row stride `gridDim.x * 4 - 1` in k_add_ln_fwd and k_add_ln_bwd: in the forward the mistake is harmless (every row is still
    visited, a few twice, with the same result) and no forward assertion fails; in the backward rows 2047, 4094, 6141 and 8188 are added twice,
    which changes dgamma / dbeta by 4 rows in 8197 - too little for an exact-slice check (ds is right) and marginal for the column-sum bound.
    The per-workgroup partial-row check of test_add_ln_past_the_caps is there for this: all three cases failed at it (max error 21 of a scale
    of 22, rel L2 0.86).
  * ew_grid_for without its round-up: test_bn_act_past_the_caps and test_bn_bwd_from_stats_past_the_cap failed at 5500 x 768 (forward / dx
    parity, rel L2 2.3e-2 to 3.6e-2 against 5e-3 to 8e-3: the second trip reads other channels' parameters), and the nine test_bn_widths cases
    at C = 40, 520, 1096 at their workgroup-count assertion; C = 64 and C = 8, 2048 need no rounding and passed.

Tie rule of svsr_topk_acc (a finding, see test_topk_past_the_cap_and_ties): the kernel counts the classes that beat the label as
"strictly greater, or equal with a lower index", i.e. the lowest index wins a tie — what a stable descending sort and torch.argmax give.
torch.topk, which the reference metric calls (LRW lightning.py:177-183, restated in oracle/lrw_oracle.py), leaves the order of equal
values unspecified: on the CPU (2.10) its partial sort put the lowest index first in only 29 % of 2,000 rows of a 7-valued grid over 500
classes, and the CUDA/ROCm radix select orders them differently again.  There is no rule to copy, so the kernel keeps its deterministic
one; the test compares with torch.topk wherever the outcome does not depend on the order of equal values (that includes rows whose label
ties with other classes inside or outside the top five) and asserts the lowest-index rule on the rows where it does.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF)


def rndf(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def errs(got, ref):
    got = got.detach().cpu().to(F64)
    ref = ref.detach().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values"
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    l2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    return err, scale, l2


def check(got, ref, name, max_tol=1.5e-2, l2_tol=6e-3):
    """tests/test_gpu_kernels.py::check with an fp64 reference: max-abs error <= max_tol * max|ref| and relative L2 error <= l2_tol."""
    err, scale, l2 = errs(got, ref)
    print(f"{name}: max err {err:.3e} (scale {scale:.3e}), rel L2 {l2:.3e}")
    assert err <= max_tol * scale and l2 <= l2_tol, f"{name}: max err {err:.3e} (scale {scale:.3e}), rel L2 {l2:.3e}"


def rel_err(a, b):
    """tests/test_gpu_lrs_kernels.py::_rel_err"""
    a, b = a.detach().cpu().to(F64).flatten(), b.detach().to(F64).flatten()
    return float((a - b).norm() / (b.norm() + 1e-12))


def check_rel(got, ref, name, tol):
    e = rel_err(got, ref)
    print(f"{name}: rel L2 {e:.3e}")
    assert e < tol, f"{name}: rel L2 {e:.3e} (bound {tol:.1e})"


def check_colsum(got, terms, name, max_tol, l2_tol):
    """A column sum of `terms` (fp64, [rows][n]) over thousands of rows: the small-shape tolerance (max_tol, l2_tol), or 4x the error a plain fp32
    torch sum of the same terms makes against the fp64 one, whichever is larger."""
    ref = terms.sum(0)
    e32 = (terms.float().sum(0).to(F64) - ref).abs().max().item()
    err, scale, l2 = errs(got, ref)
    print(f"{name}: kernel max err {err:.3e}, torch fp32 sum max err {e32:.3e} (scale {scale:.3e}, {terms.shape[0]} rows), rel L2 {l2:.3e}")
    # (either bound admits: the effective one is the looser of the two in both clauses.  At the shapes here max_tol * scale is ~1e4 times 4 * e32,
    # so the small-shape tolerance is what decides, and a slip that changes a sum by a few rows in thousands can pass it: the tests that must see
    # single rows check partial rows or exact slices instead.)
    assert err <= max(max_tol * scale, 4.0 * e32) and (l2 <= l2_tol or err <= 4.0 * e32), \
        f"{name}: max err {err:.3e} vs fp32 sum {e32:.3e} (scale {scale:.3e}), rel L2 {l2:.3e}"


def raises_arg_error(fn):
    """The entry point refuses the shape with SVSR_ERR_ARG (1001) before any launch."""
    from syncvsr_amd._lib import SvsrError

    with pytest.raises(SvsrError, match="1001"):
        fn()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
def ln_ref(a, r, gamma, beta, eps, dy=None, addend=None):
    """fp64 closed form of y = LN(a + r) * gamma + beta and of its backward."""
    x = a.to(F64) + (r.to(F64) if r is not None else 0.0)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rs
    out = {"y": xh * gamma.to(F64) + beta.to(F64), "mean": mu.flatten(), "rstd": rs.flatten()}
    if dy is not None:
        d = dy.to(F64)
        gd = d * gamma.to(F64)
        m1 = gd.mean(1, keepdim=True)
        m2 = (gd * xh).mean(1, keepdim=True)
        ds = rs * (gd - m1 - xh * m2)
        out["ds"] = ds + (addend.to(F64) if addend is not None else 0.0)
        out["dgamma_terms"] = d * xh
        out["dbeta_terms"] = d
    return out


LN_EPS = 1e-12


@pytest.mark.parametrize("case", ["r512", "addend768", "branch768"])
def test_add_ln_past_the_caps(dev, case):
    """R = 8197: the forward (2048 workgroups x 4 rows) takes a second, 5-row trip; the backward (512 workgroups x 4 rows) takes five trips, its
    per-wave dgamma/dbeta accumulators carried across them."""
    from syncvsr_amd import ops

    R = 8197
    D = 512 if case == "r512" else 768
    a = rnd((R, D), 160)
    r = rnd((R, D), 161) if case == "r512" else None
    addend = None if case == "r512" else rnd((R, D), 164)
    gamma, beta = 1 + 0.2 * rndf(D, 162), 0.2 * rndf(D, 163)
    dy = rnd((R, D), 165)
    ref = ln_ref(a, r, gamma, beta, LN_EPS, dy, addend)
    ad, rd, dyd = a.to(dev), (None if r is None else r.to(dev)), dy.to(dev)
    add = None if addend is None else addend.to(dev)
    gd, bd = gamma.to(dev), beta.to(dev)

    y, mean, rstd = ops.add_ln_fwd(ad, rd, gd, bd, LN_EPS)
    if case == "r512":
        check(y, ref["y"], "add_ln_fwd.y")                        # test_gpu_kernels.py::test_add_ln_and_embed: check(y, yref) defaults
    else:
        check_rel(y, ref["y"], "add_ln_fwd.y (D=768)", 4e-3)      # test_gpu_lrs_kernels.py::test_ln768_pre_norm_and_relu_alpha_epilogues: < 4e-3
    check(mean, ref["mean"], "add_ln_fwd.mean", 1e-3, 1e-3)       # fp32 statistics: test_gpu_kernels.py::test_bn_act's bound for mean / rstd
    check(rstd, ref["rstd"], "add_ln_fwd.rstd", 1e-3, 1e-3)
    # the second trip (rows 8192..8196) on its own
    t0 = 2048 * 4
    y2, mean2, rstd2 = ops.add_ln_fwd(ad[t0:], None if rd is None else rd[t0:], gd, bd, LN_EPS)
    assert torch.equal(y2, y[t0:]) and torch.equal(mean2, mean[t0:]) and torch.equal(rstd2, rstd[t0:])

    assert ops._query("svsr_add_ln_bwd_rows", R)[0] == 512         # (ln_bwd_grid at the default rows-per-workgroup setting: the cap)
    b0 = 512 * 4                                                   # trips 2..5 of the backward
    # which rows a workgroup visits, outright: its partial [dgamma | dbeta] row (a sum of 16 or 20 rows) against the fp64 sum over exactly the rows
    # b * 4 + wave + 2048 * trip it owns.  One wrong or doubled row in a workgroup is an error of the order of the sum itself, not of 1 / R as in
    # the column sums below.  Bounds: test_add_ln_and_embed's for dgamma / dbeta (1e-2, 6e-3).
    later = []
    ds_d = ops.add_ln_bwd(dyd, ad, rd, gd, mean, rstd, torch.zeros(D, device=dev), torch.zeros(D, device=dev), addend=add, defer=later)
    part = later[0][1].view(512, 2, D)

    def owned(terms):
        padded = torch.cat((terms, torch.zeros(5 * 2048 - R, D, dtype=F64)))
        return padded.view(5, 512, 4, D).sum((0, 2))

    check(part[:, 0], owned(ref["dgamma_terms"]), "ln.dgamma partial rows", 1e-2, 6e-3)
    check(part[:, 1], owned(ref["dbeta_terms"]), "ln.dbeta partial rows", 1e-2, 6e-3)
    if case != "branch768":
        dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        ds = ops.add_ln_bwd(dyd, ad, rd, gd, mean, rstd, dg, db, addend=add)
        assert torch.equal(ds, ds_d)
        if case == "r512":
            check(ds, ref["ds"], "add_ln_bwd.ds", 2e-2, 8e-3)      # test_add_ln_and_embed: 2e-2, 8e-3
            check_colsum(dg, ref["dgamma_terms"], "ln.dgamma", 1e-2, 6e-3)      # test_add_ln_and_embed: 1e-2, 6e-3
            check_colsum(db, ref["dbeta_terms"], "ln.dbeta", 1e-2, 6e-3)
        else:
            check_rel(ds, ref["ds"], "add_ln_bwd.ds (D=768, addend)", 6e-3)     # test_ln768...: ds < 6e-3, dgamma / dbeta < 5e-3
            check_colsum(dg, ref["dgamma_terms"], "ln.dgamma (D=768)", 1e-2, 5e-3)
            check_colsum(db, ref["dbeta_terms"], "ln.dbeta (D=768)", 1e-2, 5e-3)
        dg2, db2 = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        ds_s = ops.add_ln_bwd(dyd[b0:], ad[b0:], None if rd is None else rd[b0:], gd, mean[b0:], rstd[b0:], dg2, db2,
                              addend=None if add is None else add[b0:])
        assert torch.equal(ds_s, ds[b0:])
        return
    # the residual branch's gradient as a second output (svsr_add_ln_bwd_branch)
    seed = torch.tensor([12345], dtype=torch.int32, device=dev)
    dg0, db0 = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    ds0 = ops.add_ln_bwd(dyd, ad, None, gd, mean, rstd, dg0, db0, addend=add)
    for alpha, drop in ((0.5, (seed, 77, 0.1)), (0.5, None)):
        dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        later = []
        ds, br = ops.add_ln_bwd(dyd, ad, None, gd, mean, rstd, dg, db, addend=add, defer=later, branch=(alpha, drop))
        for fn, _ in later:
            fn()
        assert torch.equal(ds, ds0) and torch.equal(dg, dg0) and torch.equal(db, db0)
        check_rel(ds, ref["ds"], "add_ln_bwd_branch.ds", 6e-3)
        # the mask is drawn from the element index in the whole tensor: compared with svsr_scale_bf16 of the whole ds, as test_ln768... does
        assert torch.equal(br, ops.scale_bf16(ds, alpha, drop=drop))
        if drop is not None:
            for lo, hi in ((0, b0), (b0, R)):                      # the mask is live in the first trip and in the later ones alike
                assert 0.07 < float((br[lo:hi] == 0).float().mean()) < 0.13
        else:
            check_rel(br, 0.5 * ds.float().cpu().to(F64), "add_ln_bwd_branch.ds2", 1e-6)     # test_ln768...: scale < 1e-6 (a power of two: exact)
            dg2, db2 = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
            later = []
            ds_s, br_s = ops.add_ln_bwd(dyd[b0:], ad[b0:], None, gd, mean[b0:], rstd[b0:], dg2, db2, addend=add[b0:], defer=later,
                                        branch=(alpha, None))
            assert torch.equal(ds_s, ds[b0:]) and torch.equal(br_s, br[b0:])


def test_embed_ln_past_the_cap(dev):
    """B * S = 8490 rows: svsr_embed_ln_fwd's second trip starts inside sequence 273; svsr_embed_bwd_scatter sums 283 clips per thread."""
    from syncvsr_amd import ops

    B, S, D = 283, 30, 512
    R = B * S
    feats = rnd((B * (S - 1), D), 170)
    gamma, beta = 1 + 0.2 * rndf(D, 171), 0.2 * rndf(D, 172)
    cls, pos, typ = rndf(D, 173), 0.02 * rndf((32, D), 174), 0.02 * rndf((2, D), 175)
    e = torch.cat((cls.to(BF).to(F64).view(1, 1, D).expand(B, 1, D), feats.to(F64).view(B, S - 1, D)), 1) + pos[:S].to(F64) + typ[0].to(F64)
    e = e.view(R, D)
    fd, gd, bd = feats.to(dev), gamma.to(dev), beta.to(dev)
    cd, pd, td = cls.to(dev), pos.to(dev).reshape(-1), typ.to(dev).reshape(-1)
    s0, y0, m0, r0 = ops.embed_ln_fwd(fd, cd, pd, td, gd, bd, B, S, D, LN_EPS)
    check(s0, e, "embed.sum")                                      # test_add_ln_and_embed: defaults / 2e-2, 8e-3
    ref = ln_ref(s0.float().cpu(), None, gamma, beta, LN_EPS)       # the kernel normalises the bf16-rounded sum it stores
    check(y0, ref["y"], "embed.ln", 2e-2, 8e-3)
    check(m0, ref["mean"], "embed.mean", 1e-3, 1e-3)
    check(r0, ref["rstd"], "embed.rstd", 1e-3, 1e-3)
    b1 = 274                                                       # first whole sequence behind the second trip's start (row 8192 is in sequence 273)
    s1, y1, m1, r1 = ops.embed_ln_fwd(fd[b1 * (S - 1):], cd, pd, td, gd, bd, B - b1, S, D, LN_EPS)
    assert torch.equal(s1, s0[b1 * S:]) and torch.equal(y1, y0[b1 * S:]) and torch.equal(m1, m0[b1 * S:]) and torch.equal(r1, r0[b1 * S:])

    ds0 = rnd((R, D), 176)
    dcls, dpos, dtyp = torch.zeros(D, device=dev), torch.zeros(32 * D, device=dev), torch.zeros(2 * D, device=dev)
    dfe = ops.embed_bwd_scatter(ds0.to(dev), dcls, dpos, dtyp, B, S, D)
    d3 = ds0.to(F64).view(B, S, D)
    check(dfe, d3[:, 1:].reshape(-1, D), "embed.dfeats", 1e-6, 1e-6)            # test_add_ln_and_embed: 1e-6 / 1e-3
    check_colsum(dcls, d3[:, 0], "embed.dcls", 1e-3, 1e-3)
    check_colsum(dpos.view(32, D)[:S].reshape(-1), d3.reshape(B, S * D), "embed.dpos", 1e-3, 1e-3)
    assert float(dpos.view(32, D)[S:].abs().max()) == 0.0
    check_colsum(dtyp.view(2, D)[0], d3.reshape(R, D), "embed.dtype", 1e-3, 1e-3)


@pytest.mark.parametrize("D", [8, 264, 520, 1096, 2048])
def test_ln_widths(dev, D):
    """'any D % 8 == 0 up to 2048': one to four 512-column groups per lane, the last one partly filled; D = 2048 backward is the launch with
    exactly 64 KiB of dynamic LDS."""
    from syncvsr_amd import ops

    R = 37
    a, r, addend, dy = rnd((R, D), 180), rnd((R, D), 181), rnd((R, D), 182), rnd((R, D), 183)
    gamma, beta = 1 + 0.2 * rndf(D, 184), 0.2 * rndf(D, 185)
    ref = ln_ref(a, r, gamma, beta, LN_EPS, dy, addend)
    y, mean, rstd = ops.add_ln_fwd(a.to(dev), r.to(dev), gamma.to(dev), beta.to(dev), LN_EPS)
    check(y, ref["y"], f"add_ln_fwd.y D={D}")                     # test_add_ln_and_embed's bounds throughout
    check(mean, ref["mean"], "mean", 1e-3, 1e-3)
    check(rstd, ref["rstd"], "rstd", 1e-3, 1e-3)
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    ds = ops.add_ln_bwd(dy.to(dev), a.to(dev), r.to(dev), gamma.to(dev), mean, rstd, dg, db, addend=addend.to(dev))
    torch.cuda.synchronize()
    check(ds, ref["ds"], f"add_ln_bwd.ds D={D}", 2e-2, 8e-3)
    check(dg, ref["dgamma_terms"].sum(0), "ln.dgamma", 1e-2, 6e-3)
    check(db, ref["dbeta_terms"].sum(0), "ln.dbeta", 1e-2, 6e-3)


@pytest.mark.parametrize("D", [2056, 12])
def test_ln_rejects_widths_outside_its_claim(dev, D):
    from syncvsr_amd import ops

    R = 5
    a = torch.zeros((R, D), dtype=BF, device=dev)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    mean, rstd = torch.zeros(R, device=dev), torch.ones(R, device=dev)
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    raises_arg_error(lambda: ops.add_ln_fwd(a, None, gamma, beta, LN_EPS))
    raises_arg_error(lambda: ops.add_ln_bwd(a, a, None, gamma, mean, rstd, dg, db))
    raises_arg_error(lambda: ops.add_ln_bwd(a, a, None, gamma, mean, rstd, dg, db, defer=[]))
    assert float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# bias / activation backward
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _bias_case(R, N, relu):
    dy, z = rnd((R, N), 190), rnd((R, N), 191)
    zz = z.to(F64)
    if relu:
        grad = (zz > 0).to(F64)
    else:
        grad = 0.5 * (1.0 + torch.erf(zz / math.sqrt(2.0))) + zz * torch.exp(-0.5 * zz * zz) / math.sqrt(2.0 * math.pi)
    return dy, z, dy.to(F64) * grad


@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("R,N,n_valid", [(4101, 2048, 2048), (2400, 5056, 5049)])
def test_bias_act_bwd_past_the_split_cap(dev, R, N, n_valid, relu, with_db):
    """Both shapes halve `splits` (257 -> 129 slabs of 32 rows at N = 2048; 150 -> 75 at N = 5056): every workgroup walks its slab in two trips of
    16 rows, the last slab is ragged (5 rows / 32 rows), and at N = 5056 the last column block is partial with 7 columns outside n_valid."""
    from syncvsr_amd import ops

    assert ops._query("svsr_bias_act_bwd_rows", R, N)[0] == {4101: 129, 2400: 75}[R]
    dy, z, dz_ref = _bias_case(R, N, relu)
    dyd, zd = dy.to(dev), z.to(dev)
    db = torch.full((N,), 0.25, device=dev) if with_db else None
    dz = ops.bias_act_bwd(dyd, zd, db, R=R, N=N, n_valid=n_valid, ld=N, relu=relu)
    if relu:
        check_rel(dz, dz_ref, "relu_bwd.dz", 1e-6 + 4e-3)        # test_ln768_pre_norm_and_relu_alpha_epilogues: dz < 1e-6 + 4e-3, dbias < 4e-3
    else:
        check(dz, dz_ref, "gelu_bwd.dz")                          # test_gpu_kernels.py::test_linear_variants: check(dz, ...) defaults; bias_grad 1e-2, 6e-3
    if with_db:
        got = db.cpu() - 0.25
        assert float(got[n_valid:].abs().max() if n_valid < N else 0.0) == 0.0
        check_colsum(got[:n_valid], dz_ref[:, :n_valid], "bias_grad", 1e-2, 4e-3 if relu else 6e-3)
    # rows from an odd offset on (another slab partition, every row in another trip): dz is a function of its own row
    r0 = R // 2 + 3
    dz_s = ops.bias_act_bwd(dyd[r0:], zd[r0:], None, R=R - r0, N=N, n_valid=n_valid, ld=N, relu=relu)
    assert torch.equal(dz_s, dz[r0:])


# ---------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + activation (+ residual)
# ---------------------------------------------------------------------------------------------------------------------------------------
def bn_inputs(rows, C, use_res, seed):
    x = (rnd((rows, C), seed, 2.0).float() + 0.3).to(BF)
    res = rnd((rows, C), seed + 1) if use_res else None
    gamma, beta = 1 + 0.2 * rndf(C, seed + 2), 0.2 * rndf(C, seed + 3)
    dy = rnd((rows, C), seed + 4)
    xd = x.to(F64)
    mean = xd.mean(0).float()
    rstd = (1.0 / torch.sqrt(xd.var(0, unbiased=False) + 1e-5)).float()
    return x, res, gamma, beta, dy, mean, rstd


def bn_fwd_ref(x, res, gamma, beta, mean, rstd, act):
    """fp64, from the fp32 mean / rstd the kernel is handed"""
    xh = (x.to(F64) - mean.to(F64)) * rstd.to(F64)
    z = xh * gamma.to(F64) + beta.to(F64) + (res.to(F64) if res is not None else 0.0)
    y = torch.relu(z) if act == 1 else (z * torch.sigmoid(z) if act == 2 else z)
    return xh, z, y


def bn_bwd_ref(g, xh, gamma, rstd):
    """g: the gradient at the BatchNorm output (activation derivative applied): dx, and the terms of dgamma / dbeta"""
    k0 = (gamma.to(F64) * rstd.to(F64))
    return k0 * (g - g.mean(0) - xh * (g * xh).mean(0)), g * xh, g


def run_bn_case(dev, rows, C, act, use_res, big):
    from syncvsr_amd import ops

    x, res, gamma, beta, dy, mean, rstd = bn_inputs(rows, C, use_res, 200)
    xh, z, yref = bn_fwd_ref(x, res, gamma, beta, mean, rstd, act)
    shp = (rows, 1, 1, C)
    xd, dyd = x.to(dev).view(shp), dy.to(dev).view(shp)
    rsd = None if res is None else res.to(dev).view(shp)
    md, rd, gd, bd = mean.to(dev), rstd.to(dev), gamma.to(dev), beta.to(dev)
    y = ops.bn_act_fwd(xd, rsd, md, rd, gd, bd, act)
    if act == 2:
        check_rel(y.view(rows, C), yref, "bn_swish_fwd", 5e-3)    # test_gpu_lrs_kernels.py::test_bn_swish: y < 5e-3, dx < 1e-2, dgamma / dbeta / dres < 6e-3
    else:
        check(y.view(rows, C), yref, "bn_act_fwd")                # test_gpu_kernels.py::test_bn_act: y defaults, dx 2e-2 / 8e-3, dgamma / dbeta 1e-2 / 6e-3
    # the backward's ReLU mask is the saved (bf16) output's sign; the Swish derivative is recomputed from x
    if act == 1:
        g = dy.to(F64) * (y.view(rows, C).float().cpu() > 0).to(F64)
    elif act == 2:
        s = torch.sigmoid(z)
        g = dy.to(F64) * (s * (1.0 + z * (1.0 - s)))
    else:
        g = dy.to(F64)
    dx_ref, dg_terms, db_terms = bn_bwd_ref(g, xh, gamma, rstd)
    coef = torch.empty(3 * C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dx, dres = ops.bn_act_bwd(dyd, y if act == 1 else None, xd, md, rd, gd, coef, dg, db, act, use_res, beta=bd if act == 2 else None,
                              res=rsd if act == 2 else None)
    torch.cuda.synchronize()
    if act == 2:
        check_rel(dx.view(rows, C), dx_ref, "bn_swish_bwd.dx", 1e-2)
        check_colsum(dg, dg_terms, "bn.dgamma", 1e-2, 6e-3)
        check_colsum(db, db_terms, "bn.dbeta", 1e-2, 6e-3)
        if use_res:
            check_rel(dres.view(rows, C), g, "bn_swish_bwd.dres", 6e-3)
    else:
        check(dx.view(rows, C), dx_ref, "bn_act_bwd.dx", 2e-2, 8e-3)
        check_colsum(dg, dg_terms, "bn.dgamma", 1e-2, 6e-3)
        check_colsum(db, db_terms, "bn.dbeta", 1e-2, 6e-3)
        if use_res:
            check(dres.view(rows, C), g, "bn.dres")
    if not big:
        return
    # rows the second trip of the forward / apply passes wrote (2048 x 256 vectors and on; 2049 workgroups at C = 768), on their own; the start is a
    # whole row, so every thread of the second launch meets the channel group it computed its scale and shift for
    cv = C // 8
    m = cv // math.gcd(cv, 256)
    grid = -(-2048 // m) * m
    r0 = -(-grid * 256 // cv)
    assert 0 < r0 < rows
    y_s = ops.bn_act_fwd(xd[r0:], None if rsd is None else rsd[r0:], md, rd, gd, bd, act)
    assert torch.equal(y_s, y[r0:])
    if use_res:         # dres = the masked gradient: no batch statistic enters it
        coef2 = torch.empty(3 * C, device=dev)
        _, dres_s = ops.bn_act_bwd(dyd[r0:], y[r0:] if act == 1 else None, xd[r0:], md, rd, gd, coef2, torch.zeros(C, device=dev),
                                   torch.zeros(C, device=dev), act, True, beta=bd if act == 2 else None, res=rsd[r0:] if act == 2 else None)
        assert torch.equal(dres_s, dres[r0:])


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("rows,C", [(66000, 64), (5500, 768)])
def test_bn_act_past_the_caps(dev, rows, C, act, use_res):
    """528,000 vectors of 8 channels: the forward / apply passes (cap 2048 workgroups; 2049 at C = 768, rounded up to a multiple of 3) take a ragged
    second trip, the reduce pass (cap 768) a third one."""
    from syncvsr_amd import ops

    assert ops._query("svsr_bn_act_bwd_rows", rows, C)[0] == 768
    run_bn_case(dev, rows, C, act, use_res, big=True)


@pytest.mark.parametrize("rows,C", [(66000, 64), (5500, 768)])
def test_bn_bwd_from_stats_past_the_cap(dev, rows, C):
    """svsr_bn_bwd_from_stats (the apply pass behind a data-gradient epilogue's partial sums): parity, and the last rows of the second trip again
    from a launch of their own that is handed the same coefficients."""
    from syncvsr_amd import ops

    x, _, gamma, _, g16, mean, rstd = bn_inputs(rows, C, False, 210)
    xh = (x.to(F64) - mean.to(F64)) * rstd.to(F64)
    g = g16.to(F64)
    dx_ref, dg_terms, db_terms = bn_bwd_ref(g, xh, gamma, rstd)
    nrows = 7                                                      # partial rows {sum g, sum g * xhat} as a producer's epilogue would leave them
    part = torch.stack([torch.stack((db_terms[i::nrows].sum(0), dg_terms[i::nrows].sum(0))) for i in range(nrows)]).float()
    shp = (rows, 1, 1, C)
    xd, gdv = x.to(dev).view(shp), g16.to(dev).view(shp)
    md, rd, gam = mean.to(dev), rstd.to(dev), gamma.to(dev)
    coef = torch.empty(3 * C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dx = ops.bn_bwd_from_stats(gdv, xd, md, rd, gam, (part.reshape(-1).to(dev), nrows), coef, dg, db)
    check(dx.view(rows, C), dx_ref, "bn_bwd_from_stats.dx", 2e-2, 8e-3)        # test_gpu_kernels.py::test_bn_act: dx 2e-2 / 8e-3, dgamma / dbeta 1e-2 / 6e-3
    check(dg, dg_terms.sum(0), "bn.dgamma", 1e-2, 6e-3)
    check(db, db_terms.sum(0), "bn.dbeta", 1e-2, 6e-3)
    # a power-of-two row count makes sum = coef * count exact, so the finaliser of the second launch returns the same coef bit for bit
    n2 = 256 if C == 64 else 32
    r0 = rows - n2
    assert r0 * (C // 8) >= (2048 if C == 64 else 2049) * 256     # inside the second trip
    one = torch.stack((coef[C:2 * C] * n2, coef[2 * C:] * n2)).reshape(-1).contiguous()
    coef2 = torch.empty(3 * C, device=dev)
    dx_s = ops.bn_bwd_from_stats(gdv[r0:], xd[r0:], md, rd, gam, (one, 1), coef2, torch.zeros(C, device=dev), torch.zeros(C, device=dev))
    assert torch.equal(coef2, coef)
    assert torch.equal(dx_s, dx[r0:])


@pytest.mark.parametrize("act,use_res", [(1, True), (2, True), (0, False)])
@pytest.mark.parametrize("rows,C", [(40, 8), (40, 40), (37, 520), (3, 1096), (9, 2048)])
def test_bn_widths(dev, rows, C, act, use_res):
    """'any C % 8 == 0 up to 2048' (chan_ok_any): C/8 = 1, 5, 65, 137, 256.  The rows are chosen so that rounding the grid up to a multiple of
    cv / gcd(cv, 256) changes it (1 -> 5, 10 -> 65, 2 -> 137 workgroups): most workgroups then have no vector and still own a partial row."""
    from syncvsr_amd import ops

    want = {8: 1, 40: 5, 520: 65, 1096: 137, 2048: 9}[C]
    assert ops._query("svsr_bn_act_bwd_rows", rows, C)[0] == want
    run_bn_case(dev, rows, C, act, use_res, big=False)


@pytest.mark.parametrize("C", [2056, 12])
def test_bn_rejects_widths_outside_its_claim(dev, C):
    from syncvsr_amd import ops

    x = torch.zeros((4, 1, 1, C), dtype=BF, device=dev)
    v = torch.ones(C, device=dev)
    coef = torch.empty(3 * C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    assert ops._query("svsr_bn_act_bwd_rows", 4, C)[0] == 0
    raises_arg_error(lambda: ops.bn_act_fwd(x, None, v, v, v, v, 1))
    raises_arg_error(lambda: ops.bn_act_bwd(x, x, x, v, v, v, coef, dg, db, 1, False))
    raises_arg_error(lambda: ops.bn_bwd_from_stats(x, x, v, v, v, (torch.zeros(2 * C, device=dev), 1), coef, dg, db))
    assert float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


@pytest.mark.parametrize("N,H,W,C", [(8197, 3, 3, 512), (5, 1, 1, 512), (3, 6, 6, 64)])
def test_avgpool(dev, N, H, W, C):
    """N * C/8 = 524,608 output vectors: 320 past the forward's 2048 x 256; the backward walks nine times as many."""
    from syncvsr_amd import ops

    x = rnd((N, H, W, C), 220)
    y = ops.avgpool_fwd(x.to(dev))
    check(y, x.view(N, H * W, C).to(F64).mean(1), "avgpool_fwd")       # test_gpu_kernels.py::test_avgpool: defaults for both
    dy = rnd((N, C), 221)
    dx = ops.avgpool_bwd(dy.to(dev), (N, H, W, C))
    ref = (dy.to(F64) / (H * W)).to(torch.float32)
    check(dx.view(N, H * W, C), ref.view(N, 1, C).expand(N, H * W, C), "avgpool_bwd")
    assert torch.equal(dx.view(N, H * W, C), dx.view(N, H * W, C)[:, :1].expand(N, H * W, C))      # every pixel of a clip gets the same vector


# ---------------------------------------------------------------------------------------------------------------------------------------
# losses, metric
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bf16_hard", "f32_soft"])
def test_cross_entropy_past_the_caps(dev, case):
    """bf16 logits, class indices, R = 8197: three trips of the forward (cap 1024 x 4 rows), two of the backward (2048 x 4).
    fp32 logits, probability targets, label smoothing 0.1, R = 4101, C = 500 into a 512-column gradient: a 5-row second trip of the forward."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(230)
    if case == "bf16_hard":
        R, V, ldo, smoothing, gout = 8197, 320, 320, 0.0, 3.0
        logits = (torch.randn(R, V, generator=g) * 2).to(BF)
        tgt = torch.randint(0, V, (R,), generator=g)
        prob = F.one_hot(tgt, V).to(F64)
        tgt_d, prob_d = tgt.to(dev), None
        n2 = 4096                                                  # rows of the launch that repeats the later trips: a power of two (see below)
    else:
        R, V, ldo, smoothing, gout = 4101, 500, 512, 0.1, 1.0
        logits = torch.randn(R, V, generator=g) * 3
        hard = torch.randint(0, V, (R,), generator=g)
        soft = torch.zeros(R, V)
        soft[torch.arange(R), hard] = 0.7
        soft[torch.arange(R), (hard + 5) % V] += 0.3
        prob = soft.to(F64)
        tgt_d, prob_d = None, soft.to(dev)
        n2 = 2048
    z = logits.to(F64)
    lse_ref = torch.logsumexp(z, 1)
    t = prob * (1.0 - smoothing) + smoothing / V
    loss_ref = -(t * (z - lse_ref[:, None])).sum(1).mean()
    dl_ref = gout / R * (torch.exp(z - lse_ref[:, None]) * t.sum(1, keepdim=True) - t)
    ld_ = logits.to(dev)
    loss, lse = ops.ce_fwd(ld_, V, tgt_d, prob_d, R, V, smoothing)
    check(loss, loss_ref, "ce.loss", 1e-5, 1e-5)                  # test_gpu_kernels.py::test_cross_entropy_and_topk: loss 1e-5, dlogits defaults
    check(lse, lse_ref, "ce.lse", 2e-5, 1e-5)                     # test_gpu_kernels.py::test_fused_audio_head: lse 2e-5, 1e-5
    gout_d = torch.tensor(gout, device=dev)
    dl = torch.full((R, ldo), float("nan"), dtype=BF, device=dev)
    ops.ce_bwd(ld_, V, tgt_d, prob_d, R, V, smoothing, lse, gout_d, dl, ldo)
    check(dl[:, :V], dl_ref, "ce.dlogits")
    if ldo > V:
        assert float(dl[:, V:].float().abs().max()) == 0.0
    # the last n2 rows (every row of the later trips among them) from launches of their own.  dlogits carries gout / R: with n2 a power of two,
    # gout' = fl(gout / R) * n2 gives the second launch the same factor bit for bit.
    r0 = R - n2
    _, lse_s = ops.ce_fwd(ld_[r0:], V, None if tgt_d is None else tgt_d[r0:], None if prob_d is None else prob_d[r0:], n2, V, smoothing)
    assert torch.equal(lse_s, lse[r0:])
    gout_s = (torch.tensor(gout, dtype=torch.float32) / torch.tensor(float(R), dtype=torch.float32)) * n2
    dl_s = torch.empty((n2, ldo), dtype=BF, device=dev)
    ops.ce_bwd(ld_[r0:], V, None if tgt_d is None else tgt_d[r0:], None if prob_d is None else prob_d[r0:], n2, V, smoothing, lse_s, gout_s.to(dev),
               dl_s, ldo)
    assert torch.equal(dl_s, dl[r0:])


def test_topk_past_the_cap_and_ties(dev):
    """B = 1029 rows (cap 256 workgroups x 4 rows: a 5-row second trip), logits on a small integer grid so that labels tie with other classes.
    See the module docstring for the tie rule and why torch.topk cannot be followed where the order of equal values decides."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(240)
    B, C = 1029, 500
    lg = torch.randint(0, 300, (B, C), generator=g).float()        # ~1.7 classes per value: ties everywhere, five-fold ties at the top rare
    hard = torch.randint(0, C, (B,), generator=g)
    rows = torch.arange(B)
    other = (hard + 1 + torch.randint(0, C - 1, (B,), generator=g)) % C
    top = lg.max(1).values
    kind = rows % 6
    # label ties for first place with one other class (top-1 decided by the order, top-5 not) / label ties in second place / label alone on top /
    # label ties with six others on top (both decided by the order) / untouched rows (kind 4, 5)
    lg[rows[kind == 0], hard[kind == 0]] = top[kind == 0] + 5
    lg[rows[kind == 0], other[kind == 0]] = top[kind == 0] + 5
    lg[rows[kind == 1], hard[kind == 1]] = top[kind == 1]
    lg[rows[kind == 2], hard[kind == 2]] = top[kind == 2] + 1
    for j in range(7):
        lg[rows[kind == 3], (hard[kind == 3] + 71 * j) % C] = top[kind == 3] + 9
    zl = lg[rows, hard]
    greater = (lg > zl[:, None]).sum(1)
    ties = (lg == zl[:, None]).sum(1)                             # the label itself included
    lower_ties = ((lg == zl[:, None]) & (torch.arange(C)[None, :] < hard[:, None])).sum(1)
    corr = lg.topk(5, dim=1)[1] == hard.unsqueeze(1)              # the reference metric: lightning.py:177-183 / oracle/lrw_oracle.py
    ref_flags = torch.stack((corr[:, 0], corr.amax(1)), 1)
    rule_flags = torch.stack((greater + lower_ties < 1, greater + lower_ties < 5), 1)       # lowest index wins a tie
    decided = torch.stack(((greater >= 1) | (ties == 1), (greater + ties <= 5) | (greater >= 5)), 1)   # whatever the order of equal values
    assert (ties[decided[:, 0]] > 1).sum() > 50 and (ties[decided[:, 1]] > 1).sum() > 50 and (~decided).sum(0).min() > 50
    assert torch.equal(ref_flags[decided], rule_flags[decided])    # (the two definitions agree wherever both are defined)
    soft = torch.zeros(B, C)
    soft[rows, hard] = 0.5
    second = torch.where(kind < 3, (hard - 7) % C, hard)           # half the rows: a 0.5 / 0.5 mix whose argmax is the lower index (torch.argmax: first maximum)
    soft[rows, second] += 0.5
    soft_lab = soft.argmax(1)
    assert (soft_lab != hard).sum() > 20
    lgd = lg.to(dev)
    for lab_d, soft_d, lab in ((hard.to(dev), None, hard), (None, soft.to(dev), soft_lab)):
        acc = ops.topk_acc(lgd, lab_d, soft_d)
        # the per-row results the launch leaves for its fixed-order mean: ops.topk_acc hands the kernel ops.scratch(2 * B) as `rows2`, i.e. the
        # first 2 * B floats of this stream's scratch buffer (a dependency on that wrapper's body, accepted to see single rows)
        flags = ops.scratch(2 * B)[: 2 * B].view(B, 2).cpu() > 0.5
        if lab is hard:
            want, dec = rule_flags, decided
            assert torch.equal(flags[dec], ref_flags[dec])
        else:
            zs = lg[rows, lab]
            n_before = (lg > zs[:, None]).sum(1) + ((lg == zs[:, None]) & (torch.arange(C)[None, :] < lab[:, None])).sum(1)
            want = torch.stack((n_before < 1, n_before < 5), 1)
        assert torch.equal(flags, want)
        assert torch.equal(flags[1024:], want[1024:])              # the second trip
        a = acc.cpu()
        assert abs(a[0].item() - want[:, 0].float().mean().item()) < 1e-6 and abs(a[1].item() - want[:, 1].float().mean().item()) < 1e-6     # test_cross_entropy_and_topk: 1e-6
    # the second trip's rows as a launch of their own
    ops.topk_acc(lgd[1024:], hard.to(dev)[1024:], None)
    assert torch.equal(ops.scratch(2 * B)[:10].view(5, 2).cpu() > 0.5, rule_flags[1024:])


# ---------------------------------------------------------------------------------------------------------------------------------------
# optimiser-side passes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_adamw_and_cast_past_the_cap(dev):
    """n = 1,048,576 + 4,099: svsr_adamw_step and svsr_cast_bf16 (cap 4096 x 256) take a ragged second trip, svsr_grad_sumsq (1024 x 256 float4)
    too; weight decay ends inside the second trip.  Two steps against oracle.lrw_oracle.adamw_step, as test_adamw_clip_schedule."""
    from oracle import lrw_oracle as O
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(250)
    n = 1048576 + 4099
    cap = 4096 * 256
    decay_end = cap + 2000
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (3.0, 0.01)]
    pd, md, vd = p.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    shadow = torch.zeros(n, dtype=BF, device=dev)
    state = torch.zeros(4 + 1024, dtype=torch.int32, device=dev)
    lr, betas, eps, wd, max_norm, warm, total = 1e-2, (0.9, 0.999), 1e-6, 0.01, 1.0, 2, 10
    pa, pb = p[:decay_end].clone().view(-1, 1), p[decay_end:].clone()
    ma, mb, va, vb = torch.zeros_like(pa), torch.zeros_like(pb), torch.zeros_like(pa), torch.zeros_like(pb)
    for step, gr in enumerate(grads):
        gd = gr.to(dev)
        ops.grad_sumsq(gd, state)
        # the second trip's range [cap, n) on copies, before the whole-buffer launch advances the step counter: same state, same clip factor
        p2, m2, v2, s2 = pd.clone(), md.clone(), vd.clone(), shadow.clone()
        ops.adamw_range(p2, gd, m2, v2, s2, cap, n, decay_end, lr, betas, eps, wd, max_norm, warm, total, state, False)
        ops.adamw_step(pd, gd, md, vd, shadow, decay_end, lr, betas, eps, wd, max_norm, warm, total, state)
        for whole, part in ((pd, p2), (md, m2), (vd, v2), (shadow, s2)):
            assert torch.equal(whole[cap:], part[cap:])
        ga, gb = gr[:decay_end].clone().view(-1, 1), gr[decay_end:].clone()
        O.clip_grad_norm([ga, gb], max_norm)
        O.adamw_step([pa, pb], [ga, gb], [ma, mb], [va, vb], step + 1, O.cosine_lr(step, lr, warm, total), betas, eps, wd)
    ref = torch.cat((pa.view(-1), pb))
    check(pd, ref, "adamw.p", 1e-5, 1e-5)                          # test_gpu_kernels.py::test_adamw_clip_schedule: p 1e-5, shadow 8e-3 / 4e-3
    check(pd[cap:], ref[cap:], "adamw.p (second trip)", 1e-5, 1e-5)
    check(shadow, ref, "adamw.shadow", 8e-3, 4e-3)
    assert torch.equal(shadow, pd.to(BF))
    assert int(state[0].item()) == 2

    dst = torch.zeros(n, dtype=BF, device=dev)
    ops.cast_bf16(pd, dst)
    assert torch.equal(dst.cpu(), pd.cpu().to(BF))                 # test_gpu_misc.py::test_transpose_cast_multi: exact
    dst2 = torch.zeros(n - cap, dtype=BF, device=dev)
    ops.cast_bf16(pd[cap:], dst2)
    assert torch.equal(dst2, dst[cap:])


def test_fill_and_clip_prep_past_the_cap(dev):
    """svsr_fill_f32 and svsr_clip_prep share grid_for (cap 4096 x 256 = 1,048,576 elements)."""
    from syncvsr_amd import ops
    from syncvsr_amd.augment import DeviceClipPipeline

    n = 1048576 + 4099
    buf = torch.zeros(n + 64, device=dev)
    ops._call("svsr_fill_f32", buf.data_ptr(), n, 1.5, ops._stream())      # no public wrapper: ops.GradCoverage.fill() calls it the same way
    assert bool((buf[:n] == 1.5).all()) and float(buf[n:].abs().max()) == 0.0
    g = torch.Generator().manual_seed(260)
    B, T, Hs, Ws, S = 5, 28, 96, 96, 88                           # 5 * 28 * 88 * 88 = 1,084,160 output pixels
    frames = torch.randint(0, 256, (B, T, Hs, Ws), dtype=torch.uint8, generator=g)
    ev = DeviceClipPipeline(S, train=False)(frames.to(dev)).cpu()
    ref = ((frames[:, :, 4:92, 4:92].float() / 255.0) - 0.421) / 0.165
    assert ev.shape == (B, 1, T, S, S)
    assert (ev[:, 0] - ref).abs().max() < 1e-6                     # test_gpu_misc.py::test_device_clip_pipeline: the centre crop to 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------------
# attention: the position-table gradient's reduction over clips
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flash", [False, True])
def test_mha_position_gradient_past_the_cap(dev, flash):
    """k_mha_pe_reduce (dpe = sum over clips of the per-clip partial tables) at (2T - 1) * H * 64 = 343 * 768 = 263,424 > 1024 x 256 elements:
    H = 12, T = 172 is the smallest table past the cap at the model's head count; B = 2.  Reached from svsr_mha_bwd and from
    svsr_mha_flash_bwd_parts.  Reference and bounds: test_gpu_lrs_kernels.py::test_rel_mha_fwd_bwd."""
    from syncvsr_amd import ops

    B, H, T, lens = 2, 12, 172, [172, 97]
    D = H * 64
    qkv, pe, dctx = rnd((B * T, 3 * D), 1), rnd((2 * T - 1, D), 2), rnd((B * T, D), 5)
    u, v = rndf((H, 64), 3, 0.5), rndf((H, 64), 4, 0.5)
    klen = torch.tensor(lens, dtype=torch.int32)
    qf = qkv.to(F64).view(B, T, 3, H, 64).requires_grad_(True)
    pef = pe.to(F64).view(2 * T - 1, H, 64).requires_grad_(True)
    q, k, val = qf[:, :, 0], qf[:, :, 1].transpose(1, 2), qf[:, :, 2].transpose(1, 2)
    u64, v64 = u.to(F64), v.to(F64)
    qu = (q + u64).detach().to(BF).to(F64) + ((q + u64) - (q + u64).detach())            # bf16-rounded forward value, identity gradient
    qv = (q + v64).detach().to(BF).to(F64) + ((q + v64) - (q + v64).detach())
    ac = torch.matmul(qu.transpose(1, 2), k.transpose(-2, -1))
    bd_full = torch.matmul(qv.transpose(1, 2), pef.permute(1, 2, 0))
    idx = (T - 1) + torch.arange(T).view(1, T) - torch.arange(T).view(T, 1)
    bd = bd_full.gather(-1, idx.expand(B, H, T, T))
    mask = (torch.arange(T).view(1, T) < klen.view(B, 1)).view(B, 1, 1, T)
    attn = torch.softmax(((ac + bd) / 8.0).masked_fill(~mask, -1e10), -1).masked_fill(~mask, 0.0)
    ctx_ref = torch.matmul(attn, val).transpose(1, 2).reshape(B * T, D)
    ctx_ref.backward(dctx.to(F64))
    dpe_ref = pef.grad.reshape(2 * T - 1, D)

    qkv_d, pe_d, ud, vd = qkv.to(dev), pe.to(dev), u.to(dev).contiguous(), v.to(dev).contiguous()
    ctx, keep = ops.mha_fwd(qkv_d, 3 * D, qkv_d[:, D:], qkv_d[:, 2 * D:], 3 * D, B=B, H=H, Lq=T, Lk=T, pe=pe_d, bias_u=ud, bias_v=vd,
                            klen=klen.to(dev), flash=flash)
    check_rel(ctx, ctx_ref, "ctx", 1.5e-2)
    dqkv = torch.empty_like(qkv_d)
    out = ops.mha_bwd(dctx.to(dev), qkv_d, 3 * D, qkv_d[:, D:], qkv_d[:, 2 * D:], 3 * D, keep, B=B, H=H, Lq=T, Lk=T, dq=dqkv, dq_pitch=3 * D,
                      dk=dqkv[:, D:], dv=dqkv[:, 2 * D:], dkv_pitch=3 * D, pe=pe_d, bias_u=ud, bias_v=vd, pe_later=flash)
    dpe = out[2]
    if flash:
        fn, kept = out[3]
        fn()
        pe_part = kept[3]
        # the reduction itself, exactly: clips added in order in fp32, one rounding to bf16
        assert torch.equal(dpe, (pe_part[0] + pe_part[1]).to(BF))
    check_rel(dpe, dpe_ref, "dpe", 2.5e-2)
    cap = 1024 * 256
    check_rel(dpe.reshape(-1)[cap:], dpe_ref.reshape(-1)[cap:], "dpe (second trip)", 2.5e-2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# sentence-level passes with the same structure (csrc/lrs_misc.hip, grid1d: cap 2048 workgroups)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_ls_loss_past_the_cap(dev):
    """R = 8,197 decoder rows (4 per workgroup, cap 2048): bounds and reference of test_gpu_lrs_kernels.py::test_embed_pos_and_ls_loss."""
    from oracle import lrs_oracle as O
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(270)
    B, L, V, Vp = 7, 1171, 41, 64
    R = B * L
    assert R == 8197
    z = torch.randn(R, Vp, generator=g)
    target = torch.randint(0, V, (B, L), generator=g)
    target[0, 600:] = -1
    target[6, 1100:] = -1                                          # padded rows inside the second trip
    zf = z[:, :V].to(F64).view(B, L, V).requires_grad_(True)
    smoothing = 0.1
    ref_loss = O.label_smoothing_loss(zf, target, smoothing, False)
    ref_loss.backward()
    live = int((target >= 0).sum())
    zd, td = z.to(dev), target.to(dev)
    loss, lse, counts = ops.ls_loss_fwd(zd, Vp, td, R, V, smoothing, 1.0 / B)
    assert abs(loss.item() - ref_loss.item()) <= 2e-5 * max(1.0, abs(ref_loss.item())), (loss.item(), ref_loss.item())
    assert counts[1].item() == live
    assert abs(counts[0].item() / live - O.th_accuracy(zf.detach(), target)) < 1e-6
    gout = torch.ones((), device=dev)
    dz = ops.ls_loss_bwd(zd, Vp, td, R, V, smoothing, 1.0 / B, lse, gout, Vp)
    check_rel(dz[:, :V], zf.grad.reshape(R, V), "ls_loss.dz", 6e-3)
    assert float(dz[:, V:].float().abs().max()) == 0.0
    t0 = 2048 * 4
    tf = td.reshape(-1)
    _, lse_s, _ = ops.ls_loss_fwd(zd[t0:], Vp, tf[t0:], R - t0, V, smoothing, 1.0 / B)
    assert torch.equal(lse_s, lse[t0:])
    dz_s = ops.ls_loss_bwd(zd[t0:], Vp, tf[t0:], R - t0, V, smoothing, 1.0 / B, lse_s, gout, Vp)
    assert torch.equal(dz_s, dz[t0:])


def test_embed_pos_fwd_past_the_cap(dev):
    """R * D/8 = 32,780 x 16 = 524,480 vectors: 192 past 2048 x 256."""
    from oracle import lrs_oracle as O
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(280)
    B, L, D, V = 20, 1639, 128, 41
    tok = torch.randint(0, V, (B, L), generator=g)
    emb = torch.randn(V, D, generator=g)
    pe = O.abs_pos_emb(L, D).float().contiguous()
    x = ops.embed_pos_fwd(tok.to(dev), emb.to(dev), pe.to(dev), L, D, math.sqrt(D))
    ref = F.embedding(tok, emb).to(F64) * math.sqrt(D) + pe.to(F64)
    check_rel(x, ref.reshape(B * L, D), "embed_pos_fwd", 4e-3)     # test_embed_pos_and_ls_loss: < 4e-3
    x_s = ops.embed_pos_fwd(tok[B - 1:].to(dev), emb.to(dev), pe.to(dev), L, D, math.sqrt(D))      # the last sequence holds the second trip
    assert (B - 1) * L * (D // 8) < 2048 * 256 < B * L * (D // 8)
    assert torch.equal(x_s, x[(B - 1) * L:])


def test_scale_bf16_past_the_cap(dev):
    """n = 4,194,304 + 8,248 elements (cap 2048 x 256 vectors of 8).  The masked form past the cap is compared with the LayerNorm backward's second
    output in test_add_ln_past_the_caps."""
    from syncvsr_amd import ops

    n = 2048 * 256 * 8 + 8 * 1031
    x = rnd((n,), 290).to(dev)
    y = ops.scale_bf16(x, 0.5)
    assert torch.equal(y.float(), x.float() * 0.5)                 # a power of two: exact (test_ln768...: < 1e-6)
    t0 = 2048 * 256 * 8
    assert torch.equal(ops.scale_bf16(x[t0:].contiguous(), 0.5), y[t0:])
    seed = torch.tensor([4321], dtype=torch.int32, device=dev)
    yd = ops.scale_bf16(x, 2.0, drop=(seed, 9, 0.25))
    kept = yd != 0
    assert torch.equal(yd[kept].float(), (x.float() * (2.0 / 0.75)).to(BF).float()[kept])
    for lo, hi in ((0, t0), (t0, n)):
        assert 0.2 < float((~kept[lo:hi]).float().mean()) < 0.3
    assert torch.equal(yd, ops.scale_bf16(x, 2.0, drop=(seed, 9, 0.25)))


def test_ctc_row_lse_past_the_cap(dev):
    """svsr_ctc_fwd's row log-sum-exp pass at B * T = 9 x 911 = 8,199 rows (cap 2048 x 4): bounds and reference of test_gpu_lrs_kernels.py::test_ctc."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(300)
    B, T, V, Vp = 9, 911, 11, 64
    lens = [911, 700, 911, 850, 30, 911, 400, 911, 911]          # the last clip is full: all seven rows of the second trip are live
    ylens = [40, 12, 25, 8, 3, 30, 20, 5, 33]
    z = torch.randn(B * T, Vp, generator=g)
    Lmax = max(ylens)
    labels = torch.full((B, Lmax), -1, dtype=torch.long)
    ys = []
    for b, n in enumerate(ylens):
        y = torch.randint(1, V, (n,), generator=g)
        y[1] = y[0]
        labels[b, :n] = y
        ys.append(y)
    zf = z[:, :V].to(F64).view(B, T, V).requires_grad_(True)
    ref = F.ctc_loss(zf.transpose(0, 1).log_softmax(2), torch.cat(ys), torch.tensor(lens), torch.tensor(ylens), blank=0, reduction="sum",
                     zero_infinity=True) / B
    ref.backward()
    zd = z.to(dev)
    ilen = torch.tensor(lens, dtype=torch.int32, device=dev)
    loss, state = ops.ctc_fwd(zd, Vp, labels.to(dev), ilen, B, T, V)
    assert abs(loss.item() - ref.item()) <= 2e-4 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    dz = ops.ctc_grad(zd, Vp, labels.to(dev), ilen, B, T, V, state, torch.ones((), device=dev), Vp)
    got = dz.float().cpu()
    assert torch.all(got[:, V:] == 0)
    check_rel(got[:, :V], zf.grad.reshape(B * T, V), "ctc.dlogits", 6e-3)
    check_rel(got[8192:, :V], zf.grad.reshape(B * T, V)[8192:], "ctc.dlogits (rows of the second trip)", 6e-3)


def test_glu_dwconv_bwd_past_the_reduce_cap(dev):
    """k_dw_reduce (cap 256 workgroups x 256) at D * (K + 1) = 2112 * 32 = 67,584 sums: the second trip holds the last 2,048 of them, all in dbias.
    Reference and bounds: test_gpu_lrs_kernels.py::test_glu_dwconv (du < 8e-3, dw / dbias < 5e-3), in fp64."""
    from syncvsr_amd import ops

    B, T, D, K = 2, 40, 2112, 31
    u, dc = rnd((B * T, 2 * D), 310), rnd((B * T, D), 311)
    w = rndf((D, K), 312, 1 / math.sqrt(K))
    uf = u.to(F64).view(B, T, 2 * D).requires_grad_(True)
    wf, bf_ = w.to(F64).requires_grad_(True), torch.zeros(D, dtype=F64, requires_grad=True)
    g = uf[..., :D] * torch.sigmoid(uf[..., D:])
    c_ref = F.conv1d(g.transpose(1, 2), wf.view(D, 1, K), bf_, padding=(K - 1) // 2, groups=D).transpose(1, 2).reshape(B * T, D)
    c_ref.backward(dc.to(F64))
    dw, db = torch.zeros(D, K, device=dev), torch.zeros(D, device=dev)
    du = ops.glu_dwconv_bwd(dc.to(dev), u.to(dev), w.to(dev), dw, db, B, T, D, K)
    check_rel(du, uf.grad.reshape(B * T, 2 * D), "glu_dwconv.du", 8e-3)
    check_rel(dw, wf.grad, "glu_dwconv.dw", 5e-3)
    check_rel(db, bf_.grad, "glu_dwconv.dbias", 5e-3)
    first = 256 * 256 - D * K                                      # dbias entries of the first trip; the rest is the second
    check_rel(db[first:], bf_.grad[first:], "glu_dwconv.dbias (second trip)", 5e-3)


def test_transpose_bf16_multi_past_the_tile_cap(dev):
    """svsr_transpose_bf16_multi (128 workgroups per table entry walk the 64 x 64 tiles): 1536 x 512 = 192 tiles on the 16-byte path, 1100 x 601 =
    180 tiles on the element-pair path (odd row length), and two small entries.  Exact, as tests/test_gpu_misc.py::test_transpose_cast_multi."""
    import numpy as np

    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(320)
    shapes = [(1536, 1, 512), (1100, 1, 601), (40, 3, 72), (64, 9, 64)]     # (A, T, Bd)
    src_parts, entries, soff, doff = [], [], 0, 0
    for A, T, Bd in shapes:
        src_parts.append(torch.randn(A * T * Bd, generator=g).to(BF))
        Apad = (A + 63) // 64 * 64
        soff = (soff + 7) // 8 * 8                                 # 16-byte aligned entries, as the parameter buffer has them
        entries.append((soff, doff, A, T, Bd, Apad))
        soff += A * T * Bd
        doff += Bd * T * Apad
    w16 = torch.zeros(soff, dtype=BF)
    for e, part in zip(entries, src_parts):
        w16[e[0]: e[0] + part.numel()] = part
    dst = torch.zeros(doff, dtype=BF, device=dev)
    tab = np.zeros(len(entries), dtype=np.dtype([("src", "<i8"), ("dst", "<i8"), ("A", "<i4"), ("T", "<i4"), ("Bd", "<i4"), ("Apad", "<i4")]))
    for i, e in enumerate(entries):
        tab[i] = e
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    ops.transpose_shadows(None, w16.to(dev), dst, table, len(entries))
    for (so, do, A, T, Bd, Apad), part in zip(entries, src_parts):
        ref = torch.zeros(Bd, T, Apad, dtype=BF)
        ref[:, :, :A] = part.view(A, T, Bd).permute(2, 1, 0)
        got = dst[do: do + Bd * T * Apad].view(Bd, T, Apad).cpu()
        assert torch.equal(got, ref), (A, T, Bd)


def test_fill_ranges_past_the_cap(dev):
    """svsr_fill_ranges (cap 2048 workgroups x 256 16-byte stores per range): one range of 2,097,152 + 4,124 floats beside a short one; nothing
    outside the ranges is written."""
    import ctypes

    from syncvsr_amd import ops

    cap = 2048 * 256 * 4
    lo, hi = 8, 8 + cap + 4 * 1031
    n = hi + 64
    buf = torch.full((n,), 7.0, device=dev)
    ranges = (ctypes.c_int64 * 4)(lo, hi, hi + 16, hi + 24)        # host array of [begin, end) pairs, as ops.GradCoverage.fill() passes it
    ops._call("svsr_fill_ranges", buf.data_ptr(), n, ranges, 2, 0x3FC00000, ops._stream())      # the bit pattern of 1.5f
    want = torch.full((n,), 7.0)
    want[lo:hi] = 1.5
    want[hi + 16: hi + 24] = 1.5
    assert torch.equal(buf.cpu(), want)
