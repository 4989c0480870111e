"""The grouped weight-gradient launch on 128-wide tiles (-m gpu): svsr_wgrad_rows_plan_tile + svsr_igemm_wgrad_group_v2 with
{128, 2, 1} plans, through the C ABI, and the fused encoder backward's single flush that uses them.

A grouped launch runs the ordinary workgroup body (csrc/igemm_wgrad.hip wg_body) on a problem looked up in a device table, one writer
per element: its results must EQUAL those of svsr_igemm_wgrad_v2 launches of the same plans, bit for bit, in every store / add mode.
Against torch (fp32 products of the bf16 inputs, another order of additions): relative L2 < 2e-3, the bound tests/test_gpu_kernels.py
states for fp32 weight gradients and uses for this body.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

ERR_ARG = 1001
B_SEQ, S_SEQ = 4, 30
# (rows, K, N, bias, seq): a K tail of 6 rows; exactly one chunk; partial 128-wide tiles in both dimensions; the benchmark's row count on
# one tile column; rows 1 .. S-1 of every sequence (row-major enumeration: 4 "images" of 29 positions)
SHAPES = [(70, 128, 128, True, None), (64, 128, 256, False, None), (130, 192, 136, True, None), (960, 512, 128, True, None),
          (B_SEQ * (S_SEQ - 1), 128, 128, True, (S_SEQ, 1, S_SEQ - 1))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


class _Problem:
    """One linear weight gradient: inputs, its forced-tile plan, and the arguments of a C-ABI call."""

    def __init__(self, dev, shape, seed, bc=128, plan=None):
        from syncvsr_amd import ops

        rows, K, N, bias, seq = shape
        g = torch.Generator().manual_seed(seed)
        xrows = rows if seq is None else rows // seq[2] * seq[0]
        self.shape, self.bias = shape, bias
        self.x = torch.randn((xrows, K), generator=g).to(torch.bfloat16).to(dev)
        self.dy = (torch.randn((rows, N), generator=g) * 0.1).to(torch.bfloat16).to(dev)
        rp = (rows, 1, 0, 0) if seq is None else (rows // seq[2], seq[2], seq[1], 0)
        self.geo = (rows, 1, 1) if seq is None else (rows // seq[2], seq[0], seq[2])          # Nimg, in_pix, out_pix
        self.plan = plan if plan is not None else ops.wgrad_rows_plan_tile(*rp, K, N, bias, bc)

    def outputs(self, dev, fill=1.0):
        _, K, N, bias, _ = self.shape
        return torch.full((N, K), fill, dtype=torch.float32, device=dev), (torch.full((N,), fill, dtype=torch.float32, device=dev) if bias else None)

    def record(self, dw, db):
        from syncvsr_amd import ops

        _, K, N, _, _ = self.shape
        return ops._WgradProblem(self.x.data_ptr(), self.dy.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None,
                                 self.plan.words.data_ptr(), ctypes.addressof(self.plan.meta), self.geo[0], self.geo[1], K, K, N, self.geo[2], N, 1)

    def single(self, dw, db, mode):
        from syncvsr_amd import _lib, ops

        _, K, N, _, _ = self.shape
        part = torch.empty(max(self.plan.part_floats, 1), dtype=torch.float32, device=dw.device)
        return _lib.load().svsr_igemm_wgrad_v2(self.x.data_ptr(), self.dy.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None,
                                               self.plan.words.data_ptr(), self.plan.meta, self.geo[0], self.geo[1], K, K, N, self.geo[2], N, 1,
                                               part.data_ptr(), self.plan.part_floats, mode, ops._stream())

    def reference(self):
        rows, K, N, _, seq = self.shape
        x = self.x.float()
        if seq is not None:
            S, s0, n = seq
            x = x.view(-1, S, K)[:, s0:s0 + n].reshape(rows, K)
        return self.dy.float().t() @ x, self.dy.float().sum(0)


def _group(dev, records, modes):
    from syncvsr_amd import _lib, ops

    lib = _lib.load()
    n = len(records)
    arr = (ops._WgradProblem * max(n, 1))(*records)
    marr = (ctypes.c_int * max(n, 1))(*modes)
    nbytes = max(int(lib.svsr_igemm_wgrad_group_bytes(max(n, 1))), 1 << 16)
    table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.svsr_igemm_wgrad_group_v2(arr, marr, n, table.data_ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def seventeen(dev):
    """17 problems (the table travels in chunks of 16: the last one crosses a chunk): the five shapes, repeated with fresh data."""
    return [_Problem(dev, SHAPES[i % len(SHAPES)], 100 + i) for i in range(17)]


@pytest.fixture(scope="module")
def grouped_by_mode(dev, seventeen):
    """mode -> [(dw, db)] of ONE grouped launch over the 17 problems, on destinations pre-filled with 1.0 (computed once, left unchanged)."""
    out = {}
    for mode in range(4):
        outs = [q.outputs(dev) for q in seventeen]
        assert all(int(q.plan.meta[0]) == 128 and int(q.plan.meta[1]) == 2 and int(q.plan.meta[2]) == 1 and int(q.plan.meta[7]) == 0 for q in seventeen)
        assert _group(dev, [q.record(dw, db) for q, (dw, db) in zip(seventeen, outs)], [mode] * 17) == 0
        out[mode] = outs
    return out


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_grouped_wide_launch_equals_single_launches(dev, seventeen, grouped_by_mode, mode):
    for i, (q, (gdw, gdb)) in enumerate(zip(seventeen, grouped_by_mode[mode])):
        dw, db = q.outputs(dev)
        assert q.single(dw, db, mode) == 0
        torch.cuda.synchronize()
        assert torch.equal(gdw, dw), (i, q.shape, mode)
        if q.bias:
            assert torch.equal(gdb, db), (i, q.shape, mode)


def test_store_overwrites_and_add_adds(grouped_by_mode, seventeen):
    """Destinations were 1.0 everywhere: a stored element is 0.f + sum, an added one fl(1 + sum) — which is the stored one plus 1."""
    for i, q in enumerate(seventeen):
        sdw, sdb = grouped_by_mode[0][i]
        ref_dw, _ = q.reference()
        assert float((sdw - ref_dw).norm() / ref_dw.norm()) < 2e-3, "mode 0 must not keep the fill"
        for mode in (1, 2, 3):
            dw, db = grouped_by_mode[mode][i]
            assert torch.equal(dw, sdw + 1.0 if mode & 1 else sdw), (i, mode)
            if q.bias:
                assert torch.equal(db, sdb + 1.0 if mode & 2 else sdb), (i, mode)


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_grouped_wide_launch_against_torch(grouped_by_mode, seventeen, k):
    q, (dw, db) = seventeen[k], grouped_by_mode[0][k]
    ref_dw, ref_db = q.reference()
    rel = float((dw - ref_dw).norm() / ref_dw.norm())
    print(f"{q.shape}: dw rel L2 {rel:.3e}")
    assert rel < 2e-3, (q.shape, rel)
    if q.bias:
        relb = float((db - ref_db).norm() / ref_db.norm())
        print(f"{q.shape}: db rel L2 {relb:.3e}")
        assert relb < 2e-3, (q.shape, relb)


def test_errors_before_launch(dev):
    from syncvsr_amd import ops

    wide = _Problem(dev, SHAPES[0], 1, bc=128)
    narrow = _Problem(dev, SHAPES[1], 2, bc=64)
    assert [int(v) for v in narrow.plan.meta[:3]] == [64, 3, 1]
    split = _Problem(dev, (960, 512, 512, True, None), 3, plan=ops.wgrad_rows_plan(960, 1, 0, 0, 512, 512, True))
    assert int(split.plan.meta[2]) > 1 and int(split.plan.meta[7]) == 0, "the case must be a split-K plan"
    for name, probs, n in (("mixed 64 / 128", [wide, narrow], 2), ("mixed 128 / 64", [narrow, wide], 2), ("split plan", [split], 1),
                           ("split plan behind a good one", [narrow, split], 2), ("n = 0", [wide], 0), ("n = 257", [wide] * 257, 257)):
        outs = [q.outputs(dev, fill=3.0) for q in probs[:2]]
        outs = outs + [outs[0]] * (len(probs) - len(outs))
        recs = [q.record(dw, db) for q, (dw, db) in zip(probs, outs)]
        rc = _group(dev, recs if n else [], [3] * n)
        assert rc == ERR_ARG, (name, rc)
        for dw, db in outs:
            assert bool((dw == 3.0).all()) and (db is None or bool((db == 3.0).all())), name
    lib_rc = ops._lib.load().svsr_wgrad_rows_plan_tile(64, 1, 0, 0, 128, 128, 1, 96, None, 0, None, None)
    assert lib_rc == -ERR_ARG


@pytest.mark.parametrize("bc", [128, 64])
def test_lookup_at_the_seams(dev, bc):
    """Problems of 1, 2 and 1 tiles (bc = 128; four times as many at 64): the first and the last workgroup of each must find its own entry."""
    probs = [_Problem(dev, (64, 128, n, True, None), 40 + i, bc=bc) for i, n in enumerate((128, 256, 128))]
    if bc == 128:
        assert [int(q.plan.meta[4]) for q in probs] == [1, 2, 1]
    outs = [q.outputs(dev) for q in probs]
    assert _group(dev, [q.record(dw, db) for q, (dw, db) in zip(probs, outs)], [0, 0, 0]) == 0
    for q, (gdw, gdb) in zip(probs, outs):
        dw, db = q.outputs(dev)
        assert q.single(dw, db, 0) == 0
        torch.cuda.synchronize()
        assert torch.equal(gdw, dw) and torch.equal(gdb, db), q.shape
        ref_dw, _ = q.reference()
        assert float((gdw - ref_dw).norm() / ref_dw.norm()) < 2e-3


def test_ops_tile_argument_splits_narrow_problems_off(dev):
    """ops.linear_wgrad_group(tile=128): problems with K or N below 128 ride a second, 64-wide group of the same call; every result equals
    the single launch of the plan it was given."""
    from syncvsr_amd import ops

    shapes = [(960, 512, 512, True, None), (70, 64, 256, True, None), (130, 192, 72, False, None)]
    probs = [_Problem(dev, sh, 60 + i, bc=128 if min(sh[1], sh[2]) >= 128 else 64) for i, sh in enumerate(shapes)]
    outs = [q.outputs(dev, fill=0.0) for q in probs]
    ops.linear_wgrad_group([dict(x=q.x, dy=q.dy, dw=dw, db=db, rows=q.shape[0], K=q.shape[1], N=q.shape[2], x_pitch=q.shape[1], dy_pitch=q.shape[2])
                            for q, (dw, db) in zip(probs, outs)], tile=128)
    for q, (gdw, gdb) in zip(probs, outs):
        dw, db = q.outputs(dev, fill=0.0)
        assert q.single(dw, db, 3) == 0
        torch.cuda.synchronize()
        assert torch.equal(gdw, dw) and (db is None or torch.equal(gdb, db)), q.shape
        assert float(gdw.abs().max()) > 0


# ---- the fused encoder backward's single flush ----------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


@pytest.fixture(scope="module", params=[64, 128])
def encoder_runs(dev, request):
    """A 2-layer encoder, B = 2, T = 5: the backward from one tape and one upstream gradient — twice through the fused launch with a
    collector and the side stream (the merged flush on tiles of either edge, with a recording gradient-ready hook), once through the
    per-layer launch chain."""
    from syncvsr_amd import model as M
    from syncvsr_amd import ops
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.init import init_state_dict

    B, T, layers = 2, 5, 2
    cfg = default_lrw_config(model__bert__num_hidden_layers=layers)
    model = M.Model(cfg, seed=3)
    model.load_state_dict(init_state_dict(cfg, seed=11, perturb_norm=True))
    model.to(dev).train(False)
    st = model.store()
    st.refresh_shadows()
    feats = (torch.randn(B * T, 512, generator=torch.Generator().manual_seed(23)) * 0.7).to(torch.bfloat16).to(dev)
    tape = {}
    h = M._encoder_forward(model, st, tape, feats, B, T)
    dh = (torch.randn(h.shape, generator=torch.Generator().manual_seed(7)) * 1e-2).to(torch.bfloat16).to(dev)
    runs, labels = [], []

    def backward(merged):
        st.zero_grad()
        st.rebind_grads()
        seen = []
        model._wg_group = [] if merged else None
        model._side.enabled = merged
        model.grad_ready_hook = seen.append
        ops.ENC_BWD_FUSED = merged
        tile, ops.ENC_WGRAD_TILE = ops.ENC_WGRAD_TILE, request.param
        try:
            dfeats = M._encoder_backward(model, st, tape, dh, B, T)
            M._flush_deferred(model)
            model._side.join()
            torch.cuda.synchronize()
        finally:
            ops.ENC_BWD_FUSED = True
            ops.ENC_WGRAD_TILE = tile
            model._side.enabled = False
            model.grad_ready_hook = None
            model._wg_group = None
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if n.startswith(("encoder.", "cls_token"))}
        return dfeats.clone(), grads, seen

    launches = []
    call = ops._call

    def counting(name, *a, **k):
        launches.append(name)
        return call(name, *a, **k)

    ops._call = counting
    try:
        first = backward(True)
    finally:
        ops._call = call
    return dict(model=model, st=st, layers=layers, merged=[first, backward(True)], chain=backward(False), launches=launches)


def test_merged_flush_is_one_grouped_launch(encoder_runs):
    names = encoder_runs["launches"]
    assert names.count("svsr_igemm_wgrad_group_v2") == 1, names          # (no heads in this run: the eight linears of both layers)
    assert names.count("svsr_colsum_rows_multi") == 1 and "svsr_igemm_wgrad_v2" not in names, names
    assert names.index("svsr_enc_bwd") < names.index("svsr_igemm_wgrad_group_v2")


def test_merged_flush_is_bit_reproducible(encoder_runs):
    a, b = encoder_runs["merged"]
    assert torch.equal(a[0], b[0])
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), n


def test_merged_flush_matches_launch_chain(encoder_runs):
    """Relative L2 <= 2e-3 against the per-layer chain: the bound (and the key-bias rule: zero in exact arithmetic, rounding noise on both
    sides, measured against the query bias's gradient) of tests/test_gpu_enc_fused.py."""
    (d1, g1, _), (d0, g0, _) = encoder_runs["merged"][0], encoder_runs["chain"]
    worst = [(_rel(d1, d0), "dfeats")]
    for n in g0:
        if float(g0[n].float().norm()) == 0.0:
            assert float(g1[n].float().norm()) == 0.0, n
            continue
        if n.endswith("attention.self.key.bias"):
            noise = float((g1[n].float() - g0[n].float()).norm() / g0[n.replace(".key.", ".query.")].float().norm())
            assert noise <= 2e-3, (n, noise)
            continue
        worst.append((_rel(g1[n], g0[n]), n))
    worst.sort(reverse=True)
    print("largest relative L2 differences:", "  ".join(f"{r:.2e} {n}" for r, n in worst[:8]))
    assert worst[0][0] <= 2e-3, "  ".join(f"{r:.2e} {n}" for r, n in worst[:8])
    assert any(n.endswith("attention.output.dense.weight") for _, n in worst) and any(n.endswith("output.LayerNorm.weight") for _, n in worst)


def test_gradient_ready_offsets_keep_their_order(encoder_runs):
    st, layers = encoder_runs["st"], encoder_runs["layers"]
    want = [st.offsets[f"encoder.encoder.layer.{i}.attention.self.query.weight"][0] for i in reversed(range(layers))] + [st.offsets["cls_token"][0]]
    for run in encoder_runs["merged"] + [encoder_runs["chain"]]:
        assert run[2] == want, (run[2], want)
