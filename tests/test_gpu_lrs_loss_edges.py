"""The non-contraction kernels of the sentence-level training step (syncvsr_amd/csrc/lrs_misc.hip: CTC lattice and gradient, label-smoothing
loss, GLU + depthwise conv, decoder embedding backward) against the float64 restatement of tests/lrs_loss_restatement.py, row by row, at
every lattice and tile edge:

  * CTC: empty, full-to-Lmax and all-same targets, inputs exactly as long as the target needs and one frame short (zero_infinity), targets
    of 127 .. 129 and 256 / 257 labels (the second and third pass of the 256-thread state loops), 600 frames, logits x 20, T = 1, B = 1,
    V = 2, gout = 0.3, ldo > ld, and items whose ilen is outside [1, T] (no item: 0 loss, zero rows, nothing of theirs read);
  * label smoothing: R in {1, 5, 27} x V in {2, 63, 64, 65} (and 5049) x smoothing {0, 0.1} x both normalisations, argmax ties, a target at
    V - 1, every row ignored, a target >= V (NaN loss, finite gradient);
  * GLU + depthwise conv: T in {1, 31, 32, 33, 65} x K in {1, 3, 15, 31} x D in {64, 192}, more (clip, tile)s than workgroups, the BatchNorm
    partial rows one by one, dw / dbias added onto non-zero values;
  * embedding backward: a token on 4064, 4065 and 4200 rows (the list path, its boundary, the bit walk), R = 16384, R = 16385 refused.
Every output row is judged on its own (mha_restatement.row_check; the worst row is named), a row that is exactly zero in the reference is
exactly zero in the output, dz / c / du are carved out of sentinel-filled buffers with spare rows in front and behind (these kernels write
every column of their pitch, so there are no spare columns: the columns V.. of dz must be zero), the logits' pad columns and dead rows are
NaN in a second run that must give the same bits as the first.  Tolerances: lrs_loss_restatement (tolerance, sum_bound, *_tolerance)."""
import functools

import pytest
import torch

import lrs_loss_restatement as lr
from lrs_loss_restatement import BF, F64, bound_check, row_check

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B            # bf16 bit pattern of the guard rows (a finite value no kernel writes by accident)
SPARE_ROWS = 4


def _dev():
    return torch.device("cuda:0")


def _guarded(rows: int, cols: int):
    buf = torch.full((rows + 2 * SPARE_ROWS, cols), SENTINEL, dtype=torch.int16, device=_dev()).view(BF)
    return buf, buf[SPARE_ROWS:SPARE_ROWS + rows]


def _assert_guard(buf, rows: int, what: str):
    raw = buf.view(torch.int16).cpu()
    assert (raw[:SPARE_ROWS] == SENTINEL).all(), f"{what}: the spare rows in front of the first were written"
    assert (raw[SPARE_ROWS + rows:] == SENTINEL).all(), f"{what}: the spare rows after the last were written"


def _bits(t):
    """the tensor as integers: equal bits, NaN included"""
    return t.reshape(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _rows(name, what, got, ref, tol, whole_bound, fails, unit=None):
    chk = row_check(what, got, ref)
    at = chk.where if unit is None else unit(chk.where[0])
    print(f"LRS-EDGE {name} {what}: worst row {chk.worst:.3e} at {at} (tol {tol:.3e}), whole {chk.whole:.3e} (bound {whole_bound:.1e}), "
          f"rows not zero {chk.nonzero}")
    if not chk.worst < tol:
        fails.append(f"{what}: row {at} is off by {chk.worst:.3e} (tolerance {tol:.3e})")
    if not chk.whole < whole_bound:
        fails.append(f"{what}: the whole tensor is off by {chk.whole:.3e} (bound {whole_bound:.1e})")
    if chk.nonzero:
        at0 = chk.nonzero_where if unit is None else unit(chk.nonzero_where[0])
        fails.append(f"{what}: {chk.nonzero} rows are zero in the reference and not in the output (or hold NaN), first {at0}")
    return chk


def _bounded(name, what, got, ref, bound, fails):
    worst, i = bound_check(got, ref, bound)
    print(f"LRS-EDGE {name} {what}: worst row {worst:.3e} of its fp32 summation bound, row {i}")
    if not worst < 1.0:
        fails.append(f"{what}: row {i} is off by {worst:.3e} of its bound")


# ------------------------------------------------------------------------------------------------------------------------------------
# CTC
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_ctc(c: lr.CtcCase, nan_pad: bool, items=None, gout=None) -> dict:
    from syncvsr_amd import ops
    dev = _dev()
    z, lab, ilen = lr.ctc_logits(c, nan_pad), lr.ctc_labels(c), list(c.ilen)
    if items is not None:
        k = list(items)
        z, lab, ilen = z.view(c.B, c.T, c.ld)[k].reshape(len(k) * c.T, c.ld).contiguous(), lab[k].contiguous(), [ilen[b] for b in k]
    B = len(ilen)
    zd, labd = z.to(dev), lab.to(dev)
    ilend = torch.tensor(ilen, dtype=torch.int32, device=dev)
    loss, state = ops.ctc_fwd(zd, c.ld, labd, ilend, B, c.T, c.V)
    ldo = c.ld + c.ldo_extra
    buf, out = _guarded(B * c.T, ldo)
    g = torch.tensor(c.gout if gout is None else gout, dtype=torch.float32, device=dev)
    ops.ctc_grad(zd, c.ld, labd, ilend, B, c.T, c.V, state, g, ldo, out=out)
    torch.cuda.synchronize()
    _assert_guard(buf, B * c.T, "dz")
    return dict(loss=loss.cpu(), nll=state[2].cpu(), dz=out.cpu())


def _check_ctc(c: lr.CtcCase, got: dict, ref: dict) -> list:
    fails = []
    dz = got["dz"]
    if not torch.isfinite(dz.float()).all():
        fails.append("dz holds NaN or infinity")
    if not (dz[:, c.V:] == 0).all():
        fails.append("the columns V.. of dz are not zero")
    tol = lr.ctc_nll_tolerance(c.T, c.V)
    for b in range(c.B):
        a, r = float(got["nll"][b]), float(ref["nll"][b])
        print(f"LRS-EDGE {c.name} nll[{b}]: {a:.7g} against {r:.7g}, off by {abs(a - r) / max(1.0, abs(r)):.3e} (tol {tol:.3e})")
        if not ref["feasible"][b]:
            if a != 0.0:
                fails.append(f"nll of item {b} (infeasible or ilen outside [1, T]) is {a}, not 0")
        elif not abs(a - r) <= tol * max(1.0, abs(r)):
            fails.append(f"nll of item {b} is {a}, reference {r}")
    a, r = float(got["loss"]), float(ref["loss"])
    if not abs(a - r) <= tol * max(1.0, abs(r)):
        fails.append(f"loss {a}, reference {r}")
    _rows(c.name, "ctc_dz", dz[:, :c.V], ref["dz"], lr.tolerance("ctc_dz"), lr.WHOLE_BOUND["ctc_dz"], fails,
          unit=lambda row: f"clip {row // c.T} frame {row % c.T}")
    return fails


@pytest.mark.parametrize("name", [c.name for c in lr.CTC_CASES])
def test_ctc_every_item_and_every_gradient_row(name):
    """Per-item nll (exactly 0 for an infeasible item), the loss, and every row of dz against the float64 lattice; the rows t >= ilen[b] and every
    row of an infeasible item exactly zero across all ldo columns; dz carved out of a sentinel-filled buffer.  The second run has NaN in the
    logits' pad columns and in the rows t >= ilen[b]: the same bits."""
    c = lr.ctc_case(name)
    a, b = _run_ctc(c, False), _run_ctc(c, True)
    fails = _check_ctc(c, a, lr.ctc_reference(name))
    for n in a:
        if not torch.equal(a[n], b[n]):
            fails.append(f"{n} differs between two runs, the second with NaN where nothing may read")
    dzv = a["dz"].view(c.B, c.T, -1)
    for i, n in enumerate(c.ilen):
        if not (dzv[i, n:] == 0).all():
            fails.append(f"rows t >= ilen of item {i} are not zero")
    assert not fails, f"{name}: " + "; ".join(fails)


def test_ctc_items_whose_ilen_is_outside_1_to_T_are_no_items():
    """ilen of 0, -2, T + 1 and T + 3, first, in the middle and last in a batch of eight, every logit row of theirs NaN: 0 loss and zero rows for
    them, and the other four exactly as in a run of those four alone (gout halved: the same gout / B)."""
    c = lr.CTC_BAD_ILEN
    a = _run_ctc(c, True)
    fails = _check_ctc(c, a, lr.ctc_reference(c.name))
    k = list(lr.CTC_BAD_ILEN_KEPT)
    alone = _run_ctc(c, True, items=k, gout=c.gout * len(k) / c.B)
    if not torch.equal(a["nll"][k], alone["nll"]):
        fails.append("nll of the other items changes with the items that are none")
    if not torch.equal(a["dz"].view(c.B, c.T, -1)[k], alone["dz"].view(len(k), c.T, -1)):
        fails.append("dz of the other items changes with the items that are none")
    if float(a["loss"]) * (c.B / len(k)) != float(alone["loss"]):
        fails.append(f"loss {float(a['loss'])} is not {len(k)}/{c.B} of {float(alone['loss'])}")
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------------------------------------------
# label smoothing
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_ls(c: lr.LsCase, nan_pad: bool) -> dict:
    from syncvsr_amd import ops
    dev = _dev()
    z, t, inv = lr.ls_inputs(c, nan_pad)
    zd, td = z.to(dev), t.to(dev)
    loss, lse, counts = ops.ls_loss_fwd(zd, c.ld, td, c.R, c.V, c.smoothing, inv)
    ldo = c.ld + c.ldo_extra
    buf, out = _guarded(c.R, ldo)
    ops.ls_loss_bwd(zd, c.ld, td, c.R, c.V, c.smoothing, inv, lse, torch.ones((), device=dev), ldo, out=out)
    torch.cuda.synchronize()
    _assert_guard(buf, c.R, "dz")
    return dict(loss=loss.cpu(), lse=lse.cpu(), counts=counts.cpu(), dz=out.cpu())


@pytest.mark.parametrize("name", [c.name for c in lr.LS_CASES])
def test_label_smoothing_loss_counts_and_every_gradient_row(name):
    """The loss, the correct / live counts (exactly: rows 0 and 1 hold an argmax tie, row 0's target is V - 1), every row's log-sum-exp and every
    row of dz; ignored rows exactly zero; with every row ignored a loss of exactly 0; with a target >= V a NaN loss and the finite gradient of
    a row without a target column.  The second run has NaN in the logits' pad columns: the same bits."""
    c = lr.ls_case(name)
    ref = lr.ls_reference(name)
    a, b = _run_ls(c, False), _run_ls(c, True)
    fails = []
    for n in a:
        if not torch.equal(_bits(a[n]), _bits(b[n])):
            fails.append(f"{n} differs between two runs, the second with NaN in the pad columns")
    if a["counts"].tolist() != [float(ref["correct"]), float(ref["live"])]:
        fails.append(f"counts {a['counts'].tolist()}, reference {[ref['correct'], ref['live']]}")
    got, want = float(a["loss"]), float(ref["loss"])
    tol = lr.ls_loss_tolerance(c.R, c.V)
    print(f"LRS-EDGE {name} loss: {got:.8g} against {want:.8g} (tol {tol:.3e} relative)")
    if c.kind == "bad-target":
        if got == got:
            fails.append(f"the loss is {got}, not NaN")
    elif c.kind == "all-ignored":
        if got != 0.0 or (a["dz"] != 0).any():
            fails.append(f"every row is ignored: loss {got}, dz not all zero: {bool((a['dz'] != 0).any())}")
    elif not abs(got - want) <= tol * max(1.0, abs(want)):
        fails.append(f"loss {got}, reference {want}")
    e = ((a["lse"].to(F64) - ref["lse"]).abs() / ref["lse"].abs().clamp_min(1.0))
    print(f"LRS-EDGE {name} lse: worst row {float(e.max()):.3e} at {int(e.argmax())} (tol {lr.lse_tolerance(c.V):.3e})")
    if not float(e.max()) <= lr.lse_tolerance(c.V):
        fails.append(f"lse of row {int(e.argmax())} is off by {float(e.max()):.3e}")
    dz = a["dz"]
    if not torch.isfinite(dz.float()).all():
        fails.append("dz holds NaN or infinity")
    if not (dz[:, c.V:] == 0).all():
        fails.append("the columns V.. of dz are not zero")
    _rows(name, "ls_dz", dz[:, :c.V], ref["dz"], lr.tolerance("ls_dz"), lr.WHOLE_BOUND["ls_dz"], fails)
    assert not fails, f"{name}: " + "; ".join(fails)


# ------------------------------------------------------------------------------------------------------------------------------------
# GLU + depthwise conv
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_dw(c: lr.DwCase, x: dict, reduce_later: bool = False) -> dict:
    from syncvsr_amd import ops
    dev = _dev()
    B, T, D, K = c
    u, w, bias, dc = (x[n].to(dev) for n in ("u", "w", "bias", "dc"))
    cbuf, cout = _guarded(B * T, D)
    _, (stats, rows) = ops.glu_dwconv_fwd(u, w, bias, True, B, T, D, K, out=cout)
    stats = stats[:rows * 2 * D].view(rows, 2, D).cpu()
    dw, db = torch.full((D, K), lr.DW_START, device=dev), torch.full((D,), lr.DW_START, device=dev)
    dbuf, dout = _guarded(B * T, 2 * D)
    res = ops.glu_dwconv_bwd(dc, u, w, dw, db, B, T, D, K, reduce_later=reduce_later, out=dout)
    if reduce_later:
        torch.cuda.synchronize()
        assert (dw == lr.DW_START).all() and (db == lr.DW_START).all()           # nothing summed yet
        res[1][0]()
    torch.cuda.synchronize()
    _assert_guard(cbuf, B * T, "c")
    _assert_guard(dbuf, B * T, "du")
    return dict(c=cout.cpu(), stats=stats, du=dout.cpu(), dw=dw.cpu(), dbias=db.cpu())


@functools.lru_cache(maxsize=None)
def _dw_outputs(name: str) -> dict:
    c = lr.dw_case(name)
    return _run_dw(c, lr.dw_inputs(c))


@pytest.mark.parametrize("name", [c.name for c in lr.DW_CASES + lr.DW_MANY_TILES])
def test_glu_dwconv_every_row_of_every_output(name):
    """c and du row by row (carved out of sentinel-filled buffers), the BatchNorm partial rows one by one, dw and dbias added onto 0.75 — the
    fp32 outputs within the summation bound of their own terms (lrs_loss_restatement.sum_bound), the whole tensors within the bounds of
    tests/test_gpu_lrs_kernels.py — and a second run with the same bits."""
    c = lr.dw_case(name)
    B, T, D, K = c
    ref = lr.dw_reference(name)
    a = _dw_outputs(name)
    b = _run_dw(c, lr.dw_inputs(c))
    fails = [f"{n} differs between two runs" for n in a if not torch.equal(a[n], b[n])]
    frame = lambda row: f"clip {row // T} frame {row % T}"
    _rows(name, "c", a["c"], ref["c"], lr.tolerance("c"), lr.WHOLE_BOUND["c"], fails, unit=frame)
    _rows(name, "du", a["du"], ref["du"], lr.tolerance("du"), lr.WHOLE_BOUND["du"], fails, unit=frame)
    assert a["stats"].shape == ref["stats"].shape
    n1 = K + 1 + lr.DW_TT + 3                                                     # taps and bias, the frames of a tile, the four quarters
    _bounded(name, "stats sum", a["stats"][:, 0], ref["stats"][:, 0], lr.sum_bound(n1, ref["stats_abs"][:, 0]), fails)
    _bounded(name, "stats sum of squares", a["stats"][:, 1], ref["stats"][:, 1], lr.sum_bound(2 * n1, ref["stats_abs"][:, 1]), fails)
    ntile = B * ((T + lr.DW_TT - 1) // lr.DW_TT)
    n = B * T + 3 + min(lr.DW_SPLITS, ntile) + 1                                  # frames, quarters, splits, the add onto the start
    _bounded(name, "dw", a["dw"], ref["dw"] + lr.DW_START, lr.sum_bound(n, ref["dw_abs"] + lr.DW_START), fails)
    _bounded(name, "dbias", a["dbias"].view(1, D), (ref["dbias"] + lr.DW_START).view(1, D), lr.sum_bound(n, ref["dbias_abs"] + lr.DW_START).view(1, D), fails)
    for what in ("dw", "dbias"):
        e = float((a[what].to(F64) - lr.DW_START - ref[what]).norm() / ref[what].norm())
        print(f"LRS-EDGE {name} {what}: whole {e:.3e} (bound {lr.WHOLE_BOUND[what]:.1e})")
        if not e < lr.WHOLE_BOUND[what]:
            fails.append(f"{what}: the whole tensor is off by {e:.3e}")
    assert not fails, f"{name}: " + "; ".join(fails)


@pytest.mark.parametrize("name", [lr.DwCase(2, T, 64, K).name for T in (32, 33, 65) for K in (3, 31)] + [lr.DW_MANY_TILES[0].name])
def test_glu_dwconv_a_clip_is_computed_alone(name):
    """Other values in clip 1 (u and dc) leave c and du of clip 0 bit for bit: no halo of a tile reaches across a clip boundary."""
    c = lr.dw_case(name)
    x = lr.dw_inputs(c)
    y = dict(x)
    for n, seed in (("u", 21), ("dc", 22)):
        other = torch.randn(x[n].shape, generator=torch.Generator().manual_seed(seed)).to(BF)
        y[n] = torch.cat([x[n][:c.T], other[c.T:]])
    a, b = _dw_outputs(name), _run_dw(c, y)
    assert torch.equal(a["c"][:c.T], b["c"][:c.T]) and torch.equal(a["du"][:c.T], b["du"][:c.T])
    assert not torch.equal(a["c"][c.T:2 * c.T], b["c"][c.T:2 * c.T])
    assert torch.equal(a["stats"][:(c.T + 31) // 32], b["stats"][:(c.T + 31) // 32])


@pytest.mark.parametrize("name", [c.name for c in lr.DW_MANY_TILES])
def test_glu_dwconv_backward_in_parts_equals_the_single_call_with_more_tiles_than_workgroups(name):
    c = lr.dw_case(name)
    a, b = _dw_outputs(name), _run_dw(c, lr.dw_inputs(c), reduce_later=True)
    for n in ("du", "dw", "dbias"):
        assert torch.equal(a[n], b[n]), n


# ------------------------------------------------------------------------------------------------------------------------------------
# decoder embedding backward
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_emb(tok, dx, scale, D, start):
    from syncvsr_amd import ops
    dev = _dev()
    demb = torch.full((lr.EMB_V + 2, D), start, dtype=torch.float32, device=dev)      # two rows no token names
    ops.embed_pos_bwd(tok.to(dev), dx.to(dev), demb[:lr.EMB_V], D, scale)
    torch.cuda.synchronize()
    out = demb.cpu()
    assert (out[lr.EMB_V:] == start).all()
    return out[:lr.EMB_V]


@pytest.mark.parametrize("name", [c.name for c in lr.EMB_CASES])
def test_embed_pos_bwd_on_every_path(name):
    """Integer-valued dx and a scale of 4 (every partial sum exact in fp32): the result EQUALS the float64 sum, added onto 3.0, and does not
    change when the rows are permuted (another row becomes each token's first occurrence).  Then ordinary values: every row of demb within the
    fp32 summation bound of its own terms."""
    c = next(e for e in lr.EMB_CASES if e.name == name)
    tok, dx, scale = lr.emb_inputs(c, True)
    ref = lr.embed_pos_bwd(tok, dx, lr.EMB_V, scale, torch.full((lr.EMB_V, c.D), 3.0))
    got = _run_emb(tok, dx, scale, c.D, 3.0)
    diff = (got.to(F64) != ref["demb"]).any(1)
    assert not diff.any(), f"{name}: rows of demb differ, first token {int(diff.int().argmax())} ({int(ref['rows'][int(diff.int().argmax())])} rows)"
    perm = torch.randperm(c.R, generator=torch.Generator().manual_seed(3))
    assert torch.equal(_run_emb(tok[perm], dx[perm], scale, c.D, 3.0), got), f"{name}: the result depends on the order of the rows"
    tok, dx, scale = lr.emb_inputs(c, False)
    ref = lr.embed_pos_bwd(tok, dx, lr.EMB_V, scale, torch.full((lr.EMB_V, c.D), 0.5))
    got = _run_emb(tok, dx, scale, c.D, 0.5)
    bound = 4.0 * (ref["rows"].to(F64).view(-1, 1) + 2) * lr.U32 * ref["demb_abs"]
    worst, i = bound_check(got, ref["demb"], bound)
    print(f"LRS-EDGE {name} demb: worst row {worst:.3e} of its fp32 summation bound, token {i} ({int(ref['rows'][i])} rows)")
    assert worst < 1.0, f"{name}: token {i} ({int(ref['rows'][i])} rows) is off by {worst:.3e} of its bound"
    assert torch.equal(got, _run_emb(tok, dx, scale, c.D, 0.5)), f"{name}: two runs differ"


def test_embed_pos_bwd_refuses_more_rows_than_its_bit_mask_holds():
    from syncvsr_amd import _lib, ops
    dev = _dev()
    R = lr.EMB_MAX_ROWS + 1
    demb = torch.zeros(lr.EMB_V, 8, device=dev)
    with pytest.raises(_lib.SvsrError):
        ops.embed_pos_bwd(torch.zeros(R, dtype=torch.int64, device=dev), torch.zeros(R, 8, dtype=BF, device=dev), demb, 8, 1.0)
    torch.cuda.synchronize()
    assert (demb == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases notice a broken restatement
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brk", lr.BREAKS)
def test_the_kernels_do_not_pass_against_a_restatement_with_a_deliberate_mistake(brk):
    """lrs_loss_restatement.BREAKS — lattice states from 256 dropped, the skip between equal labels allowed from state 256, a workgroup that
    takes one tile of its split only, the list path's cap as the row count — each makes the checks above fail at the case built for it
    (tests/test_lrs_loss_restatement_cpu.py: and changes nothing at the shapes of tests/test_gpu_lrs_kernels.py)."""
    if brk in ("drop_states_256", "skip_equal_256"):
        for name in ("len-127-128-129", "len-256-257"):
            c = lr.ctc_case(name)
            bad = lr.ctc(lr.ctc_logits(c, False), lr.ctc_labels(c), c.ilen, c.B, c.T, c.V, c.gout, brk=brk)
            assert _check_ctc(c, _run_ctc(c, False), bad), name
    elif brk == "one_tile_per_split":
        c = lr.DW_MANY_TILES[1]
        bad = lr.glu_dwconv(**lr.dw_inputs(c), B=c.B, T=c.T, D=c.D, K=c.K, brk=brk)
        got = _dw_outputs(c.name)
        assert not row_check("du", got["du"], bad["du"]).worst < lr.tolerance("du")
        n = c.B * c.T + 3 + lr.DW_SPLITS + 1
        assert not bound_check(got["dw"], bad["dw"] + lr.DW_START, lr.sum_bound(n, bad["dw_abs"] + lr.DW_START))[0] < 1.0
    else:
        assert brk == "list_cap_rows"
        for c in lr.EMB_CASES:
            tok, dx, scale = lr.emb_inputs(c, True)
            bad = lr.embed_pos_bwd(tok, dx, lr.EMB_V, scale, torch.full((lr.EMB_V, c.D), 3.0), brk=brk)
            if c.D == 8:
                assert torch.equal(_run_emb(tok, dx, scale, c.D, 3.0).to(F64), bad["demb"]) == (c.n_big <= lr.EMB_LIST_CAP), c.name
