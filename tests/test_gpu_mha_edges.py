"""The attention kernels (syncvsr_amd/csrc/mha.hip: mha_coop.h per tile, mha_flash.h streamed keys) against the float64 restatement of
tests/mha_restatement.py, row by row, at every tile count, workgroup size and mask edge:

  * lengths on, one short of and one past the 32-query tile / 32-key block; the flash launches of 4 to 8 waves (T = 129 .. 256) and the
    group boundaries at 8 | 9 and 16 | 17 tiles (T = 256 | 257, 512 | 513); T = 1;
  * klen of 1, of a multiple of 32, of T - 1, every clip short, no klen, causal with klen, and a clip with no live key at all
    (klen = 0: both forwards mask every key — ctx rows of zeros, lse = +inf — and both backwards then write zero gradients);
  * every output row on its own: err = |got - ref| / max(|ref|, 0.05 median |ref|) (mha_restatement.row_check), the worst row named on
    failure; a row that is exactly zero in the reference (masked keys' dk / dv, position-table rows no live pair reaches) exactly zero in
    buffers that come from torch.empty;
  * dq / dk / dv carved out of sentinel-filled buffers, neighbouring (clip, head)s bit for bit against runs of fewer clips, and two runs
    bit for bit.
The tolerance of a tensor is mha_restatement.tolerance: 4 x the per-row size of the kernels' own bf16 roundings recorded there; the
whole-tensor error is held to the bounds of tests/test_gpu_lrs_kernels.py as well.  The smallest shapes run first."""
import functools

import pytest
import torch

import mha_restatement as mr
from mha_restatement import BF, DH, H

pytestmark = pytest.mark.gpu

D = H * DH
SENTINEL = 0x5A5B            # bf16 bit pattern of the guard bands (a finite value no kernel writes by accident)
SPARE_COLS, SPARE_ROWS = 8, 4


def _dev():
    return torch.device("cuda:0")


def _clips(c: mr.Case, x: dict, lo: int, hi: int):
    """the case and its inputs cut down to clips lo .. hi-1"""
    n = hi - lo
    sub = c._replace(B=n, klen=None if c.klen is None else c.klen[lo:hi])
    y = dict(x)
    for key, L in (("qkv", c.Lq), ("q", c.Lq), ("dctx", c.Lq), ("kv", c.Lk)):
        if key in x:
            y[key] = x[key][lo * L:hi * L].contiguous()
    return sub, y


def _guarded(rows: int, cols: int, dev):
    buf = torch.full((rows + SPARE_ROWS, cols + SPARE_COLS), SENTINEL, dtype=torch.int16, device=dev).view(BF)
    return buf, buf[:rows, :cols]


def _assert_guard(buf, rows: int, cols: int, what: str):
    raw = buf.view(torch.int16).cpu()
    assert (raw[rows:] == SENTINEL).all(), f"{what}: the spare rows after the last were written"
    assert (raw[:, cols:] == SENTINEL).all(), f"{what}: the spare columns of a row were written"


def _run(c: mr.Case, x: dict, flash: bool, guard: bool = False, backward: bool = True) -> dict:
    """forward (and backward) of one case on the device -> the tensors of mha_restatement.attention, on the host, as the kernels wrote them"""
    from syncvsr_amd import ops
    dev = _dev()
    B, Lq, Lk = c.B, c.Lq, c.Lk
    klen = None if c.klen is None else torch.tensor(c.klen, dtype=torch.int32, device=dev)
    dctx = x["dctx"].to(dev)
    if c.rel:
        qkv, pe = x["qkv"].to(dev), x["pe"].to(dev)
        u, v = x["u"].to(dev).contiguous(), x["v"].to(dev).contiguous()
        q, qp, k, val, kvp = qkv, 3 * D, qkv[:, D:], qkv[:, 2 * D:], 3 * D
        kw = dict(pe=pe, bias_u=u, bias_v=v)
    else:
        qd, kv = x["q"].to(dev), x["kv"].to(dev)
        q, qp, k, val, kvp = qd, D, kv, kv[:, D:], 2 * D
        kw = {}
    ctx, rec = ops.mha_fwd(q, qp, k, val, kvp, B=B, H=H, Lq=Lq, Lk=Lk, klen=klen, causal=c.causal, flash=flash, **kw)
    out = {"ctx": ctx.cpu().view(B, Lq, H, DH)}
    if flash:
        assert isinstance(rec, ops.MhaLse)
        out["lse"] = rec.lse.cpu().view(B, H, Lq)
    else:
        p = rec.cpu().view(B, H, Lq, -1)
        assert (p[..., Lk:] == 0).all(), "the padding columns of the stored probabilities are not zero"
        out["probs"] = p[..., :Lk]
    if not backward:
        return out
    if c.rel:
        if guard:
            gbuf, g = _guarded(B * Lq, 3 * D, dev)
        else:
            g = torch.empty((B * Lq, 3 * D), dtype=BF, device=dev)
        pitch = g.stride(0)
        aux = ops.mha_bwd(dctx, q, qp, k, val, kvp, rec, B=B, H=H, Lq=Lq, Lk=Lk, dq=g, dq_pitch=pitch, dk=g[:, D:], dv=g[:, 2 * D:], dkv_pitch=pitch, **kw)
        if guard:
            _assert_guard(gbuf, B * Lq, 3 * D, "dq | dk | dv")
        gh = g.cpu()
        out.update(dq=gh[:, :D].reshape(B, Lq, H, DH), dk=gh[:, D:2 * D].reshape(B, Lk, H, DH), dv=gh[:, 2 * D:].reshape(B, Lk, H, DH),
                   dq_ac=aux[0].cpu().view(B, Lq, H, DH), dq_bd=aux[1].cpu().view(B, Lq, H, DH), dpe=aux[2].cpu().view(2 * Lq - 1, H, DH))
    else:
        if guard:
            qbuf, dq = _guarded(B * Lq, D, dev)
            kbuf, dkv = _guarded(B * Lk, 2 * D, dev)
        else:
            dq = torch.empty((B * Lq, D), dtype=BF, device=dev)
            dkv = torch.empty((B * Lk, 2 * D), dtype=BF, device=dev)
        ops.mha_bwd(dctx, q, qp, k, val, kvp, rec, B=B, H=H, Lq=Lq, Lk=Lk, dq=dq, dq_pitch=dq.stride(0), dk=dkv, dv=dkv[:, D:], dkv_pitch=dkv.stride(0))
        if guard:
            _assert_guard(qbuf, B * Lq, D, "dq")
            _assert_guard(kbuf, B * Lk, 2 * D, "dk | dv")
        kh = dkv.cpu()
        out.update(dq=dq.cpu().reshape(B, Lq, H, DH), dk=kh[:, :D].reshape(B, Lk, H, DH), dv=kh[:, D:].reshape(B, Lk, H, DH))
    return out


@functools.lru_cache(maxsize=None)
def _outputs(name: str, flash: bool) -> dict:
    """one run of a case, shared by the tests that look at it (nothing modifies it)"""
    c = mr.case(name)
    return _run(c, mr.make_inputs(c), flash, guard=name in mr.GUARD_CASES)


def _checks(name: str, flash: bool) -> dict:
    ref = mr.reference(name)
    return {n: mr.row_check(n, t, ref[n]) for n, t in _outputs(name, flash).items()}


ORDERED = sorted(mr.CASES, key=lambda c: (c.Lq * c.Lk, c.B, c.name))
RUNS = [(c.name, f) for c in ORDERED for f in (False, True)]


@pytest.mark.parametrize("name,flash", RUNS)
def test_every_row_of_every_output(name, flash):
    """Forward and backward of one case against the float64 reference (module doc-string): the worst row of every tensor within
    mha_restatement.tolerance, the whole tensor within the bounds of tests/test_gpu_lrs_kernels.py, no NaN.  A row that is zero in the reference
    is measured against the floor of the metric, 0.05 of the median row.  The guard-band cases run with dq / dk / dv carved out of a
    sentinel-filled buffer of 8 spare columns per row and 4 spare rows."""
    fails = []
    for n, chk in _checks(name, flash).items():
        tol = mr.tolerance(n)
        print(f"MHA-EDGE {name} flash={int(flash)} {n}: worst row {chk.worst:.3e} at {chk.where} (tol {tol:.3e}), whole {chk.whole:.3e} (bound {mr.WHOLE_BOUND[n]:.1e})")
        if not chk.worst < tol:
            fails.append(f"{n}: row {chk.where} is off by {chk.worst:.3e} (tolerance {tol:.3e})")
        if not chk.whole < mr.WHOLE_BOUND[n]:
            fails.append(f"{n}: the whole tensor is off by {chk.whole:.3e} (bound {mr.WHOLE_BOUND[n]:.1e})")
    assert not fails, f"{name} flash={flash}: " + "; ".join(fails)


@pytest.mark.parametrize("name,flash", RUNS)
def test_a_row_that_is_zero_in_the_reference_is_zero_in_the_output(name, flash):
    """Exactly: dk / dv rows of masked keys, position-table rows no live pair reaches, every output of a clip without a live key (and an lse of
    +inf there), in buffers that come from torch.empty.  The float64 reference is exactly zero in one more kind of row: a query with ONE live
    key (klen = 1, or query 0 under the causal mask) has P = 1, so dS = P (dP - D) = 0 and with it the row's dq, dq_ac, dq_bd and its share
    of dk and dpe.

    Both implementations return these as exact zeros too: the per-tile kernels form D = sum_j P dP from the very dP, and the flash query pass
    takes D_i = dctx_i · ctx_i from the same MFMA chain that makes dP (mha_flash.h), where ctx_i is that one key's V row bit for bit.  (A D
    summed in any other order of fp32 additions leaves a few ulp of dP there: rows of about 1e-7, up to 1e-5, of a live row.)"""
    bad = {n: (chk.nonzero, chk.nonzero_where) for n, chk in _checks(name, flash).items() if chk.nonzero}
    assert not bad, f"{name} flash={flash}: rows that are exactly zero (lse: infinite) in the reference and not in the output, tensor: (rows, first) = {bad}"


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("name", mr.GUARD_CASES)
def test_a_clip_and_head_is_computed_alone(name, flash):
    """ctx rows and lse values (per tile: the probabilities) of a (clip, head) do not depend on its neighbours: a run of clip 0 alone and a run of
    clip 1 alone against the matching slices of a run of both, bit for bit."""
    c = mr.case(name)
    x = mr.make_inputs(c)
    both = _run(*_clips(c, x, 0, 2), flash, backward=False)
    for b in (0, 1):
        one = _run(*_clips(c, x, b, b + 1), flash, backward=False)
        for n, t in one.items():
            assert torch.equal(t[0], both[n][b]), (n, b)


@pytest.mark.parametrize("name", mr.DETERMINISM_CASES)
def test_two_runs_give_the_same_bits(name):
    c = mr.case(name)
    x = mr.make_inputs(c)
    a, b = _outputs(name, True), _run(c, x, True)
    for n in a:
        assert torch.equal(a[n], b[n]), n
