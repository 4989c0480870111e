"""Bit identity of the DC-TCN kernels (csrc/dctcn.hip) across library builds: svsr_tconv_fwd, svsr_tconv_fwd_save, svsr_tconv_dgrad and
svsr_tconv_wgrad, the epilogue backward of both BatchNorm statistics modes (svsr_tconv_epi_bwd, svsr_tconv_apply / svsr_tconv_epi_bwd_bs /
svsr_tconv_bn_bwd) and norm5's (svsr_tcn_norm_pool_bwd, svsr_tcn_norm_pool_bwd_bs), driven through the C ABI alone, against
tests/golden/dctcn_kernel_bits.npz.  The golden holds one
SHA-256 per output buffer (guard bands included), not the bits: the raw outputs of these cases come to about 2 MiB, twice what a committed
file may hold.  It is recorded by running this file as a program on the build to compare with:

    python tests/test_gpu_dctcn_bits.py --record

Inputs are assembled from integer draws of seeded CPU generators (bf16 bit patterns, fp32 = integer / 2^23), so they are the same bits on any
host; their digest is part of the golden and is checked first.  The operands have full mantissas and exponents spread over eight binades, so
that a changed summation order, a moved rounding of the gate product or a mis-staged row shows in the output bits.

Shapes: B = 3, T = 33 (two time tiles per clip, the second one row long; 6 slots, and with B = 3, T = 1 an odd slot count: the last
workgroup's second slot is empty), 128 staged channels (two chunks) into 64, every (k, d) of {(1, 1), (3, 1), (5, 2), (7, 5)} — the last a halo
of 15 rows, one short of TC_HALO.  The epilogue and norm5 cases: B = 3, two branches of 64 channels (C = 128: two channel blocks; norm5 C = 64),
99 rows (one full 64-row block and 35 more) and a single row, T = 33 and T = 1, the half reaches (1, 15) under hmax = 15 (the (3, 1) and
(7, 5) branches), dropout p = 0 and 0.2 with a fixed key, every activation, with and without the Swish residual.  The epilogue backward of the
two modes must agree bit for bit where the batch-statistic one runs without halo and dropout."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dctcn_kernel_bits.npz")
KD = [(1, 1), (3, 1), (5, 2), (7, 5)]
SENT = 7.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(g, *shape, emin=118, emax=127):
    """bf16 from integer draws: random sign, exponent field in [emin, emax), 7 random mantissa bits."""
    bits = (torch.randint(0, 2, shape, generator=g) << 15) | (torch.randint(emin, emax, shape, generator=g) << 7) | torch.randint(0, 128, shape, generator=g)
    return (bits - 65536 * (bits >= 32768)).to(torch.int16).view(BF)


def _unit(g, *shape):
    """fp32 in (0, 1): integer / 2^23 (exact)."""
    return torch.randint(1, 1 << 23, shape, generator=g).float() / float(1 << 23)


def _digest(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    raw = t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()
    return np.frombuffer(hashlib.sha256(raw).digest(), dtype=np.uint8).copy()


def _fwd(lib, B, T, n_in, co, ks, d, gated, act, residual, seed):
    g = _gen(seed)
    nb, rows = len(ks), B * T
    x = _bf(g, rows, n_in + 8).to(DEV)
    res = _bf(g, rows, nb * co + 16).to(DEV) if residual else None
    keep, tab = [], []
    for i, k in enumerate(ks):
        w = _bf(g, co, k, n_in, emin=116, emax=123).to(DEV)
        gate = _unit(g, B, n_in).to(DEV) if gated else None
        scale, shift, slope = (0.5 + _unit(g, co)).to(DEV), (_unit(g, co) - 0.5).to(DEV), (0.5 * _unit(g, co)).to(DEV)
        keep += [w, gate, scale, shift, slope]
        tab.append([k, w.data_ptr(), 0 if gate is None else gate.data_ptr(), scale.data_ptr(), shift.data_ptr(), slope.data_ptr(), 8 + i * co, 8 + i * co])
    tab = torch.tensor(tab, dtype=torch.int64)
    inputs = [x] + [t for t in keep if t is not None] + ([res] if residual else [])
    outs = {}
    for save in (False, True):
        out = torch.full((rows + 1, nb * co + 24), SENT, dtype=BF, device=DEV)
        acc = torch.full((rows + 1, nb * co + 8), SENT, device=DEV)
        common = (x.data_ptr(), x.stride(0), B, T, n_in, d, nb, tab.data_ptr(), co, act, out.data_ptr(), out.stride(0),
                  None if res is None else res.data_ptr(), 0 if res is None else res.stride(0), 2 if residual else 0)
        rc = lib.svsr_tconv_fwd_save(*common, acc.data_ptr(), acc.stride(0), None) if save else lib.svsr_tconv_fwd(*common, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs["out<save>" if save else "out"] = out
        if save:
            outs["acc"] = acc
    return inputs, outs


def _dgrad(lib, B, T, n_out, co, ks, d, gated, addend, cadd, seed):
    g = _gen(seed)
    nb, rows = len(ks), B * T
    dy = _bf(g, rows, nb * co + 8).to(DEV)
    x = _bf(g, rows, n_out + 8).to(DEV)
    add = _bf(g, rows, n_out).to(DEV)
    ca = _unit(g, B, n_out).to(DEV)
    keep, tab = [], []
    for i, k in enumerate(ks):
        wt = _bf(g, n_out, k, co, emin=116, emax=123).to(DEV)
        gate = _unit(g, B, n_out).to(DEV) if gated else None
        keep += [wt, gate]
        tab.append([k, wt.data_ptr(), 0 if gate is None else gate.data_ptr(), 8 + i * co])
    tab = torch.tensor(tab, dtype=torch.int64)
    out = torch.full((rows + 1, n_out + 16), SENT, dtype=BF, device=DEV)
    if addend:                                                                # in place, as the model's feature-stack gradient is accumulated
        out[:rows, :n_out] = add
    gpart = torch.full((nb * B * ((T + 31) // 32) * n_out + 32,), SENT, device=DEV)
    rc = lib.svsr_tconv_dgrad(dy.data_ptr(), dy.stride(0), B, T, co, d, nb, tab.data_ptr(), n_out, x.data_ptr() if gated else None, x.stride(0),
                              out.data_ptr() if addend else None, out.stride(0), ca.data_ptr() if cadd else None, 1.0 / T, out.data_ptr(), out.stride(0),
                              gpart.data_ptr() if gated else None, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [dy, x, add, ca] + [t for t in keep if t is not None], dict(out=out, gpart=gpart)


def _wgrad(lib, B, T, n_in, co, k, d, gated, n_valid, add, splits, seed):
    g = _gen(seed)
    rows = B * T
    x = _bf(g, rows, n_in + 8).to(DEV)
    dy = _bf(g, rows, co + 16).to(DEV)
    gate = _unit(g, B, n_in).to(DEV) if gated else None
    dw = torch.full((co * n_valid * k + 64,), SENT, device=DEV)
    dw[32: 32 + co * n_valid * k] = (_unit(g, co * n_valid * k) - 0.5).to(DEV)
    dw0 = dw.clone()
    part = torch.empty(splits * co * k * n_in, device=DEV)
    rc = lib.svsr_tconv_wgrad(x.data_ptr(), x.stride(0), None if gate is None else gate.data_ptr(), dy.data_ptr() + 16, dy.stride(0), B, T, n_in, co, k, d,
                              splits, part.data_ptr(), dw.data_ptr() + 128, n_valid, add, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [x, dy, dw0] + ([gate] if gated else []), dict(dw=dw)


ACTS = {"swish_res": (2, True), "prelu": (3, False), "relu": (1, False), "none": (0, False)}          # name -> (act, Swish residual)
DROP_KEY = 0x9E3779B9


def _i32(vals):
    return torch.tensor(list(vals), dtype=torch.int32)


def _epi_inputs(g, rows, erows, C, residual):
    """dy bf16, acc fp32 in (-2, 2), scale / shift / slope fp32 [C], res bf16 or None; every row pitch wider than C."""
    dy = _bf(g, rows, C + 8).to(DEV)
    acc = ((_unit(g, erows, C + 8) - 0.5) * 4.0).to(DEV)
    scale, shift, slope = (0.5 + _unit(g, C)).to(DEV), (_unit(g, C) - 0.5).to(DEV), (0.5 * _unit(g, C)).to(DEV)
    res = _bf(g, rows, C + 16).to(DEV) if residual else None
    return dy, acc, scale, shift, slope, res


def _epi(lib, B, T, co, nb, act, residual, seed):
    """svsr_tconv_epi_bwd over B * T rows, then svsr_tconv_epi_bwd_bs on the same inputs without halo and dropout."""
    g = _gen(seed)
    rows, C = B * T, nb * co
    dy, acc, scale, shift, slope, res = _epi_inputs(g, rows, rows, C, residual)
    blocks = (rows + 63) // 64
    outs = {}
    for bs in (False, True):
        dacc = torch.full((rows + 1, C + 24), SENT, dtype=BF, device=DEV)
        dres = torch.full((rows + 1, C + 8), SENT, dtype=BF, device=DEV)
        sums = torch.full((4 * C + 32,), SENT, device=DEV)
        part = torch.empty(blocks * 4 * C, device=DEV)
        r = (None, 0) if res is None else (res.data_ptr(), res.stride(0))
        dr = (None, 0) if res is None else (dres.data_ptr(), dres.stride(0))
        if bs:
            h = _i32([0] * nb)
            rc = lib.svsr_tconv_epi_bwd_bs(dy.data_ptr(), dy.stride(0), acc.data_ptr(), acc.stride(0), B, T, C, co, 0, nb, h.data_ptr(), act,
                                           scale.data_ptr(), shift.data_ptr(), slope.data_ptr(), *r, 2 if residual else 0, 0, 0.0, *dr,
                                           part.data_ptr(), sums.data_ptr(), None)
        else:
            rc = lib.svsr_tconv_epi_bwd(dy.data_ptr(), dy.stride(0), acc.data_ptr(), acc.stride(0), rows, C, act, scale.data_ptr(), shift.data_ptr(),
                                        slope.data_ptr(), *r, 2 if residual else 0, dacc.data_ptr(), dacc.stride(0), *dr, part.data_ptr(),
                                        sums.data_ptr(), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        if bs:
            outs.update({"dres<bs>": dres, "sums<bs>": sums})
        else:
            outs.update(dacc=dacc, dres=dres, sums=sums)
    return [dy, acc, scale, shift, slope] + ([res] if residual else []), outs


def _epibs(lib, B, T, co, hs, hmax, act, residual, p, seed):
    """One batch-statistic stage's epilogue, forward and both backward passes, on the extended axis."""
    g = _gen(seed)
    nb, rows, erows = len(hs), B * T, B * (T + 2 * hmax)
    C = nb * co
    dy, acc, scale, shift, slope, res = _epi_inputs(g, rows, erows, C, residual)
    mean, invstd, ca, cb = (_unit(g, C) - 0.5).to(DEV), (0.5 + _unit(g, C)).to(DEV), (0.25 * (_unit(g, C) - 0.5)).to(DEV), (0.25 * (_unit(g, C) - 0.5)).to(DEV)
    h = _i32(hs)
    out = torch.full((rows + 1, C + 24), SENT, dtype=BF, device=DEV)
    dres = torch.full((rows + 1, C + 8), SENT, dtype=BF, device=DEV)
    sums = torch.full((4 * C + 32,), SENT, device=DEV)
    dacc = torch.full((erows + 1, C + 24), SENT, dtype=BF, device=DEV)
    part = torch.empty(((rows + 63) // 64) * 4 * C, device=DEV)
    r = (None, 0) if res is None else (res.data_ptr(), res.stride(0))
    dr = (None, 0) if res is None else (dres.data_ptr(), dres.stride(0))
    geo = (acc.data_ptr(), acc.stride(0), B, T, C, co, hmax, nb, h.data_ptr(), act, scale.data_ptr(), shift.data_ptr(), slope.data_ptr(), *r,
           2 if residual else 0, DROP_KEY, p)
    for rc in (lib.svsr_tconv_apply(*geo, out.data_ptr(), out.stride(0), None),
               lib.svsr_tconv_epi_bwd_bs(dy.data_ptr(), dy.stride(0), *geo, *dr, part.data_ptr(), sums.data_ptr(), None),
               lib.svsr_tconv_bn_bwd(dy.data_ptr(), dy.stride(0), *geo, mean.data_ptr(), invstd.data_ptr(), ca.data_ptr(), cb.data_ptr(), dacc.data_ptr(),
                                     dacc.stride(0), None)):
        assert rc == 0, rc
    torch.cuda.synchronize()
    return [dy, acc, scale, shift, slope, mean, invstd, ca, cb] + ([res] if residual else []), dict(out=out, dres=dres, sums=sums, dacc=dacc)


def _npool(lib, B, T, C, seed):
    """norm5 + masked mean backward in both statistics modes: a fractional mask, the second clip's all zeros."""
    g = _gen(seed)
    rows = B * T
    dh, dpooled, x = _bf(g, rows, C).to(DEV), _bf(g, B, C).to(DEV), _bf(g, rows, C + 8).to(DEV)
    mask = _unit(g, B, T)
    mask[1] = 0.0
    mask = mask.to(DEV)
    scale, mean, invstd = (0.5 + _unit(g, C)).to(DEV), (_unit(g, C) - 0.5).to(DEV), (0.5 + _unit(g, C)).to(DEV)
    ca, cb = (0.25 * (_unit(g, C) - 0.5)).to(DEV), (0.25 * (_unit(g, C) - 0.5)).to(DEV)
    dx = torch.full((rows + 1, C + 16), SENT, dtype=BF, device=DEV)
    dx_bs = torch.full((rows + 1, C + 16), SENT, dtype=BF, device=DEV)
    sums = torch.full((2 * C + 32,), SENT, device=DEV)
    part = torch.empty(B * 2 * C, device=DEV)
    head = (dh.data_ptr(), dpooled.data_ptr(), x.data_ptr(), x.stride(0), B, T, C, scale.data_ptr())
    for rc in (lib.svsr_tcn_norm_pool_bwd(*head, mask.data_ptr(), dx.data_ptr(), dx.stride(0), part.data_ptr(), sums.data_ptr(), None),
               lib.svsr_tcn_norm_pool_bwd_bs(*head, mean.data_ptr(), invstd.data_ptr(), ca.data_ptr(), cb.data_ptr(), mask.data_ptr(), dx_bs.data_ptr(),
                                             dx_bs.stride(0), None)):
        assert rc == 0, rc
    torch.cuda.synchronize()
    return [dh, dpooled, x, mask, scale, mean, invstd, ca, cb], {"dx": dx, "sums": sums, "dx<bs>": dx_bs}


def _cases():
    """name -> (function, arguments).  Seeds are fixed per case; B, T, channels as the module docstring says."""
    B, T, n_in, co = 3, 33, 128, 64
    c = {}
    for k, d in KD:
        for gated in (False, True):
            tag = f"k{k}d{d}{'g' if gated else ''}"
            c[f"fwd_{tag}"] = (_fwd, (B, T, n_in, co, (k,), d, gated, 3 if k == 5 else 2, k == 3, 100 + 10 * k + gated))
            c[f"dgrad_{tag}"] = (_dgrad, (B, T, n_in, co, (k,), d, gated, not gated, gated, 200 + 10 * k + gated))
            c[f"dgrad_{tag}_add_cadd"] = (_dgrad, (B, T, n_in, co, (k,), d, gated, True, True, 300 + 10 * k + gated))
            for add in (0, 1):
                c[f"wgrad_{tag}_add{add}"] = (_wgrad, (B, T, n_in, co, k, d, gated, 120 if add else n_in, add, 2, 400 + 10 * k + 2 * gated + add))
    c["fwd_3br_g_res"] = (_fwd, (B, T, n_in, co, (3, 5, 7), 2, True, 2, True, 500))
    c["fwd_3br"] = (_fwd, (B, T, n_in, co, (7, 1, 5), 3, False, 0, False, 501))
    c["dgrad_3br_g_add_cadd"] = (_dgrad, (B, T, n_in, co, (3, 5, 7), 2, True, True, True, 502))
    c["dgrad_3br"] = (_dgrad, (B, T, n_in, co, (7, 1, 5), 3, False, False, False, 503))
    c["dgrad_2chunks_g"] = (_dgrad, (B, T, 64, 128, (5, 3), 2, True, True, False, 504))          # co = 128: two staged chunks in dgrad too
    c["fwd_T1"] = (_fwd, (3, 1, n_in, co, (3,), 1, True, 2, False, 600))
    c["dgrad_T1"] = (_dgrad, (3, 1, n_in, co, (3,), 1, True, True, True, 601))
    c["wgrad_T1"] = (_wgrad, (3, 1, n_in, co, 3, 1, True, 120, 1, 1, 602))
    for j, (tag, (act, residual)) in enumerate(ACTS.items()):
        c[f"epi_{tag}"] = (_epi, (B, T, co, 2, act, residual, 700 + j))
    c["epi_rows1"] = (_epi, (1, 1, co, 2, 2, True, 710))          # (a single row is a single clip of a single frame for the _bs entry)
    for T_ in (T, 1):
        for p in (0.0, 0.2):
            for tag in ("swish_res", "prelu"):
                c[f"epibs_T{T_}_p{int(p * 10)}_{tag}"] = (_epibs, (B, T_, co, (1, 15), 15, *ACTS[tag], p, 800 + 10 * (T_ == 1) + 2 * (p > 0) + (tag == "prelu")))
        c[f"npool_T{T_}"] = (_npool, (B, T_, 64, 900 + (T_ == 1)))
    return c


CASES = _cases()


def _run(name):
    """-> {"<case>/in": digest of the inputs, "<case>/<output>": digest} on the loaded library."""
    from syncvsr_amd import _lib

    fn, args = CASES[name]
    inputs, outs = fn(_lib.load(), *args)
    h = hashlib.sha256()
    for t in inputs:
        h.update(_digest(t).tobytes())
    got = {f"{name}/in": np.frombuffer(h.digest(), dtype=np.uint8).copy()}
    for k, t in outs.items():
        got[f"{name}/{k}"] = _digest(t)
    return got


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k].copy() for k in z.files}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_output_bits_match_the_recorded_build(name, golden):
    got = _run(name)
    assert sorted(k for k in golden if k.startswith(name + "/")) == sorted(got), "the golden holds other outputs for this case"
    assert bytes(got[f"{name}/in"]) == bytes(golden[f"{name}/in"]), "the seeded inputs differ from the recorded ones: nothing can be compared"
    for k, v in got.items():
        assert bytes(v) == bytes(golden[k]), f"{k}: output bits differ from the recorded build"
    if f"{name}/out<save>" in got:
        assert bytes(got[f"{name}/out"]) == bytes(got[f"{name}/out<save>"]), "the saving forward stores other output bits"
    for k in ("dres", "sums"):
        if f"{name}/{k}<bs>" in got:
            assert bytes(got[f"{name}/{k}"]) == bytes(got[f"{name}/{k}<bs>"]), f"{k}: the batch-statistic pass 1 without halo and dropout stores other bits"


def test_golden_covers_exactly_these_cases(golden):
    assert {k.split("/")[0] for k in golden} == set(CASES)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_dctcn_bits.py --record [path]")
    path = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN
    rec = {}
    for n in CASES:
        rec.update(_run(n))
    np.savez(path, **rec)
    print(f"recorded {len(rec)} digests of {len(CASES)} cases -> {path}")
