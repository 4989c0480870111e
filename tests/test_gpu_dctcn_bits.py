"""Bit identity of the DC-TCN convolution kernels (csrc/dctcn.hip) across library builds: svsr_tconv_fwd, svsr_tconv_fwd_save,
svsr_tconv_dgrad and svsr_tconv_wgrad, driven through the C ABI alone, against tests/golden/dctcn_kernel_bits.npz.  The golden holds one
SHA-256 per output buffer (guard bands included), not the bits: the raw outputs of these cases come to about 2 MiB, twice what a committed
file may hold.  It is recorded by running this file as a program on the build to compare with:

    python tests/test_gpu_dctcn_bits.py --record

Inputs are assembled from integer draws of seeded CPU generators (bf16 bit patterns, fp32 = integer / 2^23), so they are the same bits on any
host; their digest is part of the golden and is checked first.  The operands have full mantissas and exponents spread over eight binades, so
that a changed summation order, a moved rounding of the gate product or a mis-staged row shows in the output bits.

Shapes: B = 3, T = 33 (two time tiles per clip, the second one row long; 6 slots, and with B = 3, T = 1 an odd slot count: the last
workgroup's second slot is empty), 128 staged channels (two chunks) into 64, every (k, d) of {(1, 1), (3, 1), (5, 2), (7, 5)} — the last a halo
of 15 rows, one short of TC_HALO."""
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
