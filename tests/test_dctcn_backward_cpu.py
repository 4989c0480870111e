"""CPU half of the DC-TCN backward: the C ABI of the new entry points, the Python-side shape refusals, who owns the host tables, the O(C)
chain rule from the per-channel sums to the BatchNorm / bias gradients, and the bf16 noise floor recorded in profiles/dctcn_backward.json."""
import gc
import types
import weakref

import pytest
import torch

from dctcn_backward_ref import CLASSES, measure_floor, recorded_floor

NEW = ("svsr_tconv_fwd_save", "svsr_tconv_epi_bwd", "svsr_tconv_dgrad", "svsr_tconv_wgrad", "svsr_tcn_se_bwd", "svsr_tcn_norm_pool_bwd",
       "svsr_tcn_fold")


def test_new_entry_points_are_declared_and_bound():
    from syncvsr_amd import _lib

    decl = _lib.parse_header()
    lib = _lib.load()
    for name in NEW:
        assert name in decl, name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(decl[name])
    # the three forward entry points keep their signatures
    assert [a for _, a in decl["svsr_tconv_fwd"]] == ["x", "x_pitch", "B", "T", "n_in", "d", "nb", "branches", "co", "act", "out", "out_pitch", "res",
                                                     "res_pitch", "res_act", "stream"]
    assert [a for _, a in decl["svsr_tconv_fwd_save"]][:15] == [a for _, a in decl["svsr_tconv_fwd"]][:15]


def test_python_side_shape_refusals():
    from syncvsr_amd import ops

    bf, f32 = torch.bfloat16, torch.float32
    x, dy = torch.zeros(8, 128, dtype=bf), torch.zeros(8, 64, dtype=bf)
    with pytest.raises(ValueError):
        ops.tconv_wgrad(x, dy, torch.zeros(64, 128, 9), B=2, T=4, n_in=128, co=64, k=9, d=1)                      # k > 7
    with pytest.raises(ValueError):
        ops.tconv_wgrad(x, dy, torch.zeros(64, 128, 7), B=2, T=4, n_in=128, co=64, k=7, d=6)                      # halo 18 > 16
    with pytest.raises(ValueError):
        ops.tconv_wgrad(x, dy, torch.zeros(64, 96, 3), B=2, T=4, n_in=96, co=64, k=3, d=1)                        # n_in % 64
    with pytest.raises(ValueError):
        ops.tconv_wgrad(x, dy, torch.zeros(64, 3, 128), B=2, T=4, n_in=128, co=64, k=3, d=1)                      # dw not [co, ci, k]
    with pytest.raises(ValueError):
        ops.tconv_dgrad(dy, B=2, T=4, co=64, d=1, n_out=128, out=torch.zeros(8, 128, dtype=bf),
                        branches=[dict(k=4, wt=torch.zeros(128, 4, 64, dtype=bf), dy_off=0)])                          # even k
    with pytest.raises(ValueError):
        ops.tconv_dgrad(dy, B=2, T=4, co=64, d=1, n_out=128, out=torch.zeros(8, 128, dtype=bf),
                        branches=[dict(k=3, wt=torch.zeros(128, 3, 64, dtype=bf), dy_off=0, gate=torch.zeros(2, 128))])  # gated without x
    with pytest.raises(ValueError):
        ops.tconv_dgrad(dy, B=2, T=4, co=64, d=1, n_out=128, out=torch.zeros(8, 64, dtype=bf),
                        branches=[dict(k=3, wt=torch.zeros(128, 3, 64, dtype=bf), dy_off=0)])                          # out narrower than n_out
    with pytest.raises(ValueError):
        ops.tconv_epi_bwd(torch.zeros(8, 96, dtype=bf), torch.zeros(8, 96), torch.zeros(96), torch.zeros(96), rows=8, C=96, act=2)
    with pytest.raises(ValueError):
        ops.tconv_epi_bwd(torch.zeros(8, 64, dtype=bf), torch.zeros(8, 64, dtype=bf), torch.zeros(64), torch.zeros(64), rows=8, C=64, act=2)  # acc not fp32
    with pytest.raises(ValueError):
        ops.tcn_norm_pool_bwd(torch.zeros(8, 100, dtype=bf), torch.zeros(2, 100, dtype=bf), torch.zeros(8, 100, dtype=bf), torch.zeros(100),
                              torch.zeros(2, 4), B=2, T=4, C=100, out=torch.zeros(8, 100, dtype=bf))
    with pytest.raises(ValueError):
        ops.tcn_se_bwd(torch.zeros(8, 4096, dtype=bf), torch.zeros(1, 256, 4096, dtype=bf), torch.zeros(1, 4096, 256, dtype=bf),
                       torch.zeros(1, 2, 4096), torch.zeros(1, 2, 1, 4096), [torch.zeros(256, 4096)], [torch.zeros(4096, 256)], B=2, T=4, n_in=4096)
    assert ops.tconv_wgrad_splits(96, 29, 512, 128) == ops.tconv_wgrad_splits(96, 29, 512, 128) <= 8
    assert ops.tconv_wgrad_splits(1, 1, 64, 64) == 1
    assert f32 is torch.float32


def _table_passing_calls(ops):
    """The four wrappers that hand a host table to the library, on CPU tensors of the smallest legal shapes: (name, index of the table among the
    C arguments, call)."""
    bf = torch.bfloat16
    B, T, n, R = 1, 1, 64, 4
    x, out, one = torch.zeros(B * T, n, dtype=bf), torch.zeros(B * T, n, dtype=bf), torch.ones(n)
    fbr = [dict(k=1, w=torch.zeros(n, 1, n, dtype=bf), scale=one, shift=one, out_off=0)]
    dbr = [dict(k=1, wt=torch.zeros(n, 1, n, dtype=bf), dy_off=0, gate=torch.ones(B, n))]
    w1, w2 = torch.zeros(1, R, n, dtype=bf), torch.zeros(1, n, R, dtype=bf)
    return [("svsr_tconv_fwd", 7, lambda: ops.tconv_fwd(x, B=B, T=T, n_in=n, d=1, branches=fbr, co=n, act=0, out=out)),
            ("svsr_tconv_fwd_save", 7, lambda: ops.tconv_fwd(x, B=B, T=T, n_in=n, d=1, branches=fbr, co=n, act=0, out=out, acc=torch.zeros(B * T, n))),
            ("svsr_tconv_dgrad", 7, lambda: ops.tconv_dgrad(x, B=B, T=T, co=n, d=1, branches=dbr, n_out=n, out=out, x=x)),
            ("svsr_tcn_se_bwd", 13, lambda: ops.tcn_se_bwd(x, w1, w2, torch.ones(1, B, n), torch.zeros(1, B, 1, n), [torch.zeros(R, n)],
                                                           [torch.zeros(n, R)], B=B, T=T, n_in=n))]


def test_host_tables_belong_to_the_recorder_and_to_nobody_outside_a_recording(monkeypatch):
    """A recorded step list re-reads a launch's host table at every replay: inside a recording every table-passing wrapper hands its table to
    the recorder (StepRecorder.keep); outside one the module retains none (there is no module-level list of them any more)."""
    from syncvsr_amd import ops

    calls, made = [], []
    real_tensor = torch.tensor

    def spy(*a, **k):                                       # every host table is a torch.tensor(..., dtype=int64)
        t = real_tensor(*a, **k)
        if t.dtype == torch.int64:
            made.append(weakref.ref(t))
        return t

    def fake_call(name, *args, **kw):
        alive = [r() for r in made if r() is not None]
        calls.append((name, args, [t for t in alive if t.data_ptr() == args[_IDX[name]]]))

    cases = _table_passing_calls(ops)
    _IDX = {name: idx for name, idx, _ in cases}
    monkeypatch.setattr(ops, "_call", fake_call)
    monkeypatch.setattr(ops, "STREAM_OVERRIDE", 0)
    monkeypatch.setattr(torch, "tensor", spy)
    stub = types.SimpleNamespace(keep=[], append_only=False)
    monkeypatch.setattr(ops, "_REC", stub)
    for name, idx, fn in cases:
        fn()
        got, args, tabs = calls[-1]
        assert got == name and len(tabs) == 1, (name, got, len(tabs))
        assert any(t is tabs[0] for t in stub.keep), f"{name}: the table it passed is not in the recorder's keep list"
        assert args[idx] == tabs[0].data_ptr() and tabs[0].dtype == torch.int64 and not tabs[0].is_cuda
    assert len(stub.keep) == len(cases)
    # outside a recording: the table the call read is gone once the wrapper has returned
    monkeypatch.setattr(ops, "_REC", None)
    del made[:], calls[:], tabs
    for name, idx, fn in cases:
        fn()
        assert calls[-1][0] == name and len(calls[-1][2]) == 1
    del calls[:]
    gc.collect()
    assert len(made) == len(cases) and all(r() is None for r in made), "a host table outlived its call outside a recording"
    assert not hasattr(ops, "_TCONV_TABLES") and not hasattr(ops, "tconv_fwd_save")


def test_host_chain_rule_matches_autograd_with_a_zero_batchnorm_weight():
    """(sum g, sum g * acc) -> d bn.weight, d bn.bias, d conv.bias against autograd of BatchNorm1d(eval)(conv + bias) in fp64."""
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(3)
    C, N = 7, 50
    acc = torch.randn(N, C, generator=g, dtype=torch.float64)
    dy = torch.randn(N, C, generator=g, dtype=torch.float64)
    w = torch.randn(C, generator=g, dtype=torch.float64)
    w[2] = 0.0                                              # scale == 0: nothing may be recovered by dividing by it
    beta, bias = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    mean, var = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.1
    leaves = [t.clone().requires_grad_(True) for t in (w, beta, bias)]
    y = torch.nn.functional.batch_norm(acc + leaves[2], mean, var, leaves[0], leaves[1], training=False, eps=ops.BN_EPS)
    (y * dy).sum().backward()
    dw, db, dcb = ops.bn_conv_param_grads(dy.sum(0), (dy * acc).sum(0), w, mean, var, bias)
    for got, ref in zip((dw, db, dcb), leaves):
        assert torch.isfinite(got).all()
        assert torch.allclose(got, ref.grad, rtol=1e-12, atol=1e-12)
    dw2, db2, none = ops.bn_conv_param_grads(dy.sum(0), (dy * acc).sum(0), w, mean, var, None)
    lv = [t.clone().requires_grad_(True) for t in (w, beta)]
    (torch.nn.functional.batch_norm(acc, mean, var, lv[0], lv[1], training=False, eps=ops.BN_EPS) * dy).sum().backward()
    assert none is None and torch.allclose(dw2, lv[0].grad, rtol=1e-12, atol=1e-12) and torch.allclose(db2, lv[1].grad, rtol=1e-12, atol=1e-12)


def test_recorded_bf16_floor_is_the_measured_one():
    """Reference against reference: the restatement with its bf16 rounding points against the same restatement in fp64 (tiny configuration).
    The recorded figures (profiles/dctcn_backward.json "bf16_floor") are what the GPU model test multiplies by 4."""
    now, rec = measure_floor(), recorded_floor()
    assert set(rec) == set(CLASSES) == set(now)
    for c in CLASSES:
        print(f"bf16 floor {c}: measured {now[c]:.4e} recorded {rec[c]:.4e}")
        assert 0 < now[c] < 0.05
        assert abs(now[c] - rec[c]) <= 0.05 * now[c], (c, now[c], rec[c])
