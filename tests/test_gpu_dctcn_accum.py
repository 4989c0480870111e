"""Gradient accumulation in dctcn_train.DCTCNTrainStep (accumulate=N; Lightning's accumulate_grad_batches), single process, B = 2, the tiny
configuration (T = 7, 40 x 40), total_steps = 5, clip 1.0, given lams and seeds.

Every equality is BIT FOR BIT.  The definition of a window is written by hand from DCTCNLightningModule.loss_and_grads (loss_scale = 1/N,
accumulate False for the first micro-batch and True for the others) and ops.AdamW — entry points whose parity with the reference
tests/test_gpu_dctcn_whole_grads.py and tests/test_gpu_dctcn_trainstep.py pin — so no tolerance is needed."""
import pytest
import torch

import dctcn_dp_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _step(accumulate, state=None, seed=C.SEED):
    from syncvsr_amd.dctcn_train import DCTCNTrainStep

    cfg, dims, sd, batch = C.case()
    model = C.build_model(cfg, sd if state is None else state["model"], DEV)
    ts = DCTCNTrainStep(model, C.TOTAL, seed=seed, accumulate=accumulate)
    if state is not None:
        ts.load_state_dict(state["opt"])
    return cfg, model, ts, (C.to_args(batch, DEV), C.to_args(C.second_batch(cfg), DEV))


def _hand(n_windows: int, scale: float, per_window: int):
    """`n_windows` windows of `per_window` micro-batches (alternating the two), each loss times `scale`, written out.
    -> (model, adamw, metrics per micro-step)"""
    cfg, dims, sd, batch = C.case()
    model = C.build_model(cfg, sd, DEV)
    adamw = C.hand_adamw(model, cfg)
    mbs = (C.to_args(batch, DEV), C.to_args(C.second_batch(cfg), DEV))
    outs, i = [], 0
    for _ in range(n_windows):
        for pos in range(per_window):
            o = model.loss_and_grads(**mbs[i % 2], loss_scale=scale, accumulate=pos > 0, dropout_seed=C.SEED + i, lam=C.LAMS[i])
            outs.append(C.metrics_of(o))
            i += 1
        C.hand_optimise(model, adamw)
    return model, adamw, outs


def _same_state(model, ts, hmodel, hadamw) -> None:
    st, hs = model.store(), hmodel.store()
    assert torch.equal(st.flat, hs.flat), f"{int((st.flat != hs.flat).sum())} parameters differ"
    assert torch.equal(ts.m, hadamw.m) and torch.equal(ts.v, hadamw.v), "AdamW's moments differ"
    assert torch.equal(st.bufflat, hs.bufflat), "running statistics differ"
    assert torch.equal(ts.opt_state, hadamw.opt_state), "the device step state differs"


def test_a_window_of_two_is_the_by_hand_sequence():
    cfg, model, ts, mbs = _step(2)
    outs = [C.metrics_of(ts.step(mbs[i % 2], lam=C.LAMS[i])) for i in range(2)]
    hmodel, hadamw, houts = _hand(1, 0.5, 2)
    torch.cuda.synchronize()
    for a, b in zip(outs, houts):
        C.same_metrics(a, b)
    _same_state(model, ts, hmodel, hadamw)
    assert ts.state()["step"] == 1 and ts.steps == 1 and ts.micro_steps == 2
    # the returned metrics are the micro-batch's own, not scaled by 1 / N: those of a full-scale backward of the same micro-batch
    fresh = C.build_model(cfg, C.case()[2], DEV)
    full = fresh.loss_and_grads(**mbs[0], loss_scale=1.0, dropout_seed=C.SEED, lam=C.LAMS[0])
    C.same_metrics(outs[0], C.metrics_of(full))
    assert float(outs[0]["loss_total"]) > 0.0


def test_a_middle_micro_step_moves_nothing_but_statistics_and_gradients():
    cfg, model, ts, mbs = _step(3)
    flat0 = model.store().flat.clone()
    buf0 = model.store().bufflat.clone()
    ts.step(mbs[0], lam=C.LAMS[0])
    prep = model._prep
    assert prep is not None
    w = prep["t0"]["branches"][0]["w"]
    ptr, bits = w.data_ptr(), w.clone()
    ts.step(mbs[1], lam=C.LAMS[1])          # the middle micro-step
    torch.cuda.synchronize()
    assert torch.equal(model.store().flat, flat0), "a middle micro-step changed parameters"
    assert ts.steps == 0 and ts.micro_steps == 2 and ts.state()["step"] == 0 and ts.state()["micro_step"] == 2
    assert model._prep is prep and prep["t0"]["branches"][0]["w"].data_ptr() == ptr, "the prepared weight copies were rebuilt inside a window"
    assert torch.equal(prep["t0"]["branches"][0]["w"], bits)
    assert not torch.equal(model.store().bufflat, buf0), "running statistics advance in every micro-step"
    ts.step(mbs[0], lam=C.LAMS[2])          # the last one: the optimiser runs and the copies are stale
    torch.cuda.synchronize()
    assert ts.steps == 1 and ts.state()["step"] == 1 and ts.state()["micro_step"] == 0
    assert model._prep is None
    assert not torch.equal(model.store().flat, flat0)


def test_flush_steps_on_a_partial_window_and_on_nothing_at_a_boundary():
    cfg, model, ts, mbs = _step(3)
    assert ts.flush() is False
    for i in range(2):
        ts.step(mbs[i % 2], lam=C.LAMS[i])
    assert ts.flush() is True          # two of three micro-batches: the gradient keeps its 1 / 3 scale
    hmodel, hadamw, _ = _hand(1, 1.0 / 3, 2)
    torch.cuda.synchronize()
    _same_state(model, ts, hmodel, hadamw)
    assert ts.steps == 1 and ts.state()["step"] == 1
    assert ts.flush() is False
    assert ts.state()["step"] == 1


def test_a_state_dict_taken_inside_a_window_resumes_it_bit_for_bit():
    cfg, ma, ta, mbs = _step(2)
    outs_a = [C.metrics_of(ta.step(mbs[i % 2], lam=C.LAMS[i])) for i in range(4)]
    cfg, mb, tb, _ = _step(2)
    tb.step(mbs[0], lam=C.LAMS[0])
    saved = tb.state_dict()
    assert "accum_window" in saved and saved["accum_grad"].numel() == mb.store().numel
    state = dict(model={k: v.detach().cpu().clone() for k, v in mb.state_dict().items()},
                 opt={k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in saved.items()})
    del mb, tb
    with pytest.raises(ValueError):
        _step(3, state=state)          # a window of another length cannot finish this one
    cfg, mc, tc, _ = _step(2, state=state, seed=0)          # (the seed comes back with the state)
    assert tc.state()["micro_step"] == 1 and tc.micro_steps == 1 and tc.steps == 0
    outs_c = [C.metrics_of(tc.step(mbs[i % 2], lam=C.LAMS[i])) for i in range(1, 4)]
    torch.cuda.synchronize()
    for a, c in zip(outs_a[1:], outs_c):
        C.same_metrics(a, c)
    assert torch.equal(ma.store().flat, mc.store().flat) and torch.equal(ma.store().bufflat, mc.store().bufflat)
    assert torch.equal(ta.m, tc.m) and torch.equal(ta.v, tc.v) and torch.equal(ta.opt_state, tc.opt_state)
    assert tc.state()["step"] == 2
    assert "accum_window" not in tc.state_dict()          # at a window boundary the state keeps today's keys


def test_an_exception_inside_a_micro_step_abandons_the_window():
    cfg, model, ts, mbs = _step(2)
    for i in range(2):
        ts.step(mbs[i % 2], lam=C.LAMS[i])
    torch.cuda.synchronize()
    flat1, m1 = model.store().flat.clone(), ts.m.clone()
    ts.step(mbs[0], lam=C.LAMS[2])
    bad = dict(mbs[1], labels=mbs[1]["labels"].unsqueeze(1).repeat(1, 2))          # [B, 2]: refused on the host, nothing is launched
    with pytest.raises(ValueError, match="labels"):
        ts.step(bad, lam=C.LAMS[3])
    torch.cuda.synchronize()
    assert ts.state()["micro_step"] == 0 and ts.steps == 1 and ts.state()["step"] == 1
    assert torch.equal(model.store().flat, flat1) and torch.equal(ts.m, m1), "the abandoned window reached the parameters"
    assert ts.flush() is False          # nothing is left to step on
    # the next step() starts a new window: its first micro-step stores (zero-fills) instead of adding to what the abandoned one left
    o = ts.step(mbs[0], lam=C.LAMS[2])
    grad = model.store().grad.clone()
    twin = C.build_model(cfg, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, DEV)
    torch.cuda.synchronize()
    assert torch.equal(model.store().flat, flat1)
    # (the twin starts from the statistics AFTER the micro-step: only the gradient of a fresh, storing backward is compared — it depends on
    # the parameters and the batch, not on the running statistics)
    twin.loss_and_grads(**mbs[0], loss_scale=0.5, accumulate=False, dropout_seed=C.SEED + ts.micro_steps - 1, lam=C.LAMS[2])
    torch.cuda.synchronize()
    assert torch.equal(grad, twin.store().grad), "the first micro-step after an abandoned window added to stale gradients"
    assert bool(torch.isfinite(o["loss_total"]))


def test_three_windows_on_one_pair_of_micro_batches_lower_the_loss():
    cfg, model, ts, mbs = _step(2)
    totals = []
    for w in range(3):
        outs = [ts.step(mbs[i], lam=0.0) for i in range(2)]
        totals.append(sum(float(o["loss_total"]) for o in outs) / 2)
    print("mean loss_total per window:", totals)
    assert ts.state()["step"] == 3 and ts.state()["skipped"] == 0
    assert totals[2] < totals[0], totals
