"""svsr_adamw_onecycle_step / _range on the GPU against torch.optim.AdamW + torch.optim.lr_scheduler.OneCycleLR on the CPU in fp32.

total_steps = 7: steps 0..3 are the four consecutive steps from step 0, steps 4..6 the three that end at total_steps - 1 — one run of seven
covers both windows, the moments carried through.  Bounds: those of tests/test_gpu_kernels.py::test_adamw_clip_schedule (parameters 1e-5 of
the largest value and 1e-5 relative L2; the bf16 shadow 8e-3 / 4e-3).  What the schedule adds is asserted by itself: the learning rate and
beta1 the kernel used, read from the device state after every step, lie within 2 ulp (fp32) of ops.onecycle_values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOTAL = 7
SIZES = (1, 255, 4 * 256 + 3, 4096 * 256 + 5)          # one element, a ragged block, several blocks, past the 4096-block grid cap


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def check(got, ref, name, max_tol, l2_tol):
    got, ref = got.detach().float().cpu(), ref.detach().float()
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    l2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    assert err <= max_tol * scale and l2 <= l2_tol, f"{name}: max err {err:.3e} (scale {scale:.3e}), rel L2 {l2:.3e}"


def within_ulps(a: float, b: float, ulps: int = 2) -> bool:
    b32 = np.float32(b)
    return abs(float(np.float32(a)) - float(b32)) <= ulps * float(np.spacing(np.abs(b32)))


def _torch_reference(p, grads, decay_end, sched_kw, betas, eps, wd, max_norm):
    """-> the parameters after every step, from torch's own optimiser and scheduler (decayed 2-D tensor | undecayed 1-D tensor)."""
    pa, pb = torch.nn.Parameter(p[:decay_end].clone().view(-1, 1)), torch.nn.Parameter(p[decay_end:].clone())
    groups = [g for g in ({"params": [pa], "weight_decay": wd}, {"params": [pb], "weight_decay": 0.0}) if g["params"][0].numel()]
    opt = torch.optim.AdamW(groups, lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=TOTAL, **sched_kw)
    out = []
    for i, g in enumerate(grads):
        pa.grad, pb.grad = g[:decay_end].clone().view(-1, 1), g[decay_end:].clone()
        torch.nn.utils.clip_grad_norm_([q for q in (pa, pb) if q.numel()], max_norm)
        opt.step()
        out.append(torch.cat((pa.detach().view(-1), pb.detach())).clone())
        if i + 1 < TOTAL:
            sch.step()
    return out


@pytest.mark.parametrize("pct", (0.0, 0.3))
@pytest.mark.parametrize("where", ("none", "middle", "all"))
@pytest.mark.parametrize("n", SIZES)
def test_onecycle_adamw_matches_torch(dev, n, where, pct):
    from syncvsr_amd import ops

    decay_end = {"none": 0, "middle": n // 2, "all": n}[where]
    g = torch.Generator().manual_seed(7 + n % 1000)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (3.0, 0.01, 1.0, 0.3, 2.0, 0.05, 1.0)]
    betas, eps, wd, max_norm = (0.9, 0.999), 1e-6, 1e-2, 1.0
    sched_kw = dict(max_lr=1e-2, pct_start=pct, anneal_strategy="cos", three_phase=False)
    ref = _torch_reference(p, grads, decay_end, sched_kw, betas, eps, wd, max_norm)
    sched = ops.onecycle_schedule(total_steps=TOTAL, **sched_kw)
    pd, md, vd = p.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    shadow = torch.zeros(n, dtype=BF, device=dev)
    state = torch.zeros(ops.ONECYCLE_STATE_WORDS, dtype=torch.int32, device=dev)
    for step, gr in enumerate(grads):
        gd = gr.to(dev)
        ops.grad_sumsq(gd, state)
        if step == 2:
            # the range form over the same elements without the advance: the counter stays, a second launch then advances it over nothing
            ops.adamw_onecycle_range(pd, gd, md, vd, shadow, 0, n, decay_end, betas[1], eps, wd, max_norm, sched, state, advance=False)
            assert ops.onecycle_state(state)["step"] == step, "advance=0 must leave the counter alone"
            ops.adamw_onecycle_range(pd, gd, md, vd, shadow, 0, 0, decay_end, betas[1], eps, wd, max_norm, sched, state, advance=True)
        else:
            ops.adamw_onecycle_step(pd, gd, md, vd, shadow, decay_end, betas[1], eps, wd, max_norm, sched, state)
        s = ops.onecycle_state(state)
        lr, beta1 = ops.onecycle_values(step, **sched)
        assert s["step"] == step + 1 and s["error"] == 0 and s["skipped"] == 0, s
        assert within_ulps(s["lr"], lr) and within_ulps(s["beta1"], beta1), (step, s, lr, beta1)
        if step in (3, TOTAL - 1):          # the end of either window
            check(pd, ref[step], f"p after step {step}", 1e-5, 1e-5)
            check(shadow, ref[step], f"shadow after step {step}", 8e-3, 4e-3)
        assert torch.equal(shadow, pd.to(BF)), "the bf16 shadow is the rounded parameter"
    # pct_start = 0: torch's first phase ends at step -1, the last step lands on min_lr exactly
    if pct == 0.0:
        assert within_ulps(ops.onecycle_state(state)["lr"], sched["min_lr"])
    # the step after the last: the error code, and nothing changes
    before = [t.clone() for t in (pd, md, vd, shadow)]
    ops.grad_sumsq(grads[0].to(dev), state)
    ops.adamw_onecycle_step(pd, grads[0].to(dev), md, vd, shadow, decay_end, betas[1], eps, wd, max_norm, sched, state)
    s = ops.onecycle_state(state)
    assert s["error"] == 1001 and s["step"] == TOTAL, s
    for a, b in zip(before, (pd, md, vd, shadow)):
        assert torch.equal(a, b)


def test_schedules_no_step_can_be_taken_from_are_refused(dev):
    from syncvsr_amd import _lib, ops

    x = torch.zeros(8, device=dev)
    state = torch.zeros(ops.ONECYCLE_STATE_WORDS, dtype=torch.int32, device=dev)
    sched = ops.onecycle_schedule(1e-2, 1, pct_start=1.0)
    with pytest.raises(_lib.SvsrError):
        ops.adamw_onecycle_step(x, x, x.clone(), x.clone(), None, 8, 0.999, 1e-6, 1e-2, 0.0, sched, state)
