#!/usr/bin/env python
"""Persistent 8-wave kernel (csrc/igemm_p8.hip) against the 4-wave kernel on the trunk's stride-1 3x3 shapes: results (bitwise for the plain
epilogues: same MFMA instruction, same accumulation order) and launch time.  Run on the GPU box: python scripts/probes/p8_check.py"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from syncvsr_amd import ops

dev = torch.device("cuda:0")
BF16 = torch.bfloat16
torch.manual_seed(0)


def timeit(fn, n=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def run(N, H, C, reps=30):
    x = (torch.randn(N, H, H, C, device=dev) * 0.5).to(BF16)
    w = (torch.randn(C, 3, 3, C, device=dev) * 0.05).to(BF16)
    dy = (torch.randn(N, H, H, C, device=dev) * 0.5).to(BF16)
    add = (torch.randn(N, H, H, C, device=dev) * 0.5).to(BF16)
    xb = (torch.randn(N, H, H, C, device=dev)).to(BF16)
    yb = torch.relu(torch.randn(N, H, H, C, device=dev)).to(BF16)
    mean = torch.randn(C, device=dev) * 0.1
    rstd = torch.rand(C, device=dev) + 0.5
    gamma = torch.rand(C, device=dev) + 0.5
    beta = torch.randn(C, device=dev) * 0.1
    flops = 2.0 * N * H * H * C * C * 9
    res = {}
    for mode in (0, 1):
        ops.tune("p8", mode)
        out, st = ops.conv2d_fwd(x, w, 3, 1, 1, want_stats=True)
        pl = ops.conv_plan(0, N, H, H, C, 3, 1, 1)
        stats = st[0][: st[1] * 2 * C].view(st[1], 2, C).sum(0).clone()
        t_f = timeit(lambda: ops.conv2d_fwd(x, w, 3, 1, 1, want_stats=True), reps)
        dx = ops.conv2d_dgrad(dy, w, 3, 1, 1, (H, H), addend=add.clone())       # (in place: the result lands in the addend's buffer)
        scratch_add = add.clone()
        t_d = timeit(lambda: ops.conv2d_dgrad(dy, w, 3, 1, 1, (H, H), addend=scratch_add), reps)
        g, gst = ops.conv2d_dgrad_bn(dy, w, 3, 1, 1, (H, H), add.clone(), yb, xb, mean, rstd, gamma, beta, 1)
        gs = gst[0][: gst[1] * 2 * C].view(gst[1], 2, C).sum(0).clone()
        g2, gst2 = ops.conv2d_dgrad_bn(dy, w, 3, 1, 1, (H, H), None, None, xb, mean, rstd, gamma, beta, 1)
        gs2 = gst2[0][: gst2[1] * 2 * C].view(gst2[1], 2, C).sum(0).clone()
        t_b = timeit(lambda: ops.conv2d_dgrad_bn(dy, w, 3, 1, 1, (H, H), None, None, xb, mean, rstd, gamma, beta, 1), reps)
        scratch_add2 = add.clone()
        t_b2 = timeit(lambda: ops.conv2d_dgrad_bn(dy, w, 3, 1, 1, (H, H), scratch_add2, yb, xb, mean, rstd, gamma, beta, 1), reps)
        res[mode] = dict(out=out.clone(), stats=stats, dx=dx.clone(), g=g.clone(), gs=gs, g2=g2.clone(), gs2=gs2, label=pl.label, t=(t_f, t_d, t_b, t_b2))
    a, b = res[0], res[1]
    ok = True
    for k in ("out", "dx", "g", "g2"):
        same = torch.equal(a[k], b[k])
        ok &= same
        if not same:
            d = (a[k].float() - b[k].float()).abs()
            print(f"  {k}: MISMATCH max {d.max().item():.4g} frac {(d > 0).float().mean().item():.4g}")
    for k in ("stats", "gs", "gs2"):
        rel = ((a[k] - b[k]).abs().max() / a[k].abs().max()).item()
        ok &= rel < 1e-4
        print(f"  {k}: rel diff {rel:.2e}")
    # two runs of the new kernel are bit-identical
    ops.tune("p8", 1)
    o1, s1 = ops.conv2d_fwd(x, w, 3, 1, 1, want_stats=True)
    s1 = s1[0][: s1[1] * 2 * C].clone()
    o2, s2 = ops.conv2d_fwd(x, w, 3, 1, 1, want_stats=True)
    rep = torch.equal(o1, o2) and torch.equal(s1, s2[0][: s2[1] * 2 * C])
    print(f"N={N} {H}x{H} C={C}: {'OK' if ok else 'FAIL'} reproducible={rep} | {a['label']} fwd/dgrad+add/dgrad+bn(x)/dgrad+bn(y,add) us {a['t'][0]:.1f} {a['t'][1]:.1f} {a['t'][2]:.1f} {a['t'][3]:.1f} "
          f"({flops / a['t'][0] / 1e6:.0f} TF) | {b['label']} {b['t'][0]:.1f} {b['t'][1]:.1f} {b['t'][2]:.1f} {b['t'][3]:.1f} ({flops / b['t'][0] / 1e6:.0f} TF)")
    return ok and rep


if __name__ == "__main__":
    ops.tune("p8_min_items", 1)
    if "--order" in sys.argv:
        ops.tune("p8", 1)
        for (N, H, C) in ((928, 11, 128), (928, 6, 256), (928, 22, 128)):
            x = (torch.randn(N, H, H, C, device=dev) * 0.5).to(BF16); w = (torch.randn(C, 3, 3, C, device=dev) * 0.05).to(BF16)
            dy = (torch.randn(N, H, H, C, device=dev) * 0.5).to(BF16); add = (torch.randn(N, H, H, C, device=dev) * 0.5).to(BF16)
            xb = torch.randn(N, H, H, C, device=dev).to(BF16); yb = torch.relu(torch.randn(N, H, H, C, device=dev)).to(BF16)
            mean, rstd = torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5
            gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
            ref = None
            for stg in (1, 3, 1, 3):
                ops.tune("p8_stagger", stg)
                sa = add.clone()
                g, gst = ops.conv2d_dgrad_bn(dy, w, 3, 1, 1, (H, H), add.clone(), yb, xb, mean, rstd, gamma, beta, 1)
                key = (g.clone(), gst[0][: gst[1] * 2 * C].clone())
                if ref is None:
                    ref = key
                same = torch.equal(ref[0], key[0]) and torch.equal(ref[1], key[1])
                t_f = timeit(lambda: ops.conv2d_fwd(x, w, 3, 1, 1, want_stats=True), 30)
                t_b = timeit(lambda: ops.conv2d_dgrad_bn(dy, w, 3, 1, 1, (H, H), None, None, xb, mean, rstd, gamma, beta, 1), 30)
                t_b2 = timeit(lambda: ops.conv2d_dgrad_bn(dy, w, 3, 1, 1, (H, H), sa, yb, xb, mean, rstd, gamma, beta, 1), 30)
                print(f"N={N} {H}x{H} C={C} p8_stagger={stg}: fwd {t_f:.1f}  bn(x) {t_b:.1f}  bn(y,add) {t_b2:.1f} us  identical={same}")
        ops.tune("p8_stagger", 1)
        sys.exit(0)
    if "--sweep" in sys.argv:
        x2 = (torch.randn(928, 11, 11, 128, device=dev) * 0.5).to(BF16); w2 = (torch.randn(128, 3, 3, 128, device=dev) * 0.05).to(BF16)
        x3 = (torch.randn(928, 6, 6, 256, device=dev) * 0.5).to(BF16); w3 = (torch.randn(256, 3, 3, 256, device=dev) * 0.05).to(BF16)
        x1 = (torch.randn(928, 22, 22, 128, device=dev) * 0.5).to(BF16)
        ops.tune("p8", 1)
        for stg in (1, 0):
            for grid in (0, 224, 192):
                ops.tune("p8_stagger", stg); ops.tune("p8_grid", grid)
                t2 = timeit(lambda: ops.conv2d_fwd(x2, w2, 3, 1, 1, want_stats=True), 30)
                t3 = timeit(lambda: ops.conv2d_fwd(x3, w3, 3, 1, 1, want_stats=True), 30)
                t1 = timeit(lambda: ops.conv2d_fwd(x1, w2, 3, 1, 1, want_stats=True), 10)
                print(f"stagger {stg} grid {grid}: layer2 {t2:.1f} us  layer3 {t3:.1f} us  22x22x128 {t1:.1f} us")
        sys.exit(0)
    good = True
    good &= run(16, 11, 128, 5)           # small: holes, partial tiles (the 4-wave kernel splits K here: results agree to rounding only)
    good &= run(928, 11, 128)
    good &= run(928, 6, 256)
    good &= run(928, 3, 512)
    good &= run(928, 22, 128)
    print("ALL OK" if good else "SOME FAILED")
