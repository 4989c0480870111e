"""The downsample blocks' backward through model.py with the merged data gradient (ops.DGRAD2) on and off (-m gpu): the geometry of layer2.0
shrunk to 4 frames of 12 x 12 (a 48 x 48 clip of 4 frames: stem stride 2, pooling stride 2), with layer3.0 (6 x 6) and layer4.0 (3 x 3)
behind it.  Both forms must agree to the block tolerance of tests/test_gpu_blockwise.py (cosine >= 0.9999, norm ratio within 0.2 %) in every
parameter gradient of the block and in the gradient handed to the block below; a recorded native step list must replay the merged launch
to the eager bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
COS_FLOOR, RATIO_BAND = 0.9999, 0.002          # test_gpu_blockwise.py: one block, benchmark batch


def _cmp(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300)), float(a.norm() / (b.norm() + 1e-300))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def test_downsample_block_backward_merged_against_two_launches(dev):
    from syncvsr_amd import model as M
    from syncvsr_amd import ops
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.init import init_state_dict

    cfg = default_lrw_config(model__bert__num_hidden_layers=1)
    sd = init_state_dict(cfg, seed=11, perturb_norm=True)
    model = M.Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    st = model.store()
    st.refresh_shadows()
    g = torch.Generator().manual_seed(5)
    videos = torch.randn(1, 1, 4, 48, 48, generator=g).to(dev)
    blocks = list(M._trunk_blocks(model))
    down = [(bi, b[0]) for bi, b in enumerate(blocks) if b[4]]
    assert [p.split(".")[-2] for _, p in down] == ["layer2", "layer3", "layer4"]
    dfeats = None
    calls = {}

    def run(flag: bool):
        nonlocal dfeats
        before, ops.DGRAD2 = ops.DGRAD2, flag
        try:
            tape = {"_record_grads": {}}
            feats = M._frontend_forward(model, st, tape, videos, True)
            if dfeats is None:
                dfeats = (torch.randn(feats.shape, generator=g) * 1e-2).to(torch.bfloat16).to(dev)
            st.zero_grad()
            n0 = ops.enqueue_seq()
            M._frontend_backward(model, st, tape, dfeats)
            calls[flag] = ops.enqueue_seq() - n0
            torch.cuda.synchronize()
        finally:
            ops.DGRAD2 = before
        assert tuple(tape[f"{down[0][1]}.conv1"]["x"].shape) == (4, 12, 12, 64)
        grads = {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters() if n.startswith(model.trunk_name + ".")}
        return grads, {k: (v[0].float().cpu(), v[1]) for k, v in tape["_record_grads"].items()}

    g_on, rec_on = run(True)
    g_on2, rec_on2 = run(True)
    g_off, rec_off = run(False)
    assert calls[False] - calls[True] == 3, calls          # three launches fewer: one per downsample block
    for n in g_on:
        assert torch.equal(g_on[n], g_on2[n]), f"{n}: not reproducible"
    for bi, prefix in down:
        for n in [n for n in g_on if n.startswith(prefix + ".")]:
            cos, ratio = _cmp(g_on[n], g_off[n])
            print(f"{n:50s} cos {cos:.7f} ratio {ratio:.6f}")
            assert cos >= COS_FLOOR and abs(ratio - 1.0) <= RATIO_BAND, (n, cos, ratio)
        below = blocks[bi - 1][0]
        assert rec_on[below][1] == rec_off[below][1]
        cos, ratio = _cmp(rec_on[below][0], rec_off[below][0])
        print(f"{prefix}: gradient handed to {below:24s} cos {cos:.7f} ratio {ratio:.6f}")
        assert cos >= COS_FLOOR and abs(ratio - 1.0) <= RATIO_BAND, (prefix, cos, ratio)
        assert torch.equal(rec_on[below][0], rec_on2[below][0])
        assert not torch.equal(rec_on[below][0], rec_off[below][0]) or bi != down[0][0], "layer2.0: one rounding instead of two must show in some element"


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bn"])
def test_recorded_step_list_replays_the_merged_launch_to_the_eager_bits(dev, fused):
    from syncvsr_amd import ops

    N, H, W, planes, ci = 4, 12, 12, 128, 64

    def operands(seed):
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)
        return rn(N, 6, 6, planes), rn(N, 6, 6, planes)

    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)
    w3, w1 = rn(ci, 3, 3, planes) * 0.05, rn(ci, planes) * 0.1
    x, y = rn(N, H, W, ci), rn(N, H, W, ci)
    mean, rstd = torch.zeros(ci, device=dev), torch.ones(ci, device=dev)
    bn = (y, x, mean, rstd, torch.ones(ci, device=dev), torch.zeros(ci, device=dev), 1) if fused else None

    def run(dy, dy2):
        r = ops.conv2d_dgrad2(dy, w3, dy2, w1, (H, W), bn=bn)
        return (r[0], r[1][0][: r[1][1] * 2 * ci]) if fused else (r,)

    dy, dy2 = operands(10)
    rec = ops.StepRecorder()
    with ops.recording(rec):
        outs = run(dy, dy2)
    torch.cuda.synchronize()
    assert rec.calls() == 1
    first = [o.clone() for o in outs]
    fdy, fdy2 = operands(20)
    dy.copy_(fdy)
    dy2.copy_(fdy2)
    rec.run()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = [o.clone() for o in run(fdy, fdy2)]
    torch.cuda.synchronize()
    for i, (a, b, f) in enumerate(zip(replayed, eager, first)):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"output {i}: the replay differs from the eager launch"
        assert not torch.equal(a, f), f"output {i}: the replay did not see the refilled inputs"
