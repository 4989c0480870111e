"""GPU parity of syncvsr_amd.dctcn.DCTCNLightningModule (eval path) against the goldens recorded from the reference in fp64.

Tolerance (measured, not chosen): for each tensor, `floor` = relative error of the fp64 restatement with round_to=bfloat16 (weights and
every tensor the kernels store rounded: tests/dctcn_restatement.py) against the golden, computed on the CPU inside the test; the GPU result
must be within 2 x floor (the factor covers accumulation order only).  Both numbers are printed."""
import pytest
import torch

from dctcn_cases import DCTCN_CASES, audio_rows, dctcn_subcase, dctcn_tags, load_golden, rel_err
from dctcn_restatement import dctcn_forward

pytestmark = pytest.mark.gpu
CASES = [(n, t) for n in DCTCN_CASES for t in dctcn_tags(n)]
METRICS = ("loss_total", "loss_category", "loss_audio")


def _model(cfg, sd):
    from syncvsr_amd.dctcn import DCTCNLightningModule

    m = DCTCNLightningModule(cfg)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


@pytest.mark.parametrize("name,tag", CASES)
def test_model_matches_the_reference_within_twice_the_bf16_floor(name, tag):
    cfg, dims, sd, batch = dctcn_subcase(name, tag)
    gold = load_golden(name)
    lam = float(cfg.optim.lambda_audio)
    r16 = dctcn_forward(sd, dims, *batch, lambda_audio=lam, round_to=torch.bfloat16)
    model = _model(cfg, sd)
    out = model(*[t.to("cuda:0") for t in batch])
    torch.cuda.synchronize()
    B, C, T = r16["last_hidden_states"].shape
    rows = audio_rows(B, T)
    got = {
        "last_hidden_states": model._last["last_hidden_states"].float().cpu().view(B, T, C).transpose(1, 2),
        "logits_category": model._last["logits_category"].float().cpu(),
        "logits_audio": model._last["logits_audio"].float().cpu()[rows],
    }
    floor_of = {
        "last_hidden_states": r16["last_hidden_states"],
        "logits_category": r16["logits_category"],
        "logits_audio": r16["logits_audio"].reshape(B * T, -1)[rows],
    }
    failures = []
    for k in got:
        g = torch.as_tensor(gold[f"{tag}.{k}"])
        floor, err = rel_err(floor_of[k], g), rel_err(got[k], g)
        print(f"{name}/{tag} {k}: gpu rel err {err:.4e}, bf16 floor {floor:.4e}, ratio {err / floor:.2f}")
        if not err <= 2 * floor:
            failures.append((k, err, floor))
    for k in METRICS:
        g = float(gold[f"{tag}.{k}"])
        floor, err = abs(float(r16[k]) - g) / abs(g), abs(float(out[k]) - g) / abs(g)
        print(f"{name}/{tag} {k}: gpu {float(out[k]):.6f} golden {g:.6f} rel err {err:.4e}, bf16 floor {floor:.4e}")
        if not err <= 2 * floor:
            failures.append((k, err, floor))
    # top-1 of every clip whose golden gap clears ten times the absolute floor (the generator guarantees three quarters of them do)
    glog = torch.as_tensor(gold[f"{tag}.logits_category"])
    afloor = float((r16["logits_category"] - glog).abs().max())
    top2 = glog.topk(2, dim=-1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > 10 * afloor
    assert int(clear.sum()) * 4 >= 3 * B
    assert torch.equal(got["logits_category"].argmax(-1)[clear], glog.argmax(-1)[clear])
    for k in ("accuracy_top1", "accuracy_top5"):
        print(f"{name}/{tag} {k}: gpu {float(out[k]):.4f} golden {float(gold[f'{tag}.{k}']):.4f}")
        # labels sit at the reference's top-1 / second / far-down classes with margins of ten absolute floors (generator assertion (d))
        assert abs(float(out[k]) - float(gold[f"{tag}.{k}"])) < 1e-6, k
    assert not failures, failures


def test_tiny_intermediate_features_match_the_reference():
    name, tag = "dctcn_tiny", "nowb_t7"
    cfg, dims, sd, batch = dctcn_subcase(name, tag)
    gold = load_golden(name)
    keep16, keep = {}, {}
    dctcn_forward(sd, dims, *batch, round_to=torch.bfloat16, keep=keep16)
    model = _model(cfg, sd)
    model.features(batch[0].to("cuda:0"), None, keep=keep)
    torch.cuda.synchronize()
    for k, v in keep.items():
        g = torch.as_tensor(gold[f"{tag}.{k}"])                       # [B, C, T]
        floor, err = rel_err(keep16[k], g), rel_err(v.cpu().transpose(1, 2), g)
        print(f"{k}: gpu rel err {err:.4e}, bf16 floor {floor:.4e}")
        assert err <= 2 * floor, k


def test_a_clip_alone_and_inside_a_batch_agree_and_runs_are_bit_identical():
    from syncvsr_amd.dctcn_init import dctcn_synthetic_batch

    name, tag = "dctcn_tiny", "wb_t29"
    cfg, dims, sd, _ = dctcn_subcase(name, tag)
    videos, tokens, labels, wm, am = dctcn_synthetic_batch(cfg, 5, 29, size=40, seed=77)
    model = _model(cfg, sd)
    dev = "cuda:0"
    full = model.predict(videos.to(dev), wm.to(dev), am.to(dev)).cpu()
    again = model.predict(videos.to(dev), wm.to(dev), am.to(dev)).cpu()
    assert torch.equal(full, again)
    feats = model.features(videos.to(dev), wm.to(dev)).cpu()
    assert torch.equal(feats, model.features(videos.to(dev), wm.to(dev)).cpu())
    r64 = dctcn_forward(sd, dims, videos, tokens, labels, wm, am)
    r16 = dctcn_forward(sd, dims, videos, tokens, labels, wm, am, round_to=torch.bfloat16)
    for b in (0, 3):
        alone = model.predict(videos[b: b + 1].to(dev), wm[b: b + 1].to(dev), am[b: b + 1].to(dev)).cpu()
        ref = r64["logits_category"][b: b + 1]
        floor = rel_err(r16["logits_category"][b: b + 1], ref)
        e1, e5 = rel_err(alone, ref), rel_err(full[b: b + 1], ref)
        print(f"clip {b}: alone {e1:.4e}, in a batch of five {e5:.4e}, bf16 floor {floor:.4e}, alone vs batch {rel_err(alone, full[b: b + 1]):.4e}")
        assert e1 <= 2 * floor and e5 <= 2 * floor
        assert rel_err(alone, full[b: b + 1]) <= 2 * floor


def test_state_dict_round_trip_on_the_device():
    name, tag = "dctcn_tiny", "nowb_t7"
    cfg, dims, sd, batch = dctcn_subcase(name, tag)
    model = _model(cfg, sd)
    dev = "cuda:0"
    a = model.predict(batch[0].to(dev), None, batch[4].to(dev)).cpu()
    model.load_state_dict(dict(sd, **{"wav2vec.vector_quantizer.embedding": torch.zeros(2, 3)}))            # codec keys of a reference checkpoint
    assert torch.equal(a, model.predict(batch[0].to(dev), None, batch[4].to(dev)).cpu())
    bad = dict(sd)
    del bad["model.tcn.tcn_trunk.features.norm5.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        model.load_state_dict(bad)
    got = model.state_dict()
    assert all(torch.equal(got[k].cpu(), v) for k, v in sd.items())
    model.train()
    with pytest.raises(NotImplementedError):
        model.predict(batch[0].to(dev), None, batch[4].to(dev))
