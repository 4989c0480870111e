"""fp64 torch restatement of the reference's DC-TCN word-level model in eval mode (LRW/video/src/tcn/model.py Lipreading with
densetcn_options, tcn/models/densetcn.py, se_module.py, and lightning.py:268-312 around it), written from its state dict.

`round_to` (torch.bfloat16) rounds the matrix / convolution weights and every tensor the HIP path STORES in that format: front-end
convolution and BatchNorm outputs, the transition outputs, the gated rows a first-stage branch multiplies (bf16(x * gate): the MFMA
operand), the first-stage outputs, the downsample output, every layer output, norm5's output, the pooled row and the audio logits.  The
gates themselves stay fp32, as do BatchNorm parameters, biases and PReLU slopes.  The deviation of that mode from the fp64 mode is the
noise floor of a bf16 stack: the GPU parity tests allow twice it (accumulation order).  `no_gate` / `no_dilation` switch one mechanism
off: the golden generator uses them to prove the cases see those mechanisms."""
from __future__ import annotations

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
TCN = "model.tcn.tcn_trunk.features"


def _swish(x):
    return x * torch.sigmoid(x)


def _bn(x, W, p, dim=1):
    shape = [1] * x.dim()
    shape[dim] = -1
    return ((x - W[f"{p}.running_mean"].view(shape)) / torch.sqrt(W[f"{p}.running_var"].view(shape) + BN_EPS) * W[f"{p}.weight"].view(shape)
            + W[f"{p}.bias"].view(shape))


def _weights(sd: dict, rnd):
    """fp64 copy; weights of every contraction (ndim >= 2) rounded."""
    return {k: (rnd(v.double()) if v.dim() >= 2 else v.double()) for k, v in sd.items() if v.is_floating_point()}


def frontend(W: dict, videos: torch.Tensor, rnd) -> torch.Tensor:
    """videos [B,1,T,H,W] -> [B,T,512] (tcn/model.py:121-125,160-165; Swish ResNet18)."""
    B, _, T = videos.shape[:3]
    h = rnd(F.conv3d(rnd(videos.double()), W["model.frontend3D.0.weight"], None, stride=(1, 2, 2), padding=(2, 3, 3)))
    h = _swish(_bn(h, W, "model.frontend3D.1"))
    h = rnd(F.max_pool3d(h, (1, 3, 3), (1, 2, 2), (0, 1, 1)))
    h = h.transpose(1, 2).reshape(B * T, 64, h.size(3), h.size(4))
    for li in range(1, 5):
        for bi in range(2):
            p = f"model.trunk.layer{li}.{bi}"
            stride = 2 if (bi == 0 and li > 1) else 1
            o = rnd(F.conv2d(h, W[f"{p}.conv1.weight"], None, stride=stride, padding=1))
            o = rnd(_swish(_bn(o, W, f"{p}.bn1")))
            o = rnd(F.conv2d(o, W[f"{p}.conv2.weight"], None, stride=1, padding=1))
            if f"{p}.downsample.0.weight" in W:
                r = rnd(F.conv2d(h, W[f"{p}.downsample.0.weight"], None, stride=stride))
                r = rnd(_bn(r, W, f"{p}.downsample.1"))
            else:
                r = h
            h = rnd(_swish(_bn(o, W, f"{p}.bn2") + r))
    return rnd(h.mean((2, 3))).view(B, T, 512)


def _tconv(x, w, b, k, d):
    """x [B,C,T]: Conv1d(padding=(k-1)d, dilation=d) + symmetric Chomp1d == zero padding of (k-1)d/2 on each side of the clip."""
    return F.conv1d(x, w, b, padding=(k - 1) * d // 2, dilation=d)


def backend(W: dict, dims: dict, x: torch.Tensor, rnd, keep: dict | None = None, no_gate: bool = False, no_dilation: bool = False) -> torch.Tensor:
    """x [B,T,in_size] -> last_hidden_states [B, C, T] (densetcn.py:143-192)."""
    x = x.transpose(1, 2)                                          # [B, C, T]
    p = f"{TCN}.transition0"
    a = W[f"{p}.prelu.weight"].view(1, -1, 1)
    h = _bn(F.conv1d(x, W[f"{p}.conv.weight"]), W, f"{p}.norm")
    x = rnd(torch.where(h >= 0, h, a * h))
    if keep is not None:
        keep["transition0"] = x
    ks, ds = dims["ks"], dims["ds"]
    for bi, nl in enumerate(dims["blocks"]):
        for li in range(nl):
            p = f"{TCN}.denseblock{bi + 1}.denselayer{li + 1}"
            d = 1 if no_dilation else ds[li % len(ds)]
            outs = []
            for ki, k in enumerate(ks):
                xin = x
                if dims["se"] and not no_gate:
                    y = x.mean(2)
                    y = torch.sigmoid(_swish(y @ W[f"{p}.cbcr0_se_{ki}.fc.0.weight"].T) @ W[f"{p}.cbcr0_se_{ki}.fc.2.weight"].T)
                    y = getattr(rnd, "f32", lambda t: t)(y)                 # the gate is an fp32 tensor on the device
                    xin = rnd(x * y.unsqueeze(2))
                c = _tconv(xin, W[f"{p}.cbcr0_{ki}.net.0.weight"], W[f"{p}.cbcr0_{ki}.net.0.bias"], k, d)
                outs.append(rnd(_swish(_bn(c, W, f"{p}.cbcr0_{ki}.net.1"))))
            o0 = torch.cat(outs, 1)
            outs = []
            for ki, k in enumerate(ks):
                c = _tconv(o0, W[f"{p}.cbcr1_{ki}.net.0.weight"], W[f"{p}.cbcr1_{ki}.net.0.bias"], k, d)
                outs.append(_swish(_bn(c, W, f"{p}.cbcr1_{ki}.net.1")))
            o1 = torch.cat(outs, 1)
            res = rnd(F.conv1d(x, W[f"{p}.downsample.weight"], W[f"{p}.downsample.bias"])) if f"{p}.downsample.weight" in W else x
            x = torch.cat([x, rnd(_swish(o1 + res))], 1)
        if keep is not None:
            keep[f"denseblock{bi + 1}"] = x
        if bi != len(dims["blocks"]) - 1:
            p = f"{TCN}.transition{bi + 1}"
            x = rnd(_swish(_bn(F.conv1d(x, W[f"{p}.conv.weight"]), W, f"{p}.norm")))
    return rnd(_bn(x, W, f"{TCN}.norm5"))


def heads(W: dict, dims: dict, h: torch.Tensor, tokens: torch.Tensor, labels: torch.Tensor, attention_mask: torch.Tensor, lambda_audio: float,
          rnd) -> dict:
    """lightning.py:278-312 with lam = 0.  h [B, C, T]."""
    B, C, T = h.shape
    am = attention_mask.double()
    pooled = rnd((h * am.unsqueeze(1)).sum(2) / (am.sum(1, keepdim=True) + 1e-6))
    logits_c = pooled @ W["video_classifier.weight"].T + W["video_classifier.bias"]
    logits_a = rnd(h.transpose(1, 2) @ W["audio_projection.weight"].T + W["audio_projection.bias"])
    loss_c = F.cross_entropy(logits_c, labels)
    tok = tokens[:, : T * dims["A"]]
    loss_a = F.cross_entropy(logits_a.unflatten(2, (-1, dims["V"])).flatten(0, 2), tok.flatten())
    pred = logits_c.topk(5, dim=-1)[1] == labels.unsqueeze(1)
    return dict(logits_category=logits_c, logits_audio=logits_a, loss_category=loss_c, loss_audio=loss_a, loss_total=loss_c + loss_a * lambda_audio,
                accuracy_top1=pred[:, 0].double().mean(), accuracy_top5=pred.double().amax(1).mean())


def dctcn_forward(sd: dict, dims: dict, videos, tokens, labels, word_mask, attention_mask, lambda_audio: float = 10.0, round_to=None,
                  keep: dict | None = None, no_gate: bool = False, no_dilation: bool = False) -> dict:
    rnd = (lambda t: t) if round_to is None else (lambda t: t.to(round_to).double())
    if round_to is not None:
        rnd.f32 = lambda t: t.float().double()
    W = _weights(sd, rnd)
    x = frontend(W, videos, rnd)
    if dims["in_size"] == 513:
        x = torch.cat([x, word_mask.double().unsqueeze(2)], dim=-1)
    h = backend(W, dims, x, rnd, keep, no_gate, no_dilation)
    out = heads(W, dims, h, tokens, labels, attention_mask, lambda_audio, rnd)
    out["last_hidden_states"] = h
    return out
