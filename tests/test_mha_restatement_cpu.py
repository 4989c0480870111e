"""The float64 attention restatement (tests/mha_restatement.py), host side (no GPU): against a brute-force loop over (i, j) written from the
formula, against the oracle's _attend, against the fp32 references of tests/test_gpu_lrs_kernels.py, its hand-written rounded backward against
autograd, and the recorded per-row size of the kernels' bf16 roundings that sets the tolerances of tests/test_gpu_mha_edges.py."""
import math

import pytest
import torch

import mha_restatement as mr
from mha_restatement import BF, F64, attention, row_check

SELF = [(1, 1, None, False), (3, 3, (3, 1), False), (6, 6, (6, 4), False), (5, 5, None, True), (6, 6, (6, 3, 1), True)]
TINY = [s + (rel,) for s in SELF for rel in (False, True)] + [(4, 6, (6, 2), False, False), (6, 3, (3, 1), True, False), (1, 5, (5, 1), False, False)]


def _tiny_inputs(Lq, Lk, B, rel, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x = dict(q=r(B, Lq, 1, 64), k=r(B, Lk, 1, 64), v=r(B, Lk, 1, 64))
    if rel:
        x.update(pe=r(2 * Lq - 1, 1, 64), bias_u=r(1, 64) * 0.5, bias_v=r(1, 64) * 0.5)
    return x


@pytest.mark.parametrize("Lq,Lk,klen,causal,rel", TINY)
def test_scores_and_ctx_equal_a_loop_over_query_key_pairs_and_the_oracle(Lq, Lk, klen, causal, rel):
    from oracle.lrs_oracle import _attend
    B = 1 if klen is None else len(klen)
    x = _tiny_inputs(Lq, Lk, B, rel)
    out = attention(**x, klen=klen, causal=causal)
    live = mr.live_mask(B, Lq, Lk, klen, causal)
    scores = torch.zeros(B, 1, Lq, Lk, dtype=F64)
    ctx = torch.zeros(B, Lq, 1, 64, dtype=F64)
    for b in range(B):
        for i in range(Lq):
            s = []
            for j in range(Lk):
                qi = x["q"][b, i, 0]
                sc = float(qi @ x["k"][b, j, 0]) if not rel else float((qi + x["bias_u"][0]) @ x["k"][b, j, 0] + (qi + x["bias_v"][0]) @ x["pe"][Lq - 1 + j - i, 0])
                scores[b, 0, i, j] = sc / 8.0
                ok = (klen is None or j < klen[b]) and (not causal or j <= i)
                assert ok == bool(live[b, 0, i, j])
                s.append(sc / 8.0 if ok else -1e10)
            m = max(s)
            e = [math.exp(t - m) for t in s]
            for j in range(Lk):
                if live[b, 0, i, j]:
                    ctx[b, i, 0] += e[j] / sum(e) * x["v"][b, j, 0]
    qu = x["q"] + x["bias_u"] if rel else x["q"]
    qv = x["q"] + x["bias_v"] if rel else None
    got_scores = mr.scores_of(qu, qv, x["k"], x.get("pe"), 0.125)
    assert torch.allclose(got_scores, scores, rtol=0, atol=1e-12)
    assert torch.allclose(out["ctx"], ctx, rtol=0, atol=1e-12)
    ref = _attend(scores, x["v"].transpose(1, 2), live[:, 0])                       # mask [B, Lq, Lk] -> ctx [B, Lq, H * 64]
    assert torch.allclose(out["ctx"].reshape(B, Lq, 64), ref, rtol=0, atol=1e-12)
    # the row statistics
    lse = torch.logsumexp(scores.masked_fill(~live, -float("inf")), -1)
    assert torch.allclose(out["lse"], lse, rtol=0, atol=1e-12)
    assert torch.allclose(out["probs"].sum(-1), torch.ones(B, 1, Lq, dtype=F64), rtol=0, atol=1e-12)


def test_a_clip_with_no_live_key_gives_zero_rows_and_an_infinite_lse():
    x = _tiny_inputs(3, 4, 2, False)
    out = attention(**x, klen=(4, 0), dctx=torch.ones(2, 3, 1, 64, dtype=F64))
    assert torch.isinf(out["lse"][1]).all() and torch.isfinite(out["lse"][0]).all()
    for n in ("ctx", "dq", "dk", "dv"):
        assert (out[n][1] == 0).all() and (out[n][0] != 0).any(), n
        assert not torch.isnan(out[n]).any()


def _r(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(name, a, b, tol=2e-6):
    e = float((a.double() - b.double()).norm() / b.double().norm())
    assert e < tol, (name, e)


def test_reproduces_the_reference_of_test_rel_mha_fwd_bwd():
    """The fp32 reference of tests/test_gpu_lrs_kernels.py::test_rel_mha_fwd_bwd, restated here line by line at (B, H, T) = (3, 3, 50)."""
    B, H, T, lens = 3, 3, 50, [50, 33, 41]
    D = H * 64
    qkv = _r(B * T, 3 * D, seed=1).to(BF)
    pe = _r(2 * T - 1, D, seed=2).to(BF)
    u, v = _r(H, 64, seed=3, scale=0.5), _r(H, 64, seed=4, scale=0.5)
    dctx = _r(B * T, D, seed=5).to(BF)
    klen = torch.tensor(lens, dtype=torch.int32)
    qf = qkv.float().view(B, T, 3, H, 64).requires_grad_(True)
    pef = pe.float().view(2 * T - 1, H, 64).requires_grad_(True)
    uf, vf = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
    q, k, val = qf[:, :, 0], qf[:, :, 1].transpose(1, 2), qf[:, :, 2].transpose(1, 2)
    qu = (q + uf).detach().to(BF).float() + ((q + uf) - (q + uf).detach())
    qv = (q + vf).detach().to(BF).float() + ((q + vf) - (q + vf).detach())
    ac = torch.matmul(qu.transpose(1, 2), k.transpose(-2, -1))
    bd_full = torch.matmul(qv.transpose(1, 2), pef.permute(1, 2, 0))
    idx = (T - 1) + torch.arange(T).view(1, T) - torch.arange(T).view(T, 1)
    bd = bd_full.gather(-1, idx.expand(B, H, T, T))
    scores = (ac + bd) / 8.0
    mask = (torch.arange(T).view(1, T) < klen.view(B, 1)).view(B, 1, 1, T)
    attn = torch.softmax(scores.masked_fill(~mask, -1e10), -1).masked_fill(~mask, 0.0)
    ctx_ref = torch.matmul(attn, val).transpose(1, 2).reshape(B * T, D)
    ctx_ref.backward(dctx.float())
    lse_ref = torch.logsumexp(scores.masked_fill(~mask, -float("inf")), -1).detach()

    x = qkv.view(B, T, 3, H, 64)
    out = attention(x[:, :, 0], x[:, :, 1], x[:, :, 2], pe=pe.view(-1, H, 64), bias_u=u, bias_v=v, klen=lens, dctx=dctx.view(B, T, H, 64), round_bias=True)
    _close("ctx", out["ctx"].reshape(B * T, D), ctx_ref.detach())
    _close("probs", out["probs"], attn.detach())
    _close("lse", out["lse"], lse_ref)
    g = qf.grad
    for i, n in enumerate(("dq", "dk", "dv")):
        _close(n, out[n], g[:, :, i])
    _close("dpe", out["dpe"], pef.grad)
    _close("dq_ac", out["dq_ac"].sum((0, 1)), uf.grad)
    _close("dq_bd", out["dq_bd"].sum((0, 1)), vf.grad)


def test_reproduces_the_reference_of_test_plain_mha_fwd_bwd():
    """tests/test_gpu_lrs_kernels.py::test_plain_mha_fwd_bwd at (causal, Lq, Lk) = (False, 41, 150) and (True, 41, 41)."""
    for causal, Lq, Lk in ((False, 41, 150), (True, 41, 41)):
        B, H = 3, 2
        D = H * 64
        q = _r(B * Lq, D, seed=1).to(BF)
        kv = _r(B * Lk, 2 * D, seed=2).to(BF)
        dctx = _r(B * Lq, D, seed=3).to(BF)
        klen = None if causal else torch.tensor([Lk, max(1, Lk // 2), max(1, Lk - 3)], dtype=torch.int32)
        qf = q.float().view(B, Lq, H, 64).requires_grad_(True)
        kvf = kv.float().view(B, Lk, 2, H, 64).requires_grad_(True)
        scores = torch.matmul(qf.transpose(1, 2), kvf[:, :, 0].permute(0, 2, 3, 1)) / 8.0
        if causal:
            mask = torch.tril(torch.ones(Lq, Lk, dtype=torch.bool)).view(1, 1, Lq, Lk)
        else:
            mask = (torch.arange(Lk).view(1, Lk) < klen.view(B, 1)).view(B, 1, 1, Lk)
        attn = torch.softmax(scores.masked_fill(~mask, -1e10), -1).masked_fill(~mask, 0.0)
        ctx_ref = torch.matmul(attn, kvf[:, :, 1].transpose(1, 2)).transpose(1, 2).reshape(B * Lq, D)
        ctx_ref.backward(dctx.float())
        x = kv.view(B, Lk, 2, H, 64)
        out = attention(q.view(B, Lq, H, 64), x[:, :, 0], x[:, :, 1], klen=None if klen is None else klen.tolist(), causal=causal, dctx=dctx.view(B, Lq, H, 64))
        _close("ctx", out["ctx"].reshape(B * Lq, D), ctx_ref.detach())
        _close("dq", out["dq"], qf.grad)
        _close("dk", out["dk"], kvf.grad[:, :, 0])
        _close("dv", out["dv"], kvf.grad[:, :, 1])


@pytest.mark.parametrize("name", ["rel-T33", "rel-T96-short", "causal-T65-klen", "src-32x33", "src-33x64-dead"])
def test_the_hand_written_backward_equals_autograd_when_nothing_is_rounded(name, monkeypatch):
    """rounded=True with the rounding switched off is the same function: its backward (both forms of dS) is autograd's."""
    monkeypatch.setattr(mr, "_bf", lambda t: t.to(F64))
    c = mr.case(name)
    ref = mr.reference(name)
    for flash in (False, True):
        out = mr.restate(c, mr.make_inputs(c), rounded=True, flash=flash)
        assert set(out) == set(ref)
        for n, t in out.items():
            chk = row_check(n, t, ref[n])
            assert chk.worst < 1e-10 and chk.nonzero == 0, (n, flash, chk)


def test_the_cases_are_those_the_kernels_can_go_wrong_at():
    names = [c.name for c in mr.CASES]
    assert len(set(names)) == len(names)
    assert [c.Lq for c in mr.REL_CASES] == sorted(c.Lq for c in mr.REL_CASES)
    assert {c.Lq for c in mr.REL_CASES} >= {1, 31, 32, 33, 64, 65, 96, 129, 161, 192, 193, 225, 256, 257, 512, 513}
    for n in mr.GUARD_CASES + mr.DETERMINISM_CASES:
        mr.case(n)
    for c in mr.CASES:
        assert c.klen is None or (len(c.klen) == c.B and all(0 <= x <= c.Lk for x in c.klen))


@pytest.fixture(scope="module")
def rounding():
    """name of tensor -> (largest per-row error of rounded=True against rounded=False over every case and both forms of dS, where)"""
    worst = {}
    for c in mr.CASES:
        x = mr.make_inputs(c)
        ref = mr.reference(c.name)
        for flash in (False, True):
            out = mr.restate(c, x, rounded=True, flash=flash)
            for n, t in out.items():
                chk = row_check(n, t, ref[n])
                assert chk.nonzero == 0, (c.name, n, chk)
                if chk.worst > worst.get(n, (0.0,))[0]:
                    worst[n] = (chk.worst, c.name, flash, chk.where)
    return worst


@pytest.mark.parametrize("name", mr.TENSORS)
def test_the_recorded_rounding_errors_are_what_the_restatement_gives(name, rounding):
    got, recorded = rounding[name], mr.ROUNDING[name]
    print(name, got, recorded)
    assert 0.9 * recorded <= got[0] <= recorded, (name, got, recorded)
    assert mr.tolerance(name) == 4 * recorded
