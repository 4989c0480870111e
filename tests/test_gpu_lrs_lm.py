"""Language-model scorer on the GPU (-m gpu): the two kernels of csrc/lrs_lm.hip against torch, `TransformerLM` against the reference's
recorded outputs (tests/golden/lrs_lm_tiny.npz / lrs_lm_full.npz, made by tests/golden/make_golden_lrs_lm.py), the pooled cache against
prefix recomputation, and the LM-fused beam search against the reference's n-best and an fp64 re-scoring of what it returns."""
import math

import numpy as np
import pytest
import torch

from golden_cases import build_lrs_infer_case
from lm_cases import LM_RUNS, lm_case, token0_prefixes
from lm_restatement import LMRestatement

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rel_err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _table_attention_ref(pool, table, n, Lq, L, H, scale, pool_rows):
    """fp32 restatement of svsr_mha_table_fwd on the (bf16-rounded) pool: [n * Lq, H * 64]."""
    D = H * 64
    t = table[:, :L].long()
    rows = torch.where(t >= 0, t, -t - 2)
    has_row = (rows >= 0) & (rows < pool_rows)
    vis = (t >= 0) & (t < pool_rows)
    g = pool[rows.clamp(0, pool.shape[0] - 1)].float()                      # [n, L, pitch]
    q = g[:, L - Lq :, :D].view(n, Lq, H, 64).transpose(1, 2)
    k = g[:, :, D : 2 * D].view(n, L, H, 64).transpose(1, 2)
    v = g[:, :, 2 * D : 3 * D].view(n, L, H, 64).transpose(1, 2)
    causal = torch.arange(L).view(1, L) <= torch.arange(L - Lq, L).view(Lq, 1)
    m = (vis.view(n, 1, 1, L) & causal.view(1, 1, Lq, L))
    sc = (q @ k.transpose(-2, -1)) * scale
    att = torch.softmax(sc.masked_fill(~m, -1e30), dim=-1).masked_fill(~m, 0.0)
    ctx = (att @ v).transpose(1, 2).reshape(n, Lq, D)
    ctx = ctx * has_row[:, L - Lq :].unsqueeze(-1)                           # a query without a row gives zeros
    return ctx.reshape(n * Lq, D)


@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("n", [1, 5, 40])
@pytest.mark.parametrize("L", [1, 7, 64, 65, 200])
@pytest.mark.parametrize("full", [False, True])
def test_table_attention_kernel_matches_torch(dev, full, L, n, H):
    """Random pool, random permuted tables with masked keys (-1: no row; <= -2: a query that is never a key) and one entry outside the
    declared pool; Lq = 1 (beam step) and Lq = L (prefix pass).  Bound: the one tests/test_gpu_lrs_kernels.py::test_plain_mha_fwd_bwd applies
    to the context rows of svsr_mha_fwd (same arithmetic: bf16 in, fp32 softmax, bf16 out)."""
    from syncvsr_amd import ops

    Lq = L if full else 1
    D = H * 64
    g = torch.Generator().manual_seed(1000 * L + 10 * n + H + (1 if full else 0))
    pool_rows = n * L + 17
    pitch = 3 * D + 8                                                        # a pitch wider than the row
    pool = torch.randn(pool_rows + 5, pitch, generator=g).to(BF)            # 5 rows behind the declared pool: an entry naming them must be ignored
    table = torch.stack([torch.randperm(pool_rows, generator=g)[:L] for _ in range(n)]).to(torch.int32)
    kind = torch.rand(n, L, generator=g)
    table = torch.where(kind < 0.15, torch.full_like(table, -1), torch.where(kind < 0.3, -table - 2, table))
    if L >= 7:
        table[0, 2] = pool_rows + 1                                          # outside [0, pool_rows)
        table[n - 1, : L - 1] = -1                                           # a query whose only candidate key is itself ...
        table[n - 1, L - 1] = -table[n - 1, L - 1].abs() - 2                 # ... and that one is masked: zeros, not NaN
    tab_pitch = torch.full((n, L + 3), -7, dtype=torch.int32)                # a table pitch wider than L
    tab_pitch[:, :L] = table
    want = _table_attention_ref(pool, table, n, Lq, L, H, 0.125, pool_rows)
    got = ops.mha_table_fwd(pool.to(dev), tab_pitch.to(dev), n=n, Lq=Lq, L=L, H=H, scale=0.125, pool_rows=pool_rows)
    torch.cuda.synchronize()
    got = got.float().cpu()
    assert got.shape == (n * Lq, D) and bool(torch.isfinite(got).all())
    err = _rel_err(got, want)
    print(f"table attention full={full} L={L} n={n} H={H}: rel err {err:.2e}")
    if float(want.norm()) == 0.0:
        assert float(got.abs().max()) == 0.0
    else:
        assert err < 1.5e-2, err
    dead = want.abs().sum(-1) == 0                                            # rows that must be exact zeros (no row / no visible key)
    assert float(got[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0


def test_table_attention_rejects_bad_arguments(dev):
    from syncvsr_amd import _lib, ops

    pool = torch.zeros(8, 3 * 128, dtype=BF, device=dev)
    table = torch.zeros(2, 4, dtype=torch.int32, device=dev)
    for kw in (dict(Lq=5, L=4), dict(Lq=0, L=4), dict(Lq=1, L=4, H=3)):       # Lq > L; Lq < 1; pool narrower than 3 * H * 64
        with pytest.raises(_lib.SvsrError):
            ops.mha_table_fwd(pool, table, n=2, scale=0.125, **dict(dict(H=2), **kw))


@pytest.mark.parametrize("R,D", [(1, 128), (5, 512), (203, 64), (40, 2048), (7, 1096)])
def test_lm_embed_kernel_matches_torch(dev, R, D):
    from syncvsr_amd import ops

    g = torch.Generator().manual_seed(R + D)
    x = (2.0 * torch.randn(R, D + 8, generator=g) + 0.5).to(BF)
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    pe = torch.randn(50, D, generator=g)
    pos = torch.randint(0, 50, (R,), generator=g).to(torch.int32)
    want = torch.relu(torch.nn.functional.layer_norm(x[:, :D].float(), (D,), gamma, beta, 1e-5)) * math.sqrt(D) + pe[pos.long()]
    got = ops.lm_embed_fwd(x.to(dev), gamma.to(dev), beta.to(dev), pe.to(dev), pos.to(dev), D, 1e-5, math.sqrt(D))
    torch.cuda.synchronize()
    err = _rel_err(got.float().cpu(), want)
    print(f"lm embed R={R} D={D}: rel err {err:.2e}")
    assert got.shape == (R, D) and err < 4e-3, err                            # one bf16 rounding of the output: 2^-9 relative per element


@pytest.fixture(scope="module")
def tiny_lm(dev):
    from syncvsr_amd.lrs_lm import TransformerLM

    conf, V, sd, gold = lm_case("lrs_lm_tiny")
    lm = TransformerLM(V, conf)
    lm.load_state_dict(sd, strict=True)
    return lm.to(dev), conf, V, sd, gold


def test_batch_score_and_forward_match_the_reference(dev, tiny_lm):
    """Bounds: abs <= 0.1 and relative norm <= 1e-2, as test_gpu_lrs_infer.py applies to the decoder scorer for the same reason (peaked
    output layer, bf16 activations); forward(x, t): nll within 1e-2 relative."""
    lm, conf, V, sd, gold = tiny_lm
    calls = [("tok0", gold["tok0.ys"], gold["tok0.logp"])]
    calls += [(f"run1.lm{j}", gold[f"run1.lm{j}.ys"], gold[f"run1.lm{j}.logp"]) for j in range(4)]
    for name, ys, want in calls:
        ys, want = torch.from_numpy(ys).to(dev), torch.from_numpy(want).float()
        got, state = lm.batch_score(ys, [None] * ys.shape[0], None)
        got = got.cpu()
        a, r = float((got - want).abs().max()), float((got - want).norm() / want.norm())
        print(f"{name}: abs {a:.4f} rel {r:.2e}")
        assert got.shape == want.shape and state.table.shape == ys.shape and state.table.dtype == torch.int32
        assert a <= 0.1 and r <= 1e-2, (name, a, r)
    assert bool((torch.from_numpy(gold["tok0.ys"])[:, 1:-1] == 0).any())          # the token-0 prefixes really carry interior zeros
    x, t = torch.from_numpy(gold["fwd.x"]).to(dev), torch.from_numpy(gold["fwd.t"]).to(dev)
    mean, nll, count = (float(v) for v in lm(x, t))
    w_mean, w_nll, w_count = (float(v) for v in gold["fwd.out"])
    print(f"forward: nll {nll:.4f} vs {w_nll:.4f}, count {count} vs {w_count}")
    assert count == w_count and abs(nll - w_nll) <= 1e-2 * abs(w_nll) and abs(mean - w_mean) <= 1e-2 * abs(w_mean)
    # the single-hypothesis interface and the reference's calling convention (a list of per-hypothesis states) carry the same state
    ys = token0_prefixes(V).to(dev)
    full, _ = lm.batch_score(ys, None, None)
    s1, st1 = lm.score(ys[1, :6], None)
    s2, st2 = lm.score(ys[1], st1)
    assert st2.table.shape == (7,) and st2.pool is st1.pool and float((s2 - full[1]).abs().max()) <= 3e-2
    lp, st = lm.batch_score(ys[:, :6], [None] * 6, None)
    lp2, _ = lm.batch_score(ys, [lm.select_state(st, b) for b in range(6)], None)
    assert float((lp2 - full).abs().max()) <= 3e-2
    with pytest.raises(ValueError, match="row table"):
        lm.batch_score(ys, st[:3], None)


def test_cached_steps_equal_prefix_recomputation_and_never_rewrite_the_pool(dev, tiny_lm):
    """Seven steps through a permutation, a duplicated parent and a shrinking beam: cached log-probabilities equal those of scoring the whole
    prefix again to 3e-2 (the decoder-cache test's bound); every step appends exactly n rows per layer and leaves every earlier pool
    row bit for bit as it was — also across the pool growing (it is sized too small here on purpose)."""
    lm, conf, V, sd, gold = tiny_lm
    g = torch.Generator().manual_seed(11)
    enc = torch.zeros(3, 8, device=dev)
    states = lm.batch_init_state(enc, beam=2, maxlen=3)
    pool = states.pool
    cap0 = pool.capacity
    n = 5
    ys = torch.full((n, 1), V - 1, dtype=torch.int64, device=dev)
    for step in range(7):
        used = pool.used
        before = [b[:used].clone() for b in pool.bufs]
        logp, states = lm.batch_score(ys, states, None)
        torch.cuda.synchronize()
        assert states.pool is pool and pool.used == used + n, (step, pool.used, used, n)
        assert len(pool.bufs) == conf["layer"] and all(torch.equal(b[:used], old) for b, old in zip(pool.bufs, before)), step
        full, _ = lm.batch_score(ys, None, None)
        err = float((logp - full).abs().max())
        print(f"step {step}: n={n} cached vs recomputed {err:.4f}")
        assert logp.shape == (n, V) and states.table.shape == (n, step + 1) and err <= 3e-2, (step, err)
        tok = torch.where(torch.arange(n, device=dev) % 2 == 0, logp.argmax(-1), torch.randint(1, V - 1, (n,), generator=g).to(dev))
        if step == 2:
            tok[1] = 0                                                        # a token 0 inside a running prefix: masked as a key from now on
        prev = torch.randperm(n, generator=g).to(dev)
        if step == 1:
            prev[0] = prev[1]                                                 # two children of one parent
        if step == 3:
            prev = prev[:3]                                                   # the beam shrinks
        ys = torch.cat((ys[prev], tok[prev].unsqueeze(1)), dim=1)
        states = lm.select_states(states, prev, tok[prev])
        n = prev.numel()
    assert pool.capacity > cap0 and pool.grown >= 1
    assert lm.workspace_bytes(40, 100) == conf["layer"] * 40 * 101 * 3 * conf["att_unit"] * 2 + 40 * 101 * 4


def _rescore(sd64, args, odim, lm_ref, enc, yseq, ctcw, lmw, maxlen):
    """Scores of one hypothesis under the fp64 scorers (oracle decoder / CTC, restated LM), accumulated along its own path."""
    from oracle import lrs_oracle as O

    dec, ctc = O.OracleDecoderScorer(sd64, args), O.make_oracle_ctc_scorer(sd64, odim - 1)
    ctc.batch_init_state(enc)
    y = torch.tensor([yseq[:1]])
    state, tot = None, dict(decoder=0.0, ctc=0.0, lm=0.0)
    for tok in yseq[1 : 1 + maxlen]:                    # a closing <eos> forced at the length limit is not scored
        d, _ = dec.batch_score(y, [None], enc.unsqueeze(0))
        c, pend = ctc.batch_score_partial(y, None, state, enc)
        tot["decoder"] += float(d[0, tok])
        tot["ctc"] += float(c[0, tok])
        if lmw != 0:
            tot["lm"] += float(lm_ref.batch_score(y, None, None)[0][0, tok])
        state = ctc.select_states(pend, torch.tensor([0]), torch.tensor([tok]))
        y = torch.cat((y, torch.tensor([[tok]])), dim=1)
    return (1 - ctcw) * tot["decoder"] + ctcw * tot["ctc"] + lmw * tot["lm"], tot


def test_lm_fused_beam_search_finds_the_reference_hypotheses(dev, tiny_lm):
    """`get_beam_search_decoder(model, tokens, rnnlm=lm, lm_weight=...)` on the reference's encoder output: the best hypothesis equals the
    reference's where its margin exceeds 0.2 and beam >= 5 (else: at least as good); total / decoder / ctc / lm scores equal the fp64
    re-scoring along the returned path to 2e-2 |s| + 0.05; n-best sorted and framed by <sos> / <eos>; the language model changes the result."""
    from syncvsr_amd.lrs_infer import get_beam_search_decoder
    from syncvsr_amd.lrs_model import E2E

    lm, conf, V, lsd, gold = tiny_lm
    args, odim, sd, clip, _, _ = build_lrs_infer_case("lrs_infer_tiny")
    model = E2E(odim, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    lm_ref = LMRestatement(lsd, conf)
    tokens = [f"t{i}" for i in range(odim)]
    g_enc = torch.from_numpy(gold["enc_feat"])
    best = {}
    identical = 0
    for r, (beam, ctcw, lmw) in enumerate(LM_RUNS):
        bs = get_beam_search_decoder(model, tokens, rnnlm=lm, ctc_weight=ctcw, lm_weight=lmw, beam_size=beam)
        assert ("lm" in bs.full_scorers) == (lmw != 0)
        nbest = bs(g_enc.to(dev))
        gy = gold[f"run{r}.yseq"]
        want = gy[0][gy[0] >= 0].tolist()
        gscore = gold[f"run{r}.score"]
        best[r] = nbest[0].yseq.tolist()
        print(f"run{r}: hip best {best[r]} {nbest[0].score:.4f} | reference {want} {gscore[0]:.4f} (2nd {gscore[1]:.4f})")
        if gscore[0] - gscore[1] > 0.2 and beam >= 5:
            identical += 1
            assert best[r] == want, (r, best[r], want)
            assert abs(nbest[0].score - gscore[0]) <= 2e-2 * abs(gscore[0]) + 0.05
        else:
            assert nbest[0].score >= gscore[0] - 0.05 * abs(gscore[0])
        for h in nbest[:3]:
            tot, parts = _rescore(sd64, args, odim, lm_ref, g_enc.double(), h.yseq.tolist(), ctcw, lmw, g_enc.shape[0])
            d = h.asdict()
            print(f"   {d['score']:.4f} (fp64 {tot:.4f}) " + " ".join(f"{k} {d['scores'].get(k, 0.0):.4f} ({parts[k]:.4f})" for k in parts))
            assert abs(d["score"] - tot) <= 2e-2 * abs(tot) + 0.05, (r, d, tot)
            for k in ("decoder", "ctc") + (("lm",) if lmw != 0 else ()):
                assert abs(d["scores"][k] - parts[k]) <= 2e-2 * abs(parts[k]) + 0.05, (r, k, d, parts)
            assert ("lm" in d["scores"]) == (lmw != 0)
        assert all(nbest[i].score >= nbest[i + 1].score for i in range(len(nbest) - 1))
        assert all(h.yseq[0] == odim - 1 and h.yseq[-1] == odim - 1 for h in nbest)
    assert identical >= 2                                  # the fixture guarantees it: at most one run falls back to "at least as good"
    assert best[1] != best[2]                              # lm_weight 0.5 against lm_weight 0 at beam 30
    # rnnlm=None is what it was: same search, no "lm" anywhere
    plain = get_beam_search_decoder(model, tokens, ctc_weight=0.1, beam_size=30)
    assert "lm" not in plain.scorers and plain(g_enc.to(dev))[0].yseq.tolist() == best[2]


def test_full_size_lm_first_scoring_calls(dev):
    """16 layers, 2,048 / 512 / 128 units, 8 heads, 5,049 vocabulary units: the first two scoring calls of a beam-40 search against the
    reference's recorded rows, relative norm <= 1e-2 (the bound the 6-layer decoder meets at full size), and a 24-token forward."""
    from syncvsr_amd.lrs_lm import TransformerLM

    conf, V, sd, gold = lm_case("lrs_lm_full")
    lm = TransformerLM(V, conf)
    lm.load_state_dict(sd, strict=True)
    lm.to(dev)
    state = lm.batch_init_state(torch.zeros(30, 8, device=dev), beam=40)
    ys0 = torch.from_numpy(gold["lm0.ys"]).to(dev)
    got0, state = lm.batch_score(ys0, state, None)
    r0 = _rel_err(got0.cpu(), torch.from_numpy(gold["lm0.logp"]))
    ys1 = torch.from_numpy(gold["lm1.ys"]).to(dev)
    assert torch.equal(ys1[:, 0], ys0[0, 0].expand(40))
    prev = torch.zeros(40, dtype=torch.int64, device=dev)
    got1, state = lm.batch_score(ys1, lm.select_states(state, prev, ys1[:, 1]), None)          # the cached step a search takes
    r1 = _rel_err(got1[:2].cpu(), torch.from_numpy(gold["lm1.logp"]))
    again, _ = lm.batch_score(ys1, [None] * 40, None)                                            # and the prefix pass over the same rows
    r1p = _rel_err(again[:2].cpu(), torch.from_numpy(gold["lm1.logp"]))
    print(f"full-size LM: call 0 rel {r0:.3e}, call 1 cached rel {r1:.3e}, prefix pass rel {r1p:.3e}")
    assert r0 <= 1e-2 and r1 <= 1e-2 and r1p <= 1e-2, (r0, r1, r1p)
    assert state.pool.used == 41 and state.table.shape == (40, 2)
    x, t = torch.from_numpy(gold["fwd.x"]).to(dev), torch.from_numpy(gold["fwd.t"]).to(dev)
    mean, nll, count = (float(v) for v in lm(x, t))
    print(f"full-size forward: nll {nll:.4f} vs {float(gold['fwd.out'][1]):.4f}")
    assert count == float(gold["fwd.out"][2]) and abs(nll - float(gold["fwd.out"][1])) <= 1e-2 * abs(float(gold["fwd.out"][1]))
