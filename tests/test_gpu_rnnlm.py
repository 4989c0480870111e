"""Recurrent language-model scorer on the GPU (-m gpu): svsr_rnn_cell_step against the float64 restatement (tests/rnnlm_restatement.py) fed the
bf16-rounded weights and inputs, `RNNLM` against the reference's recorded outputs (tests/golden/lrs_rnnlm_tiny.npz, made by
tests/golden/make_golden_rnnlm.py), and the LM-fused beam search against the reference's n-best."""
import numpy as np
import pytest
import torch

from golden_cases import build_lrs_infer_case
from rnnlm_cases import LOGP_ABS, LOGP_REL, RNNLM_CASES, SEARCH, V, load_golden, rnnlm_state_dict, score_tol, search_lm
from rnnlm_restatement import RNNLMRestatement, bf16_round, cell_step

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# One launch against the restatement with the SAME bf16 operands: what is left is (a) fp32 accumulation of K <= 384 products, each |w x| <= 0.25 * 4:
# at most K * 2^-24 * sum|w x| <= 384 * 6e-8 * 384 = 9e-3 in the worst case of all roundings aligned, ~sqrt(K) * 6e-8 * sqrt(K) * 0.3 = 7e-6 for
# the random data used here; (b) v_exp_f32 / v_rcp_f32 (1 ulp each) in sigmoid and tanh = 1 - 2 / (1 + exp(2x)): 3e-7 absolute.  Bound: 2e-5.
CELL_ATOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return load_golden()


def _pad64(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("gru", [False, True])
@pytest.mark.parametrize("R", [1, 3, 65])
@pytest.mark.parametrize("U", [64, 96, 192])
def test_cell_kernel_matches_the_restatement(dev, U, R, gru, layer):
    """U 64 (no padding), 96 (a padded tail), 192 (more unit tiles, three k-steps more); E != U in layer 0 (the embedding gather: tokens read through
    a strided column), layer 1 reads the bf16 rows of the layer below; R 1, 3 and 65 (past one 16-row tile, past 64 rows: two tiles per wave);
    src: a permutation with a duplicated parent, rows of -1 and one index outside the previous rows (zero state)."""
    from syncvsr_amd import ops
    from syncvsr_amd.lrs_lm import pack_rnn_cell

    G = 3 if gru else 4
    E = (96 if U == 64 else 64) if layer == 0 else U
    Ep, Up = _pad64(E), _pad64(U)
    g = torch.Generator().manual_seed(1000 * U + 10 * R + 2 * gru + layer)
    w_ih, w_hh = (torch.rand(G * U, E, generator=g) * 2 - 1) * 0.25, (torch.rand(G * U, U, generator=g) * 2 - 1) * 0.25
    b_ih, b_hh = (torch.rand(G * U, generator=g) * 2 - 1) * 0.2, (torch.rand(G * U, generator=g) * 2 - 1) * 0.2
    P = R + 2                                                                  # rows of the previous step
    h_prev, c_prev = torch.zeros(P, Up), torch.zeros(P, Up)
    h_prev[:, :U], c_prev[:, :U] = torch.rand(P, U, generator=g) * 2 - 1, torch.randn(P, U, generator=g)
    src = torch.randperm(P, generator=g)[:R]
    if R >= 3:
        src[1], src[2] = src[0], -1                                            # a duplicated parent, a first-step row
    if R >= 65:
        src[64], src[40] = -1, P + 3                                           # ... in the second tile of a wave, and an index outside the rows
    if layer == 0:
        rows = 50
        x = torch.zeros(rows, Ep + 8)                                          # a pitch wider than the row
        x[:, :E] = torch.randn(rows, E, generator=g)
        ys = torch.randint(0, rows, (R, 3), generator=g)
        xidx, x_rows = ys[:, -1], x[:, :E][ys[:, -1]]
    else:
        x = torch.zeros(R, Up)
        x[:, :E] = torch.rand(R, E, generator=g) * 2 - 1
        ys, xidx, x_rows = None, None, x[:, :E]
    x16 = x.to(BF)
    live = (src >= 0) & (src < P)
    hp = torch.where(live.unsqueeze(1), h_prev[src.clamp(0, P - 1), :U], torch.zeros(R, U))
    cp = torch.where(live.unsqueeze(1), c_prev[src.clamp(0, P - 1), :U], torch.zeros(R, U))
    want_h, want_c = cell_step("gru" if gru else "lstm", bf16_round(w_ih.numpy()), bf16_round(w_hh.numpy()), b_ih.double().numpy(), b_hh.double().numpy(),
                               x_rows.to(BF).double().numpy(), hp.double().numpy(), None if gru else cp.double().numpy(), bf16_inputs=True)
    wpk, bias = pack_rnn_cell(w_ih, w_hh, b_ih, b_hh, gru)
    h_out = torch.full((R + 1, Up), 7.0, device=dev)                           # a row behind the R written ones: must stay as it is
    c_out = None if gru else torch.full((R + 1, Up), 7.0, device=dev)
    h16 = torch.full((R + 1, Up), 7.0, dtype=BF, device=dev)
    ys_d = None if ys is None else ys.to(dev)
    ops.rnn_cell_step(gru, wpk.to(dev), bias.to(dev), x16.to(dev), None if ys_d is None else ys_d[:, -1], h_prev.to(dev), None if gru else c_prev.to(dev),
                      src.to(dev), h_out, c_out, h16, R=R, Ep=Ep, Up=Up, U=U)
    torch.cuda.synchronize()
    got_h = h_out.cpu()
    err_h = float(np.abs(got_h[:R, :U].double().numpy() - want_h).max())
    print(f"cell U={U} R={R} gru={gru} layer={layer}: h err {err_h:.2e}")
    assert bool(torch.isfinite(got_h).all()) and err_h <= CELL_ATOL, err_h
    assert float(got_h[:R, U:].abs().max() if Up > U else 0.0) == 0.0 and bool((got_h[R] == 7.0).all())
    assert torch.equal(h16.cpu()[:R], got_h[:R].to(BF)) and bool((h16.cpu()[R] == 7.0).all())
    if not gru:
        got_c = c_out.cpu()
        err_c = float(np.abs(got_c[:R, :U].double().numpy() - want_c).max())
        print(f"   c err {err_c:.2e}")
        assert err_c <= CELL_ATOL * max(1.0, float(np.abs(want_c).max())), err_c
        assert float(got_c[:R, U:].abs().max() if Up > U else 0.0) == 0.0 and bool((got_c[R] == 7.0).all())


def test_cell_kernel_rejects_bad_arguments(dev):
    from syncvsr_amd import _lib, ops
    from syncvsr_amd.lrs_lm import pack_rnn_cell

    wpk, bias = pack_rnn_cell(torch.zeros(256, 64), torch.zeros(256, 64), torch.zeros(256), torch.zeros(256), False)
    wpk, bias = wpk.to(dev), bias.to(dev)
    x = torch.zeros(4, 64, dtype=BF, device=dev)
    h = torch.zeros(2, 4, 64, device=dev)
    with pytest.raises(_lib.SvsrError):                                        # reading and writing the same side of the pair
        ops.rnn_cell_step(False, wpk, bias, x, None, h[0], h[1], torch.zeros(4, dtype=torch.int64, device=dev), h[0], h[1], None, R=4, Ep=64, Up=64, U=64)
    with pytest.raises(_lib.SvsrError):                                        # more real units than padded ones
        ops.rnn_cell_step(False, wpk, bias, x, None, None, None, None, h[0], h[1], None, R=4, Ep=64, Up=64, U=65)


def _lm(case, dev, seed=None):
    from syncvsr_amd.lrs_lm import RNNLM

    conf, s = RNNLM_CASES[case]
    sd = rnnlm_state_dict(conf, s if seed is None else seed)
    lm = RNNLM(V, conf)
    lm.load_state_dict(sd, strict=True)
    return lm.to(dev), conf, sd


def _run_steps(lm, tok, prev, dev):
    """The scripted steps through the search's own calls: batch_init_state -> batch_score -> select_states -> ..."""
    S, n = tok.shape
    state = lm.batch_init_state(torch.zeros(3, 8, device=dev), beam=n)
    bufs = state.bufs
    ys = torch.zeros((n, 0), dtype=torch.int64, device=dev)
    lp, hs, cs = [], [], []
    for s in range(S):
        if s > 0:
            p = torch.from_numpy(prev[s]).to(dev)
            state, ys = lm.select_states(state, p, None), ys[p]
        ys = torch.cat((ys, torch.from_numpy(tok[s]).to(dev).unsqueeze(1)), dim=1)
        logp, state = lm.batch_score_clips(ys, state, None)
        assert state.bufs is bufs                                              # the search's path allocates nothing
        lp.append(logp.clone())
        hs.append(bufs.h[state.parity][:, :n].clone())
        cs.append(bufs.c[state.parity][:, :n].clone() if lm.lstm else None)
    return torch.stack(lp), torch.stack(hs), torch.stack(cs) if lm.lstm else None


@pytest.mark.parametrize("case", list(RNNLM_CASES))
def test_module_matches_the_reference(dev, gold, case):
    """Log-probabilities: the bounds of the transformer-LM scorer's tests (abs 0.1, relative norm 1e-2).  States: twice the error of the float64
    restatement with bf16-rounded weights and contraction inputs against the recorded fp32-weight reference over the same steps (measured here,
    on the host; profiles/rnnlm.json records it) — fp32 accumulation order is the only other source.  forward(x, t): 1e-2 relative."""
    from syncvsr_amd import ops

    lm, conf, sd = _lm(case, dev)
    tok, prev = gold[f"{case}.tok"], gold[f"{case}.prev"]
    r_lp, r_h, r_c = RNNLMRestatement(sd, conf, bf16_weights=True, bf16_inputs=True).run(tok, prev)
    floor_h = float(np.abs(r_h - gold[f"{case}.h"]).max())
    floor_c = float(np.abs(r_c - gold[f"{case}.c"]).max()) if lm.lstm else 0.0
    n0 = ops._ENQUEUED
    lp, h, c = _run_steps(lm, tok, prev, dev)
    launches = (ops._ENQUEUED - n0) / tok.shape[0]
    torch.cuda.synchronize()
    U = conf["unit"]
    want = torch.from_numpy(gold[f"{case}.logp"]).float()
    a, r = float((lp.cpu() - want).abs().max()), float((lp.cpu() - want).norm() / want.norm())
    err_h = float((h.cpu()[..., :U].double() - torch.from_numpy(gold[f"{case}.h"])).abs().max())
    print(f"{case}: logp abs {a:.4f} rel {r:.2e} | h err {err_h:.2e} (bf16 floor {floor_h:.2e}) | launches per step {launches}")
    assert a <= LOGP_ABS and r <= LOGP_REL, (a, r)
    assert err_h <= 2 * floor_h, (err_h, floor_h)
    if lm.lstm:
        err_c = float((c.cpu()[..., :U].double() - torch.from_numpy(gold[f"{case}.c"])).abs().max())
        print(f"   c err {err_c:.2e} (bf16 floor {floor_c:.2e})")
        assert err_c <= 2 * floor_c, (err_c, floor_c)
        assert float(c[..., U:].abs().max()) == 0.0
    assert float(h[..., U:].abs().max()) == 0.0                                # the padded units never leave zero
    assert launches == conf["layer"] + 1                                       # one cell launch per layer + the output projection
    x, t = torch.from_numpy(gold[f"{case}.fwd.x"]).to(dev), torch.from_numpy(gold[f"{case}.fwd.t"]).to(dev)
    mean, nll, count = (float(v) for v in lm(x, t))
    w_mean, w_nll, w_count = (float(v) for v in gold[f"{case}.fwd.out"])
    print(f"   forward: nll {nll:.4f} vs {w_nll:.4f}, count {count} vs {w_count}")
    assert count == w_count and abs(nll - w_nll) <= 1e-2 * abs(w_nll) and abs(mean - w_mean) <= 1e-2 * abs(w_mean)
    # two identical runs: bit for bit
    lp2, h2, c2 = _run_steps(lm, tok, prev, dev)
    assert torch.equal(lp, lp2) and torch.equal(h, h2) and (c is None or torch.equal(c, c2))


@pytest.mark.parametrize("case", ["lstm2", "gru1"])
def test_padded_units_stay_zero_over_chained_steps(dev, case):
    """Eight chained steps with duplicated parents: columns unit .. unit_pad - 1 of h (and c) are exact zeros on both sides of the pair."""
    lm, conf, sd = _lm(case, dev)
    n, U = 7, conf["unit"]
    g = torch.Generator().manual_seed(5)
    state = lm.batch_init_state(torch.zeros(3, 8, device=dev), beam=n)
    ys = torch.full((n, 1), V - 1, dtype=torch.int64, device=dev)
    for step in range(8):
        logp, state = lm.batch_score(ys, state, None)
        side = state.bufs.h[state.parity][:, :n]
        assert float(side[..., U:].abs().max()) == 0.0 and float(side[..., :U].abs().max()) > 0.0, step
        if lm.lstm:
            assert float(state.bufs.c[state.parity][:, :n][..., U:].abs().max()) == 0.0, step
        prev = torch.randint(0, n, (n,), generator=g).to(dev)
        state = lm.select_states(state, prev, None)
        ys = torch.cat((ys[prev], torch.randint(1, V - 1, (n, 1), generator=g).to(dev)), dim=1)
    assert bool(torch.isfinite(logp).all())


def test_single_hypothesis_interface_and_detached_states(dev, gold):
    """`score` is `batch_score` with n = 1, bit for bit; the reference's calling convention (a list of per-hypothesis states from select_state)
    carries the same state; a state older than two scoring calls of its search is refused, a detached one is not."""
    lm, conf, sd = _lm("lstm2", dev)
    tok = torch.from_numpy(gold["lstm2.tok"]).to(dev)
    y1 = tok[0, :1]
    s1, st1 = lm.score(y1, None)
    b1, bst1 = lm.batch_score(y1.unsqueeze(0), [None], None)
    assert torch.equal(s1, b1[0])
    y2 = torch.cat((y1, tok[1, :1]))
    s2, st2 = lm.score(y2, st1)
    b2, bst2 = lm.batch_score(y2.unsqueeze(0), bst1, None)
    assert torch.equal(s2, b2[0]) and st2.rows.dim() == 0
    # five hypotheses: batched state vs a list of detached per-hypothesis states
    ys = tok[:1].t().contiguous()
    lp, st = lm.batch_score(ys, None, None)
    ys2 = torch.cat((ys, tok[1].unsqueeze(1)), dim=1)
    each = [lm.select_state(st, b) for b in range(ys.shape[0])]
    want, st_b = lm.batch_score(ys2, st, None)
    got, _ = lm.batch_score(ys2, each, None)
    assert torch.equal(got, want)
    lm.batch_score(ys2, st_b, None)                                            # two more scoring calls on the search's buffers ...
    with pytest.raises(ValueError, match="overwritten"):
        lm.batch_score(ys2, st, None)                                          # ... and the old batched state is gone
    again, _ = lm.batch_score(ys2, each, None)                                 # the detached ones are not
    assert torch.equal(again, want)
    with pytest.raises(ValueError, match="rows for"):
        lm.batch_score(ys2[:3], st_b, None)


@pytest.fixture(scope="module")
def fused(dev, gold):
    from syncvsr_amd.lrs_infer import get_beam_search_decoder
    from syncvsr_amd.lrs_lm import RNNLM
    from syncvsr_amd.lrs_model import E2E

    conf, lsd = search_lm(gold)
    lm = RNNLM(V, conf)
    lm.load_state_dict(lsd, strict=True)
    lm.to(dev)
    args, odim, sd, clip, _, _ = build_lrs_infer_case("lrs_infer_tiny", load_golden=False)
    model = E2E(odim, args)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    tokens = [f"t{i}" for i in range(odim)]
    _, beam, ctcw, lmw = SEARCH
    assert (beam, ctcw, lmw) == (int(gold["search.beam"]), float(gold["search.ctc_weight"]), float(gold["search.lm_weight"]))
    enc = torch.from_numpy(gold["search.enc_feat"]).to(dev)
    make = lambda **kw: get_beam_search_decoder(model, tokens, ctc_weight=ctcw, beam_size=beam, **kw)      # noqa: E731
    return lm, make, enc, lmw


def _check_nbest(nbest, gold):
    gy, gs = gold["search.yseq"], gold["search.score"]
    assert float(gold["search.min_gap"]) > 0 and len(gs) >= 2
    for i in range(len(gs)):
        want = gy[i][gy[i] >= 0].tolist()
        print(f"   {i}: hip {nbest[i].yseq.tolist()} {nbest[i].score:.4f} | reference {want} {gs[i]:.4f}")
        assert nbest[i].yseq.tolist() == want, (i, nbest[i].yseq.tolist(), want)
        assert abs(nbest[i].score - gs[i]) <= score_tol(gs[i]), (i, nbest[i].score, gs[i])
        assert abs(nbest[i].scores["lm"] - float(gold["search.score_lm"][i])) <= score_tol(float(gold["search.score_lm"][i]))


def test_shallow_fusion_finds_the_reference_nbest(dev, gold, fused):
    """forward_clips on the recorded clip, on that clip twice in one batch, and the single-clip search: token sequences equal the reference's
    leading n-best (the generator asserted that no step of that search has a near-tie at the edge of the beam), scores within score_tol."""
    lm, make, enc, lmw = fused
    bs = make(rnnlm=lm, lm_weight=lmw)
    assert bs.full_scorers["lm"] is lm and lm.beam_hint == SEARCH[1]
    one = bs.forward_clips(enc.unsqueeze(0), [enc.shape[0]])
    assert len(one) == 1
    _check_nbest(one[0], gold)
    two = bs.forward_clips(torch.stack((enc, enc)), [enc.shape[0]] * 2)
    assert len(two) == 2
    for nb in two:
        _check_nbest(nb, gold)
        assert [h.yseq.tolist() for h in nb] == [h.yseq.tolist() for h in one[0]] and [h.score for h in nb] == [h.score for h in one[0]]
    single = bs(enc)
    assert [h.yseq.tolist() for h in single] == [h.yseq.tolist() for h in one[0]] and [h.score for h in single] == [h.score for h in one[0]]


def test_lm_weight_zero_is_the_search_without_a_language_model(dev, fused):
    lm, make, enc, _ = fused
    with_lm, plain = make(rnnlm=lm, lm_weight=0.0), make()
    assert "lm" not in with_lm.scorers
    a, b = with_lm.forward_clips(enc.unsqueeze(0), [enc.shape[0]])[0], plain.forward_clips(enc.unsqueeze(0), [enc.shape[0]])[0]
    assert len(a) == len(b) and all(torch.equal(x.yseq, y.yseq) and x.score == y.score and x.scores == y.scores for x, y in zip(a, b))
