"""Golden vectors for the recurrent language-model scorer (syncvsr_amd/lrs_lm.py RNNLM) and its shallow fusion.  RUNS ONLY WHERE THE
REFERENCE TREE IS PRESENT: imports the reference itself (same import stub as make_golden_lrs_lm.py, plus a stand-in for
espnet.nets.pytorch_backend.e2e_asr, which lm/default.py imports `to_device` from and the reference tree does not ship) and records what ITS
`DefaultRNNLM` (espnet/nets/pytorch_backend/lm/default.py) and ITS `BatchBeamSearch` compute, in fp64, for the seeded weights of
tests/rnnlm_cases.py.  Only numbers are stored; weights are regenerated from the seeds.

    python tests/golden/make_golden_rnnlm.py

lrs_rnnlm_tiny.npz, per case c of rnnlm_cases.RNNLM_CASES: `c.state_keys` / `c.state_shapes` (the reference's own state dict), `c.tok` / `c.prev`
(the scripted steps), `c.logp` [S, n, V], `c.h` / `c.c` [S, layers, n, U] (batch_score through the reference's list-of-dicts states), `c.fwd.x` /
`.t` / `.out` (the forward(x, t) triple).  `search.*`: the n-best of the reference's BatchBeamSearch on the lrs_infer_tiny clip with the
rnnlm_cases.SEARCH language model, `search.lm_seed` its weight seed and `search.min_gap` / `search.gap_tol` the evidence for it: the script
ASSERTS that at EVERY step of that search the gap between the last kept and the first dropped candidate exceeds rnnlm_cases.score_tol of the
last kept score; it records the leading n-best entries that are further apart than that from their successor (at least two); a seed
that fails either is skipped.  The search runs on the first rnnlm_cases.SEARCH_FRAMES encoder frames of the clip.
"""
from __future__ import annotations

import importlib.machinery
import os
import sys
import types
from argparse import Namespace

import numpy as np
import torch
import torch.nn as nn
import transformers  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from golden_cases import build_lrs_infer_case  # noqa: E402
from make_golden_lrs import import_reference  # noqa: E402
from rnnlm_cases import RNNLM_CASES, SEARCH, SEARCH_FRAMES, V, forward_pair, rnnlm_state_dict, score_tol, step_inputs  # noqa: E402
from syncvsr_amd.lrs_init import lrs_audio_dims  # noqa: E402


def stub_e2e_asr() -> None:
    m = types.ModuleType("espnet.nets.pytorch_backend.e2e_asr")
    m.__spec__ = importlib.machinery.ModuleSpec(m.__name__, None)

    def to_device(where, x):
        dev = where.device if isinstance(where, torch.Tensor) else next(where.parameters()).device
        return x.to(dev)

    m.to_device = to_device
    sys.modules[m.__name__] = m


def reference_lm(conf: dict, seed: int):
    from espnet.nets.pytorch_backend.lm.default import DefaultRNNLM

    lm = DefaultRNNLM(V, Namespace(**conf))
    lm.load_state_dict(rnnlm_state_dict(conf, seed))
    return lm.eval().double()


def run_case(name: str) -> dict:
    conf, seed = RNNLM_CASES[name]
    lm = reference_lm(conf, seed)
    res: dict[str, np.ndarray] = {}
    sd = lm.state_dict()
    res[f"{name}.state_keys"] = np.array(list(sd.keys()))
    res[f"{name}.state_shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in sd])
    if conf["tie_weights"]:
        assert sd["predictor.lo.weight"].data_ptr() == sd["predictor.embed.weight"].data_ptr()
    tok, prev = step_inputs(name)
    res[f"{name}.tok"], res[f"{name}.prev"] = tok.numpy(), prev.numpy()
    keys = ("h", "c") if conf["type"] == "lstm" else ("h",)
    lp, rec = [], {k: [] for k in keys}
    with torch.no_grad():
        states = [None] * tok.shape[1]
        ys = torch.zeros((tok.shape[1], 0), dtype=torch.int64)
        for s in range(tok.shape[0]):
            if s > 0:
                states = [states[int(p)] for p in prev[s]]
                ys = ys[prev[s]]
            ys = torch.cat((ys, tok[s].unsqueeze(1)), dim=1)
            logp, states = lm.batch_score(ys, states, None)
            lp.append(logp.numpy())
            for k in keys:
                rec[k].append(np.stack([np.stack([st[k][i].numpy() for st in states]) for i in range(conf["layer"])]))
        res[f"{name}.logp"] = np.stack(lp)
        for k in keys:
            res[f"{name}.{k}"] = np.stack(rec[k])
        x, t = forward_pair()
        res[f"{name}.fwd.x"], res[f"{name}.fwd.t"] = x.numpy(), t.numpy()
        res[f"{name}.fwd.out"] = np.array([float(v) for v in lm(x, t)])
    return res


def run_search(E2E, max_seeds: int = 400) -> dict:
    from espnet.nets.batch_beam_search import BatchBeamSearch
    from espnet.nets.scorers.length_bonus import LengthBonus

    case, beam, ctcw, lmw = SEARCH
    conf = RNNLM_CASES[case][0]
    args, odim, sd, clip, _, _ = build_lrs_infer_case("lrs_infer_tiny", load_golden=False)
    assert odim == V
    ns = Namespace(**{k: v for k, v in args.items() if k != "codec"}, codec=None)
    torch.manual_seed(0)
    model = E2E(odim, ns)
    A, G, Va = lrs_audio_dims(args)
    model.audio_classifier = nn.Linear(int(args.adim), A * G * Va)
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    model.eval().double()
    token_list = [f"t{i}" for i in range(odim)]
    with torch.no_grad():
        enc_feat, _ = model.encoder(clip.double().unsqueeze(0), None)
        enc_feat = enc_feat.squeeze(0)[:SEARCH_FRAMES].contiguous()          # a short clip: the score bound grows with |score|, the gaps do not
        for seed in range(max_seeds):
            lm = reference_lm(conf, seed)
            scorers = model.scorers()
            scorers["lm"] = lm
            scorers["length_bonus"] = LengthBonus(len(token_list))
            weights = {"decoder": 1.0 - ctcw, "ctc": ctcw, "lm": lmw, "length_bonus": 0.0}
            bs = BatchBeamSearch(beam_size=beam, vocab_size=len(token_list), weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                                 token_list=token_list, pre_beam_score_key=None if ctcw == 1.0 else "decoder")
            margins: list = []
            orig = bs.batch_beam

            def rec(weighted_scores, ids, _o=orig):
                v = weighted_scores.view(-1).topk(beam + 1)[0]
                margins.append((float(v[beam - 1] - v[beam]), score_tol(float(v[beam - 1]))))
                return _o(weighted_scores, ids)

            bs.batch_beam = rec
            nbest = bs(enc_feat)
            scores = [float(h.score) for h in nbest]
            n = 0                                                # the leading entries that no near-tie can reorder or replace
            while n < min(len(scores) - 1, beam) and scores[n] - scores[n + 1] > score_tol(scores[n]):
                n += 1
            edge_ok = all(gap > tol for gap, tol in margins)
            order_ok = n >= 2
            scores = scores[:max(n, 1)]
            worst = min(gap - tol for gap, tol in margins)
            print(f"lm seed {seed}: steps {len(margins)} worst (gap - tol) {worst:.4f} edge_ok {edge_ok} nbest {['%.3f' % s for s in scores]} order_ok {order_ok}")
            if not (edge_ok and order_ok):
                continue
            L = max(len(h.yseq) for h in nbest[:n])
            ys = np.full((n, L), -1, dtype=np.int64)
            for i, h in enumerate(nbest[:n]):
                ys[i, : len(h.yseq)] = h.yseq.numpy()
            res = {"search.lm_seed": np.int64(seed), "search.beam": np.int64(beam), "search.ctc_weight": np.float64(ctcw), "search.lm_weight": np.float64(lmw),
                   "search.yseq": ys, "search.score": np.array(scores), "search.min_gap": np.float64(min(g for g, _ in margins)),
                   "search.gap_tol": np.float64(max(t for _, t in margins)), "search.enc_feat": enc_feat.float().numpy()}
            for k in ("decoder", "ctc", "lm"):
                res[f"search.score_{k}"] = np.array([float(h.scores.get(k, 0.0)) for h in nbest[:n]])
            return res
    raise AssertionError(f"no language-model seed below {max_seeds} gives a search without a near-tie at the edge of the beam")


def main() -> None:
    stub_e2e_asr()
    E2E = import_reference()
    torch.set_num_threads(8)
    res: dict[str, np.ndarray] = {}
    for name in RNNLM_CASES:
        res.update(run_case(name))
    res.update(run_search(E2E))
    path = os.path.join(HERE, "lrs_rnnlm_tiny.npz")
    np.savez_compressed(path, **res)
    print(f"-> {path} ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
