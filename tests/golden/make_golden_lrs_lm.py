"""Golden vectors for the language-model scorer (syncvsr_amd/lrs_lm.py) and the LM-fused beam search.  RUNS ONLY WHERE THE REFERENCE
TREE IS PRESENT: imports the reference itself (same import stub as make_golden_lrs_infer.py) and records what ITS `TransformerLM`
(espnet/nets/pytorch_backend/lm/transformer.py) and ITS `BatchBeamSearch` compute, in fp64, for the seeded weights of tests/lm_cases.py.
Only numbers are stored; weights are regenerated from the seed.

    python tests/golden/make_golden_lrs_lm.py [lrs_lm_tiny] [lrs_lm_full]

lrs_lm_tiny.npz: `lm_state_keys` / `lm_state_shapes` (the reference's own state dict), `tok0.ys` / `tok0.logp` (batch_score of hand-made
prefixes with token 0 inside), `fwd.x` / `fwd.t` / `fwd.out` (forward(x, t) triple), and per run r of lm_cases.LM_RUNS on the
lrs_infer_tiny clip: the first four LM batch_score calls (`run{r}.lm{j}.ys / .logp`) and the n-best (`yseq`, `score`, `score_decoder`,
`score_ctc`, `score_lm`).  The script ASSERTS that the case is not vacuous: (a) at beam 30 the best hypothesis with lm_weight 0.5 differs
from the one with lm_weight 0; (b) in at least two of the three runs the best hypothesis leads the runner-up by more than 0.2.
lrs_lm_full.npz: two rows of the first two scoring calls of the 16-layer, 5,049-unit LM and a 24-token forward triple.
"""
from __future__ import annotations

import os
import sys
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
from lm_cases import LM_CASES, LM_RUNS, lm_state_dict, token0_prefixes  # noqa: E402
from make_golden_lrs import import_reference  # noqa: E402
from syncvsr_amd.lrs_init import lrs_audio_dims  # noqa: E402


def reference_lm(name: str):
    from espnet.nets.pytorch_backend.lm.transformer import TransformerLM

    conf, V, _, _ = LM_CASES[name]
    lm = TransformerLM(V, Namespace(**conf, dropout_rate=0.0))
    missing, unexpected = lm.load_state_dict(lm_state_dict(name), strict=True)
    assert not missing and not unexpected
    return lm.eval().double(), V


def forward_pair(V: int, B: int, L: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(1, V - 1, (B, L + 1), generator=g)
    seq[:, 0] = V - 1
    x, t = seq[:, :-1].clone(), seq[:, 1:].clone()
    if B > 1:
        x[1, L - 3 :] = 0                    # a padded tail: those positions leave the loss and are never keys
    return x, t


def run_tiny(E2E) -> dict:
    from espnet.nets.batch_beam_search import BatchBeamSearch
    from espnet.nets.scorers.length_bonus import LengthBonus

    res: dict[str, np.ndarray] = {}
    lm, V = reference_lm("lrs_lm_tiny")
    keys = list(lm.state_dict().keys())
    res["lm_state_keys"] = np.array(keys)
    res["lm_state_shapes"] = np.array([",".join(str(d) for d in lm.state_dict()[k].shape) for k in keys])
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
    with torch.no_grad():
        ys0 = token0_prefixes(V)
        res["tok0.ys"] = ys0.numpy()
        res["tok0.logp"] = lm.batch_score(ys0, [None] * ys0.shape[0], None)[0].numpy()
        # cache on / off agree inside the reference itself (its own noise floor for the fixture)
        lp1, st = lm.batch_score(ys0[:, :-1], [None] * ys0.shape[0], None)
        lp2, _ = lm.batch_score(ys0, st, None)
        assert float((lp2 - torch.from_numpy(res["tok0.logp"])).abs().max()) < 1e-9
        x, t = forward_pair(V, 3, 9, 17)
        res["fwd.x"], res["fwd.t"] = x.numpy(), t.numpy()
        res["fwd.out"] = np.array([float(v) for v in lm(x, t)])
        enc_feat, _ = model.encoder(clip.double().unsqueeze(0), None)
        enc_feat = enc_feat.squeeze(0)
        token_list = [f"t{i}" for i in range(odim)]
        best, margins = {}, []
        for r, (beam, ctcw, lmw) in enumerate(LM_RUNS):
            scorers = model.scorers()
            scorers["lm"] = lm
            scorers["length_bonus"] = LengthBonus(len(token_list))
            weights = {"decoder": 1.0 - ctcw, "ctc": ctcw, "lm": lmw, "length_bonus": 0.0}
            bs = BatchBeamSearch(beam_size=beam, vocab_size=len(token_list), weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                                 token_list=token_list, pre_beam_score_key=None if ctcw == 1.0 else "decoder")
            calls: list = []
            orig = lm.batch_score

            def rec(ys, states, xs, _o=orig):
                out = _o(ys, states, xs)
                if len(calls) < 4:
                    calls.append((ys.clone(), out[0].clone()))
                return out

            lm.batch_score = rec
            nbest = bs(enc_feat)
            del lm.batch_score
            n = min(len(nbest), 10)
            L = max(len(h.yseq) for h in nbest[:n])
            ys = np.full((n, L), -1, dtype=np.int64)
            for i, h in enumerate(nbest[:n]):
                ys[i, : len(h.yseq)] = h.yseq.numpy()
            res[f"run{r}.beam"], res[f"run{r}.ctc_weight"], res[f"run{r}.lm_weight"] = np.int64(beam), np.float64(ctcw), np.float64(lmw)
            res[f"run{r}.n_ended"] = np.int64(len(nbest))
            res[f"run{r}.yseq"] = ys
            res[f"run{r}.score"] = np.array([float(h.score) for h in nbest[:n]])
            for k in ("decoder", "ctc", "lm"):
                res[f"run{r}.score_{k}"] = np.array([float(h.scores.get(k, 0.0)) for h in nbest[:n]])
            for j, (ys_in, logp) in enumerate(calls):
                res[f"run{r}.lm{j}.ys"], res[f"run{r}.lm{j}.logp"] = ys_in.numpy(), logp.numpy()
            best[r] = nbest[0].yseq.tolist()
            margins.append(float(nbest[0].score) - float(nbest[1].score))
            print(f"run{r} beam={beam} ctc={ctcw} lm={lmw}: ended={len(nbest)} best={best[r]} score={float(nbest[0].score):.4f} margin={margins[-1]:.4f}")
        assert best[1] != best[2], "the language model does not change the best hypothesis at beam 30: pick another seed / gain in tests/lm_cases.py"
        assert sum(m > 0.2 for m in margins) >= 2, f"margins {margins}: fewer than two runs exceed 0.2, pick another seed / gain in tests/lm_cases.py"
    res["enc_feat"] = enc_feat.float().numpy()
    return res


def run_full() -> dict:
    res: dict[str, np.ndarray] = {}
    lm, V = reference_lm("lrs_lm_full")
    g = torch.Generator().manual_seed(23)
    with torch.no_grad():
        ys = torch.full((1, 1), V - 1, dtype=torch.int64)
        lp, _ = lm.batch_score(ys, [None], None)
        res["lm0.ys"], res["lm0.logp"] = ys.numpy(), lp.numpy()
        top = lp[0].topk(40).indices                      # what a beam-40 search scores next: <sos> + each of the 40 best units
        ys = torch.cat((torch.full((40, 1), V - 1, dtype=torch.int64), top.unsqueeze(1)), dim=1)
        lp, _ = lm.batch_score(ys, [None] * 40, None)
        res["lm1.ys"], res["lm1.logp"] = ys.numpy(), lp[:2].numpy()                    # two rows only: keeps the file small
        x, t = forward_pair(V, 1, 24, 29)
        res["fwd.x"], res["fwd.t"] = x.numpy(), t.numpy()
        res["fwd.out"] = np.array([float(v) for v in lm(x, t)])
    del g
    return res


def main() -> None:
    E2E = import_reference()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(LM_CASES)):
        res = run_tiny(E2E) if name == "lrs_lm_tiny" else run_full()
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **res)
        print(f"-> {path} ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
