"""Golden strings for `lrs_eval.ids_to_text`.  RUNS ONLY IN THE BUILD CONTAINER: imports the reference itself and records what ITS
`TextTransform.post_process` (datamodule/transforms.py:162-170, the target side of test_step) and ITS `parse_hypothesis`
(espnet/asr/asr_utils.py:822-843, the hypothesis side before lightning.py:122) write for seeded and hand-made id sequences over a toy
token list.  Only data is stored: the token list, the id rows padded with -1, and the two strings per row.

`datamodule/transforms.py` imports torchaudio, torchvision and sentencepiece at its top; what is not installed is given an empty stand-in
module (as make_golden_lrs.py does for timm): `post_process` and `_ids_to_str` touch none of them, and the `TextTransform` is made without
its constructor (which wants a SentencePiece model file) and handed the toy token list.

    python tests/golden/make_golden_lrs_eval.py
"""
from __future__ import annotations

import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/LRS/video"
SEED = 20241

# id 0 the CTC blank, the last id sos / eos, as TextTransform lays its list out; pieces with and without the word mark, a bare mark,
# an apostrophe piece, capitals (the word level lowers them) and ESPnet's <space>
TOKENS = ["<blank>", "<unk>", "▁the", "▁cat", "s", "▁", "'", "▁SAT", "<space>", "a", "b", "▁on", "▁Mat", "t", "▁it", "<eos>"]
HAND = [[], [2], [5], [5, 5, 3], [3, 5], [2, 3, 4, 7, 11, 2, 12], [9, 8, 10], [8, 9, 8], [14, 6, 4], [1, 3], [13, 13, 13], [5, 9, 5, 10, 5]]


def import_reference():
    for name in ("torchaudio", "torchvision", "sentencepiece"):
        try:
            importlib.import_module(name)
        except Exception:
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
    sys.path.insert(0, REF)
    from datamodule.transforms import TextTransform
    from espnet.asr.asr_utils import parse_hypothesis

    return TextTransform, parse_hypothesis


def main() -> None:
    TextTransform, parse_hypothesis = import_reference()
    tt = TextTransform.__new__(TextTransform)
    tt.token_list, tt.ignore_id = TOKENS, -1
    rng = np.random.default_rng(SEED)
    rows = [list(r) for r in HAND]
    while len(rows) < 40:
        rows.append(rng.integers(1, len(TOKENS) - 1, size=int(rng.integers(1, 9))).tolist())
    width = max(len(r) for r in rows)
    ids = np.full((len(rows), width), -1, np.int64)
    target, hyp = [], []
    eos = len(TOKENS) - 1
    for n, r in enumerate(rows):
        ids[n, : len(r)] = r
        target.append(tt.post_process(torch.from_numpy(ids[n])))
        hyp.append(parse_hypothesis({"yseq": [eos] + r + [eos], "score": 0.0}, TOKENS)[0])
    path = os.path.join(HERE, "lrs_eval_text.npz")
    np.savez_compressed(path, tokens=np.array(TOKENS), ids=ids, target_text=np.array(target), hyp_raw=np.array(hyp))
    print(f"{len(rows)} id rows -> {path} ({os.path.getsize(path)} bytes)")
    for r, t, h in list(zip(rows, target, hyp))[:14]:
        print(r, repr(t), repr(h))


if __name__ == "__main__":
    main()
