"""Bit identity of the AdamW update across library builds: svsr_adamw_step, svsr_adamw_range, svsr_adamw_onecycle_step and
svsr_adamw_onecycle_range, driven through the C ABI alone, against tests/golden/adamw_bits.npz — recorded on the build before the two update
kernels became one body with two schedule policies.  Cases, steps, what the driver itself asserts (nothing written by a step with an inf
gradient or past total_steps, the counters, the sentinels behind the buffers) and the golden's layout: tests/golden/make_golden_adamw_bits.py,
which this file imports and which records the golden when run as a program.

Per case: the parameters, both moments and the bf16 shadow behind each of the seven counted steps, and the state's scalar words behind every
launch sequence (the skipped and the refused ones too), as raw bits.  n <= 255 compares arrays, the larger sizes one SHA-256 per tensor per
step."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_adamw_bits", os.path.join(HERE, "golden", "make_golden_adamw_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def golden():
    with np.load(G.GOLDEN) as z:
        return {k: z[k].copy() for k in z.files}


@pytest.mark.parametrize("name", list(G.CASES))
def test_update_bits_match_the_recorded_build(name, golden):
    from syncvsr_amd import _lib

    grp = G.group_of(name)
    row = list(golden[f"{grp}/cases"]).index(name)
    n = G.CASES[name][0]
    assert bytes(G.inputs(n)[2]) == bytes(golden[f"{grp}/in"]), "the seeded inputs differ from the recorded ones: nothing can be compared"
    got = G.run_case(_lib.load(), name)
    for k in (*G.TENSORS, "state"):
        want = golden[f"{grp}/{k}"][row]
        assert got[k].shape == want.shape and got[k].dtype == want.dtype, (k, got[k].shape, want.shape)
        for s in range(want.shape[0]):
            assert got[k][s].tobytes() == want[s].tobytes(), f"{name}: {k} behind record {s} differs from the recorded build"


def test_golden_covers_exactly_these_cases(golden):
    assert len(G.CASES) == 4 * 3 * 5 * 2
    assert sorted({k.split("/")[0] for k in golden}) == G.GROUPS
    for grp in G.GROUPS:
        assert sorted(k.split("/")[1] for k in golden if k.startswith(grp + "/")) == sorted(("cases", "in", "state", *G.TENSORS))
        names = G.group_cases(grp)
        assert list(golden[f"{grp}/cases"]) == names
        n, records = G.CASES[names[0]][0], 9 if grp.endswith(".oc") else 8
        assert golden[f"{grp}/state"].shape == (len(names), records, 8 if grp.endswith(".oc") else 4)
        for k in G.TENSORS:
            assert golden[f"{grp}/{k}"].shape == (len(names), 7, n if n <= G.ARRAYS_UP_TO else 32)
