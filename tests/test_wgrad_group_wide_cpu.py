"""The symbols of the 128-wide grouped weight-gradient launch: declared in include/syncvsr_hip.h, exported and bound; the forced-tile
planner's host-side contract (no GPU needed: svsr_wgrad_rows_plan_tile only computes)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svsr_wgrad_rows_plan_tile",)


def test_new_symbols_are_declared_and_exported():
    from syncvsr_amd import _lib

    decl = _lib.parse_header()
    for n in NEW_SYMBOLS:
        assert n in decl, f"{n} is not declared in include/syncvsr_hip.h"
    # svsr_wgrad_rows_plan's arguments plus the tile edge, in front of the outputs
    base = [a for _, a in decl["svsr_wgrad_rows_plan"]]
    assert [a for _, a in decl["svsr_wgrad_rows_plan_tile"]] == base[:7] + ["bc"] + base[7:]
    src = open(os.path.join(ROOT, "syncvsr_amd", "csrc", "igemm_wgrad.hip")).read()
    assert "launch_wgrad_group<128, 2>" in src and "launch_wgrad_group<64, 3>" in src
    body = src[src.index("void k_igemm_wgrad_group("): src.index("// UNIT-LIST launch")]
    assert "atomic" not in body.lower(), "one writer per element, no atomics"
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), f"{n} is not exported"
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == len(decl[n])
    assert lib.svsr_steplist_knows(b"svsr_igemm_wgrad_group_v2")          # the entry the 128-wide plans are launched through


def _plan(lib, name, *args):
    meta, nfl = (ctypes.c_int * 8)(), ctypes.c_int64(-1)
    n = getattr(lib, name)(*args, None, 0, meta, ctypes.byref(nfl))
    assert n > 0, (name, args, n)
    words = (ctypes.c_int * n)()
    assert getattr(lib, name)(*args, words, n, meta, ctypes.byref(nfl)) == n
    return list(words), [int(v) for v in meta], int(nfl.value)


def test_forced_tile_plan_is_the_ordinary_plan_without_a_split():
    from syncvsr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    # (Nimg, P, src0, dst0, Ci, Co, bias): the benchmark's four encoder linears (960 rows), a K tail, a sequence slice
    for case in ((960, 1, 0, 0, 512, 1536, 1), (960, 1, 0, 0, 512, 512, 1), (960, 1, 0, 0, 512, 2048, 1), (960, 1, 0, 0, 2048, 512, 1),
                 (70, 1, 0, 0, 128, 128, 1), (4, 29, 1, 0, 128, 128, 1), (130, 1, 0, 0, 192, 136, 0)):
        words0, meta0, _ = _plan(lib, "svsr_wgrad_rows_plan", *case)
        Nimg, P, _, _, Ci, Co, _ = case
        chunks = P * ((Nimg + 63) // 64) if Nimg >= 64 else (Nimg * P + 63) // 64
        for bc in (64, 128):
            words, meta, nfl = _plan(lib, "svsr_wgrad_rows_plan_tile", *case[:7], bc)
            tasks = -(-Co // bc) * -(-Ci // bc)
            assert meta == [bc, 2 if bc == 128 else 3, 1, chunks, tasks, 1, P, 0], (case, bc, meta)
            assert nfl == 0
            if meta0[7] == 0:          # (a plain plan: the same words — rows, row enumeration flag)
                assert words == words0, (case, bc)
    # svsr_wgrad_rows_plan itself keeps choosing as before: 64-wide without a split for the wide 960-row linears, a K split for 512 x 512
    assert _plan(lib, "svsr_wgrad_rows_plan", 960, 1, 0, 0, 512, 2048, 1)[1][:3] == [64, 3, 1]
    m = _plan(lib, "svsr_wgrad_rows_plan", 960, 1, 0, 0, 512, 512, 1)[1]
    assert m[0] == 64 and m[2] > 1
    for bad in (0, 32, 96, 256):
        assert lib.svsr_wgrad_rows_plan_tile(64, 1, 0, 0, 128, 128, 1, bad, None, 0, None, None) == -1001
