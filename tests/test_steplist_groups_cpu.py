"""Op groups of the native step list (csrc/steplist.hip), host bookkeeping only: nothing here issues a launch, a copy or an event, so it
runs without a GPU (replays below leave every CALL and MEMSET out, and the only COPY names a group that is not skipped)."""
import ctypes

import pytest

ERR_ARG, ERR_GROUP_OPEN, ERR_NO_GROUP, ERR_MASK_SIZE = 1001, 1003, 1004, 1005


@pytest.fixture()
def steplist():
    from syncvsr_amd import _lib, build

    if not __import__("os").path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    h = lib.svsr_steplist_create()
    yield lib, h
    assert lib.svsr_steplist_destroy(h) == 0


def _call(lib, h) -> int:
    slots = (ctypes.c_int64 * 3)(0, 1, 0)          # svsr_word_add(word, delta, stream): recorded, never issued here
    return lib.svsr_steplist_push_call(h, b"svsr_word_add", slots, 3)


def _mask(*bits):
    return (ctypes.c_uint8 * max(len(bits), 1))(*bits)


def test_error_codes_are_declared_in_the_header():
    from syncvsr_amd import _lib

    text = open(_lib.HEADER).read()
    for name, code in (("SVSR_ERR_GROUP_OPEN", ERR_GROUP_OPEN), ("SVSR_ERR_NO_GROUP", ERR_NO_GROUP), ("SVSR_ERR_MASK_SIZE", ERR_MASK_SIZE)):
        assert f"#define {name} {code}" in text


def test_group_open_close_and_counts(steplist):
    lib, h = steplist
    assert lib.svsr_steplist_groups(h) == 0 and lib.svsr_steplist_calls(h, -1) == 0
    assert _call(lib, h) == 0                                     # outside any group
    assert lib.svsr_steplist_push_group(h, 2) == 0                # groups are numbered by the caller: 0 and 1 exist (empty) from here on
    assert lib.svsr_steplist_groups(h) == 3
    assert _call(lib, h) == 0 and _call(lib, h) == 0
    assert lib.svsr_steplist_push_memset(h, ctypes.c_void_p(4096), 0, 64, None) == 0
    assert lib.svsr_steplist_push_group(h, -1) == 0
    assert lib.svsr_steplist_push_group(h, 0) == 0
    assert _call(lib, h) == 0
    assert lib.svsr_steplist_push_group(h, -1) == 0
    assert lib.svsr_steplist_push_group(h, 2) == 0                # a group may be opened again (the backward half of a block)
    assert _call(lib, h) == 0
    assert lib.svsr_steplist_push_group(h, -1) == 0
    assert [lib.svsr_steplist_calls(h, g) for g in range(3)] == [1, 0, 3]
    assert lib.svsr_steplist_calls(h, -1) == 5
    assert lib.svsr_steplist_calls(h, 3) == -ERR_NO_GROUP
    assert lib.svsr_steplist_size(h) == 6                          # five calls and the memset
    assert lib.svsr_steplist_last_issued(h) == 0


def test_group_errors(steplist):
    lib, h = steplist
    assert lib.svsr_steplist_push_group(h, -1) == ERR_NO_GROUP    # nothing to close
    assert lib.svsr_steplist_push_group(h, -2) == ERR_ARG
    assert lib.svsr_steplist_push_group(h, 0) == 0
    assert lib.svsr_steplist_push_group(h, 1) == ERR_GROUP_OPEN   # nested
    assert lib.svsr_steplist_push_group(h, 0) == ERR_GROUP_OPEN
    assert lib.svsr_steplist_push_break(h) == -ERR_GROUP_OPEN     # no segment boundary inside a group ...
    assert lib.svsr_steplist_segments(h) == 1                     # ... and the list is unchanged
    assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), 64, None, 0) == ERR_GROUP_OPEN
    assert lib.svsr_steplist_push_group(h, -1) == 0
    assert lib.svsr_steplist_groups(h) == 1
    # a copy must name a group the list has
    assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), 64, None, 1) == ERR_NO_GROUP
    assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), 64, None, -1) == ERR_NO_GROUP
    assert lib.svsr_steplist_push_copy(h, None, ctypes.c_void_p(8192), 64, None, 0) == ERR_ARG
    assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), -1, None, 0) == ERR_ARG
    assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), 64, None, 0) == 0
    assert lib.svsr_steplist_push_break(h) == 1                   # outside a group: fine
    # the mask has one byte per group
    assert lib.svsr_steplist_set_skips(h, _mask(1, 0), 2) == ERR_MASK_SIZE
    assert lib.svsr_steplist_set_skips(h, None, 0) == ERR_MASK_SIZE
    assert lib.svsr_steplist_set_skips(h, None, 1) == ERR_ARG
    assert lib.svsr_steplist_set_skips(h, _mask(1), 1) == 0


def test_skipped_groups_are_left_out_on_the_host(steplist):
    lib, h = steplist
    for g in (0, 1):
        assert lib.svsr_steplist_push_group(h, g) == 0
        assert _call(lib, h) == 0 and _call(lib, h) == 0
        assert lib.svsr_steplist_push_memset(h, ctypes.c_void_p(4096), 0, 64, None) == 0
        assert lib.svsr_steplist_push_group(h, -1) == 0
    assert lib.svsr_steplist_push_group(h, 2) == 0 and lib.svsr_steplist_push_group(h, -1) == 0
    # issued only in a replay that skips group 2
    assert lib.svsr_steplist_push_copy(h, ctypes.c_void_p(4096), ctypes.c_void_p(8192), 64, None, 2) == 0
    assert lib.svsr_steplist_push_break(h) == 1
    assert lib.svsr_steplist_push_group(h, 1) == 0 and _call(lib, h) == 0 and lib.svsr_steplist_push_group(h, -1) == 0
    assert lib.svsr_steplist_calls(h, -1) == 5 and lib.svsr_steplist_calls(h, 1) == 3
    keep = _mask(1, 1, 0)
    assert lib.svsr_steplist_set_skips(h, keep, 3) == 0
    ctypes.memset(keep, 0, 3)                                      # the list holds a copy of the mask
    failed = ctypes.c_int(-1)
    assert lib.svsr_steplist_run(h, 0, ctypes.byref(failed)) == 0 and failed.value == -1
    assert lib.svsr_steplist_run(h, 1, ctypes.byref(failed)) == 0
    assert lib.svsr_steplist_last_issued(h) == 0
    assert lib.svsr_steplist_run(h, -1, ctypes.byref(failed)) == 0
    assert lib.svsr_steplist_last_issued(h) == 0


def test_recorder_group_bookkeeping():
    """ops.StepRecorder: groups, append-only recording of the groups the recording step skips, pass-through copies, skip masks — the
    parts that touch no device (the recorder is driven here without `ops.recording`, so nothing is executed)."""
    import torch

    from syncvsr_amd import ops

    rec = ops.StepRecorder()
    rec.skips = frozenset({1})
    with rec.group(0):
        assert not rec.append_only
        rec.call("svsr_word_add", (0, 1, 0))
    with rec.group(1):
        assert rec.append_only
        rec.call("svsr_word_add", (0, 1, 0))
        rec.call("svsr_word_add", (0, 2, 0))
    assert not rec.append_only
    assert rec.groups == 2 and rec.calls() == 3 and rec.calls(0) == 1 and rec.calls(1) == 2
    with pytest.raises(_lib_error()):
        rec.calls(2)
    with pytest.raises(ValueError):
        rec.set_skips({2})
    rec.set_skips({0, 1})
    rec.set_skips(())
    with pytest.raises(ValueError):
        rec.passthrough(torch.empty(4), torch.empty(8), 0)
    with rec.group(0):
        with pytest.raises(_lib_error()):
            with rec.group(1):
                pass
    with rec.group(0):
        with pytest.raises(_lib_error()):
            rec.add_callback(lambda: None)          # a segment break inside a group
    assert rec.segments == 1 and not rec.callbacks


def _lib_error():
    from syncvsr_amd import _lib

    return _lib.SvsrError
