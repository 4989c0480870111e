"""Thin host-side wrappers over the C ABI (include/syncvsr_hip.h): tensors in, launches out.

PyTorch is used here only as the owner of device memory and streams; every computation is a call into
libsyncvsr_hip.so on the current HIP stream.  Tensors are NHWC bf16 activations unless stated.
"""
from __future__ import annotations

import bisect
import ctypes
import os
import struct
from contextlib import contextmanager, nullcontext
from collections import namedtuple
from typing import Callable, Optional, Sequence

import torch

from . import _lib

BF16 = torch.bfloat16
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
HALO_WGRAD = True      # nine-taps-per-pass weight gradient for stride-1 3x3 convs (False: generic per-tap kernel)


_DEV_INDEX: Optional[int] = None
STREAM_OVERRIDE: Optional[int] = None      # raw hipStream_t that launches go to instead of torch's current stream (model._SideStream)


def _stream() -> int:
    """Raw hipStream_t of torch's current stream.  `torch.cuda.current_stream().cuda_stream` builds a Stream object per call
    (~9 us, a fifth of the host time of an eager step); the raw getter is ~0.3 us.  One device per process."""
    global _DEV_INDEX
    if STREAM_OVERRIDE is not None:
        return STREAM_OVERRIDE
    if _DEV_INDEX is None:
        _DEV_INDEX = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(_DEV_INDEX)


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _drop(drop) -> tuple:
    """drop = None | (seed tensor [1] int32/uint32 on the device, site id, p) -> the three C arguments."""
    if drop is None or drop[2] <= 0.0:
        return None, 0, 0.0
    return drop[0].data_ptr(), int(drop[1]), float(drop[2])


# Per-stream fp32 scratch for the partial rows / split-K slabs of the reproducible reductions (include/syncvsr_hip.h): every
# producer and its fixed-order finaliser are enqueued back to back on one stream, so one buffer per stream serves them all.
# Outgrown buffers are kept alive: a captured HIP graph may still hold their address.
_SCRATCH: dict[int, torch.Tensor] = {}
_SCRATCH_KEEP: list[torch.Tensor] = []


def scratch(nfloats: int) -> torch.Tensor:
    key = _stream()
    t = _SCRATCH.get(key)
    if t is None or t.numel() < nfloats:
        if t is not None:
            _SCRATCH_KEEP.append(t)
        t = _SCRATCH[key] = torch.empty(max(int(nfloats), 1 << 22), dtype=torch.float32, device="cuda")
    return t


class _BoundedCache(dict):
    """Per-shape launch plans and shape queries.  Variable-length batches (LRS without the length buckets) meet a new shape almost every
    step: beyond PLAN_CACHE_MAX entries the cache starts over, so host and device memory stay bounded (a plan costs ~50 us to rebuild)."""

    def __setitem__(self, key, value):
        if len(self) >= PLAN_CACHE_MAX and not PLAN_CACHE_PINNED:
            self.retire()
        super().__setitem__(key, value)

    def retire(self) -> None:
        """Starts over.  The evicted plans stay alive for one more generation (or for ever once a graph / step list holds their
        device words): a weight-gradient launch on the side stream may still be reading them, and the caching allocator would hand
        their memory to the next allocation on the main stream."""
        global _PLAN_RETIRED
        old = list(self.values())
        _PLAN_RETIRED = (_PLAN_RETIRED + old) if PLAN_CACHE_PINNED else old
        self.clear()


PLAN_CACHE_MAX = 20000
PLAN_CACHE_PINNED = False       # set once a HIP graph has captured launches: their plans' device words must stay alive
_PLAN_RETIRED: list = []
_PLAN_CACHE: _BoundedCache = _BoundedCache()


def _query(name: str, *args) -> tuple:
    """Cached host-side shape query (svsr_*_plan / svsr_*_rows): returns the int outputs (or the returned row count)."""
    key = (name, args)
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return hit
    fn = getattr(_lib.load(), name)
    if name.endswith(("_rows", "_bytes", "_floats")):
        out = (int(fn(*args)),)
    else:
        nout = {"svsr_conv3x3_wgrad_plan": (1, 1),
                "svsr_stem_conv_wgrad_plan": (1, 1)}[name]
        ints = [ctypes.c_int(0) for _ in range(nout[0])]
        longs = [ctypes.c_int64(0) for _ in range(nout[1])]
        rc = fn(*args, *[ctypes.byref(v) for v in ints], *[ctypes.byref(v) for v in longs])
        if rc != 0:
            _lib.check(rc, name)
        out = tuple(int(v.value) for v in ints) + tuple(int(v.value) for v in longs)
    _PLAN_CACHE[key] = out
    return out


REDUCTION_KNOBS = ("reduce_cus", "wg_blocks", "wg_units", "wg_unit_max", "wg_unit_min", "wg_short_k", "w3_blocks", "w3_waves", "w3_dense")


def tune_value(key: str) -> int:
    """Current value of a library tuning knob (svsr_tune_value)."""
    out = ctypes.c_int(0)
    _lib.check(_lib.load().svsr_tune_value(key.encode(), ctypes.byref(out)), f"svsr_tune_value({key})")
    return int(out.value)


def reduction_plan_params() -> list[int]:
    """The knobs that decide the ORDER in which partial sums of a weight gradient / a BatchNorm statistic are added (REDUCTION_KNOBS): with the
    same values — whatever the device's compute-unit count — two runs produce the same bits.  Stored in TrainStep.state_dict()."""
    return [tune_value(k) for k in REDUCTION_KNOBS]


def tune(key: str, value: int) -> None:
    """Result-preserving tuning knob of the library (svsr_tune); invalidates cached plans.  `bn_bwd_fused` is a host-side choice
    (which launches the trunk backward issues), kept in this module."""
    if key == "bn_bwd_fused":
        global BN_BWD_FUSED
        BN_BWD_FUSED = bool(value)
        return
    if key == "colsum_multi":
        global COLSUM_MULTI
        COLSUM_MULTI = bool(value)
        return
    rc = _lib.load().svsr_tune(key.encode(), int(value))
    if rc != 0:
        _lib.check(rc, f"svsr_tune({key})")
    _PLAN_CACHE.retire()          # plans are rebuilt with the new knob; the old ones stay alive for whoever still points at them


_INT_ARRAYS: dict = {}


def _ints(v: Sequence[int]):
    """ctypes int array for a tap list; cached (the same few tap tables recur every step and building one costs ~1 us)."""
    key = tuple(v)
    arr = _INT_ARRAYS.get(key)
    if arr is None:
        arr = _INT_ARRAYS[key] = (ctypes.c_int * len(key))(*key)
    return arr


# Optional per-launch timing with HIP events (bench.py's roofline leg): {kernel label: [(start, end, flops, bytes)]}.
_TIMING: Optional[dict[str, list]] = None


def start_event_timing() -> None:
    global _TIMING
    _TIMING = {}


def stop_event_timing() -> dict[str, dict[str, float]]:
    """-> {label: {launches, ms (sum), flops (sum), bytes (sum)}}; synchronises the device."""
    global _TIMING
    rec, _TIMING = _TIMING or {}, None
    torch.cuda.synchronize()
    out = {}
    for label, evs in rec.items():
        out[label] = dict(launches=len(evs), ms=sum(s.elapsed_time(e) for s, e, _, _ in evs),
                          flops=float(sum(f for _, _, f, _ in evs)), bytes=float(sum(b for _, _, _, b in evs)))
    return out


# --------------------------------------------------------------------------------------------------
# native step enqueuer (csrc/steplist.hip): every launch of one training step is recorded once and re-issued by ONE library
# call per step (engine.TrainStep(native=True))
# --------------------------------------------------------------------------------------------------
class StepRecorder:
    """While active (`with ops.recording(rec)`), every library launch, cross-stream wait and memset issued through this module is
    executed AND appended to a native step list; `host_callback` ends a segment, so that host-side work (a collective) can sit
    between two segments of the replay.  The recorder keeps everything the list points to alive: the tensors allocated during the
    recorded step (their storage is re-used by every replay, exactly as a captured HIP graph would) and the host-side arrays."""

    def __init__(self) -> None:
        self.lib = _lib.load()
        self.handle = self.lib.svsr_steplist_create()
        self.keep: list = []
        self.callbacks: dict[int, list[Callable[[], None]]] = {}      # segment index -> host calls that follow it
        self.main_stream: Optional[int] = None
        self.closed = False
        # layer drop (model._xt_encoder_forward / _backward): with layer_groups set, the encoder emits every block inside op group n
        # (`encoder.layers.{n}`) followed by a pass-through copy, and each replay leaves out the groups set_skips() names.  `skips`: the
        # groups the RECORDING step itself skips — recorded append-only (below), their pass-through copies executed.
        self.layer_groups = False
        self.skips: frozenset = frozenset()
        self.append_only = False
        self.cur_group: Optional[int] = None      # the op group being recorded (group()), None outside every group
        # gradient accumulation (engine.TrainStep(accumulate=N > 1)): (zero group, tail group) — the zero-fill of the gradient buffer and the
        # optimiser tail as op groups numbered behind the layer-drop groups (ops.window_group); None: the list holds neither (N = 1)
        self.window: Optional[tuple] = None

    def __del__(self):
        try:
            if self.handle:
                self.lib.svsr_steplist_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def call(self, name: str, args: tuple) -> None:
        fn = getattr(self.lib, name)
        n = len(args)
        slots = (ctypes.c_int64 * n)()
        for i, (a, t) in enumerate(zip(args, fn.argtypes)):
            if t is ctypes.c_float:
                slots[i] = struct.unpack("<q", struct.pack("<d", float(a)))[0]
            elif t is ctypes.c_void_p:
                if a is None:
                    slots[i] = 0
                elif isinstance(a, int):
                    slots[i] = a
                else:                       # a ctypes array (plan meta record, tap table): host memory the launch reads
                    slots[i] = ctypes.addressof(a)
                    self.keep.append(a)
            else:
                slots[i] = int(a)
        rc = self.lib.svsr_steplist_push_call(self.handle, name.encode(), slots, n)
        if rc != 0:
            raise _lib.SvsrError(f"{name} cannot be recorded into a step list (code {rc}): not a stream launch of include/syncvsr_hip.h?")

    def wait(self, waiter: int, signaller: int) -> None:
        _lib.check(self.lib.svsr_steplist_push_wait(self.handle, waiter, signaller), "svsr_steplist_push_wait")

    def memset(self, ptr: int, value: int, nbytes: int, stream: int) -> None:
        _lib.check(self.lib.svsr_steplist_push_memset(self.handle, ptr, value, nbytes, stream), "svsr_steplist_push_memset")

    @contextmanager
    def group(self, n: int):
        """Every launch and memset inside the block belongs to op group n.  When the recording step skips n (n in `skips`) they are
        appended WITHOUT being executed: the list must hold every block for later replays, while this step produces the bits of an
        eager step that skips n.  (Recording the whole list without executing and then running it once with the mask was the other way:
        it would also defer what executes on the host inside the step — the collectives of host_callback, allocations sized by results —
        while append-only touches nothing outside the skipped groups.)  Tensors allocated inside are kept alive like any other
        (torch.empty is wrapped for the whole recording): a later replay may execute the group.  Cross-stream waits are executed and
        recorded as always: the list issues them whatever is skipped."""
        _lib.check(self.lib.svsr_steplist_push_group(self.handle, int(n)), f"svsr_steplist_push_group({n})")
        self.append_only = n in self.skips
        self.cur_group = int(n)
        try:
            yield
        finally:
            self.append_only = False
            self.cur_group = None
            _lib.check(self.lib.svsr_steplist_push_group(self.handle, -1), "svsr_steplist_push_group(-1)")

    def passthrough(self, dst: torch.Tensor, src: torch.Tensor, group: int) -> None:
        """dst <- src (whole contiguous tensors, same size) on the current stream in every replay that skips `group` — and now, when the
        recording step skips it."""
        if dst.numel() * dst.element_size() != src.numel() * src.element_size() or not (dst.is_contiguous() and src.is_contiguous()):
            raise ValueError("passthrough copies whole contiguous tensors of one size")
        nbytes, stream = src.numel() * src.element_size(), _stream()
        if group in self.skips:
            _lib.check(self.lib.svsr_memcpy_async(dst.data_ptr(), src.data_ptr(), nbytes, stream), "svsr_memcpy_async")
        _lib.check(self.lib.svsr_steplist_push_copy(self.handle, dst.data_ptr(), src.data_ptr(), nbytes, stream, int(group)),
                   "svsr_steplist_push_copy")

    @property
    def groups(self) -> int:
        return int(self.lib.svsr_steplist_groups(self.handle))

    def calls(self, group: int = -1) -> int:
        """CALL ops of op group `group` (-1: of the whole list)."""
        n = int(self.lib.svsr_steplist_calls(self.handle, int(group)))
        if n < 0:
            _lib.check(-n, f"svsr_steplist_calls({group})")
        return n

    def set_skips(self, skips) -> None:
        """The op groups every following run() leaves out (an iterable of group indices)."""
        n = self.groups
        mask = (ctypes.c_uint8 * max(n, 1))()
        for g in skips:
            if not 0 <= g < n:
                raise ValueError(f"op group {g} is not in this step list ({n} groups)")
            mask[g] = 1
        _lib.check(self.lib.svsr_steplist_set_skips(self.handle, mask, n), "svsr_steplist_set_skips")

    def window_skips(self, zero: bool, tail: bool) -> set:
        """The window groups a micro-step leaves out: the zero-fill unless `zero`, the optimiser tail unless `tail`."""
        if self.window is None:
            return set()
        return {g for g, run in zip(self.window, (zero, tail)) if not run}

    def would_issue(self, segment: int = -1) -> dict:
        """What run() would issue for `segment` (-1: the whole list) under the current skip mask: {calls, waits, memsets, copies}.  Issues
        nothing and needs no device."""
        counts = (ctypes.c_int64 * 4)()
        _lib.check(self.lib.svsr_steplist_dry_run(self.handle, int(segment), counts), "svsr_steplist_dry_run")
        return dict(zip(("calls", "waits", "memsets", "copies"), (int(c) for c in counts)))

    @property
    def last_issued(self) -> int:
        """Launches (CALL ops) the last run() issued."""
        return int(self.lib.svsr_steplist_last_issued(self.handle))

    def add_callback(self, fn: Callable[[], None]) -> None:
        seg = self.lib.svsr_steplist_push_break(self.handle)
        if seg < 1:
            _lib.check(-seg if seg < 0 else 1001, "svsr_steplist_push_break")
        self.callbacks.setdefault(seg - 1, []).append(fn)

    @property
    def segments(self) -> int:
        return int(self.lib.svsr_steplist_segments(self.handle))

    @property
    def size(self) -> int:
        return int(self.lib.svsr_steplist_size(self.handle))

    def kept_bytes(self) -> int:
        """Device bytes this recorder keeps alive: the unique storages of the tensors allocated during the recorded step (a grow-only
        workspace first allocated inside the recording is counted here too, although it outlives the recorder)."""
        seen: dict[int, int] = {}
        for t in self.keep:
            if torch.is_tensor(t) and t.is_cuda:
                s = t.untyped_storage()
                seen[s.data_ptr()] = s.nbytes()
        return sum(seen.values())

    def run(self) -> None:
        """Re-issues the recorded step: segment by segment, each followed by its host callbacks."""
        global _ENQUEUED
        failed = ctypes.c_int(-1)
        run, h, cbs = self.lib.svsr_steplist_run, self.handle, self.callbacks
        if len(cbs) == 0:
            rc = run(h, -1, ctypes.byref(failed))
            _ENQUEUED += 1
            if rc != 0:
                _lib.check(rc, f"svsr_steplist_run (op {failed.value})")
            return
        for k in range(self.segments):
            rc = run(h, k, ctypes.byref(failed))
            _ENQUEUED += 1
            if rc != 0:
                _lib.check(rc, f"svsr_steplist_run (op {failed.value})")
            for fn in cbs.get(k, ()):
                fn()


_REC: Optional[StepRecorder] = None
_ALLOC_KEEP = ("empty", "empty_like")
_ALLOC_FORBID = ("zeros", "zeros_like", "ones", "ones_like", "full", "full_like")      # would launch a torch kernel the list does not hold


@contextmanager
def recording(rec: StepRecorder):
    """Everything launched through this module inside the block is also appended to `rec`.  torch.empty / torch.empty_like results
    are kept alive by the recorder (the replay re-uses their storage); torch.zeros & co. raise — use ops.zeros, whose fill is
    recorded.  Launch plans are pinned (their device words are referenced by the list)."""
    global _REC, PLAN_CACHE_PINNED
    if _REC is not None or _TIMING is not None:
        raise RuntimeError("nested recording / recording while per-launch event timing is on")
    saved = {n: getattr(torch, n) for n in _ALLOC_KEEP + _ALLOC_FORBID}

    def keeper(fn):
        def w(*a, **k):
            t = fn(*a, **k)
            rec.keep.append(t)
            return t
        return w

    def forbid(name):
        def w(*a, **k):
            raise RuntimeError(f"torch.{name} inside a recorded step launches a kernel the native step list does not hold (use ops.zeros)")
        return w

    for n in _ALLOC_KEEP:
        setattr(torch, n, keeper(saved[n]))
    for n in _ALLOC_FORBID:
        setattr(torch, n, forbid(n))
    _REC = rec
    rec.main_stream = _stream()
    PLAN_CACHE_PINNED = True
    try:
        yield rec
    finally:
        _REC = None
        for n, f in saved.items():
            setattr(torch, n, f)
        rec.closed = True


def active_recorder() -> Optional[StepRecorder]:
    """The recorder of the `ops.recording` block this runs in, else None."""
    return _REC


def layer_groups() -> Optional[StepRecorder]:
    """The active recorder when it asks for replayable layer drop (StepRecorder.layer_groups), else None."""
    return _REC if _REC is not None and _REC.layer_groups else None


def window_group(which: str):
    """Context: inside a recording for gradient accumulation (StepRecorder.window), the launches and memsets of the block join the
    window's "zero" or "tail" op group — appended without being executed when the recording micro-step leaves that group out.  Anywhere
    else (eager steps, accumulate = 1) it does nothing."""
    rec = _REC
    if rec is None or rec.window is None:
        return nullcontext()
    return rec.group(rec.window[("zero", "tail").index(which)])


def host_callback(fn: Callable[[], None]) -> None:
    """Runs fn() now; inside a recorded step it also closes the current segment and is called again after that segment in
    every replay (collectives and their stream joins: engine.GradReducer)."""
    fn()
    if _REC is not None:
        _REC.add_callback(fn)


def stream_wait(waiter: torch.cuda.Stream, signaller: torch.cuda.Stream) -> None:
    """`waiter` waits for everything enqueued so far on `signaller`.  Eager: torch's own event path; recorded steps: the library's."""
    if _REC is None:
        waiter.wait_stream(signaller)
        return
    w, s = waiter.cuda_stream, signaller.cuda_stream
    _lib.check(_lib.load().svsr_stream_wait(w, s), "svsr_stream_wait")
    _REC.wait(w, s)


def device_cus() -> int:
    """Compute units of the current device."""
    return int(_lib.load().svsr_device_cus())


def shader_clock_mhz(blocks: int = 256, iters: int = 20000) -> float:
    """Effective shader clock (MHz) over a ~1 ms block of MFMA work on every compute unit, right now, on the current stream: the ratio of
    s_memtime (shader cycles) to s_memrealtime (100 MHz) inside svsr_clock_probe.  Synchronises the stream."""
    out = torch.zeros(blocks * 2 + 1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().svsr_clock_probe(_p(out), blocks, iters, _stream()), "svsr_clock_probe")
    torch.cuda.current_stream().synchronize()
    h = out[: blocks * 2].view(blocks, 2).sum(0).tolist()
    return 100.0 * h[0] / max(1, h[1])


def memset(t: torch.Tensor, value: int = 0) -> None:
    """hipMemsetAsync over a contiguous tensor on the current stream."""
    nbytes, stream = t.numel() * t.element_size(), _stream()
    if _REC is not None and _REC.append_only:          # (a group the recording step skips: appended, not executed)
        _REC.memset(t.data_ptr(), value, nbytes, stream)
        return
    _lib.check(_lib.load().svsr_memset_async(t.data_ptr(), value, nbytes, stream), "svsr_memset_async")
    if _REC is not None:
        _REC.memset(t.data_ptr(), value, nbytes, stream)


# --------------------------------------------------------------------------------------------------
# first touch stores: which ranges of the flat gradient buffer need no zero-fill
# --------------------------------------------------------------------------------------------------
GRAD_STORE = True          # False: whole-buffer zero-fill, every writer adds (the behaviour before first-touch stores)
GRAD_FILL_NAN = False      # tests only (a step list or HIP graph recorded while it is set carries the whole-buffer NaN fill in every replay: never reuse one): the whole buffer is filled with NaNs ahead of the step's zero-fill — a range that is planned as stored but read would show


class GradCoverage:
    """Per-step bookkeeping of the flat fp32 gradient buffer `grad` for engine.TrainStep.  `spans` = [lo, hi) element ranges (whole tensors,
    16-byte aligned starts, no overlap) whose FIRST writer of a step is a weight-gradient launch with a store mode (igemm_wgrad, conv2d_wgrad,
    linear_wgrad_group): that launch stores 0.f + sum instead of adding to zeros, later writers of the range in the same step add.  Everything
    else — `holes`: 1-D tensors, pads, tensors whose writers only add — is zero-filled by ONE svsr_fill_ranges launch per step (fill()).
    begin() arms the map for a step; the wrappers ask touch(); end() returns the planned spans no launch stored (must be empty: their
    gradient would be last step's).  A launch is matched to a span by its exact [lo, hi), or to a run of adjacent spans it tiles exactly: one that only overlaps a planned span (a
    layer's weight written in pieces, query / key / value as three launches) would add onto memory nobody zeroed, so touch() raises before
    that launch is issued.  Beyond that, TrainStep's check of end() — after the step's kernels are enqueued, before the optimiser's; in
    native mode at record time only, which is enough because a replay repeats the recorded launches — is the only protection."""

    def __init__(self, grad: torch.Tensor, spans):
        self.grad, self.base, self.numel = grad, grad.data_ptr(), grad.numel()
        self.spans, self.holes = self.plan(spans, self.numel)
        self._planned = set(self.spans)
        self._los = [lo for lo, _ in self.spans]
        self._ranges = (ctypes.c_int64 * (2 * max(1, len(self.holes))))(*[v for h in self.holes for v in h])
        self._touched: set = set()

    @staticmethod
    def plan(spans, numel: int) -> tuple:
        """-> (sorted spans, holes): holes = the complement of the spans in [0, numel), each hole's start rounded DOWN to a multiple of 4
        (the fill runs before the step's first store: up to three elements at the end of a span are zeroed first, then stored)."""
        spans = sorted({(int(lo), int(hi)) for lo, hi in spans})
        holes, at = [], 0
        for lo, hi in spans:
            if lo % 4 or lo < at or hi <= lo or hi > numel:
                raise ValueError(f"gradient span [{lo}, {hi}) is misaligned, empty, overlaps its neighbour or leaves the buffer")
            if lo > at:
                holes.append((at // 4 * 4, lo))
            at = hi
        if numel % 4:
            raise ValueError("the flat gradient buffer is a multiple of 4 elements")
        if at < numel:
            holes.append((at // 4 * 4, numel))
        return spans, holes

    def hole_elems(self) -> int:
        return sum(hi - lo for lo, hi in self.holes)

    def fill(self) -> None:
        """The step's zero-fill on the current stream: the holes only."""
        if GRAD_FILL_NAN:
            _call("svsr_fill_f32", self.base, self.numel, float("nan"), _stream())
        if self.holes:
            _call("svsr_fill_ranges", self.base, self.numel, self._ranges, len(self.holes), 0, _stream())

    def begin(self) -> None:
        global _COVER
        self._touched = set()
        _COVER = self

    def touch(self, ptr: int, n: int) -> int:
        """1 (add) or 0 (store: the first writer of a planned span this step) for a launch that writes n floats at `ptr`."""
        lo = (ptr - self.base) // 4
        key = (lo, lo + n)
        if key not in self._planned:
            # one launch over several adjacent tensors (query | key | value, key | value of a source attention): it must tile whole planned
            # spans exactly, and they share one fate — all stored now, or all written before (add)
            i = bisect.bisect_left(self._los, lo)
            run, at = [], lo
            while i + len(run) < len(self.spans) and self.spans[i + len(run)][0] == at and self.spans[i + len(run)][1] <= lo + n:
                at = self.spans[i + len(run)][1]
                run.append(self.spans[i + len(run)])
            if len(run) > 1 and at == lo + n:
                done = [s in self._touched for s in run]
                if all(done):
                    return 1
                if any(done):
                    raise RuntimeError(f"a weight-gradient launch writes elements [{lo}, {lo + n}) of the gradient buffer: some of the first-touch spans "
                                       f"it covers were written earlier in this step, others not — it can neither add nor store")
                self._touched.update(run)
                return 0
            i = bisect.bisect_right(self._los, lo)       # spans are disjoint: only spans[i - 1] and spans[i] can overlap [lo, lo + n)
            for s in self.spans[max(0, i - 1) : i + 1]:
                if s[0] < lo + n and lo < s[1]:
                    raise RuntimeError(f"a weight-gradient launch writes elements [{lo}, {lo + n}) of the gradient buffer, part of the first-touch span "
                                       f"[{s[0]}, {s[1]}) but not all of it: the span is not zero-filled, so the launch can neither add nor store")
            return 1
        if key in self._touched:
            return 1
        self._touched.add(key)
        return 0

    def end(self) -> list:
        global _COVER
        if _COVER is self:
            _COVER = None
        return sorted(self._planned - self._touched)


_COVER: Optional[GradCoverage] = None


def _grad_add(dw: torch.Tensor, n: int) -> int:
    """SVSR_GRAD_ADD_DW bit of a weight-gradient launch writing n floats at dw: 1 unless an armed GradCoverage says this is the first
    writer of a planned span (outside a TrainStep nothing is armed: every launch adds, as `dw += ...` always meant)."""
    return 1 if _COVER is None else _COVER.touch(dw.data_ptr(), n)


def end_grad_coverage() -> list:
    return [] if _COVER is None else _COVER.end()


def zeros(shape, dtype, device) -> torch.Tensor:
    t = torch.empty(shape, dtype=dtype, device=device)
    memset(t, 0)
    return t


def word_add(word: torch.Tensor, delta: int) -> None:
    _call("svsr_word_add", _p(word), int(delta), _stream())


def lincomb2(a: torch.Tensor, b: torch.Tensor, wb: float) -> torch.Tensor:
    """0-d fp32: a + wb * b, on the device."""
    out = torch.empty((), dtype=torch.float32, device=a.device)
    _call("svsr_lincomb2", _p(a), _p(b), float(wb), _p(out), _stream())
    return out


def lincomb3_ratio(a, wa: float, b, wb: float, c, wc: float, num=None, den=None):
    """0-d fp32 (wa*a + wb*b) + wc*c and, with num / den, their quotient: on the device, torch's roundings."""
    out0 = torch.empty((), dtype=torch.float32, device=a.device)
    out1 = torch.empty((), dtype=torch.float32, device=a.device) if num is not None else None
    _call("svsr_lincomb3_ratio", _p(a), float(wa), _p(b), float(wb), _p(c), float(wc), _p(out0), _p(num), _p(den), _p(out1), _stream())
    return out0, out1


_ENQUEUED = 0      # counts what has been handed to the device: library calls and replayed step-list segments (enqueue_seq)


def enqueue_seq() -> int:
    """A number that grows with every library call and every replayed step-list segment: two equal readings mean that nothing was enqueued
    in between (engine.GradReducer: a second cross-stream fence behind the same producers is left out)."""
    return _ENQUEUED


def _call(name: str, *args, label: Optional[str] = None, flops: float = 0.0, nbytes: float = 0.0) -> None:
    global _ENQUEUED
    _ENQUEUED += 1
    if _REC is not None and _REC.append_only:          # (a group the recording step skips: appended, not executed)
        _REC.call(name, args)
        return
    timing = _TIMING
    if timing is not None:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    rc = getattr(_lib.load(), name)(*args)
    if timing is not None:
        e.record()
        timing.setdefault(label or name, []).append((s, e, flops, nbytes))
    if rc != 0:
        _lib.check(rc, name)
    if _REC is not None:
        _REC.call(name, args)


class Plan:
    """Launch plan of svsr_igemm_fwd for one shape: device copy of the plan words + the host meta record."""
    __slots__ = ("words", "meta", "bm", "bn", "ns", "tiles", "label")

    def __init__(self, builder: str, *args):
        fn = getattr(_lib.load(), builder)
        meta = (ctypes.c_int * 8)()
        n = fn(*args, None, 0, meta)
        if n <= 0:
            _lib.check(-n if n < 0 else 1001, builder)
        host = torch.empty(n, dtype=torch.int32)
        n2 = fn(*args, host.data_ptr(), n, meta)
        if n2 != n:
            _lib.check(1001, builder)
        self.words = host.to("cuda")
        self.meta = meta
        self.bm, self.bn, self.ns, self.tiles = int(meta[0]), int(meta[1]), int(meta[2]), int(meta[3])
        self.label = f"k_igemm_p8<{self.bm},{self.bn},{self.ns}>" if self.bm == 256 else f"k_igemm_fwd_glds<{self.bm},{self.bn},{self.ns}>"


def conv_plan(mode: int, N: int, H: int, W: int, Co_out: int, k: int, stride: int, pad: int) -> Plan:
    """mode 0: forward convolution of N images [H, W]; mode 1: its input-gradient (svsr_conv_plan)."""
    key = ("conv", mode, N, H, W, Co_out, k, stride, pad)
    pl = _PLAN_CACHE.get(key)
    if pl is None:
        pl = _PLAN_CACHE[key] = Plan("svsr_conv_plan", mode, N, H, W, Co_out, k, stride, pad)
    return pl


def rows_plan(Nimg: int, P: int, src0: int, dst0: int, Co_out: int) -> Plan:
    """Plan of a dense layer over rows grouped in Nimg sequences (svsr_rows_plan)."""
    key = ("rows", Nimg, P, src0, dst0, Co_out)
    pl = _PLAN_CACHE.get(key)
    if pl is None:
        pl = _PLAN_CACHE[key] = Plan("svsr_rows_plan", Nimg, P, src0, dst0, Co_out)
    return pl


class WPlan:
    """Launch plan of svsr_igemm_wgrad for one shape (device words + host meta + workspace size)."""
    __slots__ = ("words", "meta", "bc", "splits", "part_floats", "label")

    def __init__(self, builder: str, *args):
        fn = getattr(_lib.load(), builder)
        meta = (ctypes.c_int * 8)()
        nfl = ctypes.c_int64(0)
        n = fn(*args, None, 0, meta, ctypes.byref(nfl))
        if n <= 0:
            _lib.check(-n if n < 0 else 1001, builder)
        host = torch.empty(n, dtype=torch.int32)
        if fn(*args, host.data_ptr(), n, meta, ctypes.byref(nfl)) != n:
            _lib.check(1001, builder)
        self.words = host.to("cuda")
        self.meta = meta
        self.bc, self.splits, self.part_floats = int(meta[0]), int(meta[2]), int(nfl.value)
        self.label = f"k_igemm_wgrad<{self.bc},{int(meta[1])}>"


def wgrad_conv_plan(N: int, H: int, W: int, Ci: int, Co: int, k: int, stride: int, pad: int) -> WPlan:
    key = ("wconv", N, H, W, Ci, Co, k, stride, pad)
    pl = _PLAN_CACHE.get(key)
    if pl is None:
        pl = _PLAN_CACHE[key] = WPlan("svsr_wgrad_plan", N, H, W, Ci, Co, k, stride, pad)
    return pl


def wgrad_rows_plan(Nimg: int, P: int, src0: int, dst0: int, Ci: int, Co: int, has_bias: bool) -> WPlan:
    key = ("wrows", Nimg, P, src0, dst0, Ci, Co, bool(has_bias))
    pl = _PLAN_CACHE.get(key)
    if pl is None:
        pl = _PLAN_CACHE[key] = WPlan("svsr_wgrad_rows_plan", Nimg, P, src0, dst0, Ci, Co, int(has_bias))
    return pl


def wgrad_rows_plan_tile(Nimg: int, P: int, src0: int, dst0: int, Ci: int, Co: int, has_bias: bool, bc: int) -> WPlan:
    """The same rows on bc-wide tiles (64 / 128) without K split (svsr_wgrad_rows_plan_tile): a problem of a grouped launch."""
    key = ("wrows_tile", Nimg, P, src0, dst0, Ci, Co, bool(has_bias), bc)
    pl = _PLAN_CACHE.get(key)
    if pl is None:
        pl = _PLAN_CACHE[key] = WPlan("svsr_wgrad_rows_plan_tile", Nimg, P, src0, dst0, Ci, Co, int(has_bias), bc)
    return pl


# --------------------------------------------------------------------------------------------------
# implicit GEMM
# --------------------------------------------------------------------------------------------------
def igemm_fwd(plan: Plan, inp: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, *, Nimg: int, in_pix: int, Ci: int, in_pitch: int,
              Co: int, out_pix: int, out_pitch: int, wt_taps: int = 1, bias: Optional[torch.Tensor] = None,
              addend: Optional[torch.Tensor] = None, want_stats: bool = False, gelu: bool = False,
              out_pre: Optional[torch.Tensor] = None, out_f32: bool = False, relu: bool = False, alpha: float = 1.0, drop=None,
              flops: float = 0.0):
    """Runs a plan.  -> None, or with want_stats the BatchNorm partials (buffer, rows) for bn_finalize."""
    stats = st = None
    if want_stats:
        stats = scratch(plan.tiles * 2 * Co)
        st = (stats, plan.tiles)
    label = plan.label
    if _TIMING is not None and plan.bm == 64 and int(_lib.load().svsr_igemm_fwd_kgroups(plan.meta, Ci, Co, 0)) == 2:
        label = label[:-1] + ",2>"          # the in-workgroup K-split instantiation: the profiler's k_igemm_fwd_glds<64, 64, 4, 2>
    _call("svsr_igemm_fwd", _p(inp), _p(wt), _p(out), _p(out_pre), _p(bias), _p(addend), _p(stats), plan.words.data_ptr(), plan.meta,
          Nimg, in_pix, Ci, in_pitch, Co, out_pix, out_pitch, wt_taps, 1 if gelu else (2 if relu else 0), int(out_f32), float(alpha),
          *_drop(drop), _stream(), label=label, flops=flops)
    return st


def igemm_wgrad(plan: WPlan, x: torch.Tensor, dyp: torch.Tensor, dw: torch.Tensor, *, Nimg: int, in_pix: int, Ci: int, in_pitch: int,
                Co: int, out_pix: int, out_pitch: int, wt_taps: int = 1, db: Optional[torch.Tensor] = None, flops: float = 0.0,
                mode: Optional[int] = None) -> None:
    """mode (SVSR_GRAD_ADD_DW = 1 | SVSR_GRAD_ADD_DB = 2 of include/syncvsr_hip.h): None = decided here — dw by the armed GradCoverage,
    else added to; db always added to (bias gradients live in the zero-filled 1-D tail of the buffer)."""
    part = scratch(plan.part_floats) if plan.part_floats else None
    if mode is None:
        mode = _grad_add(dw, Co * wt_taps * Ci) | 2
    _call("svsr_igemm_wgrad_v2", _p(x), _p(dyp), _p(dw), _p(db), plan.words.data_ptr(), plan.meta, Nimg, in_pix, Ci, in_pitch, Co, out_pix,
          out_pitch, wt_taps, _p(part), plan.part_floats, mode, _stream(), label=plan.label, flops=flops)


class _WgradProblem(ctypes.Structure):
    """svsr_wgrad_problem of include/syncvsr_hip.h"""
    _fields_ = [("x", ctypes.c_void_p), ("dy", ctypes.c_void_p), ("dw", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("plan_dev", ctypes.c_void_p),
                ("meta", ctypes.c_void_p), ("Nimg", ctypes.c_int), ("in_pix", ctypes.c_int), ("Ci", ctypes.c_int), ("in_pitch", ctypes.c_int),
                ("Co", ctypes.c_int), ("out_pix", ctypes.c_int), ("out_pitch", ctypes.c_int), ("wt_taps", ctypes.c_int)]


_WG_TABLES: dict = {}


def _group_table(nbytes: int, device) -> torch.Tensor:
    """Problem table of a grouped launch: one grow-only buffer per (device, stream the launch goes to).  The launch may run on the
    model's side stream (STREAM_OVERRIDE) while this function's allocations belong to torch's current stream: a tensor made here and
    dropped on return could be handed to the next main-stream allocation while the side stream still reads it.  In-stream order makes
    re-use by the next grouped launch on the same stream safe (its table writer runs behind this launch's contraction)."""
    key = (str(device), _stream())
    t = _WG_TABLES.get(key)
    if t is None or t.numel() < nbytes:
        if t is not None:
            _SCRATCH_KEEP.append(t)          # a captured graph / recorded step list / pending launch may still hold its address
        t = _WG_TABLES[key] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
    return t


def linear_wgrad_group(problems: Sequence[dict], tile: Optional[int] = None) -> None:
    """problems: keyword arguments of linear_wgrad calls (x, dy, dw, rows, K, N, x_pitch, dy_pitch, seq, db).  tile=None: those whose plan has
    no K split on 64-wide tiles go out as one svsr_igemm_wgrad_group launch; the others (the encoder's attention.output.dense at the LRW shapes)
    as launches of their own.  tile=64 / 128: EVERY problem rides a grouped launch, planned unsplit on tiles of that edge
    (svsr_wgrad_rows_plan_tile) — for a caller whose problems fill the chip together (all encoder layers at once); with tile=128 the problems
    narrower than a tile (K or N below 128) form a second, 64-wide group of the same call."""
    if tile not in (None, 64, 128):
        raise ValueError(f"linear_wgrad_group: tile must be None, 64 or 128, not {tile!r}")
    groups: dict = {}          # tile edge -> (problem records, plans, modes, flops)
    for q in problems:
        rows, K, N, seq, db = q["rows"], q["K"], q["N"], q.get("seq"), q.get("db")
        rp = (rows, 1, 0, 0) if seq is None else (rows // seq[2], seq[2], seq[1], 0)
        geo = (rows, 1, 1) if seq is None else (rows // seq[2], seq[0], seq[2])
        if tile is None:
            plan = wgrad_rows_plan(*rp, K, N, db is not None)
            if not (plan.bc == 64 and int(plan.meta[1]) == 3 and plan.splits == 1):
                linear_wgrad(q["x"], q["dy"], q["dw"], rows=rows, K=K, N=N, x_pitch=q["x_pitch"], dy_pitch=q["dy_pitch"], seq=seq, db=db)
                continue
        else:
            plan = wgrad_rows_plan_tile(*rp, K, N, db is not None, tile if K >= tile and N >= tile else 64)
        g = groups.setdefault(plan.bc, ([], [], [], [0.0]))
        g[0].append(_WgradProblem(_p(q["x"]), _p(q["dy"]), _p(q["dw"]), _p(db), plan.words.data_ptr(), ctypes.addressof(plan.meta),
                                  geo[0], geo[1], K, q["x_pitch"], N, geo[2], q["dy_pitch"], 1))
        g[1].append(plan)
        g[2].append(_grad_add(q["dw"], N * K) | 2)
        g[3][0] += 2.0 * rows * K * N
    for bc in sorted(groups, reverse=True):
        grouped, _, modes, flops = groups[bc]
        arr = (_WgradProblem * len(grouped))(*grouped)
        nbytes = int(_lib.load().svsr_igemm_wgrad_group_bytes(len(grouped)))
        table = _group_table(nbytes, problems[0]["x"].device)
        _call("svsr_igemm_wgrad_group_v2", arr, (ctypes.c_int * len(modes))(*modes), len(grouped), _p(table), nbytes, _stream(),
              label=f"k_igemm_wgrad_group<{bc},{2 if bc == 128 else 3}>", flops=flops[0])


def conv_out_size(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1


def conv2d_fwd(x: torch.Tensor, w16: torch.Tensor, k: int, stride: int, pad: int, want_stats: bool = False):
    """x [N,H,W,Ci] bf16, w16 bf16 [Co][k][k][Ci] -> ([N,Ho,Wo,Co] bf16, stats) where stats is None or the BatchNorm partial
    sums (buffer, rows) to hand to bn_finalize next on this stream."""
    N, H, W, Ci = x.shape
    Co = w16.shape[0]
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    out = torch.empty((N, Ho, Wo, Co), dtype=BF16, device=x.device)
    if _c64_ok(Ci, Co, k, stride, pad, W):
        return out, conv3x3_c64(x, w16, out, None, want_stats, _conv_taps(k, pad))
    st = igemm_fwd(conv_plan(0, N, H, W, Co, k, stride, pad), x, w16, out, Nimg=N, in_pix=H * W, Ci=Ci, in_pitch=Ci, Co=Co,
                   out_pix=Ho * Wo, out_pitch=Co, wt_taps=k * k, want_stats=want_stats, flops=2.0 * N * Ho * Wo * Co * Ci * k * k)
    return out, st


_TAPS: dict = {}


def _conv_taps(k: int, pad: int) -> tuple:
    t = _TAPS.get((k, pad))
    if t is None:
        t = _TAPS[(k, pad)] = tuple((kh - pad, kw - pad, kh * k + kw) for kh in range(k) for kw in range(k))
    return t


C64_CONV = True        # persistent weights-in-LDS kernel for conv3x3(64, 64) stride 1 (False: generic implicit GEMM)


_C64_TABS: dict = {}


def c64_pixtab(N: int, H: int, W: int, device) -> torch.Tensor:
    """Device copy of svsr_conv3x3_c64_pixtab(N, H, W) (padded coordinate -> pixel index or -1), cached per shape like a launch plan."""
    key = (N, H, W, str(device))
    t = _C64_TABS.get(key)
    if t is None:
        lib = _lib.load()
        n = int(lib.svsr_conv3x3_c64_pixtab(N, H, W, None, 0))
        if n <= 0:
            raise _lib.SvsrError(f"svsr_conv3x3_c64_pixtab({N}, {H}, {W}) failed ({n})")
        host = torch.empty(n, dtype=torch.int32)
        got = int(lib.svsr_conv3x3_c64_pixtab(N, H, W, host.data_ptr(), n))
        if got != n:
            raise _lib.SvsrError(f"svsr_conv3x3_c64_pixtab wrote {got} of {n} entries")
        t = _C64_TABS[key] = host.to(device)
    return t


def _c64_ok(Ci: int, Co: int, k: int, stride: int, pad: int, W: int) -> bool:
    return C64_CONV and Ci == 64 and Co == 64 and k == 3 and stride == 1 and pad == 1 and W <= 29


def conv3x3_c64(x: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, addend: Optional[torch.Tensor], want_stats: bool,
                taps: Sequence[tuple[int, int, int]]):
    N, H, W, _ = x.shape
    dy, dx, tw = zip(*taps)
    stats = st = None
    if want_stats:
        rows = _query("svsr_conv3x3_c64_stat_rows", N, H, W)[0]
        stats = scratch(rows * 2 * 64)
        st = (stats, rows)
    _call("svsr_conv3x3_c64", _p(x), _p(wt), _p(out), _p(addend), _p(stats), N, H, W, _ints(dy), _ints(dx), _ints(tw), _p(c64_pixtab(N, H, W, x.device)), _stream(),
          label="k_conv3x3_c64", flops=2.0 * N * H * W * 64 * 64 * 9)
    return st


def conv2d_dgrad(dy: torch.Tensor, w16t: torch.Tensor, k: int, stride: int, pad: int, in_hw: tuple[int, int],
                 addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy [N,Ho,Wo,Co], w16t bf16 [Ci][k][k][Co] (transposed shadow) -> dx [N,H,W,Ci] (+ addend, in place when given).

    One launch for any stride: the plan's classes cover the output-parity classes of a strided convolution with their own
    taps (the transposed convolution never multiplies by the inserted zeros), and pixels no tap reaches are written as 0."""
    N, Ho, Wo, Co = dy.shape
    Ci = w16t.shape[0]
    H, W = in_hw
    dx = torch.empty((N, H, W, Ci), dtype=BF16, device=dy.device) if addend is None else addend
    if stride == 1 and _c64_ok(Ci, Co, k, stride, pad, W):
        taps = tuple((pad - kh, pad - kw, kh * k + kw) for kh in range(k) for kw in range(k))
        conv3x3_c64(dy, w16t, dx, addend, False, taps)
        return dx
    igemm_fwd(conv_plan(1 if addend is None else 2, N, H, W, Ci, k, stride, pad), dy, w16t, dx, Nimg=N, in_pix=Ho * Wo, Ci=Co, in_pitch=Co, Co=Ci, out_pix=H * W,
              out_pitch=Ci, wt_taps=k * k, addend=addend, flops=2.0 * N * Ho * Wo * Co * Ci * k * k)
    return dx


BN_BWD_FUSED = True    # ReLU trunk: first pass of the BatchNorm backward inside the producing data-gradient launch (False: separate pass)


def conv2d_dgrad_bn(dy: torch.Tensor, w16t: torch.Tensor, k: int, stride: int, pad: int, in_hw: tuple[int, int],
                    addend: Optional[torch.Tensor], y: Optional[torch.Tensor], x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                    gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, act: int = 1):
    """conv2d_dgrad whose result is the gradient of y = relu(bn(x) [+ residual]) (y, x shaped like the result): the launch stores
    g = (y > 0) * (dgrad + addend) instead and takes the first pass of that BatchNorm's backward in its epilogue.
    y=None (no residual branch): the mask is recomputed from x, gamma, beta and y is not read.
    act=2 (Swish): g = (dgrad + addend) * swish'(bn(x) + r) where `y` is the residual INPUT r (or None); gamma / beta required.
    -> (g, (stats, rows)) for bn_bwd_from_stats.  In place when addend is given."""
    N, Ho, Wo, Co = dy.shape
    Ci = w16t.shape[0]
    H, W = in_hw
    if x.shape != (N, H, W, Ci) or not x.is_contiguous() or (y is not None and (y.shape != x.shape or not y.is_contiguous())):
        raise ValueError("conv2d_dgrad_bn: y / x must be contiguous tensors with the geometry of the result")
    if (y is None or act == 2) and (gamma is None or beta is None):
        raise ValueError("conv2d_dgrad_bn: y=None / act=2 need gamma and beta")
    g = torch.empty((N, H, W, Ci), dtype=BF16, device=dy.device) if addend is None else addend
    if stride == 1 and _c64_ok(Ci, Co, k, stride, pad, W):
        taps = tuple((pad - kh, pad - kw, kh * k + kw) for kh in range(k) for kw in range(k))
        tdy, tdx, tw = zip(*taps)
        rows = _query("svsr_conv3x3_c64_stat_rows", N, H, W)[0]
        stats = scratch(rows * 2 * 64)
        _call("svsr_conv3x3_c64_dgrad_bn", _p(dy), _p(w16t), _p(g), _p(addend), _p(stats), N, H, W, _ints(tdy), _ints(tdx), _ints(tw),
              _p(y), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), act, _p(c64_pixtab(N, H, W, dy.device)), _stream(), label="k_conv3x3_c64+bn", flops=2.0 * N * H * W * 64 * 64 * 9)
        return g, (stats, rows)
    plan = conv_plan(1, N, H, W, Ci, k, stride, pad)        # mode 1: every pixel of the result is visited once
    stats = scratch(plan.tiles * 2 * Ci)
    _call("svsr_igemm_dgrad_bn", _p(dy), _p(w16t), _p(g), _p(addend), _p(stats), plan.words.data_ptr(), plan.meta, N, Ho * Wo, Co, Co, Ci,
          H * W, Ci, k * k, _p(y), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), act, _stream(), label=plan.label + "+bn", flops=2.0 * N * Ho * Wo * Co * Ci * k * k)
    return g, (stats, plan.tiles)


DGRAD2 = True          # downsample blocks: the 1x1 branch's data gradient rides the 3x3 launch (False: two launches, the second adds to the first)


def conv2d_dgrad2(dy: torch.Tensor, w16t: torch.Tensor, dy2: torch.Tensor, w16t2: torch.Tensor, in_hw: tuple[int, int], bn: Optional[tuple] = None):
    """The input gradient of a downsample block in one launch: the 3x3 / stride 2 / pad 1 data gradient of (dy, w16t [Ci][3][3][Co]) plus the
    1x1 / stride 2 data gradient of (dy2, w16t2 [Ci][Co]), both [N,Ho,Wo,Co], summed in fp32 and rounded once -> dx [N,H,W,Ci].
    bn = (y, x, mean, rstd, gamma, beta, act): the epilogue of conv2d_dgrad_bn on the sum -> (g, (stats, rows))."""
    N, Ho, Wo, Co = dy.shape
    Ci = w16t.shape[0]
    H, W = in_hw
    if dy2.shape != dy.shape or not (dy.is_contiguous() and dy2.is_contiguous()) or w16t2.numel() != Ci * Co or w16t.numel() != Ci * 9 * Co:
        raise ValueError("conv2d_dgrad2: dy2 must have dy's shape, the weights must be [Ci][3][3][Co] and [Ci][Co]")
    plan = conv_plan(3, N, H, W, Ci, 3, 2, 1)
    dx = torch.empty((N, H, W, Ci), dtype=BF16, device=dy.device)
    flops = 2.0 * N * Ho * Wo * Co * Ci * 10
    head = (_p(dy), _p(w16t), _p(dy2), _p(w16t2), _p(dx))
    label = plan.label[:-1] + ",1,true>"          # the profiler's name of the two-operand instantiation
    if bn is None:
        _call("svsr_igemm_dgrad2", *head, None, None, None, plan.words.data_ptr(), plan.meta, N, Ho * Wo, Co, Co, Ci, H * W, Ci, 9, 0, 0, 1.0,
              *_drop(None), _stream(), label=label, flops=flops)
        return dx
    y, x, mean, rstd, gamma, beta, act = bn
    if x.shape != dx.shape or not x.is_contiguous() or (y is not None and (y.shape != x.shape or not y.is_contiguous())):
        raise ValueError("conv2d_dgrad2: y / x must be contiguous tensors with the geometry of the result")
    if (y is None or act == 2) and (gamma is None or beta is None):
        raise ValueError("conv2d_dgrad2: y=None / act=2 need gamma and beta")
    stats = scratch(plan.tiles * 2 * Ci)
    _call("svsr_igemm_dgrad2_bn", *head, _p(stats), plan.words.data_ptr(), plan.meta, N, Ho * Wo, Co, Co, Ci, H * W, Ci, 9, _p(y), _p(x),
          _p(mean), _p(rstd), _p(gamma), _p(beta), act, _stream(), label=label + "+bn", flops=flops)
    return dx, (stats, plan.tiles)


def bn_bwd_from_stats(g, x, mean, rstd, gamma, stats, coef, dgamma, dbeta) -> torch.Tensor:
    """Second half of the BatchNorm backward after conv2d_dgrad_bn: -> dx (gradient of the BatchNorm input x)."""
    part, rows = stats
    C = x.shape[-1]
    dx = torch.empty_like(x)
    _call("svsr_bn_bwd_from_stats", _p(g), _p(x), _p(mean), _p(rstd), _p(gamma), _p(part), rows, _p(coef), _p(dgamma), _p(dbeta), _p(dx),
          x.numel() // C, C, _stream())
    return dx


def bn_bwd_from_stats_ds(g, x, mean, rstd, gamma, stats, coef, dgamma, dbeta, xd, mean_d, rstd_d):
    """bn_bwd_from_stats for bn2 of a downsample block, whose apply pass also takes the first pass of the 1x1 branch's BatchNorm backward
    (xd its input): -> (dx, (rows, count)) with the partial rows of that branch, in this stream's scratch, for its own bn_bwd_from_stats —
    which has to be the next call on this stream that uses the scratch."""
    part, rows = stats
    C = x.shape[-1]
    dx = torch.empty_like(x)
    rows_d = _query("svsr_bn_act_bwd_rows", x.numel() // C, C)[0]
    slots = scratch(rows_d * 2 * C)
    _call("svsr_bn_bwd_from_stats_ds", _p(g), _p(x), _p(mean), _p(rstd), _p(gamma), _p(part), rows, _p(coef), _p(dgamma), _p(dbeta), _p(dx),
          _p(xd), _p(mean_d), _p(rstd_d), _p(slots), x.numel() // C, C, _stream())
    return dx, (slots, rows_d)


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, k: int, stride: int, pad: int, use_tr: bool = True, mode: Optional[int] = None) -> None:
    """dw fp32 [Co][k][k][Ci] += sum dy[n,y,x,co] * x[n, y*s+kh-pad, x*s+kw-pad, ci]  (mode 0: = 0.f + sum, see igemm_wgrad)."""
    N, H, W, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    if HALO_WGRAD and use_tr and k == 3 and stride == 1 and pad == 1 and W <= 29 and H * W >= 100 and Ci % 64 == 0 and Co % 64 == 0:
        # all nine taps in one pass over zero-padded coordinates (wgrad3x3.hip)
        _, nfl = _query("svsr_conv3x3_wgrad_plan", N, H, W, Ci, Co)
        part = scratch(nfl) if nfl else None
        _call("svsr_conv3x3_wgrad_v2", _p(x), _p(dy), _p(dw), N, H, W, Ci, Co, _p(part), nfl, _grad_add(dw, Co * 9 * Ci) if mode is None else mode & 1, _stream(),
              label="k_wgrad3x3_halo", flops=2.0 * N * H * W * Co * Ci * 9)
        return
    igemm_wgrad(wgrad_conv_plan(N, H, W, Ci, Co, k, stride, pad), x, dy, dw, Nimg=N, in_pix=H * W, Ci=Ci, in_pitch=Ci, Co=Co,
                out_pix=Ho * Wo, out_pitch=Co, wt_taps=k * k, flops=2.0 * N * Ho * Wo * Co * Ci * k * k, mode=mode)


def halo_wgrad_ok(x: torch.Tensor, dy: torch.Tensor, k: int, stride: int, pad: int) -> bool:
    N, H, W, Ci = x.shape
    Co = dy.shape[-1]
    return HALO_WGRAD and k == 3 and stride == 1 and pad == 1 and W <= 29 and H * W >= 100 and Ci % 64 == 0 and Co % 64 == 0


# The two slab sets of the chained halo weight gradient, per stream: launch i writes set i mod 2 while its workgroups add set (i - 1) mod 2
# into the previous convolution's dW.  Not the per-stream scratch: other producers (the strided convolutions' weight gradients, the postponed
# column sums) go through that between two launches of a chain.  Outgrown sets are kept alive like outgrown scratch.
_W3_SETS: dict[tuple, torch.Tensor] = {}


def _w3_set(which: int, nfloats: int) -> torch.Tensor:
    key = (_stream(), which)
    t = _W3_SETS.get(key)
    if t is None or t.numel() < nfloats:
        if t is not None:
            _SCRATCH_KEEP.append(t)
        t = _W3_SETS[key] = torch.empty(max(int(nfloats), 1 << 20), dtype=torch.float32, device="cuda")
    return t


def _w3_outside_groups(what: str) -> None:
    if _REC is not None and _REC.cur_group is not None:
        raise RuntimeError(f"{what} inside op group {_REC.cur_group} of a recorded step: a replay that skips the group would leave the chain's "
                           "pending slabs un-added (flush the chain before the group)")


def conv3x3_wgrad_chain(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, pending: Optional[dict], mode: Optional[int] = None) -> Optional[dict]:
    """The halo weight gradient of conv2d_wgrad (halo_wgrad_ok shapes) as a link of a chain on the current stream: the launch leaves its
    split-K slabs un-added and returns them as a `pending` record; the NEXT call's launch — any geometry, any channel counts — adds them into
    their dw in its prologue (same order of additions as the stand-alone reduce, same bits), and conv3x3_wgrad_flush ends the chain.  A dw is
    final only behind the launch that carries its record.  -> the new record (None where the plan has one split: dw is written directly)."""
    N, H, W, Ci = x.shape
    Co = dy.shape[-1]
    _w3_outside_groups("conv3x3_wgrad_chain")
    if pending is not None and pending["stream"] != _stream():
        raise RuntimeError("conv3x3_wgrad_chain: the pending slabs were written on another stream")
    splits, nfl = _query("svsr_conv3x3_wgrad_plan", N, H, W, Ci, Co)
    which = 0 if pending is None else 1 - pending["set"]
    part = _w3_set(which, nfl) if nfl else None
    add = _grad_add(dw, Co * 9 * Ci) if mode is None else mode & 1
    pp = pending or dict(part=None, dw=None, splits=0, Ci=0, Co=0, add=0)
    _call("svsr_conv3x3_wgrad_chain", _p(x), _p(dy), _p(dw), N, H, W, Ci, Co, _p(part), nfl, add, 1, _p(pp["part"]), _p(pp["dw"]), pp["splits"],
          pp["Ci"], pp["Co"], pp["add"], _stream(), label="k_wgrad3x3_halo", flops=2.0 * N * H * W * Co * Ci * 9)
    return dict(part=part, dw=dw, splits=splits, Ci=Ci, Co=Co, add=add, set=which, stream=_stream()) if splits > 1 else None


def conv3x3_wgrad_flush(pending: Optional[dict]) -> None:
    """Ends a chain: the stand-alone reduce of the last launch's slabs."""
    if pending is None:
        return
    _w3_outside_groups("conv3x3_wgrad_flush")
    if pending["stream"] != _stream():
        raise RuntimeError("conv3x3_wgrad_flush: the pending slabs were written on another stream")
    _call("svsr_conv3x3_wgrad_reduce", _p(pending["part"]), _p(pending["dw"]), pending["splits"], pending["Ci"], pending["Co"], pending["add"],
          _stream(), label="k_wgrad3_reduce")


def linear_fwd(x: torch.Tensor, w16: torch.Tensor, bias: Optional[torch.Tensor], *, rows: int, K: int, N: int, x_pitch: int,
               out: Optional[torch.Tensor] = None, out_pitch: Optional[int] = None, gelu: bool = False,
               out_f32: bool = False, addend: Optional[torch.Tensor] = None,
               seq: Optional[tuple[int, int, int]] = None, relu: bool = False, alpha: float = 1.0,
               drop=None) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
    """out[rows, N] = alpha * dropout(act(x[rows, K] @ w16[N, K]^T + bias)) + addend, act = gelu | relu | none.  `seq=(S, s0, n)` selects rows s0..s0+n-1 of every
    length-S sequence of x (x is [B*S, K]) as the source and writes a dense [B*n, N] result."""
    out_pitch = out_pitch or N
    if out is None:
        out = torch.empty((rows, out_pitch), dtype=torch.float32 if out_f32 else BF16, device=x.device)
    pre = torch.empty_like(out) if gelu else None
    if seq is None:
        plan, geo = rows_plan(rows, 1, 0, 0, N), dict(Nimg=rows, in_pix=1, out_pix=1)
    else:
        S, s0, n = seq
        plan, geo = rows_plan(rows // n, n, s0, 0, N), dict(Nimg=rows // n, in_pix=S, out_pix=n)
    igemm_fwd(plan, x, w16, out, Ci=K, in_pitch=x_pitch, Co=N, out_pitch=out_pitch, bias=bias, addend=addend, gelu=gelu, out_pre=pre,
              out_f32=out_f32, relu=relu, alpha=alpha, drop=drop, flops=2.0 * rows * N * K, **geo)
    return out, pre


def linear_dgrad(dy: torch.Tensor, w16t: torch.Tensor, *, rows: int, N: int, K: int, dy_pitch: int, out: Optional[torch.Tensor] = None,
                 addend: Optional[torch.Tensor] = None, seq: Optional[tuple[int, int, int]] = None, alpha: float = 1.0,
                 drop=None) -> torch.Tensor:
    """dx[rows, K] = dy[rows, N] @ w16t[K, Npad]^T-of-transpose, i.e. dy @ W.  With `seq=(S, s0, n)` the dense dy rows
    [B*n] are scattered to rows s0.. of every length-S sequence of dx [B*S, K]."""
    Np = w16t.shape[-1]
    if seq is None:
        if out is None:
            out = torch.empty((rows, K), dtype=BF16, device=dy.device)
        plan, geo = rows_plan(rows, 1, 0, 0, K), dict(Nimg=rows, in_pix=1, out_pix=1)
    else:
        S, s0, n = seq
        assert out is not None
        plan, geo = rows_plan(rows // n, n, 0, s0, K), dict(Nimg=rows // n, in_pix=n, out_pix=S)
    igemm_fwd(plan, dy, w16t, out, Ci=Np, in_pitch=dy_pitch, Co=K, out_pitch=K, addend=addend, alpha=alpha, drop=drop,
              flops=2.0 * rows * N * K, **geo)
    return out


def linear_dgrad_bn(dy: torch.Tensor, w16t: torch.Tensor, *, rows: int, N: int, K: int, dy_pitch: int, x: torch.Tensor, mean: torch.Tensor,
                    rstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, act: int):
    """linear_dgrad whose result is the gradient of act(bn(x)) (x [rows, K], no residual branch): the launch stores
    g = dgrad * act'(bn(x)) instead and takes the first pass of that BatchNorm's backward in its epilogue (see conv2d_dgrad_bn).
    -> (g, (stats, rows)) for bn_bwd_from_stats."""
    Np = w16t.shape[-1]
    if x.shape != (rows, K) or not x.is_contiguous():
        raise ValueError("linear_dgrad_bn: x must be a contiguous [rows, K] tensor")
    g = torch.empty((rows, K), dtype=BF16, device=dy.device)
    plan = rows_plan(rows, 1, 0, 0, K)
    stats = scratch(plan.tiles * 2 * K)
    _call("svsr_igemm_dgrad_bn", _p(dy), _p(w16t), _p(g), None, _p(stats), plan.words.data_ptr(), plan.meta, rows, 1, Np, dy_pitch, K,
          1, K, 1, None, _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), act, _stream(), label=plan.label + "+bn", flops=2.0 * rows * N * K)
    return g, (stats, plan.tiles)


_CONST_VECS: dict = {}


def linear_dgrad_relu(dy: torch.Tensor, w16t: torch.Tensor, *, rows: int, N: int, K: int, dy_pitch: int, y: torch.Tensor, gscale: float = 1.0):
    """linear_dgrad for a layer whose input was y = dropout(relu(z)) [rows, K]: the launch stores dz = (y > 0 ? gscale * dgrad : 0) and the column
    sums of dz per row tile (svsr_igemm_dgrad_relu) -> (dz, (stats, tiles)): colsum_rows(stats, tiles, 2 * K, db, K) is the bias gradient of
    the layer that produced z."""
    Np = w16t.shape[-1]
    if y.shape != (rows, K) or not y.is_contiguous():
        raise ValueError("linear_dgrad_relu: y must be a contiguous [rows, K] tensor")
    key = (str(dy.device), K)
    cv = _CONST_VECS.get(key)
    if cv is None:
        import numpy as np          # (host arrays + copies: made once, also inside a recorded step — no fill kernel for the recorder to miss)

        cv = _CONST_VECS[key] = tuple(torch.from_numpy(np.full(K, v, dtype=np.float32)).to(dy.device) for v in (0.0, 1.0))
    dz = torch.empty((rows, K), dtype=BF16, device=dy.device)
    plan = rows_plan(rows, 1, 0, 0, K)
    stats = torch.empty(plan.tiles * 2 * K, dtype=torch.float32, device=dy.device)      # (a buffer of its own: its sum may run later, on another stream)
    _call("svsr_igemm_dgrad_relu", _p(dy), _p(w16t), _p(dz), _p(stats), plan.words.data_ptr(), plan.meta, rows, 1, Np, dy_pitch, K, 1, K, 1,
          _p(y), _p(cv[0]), _p(cv[1]), float(gscale), _stream(), label=plan.label + "+relu", flops=2.0 * rows * N * K)
    return dz, (stats, plan.tiles)


def linear_wgrad(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, *, rows: int, K: int, N: int, x_pitch: int, dy_pitch: int,
                 seq: Optional[tuple[int, int, int]] = None, db: Optional[torch.Tensor] = None, mode: Optional[int] = None) -> None:
    """dw fp32 [N][K] += dy[rows, N]^T @ x[rows, K];  db fp32 [N] += column sums of dy (bias gradient), if given."""
    if seq is None:
        plan, geo = wgrad_rows_plan(rows, 1, 0, 0, K, N, db is not None), dict(Nimg=rows, in_pix=1, out_pix=1)
    else:
        S, s0, n = seq
        plan, geo = wgrad_rows_plan(rows // n, n, s0, 0, K, N, db is not None), dict(Nimg=rows // n, in_pix=S, out_pix=n)
    igemm_wgrad(plan, x, dy, dw, Ci=K, in_pitch=x_pitch, Co=N, out_pitch=dy_pitch, db=db, flops=2.0 * rows * N * K, mode=mode, **geo)


# --------------------------------------------------------------------------------------------------
# stem
# --------------------------------------------------------------------------------------------------
_STEM_WS: dict = {}


def stem_conv_fwd(videos: torch.Tensor, w: torch.Tensor, want_stats: bool = False, use_ws: bool = True, out: Optional[torch.Tensor] = None):
    """-> (out [B*T,H/2,W/2,64] bf16, BatchNorm partials (buffer, rows) or None).  use_ws=False withholds the workspace of the DMA-fed
    kernel: the direct kernel then runs at any W (what a C-ABI caller without a workspace gets).  out: a contiguous tensor to write into."""
    B, C, T, H, W = videos.shape
    assert C == 1 and videos.dtype == torch.float32 and videos.is_contiguous()
    if out is None:
        out = torch.empty((B * T, H // 2, W // 2, 64), dtype=BF16, device=videos.device)
    assert out.shape == (B * T, H // 2, W // 2, 64) and out.dtype == BF16 and out.is_contiguous()
    stats = st = None
    if want_stats:
        rows = _query("svsr_stem_conv_fwd_stat_rows", B, T, H, W)[0]
        stats = scratch(rows * 2 * 64)
        st = (stats, rows)
    nws = _query("svsr_stem_conv_fwd_ws_bytes", B, T, H, W)[0] if use_ws else 0
    ws = None
    if nws:         # bf16 copy of the clip + packed weights for the DMA-fed kernel: one grow-only buffer per device and stream (`stats`
        key = (videos.device, _stream())        # lives in the shared scratch; variable-length LRS batches must not pile up one buffer per shape)
        ws = _STEM_WS.get(key)
        if ws is None or ws.numel() < nws:
            if ws is not None:
                _SCRATCH_KEEP.append(ws)      # a captured graph / recorded step list may still hold its address
            ws = _STEM_WS[key] = torch.empty(nws, dtype=torch.uint8, device=videos.device)
    _call("svsr_stem_conv_fwd", _p(videos), _p(w), _p(out), _p(stats), B, T, H, W, _p(ws), nws, _stream(),
          label="k_stem_conv_fwd", flops=2.0 * B * T * (H // 2) * (W // 2) * 64 * 245)
    return out, st


def stem_conv_wgrad(videos: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, use_tr: bool = True) -> None:
    B, _, T, H, W = videos.shape
    _, nfl = _query("svsr_stem_conv_wgrad_plan", B, T, H, W)
    _call("svsr_stem_conv_wgrad", _p(videos), _p(dy), _p(dw), B, T, H, W, int(use_tr), _p(scratch(nfl)), nfl, _stream(),
          label=f"k_stem_conv_wgrad<{'true' if use_tr else 'false'}>", flops=2.0 * B * T * (H // 2) * (W // 2) * 64 * 245)


ACT_NONE, ACT_RELU, ACT_GELU, ACT_SWISH = 0, 1, 1, 2     # ReLU/GELU share code 1: ReLU in the BN passes, GELU in the stem pass


def stem_bn_gelu_pool_fwd(x: torch.Tensor, mean, rstd, gamma, beta, act: int = ACT_GELU, want_win: bool = False, out: Optional[torch.Tensor] = None):
    """-> (y, amax) or, with want_win, (y, amax, xwin): xwin = the convolution output at every window's arg-max, for
    stem_bn_gelu_pool_bwd(xwin=...) (reduce pass over pooled-size tensors, apply pass without activation derivatives).
    out: a contiguous tensor to write y into."""
    N, Hc, Wc, C = x.shape
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    y = torch.empty((N, Hp, Wp, C), dtype=BF16, device=x.device) if out is None else out
    assert y.shape == (N, Hp, Wp, C) and y.dtype == BF16 and y.is_contiguous()
    amax = torch.empty((N, Hp, Wp, C), dtype=torch.uint8, device=x.device)
    xwin = torch.empty((N, Hp, Wp, C), dtype=BF16, device=x.device) if want_win else None
    _call("svsr_stem_bn_act_pool_fwd", _p(x), _p(y), _p(amax), _p(mean), _p(rstd), _p(gamma), _p(beta), N, Hc, Wc, Hp, Wp, C, act, _p(xwin), _stream())
    return (y, amax, xwin) if want_win else (y, amax)


def stem_bn_gelu_pool_bwd(dpool, amax, x, mean, rstd, gamma, beta, coef, dgamma, dbeta, act: int = ACT_GELU, xwin=None, want_dx: bool = True,
                          out: Optional[torch.Tensor] = None):
    """-> dx (gradient of the stem convolution's output); with want_dx=False (needs xwin) -> gpool, and `coef` is left filled: the inputs of
    stem_bwd_wgrad, which makes dx tile by tile inside the weight-gradient pass instead of writing it.  out: a contiguous tensor to write dx into."""
    N, Hc, Wc, C = x.shape
    _, Hp, Wp, _ = dpool.shape
    assert want_dx or xwin is not None
    dx = (torch.empty_like(x) if out is None else out) if want_dx else None
    assert dx is None or (dx.shape == x.shape and dx.dtype == x.dtype and dx.is_contiguous())
    slots = scratch(_query("svsr_stem_bn_act_pool_bwd_rows", N, Hc, Wc, C)[0] * 2 * C)
    gpool = torch.empty_like(dpool) if xwin is not None else None
    _call("svsr_stem_bn_act_pool_bwd", _p(dpool), _p(amax), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(slots), _p(coef),
          _p(dgamma), _p(dbeta), _p(dx), N, Hc, Wc, Hp, Wp, C, act, _p(xwin), _p(gpool), _stream())
    return dx if want_dx else gpool


def stem_bwd_wgrad_ok(videos: torch.Tensor) -> bool:
    """Whether the stem's backward apply pass can run inside its weight-gradient pass (svsr_stem_bwd_wgrad) at this shape."""
    B, _, T, H, W = videos.shape
    return bool(_lib.load().svsr_stem_bwd_wgrad_ok(B, T, H, W))


def stem_bwd_wgrad(videos: torch.Tensor, gpool, amax, x, mean, rstd, coef, dw: torch.Tensor) -> None:
    """dw += the stem convolution's weight gradient, from the pooled-size gradient `gpool` (stem_bn_gelu_pool_bwd(want_dx=False)),
    the window winners `amax`, the convolution output `x` and the finalised BatchNorm-backward coefficients `coef`."""
    B, _, T, H, W = videos.shape
    _, nfl = _query("svsr_stem_conv_wgrad_plan", B, T, H, W)
    _call("svsr_stem_bwd_wgrad", _p(videos), _p(gpool), _p(amax), _p(x), _p(mean), _p(rstd), _p(coef), _p(dw), B, T, H, W, _p(scratch(nfl)), nfl,
          _stream(), label="k_stem_bwd_wgrad", flops=2.0 * B * T * (H // 2) * (W // 2) * 64 * 245)


# --------------------------------------------------------------------------------------------------
# BatchNorm / activation / pooling
# --------------------------------------------------------------------------------------------------
def bn_finalize(stats, C: int, count: int, mean, rstd, running_mean=None, running_var=None, nbt=None) -> None:
    """stats = (buffer, rows): the partial sums [rows][2][C] the producing convolution just wrote on this stream."""
    part, rows = stats
    _call("svsr_bn_finalize", _p(part), rows, C, float(count), BN_EPS, BN_MOMENTUM, _p(mean), _p(rstd), _p(running_mean), _p(running_var),
          _p(nbt), _stream())


def bn_eval_prepare(running_mean, running_var, mean, rstd) -> None:
    _call("svsr_bn_eval_prepare", _p(running_mean), _p(running_var), running_mean.numel(), BN_EPS, _p(mean), _p(rstd), _stream())


def bn_act_fwd(x, res, mean, rstd, gamma, beta, act: int) -> torch.Tensor:
    C = x.shape[-1]
    y = torch.empty_like(x)
    _call("svsr_bn_act_fwd", _p(x), _p(res), _p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), x.numel() // C, C, act, _stream())
    return y


def bn_act_fwd2(x, xd, mean, rstd, gamma, beta, mean_d, rstd_d, gamma_d, beta_d) -> torch.Tensor:
    """relu(bn(x) + bn_d(xd)) in one launch: bn_act_fwd(x, bn_act_fwd(xd, None, ..., 0), ..., 1) bit for bit."""
    C = x.shape[-1]
    y = torch.empty_like(x)
    _call("svsr_bn_act_fwd2", _p(x), _p(xd), _p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(mean_d), _p(rstd_d), _p(gamma_d), _p(beta_d),
          x.numel() // C, C, _stream())
    return y


def bn_act_bwd(dy, y, x, mean, rstd, gamma, coef, dgamma, dbeta, act: int, want_dres: bool, beta=None, res=None):
    C = x.shape[-1]
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    slots = scratch(_query("svsr_bn_act_bwd_rows", x.numel() // C, C)[0] * 2 * C)
    _call("svsr_bn_act_bwd", _p(dy), _p(y), _p(x), _p(mean), _p(rstd), _p(gamma), _p(slots), _p(coef), _p(dgamma), _p(dbeta), _p(dx),
          _p(dres), x.numel() // C, C, act, _p(beta), _p(res), _stream())
    return dx, dres


def avgpool_fwd(x: torch.Tensor) -> torch.Tensor:
    N, H, W, C = x.shape
    y = torch.empty((N, C), dtype=BF16, device=x.device)
    _call("svsr_avgpool_fwd", _p(x), _p(y), N, H * W, C, _stream())
    return y


def avgpool_bwd(dy: torch.Tensor, shape) -> torch.Tensor:
    N, H, W, C = shape
    dx = torch.empty(shape, dtype=BF16, device=dy.device)
    _call("svsr_avgpool_bwd", _p(dy), _p(dx), N, H * W, C, _stream())
    return dx


# --------------------------------------------------------------------------------------------------
# transformer passes
# --------------------------------------------------------------------------------------------------
def add_ln_fwd(a, r, gamma, beta, eps: float):
    R, D = a.shape
    y = torch.empty_like(a)
    mean = torch.empty(R, dtype=torch.float32, device=a.device)
    rstd = torch.empty(R, dtype=torch.float32, device=a.device)
    _call("svsr_add_ln_fwd", _p(a), _p(r), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), R, D, eps, _stream())
    return y, mean, rstd


def colsum_rows(part, rows: int, ld: int, out0, n0: int, out1=None, n1: int = 0) -> None:
    _call("svsr_colsum_rows", _p(part), rows, ld, _p(out0), n0, _p(out1), n1, 1, 1.0, _stream())


class _ColsumEntry(ctypes.Structure):       # include/syncvsr_hip.h svsr_colsum_rows_multi: 64 bytes
    _fields_ = [("ws", ctypes.c_void_p), ("out0", ctypes.c_void_p), ("out1", ctypes.c_void_p), ("ld", ctypes.c_int64), ("n0", ctypes.c_int64),
                ("n1", ctypes.c_int64), ("nrows", ctypes.c_int32), ("accumulate", ctypes.c_int32), ("scale", ctypes.c_float), ("reserved", ctypes.c_int32)]


COLSUM_MULTI = True       # host-side knob "colsum_multi": a layer's postponed parameter-gradient reductions as one launch per 16


def _deferred_colsum(part, rows: int, ld: int, out0, n0: int, out1=None, n1: int = 0):
    """A postponed colsum_rows(...) (accumulating) as a closure for a model's deferred list; run_deferred() merges neighbours into one launch."""
    f = lambda: colsum_rows(part, rows, ld, out0, n0, out1, n1)
    f.colsum = (part, rows, ld, out0, n0, out1, n1)
    return f


def run_deferred(fns) -> None:
    """Runs a model's postponed reductions on the current stream: those made by _deferred_colsum as svsr_colsum_rows_multi launches (results
    identical to the separate launches: every problem keeps its own order of additions), the others one by one."""
    batch: list = []

    def flush():
        if len(batch) == 1:
            colsum_rows(*batch[0])
        elif batch:
            arr = (_ColsumEntry * len(batch))()
            for e, (part, rows, ld, out0, n0, out1, n1) in zip(arr, batch):
                e.ws, e.out0, e.out1, e.ld, e.n0, e.n1, e.nrows, e.accumulate, e.scale = _p(part), _p(out0), _p(out1), ld, n0, n1, rows, 1, 1.0
            _call("svsr_colsum_rows_multi", arr, len(batch), _stream())
        batch.clear()

    for f in fns:
        a = getattr(f, "colsum", None)
        if a is None or not COLSUM_MULTI:
            flush()
            f()
            continue
        outs = {_p(a[3]), _p(a[5])} - {None}
        if any(({_p(b[3]), _p(b[5])} - {None}) & outs for b in batch):       # (two contributions to one gradient: separate launches, in order)
            flush()
        batch.append(a)
    flush()


def add_ln_bwd(dy, a, r, gamma, mean, rstd, dgamma, dbeta, addend=None, out=None, defer: Optional[list] = None, branch=None):
    """defer = a list: the parameter-gradient reduction is not launched; a closure that launches it (on whatever stream is current when it
    is called) is appended instead — the partial rows then live in a buffer of their own.
    branch = (alpha, drop) (with defer): additionally returns alpha * dropout_mask(ds) — the gradient of the residual branch that ends in this
    sum, bit for bit what scale_bf16(ds, alpha, drop) would compute — as a second tensor: -> (ds, ds_branch)."""
    R, D = a.shape
    ds = torch.empty_like(a) if out is None else out
    if defer is not None:
        rows = _query("svsr_add_ln_bwd_rows", R)[0]
        part = torch.empty(rows * 2 * D, dtype=torch.float32, device=a.device)
        if branch is not None:
            alpha, drop = branch
            ds2 = torch.empty_like(a)
            _call("svsr_add_ln_bwd_branch", _p(dy), _p(a), _p(r), _p(gamma), _p(mean), _p(rstd), _p(ds), R, D, _p(addend), _p(part), _p(ds2), float(alpha),
                  *_drop(drop), _stream())
            defer.append((_deferred_colsum(part, rows, 2 * D, dgamma, D, dbeta, D), part))
            return ds, ds2
        _call("svsr_add_ln_bwd_partials", _p(dy), _p(a), _p(r), _p(gamma), _p(mean), _p(rstd), _p(ds), R, D, _p(addend), _p(part), _stream())
        defer.append((_deferred_colsum(part, rows, 2 * D, dgamma, D, dbeta, D), part))
        return ds
    part = scratch(_query("svsr_add_ln_bwd_rows", R)[0] * 2 * D)
    _call("svsr_add_ln_bwd", _p(dy), _p(a), _p(r), _p(gamma), _p(mean), _p(rstd), _p(ds), _p(dgamma), _p(dbeta), R, D, _p(addend), _p(part),
          _stream())
    return ds


def embed_ln_fwd(feats, cls, pos, type0, gamma, beta, B: int, S: int, D: int, eps: float, drop_in=None, drop_out=None):
    """drop_in / drop_out = (seed word, site, p) of emb_dropout and BertEmbeddings' dropout (same seed word), or None."""
    dev = feats.device
    seed = (drop_in or drop_out or (None,))[0]
    si, pi = (drop_in[1], drop_in[2]) if drop_in is not None else (0, 0.0)
    so, po = (drop_out[1], drop_out[2]) if drop_out is not None else (0, 0.0)
    s = torch.empty((B * S, D), dtype=BF16, device=dev)
    y = torch.empty((B * S, D), dtype=BF16, device=dev)
    mean = torch.empty(B * S, dtype=torch.float32, device=dev)
    rstd = torch.empty(B * S, dtype=torch.float32, device=dev)
    _call("svsr_embed_ln_fwd", _p(feats), _p(cls), _p(pos), _p(type0), _p(gamma), _p(beta), _p(s), _p(y), _p(mean), _p(rstd), B, S, D,
          eps, _p(seed), int(si), float(pi), int(so), float(po), _stream())
    return s, y, mean, rstd


def embed_bwd_scatter(ds, dcls, dpos, dtype0, B: int, S: int, D: int, drop_in=None) -> torch.Tensor:
    dfeats = torch.empty((B * (S - 1), D), dtype=BF16, device=ds.device)
    _call("svsr_embed_bwd_scatter", _p(ds), _p(dfeats), _p(dcls), _p(dpos), _p(dtype0), B, S, D, _p(scratch(S * D)), *_drop(drop_in),
          _stream())
    return dfeats


# -- fused forward of the HF-BERT encoder layers (csrc/enc_fused.hip) ---------------------------------
class _EncLayer(ctypes.Structure):
    """svsr_enc_layer of include/syncvsr_hip.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("wqkv", "wo", "w1", "w2", "bqkv", "bo", "b1", "b2", "g1", "be1", "g2", "be2",
                                               "qkv", "probs", "ctx", "ao", "x1", "z", "hg", "f", "xout", "m1", "r1", "m2", "r2")] + \
               [("site_probs", ctypes.c_uint), ("site_ao", ctypes.c_uint), ("site_fo", ctypes.c_uint), ("pad_", ctypes.c_uint)]


ENC_FUSED = os.environ.get("SVSR_ENC_FUSED", "1") != "0"     # the whole encoder forward as one launch (False: seven launches per layer)
_ENC_WS: dict = {}


_ENC_FUSED_USED = False      # a fused-encoder launch has been issued by this process (svsr_enc_fwd / svsr_enc_bwd)


def enc_gave_up_peek() -> bool:
    """True once a fused-encoder launch had a bounded cluster wait give up — read from pinned host memory, NO synchronisation (the value may
    trail the device by the flight time of one store): engine.TrainStep looks at it before every step."""
    return _ENC_FUSED_USED and bool(_lib.load().svsr_enc_gave_up_peek())


def check_enc_clusters(reset: bool = True) -> bool:
    """True if any svsr_enc_fwd / svsr_enc_bwd launch since the last reset had a bounded cluster wait give up (synchronises the device; not
    called at all while no fused launch has been issued).  Raises when the flag itself cannot be read (a sticky HIP error, the wrong device)."""
    if not _ENC_FUSED_USED:
        return False
    rc = int(_lib.load().svsr_enc_gave_up(1 if reset else 0))
    if rc < 0:
        raise _lib.SvsrError("svsr_enc_gave_up could not read the fused encoder's error word (hipMemcpyFromSymbol failed: an earlier HIP error is "
                             "pending on this device, or the library was loaded for another one)")
    return rc == 1


def disable_enc_fused(why: str) -> None:
    """Routes the word-level encoder to the per-layer launch chain for the rest of the process (a cluster wait gave up: the 8 workgroups of a
    sequence were not resident together — a co-tenant kernel holding LDS or compute units, a partitioned device)."""
    global ENC_FUSED, ENC_BWD_FUSED
    import warnings

    if ENC_FUSED or ENC_BWD_FUSED:
        warnings.warn(f"fused encoder disabled: {why}; the encoder runs on the per-layer launch chain (svsr_igemm_fwd / svsr_mha_fwd / "
                      f"svsr_add_ln_fwd ...) from here on", RuntimeWarning, stacklevel=2)
    ENC_FUSED = ENC_BWD_FUSED = False


def enc_fused_ok(D: int, H: int, inter: int, S: int) -> bool:
    return ENC_FUSED and D == 512 and H == 8 and inter == 2048 and 1 <= S <= 32


def enc_fwd(x0: torch.Tensor, layers: Sequence[dict], B: int, S: int, eps: float, seed: Optional[torch.Tensor], p_hidden: float, p_attn: float) -> None:
    """layers: per layer a dict of tensors under the field names of svsr_enc_layer (+ site_probs / site_ao / site_fo ints).
    Up to 8 layers per launch; deeper encoders take several (the last output of one call is the input of the next)."""
    dev = x0.device
    nbytes = int(_lib.load().svsr_enc_fwd_ws_bytes(B))
    key = (str(dev), _stream())
    ws = _ENC_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _SCRATCH_KEEP.append(ws)
        ws = _ENC_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    x = x0
    for i0 in range(0, len(layers), 8):
        chunk = layers[i0: i0 + 8]
        arr = (_EncLayer * len(chunk))()
        for rec, q in zip(arr, chunk):
            for name, _ in _EncLayer._fields_[:25]:
                setattr(rec, name, q[name].data_ptr())
            rec.site_probs, rec.site_ao, rec.site_fo, rec.pad_ = int(q["site_probs"]), int(q["site_ao"]), int(q["site_fo"]), 0
        global _ENC_FUSED_USED
        _ENC_FUSED_USED = True
        _call("svsr_enc_fwd", _p(x), arr, len(chunk), B, S, float(eps), _p(seed), float(p_hidden), float(p_attn), _p(ws), nbytes, _stream(),
              label="k_enc_fwd", flops=float(len(chunk)) * 2.0 * B * S * (4 * 512 * 512 + 2 * 512 * 2048) + float(len(chunk)) * 4.0 * B * 8 * S * S * 64)
        x = chunk[-1]["xout"]


class _EncBwdLayer(ctypes.Structure):
    """svsr_enc_bwd_layer of include/syncvsr_hip.h"""
    _PTRS = ("w2t", "w1t", "wot", "wqkvt", "g1", "g2", "f", "x1", "ao", "xin", "z", "qkv", "probs", "m1", "r1", "m2", "r2",
             "ds2", "df", "dz", "dx1", "ds1", "dao", "dqkv", "dx", "part1", "part2")
    _fields_ = [(n, ctypes.c_void_p) for n in _PTRS] + \
               [("site_probs", ctypes.c_uint), ("site_ao", ctypes.c_uint), ("site_fo", ctypes.c_uint), ("pad_", ctypes.c_uint)]


ENC_BWD_FUSED = os.environ.get("SVSR_ENC_BWD_FUSED", "1") != "0"     # the whole encoder backward as one launch (False: 13 launches per layer)
# tile edge of the ONE grouped weight-gradient launch behind the fused backward (linear_wgrad_group(tile=...)).  Six layers are 1,152 tiles of
# 128 x 128 = 2.25 rounds of two workgroups per CU, at half the staged bytes per FLOP of the 4,608 tiles of 64 x 64 (six rounds of three):
# measured at the benchmark's shapes the wide launch is the faster one; 64 is the other supported value
ENC_WGRAD_TILE = 128
_ENC_BWD_WS: dict = {}


def enc_bwd(dy: torch.Tensor, layers: Sequence[dict], B: int, S: int, seed: Optional[torch.Tensor], p_hidden: float, p_attn: float) -> None:
    """layers (forward order, at most 8): per layer a dict of tensors under the field names of svsr_enc_bwd_layer (+ the three site ints)."""
    if len(layers) > 8:
        raise ValueError("svsr_enc_bwd takes at most 8 layers per launch")
    dev = dy.device
    nbytes = int(_lib.load().svsr_enc_bwd_ws_bytes(B))
    key = (str(dev), _stream())
    ws = _ENC_BWD_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _SCRATCH_KEEP.append(ws)
        ws = _ENC_BWD_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    arr = (_EncBwdLayer * len(layers))()
    for rec, q in zip(arr, layers):
        for name in _EncBwdLayer._PTRS:
            setattr(rec, name, q[name].data_ptr())
        rec.site_probs, rec.site_ao, rec.site_fo, rec.pad_ = int(q["site_probs"]), int(q["site_ao"]), int(q["site_fo"]), 0
    n = len(layers)
    global _ENC_FUSED_USED
    _ENC_FUSED_USED = True
    _call("svsr_enc_bwd", _p(dy), arr, n, B, S, _p(seed), float(p_hidden), float(p_attn), _p(ws), nbytes, _stream(),
          label="k_enc_bwd", flops=float(n) * 2.0 * B * S * (4 * 512 * 512 + 2 * 512 * 2048) + float(n) * 8.0 * B * 8 * S * S * 64)


# -- `type: x-transformers` encoder passes (csrc/xt.hip) ---------------------------------------------
def rmsnorm_fwd(x, g, D: int, eps: float = 1e-8):
    """x bf16 [R][ld] (pad columns zero) -> (y, inv [R])."""
    R, ld = x.shape
    y = torch.empty_like(x)
    inv = torch.empty(R, dtype=torch.float32, device=x.device)
    _call("svsr_rmsnorm_fwd", _p(x), _p(g), _p(y), _p(inv), R, D, ld, float(eps), _stream())
    return y, inv


def rmsnorm_bwd(dy, x, g, inv, dg, D: int, addend=None) -> torch.Tensor:
    R, ld = x.shape
    dx = torch.empty_like(x)
    part = scratch(_query("svsr_rmsnorm_bwd_rows", R)[0] * ld)
    _call("svsr_rmsnorm_bwd", _p(dy), _p(x), _p(g), _p(inv), _p(addend), _p(dx), _p(dg), _p(part), R, D, ld, _stream())
    return dx


def rotary_table(S: int, device, rot: int = 32, theta: float = 10000.0) -> torch.Tensor:
    """fp32 [S][rot]: cos then sin of position * theta^(-2j/rot), computed with the same torch ops as x-transformers' RotaryEmbedding."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, rot, 2).float() / rot))
    freqs = torch.einsum("i,j->ij", torch.arange(S).float(), inv_freq)
    return torch.cat((freqs.cos(), freqs.sin()), dim=-1).contiguous().to(device)


def rotary_(qkv: torch.Tensor, tab: torch.Tensor, S: int, heads_total: int, sign: int = 1) -> None:
    R, ld = qkv.shape
    assert tab.shape == (S, 32) and tab.dtype == torch.float32
    _call("svsr_rotary", _p(qkv), _p(tab), R, S, heads_total, ld, int(sign), _stream())


def geglu_fwd(u: torch.Tensor, I: int, ldy: int, drop=None) -> torch.Tensor:
    R, ldu = u.shape
    y = torch.empty((R, ldy), dtype=BF16, device=u.device)
    _call("svsr_geglu_fwd", _p(u), _p(y), R, I, ldu, ldy, *_drop(drop), _stream())
    return y


def geglu_bwd(dy: torch.Tensor, u: torch.Tensor, I: int, drop=None) -> torch.Tensor:
    R, ldu = u.shape
    du = torch.empty_like(u)
    _call("svsr_geglu_bwd", _p(dy), _p(u), _p(du), R, I, ldu, dy.shape[1], *_drop(drop), _stream())
    return du


def xt_embed_fwd(feats, wmask, cls, B: int, S: int, F: int, D: int, ld: int, drop=None) -> torch.Tensor:
    x0 = torch.empty((B * S, ld), dtype=BF16, device=feats.device)
    _call("svsr_xt_embed_fwd", _p(feats), _p(wmask), _p(cls), _p(x0), B, S, F, D, ld, *_drop(drop), _stream())
    return x0


def xt_embed_bwd(dx0, dcls, B: int, S: int, F: int, D: int, drop=None) -> torch.Tensor:
    dfeats = torch.empty((B * (S - 1), F), dtype=BF16, device=dx0.device)
    _call("svsr_xt_embed_bwd", _p(dx0), _p(dfeats), _p(dcls), B, S, F, D, dx0.shape[1], *_drop(drop), _stream())
    return dfeats


def bias_act_bwd(dy, z, db, *, R: int, N: int, n_valid: int, ld: int, relu: bool = False, gscale: float = 1.0, defer: Optional[list] = None) -> torch.Tensor:
    """db[:n_valid] += column sums of dz, where dz = dy * act'(z) if z is given (returned) else dy; act = GELU from the
    pre-activation z, or (relu=True) ReLU from the saved output z."""
    dz = torch.empty_like(dy) if z is not None else None
    rows = _query("svsr_bias_act_bwd_rows", R, N)[0] if db is not None else 0
    if defer is not None and rows:
        part = torch.empty(rows * N, dtype=torch.float32, device=dy.device)
        _call("svsr_bias_act_bwd_partials", _p(dy), _p(z), _p(dz), _p(db), R, N, n_valid, ld, 2 if relu else 1, float(gscale), _p(part), _stream())
        defer.append((_deferred_colsum(part, rows, N, db, n_valid), part))
        return dz if z is not None else dy
    part = scratch(rows * N) if rows else None
    _call("svsr_bias_act_bwd", _p(dy), _p(z), _p(dz), _p(db), R, N, n_valid, ld, 2 if relu else 1, float(gscale), _p(part), _stream())
    return dz if z is not None else dy


# --------------------------------------------------------------------------------------------------
# losses / metric / optimiser
# --------------------------------------------------------------------------------------------------
def ce_fwd(logits, ld: int, target_idx, target_prob, R: int, V: int, smoothing: float):
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lse = torch.empty(R, dtype=torch.float32, device=dev)
    ldt = 0 if target_prob is None else target_prob.shape[-1]
    _call("svsr_ce_fwd", _p(logits), int(logits.dtype == torch.float32), ld, _p(target_idx), _p(target_prob), ldt, R, V,
          float(smoothing), _p(loss), _p(lse), _p(scratch(R)), _stream())
    return loss, lse


def ce_bwd(logits, ld: int, target_idx, target_prob, R: int, V: int, smoothing: float, lse, gout, dlogits, ldo: int) -> None:
    ldt = 0 if target_prob is None else target_prob.shape[-1]
    _call("svsr_ce_bwd", _p(logits), int(logits.dtype == torch.float32), ld, _p(target_idx), _p(target_prob), ldt, R, V,
          float(smoothing), _p(lse), _p(gout), _p(dlogits), ldo, _stream())


def linear_ce_ok(R: int, K: int, G: int, V: int) -> bool:
    """True when the fused projection + cross-entropy kernels (csrc/audio_head.hip) take this shape."""
    return bool(_lib.load().svsr_linear_ce_ok(R, K, G, V))


def linear_ce_fwd(h: torch.Tensor, w16: torch.Tensor, bias, tok: torch.Tensor, R: int, K: int, G: int, V: int, seq=None):
    """-> (loss, lse [R*G]): mean cross-entropy of (h W^T + bias).reshape(-1, V) against tok, logits never stored (svsr_linear_ce_fwd).
    seq = (S, s0, T): row r reads hidden row (r // T) * S + s0 + r % T."""
    dev = h.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lse = torch.empty(R * G, dtype=torch.float32, device=dev)
    S, s0, T = seq if seq is not None else (0, 0, 0)
    _call("svsr_linear_ce_fwd", _p(h), _p(w16), _p(bias), _p(tok), R, K, G, V, S, s0, T, _p(loss), _p(lse), _p(scratch(R * G)), _stream(),
          label="k_linear_ce", flops=2.0 * R * K * G * V)
    return loss, lse


def linear_ce_bwd(h: torch.Tensor, w16: torch.Tensor, bias, tok: torch.Tensor, R: int, K: int, G: int, V: int, lse: torch.Tensor, gout: torch.Tensor,
                  dlogits: torch.Tensor, seq=None) -> None:
    """dlogits [R][G*V] bf16 = gout / (R*G) * (softmax - onehot), the logits recomputed (svsr_linear_ce_bwd)."""
    S, s0, T = seq if seq is not None else (0, 0, 0)
    _call("svsr_linear_ce_bwd", _p(h), _p(w16), _p(bias), _p(tok), R, K, G, V, S, s0, T, _p(lse), _p(gout), _p(dlogits), _stream(),
          label="k_linear_ce", flops=2.0 * R * K * G * V)


def topk_acc(logits_f32, labels, soft_labels) -> torch.Tensor:
    B, C = logits_f32.shape
    out = torch.empty(2, dtype=torch.float32, device=logits_f32.device)
    _call("svsr_topk_acc", _p(logits_f32), _p(labels), _p(soft_labels), B, C, _p(out), _p(scratch(2 * B)), _stream())
    return out


def grad_sumsq(g: torch.Tensor, opt_state: torch.Tensor) -> None:
    _call("svsr_grad_sumsq", _p(g), g.numel(), _p(opt_state), _stream())


SUMSQ_PARTS = 1024      # partial sums of squares in the optimiser's device state (loss_optim.hip OPT_PARTS)
OPT_STATE_WORDS = 4 + SUMSQ_PARTS               # svsr_adamw_step's device state: {step, skipped, lr_last, gnorm_last}, then the partial sums
ONECYCLE_STATE_WORDS = OPT_STATE_WORDS + 4      # svsr_adamw_onecycle_step's: the same, then {beta1_last, error, 2 reserved words}


def grad_sumsq_parts(g: torch.Tensor, start: int, n: int, opt_state: torch.Tensor, part0: int, nparts: int) -> None:
    """sum of squares of g[start : start + n] into the partial sums [part0, part0 + nparts) (start a multiple of 4 floats)"""
    assert start % 4 == 0
    _call("svsr_grad_sumsq_parts", g.data_ptr() + 4 * start, n, _p(opt_state), part0, nparts, _stream())


# the schedule of svsr_adamw_step / _range: lr under a cosine with linear warm-up (total_steps <= 0: constant), beta1 constant
CosineSchedule = namedtuple("CosineSchedule", "lr beta1 warmup total_steps", defaults=(0, 0))


def adamw(p, g, m, v, shadow, decay_end: int, sched, beta2: float, eps: float, weight_decay: float, max_norm: float, opt_state,
          lo: int = 0, hi: Optional[int] = None, advance: bool = True) -> None:
    """One AdamW update (clip, bias correction, decoupled decay, bf16 shadow) of elements [lo, hi) of the flat buffers; decay_end: absolute end of
    the decayed region; advance: count the step (the last range of a step only).  sched: a CosineSchedule (svsr_adamw_*, opt_state int32
    [OPT_STATE_WORDS]) or onecycle_schedule's dict (svsr_adamw_onecycle_*, [ONECYCLE_STATE_WORDS]).  The whole buffer with advance is the `_step`
    symbol, anything else `_range`.  Nothing is read back: a step that is skipped or past its schedule shows in opt_state_words."""
    onecycle = isinstance(sched, dict)
    assert opt_state.dtype == torch.int32 and opt_state.numel() >= (ONECYCLE_STATE_WORDS if onecycle else OPT_STATE_WORDS)
    n = (p.numel() if hi is None else hi) - lo
    whole = bool(advance) and lo == 0 and n == p.numel()
    ptrs = [None if t is None else t.data_ptr() + t.element_size() * lo for t in (p, g, m, v, shadow)]
    if onecycle:
        name, hp = "svsr_adamw_onecycle", (beta2, eps, weight_decay, max_norm, _onecycle_record(sched))
    else:
        name, hp = "svsr_adamw", (sched.lr, sched.beta1, beta2, eps, weight_decay, max_norm, sched.warmup, sched.total_steps)
    sym, dec, tail = (name + "_step", decay_end, ()) if whole else (name + "_range", min(max(decay_end - lo, 0), n), (int(advance),))
    _call(sym, *ptrs, n, dec, *hp, _p(opt_state), *tail, _stream())


# the four earlier wrappers' names and argument orders, kept for their callers (the kernel-level tests): each IS adamw
def adamw_step(p, g, m, v, shadow, decay_end, lr, betas, eps, weight_decay, max_norm, warmup, total_steps, opt_state):
    adamw(p, g, m, v, shadow, decay_end, CosineSchedule(lr, betas[0], warmup, total_steps), betas[1], eps, weight_decay, max_norm, opt_state)


def adamw_range(p, g, m, v, shadow, lo, hi, decay_end, lr, betas, eps, weight_decay, max_norm, warmup, total_steps, opt_state, advance):
    adamw(p, g, m, v, shadow, decay_end, CosineSchedule(lr, betas[0], warmup, total_steps), betas[1], eps, weight_decay, max_norm, opt_state, lo, hi, advance)


def adamw_onecycle_step(p, g, m, v, shadow, decay_end, beta2, eps, weight_decay, max_norm, sched, opt_state):
    adamw(p, g, m, v, shadow, decay_end, sched, beta2, eps, weight_decay, max_norm, opt_state)


def adamw_onecycle_range(p, g, m, v, shadow, lo, hi, decay_end, beta2, eps, weight_decay, max_norm, sched, opt_state, advance):
    adamw(p, g, m, v, shadow, decay_end, sched, beta2, eps, weight_decay, max_norm, opt_state, lo, hi, advance)


def opt_state_words(opt_state: torch.Tensor) -> dict:
    """The scalar words of the optimiser's device state, read back (synchronises): steps counted, skipped steps, lr and gradient norm of the last
    advancing launch; of the OneCycle layout also that step's beta1 and the error word (0, or 1001 once a step past total_steps was asked for)."""
    raw = opt_state.detach().cpu()
    f = raw.view(torch.float32)
    words = dict(step=int(raw[0]), skipped=int(raw[1]), lr=float(f[2]), gnorm=float(f[3]))
    if raw.numel() >= ONECYCLE_STATE_WORDS:
        words.update(beta1=float(f[OPT_STATE_WORDS]), error=int(raw[OPT_STATE_WORDS + 1]))
    return words


class AdamW:
    """The optimiser of one flat parameter store, apart from whatever steps it: both moments, the device state, the hyper-parameters and the
    schedule (a CosineSchedule or onecycle_schedule's dict).  `store`: the model's ParamStore.  sumsq: the clip's sum of squares of store.grad, all or
    [start, start + n) into partial sums [part0, part0 + nparts).  load_moments: which words of the saved state come back is the step class's format."""

    def __init__(self, store, sched, beta2: float, eps: float, weight_decay: float, max_norm: float):
        self.sched, self.beta2, self.eps, self.weight_decay, self.max_norm = sched, float(beta2), float(eps), float(weight_decay), float(max_norm)
        self.m, self.v = torch.zeros_like(store.flat), torch.zeros_like(store.flat)
        self.opt_state = torch.zeros(ONECYCLE_STATE_WORDS if isinstance(sched, dict) else OPT_STATE_WORDS, dtype=torch.int32, device=store.flat.device)

    def sumsq(self, store, start: int = 0, n: Optional[int] = None, part0: int = 0, nparts: int = SUMSQ_PARTS) -> None:
        if n is None:
            grad_sumsq(store.grad, self.opt_state)
        else:
            grad_sumsq_parts(store.grad, start, n, self.opt_state, part0, nparts)

    def apply(self, store, lo: int = 0, hi: Optional[int] = None, advance: bool = True) -> None:
        adamw(store.flat, store.grad, self.m, self.v, store.w16, store.decay_end, self.sched, self.beta2, self.eps, self.weight_decay,
              self.max_norm, self.opt_state, lo, hi, advance)

    def state(self) -> dict:
        return opt_state_words(self.opt_state)

    def moments(self) -> dict:
        return {"exp_avg": self.m.detach().clone(), "exp_avg_sq": self.v.detach().clone(), "opt_state": self.opt_state.detach().clone()}

    def load_moments(self, sd: dict) -> None:
        if sd["exp_avg"].numel() != self.m.numel():
            raise ValueError("optimiser state belongs to a different parameter layout")
        self.m.copy_(sd["exp_avg"])
        self.v.copy_(sd["exp_avg_sq"])


# -- AdamW under OneCycleLR (svsr_adamw_onecycle_step / _range): the DC-TCN recipe ----------------------------------------------
class _OneCycleRecord(ctypes.Structure):
    """svsr_onecycle_t of include/syncvsr_hip.h: the host record a launch reads the schedule's constants from."""
    _fields_ = [(k, ctypes.c_double) for k in ("max_lr", "initial_lr", "min_lr", "base_momentum", "max_momentum", "pct_start")] + \
               [(k, ctypes.c_int32) for k in ("three_phase", "cos_anneal", "total_steps", "reserved")]


def onecycle_schedule(max_lr: float, total_steps: int, pct_start: float = 0.3, anneal_strategy: str = "cos", three_phase: bool = False,
                      div_factor: float = 25.0, final_div_factor: float = 1e4, base_momentum: float = 0.85, max_momentum: float = 0.95) -> dict:
    """OneCycleLR's constructor arguments (its names and defaults) -> the constants both the kernel and onecycle_values take."""
    if anneal_strategy not in ("cos", "linear"):
        raise ValueError(f"anneal_strategy must be one of 'cos' or 'linear', instead got {anneal_strategy}")
    if not isinstance(total_steps, int) or total_steps <= 0:
        raise ValueError(f"Expected positive integer total_steps, but got {total_steps}")
    pct_start = float(pct_start)
    if pct_start < 0 or pct_start > 1:
        raise ValueError(f"Expected float between 0 and 1 pct_start, but got {pct_start}")
    initial_lr = float(max_lr) / float(div_factor)
    return dict(max_lr=float(max_lr), initial_lr=initial_lr, min_lr=initial_lr / float(final_div_factor), base_momentum=float(base_momentum),
                max_momentum=float(max_momentum), pct_start=pct_start, three_phase=bool(three_phase), cos=anneal_strategy == "cos",
                total_steps=total_steps)


def onecycle_values(step: int, *, max_lr: float, initial_lr: float, min_lr: float, base_momentum: float, max_momentum: float, pct_start: float,
                    three_phase: bool, cos: bool, total_steps: int) -> tuple[float, float]:
    """(learning rate, beta1) of optimiser step `step` (0-based) as OneCycleLR.get_lr computes them at last_epoch = step, in Python
    floats: the host restatement of what k_adamw's OneCycleSched computes on the device (for logging and the tests).  A step past the schedule
    raises ValueError as torch does; a phase of length zero divides by zero as torch does."""
    import math

    if not 0 <= step < total_steps:
        raise ValueError(f"Tried to step {step + 1} times. The specified number of total steps is {total_steps}")
    phases = [(float(pct_start * total_steps) - 1, initial_lr, max_lr, max_momentum, base_momentum)]
    if three_phase:
        phases += [(float(2 * pct_start * total_steps) - 2, max_lr, initial_lr, base_momentum, max_momentum),
                   (total_steps - 1, initial_lr, min_lr, max_momentum, max_momentum)]
    else:
        phases += [(total_steps - 1, max_lr, min_lr, base_momentum, max_momentum)]

    def anneal(start, end, pct):
        if cos:
            return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)
        return (end - start) * pct + start

    start_step = 0.0
    for i, (end_step, lr0, lr1, m0, m1) in enumerate(phases):
        if step <= end_step or i == len(phases) - 1:
            pct = (step - start_step) / (end_step - start_step)
            return anneal(lr0, lr1, pct), anneal(m0, m1, pct)
        start_step = end_step
    raise AssertionError("unreachable")


_ONECYCLE_RECORDS: dict = {}


def _onecycle_record(sched: dict):
    """The host record of a schedule as a ctypes byte array (what a void* argument takes); cached for the life of the process (a recorded
    step list keeps reading it)."""
    key = tuple(sorted(sched.items()))
    rec = _ONECYCLE_RECORDS.get(key)
    if rec is None:
        s = _OneCycleRecord(sched["max_lr"], sched["initial_lr"], sched["min_lr"], sched["base_momentum"], sched["max_momentum"],
                            sched["pct_start"], int(sched["three_phase"]), int(sched["cos"]), int(sched["total_steps"]), 0)
        rec = _ONECYCLE_RECORDS[key] = (ctypes.c_uint8 * ctypes.sizeof(s)).from_buffer_copy(bytes(s))
    return rec


onecycle_state = opt_state_words          # (of a OneCycle optimiser's state: step, skipped, lr, gnorm, beta1, error)


def transpose_shadows_range(w16, dst, table: torch.Tensor, first: int, count: int) -> None:
    """Entries [first, first + count) of the transposed-shadow table (from the bf16 shadow)."""
    if count > 0:
        _call("svsr_transpose_bf16_multi", _p(w16), _p(dst), table.data_ptr() + 32 * first, count, _stream())


def clip_prep(frames_u8: torch.Tensor, params: torch.Tensor, H: int, W: int, mean: float = 0.421, std: float = 0.165) -> torch.Tensor:
    """uint8 clips [B, T, Hs, Ws] + int32 params [B, 5] = (top, left, h, w, flip) -> fp32 [B, 1, T, H, W] (svsr_clip_prep)."""
    B, T, Hs, Ws = frames_u8.shape
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and params.dtype == torch.int32 and params.shape == (B, 5)
    out = torch.empty((B, 1, T, H, W), dtype=torch.float32, device=frames_u8.device)
    _call("svsr_clip_prep", _p(frames_u8), _p(params), _p(out), B, T, Hs, Ws, H, W, float(mean), float(std), _stream())
    return out


def lrs_clip_prep(src_u8: torch.Tensor, off: torch.Tensor, params: torch.Tensor, Tpad: int, H: int, W: int, mean: float = 0.421,
                  std: float = 0.165, tmask: Optional[torch.Tensor] = None, max_blocks: int = 0) -> torch.Tensor:
    """Packed uint8 frames [sum T_b, Hs, Ws] + int32 frame offsets [B + 1] + int32 params [B, 5] = (top, left, h, w, flip) -> fp32
    [B, Tpad, 1, H, W] with frames behind a clip's length 0.0 (svsr_lrs_clip_prep).  tmask: uint8 [B, Tpad], a marked real frame is written as
    (0 - mean) / std.  max_blocks > 0: a grid cap for tests (the result does not depend on it)."""
    B = off.numel() - 1
    assert src_u8.dtype == torch.uint8 and src_u8.dim() == 3 and src_u8.is_contiguous()
    assert off.dtype == torch.int32 and off.is_contiguous() and B >= 1 and params.dtype == torch.int32 and params.shape == (B, 5) and params.is_contiguous()
    assert tmask is None or (tmask.dtype == torch.uint8 and tmask.shape == (B, Tpad) and tmask.is_contiguous())
    out = torch.empty((B, Tpad, 1, H, W), dtype=torch.float32, device=src_u8.device)
    _call("svsr_lrs_clip_prep", _p(src_u8), src_u8.shape[0], _p(off), _p(params), _p(tmask), _p(out), B, int(Tpad), src_u8.shape[1], src_u8.shape[2],
          int(H), int(W), float(mean), float(std), int(max_blocks), _stream(), label="k_lrs_clip_prep", nbytes=float(src_u8.numel() + 4 * out.numel()))
    return out


LRW_CLIP_MAX_FRAMES = 256          # LW_MAXT of csrc/lrw_prep.hip


def _lrw_clip_check(frames_u8: torch.Tensor, params: torch.Tensor, H: int, W: int) -> tuple[int, int, int, int]:
    """The argument errors the two LRW clip kernels share, raised before any launch."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_contiguous():
        raise ValueError("frames_u8 must be a contiguous uint8 tensor [B, T, Hs, Ws]")
    B, T, Hs, Ws = frames_u8.shape
    if params.dtype != torch.int32 or params.shape != (B, 5) or not params.is_contiguous():
        raise ValueError(f"params must be a contiguous int32 tensor [B, 5] = {(B, 5)}")
    if T > LRW_CLIP_MAX_FRAMES:
        raise ValueError(f"clips of {T} frames: the LRW clip kernels take at most {LRW_CLIP_MAX_FRAMES}")
    if B < 1 or T < 1 or min(Hs, Ws, int(H), int(W)) < 1:
        raise ValueError("empty batch, clip or frame")
    return B, T, Hs, Ws


def lrw_clip_sums(frames_u8: torch.Tensor, params: torch.Tensor, H: int, W: int, max_blocks: int = 0) -> torch.Tensor:
    """uint8 clips [B, T, Hs, Ws] + int32 params [B, 5] = (top, left, h, w, flip) -> fp32 [B, T]: the sum over each frame of what clip_prep
    samples in front of Normalize (svsr_lrw_clip_sums; a fixed reduction order, independent of the grid).  max_blocks > 0: a grid cap for
    tests (the result does not depend on it)."""
    B, T, Hs, Ws = _lrw_clip_check(frames_u8, params, H, W)
    out = torch.empty((B, T), dtype=torch.float32, device=frames_u8.device)
    _call("svsr_lrw_clip_sums", _p(frames_u8), _p(params), _p(out), B, T, Hs, Ws, int(H), int(W), int(max_blocks), _stream(),
          label="k_lrw_clip_sums", nbytes=float(frames_u8.numel() + 4 * out.numel()))
    return out


def lrw_clip_mix(frames_u8: torch.Tensor, params: torch.Tensor, frame_src: torch.Tensor, H: int, W: int, runs: Optional[torch.Tensor] = None,
                 frame_sums: Optional[torch.Tensor] = None, replace_with_zero: bool = False, mean: float = 0.421, std: float = 0.165,
                 max_blocks: int = 0) -> torch.Tensor:
    """uint8 clips [B, T, Hs, Ws] + int32 params [B, 5] + int32 frame_src [B, T] (augment.make_plan's map) -> fp32 [B, 1, T, H, W]
    (svsr_lrw_clip_mix): out[b, 0, t] is frame t of clip s = frame_src[b, t] with clip s's crop, flip and time mask, normalised.  runs: int32
    [B, n_mask, 2] = (start, length) per clip in TimeMask's order, or None; a masked frame is the clip's mean as masked so far, derived from
    frame_sums = lrw_clip_sums(...) (or 0 with replace_with_zero, which needs no sums).  max_blocks as in lrw_clip_sums."""
    B, T, Hs, Ws = _lrw_clip_check(frames_u8, params, H, W)
    if frame_src.dtype != torch.int32 or frame_src.shape != (B, T) or not frame_src.is_contiguous():
        raise ValueError(f"frame_src must be a contiguous int32 tensor [B, T] = {(B, T)}")
    n_mask = 0
    if runs is not None:
        if runs.dtype != torch.int32 or runs.dim() != 3 or runs.shape[0] != B or runs.shape[2] != 2 or not runs.is_contiguous():
            raise ValueError("runs must be a contiguous int32 tensor [B, n_mask, 2]")
        n_mask = runs.shape[1]
    if n_mask > 0 and not replace_with_zero:
        if frame_sums is None:
            raise ValueError("mean-filled runs need frame_sums (ops.lrw_clip_sums)")
        if frame_sums.dtype != torch.float32 or frame_sums.shape != (B, T) or not frame_sums.is_contiguous():
            raise ValueError(f"frame_sums must be a contiguous fp32 tensor [B, T] = {(B, T)}")
    out = torch.empty((B, 1, T, H, W), dtype=torch.float32, device=frames_u8.device)
    _call("svsr_lrw_clip_mix", _p(frames_u8), _p(params), _p(frame_src), _p(runs) if n_mask else None, _p(frame_sums) if n_mask else None, _p(out),
          B, T, Hs, Ws, int(H), int(W), n_mask, int(bool(replace_with_zero)), float(mean), float(std), int(max_blocks), _stream(),
          label="k_lrw_clip_mix", nbytes=float(frames_u8.numel() + 4 * out.numel()))
    return out


DCTCN_CLIP_MAX_FRAMES = 256          # DT_MAXT of csrc/dctcn_prep.hip


def _dctcn_clip_check(frames_u8: torch.Tensor) -> tuple[int, int, int, int]:
    """The argument errors the two DC-TCN clip kernels share, raised before any launch."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_contiguous():
        raise ValueError("frames_u8 must be a contiguous uint8 tensor [B, T, Hs, Ws]")
    B, T, Hs, Ws = frames_u8.shape
    if T > DCTCN_CLIP_MAX_FRAMES:
        raise ValueError(f"clips of {T} frames: the DC-TCN clip kernels take at most {DCTCN_CLIP_MAX_FRAMES}")
    if B < 1 or T < 1 or min(Hs, Ws) < 1:
        raise ValueError("empty batch, clip or frame")
    return B, T, Hs, Ws


def dctcn_clip_sums(frames_u8: torch.Tensor, max_blocks: int = 0) -> torch.Tensor:
    """uint8 clips [B, T, Hs, Ws] -> [B, T], the exact integer sum of every stored frame (svsr_dctcn_clip_sums).  The values are uint32,
    held in an int32 tensor: widen and mask with 0xFFFFFFFF to read them on the host (a frame of more than 2^23 bright pixels passes
    2^31).  max_blocks > 0: a grid cap for tests (the result does not depend on it)."""
    B, T, Hs, Ws = _dctcn_clip_check(frames_u8)
    out = torch.empty((B, T), dtype=torch.int32, device=frames_u8.device)
    _call("svsr_dctcn_clip_sums", _p(frames_u8), _p(out), B, T, Hs, Ws, int(max_blocks), _stream(),
          label="k_dctcn_clip_sums", nbytes=float(frames_u8.numel() + 4 * out.numel()))
    return out


def dctcn_clip_mix(frames_u8: torch.Tensor, table: torch.Tensor, H: int, W: int, frame_sums: Optional[torch.Tensor] = None, lam: float = 0.0,
                   mean: float = 0.421, std: float = 0.165, max_blocks: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 clips [B, T, Hs, Ws] + int32 table [B, 9] = (top, left, h, w, flip, shift, trunc, mask_off, mask_len) -> fp32 [B, 1, T, H, W]
    (svsr_dctcn_clip_mix): the reference's DC-TCN scaling, frame mask, trim, crop / flip and Normalize of every clip, mixed with its batch
    neighbour b - 1 at weight lam (0 <= lam <= 0.5; 0: no neighbour is read).  frame_sums = dctcn_clip_sums(frames_u8), or None when no
    clip masks anything (mask runs are then ignored).  out: a contiguous fp32 [B, 1, T, H, W] to write into (any alignment).
    max_blocks as in dctcn_clip_sums."""
    B, T, Hs, Ws = _dctcn_clip_check(frames_u8)
    H, W = int(H), int(W)
    if table.dtype != torch.int32 or table.shape != (B, 9) or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous int32 tensor [B, 9] = {(B, 9)}")
    if frame_sums is not None and (frame_sums.dtype != torch.int32 or frame_sums.shape != (B, T) or not frame_sums.is_contiguous()):
        raise ValueError(f"frame_sums must be what dctcn_clip_sums returns: a contiguous int32 tensor [B, T] = {(B, T)}")
    if min(H, W) < 1:
        raise ValueError("empty batch, clip or frame")
    if not 0.0 <= float(lam) <= 0.5:
        raise ValueError("lam must lie in [0, 0.5]")
    if not float(std) > 0.0:
        raise ValueError("std must be positive")
    if out is None:
        out = torch.empty((B, 1, T, H, W), dtype=torch.float32, device=frames_u8.device)
    elif out.dtype != torch.float32 or out.shape != (B, 1, T, H, W) or not out.is_contiguous() or out.device != frames_u8.device:
        raise ValueError(f"out must be a contiguous fp32 tensor {(B, 1, T, H, W)} on the clips' device")
    _call("svsr_dctcn_clip_mix", _p(frames_u8), _p(table), _p(frame_sums), _p(out), B, T, Hs, Ws, H, W, float(lam), float(mean), float(std),
          int(max_blocks), _stream(), label="k_dctcn_clip_mix", nbytes=float((2 if lam else 1) * frames_u8.numel() + 4 * out.numel()))
    return out


def dctcn_wave_trim(wave: torch.Tensor, table: torch.Tensor, max_blocks: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 waveforms [B, L] + int32 table [B, 2] = (ashift, azero) -> fp32 [B, L]: out[b, i] = wave[b, (i - ashift) mod L] for i < azero,
    0 behind (svsr_dctcn_wave_trim; out of place).  max_blocks as in dctcn_clip_sums."""
    if wave.dtype != torch.float32 or wave.dim() != 2 or not wave.is_contiguous() or wave.numel() == 0:
        raise ValueError("wave must be a contiguous, non-empty fp32 tensor [B, L]")
    B, L = wave.shape
    if table.dtype != torch.int32 or table.shape != (B, 2) or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous int32 tensor [B, 2] = {(B, 2)}")
    if out is None:
        out = torch.empty_like(wave)
    elif out.dtype != torch.float32 or out.shape != wave.shape or not out.is_contiguous() or out.data_ptr() == wave.data_ptr():
        raise ValueError("out must be a contiguous fp32 tensor of wave's shape and must not be wave itself")
    _call("svsr_dctcn_wave_trim", _p(wave), _p(table), _p(out), B, L, int(max_blocks), _stream(), label="k_dctcn_wave_trim",
          nbytes=float(8 * wave.numel()))
    return out


def wave_prep(wave: torch.Tensor, lengths: torch.Tensor, noise: Optional[torch.Tensor] = None, nstart: Optional[torch.Tensor] = None,
              snr_db: Optional[torch.Tensor] = None, eps: float = 1e-8, max_blocks: int = 0) -> torch.Tensor:
    """wave fp32 or int16 [B, Spad] (int16 counts as v / 32768), lengths int32 [B] -> fp32 [B, Spad]: per clip over its real samples,
    noise[nstart[b] : nstart[b] + len] mixed in at snr_db[b] (torchaudio's add_noise; noise=None: no mix), then the layer norm over the
    waveform; samples behind the length are 0.0 (svsr_wave_prep: two launches, partial sums in the per-stream scratch)."""
    B, Spad = wave.shape
    assert wave.dtype in (torch.float32, torch.int16) and wave.is_contiguous() and lengths.dtype == torch.int32 and lengths.numel() == B and lengths.is_contiguous()
    if noise is not None:
        assert noise.dtype == torch.float32 and noise.dim() == 1 and noise.is_contiguous()
        assert nstart.dtype == torch.int32 and nstart.numel() == B and nstart.is_contiguous() and snr_db.dtype == torch.float32 and snr_db.numel() == B and snr_db.is_contiguous()
    out = torch.empty((B, Spad), dtype=torch.float32, device=wave.device)
    ws_bytes = _query("svsr_wave_prep_ws_bytes", B, Spad)[0]
    ws = scratch((ws_bytes + 3) // 4)
    _call("svsr_wave_prep", _p(wave), int(wave.dtype == torch.int16), _p(lengths), _p(noise), 0 if noise is None else noise.numel(),
          _p(nstart) if noise is not None else None, _p(snr_db) if noise is not None else None, _p(out), B, Spad, float(eps), _p(ws), ws_bytes,
          int(max_blocks), _stream(), label="k_wave_prep", nbytes=float(wave.numel() * wave.element_size() * 2 + 4 * out.numel()))
    return out


def cast_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    _call("svsr_cast_bf16", _p(src), _p(dst), src.numel(), _stream())


def transpose_cast_multi(src, dst, table: torch.Tensor, n_entries: int) -> None:
    _call("svsr_transpose_cast_multi", _p(src), _p(dst), _p(table), n_entries, _stream())


def transpose_shadows(flat, w16, dst, table: torch.Tensor, n_entries: int) -> None:
    """Transposed bf16 shadows of the 2-D weights, from the (fresh) bf16 shadow w16: the same bits as from the fp32 buffer `flat`, which
    is not read (half the bytes)."""
    _call("svsr_transpose_bf16_multi", _p(w16), _p(dst), _p(table), n_entries, _stream())


# --------------------------------------------------------------------------------------------------
# LRS: attention, Conformer convolution module, CTC, decoder embedding, label-smoothing loss
# --------------------------------------------------------------------------------------------------
def probs_pitch(Lk: int) -> int:
    return (Lk + 7) // 8 * 8


class MhaLse:
    """What the flash forward keeps for the backward instead of the probabilities: the rows' log-sum-exp, the output and the masks it ran with."""
    __slots__ = ("lse", "ctx", "klen", "causal", "ldp")

    def __init__(self, lse, ctx, klen, causal, ldp):
        self.lse, self.ctx, self.klen, self.causal, self.ldp = lse, ctx, klen, causal, ldp


def mha_fwd(q, q_pitch: int, k, v, kv_pitch: int, *, B: int, H: int, Lq: int, Lk: int, pe=None, bias_u=None, bias_v=None, klen=None,
            causal: bool = False, drop=None, flash: bool = False):
    """-> (ctx [B*Lq, H*64] bf16, probs [B*H, Lq, ldp] bf16).  q/k/v are views into (fused) projection outputs.
    flash=True: svsr_mha_flash_fwd — the second result is an MhaLse record (no probabilities are stored); hand it to mha_bwd."""
    ldp = probs_pitch(Lk)
    ctx = torch.empty((B * Lq, H * 64), dtype=BF16, device=q.device)
    flops = 2.0 * B * H * Lq * Lk * 64 * (3 if pe is not None else 2)
    if flash:
        lse = torch.empty((B * H, Lq), dtype=torch.float32, device=q.device)
        _call("svsr_mha_flash_fwd", _p(q), q_pitch, _p(k), _p(v), kv_pitch, _p(pe), 0 if pe is None else pe.stride(0), _p(bias_u), _p(bias_v),
              _p(klen), int(causal), B, H, 64, Lq, Lk, ldp, 0.125, _p(ctx), H * 64, _p(lse), *_drop(drop), _stream(), label="k_mhaf_fwd", flops=flops)
        return ctx, MhaLse(lse, ctx, klen, bool(causal), ldp)
    probs = torch.empty((B * H, Lq, ldp), dtype=BF16, device=q.device)
    _call("svsr_mha_fwd", _p(q), q_pitch, _p(k), _p(v), kv_pitch, _p(pe), 0 if pe is None else pe.stride(0), _p(bias_u), _p(bias_v),
          _p(klen), int(causal), B, H, 64, Lq, Lk, ldp, 0.125, _p(ctx), H * 64, _p(probs), *_drop(drop), _stream(),
          label="k_mha_fwd", flops=flops)
    return ctx, probs


def mha_pe_transpose(pe: torch.Tensor, H: int, Lq: int) -> torch.Tensor:
    """The transposed position table the query pass of the flash backward reads (mha_bwd(..., pet=...)): it depends on pe alone."""
    nws = int(_lib.load().svsr_mha_flash_ws_bytes(H, Lq))
    ws = torch.empty(nws, dtype=torch.uint8, device=pe.device)
    _call("svsr_mha_pe_transpose", _p(pe), pe.stride(0), H, Lq, _p(ws), nws, _stream())
    return ws


def mha_bwd(dctx, q, q_pitch: int, k, v, kv_pitch: int, probs, *, B: int, H: int, Lq: int, Lk: int, dq, dq_pitch: int, dk, dv,
            dkv_pitch: int, pe=None, bias_u=None, bias_v=None, drop=None, pe_later: bool = False, pet: Optional[torch.Tensor] = None):
    """Writes dq/dk/dv (views with the given pitches).  Relative-position form returns (dq_ac, dq_bd, dpe) as well.
    probs: the forward's second result (the probabilities, or the MhaLse record of a flash forward).
    pe_later (flash + relative positions): a fourth result — (fn, keep): fn() issues the position-table pass that fills dpe on the stream
    current WHEN IT IS CALLED (only the weight gradient of linear_pos reads dpe: the model hands fn to its side stream); keep = the tensors
    that pass reads."""
    rel = pe is not None
    D = H * 64
    dq_ac = torch.empty((B * Lq, D), dtype=BF16, device=q.device) if rel else None
    dq_bd = torch.empty((B * Lq, D), dtype=BF16, device=q.device) if rel else None
    dpe = torch.empty((2 * Lq - 1, D), dtype=BF16, device=q.device) if rel else None
    pe_part = torch.empty((B, 2 * Lq - 1, D), dtype=torch.float32, device=q.device) if rel else None
    flops = 2.0 * B * H * Lq * Lk * 64 * (7 if rel else 4)
    if isinstance(probs, MhaLse):
        rec = probs
        ldp = rec.ldp
        pbuf = torch.empty((B * H, Lq, ldp), dtype=BF16, device=q.device)       # workspace: P and dS of the query pass for the key / table passes
        ds = torch.empty_like(pbuf)
        nws = int(_lib.load().svsr_mha_flash_ws_bytes(H, Lq)) if rel else 0
        have_pet = 4 if (rel and pet is not None) else 0          # (mha_pe_transpose made the table ahead of time)
        ws = pet if have_pet else (torch.empty(nws, dtype=torch.uint8, device=q.device) if nws else None)
        def launch(parts: int, fl: float) -> None:
            _call("svsr_mha_flash_bwd_parts", _p(dctx), dctx.stride(0), _p(rec.ctx), rec.ctx.stride(0), _p(rec.lse), _p(q), q_pitch, _p(k), _p(v), kv_pitch,
                  _p(pe), 0 if pe is None else pe.stride(0), _p(bias_u), _p(bias_v), _p(rec.klen), int(rec.causal), _p(pbuf), _p(ds), B, H, 64, Lq, Lk, ldp,
                  0.125, _p(dq), dq_pitch, _p(dq_ac), _p(dq_bd), D, _p(dk), _p(dv), dkv_pitch, _p(dpe), D, _p(pe_part), _p(ws), nws, *_drop(drop), parts,
                  _stream(), label="k_mhaf_bwd" if parts & 1 else "k_mha_bwd_pe", flops=fl)

        if rel and pe_later:
            launch(1 | have_pet, flops * 6.0 / 7.0)
            return dq_ac, dq_bd, dpe, (lambda: launch(2, flops / 7.0), (ds, q, dpe, pe_part))
        launch(3 | have_pet, flops)
        return dq_ac, dq_bd, dpe
    ldp = probs.shape[-1]
    ds = torch.empty_like(probs)
    _call("svsr_mha_bwd", _p(dctx), dctx.stride(0), _p(q), q_pitch, _p(k), _p(v), kv_pitch, _p(pe), 0 if pe is None else pe.stride(0),
          _p(bias_u), _p(bias_v), _p(probs), _p(ds), B, H, 64, Lq, Lk, ldp, 0.125, _p(dq), dq_pitch, _p(dq_ac), _p(dq_bd), D,
          _p(dk), _p(dv), dkv_pitch, _p(dpe), D, _p(pe_part), *_drop(drop), _stream(), label="k_mha_bwd", flops=flops)
    return dq_ac, dq_bd, dpe


def glu_dwconv_fwd(u, w, bias, want_stats: bool, B: int, T: int, D: int, K: int, out: Optional[torch.Tensor] = None):
    """-> (c [B*T, D] bf16, BatchNorm1d partials (buffer, rows) or None); out: a contiguous [B*T, D] bf16 buffer of the caller's for c"""
    c = torch.empty((B * T, D), dtype=BF16, device=u.device) if out is None else out
    assert c.shape == (B * T, D) and c.dtype == BF16 and c.is_contiguous()
    stats = st = None
    if want_stats:
        rows = _query("svsr_glu_dwconv_fwd_stat_rows", B, T)[0]
        stats = scratch(rows * 2 * D)
        st = (stats, rows)
    _call("svsr_glu_dwconv_fwd", _p(u), _p(w), _p(bias), _p(c), _p(stats), B, T, D, K, _stream())
    return c, st


DW_SPLITS = 96        # workgroups per 64-channel block of svsr_glu_dwconv_bwd: one (clip, 32-frame tile) each at B = 16, T <= 192 (16 splits left a quarter of the CUs idle with several tiles in a row each)


def glu_dwconv_bwd(dc, u, w, dw, dbias, B: int, T: int, D: int, K: int, reduce_later: bool = False, out: Optional[torch.Tensor] = None):
    """-> du; reduce_later: -> (du, (fn, keep)) — fn() issues the fixed-order sum of the partial rows into dw / dbias on the stream current when
    it is called (parameter gradients: the model hands fn to its side stream), keep = the partial rows.  out: a contiguous [B*T, 2D] bf16
    buffer of the caller's for du."""
    du = torch.empty_like(u) if out is None else out
    assert du.shape == (B * T, 2 * D) and du.dtype == BF16 and du.is_contiguous()
    part = torch.empty(DW_SPLITS * D * (K + 1), dtype=torch.float32, device=u.device)

    def launch(parts: int) -> None:
        _call("svsr_glu_dwconv_bwd_parts", _p(dc), _p(u), _p(w), _p(du), _p(dw), _p(dbias), _p(part), DW_SPLITS, B, T, D, K, parts, _stream())

    if reduce_later:
        launch(1)
        return du, (lambda: launch(2), (part,))
    launch(3)
    return du


def lrs_targets(label: torch.Tensor, odim: int, ignore_id: int, eos: int):
    """label int64 [B, L] on the device, ignore_id padding (anywhere in a row: dropped) -> (labels [B, L] with -1, ys_in [B, L+1], ys_out [B, L+1]):
    add_sos_eos in one launch.  A label outside [1, odim) becomes eos and sets the sticky word lrs_target_errors() reads."""
    B, L = label.shape
    label = label.contiguous()
    labels = torch.empty_like(label)
    ys_in = torch.empty((B, L + 1), dtype=torch.int64, device=label.device)
    ys_out = torch.empty_like(ys_in)
    _call("svsr_lrs_targets", _p(label), B, L, odim, ignore_id, eos, _p(labels), _p(ys_in), _p(ys_out), _stream())
    return labels, ys_in, ys_out


def lrs_target_errors(reset: bool = True) -> bool:
    """True if a svsr_lrs_targets launch since the last reset met a label outside [1, odim) (synchronises the device)."""
    rc = int(_lib.load().svsr_lrs_target_errors(1 if reset else 0))
    if rc < 0:
        raise _lib.SvsrError("svsr_lrs_target_errors could not read the error word (an earlier HIP error is pending on this device)")
    return rc == 1


def ctc_fwd(logits, ld: int, labels, ilen, B: int, T: int, V: int):
    """logits fp32 [B*T, ld]; labels int64 [B, Lmax] (-1 padded); ilen int32 [B] -> (loss 0-d, state for ctc_grad)."""
    Lmax = labels.shape[1]
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lse = torch.empty(B * T, dtype=torch.float32, device=dev)
    ab = torch.empty((B, T, 2 * Lmax + 1), dtype=torch.float32, device=dev)
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    _call("svsr_ctc_fwd", _p(logits), ld, _p(labels), Lmax, _p(ilen), B, T, V, _p(lse), _p(ab), _p(nll), _p(loss), _stream())
    return loss, (lse, ab, nll)


def ctc_grad(logits, ld: int, labels, ilen, B: int, T: int, V: int, state, gout, ldo: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> dlogits [B*T, ldo] bf16 (every column written, V.. with zeros); out: a contiguous buffer of the caller's for it"""
    lse, ab, nll = state
    dz = torch.empty((B * T, ldo), dtype=BF16, device=logits.device) if out is None else out
    assert dz.shape == (B * T, ldo) and dz.dtype == BF16 and dz.is_contiguous()
    _call("svsr_ctc_grad", _p(logits), ld, _p(labels), labels.shape[1], _p(ilen), B, T, V, _p(lse), _p(ab), _p(nll), _p(gout), _p(dz), ldo,
          _stream())
    return dz


def ctc_prefix_score(logp: torch.Tensor, r_prev: torch.Tensor, last: torch.Tensor, ids: Optional[torch.Tensor], out_len: int, blank: int,
                     eos: int) -> tuple[torch.Tensor, torch.Tensor]:
    """logp fp32 [T, V], r_prev fp32 [n, T, 2], last int64 [n], ids int64 [n, S] or None (all V labels)
    -> (r_new fp32 [n, S, T, 2], psi fp32 [n, S]).  See svsr_ctc_prefix_score."""
    T, V = logp.shape
    n = r_prev.shape[0]
    assert logp.dtype == torch.float32 and logp.is_contiguous() and r_prev.dtype == torch.float32 and r_prev.shape == (n, T, 2)
    assert r_prev.is_contiguous() and last.dtype == torch.int64 and last.numel() == n
    assert ids is None or (ids.dtype == torch.int64 and ids.is_contiguous() and ids.shape[0] == n)
    S = V if ids is None else ids.shape[1]
    r_new = torch.empty((n, S, T, 2), dtype=torch.float32, device=logp.device)
    psi = torch.empty((n, S), dtype=torch.float32, device=logp.device)
    _call("svsr_ctc_prefix_score", _p(logp), V, _p(r_prev), _p(last), _p(ids), _p(r_new), _p(psi), T, V, n, S, int(out_len), int(blank), int(eos),
          _stream())
    return r_new, psi


def embed_pos_fwd(tok, emb, pe, L: int, D: int, scale: float) -> torch.Tensor:
    R = tok.numel()
    x = torch.empty((R, D), dtype=BF16, device=emb.device)
    _call("svsr_embed_pos_fwd", _p(tok), _p(emb), _p(pe), _p(x), R, L, D, float(scale), _stream())
    return x


def embed_pos_bwd(tok, dx, demb, D: int, scale: float) -> None:
    _call("svsr_embed_pos_bwd", _p(tok), _p(dx), _p(demb), tok.numel(), D, float(scale), _stream())


def ls_loss_fwd(logits, ld: int, target, R: int, V: int, smoothing: float, inv_denom: float):
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lse = torch.empty(R, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.float32, device=dev)
    _call("svsr_ls_loss_fwd", _p(logits), ld, _p(target), R, V, float(smoothing), float(inv_denom), _p(loss), _p(lse), _p(counts),
          _p(scratch(3 * R)), _stream())
    return loss, lse, counts


def ls_loss_bwd(logits, ld: int, target, R: int, V: int, smoothing: float, inv_denom: float, lse, gout, ldo: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> dlogits [R, ldo] bf16 (every column written, V.. with zeros); out: a contiguous buffer of the caller's for it"""
    dz = torch.empty((R, ldo), dtype=BF16, device=logits.device) if out is None else out
    assert dz.shape == (R, ldo) and dz.dtype == BF16 and dz.is_contiguous()
    _call("svsr_ls_loss_bwd", _p(logits), ld, _p(target), R, V, float(smoothing), float(inv_denom), _p(lse), _p(gout), _p(dz), ldo, _stream())
    return dz


def scale_bf16(x: torch.Tensor, alpha: float, drop=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = alpha * dropout(x) (x contiguous; the dropout element index is the position in x)."""
    y = torch.empty_like(x) if out is None else out
    _call("svsr_scale_bf16", _p(x), _p(y), x.numel(), float(alpha), *_drop(drop), _stream())
    return y


# --------------------------------------------------------------------------------------------------
# wav2vec2 audio tokeniser (csrc/w2v_codec.hip)
# --------------------------------------------------------------------------------------------------
def w2v_stats_floats(B: int, F0: int) -> int:
    """fp32 workspace of the GroupNorm partial sums of layer 0 (svsr_w2v_stats_floats)."""
    n = int(_lib.load().svsr_w2v_stats_floats(B, F0))
    if n < 0:
        _lib.check(-n, "svsr_w2v_stats_floats")
    return n


def w2v_conv0(wave: torch.Tensor, B: int, L_in: int, pad: int, w: torch.Tensor, bias, gamma, beta, eps: float, out: torch.Tensor,
              out_rows: int, stats, group: bool) -> None:
    """Layer 0 of the feature encoder: wave fp32 [B][L_in] (+ pad zeros) -> out bf16 [B][out_rows][512] (svsr_w2v_conv0)."""
    F0 = (L_in + pad - 10) // 5 + 1
    _call("svsr_w2v_conv0", _p(wave), B, L_in, pad, _p(w), _p(bias), _p(gamma), _p(beta), float(eps), _p(out), out_rows, _p(stats),
          1 if group else 0, _stream(), label="k_w2v_conv0", flops=2.0 * B * F0 * 512 * 10)


def w2v_norm_gelu(x: torch.Tensor, B: int, F: int, rows: int, gamma, beta, eps: float, stats=None, group: bool = False) -> None:
    """In place: GELU(LayerNorm(512)) of the F valid rows of every clip, or GELU(GroupNorm) of layer 0 from its partial sums (svsr_w2v_norm_gelu)."""
    _call("svsr_w2v_norm_gelu", _p(x), B, F, rows, _p(gamma), _p(beta), float(eps), _p(stats), F if group else 0, 1 if group else 0,
          _stream(), label="k_w2v_norm_gelu")


def w2v_quantize(feat: torch.Tensor, R: int, F: int, keep: int, gamma, beta, eps: float, w16: torch.Tensor, bias: torch.Tensor,
                 tok: torch.Tensor, seed: Optional[torch.Tensor] = None, site: int = 0, logits_out: Optional[torch.Tensor] = None) -> None:
    """feature_projection LayerNorm + weight_proj + per-group argmax (or argmax of logits + Gumbel noise with `seed`) -> tok int64
    [R / F][keep][2] (frames t < keep of every clip of F frames; svsr_w2v_quantize)."""
    _call("svsr_w2v_quantize", _p(feat), R, F, keep, _p(gamma), _p(beta), float(eps), _p(w16), _p(bias), _p(seed), int(site), _p(tok), _p(logits_out),
          _stream(), label="k_w2v_quantize", flops=2.0 * R * 512 * 640)


# vq-wav2vec k-means audio tokeniser (csrc/vq_codec.hip)

def vq_part_floats(B: int, F: int, kind: int) -> int:
    """Floats of a GroupNorm partial-sum buffer for B clips of F frames: kind 0 layers 0-7, kind 1 the projection (svsr_vq_part_floats)."""
    n = int(_lib.load().svsr_vq_part_floats(B, F, kind))
    if n < 0:
        _lib.check(-n, "svsr_vq_part_floats")
    return n


def vq_conv0_stats(wave: torch.Tensor, B: int, L_in: int, pad: int, w: torch.Tensor, part: torch.Tensor) -> None:
    """Layer 0 of the feature extractor, statistics only: wave fp32 [B][L_in] (+ pad zeros) -> partial sums of its GroupNorm (svsr_vq_conv0_stats)."""
    F0 = (L_in + pad - 10) // 5 + 1
    _call("svsr_vq_conv0_stats", _p(wave), B, L_in, pad, _p(w), _p(part), _stream(), label="k_vq_conv0<stats>", flops=2.0 * B * F0 * 512 * 10)


def vq_conv0_apply(wave: torch.Tensor, B: int, L_in: int, pad: int, w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                   part: torch.Tensor, out: torch.Tensor, out_rows: int) -> None:
    """Layer 0 again + GroupNorm(1, 512) + ReLU -> out bf16 [B][out_rows][512] (svsr_vq_conv0_apply)."""
    F0 = (L_in + pad - 10) // 5 + 1
    _call("svsr_vq_conv0_apply", _p(wave), B, L_in, pad, _p(w), _p(gamma), _p(beta), float(eps), _p(part), _p(out), out_rows, _stream(),
          label="k_vq_conv0<apply>", flops=2.0 * B * F0 * 512 * 10)


def vq_gn_partial(x: torch.Tensor, B: int, F: int, rows: int, part: torch.Tensor) -> None:
    """Partial sums of the F valid rows of every clip of x bf16 [B][rows][512] (svsr_vq_gn_partial)."""
    _call("svsr_vq_gn_partial", _p(x), B, F, rows, _p(part), _stream(), label="k_vq_gn_partial")


def vq_gn_relu(x: torch.Tensor, B: int, F: int, rows: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, part: torch.Tensor,
               log: bool = False) -> None:
    """In place over the valid rows: relu(GroupNorm(1, 512)), with log: log(. + 1) on top (svsr_vq_gn_relu)."""
    _call("svsr_vq_gn_relu", _p(x), B, F, rows, _p(gamma), _p(beta), float(eps), _p(part), 1 if log else 0, _stream(), label="k_vq_gn_relu")


def vq_project(x: torch.Tensor, B: int, F: int, w16: torch.Tensor, ze: torch.Tensor, part: torch.Tensor) -> None:
    """The quantiser's grouped projection: x bf16 [B * F][512] -> ze fp32 [B * F][512] + its GroupNorm partial sums (svsr_vq_project)."""
    _call("svsr_vq_project", _p(x), B, F, _p(w16), _p(ze), _p(part), _stream(), label="k_vq_project", flops=2.0 * B * F * 512 * 256)


def vq_assign(ze: torch.Tensor, B: int, F: int, keep: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, part: torch.Tensor,
              emb16: torch.Tensor, e2: torch.Tensor, tok: torch.Tensor, scores_out: Optional[torch.Tensor] = None) -> None:
    """GroupNorm(2, 512) + nearest centroid per group -> tok int64 [B][keep][2] (svsr_vq_assign)."""
    _call("svsr_vq_assign", _p(ze), B, F, keep, _p(gamma), _p(beta), float(eps), _p(part), _p(emb16), _p(e2), _p(tok), _p(scores_out), _stream(),
          label="k_vq_assign", flops=2.0 * B * F * 512 * 320)


# --------------------------------------------------------------------------------------------------
# Transformer language-model scorer (csrc/lrs_lm.hip)
# --------------------------------------------------------------------------------------------------
def mha_table_fwd(pool: torch.Tensor, table: torch.Tensor, *, n: int, Lq: int, L: int, H: int, scale: float, pool_rows: Optional[int] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pool bf16 [rows, pitch >= 3 * H * 64] (q | k | v per row), table int32 [n, >= L] -> ctx bf16 [n * Lq, H * 64]: query positions
    L - Lq .. L - 1 of every hypothesis over the keys its table names (svsr_mha_table_fwd; entry encoding: include/syncvsr_hip.h)."""
    assert pool.dtype == BF16 and pool.dim() == 2 and pool.stride(1) == 1 and table.dtype == torch.int32 and table.dim() == 2 and table.stride(1) == 1
    assert table.shape[0] >= n and table.shape[1] >= L
    rows = pool.shape[0] if pool_rows is None else int(pool_rows)
    assert 0 < rows <= pool.shape[0]
    D = H * 64
    ctx = torch.empty((n * Lq, D), dtype=BF16, device=pool.device) if out is None else out
    _call("svsr_mha_table_fwd", _p(pool), rows, pool.stride(0), _p(table), table.stride(0), n, Lq, L, H, float(scale), _p(ctx), ctx.stride(0), _stream(),
          label="k_mha_table", flops=4.0 * n * Lq * L * D, nbytes=256.0 * n * Lq * H * L)
    return ctx


def lm_embed_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, pe: torch.Tensor, pos: torch.Tensor, D: int, eps: float, scale: float) -> torch.Tensor:
    """x bf16 [R, >= D] -> bf16 [R, D] = relu(LayerNorm(x)) * scale + pe[pos] (svsr_lm_embed_fwd); pe fp32 [rows, D], pos int32 [R]."""
    R = x.shape[0]
    assert x.dtype == BF16 and x.stride(1) == 1 and pe.dtype == torch.float32 and pe.is_contiguous() and pe.shape[1] == D
    assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.numel() == R
    out = torch.empty((R, D), dtype=BF16, device=x.device)
    _call("svsr_lm_embed_fwd", _p(x), x.stride(0), _p(gamma), _p(beta), _p(pe), pe.shape[0], _p(pos), R, D, float(eps), float(scale), _p(out), _stream(),
          label="k_lm_embed")
    return out


# --------------------------------------------------------------------------------------------------
# Recurrent language-model scorer (csrc/lrs_rnnlm.hip)
# --------------------------------------------------------------------------------------------------
def rnn_cell_step(gru: bool, wpk: torch.Tensor, bias: torch.Tensor, x: torch.Tensor, xidx: Optional[torch.Tensor], h_prev: Optional[torch.Tensor],
                  c_prev: Optional[torch.Tensor], src: Optional[torch.Tensor], h_out: torch.Tensor, c_out: Optional[torch.Tensor],
                  h16_out: Optional[torch.Tensor], *, R: int, Ep: int, Up: int, U: int) -> None:
    """One recurrent layer of one step for R hypotheses (svsr_rnn_cell_step; layouts: include/syncvsr_hip.h).  x bf16 [rows, >= Ep]: the embedding
    table with xidx int64 [R] (any stride: a column of the prefixes) = the tokens, or the rows of the layer below with xidx None; h_prev / c_prev
    fp32 [rows, Up] read through src int64 [R] (None: zero state); h_out / c_out fp32 and h16_out bf16 [>= R, Up] are written."""
    assert wpk.dtype == BF16 and wpk.is_contiguous() and wpk.numel() == (3 if gru else 4) * Up * (Ep + Up)
    assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == 4 * Up
    assert x.dtype == BF16 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= Ep and (xidx is not None or x.shape[0] >= R)
    assert xidx is None or (xidx.dtype == torch.int64 and xidx.dim() == 1 and xidx.numel() >= R)
    assert src is None or (src.dtype == torch.int64 and src.is_contiguous() and src.numel() >= R and h_prev is not None)
    for t in (h_prev, c_prev, h_out, c_out):
        assert t is None or (t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] == Up)
    assert h_out.shape[0] >= R and (c_out is None or c_out.shape[0] >= R)
    assert h16_out is None or (h16_out.dtype == BF16 and h16_out.is_contiguous() and h16_out.shape[0] >= R and h16_out.shape[1] == Up)
    G = 3 if gru else 4
    _call("svsr_rnn_cell_step", int(bool(gru)), _p(wpk), _p(bias), _p(x), x.stride(0), x.shape[0], _p(xidx), 1 if xidx is None else max(xidx.stride(0), 1),
          _p(h_prev), _p(c_prev), _p(src), 0 if h_prev is None else h_prev.shape[0], _p(h_out), _p(c_out), _p(h16_out), R, Ep, Up, U, _stream(),
          label="k_rnn_cell", flops=2.0 * R * G * Up * (Ep + Up), nbytes=2.0 * G * Up * (Ep + Up))


# --------------------------------------------------------------------------------------------------
# Multi-clip beam search (csrc/lrs_search.hip)
# --------------------------------------------------------------------------------------------------
BEAM_SELECT_MAX_PLANES = 4


def beam_select_slices(V: int, beam: int, max_rows: int) -> int:
    """Stage-1 workgroups per clip of svsr_beam_select for clips of at most `max_rows` rows; 0: outside the kernel's bounds."""
    return int(_lib.load().svsr_beam_select_slices(int(V), int(beam), int(max_rows)))


def beam_select(planes, weights, run: torch.Tensor, clip_of: torch.Tensor, row_lo: torch.Tensor, out_off: torch.Tensor, *, beam: int, V: int,
                max_rows: int, out_rows: int):
    """The selection step of a multi-clip search (svsr_beam_select): planes fp32 [n, >= V] (up to 4, one row pitch), weights floats, run fp32
    [n], clip_of int32 [n], row_lo int32 [C + 1], out_off int32 [C], max_rows = rows of the largest clip, out_rows = sum_c min(beam, rows_c * V)
    -> (prev int64 [out_rows], tok int64 [out_rows], total fp32 [out_rows], vals fp32 [len(planes), out_rows], clip_out int32 [out_rows],
    count int32 [C]).  Outside the kernel's bounds (include/syncvsr_hip.h) it raises: there is no other path."""
    P = len(planes)
    n, C = run.numel(), row_lo.numel() - 1
    if not 1 <= P <= BEAM_SELECT_MAX_PLANES:
        raise ValueError(f"svsr_beam_select adds up 1 to {BEAM_SELECT_MAX_PLANES} score planes, got {P}")
    ldv = planes[0].stride(0)
    planes = [s if (s.stride(0) == ldv and s.stride(1) == 1) else s.contiguous() for s in planes]
    if any(s.stride(0) != ldv for s in planes):
        planes = [s.contiguous() for s in planes]
        ldv = planes[0].stride(0)
    assert all(s.dtype == torch.float32 and s.dim() == 2 and s.shape[0] == n and s.shape[1] >= V and s.stride(1) == 1 for s in planes)
    assert run.dtype == torch.float32 and run.is_contiguous() and clip_of.dtype == torch.int32 and clip_of.is_contiguous() and clip_of.numel() == n
    assert row_lo.dtype == torch.int32 and row_lo.is_contiguous() and out_off.dtype == torch.int32 and out_off.is_contiguous() and out_off.numel() >= C
    G = beam_select_slices(V, beam, max_rows)
    if G < 1:
        raise ValueError(f"svsr_beam_select cannot rank clips of {max_rows} rows x {V} units at beam {beam}: it needs beam <= 256, rows * V <= 2^20 "
                         "and ceil(rows * V / 4096) * beam <= 4096")
    dev = run.device
    cand = torch.empty(C * G * beam, dtype=torch.int64, device=dev)
    prev = torch.empty(out_rows, dtype=torch.int64, device=dev)
    tok = torch.empty(out_rows, dtype=torch.int64, device=dev)
    total = torch.empty(out_rows, dtype=torch.float32, device=dev)
    vals = torch.empty((P, out_rows), dtype=torch.float32, device=dev)
    clip_out = torch.empty(out_rows, dtype=torch.int32, device=dev)
    count = torch.empty(C, dtype=torch.int32, device=dev)
    ptrs = [_p(s) for s in planes] + [None] * (BEAM_SELECT_MAX_PLANES - P)
    ws = [float(w) for w in weights] + [0.0] * (BEAM_SELECT_MAX_PLANES - P)
    _call("svsr_beam_select", *ptrs, *ws, P, ldv, _p(run), _p(clip_of), _p(row_lo), _p(out_off), n, C, int(V), int(beam), int(max_rows), int(out_rows),
          _p(cand), _p(prev), _p(tok), _p(total), _p(vals), _p(clip_out), _p(count), _stream(), label="k_beam_select",
          nbytes=4.0 * n * V * P)
    return prev, tok, total, vals, clip_out, count


def ctc_prefix_score_clips(logp: torch.Tensor, tlen: torch.Tensor, r_prev: torch.Tensor, last: torch.Tensor, ids: Optional[torch.Tensor],
                           clip_of: torch.Tensor, out_len: int, blank: int, eos: int) -> tuple[torch.Tensor, torch.Tensor]:
    """logp fp32 [C, Tmax, V], tlen int32 [C], r_prev fp32 [n, Tmax, 2], last int64 [n], ids int64 [n, S] or None (all V labels), clip_of
    int32 [n] -> (r_new fp32 [n, S, Tmax, 2], psi fp32 [n, S]).  See svsr_ctc_prefix_score_clips."""
    C, Tmax, V = logp.shape
    n = r_prev.shape[0]
    assert logp.dtype == torch.float32 and logp.is_contiguous() and r_prev.dtype == torch.float32 and r_prev.shape == (n, Tmax, 2)
    assert r_prev.is_contiguous() and last.dtype == torch.int64 and last.is_contiguous() and last.numel() == n
    assert tlen.dtype == torch.int32 and tlen.is_contiguous() and tlen.numel() == C
    assert clip_of.dtype == torch.int32 and clip_of.is_contiguous() and clip_of.numel() == n
    assert ids is None or (ids.dtype == torch.int64 and ids.is_contiguous() and ids.shape[0] == n)
    S = V if ids is None else ids.shape[1]
    r_new = torch.empty((n, S, Tmax, 2), dtype=torch.float32, device=logp.device)
    psi = torch.empty((n, S), dtype=torch.float32, device=logp.device)
    _call("svsr_ctc_prefix_score_clips", _p(logp), V, _p(r_prev), _p(last), _p(ids), _p(clip_of), _p(tlen), _p(r_new), _p(psi), C, Tmax, V, n, S,
          int(out_len), int(blank), int(eos), _stream(), label="k_ctc_prefix_clips")
    return r_new, psi


CTC_ALIGN_MAX_LABELS = 1023      # 2 L + 1 states <= 2048 (csrc/lrs_search.hip CA_MAX_S)


def ctc_align(logp: torch.Tensor, tlen: torch.Tensor, labels: torch.Tensor, blank: int = 0,
              V: Optional[int] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """logp fp32 [B, Tmax, ldp] log-probabilities (V <= ldp: the first V columns are the vocabulary, default all), tlen int32 [B], labels
    int64 [B, Lmax] padded with -1 at the tail -> (frames int32 [B, Tmax], spans int32 [B, Lmax, 2], score fp32 [B]): the best CTC path of
    every clip.  A clip without a path has score -inf and -1 everywhere.  See svsr_ctc_align."""
    B, Tmax, ldp = logp.shape
    V = ldp if V is None else int(V)
    assert logp.dtype == torch.float32 and logp.is_contiguous() and tlen.dtype == torch.int32 and tlen.is_contiguous() and tlen.numel() == B
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.dim() == 2 and labels.shape[0] == B
    Lmax = labels.shape[1]
    dev = logp.device
    bp = torch.empty((B, Tmax, 2 * Lmax + 1), dtype=torch.uint8, device=dev)
    frames = torch.empty((B, Tmax), dtype=torch.int32, device=dev)
    spans = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    _call("svsr_ctc_align", _p(logp), ldp, _p(tlen), _p(labels), Lmax, B, Tmax, V, int(blank), _p(bp), _p(frames), _p(spans), _p(score), _stream(),
          label="k_ctc_align")
    return frames, spans, score


CTC_GREEDY_MAX_FRAMES = 4096     # Tmax of svsr_ctc_collapse: a clip's winners and log-probabilities in LDS (csrc/lrs_search.hip CG_MAX_T)


def ctc_frame_best(logits: torch.Tensor, tlen: torch.Tensor, *, Tmax: int, V: int) -> tuple[torch.Tensor, torch.Tensor]:
    """logits fp32 [C * Tmax, ldp >= V] (the fp32 output of `linear_fwd` for ctc_lo), tlen int32 [C] -> (best int32 [C, Tmax] the column of
    the largest logit of every live frame, -1 behind tlen; best_logp fp32 [C, Tmax] its log-probability, 0 behind tlen).  Columns >= V and
    frames behind tlen are never read.  See svsr_ctc_frame_best."""
    C = tlen.numel()
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == C * Tmax
    assert tlen.dtype == torch.int32 and tlen.is_contiguous()
    best = torch.empty((C, Tmax), dtype=torch.int32, device=logits.device)
    best_logp = torch.empty((C, Tmax), dtype=torch.float32, device=logits.device)
    _call("svsr_ctc_frame_best", _p(logits), logits.stride(0), _p(tlen), C, int(Tmax), int(V), _p(best), _p(best_logp), _stream(),
          label="k_ctc_frame_best", nbytes=4.0 * C * Tmax * V)
    return best, best_logp


def ctc_collapse(best: torch.Tensor, best_logp: torch.Tensor, tlen: torch.Tensor, blank: int = 0, Lcap: Optional[int] = None):
    """best int32 [C, Tmax], best_logp fp32 [C, Tmax], tlen int32 [C] -> (tokens int64 [C, Lcap], spans int32 [C, Lcap, 2], token_logp fp32
    [C, Lcap], ntok int32 [C], score fp32 [C]): runs merged, blanks dropped; rows behind ntok hold -1 / (-1, -1) / 0.  Lcap defaults to Tmax
    (a clip has no more tokens than frames).  Tmax <= CTC_GREEDY_MAX_FRAMES.  See svsr_ctc_collapse."""
    C, Tmax = best.shape
    Lcap = Tmax if Lcap is None else int(Lcap)
    assert best.dtype == torch.int32 and best.is_contiguous() and best_logp.dtype == torch.float32 and best_logp.is_contiguous()
    assert best_logp.shape == best.shape and tlen.dtype == torch.int32 and tlen.is_contiguous() and tlen.numel() == C
    dev = best.device
    rows = max(Lcap, 0)
    tokens = torch.empty((C, rows), dtype=torch.int64, device=dev)
    spans = torch.empty((C, rows, 2), dtype=torch.int32, device=dev)
    token_logp = torch.empty((C, rows), dtype=torch.float32, device=dev)
    ntok = torch.empty(C, dtype=torch.int32, device=dev)
    score = torch.empty(C, dtype=torch.float32, device=dev)
    _call("svsr_ctc_collapse", _p(best), _p(best_logp), _p(tlen), C, Tmax, Lcap, int(blank), _p(tokens), _p(spans), _p(token_logp), _p(ntok),
          _p(score), _stream(), label="k_ctc_collapse")
    return tokens, spans, token_logp, ntok, score


EDIT_MAX_LEN = 1024              # ids per side of svsr_edit_distance: 64 lanes x 16 columns in registers (csrc/lrs_eval.hip ED_MAX_LEN)


def _id_rows(t: torch.Tensor, name: str) -> int:
    """Row stride (in ids) of the int64 rows `t` as svsr_edit_distance takes it.  The kernel cuts a row's length to its stride, so a stride
    wider than the row must lie inside the tensor's storage for the last row too."""
    n, w = t.shape
    if w == 0:
        return 0
    ld = t.stride(0) if n > 1 else w
    assert t.stride(1) == 1 and ld >= w, f"{name}: rows of unit stride, one after the other"
    if ld > w:
        assert t.storage_offset() + n * ld <= t.untyped_storage().nbytes() // 8, f"{name}: the last row's stride runs past the storage"
    return ld


def edit_distance(hyp: torch.Tensor, hyp_len: torch.Tensor, ref: torch.Tensor, ref_len: torch.Tensor) -> torch.Tensor:
    """hyp int64 [N, Lh], hyp_len int32 [N], ref int64 [N, Lr], ref_len int32 [N] -> int32 [N, 4] = (distance, substitutions, deletions,
    insertions) of every pair; hyp_len == ref_len - deletions + insertions.  Rows may be views of wider rows (unit stride along a row);
    nothing behind a row's length is read.  Lh, Lr <= EDIT_MAX_LEN (ValueError, before any launch).  See svsr_edit_distance."""
    assert hyp.dtype == torch.int64 and hyp.dim() == 2 and ref.dtype == torch.int64 and ref.dim() == 2 and ref.shape[0] == hyp.shape[0]
    N = hyp.shape[0]
    assert hyp_len.dtype == torch.int32 and hyp_len.is_contiguous() and hyp_len.numel() == N
    assert ref_len.dtype == torch.int32 and ref_len.is_contiguous() and ref_len.numel() == N
    if hyp.shape[1] > EDIT_MAX_LEN or ref.shape[1] > EDIT_MAX_LEN:
        raise ValueError(f"sequences of more than {EDIT_MAX_LEN} ids are not supported, got rows of {hyp.shape[1]} and {ref.shape[1]}")
    ldh, ldr = _id_rows(hyp, "hyp"), _id_rows(ref, "ref")
    out = torch.empty((N, 4), dtype=torch.int32, device=hyp.device)
    if N == 0:
        return out
    _call("svsr_edit_distance", _p(hyp) if ldh else None, ldh, _p(hyp_len), _p(ref) if ldr else None, ldr, _p(ref_len), N, _p(out), _stream(),
          label="k_edit_distance")
    return out


def mha_src_step_fwd(q: torch.Tensor, kv: torch.Tensor, clip_of: torch.Tensor, tlen: torch.Tensor, *, Tmax: int, H: int,
                     scale: float = 0.125, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q bf16 [n, >= H * 64], kv bf16 [C * Tmax, >= 2 * H * 64] (k | v per row), clip_of int32 [n], tlen int32 [C] -> ctx bf16 [n, H * 64]: row r
    over the tlen[clip_of[r]] source frames of its clip (svsr_mha_src_step_fwd).  out: bf16 [n, H * 64] of any row pitch (a column slice of
    a wider tensor) to write instead of a new tensor."""
    n, C = q.shape[0], tlen.numel()
    assert q.dtype == BF16 and q.dim() == 2 and q.stride(1) == 1 and kv.dtype == BF16 and kv.dim() == 2 and kv.stride(1) == 1
    assert kv.shape[0] == C * Tmax and clip_of.dtype == torch.int32 and clip_of.is_contiguous() and clip_of.numel() == n
    assert tlen.dtype == torch.int32 and tlen.is_contiguous()
    ctx = torch.empty((n, H * 64), dtype=BF16, device=q.device) if out is None else out
    assert ctx.dtype == BF16 and ctx.shape == (n, H * 64) and ctx.stride(1) == 1
    _call("svsr_mha_src_step_fwd", _p(q), q.stride(0), _p(kv), kv.stride(0), _p(clip_of), _p(tlen), C, int(Tmax), n, H, float(scale), _p(ctx),
          ctx.stride(0), _stream(), label="k_mha_src_step", flops=4.0 * n * Tmax * H * 64, nbytes=256.0 * n * H * Tmax)
    return ctx


# --------------------------------------------------------------------------------------------------
# Dense temporal back-end of the DC-TCN model (csrc/dctcn.hip)
# --------------------------------------------------------------------------------------------------
ACT_PRELU = 3
TCONV_MAX_HALO = 16      # (k - 1) * d / 2 rows of the same clip on either side of a time tile (csrc/dctcn.hip TC_HALO)


def tconv_ok(n_in: int, co: int, k: int, d: int) -> bool:
    """The shapes svsr_tconv_fwd takes (anything else is SVSR_ERR_ARG there)."""
    return n_in >= 64 and n_in % 64 == 0 and co >= 64 and co % 64 == 0 and k in (1, 3, 5, 7) and d >= 1 and (k - 1) * d // 2 <= TCONV_MAX_HALO


def _rows_view(t: torch.Tensor, rows: int, width: int, dtype) -> None:
    if not (t.dtype == dtype and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= rows and t.shape[1] >= width):
        raise ValueError(f"expected a {dtype} [>= {rows}, >= {width}] row tensor with unit channel stride, got {tuple(t.shape)} {t.dtype}")


def _packed(t: Optional[torch.Tensor], dtype, shape=None, numel: Optional[int] = None, optional: bool = False) -> None:
    """A contiguous tensor of `dtype` with exactly `shape`, or (shape None) exactly `numel` elements; optional: None passes."""
    if t is None and optional:
        return
    if not (t.dtype == dtype and t.is_contiguous() and (tuple(t.shape) == tuple(shape) if shape is not None else t.numel() == numel)):
        raise ValueError(f"expected a contiguous {dtype} tensor of {'shape ' + str(tuple(shape)) if shape is not None else str(numel) + ' elements'}, "
                         f"got {tuple(t.shape)} {t.dtype}")


def _host_table(rows) -> torch.Tensor:
    """The host int64 table a launch reads during the call: the caller holds the result until the call has returned.  A recorded step list
    re-reads it at every replay, so inside a recording the recorder owns it too (StepRecorder.keep)."""
    tab = torch.tensor(rows, dtype=torch.int64)
    if _REC is not None:
        _REC.keep.append(tab)
    return tab


def _tconv_table(branches: Sequence[dict], B: int, n_in: int, co: int, out: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> list:
    """The per-branch operand checks and host table rows of svsr_tconv_fwd: {k, w, gate, scale, shift, slope, out_off, res_off}.  Without
    out (svsr_tconv_fwd_ext: no epilogue) only k, w and gate are read and the other words stay zero."""
    rows = []
    for br in branches:
        w, k, g = br["w"], int(br["k"]), br.get("gate")
        _packed(w, BF16, (co, k, n_in))
        _packed(g, torch.float32, (B, n_in), optional=True)
        if out is None:
            rows.append((k, _p(w), _p(g) or 0, 0, 0, 0, 0, 0))
            continue
        for n in ("scale", "shift", "slope"):
            _packed(br.get(n), torch.float32, numel=co, optional=True)
        off, roff = int(br["out_off"]), int(br.get("res_off", 0))
        if not (0 <= off and off + co <= out.shape[1] and (res is None or (0 <= roff and roff + co <= res.shape[1]))):
            raise ValueError(f"tconv_fwd: channels [{off}, {off + co}) / [{roff}, {roff + co}) lie outside the output / residual rows")
        rows.append((k, _p(w), _p(g) or 0, _p(br["scale"]), _p(br["shift"]), _p(br.get("slope")) or 0, off, roff))
    return rows


def tconv_fwd(x: torch.Tensor, *, B: int, T: int, n_in: int, d: int, branches: Sequence[dict], co: int, act: int, out: torch.Tensor,
              res: Optional[torch.Tensor] = None, res_act: int = ACT_NONE, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Up to three dilated temporal convolutions of the rows x bf16 [B*T, pitch >= n_in] in one launch (svsr_tconv_fwd).  Each branch is a dict
    k, w (bf16 [co, k, n_in]), scale / shift (fp32 [co]), out_off, and optionally gate (fp32 [B, n_in]), slope (fp32 [co], PReLU), res_off.
    out bf16 [B*T, pitch]: channels [out_off, out_off + co) of every row are written, nothing else.  With acc (fp32 [B*T, >= nb * co]) the
    kernel's saving instantiation runs (svsr_tconv_fwd_save): the same output bits, and the fp32 accumulators of branch i at channels
    [i * co, (i + 1) * co) of acc — what the backward of the back-end reads."""
    _rows_view(x, B * T, n_in, BF16)
    _rows_view(out, B * T, 0, BF16)
    if acc is not None:
        _rows_view(acc, B * T, len(branches) * co, torch.float32)
    if res is not None:
        _rows_view(res, B * T, 0, BF16)
    rows = _tconv_table(branches, B, n_in, co, out, res)
    flops = sum(2.0 * B * T * n_in * r[0] * co for r in rows)
    tab = _host_table(rows)
    head = (_p(x), x.stride(0), B, T, n_in, int(d), len(branches), tab.data_ptr(), co, int(act), _p(out), out.stride(0), _p(res),
            0 if res is None else res.stride(0), int(res_act))
    if acc is None:
        _call("svsr_tconv_fwd", *head, _stream(), label="k_tconv", flops=flops)
    else:
        _call("svsr_tconv_fwd_save", *head, _p(acc), acc.stride(0), _stream(), label="k_tconv<save>", flops=flops)
    return out


def tcn_se_fwd(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, *, B: int, T: int, n_in: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x bf16 [B*T, pitch >= n_in], w1 bf16 [nb, R, n_in], w2 bf16 [nb, n_in, R] -> gate fp32 [nb, B, n_in] = sigmoid(W2 swish(W1 mean_t x))
    (svsr_tcn_se_fwd): the time mean once, the nb gates of a layer in one launch."""
    nb, R = w1.shape[0], w1.shape[1]
    _rows_view(x, B * T, n_in, BF16)
    _packed(w1, BF16, (nb, R, n_in))
    _packed(w2, BF16, (nb, n_in, R))
    gate = torch.empty((nb, B, n_in), dtype=torch.float32, device=x.device) if out is None else out
    _packed(gate, torch.float32, (nb, B, n_in))
    _call("svsr_tcn_se_fwd", _p(x), x.stride(0), B, T, n_in, R, nb, _p(w1), _p(w2), _p(gate), _stream(), label="k_tcn_se")
    return gate


def tcn_norm_pool_fwd(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, mask: torch.Tensor, *, B: int, T: int, C: int):
    """x bf16 [B*T, pitch >= C], mask fp32 [B, T] -> (h bf16 [B*T, C] = x * scale + shift, pooled bf16 [B, C] = masked mean of h over time)
    (svsr_tcn_norm_pool_fwd)."""
    _rows_view(x, B * T, C, BF16)
    _packed(mask, torch.float32, numel=B * T)
    for t in (scale, shift):
        _packed(t, torch.float32, numel=C)
    h = torch.empty((B * T, C), dtype=BF16, device=x.device)
    pooled = torch.empty((B, C), dtype=BF16, device=x.device)
    _call("svsr_tcn_norm_pool_fwd", _p(x), x.stride(0), B, T, C, _p(scale), _p(shift), _p(mask), _p(h), _p(pooled), _stream(), label="k_tcn_norm_pool")
    return h, pooled


# -- backward of the back-end (statistics mode of the forward: running-statistic BatchNorm, no dropout) ------------------------------
def tconv_epi_bwd(dy: torch.Tensor, acc: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, *, rows: int, C: int, act: int,
                  slope: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, res_act: int = ACT_NONE,
                  dacc: Optional[torch.Tensor] = None, dres: Optional[torch.Tensor] = None):
    """Epilogue backward (svsr_tconv_epi_bwd).  dy bf16 [rows, C] (a channel slice of a wider row tensor is fine), acc fp32 [rows, C], scale /
    shift fp32 [C] -> (dacc bf16 [rows, C], dres bf16 [rows, C] or None, sums fp32 [4, C] = sum g, sum g * acc, sum du * min(z, 0), sum du)."""
    if C < 64 or C % 64:
        raise ValueError("tconv_epi_bwd: the channel count must be a multiple of 64")
    _rows_view(dy, rows, C, BF16)
    _rows_view(acc, rows, C, torch.float32)
    for t in (scale, shift, slope):
        _packed(t, torch.float32, numel=C, optional=True)
    dev = dy.device
    if dacc is None:
        dacc = torch.empty((rows, C), dtype=BF16, device=dev)
    _rows_view(dacc, rows, C, BF16)
    if res is not None:
        _rows_view(res, rows, C, BF16)
        if dres is None:
            dres = torch.empty((rows, C), dtype=BF16, device=dev)
        _rows_view(dres, rows, C, BF16)
    part = torch.empty(((rows + 63) // 64) * 4 * C, dtype=torch.float32, device=dev)
    sums = torch.empty((4, C), dtype=torch.float32, device=dev)
    _call("svsr_tconv_epi_bwd", _p(dy), dy.stride(0), _p(acc), acc.stride(0), rows, C, int(act), _p(scale), _p(shift), _p(slope), _p(res),
          0 if res is None else res.stride(0), int(res_act), _p(dacc), dacc.stride(0), _p(dres) if res is not None else None,
          0 if res is None else dres.stride(0), _p(part), _p(sums), _stream(), label="k_tconv_epi_bwd")
    return dacc, (dres if res is not None else None), sums


def tconv_dgrad(dy: torch.Tensor, *, B: int, T: int, co: int, d: int, branches: Sequence[dict], n_out: int, out: torch.Tensor,
                x: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None, cadd: Optional[torch.Tensor] = None,
                cadd_scale: float = 1.0, hmax: Optional[int] = None) -> Optional[torch.Tensor]:
    """Data gradient of up to three branches in one launch (svsr_tconv_dgrad).  Each branch: k, wt (bf16 [n_out, k, co], transposed and tap-flipped:
    tconv_wt), dy_off, optionally gate (fp32 [B, n_out]).  out bf16 [B*T, >= n_out] = addend + cadd[b] * cadd_scale + sum gate_i * dxg_i.
    -> the gate partials fp32 [nb, B, tiles, n_out] if any branch is gated (x, the forward's input rows, is required then), else None.
    hmax None (a running-statistic stage's record): svsr_tconv_dgrad.  hmax given (svsr_tconv_dgrad_ext; 0 is the plain launch through that
    entry): dy is the gradient of the extended accumulators, bf16 [B * (T + 2 * hmax), .] (tconv_bn_bwd)."""
    rows, ext, hmax = B * T, hmax is not None, int(hmax or 0)
    for br in branches:
        if not tconv_ok(co, n_out, int(br["k"]), int(d)):
            raise ValueError("tconv_dgrad: outside the shape domain of svsr_tconv_fwd (channels a multiple of 64, odd k <= 7, (k - 1) d / 2 <= 16)")
    _rows_view(out, rows, n_out, BF16)
    gated = any(br.get("gate") is not None for br in branches)
    if gated:
        if x is None:
            raise ValueError("tconv_dgrad: gated branches need x, the rows the forward multiplied")
        _rows_view(x, rows, n_out, BF16)
    if addend is not None:
        _rows_view(addend, rows, n_out, BF16)
    _rows_view(dy, B * (T + 2 * hmax), 0, BF16)
    _packed(cadd, torch.float32, (B, n_out), optional=True)
    tab_rows = []
    for br in branches:
        k, wt, off, g = int(br["k"]), br["wt"], int(br["dy_off"]), br.get("gate")
        _packed(wt, BF16, (n_out, k, co))
        if not (0 <= off and off + co <= dy.shape[1]):
            raise ValueError(f"tconv_dgrad: channels [{off}, {off + co}) lie outside the gradient rows")
        _packed(g, torch.float32, (B, n_out), optional=True)
        tab_rows.append((k, _p(wt), _p(g) or 0, off))
    gpart = torch.empty((len(branches), B, (T + 31) // 32, n_out), dtype=torch.float32, device=dy.device) if gated else None
    tab = _host_table(tab_rows)
    head = (_p(dy), dy.stride(0), B, T, co, int(d), len(branches), tab.data_ptr(), n_out, _p(x), 0 if x is None else x.stride(0), _p(addend),
            0 if addend is None else addend.stride(0), _p(cadd), float(cadd_scale), _p(out), out.stride(0), _p(gpart))
    flops = sum(2.0 * rows * n_out * r[0] * co for r in tab_rows)
    if ext:
        _call("svsr_tconv_dgrad_ext", *head, hmax, _stream(), label="k_tconv_dgrad", flops=flops)
    else:
        _call("svsr_tconv_dgrad", *head, _stream(), label="k_tconv_dgrad", flops=flops)
    return gpart


def tconv_wt(w16: torch.Tensor) -> torch.Tensor:
    """bf16 Conv1d weight in the parameter's layout [co, ci, k] -> the data-gradient shadow [ci, k, co] with the taps flipped."""
    return w16.permute(1, 2, 0).flip(1).contiguous()


def tconv_wgrad_splits(B: int, T: int, n_in: int, co: int) -> int:
    """Row splits of svsr_tconv_wgrad: enough workgroups for ~2 per compute unit of a 256-CU device, at most 8 and at most the slot pairs
    (a fixed function of the shape: the summation order does not depend on the device)."""
    pairs = (B * ((T + 31) // 32) + 1) // 2
    return max(1, min(pairs, 8, -(-512 // ((n_in // 64) * (co // 64)))))


def tconv_wgrad(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, *, B: int, T: int, n_in: int, co: int, k: int, d: int,
                gate: Optional[torch.Tensor] = None, add: bool = False, splits: Optional[int] = None, hmax: Optional[int] = None) -> None:
    """dw fp32 [co, n_valid <= n_in, k] (contiguous, the parameter's layout) = (add ? dw : 0) + sum_rows dy^T (x) shifted bf16(x * gate)
    (svsr_tconv_wgrad).  x bf16 [B*T, >= n_in], dy bf16 [B*T, >= co] (the branch's channel slice).  hmax given (svsr_tconv_wgrad_ext; 0 is the plain launch): dy is the
    gradient of the extended accumulators, bf16 [B * (T + 2 * hmax), >= co], and the sum runs over all of its rows."""
    if not tconv_ok(n_in, co, int(k), int(d)):
        raise ValueError("tconv_wgrad: outside the shape domain of svsr_tconv_fwd (channels a multiple of 64, odd k <= 7, (k - 1) d / 2 <= 16)")
    rows, ext, hmax = B * T, hmax is not None, int(hmax or 0)
    _rows_view(x, rows, n_in, BF16)
    _rows_view(dy, B * (T + 2 * hmax), co, BF16)
    if not (dw.dtype == torch.float32 and dw.is_contiguous() and dw.dim() == 3 and dw.shape[0] == co and dw.shape[2] == k and 1 <= dw.shape[1] <= n_in):
        raise ValueError(f"tconv_wgrad: dw must be a contiguous fp32 [co, <= n_in, k] tensor, got {tuple(dw.shape)}")
    _packed(gate, torch.float32, (B, n_in), optional=True)
    S = tconv_wgrad_splits(B, T + 2 * hmax, n_in, co) if splits is None else int(splits)
    part = torch.empty(S * co * k * n_in, dtype=torch.float32, device=x.device)
    head = (_p(x), x.stride(0), _p(gate), _p(dy), dy.stride(0), B, T, n_in, co, int(k), int(d), S, _p(part), _p(dw), dw.shape[1], int(bool(add)))
    if ext:
        _call("svsr_tconv_wgrad_ext", *head, hmax, _stream(), label=f"k_tconv_wgrad<{k}>", flops=2.0 * B * (T + 2 * hmax) * n_in * k * co)
    else:
        _call("svsr_tconv_wgrad", *head, _stream(), label=f"k_tconv_wgrad<{k}>", flops=2.0 * rows * n_in * k * co)


def tcn_se_bwd(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, gate: torch.Tensor, gpart: torch.Tensor, dw1: Sequence[torch.Tensor],
               dw2: Sequence[torch.Tensor], *, B: int, T: int, n_in: int, add: bool = False) -> torch.Tensor:
    """Squeeze-and-excitation backward (svsr_tcn_se_bwd): gate partials of tconv_dgrad -> dm fp32 [B, n_in] (gradient of the time mean over
    all branches) and the weight gradients dw1[i] fp32 [R, n_in], dw2[i] fp32 [n_in, R] written (add: added to)."""
    nb, R = w1.shape[0], w1.shape[1]
    _rows_view(x, B * T, n_in, BF16)
    _packed(w1, BF16, (nb, R, n_in))
    _packed(w2, BF16, (nb, n_in, R))
    _packed(gate, torch.float32, (nb, B, n_in))
    _packed(gpart, torch.float32, (nb, B, (T + 31) // 32, n_in))
    if 2 * (3 * n_in + 2 * R) * 4 > 64 * 1024:
        raise ValueError("tcn_se_bwd: n_in too wide for the workgroup's LDS (2 clips x (3 n_in + 2 R) floats <= 64 KiB)")
    if not (len(dw1) == nb and len(dw2) == nb):
        raise ValueError(f"tcn_se_bwd: one dw1 and one dw2 per branch ({nb}), got {len(dw1)} and {len(dw2)}")
    for t in (*dw1, *dw2):
        _packed(t, torch.float32, numel=R * n_in)
    dev = x.device
    work = torch.empty(nb * B * n_in + 2 * nb * B * R + B * n_in, dtype=torch.float32, device=dev)
    dm = torch.empty((B, n_in), dtype=torch.float32, device=dev)
    tab = _host_table([_p(t) for t in dw1] + [_p(t) for t in dw2])
    _call("svsr_tcn_se_bwd", _p(x), x.stride(0), B, T, n_in, R, nb, _p(w1), _p(w2), _p(gate), _p(gpart), _p(work), _p(dm), tab.data_ptr(),
          int(bool(add)), _stream(), label="k_tcn_se_bwd")
    return dm


def _norm_pool_bwd_args(what: str, dh, dpooled, x, out, mask, vecs, B: int, T: int, C: int) -> None:
    if C < 8 or C % 8:
        raise ValueError(f"{what}: C must be a multiple of 8")
    _packed(dh, BF16, (B * T, C))
    _packed(dpooled, BF16, (B, C))
    _rows_view(x, B * T, C, BF16)
    _rows_view(out, B * T, C, BF16)
    _packed(mask, torch.float32, numel=B * T)
    for t in vecs:
        _packed(t, torch.float32, numel=C)


def tcn_norm_pool_bwd(dh: torch.Tensor, dpooled: torch.Tensor, x: torch.Tensor, scale: torch.Tensor, mask: torch.Tensor, *, B: int, T: int, C: int,
                      out: torch.Tensor):
    """norm5 + masked mean backward (svsr_tcn_norm_pool_bwd): dh bf16 [B*T, C], dpooled bf16 [B, C], x bf16 [B*T, >= C] (the forward's input)
    -> out bf16 [B*T, >= C] channels [0, C) written, sums fp32 [2, C] = (sum g, sum g * x)."""
    _norm_pool_bwd_args("tcn_norm_pool_bwd", dh, dpooled, x, out, mask, (scale,), B, T, C)
    part = torch.empty(B * 2 * C, dtype=torch.float32, device=dh.device)
    sums = torch.empty((2, C), dtype=torch.float32, device=dh.device)
    _call("svsr_tcn_norm_pool_bwd", _p(dh), _p(dpooled), _p(x), x.stride(0), B, T, C, _p(scale), _p(mask), _p(out), out.stride(0), _p(part), _p(sums),
          _stream(), label="k_tcn_norm_pool_bwd")
    return out, sums


def bn_conv_param_grads(sum_g: torch.Tensor, sum_g_acc: torch.Tensor, weight: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor,
                        conv_bias: Optional[torch.Tensor], eps: float = BN_EPS):
    """The O(C) chain rule of y = BatchNorm1d(eval)(acc + conv_bias) from the per-channel sums of g = dL/dy and g * acc:
    -> (d bn.weight, d bn.bias, d conv.bias or None).  scale = weight * r is never divided by: a BatchNorm weight of 0 is exact."""
    r = torch.rsqrt(running_var + eps)
    off = -running_mean if conv_bias is None else conv_bias - running_mean
    d_weight = r * (sum_g_acc + off * sum_g)
    d_cbias = None if conv_bias is None else sum_g * (weight * r)
    return d_weight, sum_g, d_cbias


# -- batch-statistic stages of the back-end (loss_and_backend_grads(train_stats=True)) ---------------------------------------------
# The extended axis: hs[i] = (k_i - 1) * d / 2 per branch, hmax >= max(hs); a clip owns T + 2 * hmax rows, time t is row t + hmax, branch i
# (channels [i * co, (i + 1) * co)) owns the rows [hmax - hs[i], hmax + hs[i] + T): the positions the reference's BatchNorm1d sees before the chomp.
def tconv_halos(ks: Sequence[int], d: int) -> list:
    return [(int(k) - 1) * int(d) // 2 for k in ks]


def _int_table(vals) -> torch.Tensor:
    tab = torch.tensor([int(v) for v in vals], dtype=torch.int32)
    if _REC is not None:
        _REC.keep.append(tab)
    return tab


def _ext_geo(B: int, T: int, co: int, hmax: int, hs: Sequence[int]):
    hs = [int(h) for h in hs]
    if not (1 <= len(hs) <= 3 and 0 <= int(hmax) <= TCONV_MAX_HALO and all(0 <= h <= hmax for h in hs) and co >= 64 and co % 64 == 0):
        raise ValueError(f"extended axis: one to three branches of a multiple of 64 channels with 0 <= h <= hmax <= {TCONV_MAX_HALO}, got {hs}, {hmax}, {co}")
    return hs, len(hs) * co, B * (T + 2 * int(hmax))


def tconv_fwd_ext(x: torch.Tensor, *, B: int, T: int, n_in: int, d: int, branches: Sequence[dict], co: int, hmax: Optional[int] = None,
                  acc: Optional[torch.Tensor] = None):
    """The convolutions of tconv_fwd at every position the reference's BatchNorm1d sees (svsr_tconv_fwd_ext): branches hold k, w and optionally
    gate.  -> (acc fp32 [B * (T + 2 * hmax), nb * co], hmax, hs).  Rows of a branch's channels outside its own extent are not written."""
    hs = tconv_halos([br["k"] for br in branches], d)
    hmax = max(hs) if hmax is None else int(hmax)
    hs, C, erows = _ext_geo(B, T, co, hmax, hs)
    _rows_view(x, B * T, n_in, BF16)
    if acc is None:
        acc = torch.empty((erows, C), dtype=torch.float32, device=x.device)
    _rows_view(acc, erows, C, torch.float32)
    if not all(tconv_ok(n_in, co, int(br["k"]), int(d)) for br in branches):
        raise ValueError("tconv_fwd_ext: outside the shape domain of svsr_tconv_fwd")
    rows = _tconv_table(branches, B, n_in, co)
    tab = _host_table(rows)
    _call("svsr_tconv_fwd_ext", _p(x), x.stride(0), B, T, n_in, int(d), len(branches), tab.data_ptr(), co, hmax, _p(acc), acc.stride(0), _stream(),
          label="k_tconv<ext>", flops=sum(2.0 * B * (T + 2 * h) * n_in * r[0] * co for r, h in zip(rows, hs)))
    return acc, hmax, hs


def tcn_colstats(x: torch.Tensor, *, B: int, T: int, co: int, hmax: int = 0, hs: Sequence[int] = (0,)) -> torch.Tensor:
    """Per channel (mean, sum (x - mean)^2) over the B * (T + 2 * hs[i]) own rows of every branch (svsr_tcn_colstats): x fp32 (the extended
    accumulators) or bf16 (an activation stack: hmax = 0) [B * (T + 2 * hmax), >= nb * co] -> stats fp32 [2, nb * co]."""
    hs, C, erows = _ext_geo(B, T, co, hmax, hs)
    if x.dtype not in (torch.float32, BF16):
        raise ValueError("tcn_colstats: fp32 or bf16 rows")
    _rows_view(x, erows, C, x.dtype)
    part = torch.empty(B * 2 * C, dtype=torch.float32, device=x.device)
    stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
    tab = _int_table(hs)
    _call("svsr_tcn_colstats", _p(x), x.stride(0), int(x.dtype == BF16), B, T, C, co, int(hmax), len(hs), tab.data_ptr(), _p(part), _p(stats), _stream(),
          label="k_tcn_colstats")
    return stats


def _epi_args(acc, scale, shift, slope, res, B, T, co, hmax, hs, act, res_act, drop):
    hs, C, erows = _ext_geo(B, T, co, hmax, hs)
    _rows_view(acc, erows, C, torch.float32)
    for t in (scale, shift):
        _packed(t, torch.float32, numel=C)
    _packed(slope, torch.float32, numel=C, optional=True)
    if res is not None:
        _rows_view(res, B * T, C, BF16)
    key, p = (0, 0.0) if drop is None else (int(drop[0]) & 0xFFFFFFFF, float(drop[1]))
    tab = _int_table(hs)
    return C, erows, tab, (_p(acc), acc.stride(0), B, T, C, co, int(hmax), len(hs), tab.data_ptr(), int(act), _p(scale), _p(shift), _p(slope), _p(res),
                           0 if res is None else res.stride(0), int(res_act), key, p)


def tconv_apply(acc: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, *, B: int, T: int, co: int, hmax: int, hs: Sequence[int], act: int,
                out: torch.Tensor, slope: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, res_act: int = ACT_NONE,
                drop: Optional[tuple] = None) -> torch.Tensor:
    """The epilogue of a batch-statistic stage over the T interior rows (svsr_tconv_apply): out bf16 [B*T, >= C] channels [0, C) =
    res_act(dropout(act(fma(acc, scale, shift))) + res).  drop = (key, p): dropout.site_key(seed, site) and the probability."""
    C, _, tab, head = _epi_args(acc, scale, shift, slope, res, B, T, co, hmax, hs, act, res_act, drop)
    _rows_view(out, B * T, C, BF16)
    _call("svsr_tconv_apply", *head, _p(out), out.stride(0), _stream(), label="k_tconv_apply")
    return out


def tconv_epi_bwd_bs(dy: torch.Tensor, acc: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, *, B: int, T: int, co: int, hmax: int,
                     hs: Sequence[int], act: int, slope: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, res_act: int = ACT_NONE,
                     drop: Optional[tuple] = None):
    """Pass 1 of a batch-statistic stage's backward (svsr_tconv_epi_bwd_bs) -> (dres bf16 [B*T, C] or None, sums fp32 [4, C] as tconv_epi_bwd's)."""
    C, _, tab, head = _epi_args(acc, scale, shift, slope, res, B, T, co, hmax, hs, act, res_act, drop)
    _rows_view(dy, B * T, C, BF16)
    dres = torch.empty((B * T, C), dtype=BF16, device=dy.device) if res is not None else None
    part = torch.empty(((B * T + 63) // 64) * 4 * C, dtype=torch.float32, device=dy.device)
    sums = torch.empty((4, C), dtype=torch.float32, device=dy.device)
    _call("svsr_tconv_epi_bwd_bs", _p(dy), dy.stride(0), *head, _p(dres), 0 if dres is None else dres.stride(0), _p(part), _p(sums), _stream(),
          label="k_tconv_epi_bwd_bs")
    return dres, sums


def tconv_bn_bwd(dy: torch.Tensor, acc: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                 ca: torch.Tensor, cb: torch.Tensor, *, B: int, T: int, co: int, hmax: int, hs: Sequence[int], act: int,
                 slope: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, res_act: int = ACT_NONE, drop: Optional[tuple] = None):
    """Pass 2 (svsr_tconv_bn_bwd) -> dacc bf16 [B * (T + 2 * hmax), C]: scale * (g - ca - xhat * cb) on a branch's own rows, zeros elsewhere."""
    C, erows, tab, head = _epi_args(acc, scale, shift, slope, res, B, T, co, hmax, hs, act, res_act, drop)
    _rows_view(dy, B * T, C, BF16)
    for t in (mean, invstd, ca, cb):
        _packed(t, torch.float32, numel=C)
    dacc = torch.empty((erows, C), dtype=BF16, device=dy.device)
    _call("svsr_tconv_bn_bwd", _p(dy), dy.stride(0), *head, _p(mean), _p(invstd), _p(ca), _p(cb), _p(dacc), dacc.stride(0), _stream(),
          label="k_tconv_bn_bwd")
    return dacc


def tcn_norm_pool_bwd_bs(dh: torch.Tensor, dpooled: torch.Tensor, x: torch.Tensor, scale: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                         ca: torch.Tensor, cb: torch.Tensor, mask: torch.Tensor, *, B: int, T: int, C: int, out: torch.Tensor) -> torch.Tensor:
    """tcn_norm_pool_bwd's dx with norm5's batch statistics in the chain (svsr_tcn_norm_pool_bwd_bs): out = scale * (g - ca - xhat * cb)."""
    _norm_pool_bwd_args("tcn_norm_pool_bwd_bs", dh, dpooled, x, out, mask, (scale, mean, invstd, ca, cb), B, T, C)
    _call("svsr_tcn_norm_pool_bwd_bs", _p(dh), _p(dpooled), _p(x), x.stride(0), B, T, C, _p(scale), _p(mean), _p(invstd), _p(ca), _p(cb), _p(mask),
          _p(out), out.stride(0), _stream(), label="k_tcn_norm_pool_bwd_bs")
    return out


def bn_batch_affine(stats: torch.Tensor, n: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = BN_EPS):
    """The O(C) step between tcn_colstats and the apply: stats [2, C] = (mean, sum (x - mean)^2) over n [C] positions ->
    (scale = weight * invstd, shift = bias - mean * scale, mean, invstd, unbiased variance).  A conv bias cancels under batch statistics."""
    mean, var = stats[0], stats[1] / n
    invstd = torch.rsqrt(var + eps)
    scale = weight * invstd
    return scale.contiguous(), (bias - mean * scale).contiguous(), mean.contiguous(), invstd.contiguous(), stats[1] / (n - 1.0)


def bn_batch_param_grads(sum_g: torch.Tensor, sum_g_x: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, n: torch.Tensor):
    """From pass 1's sums of g and g * x: -> (d bn.weight = sum g * xhat, d bn.bias = sum g, ca = sum g / n, cb = sum g * xhat / n)."""
    d_weight = invstd * (sum_g_x - mean * sum_g)
    return d_weight, sum_g, (sum_g / n).contiguous(), (d_weight / n).contiguous()
