"""First-touch stores of the flat gradient buffer (-m gpu): the word-level model at the benchmark shape (32 clips of 29 x 88 x 88).

Reference = the same steps with ops.GRAD_STORE off: the whole buffer zero-filled and every writer in add mode (the behaviour before the change,
kept reachable through the mode flag).  Everything is compared BIT FOR BIT — a store writes 0.f + sum, exactly what the add onto zeros left.
The coverage proof fills the whole buffer with NaNs ahead of the step's own (shrunk) zero-fill: a planned span that some launch read instead
of storing, or that nobody wrote, would leave NaNs in the gradients, the moments and the parameters."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 4


def _setup():
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.init import init_state_dict, synthetic_batch

    dev = torch.device("cuda:0")
    cfg = default_lrw_config()
    cfg.optim.scheduler.num_warmup_steps = 1
    sd = init_state_dict(cfg, seed=0)
    batch = [t.to(dev) for t in synthetic_batch(cfg, 32, seed=1234)]
    return dev, cfg, sd, batch


def _run(dev, cfg, sd, batch, *, store: bool, nan: bool = False, **kw):
    from syncvsr_amd import ops
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    saved = ops.GRAD_STORE, ops.GRAD_FILL_NAN
    ops.GRAD_STORE, ops.GRAD_FILL_NAN = store, nan
    try:
        model = Model(cfg)
        model.load_state_dict(sd)
        model.to(dev).train()
        ts = TrainStep(model, cfg, **kw)
        losses = [ts.step(*batch)["loss_total"].clone() for _ in range(STEPS)]
        ts.synchronize()
        torch.cuda.synchronize()
        st = model.store()
        cov = ts.__dict__.get("_cover", (None, None))[1]
        assert (cov is not None) == store, "the first-touch map must be in use exactly when ops.GRAD_STORE is on"
        pads = torch.ones(st.numel, dtype=torch.bool, device=dev)
        for n, (o, numel, shape) in st.offsets.items():
            if tuple(st.phys[n]) == tuple(shape):
                pads[o : o + numel] = False
            else:            # padded storage: everything outside the logical corner
                m = torch.ones(st.phys[n], dtype=torch.bool, device=dev)
                m[tuple(slice(0, d) for d in shape)] = False
                pads[o : o + numel] = m.reshape(-1)
        return dict(losses=torch.stack(losses), grad=st.grad.clone(), flat=st.flat.clone(), m=ts.m.clone(), v=ts.v.clone(), buffers=st.bufflat.clone(),
                    pad_grad=st.grad[pads].clone(), launches=ts._rec.size if ts._rec is not None else None)
    finally:
        ops.GRAD_STORE, ops.GRAD_FILL_NAN = saved


_REF: dict = {}


def _reference(dev, cfg, sd, batch):
    if "r" not in _REF:
        _REF["r"] = _run(dev, cfg, sd, batch, store=False)
    return _REF["r"]


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("mode", ["eager", "native", "graph"])
def test_store_steps_equal_the_all_add_steps_bit_for_bit(mode):
    """4 optimiser steps with first-touch stores — eager, native step list, HIP-graph replay — against 4 eager steps of the all-add path:
    losses, gradients, parameters, both AdamW moments and the running statistics carry the same bits; the NaN pre-fill proves that no
    planned span was read before it was stored and none was left without a writer; pads stay exactly zero."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dev, cfg, sd, batch = _setup()
    ref = _reference(dev, cfg, sd, batch)
    kw = dict(native=True) if mode == "native" else dict(use_graph=True) if mode == "graph" else {}
    got = _run(dev, cfg, sd, batch, store=True, nan=True, **kw)
    for k in ("losses", "grad", "flat", "m", "v", "buffers"):
        x, y = got[k], ref[k]
        assert bool(torch.isfinite(x).all()), f"{mode}: {k} holds {int((~torch.isfinite(x)).sum())} non-finite values (a stale or unwritten gradient range)"
        diff = int((x.view(torch.int32) != y.view(torch.int32)).sum())
        print(f"{mode}: {k}: {diff} of {x.numel()} words differ from the all-add path")
        assert diff == 0, f"{mode}: {k}: {diff} of {x.numel()} words differ from the all-add path"
    assert int((got["pad_grad"].view(torch.int32) != 0).sum()) == 0, "a storage pad of the gradient buffer is not exactly +0"


def test_native_list_is_no_longer_with_the_range_fill():
    """The recorded list: one svsr_fill_ranges launch stands where the whole-buffer memset stood."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dev, cfg, sd, batch = _setup()
    a = _run(dev, cfg, sd, batch, store=False, native=True)
    b = _run(dev, cfg, sd, batch, store=True, native=True)
    print("ops per recorded step: all-add", a["launches"], "first-touch stores", b["launches"])
    assert b["launches"] <= a["launches"]
    for k in ("losses", "grad", "flat"):
        assert _same(a[k], b[k]), k


def test_nothing_stays_armed_after_a_step():
    """Outside a TrainStep step every weight-gradient launch adds (model.accumulate_into_grads(True): the documented hand-rolled accumulation
    loop): the first-touch map is disarmed when the optimiser starts."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from golden_cases import build_case
    from syncvsr_amd import ops
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg, sd, batch, training, gold = build_case("lrw_tiny")
    gb = [t.to(dev) for t in batch]
    model = Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, cfg)
    ts.step(*gb)
    assert ops._COVER is None
    torch.cuda.synchronize()


def test_backward_after_a_step_adds_in_the_hand_rolled_loop():
    """The documented accumulate_into_grads(True) loop after a TrainStep step: a second backward from the same state (weights, running
    statistics, dropout word restored) leaves exactly twice the first one's gradient (x + x is exact) — no launch kept a store mode."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from golden_cases import build_case
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg, sd, batch, training, gold = build_case("lrw_tiny")
    gb = [t.to(dev) for t in batch]
    model = Model(cfg)
    model.load_state_dict(sd)
    model.to(dev).train()
    ts = TrainStep(model, cfg)
    ts.step(*gb)
    ts.synchronize()
    st = model.store()
    bufs, rng = st.bufflat.clone(), model.rng_state()

    def backward(keep: bool) -> torch.Tensor:
        st.bufflat.copy_(bufs)
        model.load_rng_state(rng)
        model.accumulate_into_grads(keep)
        model(*gb)["loss_total"].backward()
        torch.cuda.synchronize()
        return st.grad.clone()

    g1 = backward(False)
    assert torch.equal(backward(False), g1), "two backward passes from one state differ: the doubling check below would prove nothing"
    g2 = backward(True)
    model.accumulate_into_grads(False)
    assert float(g1.abs().max()) > 0 and torch.equal(g2, g1 + g1), f"{int((g2 != g1 + g1).sum())} elements are not twice the first backward's"


def test_store_spans_are_the_ranges_the_backward_writes(monkeypatch):
    """model.grad_store_spans against the writers the model ISSUES: every weight-gradient launch of one eager backward at the benchmark
    configuration (tiny batch) that targets an unpadded tensor of the gradient buffer through a store-capable wrapper, and nothing else,
    is a declared span — each written by exactly one launch."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import ops
    from syncvsr_amd.config import default_lrw_config
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.init import init_state_dict, synthetic_batch
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg = default_lrw_config()
    model = Model(cfg)
    model.load_state_dict(init_state_dict(cfg, seed=0))
    model.to(dev).train()
    batch = [t.to(dev) for t in synthetic_batch(cfg, 2, seed=5)]
    ts = TrainStep(model, cfg)
    st = model.store()
    seen: list = []
    real = ops._grad_add

    def spy(dw, n):
        lo = (dw.data_ptr() - st.grad.data_ptr()) // 4
        if 0 <= lo < st.numel:
            seen.append((lo, lo + n))
        return real(dw, n)

    monkeypatch.setattr(ops, "_grad_add", spy)
    ts.step(*batch)
    torch.cuda.synchronize()
    unpadded = {(o, o + n) for name, (o, n, shape) in st.offsets.items() if tuple(st.phys[name]) == tuple(shape)}
    qkv = {(st.offsets[f"encoder.encoder.layer.{i}.attention.self.query.weight"][0],) for i in range(model.layers)}
    writes = [s for s in seen if s in unpadded or (s[0],) in qkv]
    spans = sorted(model.grad_store_spans(st.offsets, st.phys))
    assert sorted(writes) == spans, (len(writes), len(spans))
    assert len(seen) == len(set(seen)), "a range has two weight-gradient launches in one backward"


def _accum_scenario(store: bool, native: bool, n: int) -> dict:
    """Windows of n micro-steps on the tiny word-level case: one whole window, a window whose middle (n = 3) or last (n = 2) micro-step records
    again, a checkpoint inside the next window resumed into a fresh model and TrainStep, and a partial window closed by flush()."""
    from golden_cases import build_case
    from syncvsr_amd import ops
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg, sd, batch, training, gold = build_case("lrw_tiny")
    gb = [t.to(dev) for t in batch]
    saved = ops.GRAD_STORE
    ops.GRAD_STORE = store
    try:
        def make():
            m = Model(cfg)
            m.load_state_dict(sd)
            return m.to(dev).train()

        model = make()
        ts = TrainStep(model, cfg, native=native, accumulate=n)
        losses = []

        def step(t):
            losses.append(t.step(*gb)["loss_total"].clone())
            assert ops._COVER is None, "a first-touch map is armed inside an accumulation window"

        for _ in range(n):
            step(ts)
        step(ts)
        if native:
            torch.cuda.synchronize()
            ts._rec = None                       # the next micro-step (not the first of its window) records again
        for _ in range(n - 1):
            step(ts)
        step(ts)                                 # first micro-step of the third window, then a checkpoint inside it
        msd, tsd = {k: v.clone() for k, v in model.state_dict().items()}, ts.state_dict()
        model2 = make()
        model2.load_state_dict(msd)
        ts2 = TrainStep(model2, cfg, native=native, accumulate=n)
        ts2.load_state_dict(tsd)
        for _ in range(n - 1):
            step(ts2)
        step(ts2)                                # a partial window of one micro-step ...
        assert ts2.flush() is True               # ... stepped on
        ts2.synchronize()
        torch.cuda.synchronize()
        st = model2.store()
        return dict(losses=torch.stack(losses), flat=st.flat.clone(), m=ts2.m.clone(), v=ts2.v.clone(), buffers=st.bufflat.clone(),
                    step=ts2.state()["step"])
    finally:
        ops.GRAD_STORE = saved


@pytest.mark.parametrize("native", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_accumulation_windows_are_untouched_by_first_touch_stores(native, n):
    """accumulate = 2, 3 (eager and native; a re-recording micro-step, resume from state_dict() inside a window, flush() on a partial window):
    windows keep the whole-buffer fill and the add mode, so parameters, moments and running statistics are bit-identical with ops.GRAD_STORE on
    and off, and no first-touch map is ever armed inside a window."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    a, b = _accum_scenario(True, native, n), _accum_scenario(False, native, n)
    assert a["step"] == b["step"] == 4
    for k in ("losses", "flat", "m", "v", "buffers"):
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"accumulate={n}, native={native}: {k} differs"


def test_layer_drop_with_scripted_skips_keeps_the_whole_buffer_fill():
    """lrw-xt: the x-transformers encoder declares no spans (a skipped block has no writer), so steps with scripted skips are the same
    with ops.GRAD_STORE on and off, eager and native, and every gradient is finite."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import ops
    from syncvsr_amd.config import xtransformers_lrw_config
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.init import init_state_dict, synthetic_batch
    from syncvsr_amd.model import Model

    dev = torch.device("cuda:0")
    cfg = xtransformers_lrw_config(True, model__bert__depth=3, model__bert__layer_dropout=0.3, optim__scheduler__num_warmup_steps=1)
    sd = init_state_dict(cfg, seed=3, perturb_norm=True)
    batch = [t.to(dev) for t in synthetic_batch(cfg, 4, frames=5, size=32, seed=100)]
    skips = [{1}, set(), {0, 3}, {2, 5}]

    def run(store: bool, native: bool):
        saved = ops.GRAD_STORE
        ops.GRAD_STORE = store
        try:
            model = Model(cfg, seed=77)
            model.load_state_dict(sd)
            model.to(dev).train()
            assert model.grad_store_spans(model.store().offsets, model.store().phys) == []
            ts = TrainStep(model, cfg, native=native)
            for s in skips:
                model.layer_skip_override = set(s)
                ts.step(*batch)
                assert ops._COVER is None
            ts.synchronize()
            torch.cuda.synchronize()
            st = model.store()
            return st.grad.clone(), st.flat.clone(), ts.m.clone()
        finally:
            ops.GRAD_STORE = saved

    ref = run(False, False)
    for native in (False, True):
        got = run(True, native)
        for x, y in zip(got, ref):
            assert bool(torch.isfinite(x).all()) and torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("native", [False, True])
def test_lrs_bench_shape_coverage_proof(native):
    """The sentence-level model at the benchmark shape (16 clips padded to 160 frames, dropout 0.1): three steps with first-touch stores on a
    NaN pre-filled gradient buffer, eager and native, against three eager steps of the all-add path: gradients, parameters, moments and
    running statistics finite and bit-identical, pads of the gradient buffer exactly zero."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import ops
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.lrs_data import LengthBucketBatchSampler, reference_length_histogram
    from syncvsr_amd.lrs_init import LRS_ODIM, default_lrs_args, lrs_init_state_dict, lrs_synthetic_batch
    from syncvsr_amd.lrs_model import E2E

    dev = torch.device("cuda:0")
    args = default_lrs_args(dropout_rate=0.1, transformer_attn_dropout_rate=0.1)
    pool = reference_length_histogram(4096, seed=7) * 150 // 155
    sampler = LengthBucketBatchSampler(pool, 16, 1, 0, width=16, seed=11)
    idx = max(range(len(sampler)), key=lambda i: sampler.padded_frames()[i])
    frames = sampler.padded_frames()[idx]
    assert frames == 160, frames
    batch = [t.to(dev) for t in lrs_synthetic_batch(args, 16, frames, seed=1234, lengths=pool[list(sampler)[idx]])]
    sd = lrs_init_state_dict(args, LRS_ODIM, seed=0)

    def run(store: bool, nan: bool, native: bool):
        saved = ops.GRAD_STORE, ops.GRAD_FILL_NAN
        ops.GRAD_STORE, ops.GRAD_FILL_NAN = store, nan
        try:
            model = E2E(LRS_ODIM, args)
            model.load_state_dict(sd, strict=True)
            model.to(dev).train()
            model.reseed_dropout(41)
            ts = TrainStep(model, native=native)
            for _ in range(3):
                ts.step(*batch)
                assert ops._COVER is None
            ts.synchronize()
            torch.cuda.synchronize()
            assert (ts.__dict__.get("_cover", (None, None))[1] is not None) == store
            st = model.store()
            pads = [torch.zeros(1, device=dev)]
            for n, (o, numel, shape) in st.offsets.items():
                if tuple(st.phys[n]) != tuple(shape):
                    m = torch.ones(st.phys[n], dtype=torch.bool, device=dev)
                    m[tuple(slice(0, d) for d in shape)] = False
                    pads.append(st.grad[o : o + numel][m.reshape(-1)])
            return dict(grad=st.grad.clone(), flat=st.flat.clone(), m=ts.m.clone(), v=ts.v.clone(), buffers=st.bufflat.clone()), torch.cat(pads)
        finally:
            ops.GRAD_STORE, ops.GRAD_FILL_NAN = saved

    if "lrs" not in _REF:
        _REF["lrs"] = run(False, False, False)
    ref, _ = _REF["lrs"]
    got, pads = run(True, True, native)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), f"{k}: {int((~torch.isfinite(got[k])).sum())} non-finite values"
        diff = int((got[k].view(torch.int32) != ref[k].view(torch.int32)).sum())
        print(f"lrs native={native}: {k}: {diff} of {got[k].numel()} words differ from the all-add path")
        assert diff == 0, f"{k}: {diff} words differ"
    assert int((pads.view(torch.int32) != 0).sum()) == 0


_HALO_SHAPES = (torch.empty(128, 22, 22, 64, device="meta"), torch.empty(128, 22, 22, 64, device="meta"))


def _mode_case(kind: str, dev):
    """-> run(mode, dw, db): one weight-gradient launch of the given kind through the ops wrapper; (dw elements, db elements or 0)."""
    from syncvsr_amd import ops

    g = torch.Generator(device="cpu").manual_seed(17)

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16).to(dev)

    if kind in ("linear_direct", "linear_units", "linear_splitk"):
        rows, K, N = (960, 512, 2048) if kind == "linear_direct" else (2400, 768, 3072)
        x, dy = rnd(rows, K), rnd(rows, N)
        return (lambda mode, dw, db: ops.linear_wgrad(x, dy, dw, rows=rows, K=K, N=N, x_pitch=K, dy_pitch=N, db=db, mode=mode)), N * K, N
    if kind == "conv1x1_units":
        x, dy = rnd(256, 11, 11, 128), rnd(256, 6, 6, 256)
        return (lambda mode, dw, db: ops.conv2d_wgrad(x, dy, dw, 1, 2, 0, mode=mode)), 256 * 128, 0
    if kind == "conv3x3_halo":
        x, dy = rnd(128, 22, 22, 64), rnd(128, 22, 22, 64)
        return (lambda mode, dw, db: ops.conv2d_wgrad(x, dy, dw, 3, 1, 1, mode=mode)), 64 * 9 * 64, 0
    if kind == "conv3x3_empty_taps":       # a 1 x 1 map: only the centre tap has a position; the other eight must still be WRITTEN (zeros)
        x, dy = rnd(2048, 1, 1, 64), rnd(2048, 1, 1, 64)
        return (lambda mode, dw, db: ops.conv2d_wgrad(x, dy, dw, 3, 1, 1, mode=mode)), 64 * 9 * 64, 0
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["linear_direct", "linear_units", "linear_splitk", "conv1x1_units", "conv3x3_halo", "conv3x3_empty_taps"])
def test_store_mode_of_every_weight_gradient_path(kind):
    """Every kernel path with a store / add mode — direct write, unit list + reducers (both forms), split-K + column sum, halo 3 x 3 + reducer,
    and a plan with taps no position reaches — for every mode: a destination whose ADD bit is clear is pre-filled with NaNs and must come
    out bit-identical to the add onto zeros (never read, every element written); one whose bit is set starts from zeros."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import ops

    dev = torch.device("cuda:0")
    units_before = ops.tune_value("wg_units")
    if kind == "linear_splitk":
        ops.tune("wg_units", 0)
    try:
        run, ndw, ndb = _mode_case(kind, dev)
        # the path each kind must reach (meta of the plan: {tile, ring, splits | slots, chunks | units, tasks, taps, max positions, unit offset})
        plan = {"linear_direct": lambda: ops.wgrad_rows_plan(960, 1, 0, 0, 512, 2048, True), "linear_units": lambda: ops.wgrad_rows_plan(2400, 1, 0, 0, 768, 3072, True),
                "linear_splitk": lambda: ops.wgrad_rows_plan(2400, 1, 0, 0, 768, 3072, True), "conv1x1_units": lambda: ops.wgrad_conv_plan(256, 11, 11, 128, 256, 1, 2, 0),
                "conv3x3_empty_taps": lambda: ops.wgrad_conv_plan(2048, 1, 1, 64, 64, 3, 1, 1)}.get(kind)
        if plan is not None:
            meta = [int(v) for v in plan().meta]
            slots, tasks = meta[2], meta[4]
            if kind == "linear_direct":
                assert meta[7] == 0 and meta[2] == 1, meta                     # no unit list, no K split: tiles go to dW directly
            elif kind == "linear_splitk":
                assert meta[7] == 0 and meta[2] > 1, meta                      # K split: slabs + k_colsum
            elif kind == "linear_units":
                assert meta[7] > 0 and 0 < slots <= 8 * tasks, meta            # unit list, few slots per task: k_wgrad_unit_reduce_flat
            elif kind == "conv1x1_units":
                assert meta[7] > 0 and slots > 8 * tasks, meta                 # unit list, many slots per task: k_wgrad_unit_reduce
            else:
                assert meta[7] > 0 and meta[5] == 9, meta                      # unit list over nine taps, eight of them empty
        else:
            assert ops.halo_wgrad_ok(*_HALO_SHAPES, 3, 1, 1)                   # conv3x3_halo: k_wgrad3x3_halo (+ k_wgrad3_reduce when split)
        dw0 = torch.zeros(ndw, dtype=torch.float32, device=dev)
        db0 = torch.zeros(ndb, dtype=torch.float32, device=dev) if ndb else None
        run(3, dw0, db0)
        torch.cuda.synchronize()
        assert float(dw0.abs().max()) > 0
        if kind == "conv3x3_empty_taps":
            assert int((dw0.view(64, 9, 64)[:, [0, 1, 2, 3, 5, 6, 7, 8]] != 0).sum()) == 0
        for mode in ((0, 1, 2) if ndb else (0,)):
            dw = torch.full((ndw,), float("nan"), device=dev) if not mode & 1 else torch.zeros(ndw, device=dev)
            db = None if not ndb else (torch.full((ndb,), float("nan"), device=dev) if not mode & 2 else torch.zeros(ndb, device=dev))
            run(mode, dw, db)
            torch.cuda.synchronize()
            assert torch.equal(dw.view(torch.int32), dw0.view(torch.int32)), f"{kind} mode {mode}: dw"
            if ndb:
                assert torch.equal(db.view(torch.int32), db0.view(torch.int32)), f"{kind} mode {mode}: db"
        # and the add mode adds: a second launch onto the result doubles it
        run(3, dw0, db0)
        torch.cuda.synchronize()
        assert torch.equal(dw0, dw + dw)
    finally:
        if kind == "linear_splitk":
            ops.tune("wg_units", units_before)


def test_recorded_list_holds_a_range_fill_where_the_memset_stood():
    """svsr_steplist_dry_run of the recorded benchmark step: one memset fewer, one call more, the same number of ops."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from syncvsr_amd import ops
    from syncvsr_amd.engine import TrainStep
    from syncvsr_amd.model import Model

    dev, cfg, sd, batch = _setup()
    counts = {}
    for store in (False, True):
        saved = ops.GRAD_STORE
        ops.GRAD_STORE = store
        try:
            model = Model(cfg)
            model.load_state_dict(sd)
            model.to(dev).train()
            ts = TrainStep(model, cfg, native=True)
            ts.step(*batch)
            torch.cuda.synchronize()
            counts[store] = dict(ts._rec.would_issue(), size=ts._rec.size)
            if store:
                cov = ts._cover[1]
                filled = cov.hole_elems() * 4
                uncovered = model.store().numel * 4 - sum(hi - lo for lo, hi in cov.spans) * 4
                print("bytes zero-filled per step:", model.store().numel * 4, "->", filled)
                assert uncovered <= filled <= uncovered + 12 * len(cov.holes)                # the fill IS the remainder (+ <= 3 floats per hole)
                assert filled < 2 * 2 ** 20 and len(cov.holes) <= 16                          # < 2 MB of 128 MB, one launch
        finally:
            ops.GRAD_STORE = saved
    print(counts)
    assert counts[True]["memsets"] == counts[False]["memsets"] - 1
    assert counts[True]["calls"] == counts[False]["calls"] + 1
    assert counts[True]["size"] == counts[False]["size"]
