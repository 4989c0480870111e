"""The case table of the exact contraction suite (tests/test_contraction_restatement_cpu.py, tests/test_gpu_contraction_edges.py): operation,
shape, tuning knobs (names of g_tune_names in runtime.hip, set through ops.tune) and the instantiation the launch must reach, plus `probe`,
which asks the host-side plan builders (words = None: meta only, no device) what a case would launch under the knobs now in force.

Cases are kept small; the largest is 5,121 rows x 512 columns at K = 64 (the ring-depth-3 form of the
64 x 64 tile needs more than 2.5 x 256 tiles)."""
from __future__ import annotations

import ctypes
from contextlib import contextmanager
from dataclasses import dataclass, field

GLDS = "k_igemm_fwd_glds"
C64_CH = 256          # padded positions per chunk of k_conv3x3_c64 (conv3x3_c64.hip)
REQUIRED_LABELS = (
    f"{GLDS}<64,64,4>", f"{GLDS}<64,64,3>", f"{GLDS}<64,64,4,2>", f"{GLDS}<128,128,2>", f"{GLDS}<128,64,2>", f"{GLDS}<128,64,3>",
    f"{GLDS}<128,64,3,2>",
    f"{GLDS}<64,64,4>+bn", f"{GLDS}<64,64,3>+bn", f"{GLDS}<128,128,2>+bn", f"{GLDS}<128,64,2>+bn", f"{GLDS}<128,64,3>+bn",
    "k_igemm_p8<256,128,3>", "k_igemm_p8<256,64,3>", "k_igemm_p8<256,128,3>+bn", "k_igemm_p8<256,64,3>+bn",
    "k_conv3x3_c64", "k_conv3x3_c64+addend", "k_conv3x3_c64+bn",
    "k_igemm_wgrad<64,3>/split", "k_igemm_wgrad<128,2>/split",
    "k_igemm_wgrad<64,3>/units+k_wgrad_unit_reduce_flat", "k_igemm_wgrad<64,3>/units+k_wgrad_unit_reduce",
    "k_igemm_wgrad<128,2>/units+k_wgrad_unit_reduce_flat", "k_igemm_wgrad<128,2>/units+k_wgrad_unit_reduce",
    "k_igemm_wgrad_group<64,3>", "k_igemm_wgrad_group<128,2>",
    "k_wgrad3x3_halo<8,true>", "k_wgrad3x3_halo<8,false>", "k_wgrad3x3_halo<4,true>", "k_wgrad3x3_halo<4,false>",
)


@dataclass(frozen=True)
class Case:
    name: str
    op: str                      # conv_fwd | dgrad | dgrad_bn | linear | lin_dgrad | lin_dgrad_relu | lin_dgrad_bn | c64 | wgrad | lin_wgrad | group | wgrad3 | chain
    shape: dict                  # convolutions: N H W Ci Co k s p (forward geometry); dense layers: R K N [seq]
    knobs: dict
    label: str
    opts: dict = field(default_factory=dict)
    expect: dict = field(default_factory=dict)     # plan facts the census asserts: splits, units, tiles ...
    cost: int = 0

    @property
    def id(self) -> str:
        return self.name


def _lib():
    from syncvsr_amd import _lib as L

    return L.load()


@contextmanager
def knobs(case_or_dict):
    """sets the knobs of a case; restores each to the value ops.tune_value gave before"""
    from syncvsr_amd import ops

    kv = case_or_dict.knobs if isinstance(case_or_dict, Case) else case_or_dict
    before = {k: ops.tune_value(k) for k in kv}
    try:
        for k, v in kv.items():
            ops.tune(k, v)
        yield
    finally:
        for k, v in before.items():
            ops.tune(k, v)


def _meta8(name: str, *args, wgrad: bool = False):
    meta = (ctypes.c_int * 8)()
    if wgrad:
        nfl = ctypes.c_int64(-1)
        n = getattr(_lib(), name)(*args, None, 0, meta, ctypes.byref(nfl))
        assert n > 0, (name, args, n)
        return meta, int(nfl.value)
    n = getattr(_lib(), name)(*args, None, 0, meta)
    assert n > 0, (name, args, n)
    return meta, 0


def rows_geo(shape: dict, scatter: bool = False):
    """dense layer -> (Nimg, P, src0, dst0), rows of the contraction"""
    R, seq = shape["R"], shape.get("seq")
    if seq is None:
        return (R, 1, 0, 0), R
    S, s0, n = seq
    return ((R // n, n, 0, s0) if scatter else (R // n, n, s0, 0)), R


def _glds_label(meta, Ci: int, Co: int, bn_epi: bool) -> str:
    bm, bn, ns = int(meta[0]), int(meta[1]), int(meta[2])
    if bm == 256:
        return f"k_igemm_p8<256,{bn},{ns}>" + ("+bn" if bn_epi else "")
    kg = int(_lib().svsr_igemm_fwd_kgroups(meta, Ci, Co, int(bn_epi)))
    if kg == 2:
        return f"{GLDS}<{bm},{bn},{3 if bm == 128 else 4},2>"
    return f"{GLDS}<{bm},{bn},{ns}>" + ("+bn" if bn_epi else "")


def w3_dense(H: int, W: int) -> bool:
    """which of the two walks svsr_conv3x3_wgrad takes (not in its plan query): with w3_blocks so large that every chunk is a split, the split
    count is the chunk count — of the real pixels (dense) or of the zero-padded grid."""
    with knobs({"w3_blocks": 1 << 30}):
        sp, nf = ctypes.c_int(0), ctypes.c_int64(0)
        assert _lib().svsr_conv3x3_wgrad_plan(3, H, W, 64, 64, ctypes.byref(sp), ctypes.byref(nf)) == 0
    dense, padded = -(-3 * H * W // 128), -(-3 * (H + 2) * (W + 2) // 128)
    assert dense != padded and sp.value in (dense, padded), (H, W, sp.value)
    return sp.value == dense


def probe(c: Case) -> dict:
    """What the case launches under the knobs in force now: {label, tiles | splits | units | slots | rows ...}.  Host only."""
    from syncvsr_amd import ops

    s, lib = c.shape, _lib()
    if c.op in ("conv_fwd", "dgrad", "dgrad_bn"):
        fwd = c.op == "conv_fwd"
        mode = 0 if fwd else (2 if c.opts.get("addend") == "inplace" and c.op == "dgrad" else 1)
        co_launch, ci_launch = (s["Co"], s["Ci"]) if fwd else (s["Ci"], s["Co"])
        meta, _ = _meta8("svsr_conv_plan", mode, s["N"], s["H"], s["W"], co_launch, s["k"], s["s"], s["p"])
        kg_bn = c.op == "dgrad_bn"
        return dict(label=_glds_label(meta, ci_launch, co_launch, kg_bn), tiles=int(meta[3]), classes=int(meta[5]), max_taps=int(meta[6]),
                    rows=int(meta[7]), kgroups_plain=int(lib.svsr_igemm_fwd_kgroups(meta, ci_launch, co_launch, 0)), mode=mode)
    if c.op in ("linear", "lin_dgrad", "lin_dgrad_relu", "lin_dgrad_bn"):
        fwd = c.op == "linear"
        geo, _ = rows_geo(s, scatter=not fwd)
        co_launch, ci_launch = (s["N"], s["K"]) if fwd else (s["K"], s["N"])
        meta, _ = _meta8("svsr_rows_plan", *geo, co_launch)
        bn_epi = c.op in ("lin_dgrad_relu", "lin_dgrad_bn")
        return dict(label=_glds_label(meta, ci_launch, co_launch, bn_epi), tiles=int(meta[3]), rows=int(meta[7]),
                    kgroups_plain=int(lib.svsr_igemm_fwd_kgroups(meta, ci_launch, co_launch, 0)))
    if c.op == "c64":
        rows = int(lib.svsr_conv3x3_c64_stat_rows(s["N"], s["H"], s["W"]))
        q = s["N"] * (s["H"] + 2) * (s["W"] + 2)
        form = c.opts["form"]
        return dict(label="k_conv3x3_c64" + {"fwd": "", "dgrad": "+addend", "dgrad_bn": "+bn"}[form], rows=rows, chunks=-(-q // C64_CH), rem=q % C64_CH,
                    chunks_per_workgroup=-(-(-(-q // C64_CH)) // rows))
    if c.op in ("wgrad", "lin_wgrad"):
        if c.op == "wgrad":
            meta, nfl = _meta8("svsr_wgrad_plan", s["N"], s["H"], s["W"], s["Ci"], s["Co"], s["k"], s["s"], s["p"], wgrad=True)
        else:
            geo, _ = rows_geo(s)
            meta, nfl = _meta8("svsr_wgrad_rows_plan", *geo, s["K"], s["N"], int(bool(c.opts.get("db"))), wgrad=True)
        base = f"k_igemm_wgrad<{int(meta[0])},{int(meta[1])}>"
        if int(meta[7]) > 0:        # unit list: meta = {bc, ns, slots, units, tasks, taps, maxP, word offset}
            slots, units, tasks = int(meta[2]), int(meta[3]), int(meta[4])
            red = "" if slots <= 0 else ("+k_wgrad_unit_reduce_flat" if slots <= 8 * tasks else "+k_wgrad_unit_reduce")
            # the words (host memory): units {task, first chunk, chunks, slot} at meta[7], then the task table {first slot, slots}
            name, args = (("svsr_wgrad_plan", (s["N"], s["H"], s["W"], s["Ci"], s["Co"], s["k"], s["s"], s["p"])) if c.op == "wgrad" else
                          ("svsr_wgrad_rows_plan", (*rows_geo(s)[0], s["K"], s["N"], int(bool(c.opts.get("db"))))))
            n = getattr(lib, name)(*args, None, 0, meta, ctypes.byref(ctypes.c_int64(0)))
            words = (ctypes.c_int * n)()
            assert getattr(lib, name)(*args, words, n, meta, ctypes.byref(ctypes.c_int64(0))) == n
            u0 = int(meta[7])
            per_task, work = [0] * tasks, [0] * tasks
            for u in range(units):
                per_task[words[u0 + 4 * u]] += 1
                work[words[u0 + 4 * u]] += words[u0 + 4 * u + 2]
            return dict(label=base + "/units" + red, slots=slots, units=units, tasks=tasks, taps=int(meta[5]), part=nfl,
                        units_per_task=sorted({k for k, w in zip(per_task, work) if w > 0}), empty_tasks=sum(1 for w in work if w == 0))
        return dict(label=base + "/split", splits=int(meta[2]), chunks=int(meta[3]), tasks=int(meta[4]), taps=int(meta[5]), part=nfl)
    if c.op == "group":
        tile, out = c.opts["tile"], []
        for q in s["problems"]:
            geo, _ = rows_geo(q)
            bc = tile if q["K"] >= tile and q["N"] >= tile else 64
            meta, nfl = _meta8("svsr_wgrad_rows_plan_tile", *geo, q["K"], q["N"], int(bool(q.get("db"))), bc, wgrad=True)
            assert int(meta[2]) == 1 and int(meta[7]) == 0 and nfl == 0
            out.append(int(meta[0]))
        return dict(label=f"k_igemm_wgrad_group<{tile},{2 if tile == 128 else 3}>", tiles_of=out, groups=sorted(set(out)))
    if c.op in ("wgrad3", "chain"):
        links = s["links"] if c.op == "chain" else [s]
        waves, res = ops.tune_value("w3_waves"), []
        for q in links:
            sp, nf = ctypes.c_int(0), ctypes.c_int64(0)
            assert lib.svsr_conv3x3_wgrad_plan(q["N"], q["H"], q["W"], q["Ci"], q["Co"], ctypes.byref(sp), ctypes.byref(nf)) == 0
            res.append((sp.value, f"k_wgrad3x3_halo<{waves},{'true' if w3_dense(q['H'], q['W']) else 'false'}>"))
        return dict(label=res[0][1], splits=[r[0] for r in res], labels=[r[1] for r in res])
    raise ValueError(c.op)


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def _conv(N, H, W, Ci, Co, k, s, p):
    return dict(N=N, H=H, W=W, Ci=Ci, Co=Co, k=k, s=s, p=p)


def _lin(R, K, N, seq=None):
    d = dict(R=R, K=K, N=N)
    if seq is not None:
        d["seq"] = seq
    return d


T128 = {"igemm_tile": 128, "igemm_bn64_below": 0}
P8 = {"p8_min_items": 1}
UNITS = {"wg_units": 1, "wg_short_k": 0, "wg_unit_max": 2, "wg_unit_min": 1, "wg_blocks": 4}


def _cases() -> list:
    C, L = [], f"{GLDS}"
    add = lambda *a, **k: C.append(Case(*a, **k))
    # ---- k_igemm_fwd_glds<64,64,4>: dense layers, every epilogue option, M / N / K tails -----------------------------------------------
    add("lin_m1_co8_bias", "linear", _lin(1, 64, 8), {}, f"{L}<64,64,4>", dict(bias=True))
    add("lin_m63_co72_relu", "linear", _lin(63, 128, 72), {}, f"{L}<64,64,4>", dict(bias=True, act="relu"))
    add("lin_m64_co64_k3", "linear", _lin(64, 192, 64), {}, f"{L}<64,64,4>", dict(alpha=0.5, addend="separate"))
    add("lin_m65_co100_scalar", "linear", _lin(65, 256, 100), {}, f"{L}<64,64,4>", dict(bias=True, alpha=2.0, addend="alias"))
    add("lin_m129_co136_pitch_f32", "linear", _lin(129, 320, 136), {}, f"{L}<64,64,4>", dict(bias=True, pitch=152, f32=True))
    add("lin_m65_co100_pitch_f32", "linear", _lin(65, 64, 100), {}, f"{L}<64,64,4>", dict(pitch=101, f32=True, addend="separate"))
    add("lin_m129_co192_gelu", "linear", _lin(129, 128, 192), {}, f"{L}<64,64,4>", dict(bias=True, act="gelu", pitch=200))
    add("lin_m65_co100_gelu_scalar", "linear", _lin(65, 64, 100), {}, f"{L}<64,64,4>", dict(bias=True, act="gelu"))
    add("lin_seq_s0_n1", "linear", _lin(5, 128, 72, seq=(7, 0, 1)), {}, f"{L}<64,64,4>", dict(bias=True))
    add("lin_seq_s1_nS1", "linear", _lin(66, 64, 128, seq=(7, 1, 6)), {}, f"{L}<64,64,4>", dict(addend="alias"))
    add("lin_dgrad_seq_s1_n1", "lin_dgrad", _lin(5, 128, 64, seq=(7, 1, 1)), {}, f"{L}<64,64,4>", dict(prefill=True))
    add("lin_dgrad_seq_s0_nS1", "lin_dgrad", _lin(66, 136, 64, seq=(7, 0, 6)), {}, f"{L}<64,64,4>", dict(prefill=True, alpha=0.5, addend="alias"))
    add("lin_dgrad_k4", "lin_dgrad", _lin(129, 72, 256), {}, f"{L}<64,64,4>", dict())
    # K steps 12 / 13 on few tiles: the in-workgroup K split; with a BatchNorm-backward epilogue the same plan must not split
    add("lin_k12_kgroups", "linear", _lin(65, 768, 72), {}, f"{L}<64,64,4,2>", dict(bias=True))
    add("lin_k13_kgroups", "linear", _lin(129, 832, 100), {}, f"{L}<64,64,4,2>", dict(alpha=0.25, addend="separate"))
    add("lin_k11_no_kgroups", "linear", _lin(65, 704, 72), {}, f"{L}<64,64,4>", dict())
    add("lin_k12_ksplit_off", "linear", _lin(65, 768, 72), {"igemm_ksplit": 0}, f"{L}<64,64,4>", dict())
    add("relu_k12_no_kgroups", "lin_dgrad_relu", _lin(65, 72, 768), {}, f"{L}<64,64,4>+bn", dict(gscale=2.0), dict(kgroups_plain=2))
    add("relu_m1", "lin_dgrad_relu", _lin(1, 8, 64), {}, f"{L}<64,64,4>+bn", dict(gscale=1.0))
    add("lin_bn_relu_free_x", "lin_dgrad_bn", _lin(129, 136, 128), {}, f"{L}<64,64,4>+bn", dict(act=1))
    add("lin_bn_swish", "lin_dgrad_bn", _lin(65, 72, 64), {}, f"{L}<64,64,4>+bn", dict(act=2))
    # ---- convolutions on 64 x 64 tiles: nine tap classes with their own tails, stride 2, clamped centres -------------------------------
    add("conv_2x2_s1", "conv_fwd", _conv(17, 2, 2, 64, 72, 3, 1, 1), {}, f"{L}<64,64,4>", dict(stats=True))
    add("conv_3x3_s1_classes", "conv_fwd", _conv(65, 3, 3, 64, 100, 3, 1, 1), {}, f"{L}<64,64,4>", dict(stats=True))
    add("conv_5x4_s1_k18_kgroups", "conv_fwd", _conv(13, 5, 4, 128, 136, 3, 1, 1), {}, f"{L}<64,64,4,2>", dict(stats=True, pitch=144))
    add("conv_6x6_s2", "conv_fwd", _conv(9, 6, 6, 64, 128, 3, 2, 1), {"p8": 0}, f"{L}<64,64,4>", dict(stats=True))
    add("conv_11x11_s2_odd", "conv_fwd", _conv(3, 11, 11, 64, 72, 3, 2, 1), {}, f"{L}<64,64,4>", dict(stats=True))
    add("conv_1x1_s2_even", "conv_fwd", _conv(5, 6, 6, 128, 192, 1, 2, 0), {}, f"{L}<64,64,4>", dict(stats=True))
    add("conv_1x1_s2_odd", "conv_fwd", _conv(5, 5, 5, 64, 8, 1, 2, 0), {}, f"{L}<64,64,4>", dict(stats=True))
    add("dgrad_3x3_s1_plain", "dgrad", _conv(8, 3, 3, 72, 64, 3, 1, 1), {}, f"{L}<64,64,4>", dict())
    add("dgrad_6x6_s2_inplace", "dgrad", _conv(9, 6, 6, 64, 128, 3, 2, 1), {}, f"{L}<64,64,4>", dict(addend="inplace"))
    add("dgrad_11x11_s2_odd_clamped", "dgrad", _conv(3, 11, 11, 64, 64, 3, 2, 1), {}, f"{L}<64,64,4>", dict(addend="separate"))
    add("dgrad_5x4_s2_odd", "dgrad", _conv(13, 5, 4, 136, 64, 3, 2, 1), {}, f"{L}<64,64,4>", dict())
    add("dgrad_1x1_s2_even_mode1", "dgrad", _conv(5, 6, 6, 72, 64, 1, 2, 0), {}, f"{L}<64,64,4>", dict(addend="separate"))
    add("dgrad_1x1_s2_odd_mode1_plain", "dgrad", _conv(5, 5, 5, 64, 128, 1, 2, 0), {}, f"{L}<64,64,4>", dict())
    add("dgrad_1x1_s2_even_mode2", "dgrad", _conv(5, 6, 6, 64, 64, 1, 2, 0), {}, f"{L}<64,64,4>", dict(addend="inplace"))
    add("dgrad_bn_3x3_s1_mask_y", "dgrad_bn", _conv(8, 3, 3, 72, 64, 3, 1, 1), {}, f"{L}<64,64,4>+bn", dict(mask="y", addend=True))
    add("dgrad_bn_6x6_s2_mask_x", "dgrad_bn", _conv(9, 6, 6, 64, 128, 3, 2, 1), {}, f"{L}<64,64,4>+bn", dict(mask="x"))
    add("dgrad_bn_11x11_s2_k_long", "dgrad_bn", _conv(1, 11, 11, 64, 256, 3, 2, 1), {}, f"{L}<64,64,4>+bn", dict(mask="y"), dict(kgroups_plain=2))
    add("dgrad_bn_swish_res", "dgrad_bn", _conv(8, 3, 3, 72, 64, 3, 1, 1), {}, f"{L}<64,64,4>+bn", dict(act=2, res=True, addend=True))
    # ---- <64,64,3>: more than 2.5 x 256 tiles -------------------------------------------------------------------------------------------
    add("lin_many_tiles_ns3", "linear", _lin(5121, 64, 512), {"igemm_lin_bn64": 0}, f"{L}<64,64,3>", dict(bias=True), cost=2)
    add("relu_many_tiles_ns3", "lin_dgrad_relu", _lin(5121, 512, 64), {"igemm_lin_bn64": 0}, f"{L}<64,64,3>+bn", dict(gscale=2.0), cost=2)
    # ---- <128,128,2> ---------------------------------------------------------------------------------------------------------------------
    add("lin_t128_m129_co136", "linear", _lin(129, 192, 136), T128, f"{L}<128,128,2>", dict(bias=True, act="relu", pitch=144))
    add("lin_t128_m127_co100_f32", "linear", _lin(127, 64, 100), T128, f"{L}<128,128,2>", dict(f32=True, bias=True))
    add("lin_t128_m257_gelu", "linear", _lin(257, 128, 192), T128, f"{L}<128,128,2>", dict(act="gelu", bias=True))
    add("conv_t128_6x6_s1", "conv_fwd", _conv(29, 6, 6, 64, 192, 3, 1, 1), dict(T128, p8=0), f"{L}<128,128,2>", dict(stats=True))
    add("dgrad_t128_11x11_s2", "dgrad", _conv(5, 11, 11, 136, 64, 3, 2, 1), T128, f"{L}<128,128,2>", dict(addend="inplace"))
    add("dgrad_bn_t128_6x6_s1", "dgrad_bn", _conv(29, 6, 6, 72, 64, 3, 1, 1), T128, f"{L}<128,128,2>+bn", dict(mask="x", addend=True))
    # ---- <128,64,2>: Co <= 64 with at most four taps; multi-tap Co > 64 with few tiles ----------------------------------------------------
    add("dgrad_t128_co64_s2", "dgrad", _conv(33, 6, 6, 64, 128, 3, 2, 1), {"igemm_tile": 128}, f"{L}<128,64,2>", dict(addend="separate"))
    add("conv_t128_1x1_co8", "conv_fwd", _conv(43, 3, 3, 192, 8, 1, 1, 0), {"igemm_tile": 128}, f"{L}<128,64,2>", dict(stats=True))
    add("conv_t128_few_tiles_co136", "conv_fwd", _conv(15, 3, 3, 64, 136, 3, 1, 1), {"igemm_tile": 128}, f"{L}<128,64,2>", dict(stats=True))
    add("dgrad_bn_t128_co64_s2", "dgrad_bn", _conv(33, 6, 6, 64, 128, 3, 2, 1), {"igemm_tile": 128}, f"{L}<128,64,2>+bn", dict(mask="y"))
    # ---- <128,64,3> ----------------------------------------------------------------------------------------------------------------------
    add("lin_bn64_m129_co100", "linear", _lin(129, 128, 100), {"igemm_lin_bn64": 1}, f"{L}<128,64,3>", dict(bias=True, addend="separate", alpha=4.0))
    add("lin_bn64_m1_co72", "linear", _lin(1, 64, 72), {"igemm_lin_bn64": 1}, f"{L}<128,64,3>", dict(bias=True, act="gelu"))
    add("conv_t128_co64_9taps_ci128", "conv_fwd", _conv(15, 3, 3, 128, 64, 3, 1, 1), {"igemm_tile": 128}, f"{L}<128,64,3>", dict(stats=True))
    add("dgrad_bn_t128_co64_9taps", "dgrad_bn", _conv(15, 3, 3, 64, 128, 3, 1, 1), {"igemm_tile": 128}, f"{L}<128,64,3>+bn", dict(mask="y", addend=True))
    add("lin_bn_bn64_k12", "lin_dgrad_bn", _lin(129, 72, 768), {"igemm_lin_bn64": 1}, f"{L}<128,64,3>+bn", dict(act=1), dict(kgroups_plain=2))
    # ---- <128,64,3,2> ----------------------------------------------------------------------------------------------------------------------
    add("lin_bn64_k12_kgroups", "linear", _lin(129, 768, 100), {"igemm_lin_bn64": 1}, f"{L}<128,64,3,2>", dict(bias=True, act="relu"))
    add("lin_bn64_k13_kgroups", "linear", _lin(257, 832, 72), {"igemm_lin_bn64": 1}, f"{L}<128,64,3,2>", dict(addend="alias", alpha=0.5))
    # ---- k_igemm_p8 --------------------------------------------------------------------------------------------------------------------------
    for grid, stg in ((0, 3), (1, 0), (2, 3), (3, 0)):
        kn = dict(P8, p8_grid=grid, p8_stagger=stg)
        add(f"p8_fwd_co128_g{grid}_s{stg}", "conv_fwd", _conv(29, 6, 6, 64, 128, 3, 1, 1), kn, "k_igemm_p8<256,128,3>", dict(stats=True))
    add("p8_fwd_co192_g2", "conv_fwd", _conv(65, 2, 2, 64, 192, 3, 1, 1), dict(P8, p8_grid=2), "k_igemm_p8<256,64,3>", dict(stats=True))
    add("p8_fwd_s2_co128_g3", "conv_fwd", _conv(29, 11, 11, 64, 128, 3, 2, 1), dict(P8, p8_grid=3, p8_stagger=0), "k_igemm_p8<256,128,3>", dict(stats=True))
    add("p8_fwd_s2_co192", "conv_fwd", _conv(8, 6, 6, 128, 192, 3, 2, 1), P8, "k_igemm_p8<256,64,3>", dict(stats=True, pitch=200))
    add("p8_dgrad_co128_g2", "dgrad", _conv(29, 3, 3, 128, 64, 3, 1, 1), dict(P8, p8_grid=2, p8_stagger=0), "k_igemm_p8<256,128,3>", dict(addend="inplace"))
    add("p8_dgrad_co192_g1", "dgrad", _conv(5, 11, 11, 192, 64, 3, 1, 1), dict(P8, p8_grid=1), "k_igemm_p8<256,64,3>", dict())
    add("p8_dgrad_bn_co128_g3", "dgrad_bn", _conv(29, 3, 3, 128, 64, 3, 1, 1), dict(P8, p8_grid=3), "k_igemm_p8<256,128,3>+bn", dict(mask="y", addend=True))
    add("p8_dgrad_bn_co192_g2", "dgrad_bn", _conv(5, 5, 4, 192, 128, 3, 1, 1), dict(P8, p8_grid=2, p8_stagger=0), "k_igemm_p8<256,64,3>+bn", dict(mask="x"))
    # ---- k_conv3x3_c64: N * (H + 2) * (W + 2) padded positions one below / at / one above a multiple of the 256-position chunk (C64_CH) ----------
    #   W = 2: 2 x 32 x 4 = 256 (an even row pitch never gives +-1); W = 11: 1 x 59 x 13 = 767 = 3 * 256 - 1, 1 x 197 x 13 = 2561 = 10 * 256 + 1;
    #   W = 29 (the cap): 3 x 11 x 31 = 1023 = 4 * 256 - 1, 1 x 223 x 31 = 6913 = 27 * 256 + 1;
    #   many chunks: 18 x 13 x 13 = 3042 -> 12 chunks, one per workgroup by default and SIX per workgroup with reduce_cus = 2
    c64 = (("w2_eq", (2, 30, 2), 1, 0, "x"), ("w11_below", (1, 57, 11), 3, 255, "y"), ("w11_above", (1, 195, 11), 11, 1, "x"),
           ("w29_below", (3, 9, 29), 4, 255, "y"), ("w29_above", (1, 221, 29), 28, 1, "x"), ("w11_many", (18, 11, 11), 12, 226, "y"))
    for name, (N, H, W), chunks, rem, mask in c64:
        for form in ("fwd", "dgrad", "dgrad_bn"):
            for rc in ((0, 2) if name == "w11_many" else (0,)):
                opts = dict(form=form)
                if form == "dgrad_bn":          # mask read from y, or recomputed from x (the from_x branch); the reduce_cus = 2 twin takes the other one
                    opts["mask"] = mask if not rc else {"x": "y", "y": "x"}[mask]
                add(f"c64_{form}_{name}" + ("_rc2" if rc else ""), "c64", dict(N=N, H=H, W=W), {"reduce_cus": rc} if rc else {},
                    "k_conv3x3_c64" + {"fwd": "", "dgrad": "+addend", "dgrad_bn": "+bn"}[form], opts,
                    dict(chunks=chunks, rem=rem, rows=min(chunks, rc or 256), chunks_per_workgroup=-(-chunks // min(chunks, rc or 256))))
    # ---- k_igemm_wgrad: split grids -------------------------------------------------------------------------------------------------------------
    SPLIT = {"wg_units": 0}
    add("wg64_split1", "lin_wgrad", _lin(129, 72, 104), dict(SPLIT, wg_blocks=1), "k_igemm_wgrad<64,3>/split", dict(db=True, mode=0), dict(splits=1))
    add("wg64_split2_add", "lin_wgrad", _lin(513, 64, 136), dict(SPLIT, wg_blocks=6), "k_igemm_wgrad<64,3>/split", dict(db=True, mode=3, prefill=True), dict(splits=2))
    add("wg64_split_more_than_chunks", "lin_wgrad", _lin(130, 64, 64), dict(SPLIT, wg_blocks=64), "k_igemm_wgrad<64,3>/split", dict(db=False, mode=0), dict(splits=3))
    add("wg64_seq_gather", "lin_wgrad", _lin(66, 128, 72, seq=(7, 1, 6)), SPLIT, "k_igemm_wgrad<64,3>/split", dict(db=True, mode=1, prefill=True))
    add("wg64_seq_n1_s0", "lin_wgrad", _lin(65, 64, 8, seq=(7, 0, 1)), SPLIT, "k_igemm_wgrad<64,3>/split", dict(db=True, mode=2, prefill=True))
    for N in (63, 64, 65, 130):
        for im in (0, 1):
            add(f"wg64_conv_s2_N{N}_im{im}", "wgrad", _conv(N, 5, 4, 64, 72, 3, 2, 1), dict(SPLIT, wg_imgmajor=im), "k_igemm_wgrad<64,3>/split",
                dict(mode=0 if im else 1, prefill=not im))
    add("wg64_conv_unreached_tap", "wgrad", _conv(70, 1, 3, 64, 64, 3, 1, 1), SPLIT, "k_igemm_wgrad<64,3>/split", dict(mode=0))
    add("wg128_split1", "lin_wgrad", _lin(1100, 768, 768), dict(SPLIT, wg_blocks=1), "k_igemm_wgrad<128,2>/split", dict(db=True, mode=0), dict(splits=1), cost=1)
    add("wg128_split2", "lin_wgrad", _lin(1537, 776, 776), dict(SPLIT, wg_blocks=98), "k_igemm_wgrad<128,2>/split", dict(db=True, mode=3, prefill=True), dict(splits=2), cost=1)
    # ---- unit lists ---------------------------------------------------------------------------------------------------------------------------------
    add("wgu64_flat_2_units", "lin_wgrad", _lin(193, 72, 104), UNITS, "k_igemm_wgrad<64,3>/units+k_wgrad_unit_reduce_flat", dict(db=True, mode=0))
    add("wgu64_reduce_many_units", "lin_wgrad", _lin(1217, 64, 64), dict(UNITS, wg_unit_max=1, wg_blocks=1), "k_igemm_wgrad<64,3>/units+k_wgrad_unit_reduce",
        dict(db=True, mode=3, prefill=True))
    add("wgu64_conv_s2_eight_queues", "wgrad", _conv(130, 6, 6, 64, 72, 3, 2, 1), UNITS, "k_igemm_wgrad<64,3>/units+k_wgrad_unit_reduce_flat", dict(mode=0))
    # taps of 2, 3, 4 and 6 chunks (64 images, image-major: chunks = positions of the tap) under a unit length of 2: tasks of 1, 2 and 3 units
    add("wgu64_conv_s2_1_2_3_units", "wgrad", _conv(64, 5, 4, 64, 72, 3, 2, 1), UNITS, "k_igemm_wgrad<64,3>/units+k_wgrad_unit_reduce_flat", dict(mode=0),
        dict(units_per_task=[1, 2, 3], units=36))
    add("wgu64_conv_unreached_tap", "wgrad", _conv(70, 1, 3, 64, 64, 3, 1, 1), UNITS, "k_igemm_wgrad<64,3>/units+k_wgrad_unit_reduce_flat", dict(mode=0))
    add("wgu128_flat", "lin_wgrad", _lin(257, 768, 776), UNITS, "k_igemm_wgrad<128,2>/units+k_wgrad_unit_reduce_flat", dict(db=True, mode=1, prefill=True), cost=1)
    add("wgu128_reduce", "lin_wgrad", _lin(1217, 768, 768), dict(UNITS, wg_unit_max=1, wg_blocks=1), "k_igemm_wgrad<128,2>/units+k_wgrad_unit_reduce",
        dict(db=True, mode=0), cost=2)
    # ---- grouped launches -------------------------------------------------------------------------------------------------------------------------
    add("group64", "group", dict(problems=[_lin(65, 72, 104) | {"db": True}, _lin(66, 128, 64, seq=(7, 1, 6)), _lin(1, 64, 8) | {"db": True}]), {},
        "k_igemm_wgrad_group<64,3>", dict(tile=64))
    add("group128_with_narrow", "group", dict(problems=[_lin(129, 136, 192) | {"db": True}, _lin(65, 128, 128), _lin(65, 64, 136) | {"db": True}]), {},
        "k_igemm_wgrad_group<128,2>", dict(tile=128), dict(groups=[64, 128]))
    # ---- k_wgrad3x3_halo: totals one below / at / one above a multiple of the 128-position chunk — of the real pixels N * H * W in the dense form,
    # of the padded grid N * (H + 2) * (W + 2) in the padded walk ---------------------------------------------------------------------------------
    #   dense:  10 x 10, N = 32 -> 3200 = 25 * 128;  11 x 11, N = 55 -> 6655 = 52 * 128 - 1;  11 x 11, N = 73 -> 8833 = 69 * 128 + 1
    #   padded: 12 x 12, N = 32 -> 4608 = 36 * 128;  13 x 13, N = 25 -> 4225 = 33 * 128 + 1;  13 x 13, N = 103 -> 17407 = 136 * 128 - 1
    #   (10 x 29: 372 N is even, never +-1; N = 4 -> 1488 = 11 * 128 + 80)
    for waves in (8, 4):
        for dense in (1, 0):
            kn = {"w3_waves": waves, "w3_dense": dense}
            lab = f"k_wgrad3x3_halo<{waves},{'true' if dense else 'false'}>"
            add(f"w3_{waves}_{dense}_10x10_eq_direct_store", "wgrad3", dict(N=32, H=10, W=10, Ci=64, Co=64), dict(kn, w3_blocks=1), lab, dict(mode=0), dict(splits=[1]))
            add(f"w3_{waves}_{dense}_11x11_padded_above_direct_add", "wgrad3", dict(N=25, H=11, W=11, Ci=64, Co=128), dict(kn, w3_blocks=1), lab,
                dict(mode=1, prefill=True), dict(splits=[1]))
            add(f"w3_{waves}_{dense}_11x11_below_slabs", "wgrad3", dict(N=55, H=11, W=11, Ci=64, Co=64), kn, lab, dict(mode=0), cost=1)
            # (128 real pixels of a 10 x 29 map span more padded rows than the dense form's X tile holds: the padded walk, whatever w3_dense says)
            add(f"w3_{waves}_{dense}_10x29_slabs_add", "wgrad3", dict(N=4, H=10, W=29, Ci=128, Co=64), kn, f"k_wgrad3x3_halo<{waves},false>", dict(mode=1, prefill=True))
            add(f"w3_{waves}_{dense}_11x11_above_slabs", "wgrad3", dict(N=73, H=11, W=11, Ci=64, Co=64), kn, lab, dict(mode=1, prefill=True), cost=1)
            if not dense:
                add(f"w3_{waves}_0_11x11_padded_below_slabs", "wgrad3", dict(N=103, H=11, W=11, Ci=64, Co=64), kn, lab, dict(mode=0), cost=1)
            add(f"w3_{waves}_{dense}_chain", "chain", dict(links=[dict(N=9, H=11, W=11, Ci=64, Co=128), dict(N=4, H=10, W=29, Ci=128, Co=64)]), kn, lab, dict(mode=0))
    return C


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def ordered() -> list:
    """smallest first"""
    return sorted(CASES, key=lambda c: c.cost)


# ---------------------------------------------------------------------------------------------------------------------
# where a wrong element falls: the text assert_bits adds to its report
# ---------------------------------------------------------------------------------------------------------------------
def _tile_edges(label: str):
    """(rows, columns) of the output tile of an instantiation label"""
    import re

    m = re.search(r"<(\d+),(\d+)", label)
    if label.startswith("k_igemm_wgrad"):
        return int(m.group(1)), int(m.group(1))
    return (int(m.group(1)), int(m.group(2))) if m else (64, 64)


def tap_classes(c: Case):
    """per output pixel of one image, in raster order: (the taps (kh, kw) that reach it, its rank among the pixels with the same taps) — the class
    of svsr_conv_plan and the pixel's index inside it.  Forward: output pixels; data gradients: pixels of dx."""
    s = c.shape
    k, st, p = (s.get("k", 3), s.get("s", 1), s.get("p", 1))
    H, W = s["H"], s["W"]
    Ho, Wo = (H + 2 * p - k) // st + 1, (W + 2 * p - k) // st + 1
    fwd = c.op == "conv_fwd" or (c.op == "c64" and c.opts["form"] == "fwd")
    out, seen = [], {}
    for y in range(Ho if fwd else H):
        for x in range(Wo if fwd else W):
            if fwd:
                key = tuple((kh, kw) for kh in range(k) for kw in range(k) if 0 <= y * st + kh - p < H and 0 <= x * st + kw - p < W)
            else:
                key = tuple((kh, kw) for kh in range(k) for kw in range(k)
                            if (y + p - kh) % st == 0 and (x + p - kw) % st == 0 and 0 <= (y + p - kh) // st < Ho and 0 <= (x + p - kw) // st < Wo)
            out.append((key, seen.get(key, 0)))
            seen[key] = seen.get(key, 0) + 1
    return out, seen, (Wo if fwd else W)


def where_of(c: Case, kind: str, plan: dict):
    """-> callback (row, column) of the flattened [rows, columns] output -> the tile, tap class, chunk or split the element falls in"""
    bm, bn = _tile_edges(c.label)
    s = c.shape
    if kind in ("stats", "sums"):
        return lambda r, col: f"{'first' if r == 0 else 'second'} sum of column {col}, column tile {col // bn}, added over {plan.get('tiles', plan.get('rows'))} partial rows"
    if kind.startswith("dw") or kind.startswith("db"):
        if c.op in ("wgrad3", "chain"):
            q = s["links"][int(kind[2:])] if c.op == "chain" else s
            sp = plan["splits"][int(kind[2:]) if c.op == "chain" else 0]
            return lambda r, col: (f"co {r // 9}, tap (kh {r % 9 // 3}, kw {r % 3}), ci {col}: 64 x 64 task (co tile {r // 9 // 64}, ci tile {col // 64}); "
                                   + (f"the sum of {sp} split slabs" if sp > 1 else "one split, written directly"))
        kk = s.get("k", 1) ** 2
        how = (f"the sum of {plan['splits']} split slabs" if plan.get("splits", 1) > 1 else "one split, written directly") if "splits" in plan else \
            f"unit list: {plan.get('units')} units in {plan.get('slots')} slab slots"
        if kind.startswith("db"):
            return lambda r, col: f"bias gradient of output {col}, co tile {col // bm}; {how}"
        k1 = s.get("k", 1)
        return lambda r, col: f"co {r // kk}, tap (kh {r % kk // k1}, kw {r % k1}), ci {col}: task (co tile {r // kk // bm}, ci tile {col // bm}); {how}"
    if c.op in ("conv_fwd", "dgrad", "dgrad_bn", "c64"):
        cls, sizes, width = tap_classes(c)
        P = len(cls)

        def where(r, col):
            n, j = divmod(r, P)
            key, rank = cls[j]
            y, x = divmod(j, width)
            if c.op == "c64":
                qpos = n * (s["H"] + 2) * (s["W"] + 2) + (y + 1) * (s["W"] + 2) + x + 1
                return f"image {n} pixel ({y}, {x}), {len(key)} in-grid taps, padded position {qpos} = chunk {qpos // C64_CH} row {qpos % C64_CH}"
            m = n * sizes[key] + rank
            return (f"image {n} pixel ({y}, {x}), tap class {list(key)} ({len(key)} taps, {sizes[key]} pixels per image): row {m} of the class = its row "
                    f"tile {m // bm} (of {-(-s['N'] * sizes[key] // bm)}) row {m % bm}, column tile {col // bn}")
        return where
    return lambda r, col: f"row tile {r // bm} (row {r % bm} of it), column tile {col // bn}"


# ---------------------------------------------------------------------------------------------------------------------
# operands, references and budgets of a case (CPU; shared by both test files)
# ---------------------------------------------------------------------------------------------------------------------
def build(c: Case) -> dict:
    """-> {"in": operands as the kernels take them, "ref": float64 references per output kind, "abs": the same contraction over |operands|
    (sum of |products| per element), plus whatever the op needs}.  Deterministic per case name."""
    import zlib

    import torch

    import contraction_restatement as R

    seed = zlib.crc32(c.name.encode()) & 0xFFFF
    s, o = c.shape, c.opts
    ints = lambda shape, k, lo=-2, hi=2: torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed + k)).float()
    pow2 = lambda shape, k: 2.0 ** torch.randint(-1, 2, shape, generator=torch.Generator().manual_seed(seed + k)).float()
    d = {"in": {}, "ref": {}, "abs": {}}
    I, ref, ab = d["in"], d["ref"], d["abs"]

    def bn_operands(shape, C):
        I["x"] = ints(shape, 11).to(R.BF)
        I["mean"], I["rstd"] = ints((C,), 12, -1, 1), pow2((C,), 13)
        I["gamma"], I["beta"] = pow2((C,), 14) * (1 - 2 * (torch.arange(C) % 3 == 0).float()), ints((C,), 15, -1, 1)
        if o.get("mask") == "y":
            I["y"] = ints(shape, 16, -1, 1).to(R.BF)
        if o.get("res"):
            I["y"] = ints(shape, 16, -1, 1).to(R.BF)          # the residual INPUT r of the Swish form

    def bn_refs(dd, dabs, C):
        if o.get("act", 1) == 2:
            g, gb, z = R.dgrad_bn_swish(dd, I["x"], I["mean"], I["rstd"], I["gamma"], I["beta"], I.get("y"))
            ref["g_swish"], ref["gb"], ref["z"] = g, gb, z
        else:
            mask = (I["y"].double() > 0) if "y" in I else R.bn_mask(I["x"], I["mean"], I["rstd"], I["gamma"], I["beta"])
            ref["g"], ref["sums"] = R.dgrad_bn_relu(dd, mask, I["x"], I["mean"], I["rstd"], o.get("gscale", 1.0))
            ga = R.rne_bf16(dabs) * o.get("gscale", 1.0)
            xh = ((I["x"].double() - I["mean"].double()) * I["rstd"].double()).abs()
            ab["sum_g"], ab["sum_g_xhat"] = ga.reshape(-1, C).sum(0), (ga * xh).reshape(-1, C).sum(0)
        ab["g"] = dabs

    if c.op in ("conv_fwd", "dgrad", "dgrad_bn", "wgrad", "wgrad3", "chain", "c64"):
        links = s["links"] if c.op == "chain" else [s]
        for li, q in enumerate(links):
            if c.op == "c64":
                q = dict(q, Ci=64, Co=64, k=3, s=1, p=1)
            elif c.op in ("wgrad3", "chain"):
                q = dict(q, k=3, s=1, p=1)
            N, H, W, Ci, Co, k, st, p = (q[n] for n in ("N", "H", "W", "Ci", "Co", "k", "s", "p"))
            Ho, Wo = R.out_size(H, k, st, p), R.out_size(W, k, st, p)
            sfx = str(li) if c.op == "chain" else ""
            fwd_like = c.op == "conv_fwd" or (c.op == "c64" and o["form"] == "fwd")
            if fwd_like:
                I["x"], I["w"] = R.exact((N, H, W, Ci), seed + 1), R.exact((Co, k, k, Ci), seed + 2)
                acc = R.conv_fwd(I["x"], I["w"], st, p)
                ref["out"], ref["stats"] = acc, R.fwd_stats(acc)
                ab["out"] = R.conv_fwd(I["x"].abs(), I["w"].abs(), st, p)
                ab["sum"], ab["sumsq"] = ab["out"].reshape(-1, Co).sum(0), ref["stats"][1]
            elif c.op in ("dgrad", "dgrad_bn", "c64"):
                I["dy"], w = R.exact((N, Ho, Wo, Co), seed + 1), R.exact((Co, k, k, Ci), seed + 2)
                I["wt"] = w.permute(3, 1, 2, 0).contiguous()          # transposed shadow [Ci][k][k][Co]
                dd, dabs = R.conv_dgrad(I["dy"], w, st, p, (H, W)), R.conv_dgrad(I["dy"].abs(), w.abs(), st, p, (H, W))
                d["reach"] = R.dgrad_reach(k, st, p, (H, W))
                if o.get("addend") or (c.op == "c64" and o["form"] == "dgrad"):
                    I["addend"] = ints((N, H, W, Ci), 3, -3, 3).to(R.BF)
                    dd, dabs = dd + I["addend"].double(), dabs + I["addend"].double().abs()
                if c.op == "dgrad_bn" or (c.op == "c64" and o["form"] == "dgrad_bn"):
                    bn_operands((N, H, W, Ci), Ci)
                    bn_refs(dd, dabs, Ci)
                else:
                    ref["out"], ab["out"] = dd, dabs
            else:
                I["x" + sfx], I["dy" + sfx] = R.exact((N, H, W, Ci), seed + 1 + 10 * li), R.exact((N, Ho, Wo, Co), seed + 2 + 10 * li)
                ref["dw" + sfx] = R.conv_wgrad(I["x" + sfx], I["dy" + sfx], k, st, p)
                ab["dw" + sfx] = R.conv_wgrad(I["x" + sfx].abs(), I["dy" + sfx].abs(), k, st, p)
                if o.get("prefill"):
                    I["dw0" + sfx] = ints((Co, k, k, Ci), 4 + li, -4, 4)
                    ref["dw" + sfx], ab["dw" + sfx] = ref["dw" + sfx] + I["dw0" + sfx].double(), ab["dw" + sfx] + I["dw0" + sfx].double().abs()
        return d
    if c.op == "group":
        for i, q in enumerate(s["problems"]):
            sub = build(Case(f"{c.name}.{i}", "lin_wgrad", {k: v for k, v in q.items() if k != "db"}, {}, "", dict(db=q.get("db", False), prefill=i % 2 == 1)))
            for part in ("in", "ref", "abs"):
                for k, v in sub[part].items():
                    d[part][f"{k}{i}"] = v
        return d
    # dense layers
    Rr, K, N, seq = s["R"], s["K"], s["N"], s.get("seq")
    rows_all = Rr if seq is None else (Rr // seq[2]) * seq[0]
    if c.op == "linear":
        I["x"], I["w"] = R.exact((rows_all, K), seed + 1), R.exact((N, K), seed + 2)
        acc, aabs = R.linear(I["x"], I["w"], seq), R.linear(I["x"].abs(), I["w"].abs(), seq)
        if o.get("bias"):
            I["bias"] = ints((N,), 3, -3, 3)
            aabs = aabs + I["bias"].abs().double()
        if o.get("addend"):
            I["addend"] = ints((Rr, N), 4, -3, 3).to(R.BF)
            aabs = aabs * abs(o.get("alpha", 1.0)) + I["addend"].double().abs()
        ref["out"], ref["pre"] = R.epilogue(acc, I.get("bias"), o.get("act", "none"), o.get("alpha", 1.0), I.get("addend"))
        ab["out"] = aabs
        return d
    Np = -(-N // 64) * 64
    if c.op in ("lin_dgrad", "lin_dgrad_relu", "lin_dgrad_bn"):
        I["dy"], w = R.exact((Rr, Np), seed + 1), R.exact((N, K), seed + 2)
        I["wt"] = torch.zeros(K, Np, dtype=R.BF)
        I["wt"][:, :N] = w.t()
        dd, dabs = I["dy"][:, :N].double() @ w.double(), I["dy"][:, :N].double().abs() @ w.double().abs()
        if c.op == "lin_dgrad":
            a = o.get("alpha", 1.0)
            dd, dabs = dd * a, dabs * abs(a)
            if o.get("addend"):
                I["addend"] = ints((rows_all, K), 4, -3, 3).to(R.BF)
                tgt = slice(None) if seq is None else R.seq_rows(Rr // seq[2], seq[0], seq[1], seq[2])
                dd, dabs = dd + I["addend"][tgt].double(), dabs + I["addend"][tgt].double().abs()
            ref["out"], ab["out"] = dd, dabs
        elif c.op == "lin_dgrad_relu":
            I["y"] = ints((Rr, K), 5, -1, 2).clamp_min(0).to(R.BF)
            zero, one = torch.zeros(K), torch.ones(K)
            ref["g"], ref["sums"] = R.dgrad_bn_relu(dd, I["y"].double() > 0, I["y"], zero, one, o["gscale"])
            ab["g"] = dabs
            ab["sum_g"] = (R.rne_bf16(dabs) * o["gscale"]).sum(0)
        else:
            bn_operands((Rr, K), K)
            bn_refs(dd, dabs, K)
        return d
    if c.op == "lin_wgrad":
        I["x"], I["dy"] = R.exact((rows_all, K), seed + 1), R.exact((Rr, N), seed + 2)
        ref["dw"], ref["db"] = R.linear_wgrad(I["x"], I["dy"], seq)
        ab["dw"], ab["db"] = R.linear_wgrad(I["x"].abs(), I["dy"].abs(), seq)
        mode = o.get("mode", 3)          # SVSR_GRAD_ADD_DW = 1 | SVSR_GRAD_ADD_DB = 2: a destination that is added to starts from small integers
        if o.get("prefill") and mode & 1:
            I["dw0"] = ints((N, K), 4, -4, 4)
            ref["dw"], ab["dw"] = ref["dw"] + I["dw0"].double(), ab["dw"] + I["dw0"].double().abs()
        if o.get("prefill") and mode & 2:
            I["db0"] = ints((N,), 5, -4, 4)
            ref["db"], ab["db"] = ref["db"] + I["db0"].double(), ab["db"] + I["db0"].double().abs()
        if not o.get("db"):
            del ref["db"], ab["db"]
        return d
    raise ValueError(c.op)
