"""Seeded cases and plain references of the beam-search kernel tests (tests/test_gpu_lrs_search_clips.py, tests/test_search_cases_cpu.py):
source attention of one query row per hypothesis (csrc/lrs_search.hip k_mha_src_step) with its fp64 statement, an fp32 restatement of the
kernel's chunked online softmax and two deliberately wrong variants of it, the selection planes of svsr_beam_select at its edges, and the
statement of the search itself: the single-clip loop `BatchBeamSearch.forward` ran before it became a one-clip group of the multi-clip search.
Everything here is plain torch; the GPU tests copy the inputs over and compare."""
from __future__ import annotations

import functools

import torch

BF16 = torch.bfloat16
LOGZERO = -1.0e10

# ----------------------------------------------------------------------------------------------------------------------
# source attention
# ----------------------------------------------------------------------------------------------------------------------
# name -> (seed, H, Tmax, tlens, clip_of).  A tlen above Tmax stands for a clip whose Tmax frames are all valid (the kernel clamps).
#   t150: clips of 1, 64, 65, 150, 0, 129 frames (one chunk, exactly one, one + 1 key, two + 22, none, two + 1), rows without a clip (-1, 6),
#         15 rows x 3 heads = 45 waves: the last workgroup is one wave
#   t130: 12 heads; the over-long length belongs to clip 0, so frames "130 .. 136" of it would be the first frames of clip 1, and its row
#         is the diffuse one: seven more keys move every channel
#   t1:   one key
SRC_STEP_SHAPES = {
    "t150": (31, 3, 150, (1, 64, 65, 150, 0, 129), (0, 1, 1, 2, 2, 3, 3, 3, 3, 4, -1, 6, 5, 5, 3)),
    "t130": (32, 12, 130, (130 + 7, 63, 130), (1, 1, 2, 2, 0)),
    "t1": (33, 1, 1, (1,), (0,)),
}
SRC_STEP_PEAK = 12.0
SRC_STEP_KV_PAD = 8


def _frames(clip: int, tlens, Tmax: int) -> int:
    return min(int(tlens[clip]), Tmax) if 0 <= clip < len(tlens) else 0


def src_step_reference(q, kv, clip_of, tlen, Tmax: int, H: int, scale: float):
    """fp64 statement of svsr_mha_src_step_fwd.  q [n, H * 64], kv [C * Tmax, >= 2 * H * 64] (k | v per row; only frames below
    min(tlen, Tmax) of a clip and only the first 2 * H * 64 columns are touched), clip_of [n], tlen [C] -> (ctx [n, H * 64],
    A [n, H * 64] = sum_k p_k |v_k|: the scale of the terms each output adds up).  A row whose clip is outside [0, C) or has no frame: zeros."""
    n, D = len(clip_of), H * 64
    ctx = torch.zeros((n, D), dtype=torch.float64)
    A = torch.zeros((n, D), dtype=torch.float64)
    for r in range(n):
        c = int(clip_of[r])
        T = _frames(c, tlen, Tmax)
        if T < 1:
            continue
        rows = kv[c * Tmax : c * Tmax + T].double()
        for h in range(H):
            k, v = rows[:, h * 64 : (h + 1) * 64], rows[:, D + h * 64 : D + (h + 1) * 64]
            s = (k @ q[r, h * 64 : (h + 1) * 64].double()) * scale
            p = torch.exp(s - s.max())
            p = p / p.sum()
            ctx[r, h * 64 : (h + 1) * 64] = p @ v
            A[r, h * 64 : (h + 1) * 64] = p @ v.abs()
    return ctx, A


def src_step_case(seed: int, H: int, Tmax: int, tlens, clip_of, scale: float = 0.125):
    """bf16 inputs of one source-attention case -> dict(q_wide [n, 3D] (the query is columns D .. 2D), kv [C * Tmax, 2D + 8], clip_of, tlens,
    Tmax, H, scale, peaks).  q ~ N(0, 1), k ~ 0.5 N(0, 1), v ~ N(0, 1); frames past a clip's length and the 8 columns behind k | v are NaN.
    Every live row but the last one has, per head, one PEAK key k = (12 / scale) q / |q|^2 at a frame of its clip (the rows of a clip take
    T - 1, 0, 63, 64, T // 2 in turn, clamped to T - 1): it scores 12 against about N(0, 1/4) for the others, so the output is essentially
    that frame's value and a chunk that is mis-weighted, dropped or read at the wrong frame shows.  The last row attends diffusely."""
    g = torch.Generator().manual_seed(seed)
    n, C, D = len(clip_of), len(tlens), H * 64
    q_wide = torch.randn(n, 3 * D, generator=g).to(BF16)
    kv = torch.full((C * Tmax, 2 * D + SRC_STEP_KV_PAD), float("nan"))
    for c in range(C):
        T = _frames(c, tlens, Tmax)
        kv[c * Tmax : c * Tmax + T, :D] = 0.5 * torch.randn(T, D, generator=g)
        kv[c * Tmax : c * Tmax + T, D : 2 * D] = torch.randn(T, D, generator=g)
    q = q_wide[:, D : 2 * D].float()
    peaks, turn = {}, {}
    for r in range(n - 1 if n > 1 else 1):
        c = int(clip_of[r])
        T = _frames(c, tlens, Tmax)
        if T < 1:
            continue
        j = turn.get(c, 0)
        turn[c] = j + 1
        p = min((T - 1, 0, 63, 64, T // 2)[j % 5], T - 1)
        peaks[r] = p
        for h in range(H):
            qh = q[r, h * 64 : (h + 1) * 64]
            kv[c * Tmax + p, h * 64 : (h + 1) * 64] = (SRC_STEP_PEAK / scale) * qh / float(qh.square().sum())
    return dict(q_wide=q_wide, kv=kv.to(BF16), clip_of=[int(c) for c in clip_of], tlens=[int(t) for t in tlens], Tmax=Tmax, H=H, scale=scale,
                peaks=peaks)


@functools.lru_cache(maxsize=None)
def src_step_shape(name: str):
    """-> (case, ctx fp64, A fp64) of SRC_STEP_SHAPES[name]; built once per process, shared and never written."""
    seed, H, Tmax, tlens, clip_of = SRC_STEP_SHAPES[name]
    case = src_step_case(seed, H, Tmax, tlens, clip_of)
    D = H * 64
    want, A = src_step_reference(case["q_wide"][:, D : 2 * D], case["kv"], case["clip_of"], case["tlens"], Tmax, H, case["scale"])
    return case, want, A


def src_step_dead_rows(case) -> list:
    return [r for r, c in enumerate(case["clip_of"]) if _frames(c, case["tlens"], case["Tmax"]) < 1]


def src_step_ratio(got, want, A) -> float:
    """max over the elements of |got - want| / (2^-8 |want| + 2^-10 A): two half-ulps of the bf16 result, and the fp32 error of the scores and
    of exp (about 1e-4 relative on the weights at scores of magnitude 12) on the scale of the terms added up.  An element whose bound is 0
    (a dead row) must be exact: any error there is an infinite ratio."""
    err = (got.double() - want).abs()
    bound = want.abs() * 2.0 ** -8 + A * 2.0 ** -10
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    return float(ratio.max())


def src_step_chunked_fp32(q, kv, clip_of, tlen, Tmax: int, H: int, scale: float, skip_rescale: bool = False, drop_partial_tail: bool = False):
    """The kernel's arithmetic restated in fp32 torch: keys in chunks of 64, running maximum m, l and acc rescaled by exp(m - m_new), values
    of a chunk added with the chunk's weights, the quotient rounded to bf16.  skip_rescale: l and acc of the earlier chunks keep their old
    scale (corr = 1).  drop_partial_tail: a chunk of fewer than 64 keys adds the values of all but its last key.  Both are WRONG on
    purpose: the tests show that the cases tell them from the right one."""
    n, D = len(clip_of), H * 64
    out = torch.zeros((n, D), dtype=BF16)
    f32 = torch.float32
    for r in range(n):
        c = int(clip_of[r])
        T = _frames(c, tlen, Tmax)
        if T < 1:
            continue
        rows = kv[c * Tmax : c * Tmax + T].to(f32)
        for h in range(H):
            qh = q[r, h * 64 : (h + 1) * 64].to(f32)
            m, l, acc = torch.tensor(float("-inf")), torch.zeros((), dtype=f32), torch.zeros(64, dtype=f32)
            for k0 in range(0, T, 64):
                cnt = min(64, T - k0)
                s = (rows[k0 : k0 + cnt, h * 64 : (h + 1) * 64] @ qh) * scale
                mn = torch.maximum(m, s.max())
                corr = torch.ones((), dtype=f32) if (skip_rescale and k0 > 0) else torch.exp(m - mn)
                p = torch.exp(s - mn)
                l = l * corr + p.sum()
                use = cnt - 1 if (drop_partial_tail and cnt < 64) else cnt
                acc = acc * corr + p[:use] @ rows[k0 : k0 + use, D + h * 64 : D + (h + 1) * 64]
                m = mn
            out[r, h * 64 : (h + 1) * 64] = (acc / l).to(BF16)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# selection
# ----------------------------------------------------------------------------------------------------------------------
BEAM_WEIGHTS = (0.9, 0.1, 0.3, -0.2)


def beam_layout(rows, V: int, beam: int):
    """rows per clip -> (row_lo [C + 1], out_off [C], out_rows)"""
    row_lo, out_off, o = [0], [], 0
    for r in rows:
        row_lo.append(row_lo[-1] + r)
        out_off.append(o)
        o += min(beam, r * V)
    return row_lo, out_off, o


def beam_planes(seed: int, n: int, V: int, nplanes: int, ld: int = 0):
    """The planes of test_beam_select_kernel_equals_its_torch_statement — log-probability-like on a coarse grid (exact ties among the best), a
    CTC-like plane that is LOGZERO outside a few candidates, a quarter-grid plane — and a fourth coarse-grid plane that enters with a negative
    weight; the first `nplanes` of them, fp32 [n, max(ld, V)], with their weights and the running scores.  Columns V .. of a wider pitch
    hold NaN in plane 0 and +inf in the others: nothing may read them."""
    g = torch.Generator().manual_seed(seed)
    planes = [-torch.randint(0, 40, (n, V), generator=g).float() * 0.25, torch.full((n, V), LOGZERO), (-torch.rand(n, V, generator=g) * 8 * 4).round() / 4,
              -torch.randint(0, 4, (n, V), generator=g).float() * 0.5]
    live = torch.rand(n, V, generator=g) < (0.9 if V < 100 else 0.01)
    planes[1][live] = -torch.randint(0, 16, (int(live.sum()),), generator=g).float() * 0.5
    run = -torch.randint(0, 6, (n,), generator=g).float() * 0.5
    planes = planes[:nplanes]
    if ld > V:
        wide = [torch.full((n, ld), float("nan") if i == 0 else float("inf")) for i in range(nplanes)]
        for w, p in zip(wide, planes):
            w[:, :V] = p
        planes = wide
    return planes, list(BEAM_WEIGHTS[:nplanes]), run


def beam_plant(planes, V: int, lo: int, flats, values) -> None:
    """Make the elements at flat indices `flats` of the clip that starts at row `lo` the clip's best: plane 0 takes `values` (far above the
    grid), the other planes 0 there."""
    f = torch.as_tensor(flats)
    r, v = lo + f // V, f % V
    planes[0][r, v] = torch.as_tensor(values, dtype=torch.float32)
    for p in planes[1:]:
        p[r, v] = 0.0


def beam_boundary_case(which: str):
    """V = 5049, beam = 40, a clip of 40 rows: slices of 2,048 elements, 99 of them, the last one of 1,256 -> (planes, weights, run, rows).
    'straddle': the 40 best share ONE total, twenty across f = 2047 | 2048 and twenty across 4095 | 4096 (all in row 0: one running score) —
                the ties come out in index order across three slices;
    'tail':     the 40 best inside the last, partial slice (some tied), so the merge takes every candidate of that slice;
    'head':     the 40 best inside slice 0, while the launch's other clip has no rows."""
    V, beam = 5049, 40
    rows = {"straddle": [40], "tail": [40], "head": [40, 0]}[which]
    planes, weights, run = beam_planes(77, 40, V, 3)
    N = 40 * V
    if which == "straddle":
        flats = list(range(2048 - 10, 2048 + 10)) + list(range(4096 - 10, 4096 + 10))
        values = [100.0] * 40
    elif which == "tail":
        last = (N - 1) // 2048 * 2048
        assert N - last == 1256 and last // V == (N - 1) // V                 # one row: one running score
        flats = [last + 3 + 31 * i for i in range(40)]
        values = [100.0 + (i * 7) % 11 for i in range(40)]
    else:
        flats = [5 + 51 * i for i in range(40)]
        assert flats[-1] < 2048
        values = [100.0 + (i * 5) % 13 for i in range(40)]
    beam_plant(planes, V, 0, flats, values)
    return planes, weights, run, rows, V, beam, flats


def beam_special_case(which: str):
    """One plane with NaN, +inf and -inf inside [0, V) of live clips (one plane: no inf - inf) -> (planes, weights, run, rows, V, beam).
    'all':  rows (3, 2) x 41 units at beam 256: every element is written, so the whole order shows — NaN first by index, +inf, the finite
            totals, -inf last;
    'wide': 40 rows x 5049 units at beam 40: the specials sit in different slices."""
    if which == "all":
        rows, V, beam = [3, 2], 41, 256
        spots = {"nan": [(0, 40), (2, 0), (1, 7), (4, 3)], "inf": [(0, 0), (2, 40), (3, 11)], "-inf": [(1, 0), (0, 39), (4, 40), (3, 0)]}
    else:
        rows, V, beam = [40], 5049, 40
        spots = {"nan": [(39, 5048), (0, 2047), (17, 100)], "inf": [(0, 2048), (25, 0)], "-inf": [(0, 0), (39, 5047), (20, 20)]}
    planes, weights, run = beam_planes(78, sum(rows), V, 1)
    for name, where in spots.items():
        for r, v in where:
            planes[0][r, v] = float(name)
    planes[0][spots["nan"][0]] = -float("nan")                                 # a NaN with the sign bit set is a NaN like the others
    return planes, weights, run, rows, V, beam


def beam_rank_key(total: torch.Tensor) -> torch.Tensor:
    """The rank of a total under the documented order as an integer: the monotone map of fp32 bits, NaN above everything."""
    u = total.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    return torch.where(torch.isnan(total), torch.full_like(key, 0xFFFFFFFF), key)


# name -> builder of (planes, weights, run, rows, V, beam): every edge case of the selection, shared by the GPU test and the CPU test of the
# reference's own order
BEAM_EDGE_CASES = {
    "planes1": lambda: beam_planes(71, 11, 300, 1) + ([1, 5, 2, 3], 300, 40),
    "planes2": lambda: beam_planes(72, 11, 300, 2) + ([1, 5, 2, 3], 300, 40),
    "planes4": lambda: beam_planes(73, 11, 300, 4) + ([1, 5, 2, 3], 300, 40),
    "planes4_5049": lambda: beam_planes(74, 57, 5049, 4) + ([40, 0, 17], 5049, 40),
    "pitch5056": lambda: beam_planes(75, 57, 5049, 3, ld=5056) + ([40, 0, 17], 5049, 40),
    "pitch48": lambda: beam_planes(76, 5, 41, 3, ld=48) + ([3, 2], 41, 256),
    "special_all": lambda: beam_special_case("all"),
    "special_wide": lambda: beam_special_case("wide"),
    "straddle": lambda: beam_boundary_case("straddle")[:6],
    "tail": lambda: beam_boundary_case("tail")[:6],
    "head": lambda: beam_boundary_case("head")[:6],
}


@functools.lru_cache(maxsize=None)
def beam_edge_case(name: str):
    """-> (planes, weights, run, rows, V, beam, want) with want = beam_select_reference on the CPU tensors; built once, never written."""
    from syncvsr_amd.lrs_infer import beam_select_reference

    planes, weights, run, rows, V, beam = BEAM_EDGE_CASES[name]()
    row_lo, _, _ = beam_layout(rows, V, beam)
    return planes, weights, run, rows, V, beam, beam_select_reference(planes, weights, run, row_lo, beam, V)


# ----------------------------------------------------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------------------------------------------------
def _take(states, keep: torch.Tensor):
    if states is None:
        return None
    if isinstance(states, tuple):
        return tuple(s[keep] for s in states)
    return states[keep]


def _single_clip_step(search, run: dict, x: torch.Tensor) -> dict:
    """One position: running = dict(yseq [n, L], score [n], scores {k: [n]}, states {k: batched state})."""
    yseq = run["yseq"]
    n, V = yseq.shape[0], search.n_vocab
    xs = x.unsqueeze(0).expand(n, *x.shape)
    weighted = torch.zeros((n, V), dtype=x.dtype, device=x.device)
    sc, st = {}, {}
    for k, d in search.full_scorers.items():
        sc[k], st[k] = d.batch_score(yseq, run["states"][k], xs)
        weighted += search.weights[k] * sc[k].to(x.dtype)
    part_ids = None
    if search.do_pre_beam:
        pre = weighted if search.pre_beam_score_key == "full" else sc[search.pre_beam_score_key]
        part_ids = torch.topk(pre, search.pre_beam_size, dim=-1)[1]
    for k, d in search.part_scorers.items():
        sc[k], st[k] = d.batch_score_partial(yseq, part_ids, run["states"][k], x)
        weighted += search.weights[k] * sc[k].to(x.dtype)
    weighted += run["score"].to(x.dtype).unsqueeze(1)
    top = weighted.view(-1).topk(min(search.beam_size, n * V))[1]
    prev, tok = torch.div(top, V, rounding_mode="trunc"), top % V
    return dict(
        yseq=torch.cat((yseq[prev], tok.unsqueeze(1)), dim=1),
        score=weighted[prev, tok],
        scores={k: run["scores"][k][prev] + sc[k][prev, tok].to(x.dtype) for k in search.scorers},
        states={k: search.scorers[k].select_states(st[k], prev, tok) for k in search.scorers},
    )


def single_clip_search(search, x: torch.Tensor, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> list:
    """The statement of `BatchBeamSearch.forward`: x, the encoder output of ONE clip [T, D] -> ended hypotheses, best first
    (beam_search.py:333-405).  This is the loop `forward` ran while the package had a search per entry point, moved here as it was: `search`
    gives its weights, scorers and settings only, and the scorers are spoken to in the reference's single-clip protocol (`batch_init_state(x)`,
    `batch_score(ys, states, xs)` / `batch_score_partial(y, ids, state, x)`, `select_states`), torch.topk selects, and nothing of the
    multi-clip search runs."""
    from syncvsr_amd.lrs_infer import Hypothesis, end_detect

    if maxlenratio == 0:
        maxlen = x.shape[0]
    elif maxlenratio < 0:
        maxlen = -1 * int(maxlenratio)
    else:
        maxlen = max(1, int(maxlenratio * x.size(0)))
    run = dict(yseq=torch.tensor([[search.sos]], dtype=torch.int64, device=x.device), score=torch.zeros(1, dtype=x.dtype, device=x.device),
               scores={k: torch.zeros(1, dtype=x.dtype, device=x.device) for k in search.scorers},
               states={k: d.batch_init_state(x) for k, d in search.scorers.items()})
    ended: list = []
    for i in range(maxlen):
        run = _single_clip_step(search, run, x)
        n = run["yseq"].shape[0]
        if i == maxlen - 1:          # batch_beam_search.py:318-334: close every running hypothesis at the length limit
            run["yseq"] = torch.cat((run["yseq"], torch.full((n, 1), search.eos, dtype=torch.int64, device=x.device)), dim=1)
        is_eos = run["yseq"][:, -1] == search.eos
        scores_cpu = run["score"].tolist()
        for b in torch.nonzero(is_eos).view(-1).tolist():
            ended.append(Hypothesis(yseq=run["yseq"][b], score=scores_cpu[b], scores={k: float(v[b]) for k, v in run["scores"].items()}))
        keep = torch.nonzero(~is_eos).view(-1)
        run = dict(yseq=run["yseq"][keep], score=run["score"][keep], scores={k: v[keep] for k, v in run["scores"].items()},
                   states={k: _take(v, keep) for k, v in run["states"].items()})
        if maxlenratio == 0.0 and end_detect([dict(score=h.score, yseq=h.yseq) for h in ended], i):
            break
        if keep.numel() == 0:
            break
    nbest = sorted(ended, key=lambda h: h.score, reverse=True)
    if not nbest:                      # beam_search.py:383-392
        return [] if minlenratio < 0.1 else single_clip_search(search, x, maxlenratio, max(0.0, minlenratio - 0.1))
    return nbest
