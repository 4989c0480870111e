"""Records tests/golden/adamw_bits.npz: the bits the four AdamW entry points of the C ABI (svsr_adamw_step, svsr_adamw_range,
svsr_adamw_onecycle_step, svsr_adamw_onecycle_range) leave in the parameters, both moments, the bf16 shadow and the scalar words of the
device state, step by step, on the library that is loaded.  tests/test_gpu_adamw_bits.py runs the same cases (it imports this file) and
compares.  Needs the GPU:

    python tests/golden/make_golden_adamw_bits.py [path]

Nothing but the C ABI is used, so the same file records on any commit whose library exports the four symbols: the golden was recorded on the
build BEFORE the two update kernels became one body with two schedule policies, and that change was required to reproduce it.

Cases: n in {1, 255, 4*256+3, 4096*256+5} (one element; a ragged block; several blocks; past the 4096-block grid cap) x decay_end in
{0, n // 2, n} x five schedules x max_norm in {1, 0}.  Schedules: `const` (total_steps = 0) and `cosine` (warm-up 2, total_steps 6: the
seventh step lands past the schedule's end) through svsr_adamw_*; `oc_cos` (pct_start 0.3), `oc_cos0` (pct_start 0) and `oc_lin3` (linear,
three_phase), all total_steps 7, through svsr_adamw_onecycle_*.

One case is seven counted steps with gradient scales (3, 0.01, 1, 0.3, 2, 0.05, 1), each behind svsr_grad_sumsq.  Steps 0, 1, 3, 5, 6 are one
`_step` call.  Step 2 is three `_range` calls whose cut points are no multiples of four, the last one advancing.  Step 4 is one `_range` call
over everything that does not advance and one with n = 0 that does.  Between steps 3 and 4 one step has a single inf among its gradients: the
driver asserts that it writes nothing and that `skipped` counts it.  Behind the seven, the OneCycle schedules get one step past total_steps:
nothing written, the error word set.  A record is taken behind every one of these.

The buffers carry eight sentinel elements behind their n, which the driver checks after every launch.  The file keeps, per (n, entry-point
family): the SHA-256 of the inputs, the state's scalar words of every record, and of the seven counted steps either the arrays (n <= 255)
or one SHA-256 per tensor per step (the arrays of n = 4*256+3 alone would come to 3 MiB, three times what a committed file may hold).
Inputs are integer draws of seeded CPU generators (fp32 = integer / 2^23), the same bits on any host."""
import hashlib
import os
import struct
import sys
from functools import lru_cache

import numpy as np
import torch

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adamw_bits.npz")
SIZES = (1, 255, 4 * 256 + 3, 4096 * 256 + 5)
CUTS = {1: (0, 1), 255: (85, 170), 4 * 256 + 3: (341, 686), 4096 * 256 + 5: (349527, 699054)}       # step 2's ranges: [0, a) [a, b) [b, n)
DECAY = {"d0": lambda n: 0, "dhalf": lambda n: n // 2, "dn": lambda n: n}
SCALES = (3.0, 0.01, 1.0, 0.3, 2.0, 0.05, 1.0)
ARRAYS_UP_TO = 255
GUARD, SENT = 8, 7.0
PARTS = 1024                                              # partial sums between the state's first four scalar words and its last four
COSINE = {"const": dict(lr=1e-2, beta1=0.9, beta2=0.98, eps=1e-6, wd=0.03, warmup=0, total_steps=0),
          "cosine": dict(lr=1e-2, beta1=0.9, beta2=0.98, eps=1e-6, wd=0.03, warmup=2, total_steps=6)}
ONECYCLE = {"oc_cos": dict(pct_start=0.3, cos=1, three_phase=0), "oc_cos0": dict(pct_start=0.0, cos=1, three_phase=0),
            "oc_lin3": dict(pct_start=0.3, cos=0, three_phase=1)}
OC_HP = dict(max_lr=1e-2, beta2=0.999, eps=1e-6, wd=1e-2, total_steps=7, div_factor=25.0, final_div_factor=1e4, base_momentum=0.85,
             max_momentum=0.95)
TENSORS = ("p", "m", "v", "shadow")


def family(sched: str) -> str:
    return "oc" if sched in ONECYCLE else "cos"


def case_name(n, dec, sched, max_norm) -> str:
    return f"n{n}_{dec}_{sched}_mn{int(max_norm)}"


CASES = {case_name(n, dec, sched, mn): (n, dec, sched, mn)
         for n in SIZES for dec in DECAY for sched in (*COSINE, *ONECYCLE) for mn in (1.0, 0.0)}


def group_of(name: str) -> str:
    n, _, sched, _ = CASES[name]
    return f"n{n}.{family(sched)}"


def group_cases(group: str) -> list:
    return [c for c in CASES if group_of(c) == group]


GROUPS = sorted({group_of(c) for c in CASES})


def _unit(g, *shape):
    """fp32 in (0, 1): integer / 2^23 (exact)."""
    return torch.randint(1, 1 << 23, shape, generator=g).float() / float(1 << 23)


@lru_cache(maxsize=None)
def inputs(n: int):
    """-> (p0 [n], gradients [9][n]: the seven counted steps', the inf step's, the step's past the schedule; SHA-256 of all of it)."""
    g = torch.Generator().manual_seed(1000 + SIZES.index(n))
    p0 = _unit(g, n) - 0.5
    grads = [(_unit(g, n) - 0.5) * 2.0 * s for s in SCALES]
    bad = _unit(g, n) - 0.5
    bad[n // 2] = float("inf")
    grads += [bad, _unit(g, n) - 0.5]
    h = hashlib.sha256(p0.numpy().tobytes())
    for t in grads:
        h.update(t.numpy().tobytes())
    return p0, grads, np.frombuffer(h.digest(), dtype=np.uint8).copy()


def onecycle_record(sched: str):
    """The 64-byte host record svsr_onecycle_t: six doubles, four ints."""
    s = ONECYCLE[sched]
    initial = OC_HP["max_lr"] / OC_HP["div_factor"]
    raw = struct.pack("<6d4i", OC_HP["max_lr"], initial, initial / OC_HP["final_div_factor"], OC_HP["base_momentum"], OC_HP["max_momentum"],
                      s["pct_start"], s["three_phase"], s["cos"], OC_HP["total_steps"], 0)
    assert len(raw) == 64
    import ctypes

    return (ctypes.c_uint8 * 64).from_buffer_copy(raw)


def _raw(t: torch.Tensor) -> bytes:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()


def run_case(lib, name: str) -> dict:
    """-> {"state": int32 [records][words], and per tensor either int32 / int16 [7][n] or uint8 [7][32] digests (n > ARRAYS_UP_TO)}."""
    n, dec, sched, max_norm = CASES[name]
    oc = sched in ONECYCLE
    decay_end = DECAY[dec](n)
    p0, grads, _ = inputs(n)
    buf = {k: torch.full((n + GUARD,), SENT if k == "p" else 0.0, device=DEV) for k in ("p", "m", "v")}
    buf["p"][:n] = p0.to(DEV)
    buf["m"][n:] = SENT
    buf["v"][n:] = SENT
    buf["shadow"] = torch.full((n + GUARD,), SENT, dtype=torch.bfloat16, device=DEV)
    g = torch.empty(n, device=DEV)
    state = torch.zeros(4 + PARTS + (4 if oc else 0), dtype=torch.int32, device=DEV)
    rec = onecycle_record(sched) if oc else None
    hp = None if oc else COSINE[sched]

    def launch(lo, hi, advance, whole_step=False):
        ptr = [buf[k].data_ptr() + buf[k].element_size() * lo for k in ("p", "m", "v", "shadow")]
        head = (ptr[0], g.data_ptr() + 4 * lo, ptr[1], ptr[2], ptr[3], hi - lo, min(max(decay_end - lo, 0), hi - lo))
        if oc:
            mid = (OC_HP["beta2"], OC_HP["eps"], OC_HP["wd"], max_norm, rec, state.data_ptr())
            fn = lib.svsr_adamw_onecycle_step if whole_step else lib.svsr_adamw_onecycle_range
        else:
            mid = (hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], max_norm, hp["warmup"], hp["total_steps"], state.data_ptr())
            fn = lib.svsr_adamw_step if whole_step else lib.svsr_adamw_range
        rc = fn(*head, *mid, None) if whole_step else fn(*head, *mid, int(advance), None)
        assert rc == 0, (name, rc)

    def step(grad, how):
        g.copy_(grad.to(DEV))
        assert lib.svsr_grad_sumsq(g.data_ptr(), n, state.data_ptr(), None) == 0
        if how == "step":
            launch(0, n, True, whole_step=True)
        elif how == "three":
            a, b = CUTS[n]
            launch(0, a, False)
            launch(a, b, False)
            launch(b, n, True)
        else:
            launch(0, n, False)
            launch(n, n, True)
        torch.cuda.synchronize()
        raw = {k: _raw(buf[k]) for k in TENSORS}
        for k in TENSORS:
            assert bool((buf[k][n:].float() == SENT).all()), f"{name}: {k} was written past its {n} elements"
        words = state.cpu()
        return raw, torch.cat([words[:4], words[4 + PARTS:]]).numpy()

    out = {k: [] for k in TENSORS}
    states = []

    def keep(raw):
        for k in TENSORS:
            if n <= ARRAYS_UP_TO:
                out[k].append(np.frombuffer(raw[k], dtype=np.int16 if k == "shadow" else np.int32)[:n].copy())
            else:
                out[k].append(np.frombuffer(hashlib.sha256(raw[k]).digest(), dtype=np.uint8).copy())

    last = None
    for i in range(7):
        raw, words = step(grads[i], {2: "three", 4: "empty_advance"}.get(i, "step"))
        assert words[0] == i + 1 and words[1] == (i > 3), (name, i, words)
        keep(raw)
        states.append(words)
        last = raw
        if i == 3:                                     # a gradient norm that is not finite: nothing written, counted in `skipped`
            raw, words = step(grads[7], "step")
            assert raw == last, f"{name}: the step with an inf gradient wrote something"
            assert words[0] == 4 and words[1] == 1, (name, words)
            states.append(words)
    if oc:                                             # past total_steps: nothing written, the error word set
        raw, words = step(grads[8], "step")
        assert raw == last, f"{name}: the step past total_steps wrote something"
        assert words[0] == 7 and words[1] == 1 and words[5] == 1001, (name, words)
        states.append(words)
    res = {k: np.stack(v) for k, v in out.items()}
    res["state"] = np.stack(states).astype(np.int32)
    return res


def run_group(lib, group: str) -> dict:
    """-> the golden's keys of one (n, family): "<group>/cases", "/in", "/state" and the four tensors', a leading axis over the cases."""
    names = group_cases(group)
    runs = [run_case(lib, c) for c in names]
    got = {f"{group}/cases": np.array(names), f"{group}/in": inputs(CASES[names[0]][0])[2]}
    for k in (*TENSORS, "state"):
        got[f"{group}/{k}"] = np.stack([r[k] for r in runs])
    return got


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from syncvsr_amd import _lib

    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = {}
    for grp in GROUPS:
        rec.update(run_group(_lib.load(), grp))
    np.savez_compressed(path, **rec)
    print(f"recorded {len(CASES)} cases in {len(GROUPS)} groups -> {path} ({os.path.getsize(path)} bytes)")
