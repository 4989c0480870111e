"""Memory-safety pass over CTC forced alignment (-m gpu): the kernel tests of tests/test_gpu_ctc_align.py again in child pytest processes
under the two allocators of tests/conftest.py (see tests/test_gpu_redzone.py) — SVSR_REDZONE=1 (poisoned red zones around every tensor: a
stray STORE fails the test that made it) and SVSR_TAILFLUSH=1 (every tensor ends against an unmapped page: a READ behind it ends the child in
the test that made it).  svsr_ctc_align reaches logp through a label (ids of V, -7 and 2^32 + 5 are among the cases), the back-pointer
workspace through (frame, state) with an odd row of 2 Lmax + 1 bytes, and frames / spans through the walked path, at 41 and 5,049 units, 1
to 261 states, clips of 1 to 160 frames shorter than the padded batch."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILE = os.path.join(HERE, "test_gpu_ctc_align.py")
KERNEL_TESTS = "test_kernel"


def _run(env_key: str):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE, os.environ.get("PYTHONPATH", "")]))
    env.pop("SVSR_REDZONE", None)
    env.pop("SVSR_TAILFLUSH", None)
    env[env_key] = "1"
    cmd = [sys.executable, "-m", "pytest", "-v", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", KERNEL_TESTS, FILE]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if "::" in ln]
    tail = "last test line: " + (lines[-1] if lines else "(none)") + "\n" + r.stdout[-2500:] + "\n" + r.stderr[-2500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " skipped" not in r.stdout.strip().splitlines()[-1] and "redzone" not in r.stderr, tail
    print(r.stdout.strip().splitlines()[-1])


def test_alignment_kernel_passes_with_red_zones_around_every_tensor():
    _run("SVSR_REDZONE")


def test_alignment_kernel_passes_with_every_tensor_flush_against_an_unmapped_page():
    _run("SVSR_TAILFLUSH")
