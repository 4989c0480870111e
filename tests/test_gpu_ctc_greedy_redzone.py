"""Memory-safety pass over CTC greedy decoding (-m gpu): the kernel tests of tests/test_gpu_ctc_greedy.py again in child pytest processes
under the two allocators of tests/conftest.py (see tests/test_gpu_redzone.py) — SVSR_REDZONE=1 (poisoned red zones around every tensor: a
stray STORE fails the test that made it) and SVSR_TAILFLUSH=1 (every tensor ends against an unmapped page: a READ behind it ends the child in
the test that made it).  svsr_ctc_frame_best reads rows of 1 to 8,191 units with 16-byte and single loads, at pitches equal to V and wider,
and must stop at column V and at frame tlen; svsr_ctc_collapse writes token rows counted by a prefix sum, up to one per frame (the capacity
itself) and with a capacity below the count, for clips of 0 to 2,048 frames."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILE = os.path.join(HERE, "test_gpu_ctc_greedy.py")
KERNEL_TESTS = "kernel"


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


def test_greedy_kernels_pass_with_red_zones_around_every_tensor():
    _run("SVSR_REDZONE")


def test_greedy_kernels_pass_with_every_tensor_flush_against_an_unmapped_page():
    _run("SVSR_TAILFLUSH")
