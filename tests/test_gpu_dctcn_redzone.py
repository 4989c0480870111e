"""Memory-safety pass over the DC-TCN back-end (-m gpu): tests/test_gpu_dctcn_kernels.py and the tiny model cases again in child pytest processes under the two
allocators of tests/conftest.py (see tests/test_gpu_redzone.py) — SVSR_REDZONE=1 (poisoned red zones around every tensor: a stray STORE
fails the test that made it) and SVSR_TAILFLUSH=1 (every tensor ends against an unmapped page: a READ behind it ends the child in the test
that made it).  The halo rows of a time tile, the channel prefix read through the row pitch and the channel offset of the output are all
computed addresses: exactly where an out-of-bounds access hides.  (The full-size model case is left to the plain run: the two allocators make its front-end slow.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILES = [os.path.join(HERE, "test_gpu_dctcn_kernels.py"), os.path.join(HERE, "test_gpu_dctcn_model.py")]


def _run(env_key: str):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE, os.environ.get("PYTHONPATH", "")]))
    env.pop("SVSR_REDZONE", None)
    env.pop("SVSR_TAILFLUSH", None)
    env[env_key] = "1"
    cmd = [sys.executable, "-m", "pytest", "-v", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not dctcn_full", *FILES]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    lines = [ln for ln in r.stdout.splitlines() if "::" in ln]
    tail = "last test line: " + (lines[-1] if lines else "(none)") + "\n" + r.stdout[-2500:] + "\n" + r.stderr[-2500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " skipped" not in r.stdout.strip().splitlines()[-1] and "redzone" not in r.stderr, tail
    print(r.stdout.strip().splitlines()[-1])


def test_dctcn_tests_pass_with_red_zones_around_every_tensor():
    _run("SVSR_REDZONE")


def test_dctcn_tests_pass_with_every_tensor_flush_against_an_unmapped_page():
    _run("SVSR_TAILFLUSH")
