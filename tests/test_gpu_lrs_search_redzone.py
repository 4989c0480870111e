"""Memory-safety pass over the multi-clip search (-m gpu): the kernel tests of tests/test_gpu_lrs_search_clips.py again in child pytest
processes under the two allocators of tests/conftest.py (see tests/test_gpu_redzone.py) — SVSR_REDZONE=1 (poisoned red zones around every
tensor: a stray STORE fails the test that made it) and SVSR_TAILFLUSH=1 (every tensor ends against an unmapped page: a READ behind it ends
the child in the test that made it).  All three entry points reach their operands through computed indices (row -> clip -> frame block,
flat index -> (row, token), output offsets), at shapes that are no multiples of the 64-lane waves, the 256-thread workgroups or the
slices: 41 and 5,049 units, 1 to 40 rows per clip, clips of 1, 5, 9, 37 frames; source attention over clips of 1 to 150 frames (partial last
chunks of keys, a length above Tmax, rows without a clip), plane pitches wider than V, candidate ids far outside the vocabulary."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILE = os.path.join(HERE, "test_gpu_lrs_search_clips.py")
KERNEL_TESTS = "beam_select or ctc_prefix_clips or mha_src_step or decoder_step or tiny_model"


def _run(env_key: str):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE, os.environ.get("PYTHONPATH", "")]))
    env.pop("SVSR_REDZONE", None)
    env.pop("SVSR_TAILFLUSH", None)
    env[env_key] = "1"
    cmd = [sys.executable, "-m", "pytest", "-v", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", KERNEL_TESTS, FILE]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    lines = [ln for ln in r.stdout.splitlines() if "::" in ln]
    tail = "last test line: " + (lines[-1] if lines else "(none)") + "\n" + r.stdout[-2500:] + "\n" + r.stderr[-2500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " skipped" not in r.stdout.strip().splitlines()[-1] and "redzone" not in r.stderr, tail
    print(r.stdout.strip().splitlines()[-1])


def test_search_kernels_pass_with_red_zones_around_every_tensor():
    _run("SVSR_REDZONE")


def test_search_kernels_pass_with_every_tensor_flush_against_an_unmapped_page():
    _run("SVSR_TAILFLUSH")
