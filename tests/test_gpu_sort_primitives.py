"""The device primitives under every kernel chain, pinned directly: launch_radix_sort_u64 (one-launch and three-launch passes),
launch_radix_sort_u64_devn, launch_exclusive_sum_u32 (kernels/sort.hip) and launch_prefix_max (kernels/depth.hip) against plain numpy
references, at the sizes where their tiling or algorithm changes (tests/sort_primitives_inputs.py; shown not to be vacuous by
tests/test_sort_primitives_inputs.py). The hooks live in libcsvgpu_testhooks.so only: each section runs in a child process that loads
that build (CSVGPU_LIB) and executes tests/sort_primitives_check.py. Every sort also asserts CSV_OK, a clear look-back flag and
untouched slots behind the first n of all four buffers."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(section):
    env = dict(os.environ, CSVGPU_LIB=os.path.join(ROOT, "contextsv_amd", "lib", "libcsvgpu_testhooks.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sort_primitives_check.py"), section], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-3000:])


def test_radix_sort_both_modes_at_every_tile_size():
    _run("sort")


def test_radix_sort_with_the_count_on_the_device():
    """Also: an n_bound of 2^30 or more is refused (CSV_EINVAL) by the launcher, before anything is staged or launched."""
    _run("sort_devn")


def test_exclusive_sum_on_every_path():
    _run("exclusive_sum")


def test_prefix_max_through_the_spine_s_second_loop():
    _run("prefix_max")
