"""The occlusion pass between the objects of one frame (csrc/raster.hip, rnnpose_raster_occlusion_f32) EXECUTED ON THE HOST
(tests/host_exec/, see tests/test_kernels_on_host.py) in the `-m "not gpu"` tier: tests 1-6 of tests/test_gpu_occlusion.py -- the ray
caster cases, the coincident twin, the closed form, frames, ties and the edges of the pass -- UNMODIFIED, in a subprocess under the
plugin tests/host_exec/pytest_hostexec.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))

G = "tests/test_gpu_occlusion.py::"
SELECT = [G + "test_occlusion_against_the_ray_caster",
          G + "test_a_coincident_twin_hides_nothing",
          G + "test_two_fronto_parallel_quads",
          G + "test_objects_of_another_frame_neither_hide_nor_are_hidden",
          G + "test_coincident_occluders_resolve_to_the_lower_index",
          G + "test_an_occluder_that_contributes_no_face_hides_nothing",
          G + "test_an_occluder_across_the_near_plane_agrees_with_the_ray_caster",
          G + "test_no_pairs_gives_the_own_coverage",
          G + "test_depth_inout_changes_the_occluded_pixels_only",
          G + "test_bad_pairs_raise_on_the_host_before_any_launch",
          G + "test_bad_pairs_through_the_c_abi_write_nothing",
          G + "test_occluder_keys_equal_the_own_keys_of_the_occluder_under_the_same_window"]
EXPECTED = 4 + 1 + 4 + 1 + 2 + 2 + 1 + 1 + 1 + 1 + 1 + 1      # parametrised cases


def test_occlusion_gpu_tests_pass_on_the_host_executed_kernels(tmp_path_factory):
    import build_host
    try:
        build_host.clang()
    except RuntimeError as e:
        pytest.skip(str(e))
    lib = build_host.build(str(tmp_path_factory.mktemp("host_exec")))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + ROOT, HOSTEXEC_DIR=os.path.dirname(lib))
    cmd = [sys.executable, "-m", "pytest", "-p", "host_exec.pytest_hostexec", "-m", "gpu", "-q", "-p", "no:cacheprovider"] + SELECT
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = r.stdout[-3000:]
    m = re.search(r"(\d+) passed", tail)
    assert r.returncode == 0 and m and " failed" not in tail.splitlines()[-1], tail
    assert int(m.group(1)) == EXPECTED, tail
