"""The indexed zoom crop and the renderer's resident attribute tables EXECUTED ON THE HOST (tests/host_exec/, see
tests/test_kernels_on_host.py) in the `-m "not gpu"` tier: the crop and table tests of tests/test_gpu_scene.py, UNMODIFIED, in a
subprocess under the plugin tests/host_exec/pytest_hostexec.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))

G = "tests/test_gpu_scene.py::"
SELECT = [G + "test_indexed_crop_with_identity_index_equals_plain_crop_bitwise",
          G + "test_indexed_crop_equals_crop_of_the_gathered_copy",
          G + "test_indexed_crop_matches_torch_grid_sample_on_the_cpu",
          G + "test_indexed_crop_refuses_an_index_out_of_range_before_launching",
          G + "test_resident_attribute_tables_equal_the_explicit_list_bitwise"]
EXPECTED = 6 + 3 + 1 + 1 + 2          # parametrised cases


def test_scene_gpu_tests_pass_on_the_host_executed_kernels(tmp_path_factory):
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
