"""SuperPoint2D's kernels EXECUTED ON THE HOST (tests/host_exec/, see tests/test_kernels_on_host.py) in the `-m "not gpu"` tier: the
glue-kernel tests of tests/test_gpu_desc2d.py and its fixture-parity test on case b (B = 1, 40 x 56: the whole network, every
convolution on the strip kernels), UNMODIFIED, in a subprocess under the plugin tests/host_exec/pytest_hostexec.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))

SELECT = ["tests/test_gpu_desc2d.py::test_desc2d_matches_the_reference_fixture[b]", "tests/test_gpu_desc2d.py::test_maxpool2x2_is_max_pool2d",
          "tests/test_gpu_desc2d.py::test_upsample2x_is_interpolate", "tests/test_gpu_desc2d.py::test_pixel_head_vs_fp64"]
EXPECTED = 1 + 3 + 6 + 9


def test_desc2d_gpu_tests_pass_on_the_host_executed_kernels(tmp_path_factory):
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
