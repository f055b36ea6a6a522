"""The LINEMOD metric kernels (csrc/eval_metrics.hip: rnnpose_nn_search_f32, rnnpose_pose_metrics_f64, findNearestPointIdxLauncher)
EXECUTED ON THE HOST (tests/host_exec/, see tests/test_kernels_on_host.py) in the `-m "not gpu"` tier: tests/test_gpu_eval_edges.py,
UNMODIFIED, in a subprocess under the plugin tests/host_exec/pytest_hostexec.py.  Nothing is left to the GPU: the largest launch is
2049 x 513 distances in three batch elements, the module has no large shapes, renders nothing and captures no graph, and the drop-in
symbol's hipMalloc / hipMemcpy are host allocations and copies there.  What host mode cannot show is the device's own arithmetic (its
acos, sqrt and divide, and whether the device compiler contracts): the MI355X run of the same module is what pins those
(profiles/eval_edges_mutation.txt has both tables)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))

# nn_search cases, planted winners, exclude_self, contraction clouds, non-finite input, the host-pointer launcher; pose_metrics cases x 2,
# batch independence x 2, planted rotations x 2, symmetric cloud, NaN pose x 2, depth 0; C-ABI refusals, front-end refusals; evaluator x 2
EXPECTED = 13 + 4 + 6 + 2 + 1 + 1 + 10 * 2 + 2 + 2 + 1 + 2 + 1 + 1 + 1 + 2


def test_eval_edge_tests_pass_on_the_host_executed_kernels(tmp_path_factory):
    import build_host
    try:
        build_host.clang()
    except RuntimeError as e:
        pytest.skip(str(e))
    lib = build_host.build(str(tmp_path_factory.mktemp("host_exec")))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + ROOT, HOSTEXEC_DIR=os.path.dirname(lib))
    cmd = [sys.executable, "-m", "pytest", "-p", "host_exec.pytest_hostexec", "-m", "gpu", "-q", "-p", "no:cacheprovider", "tests/test_gpu_eval_edges.py"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = r.stdout[-3000:]
    m = re.search(r"(\d+) passed", tail)
    assert r.returncode == 0 and m and " failed" not in tail.splitlines()[-1], tail
    assert int(m.group(1)) == EXPECTED, tail
