"""The top-K RANSAC kernels (csrc/pnp_topk.cuh through the entry point in csrc/eval_metrics.hip) EXECUTED ON THE HOST
(tests/host_exec/, see tests/test_kernels_on_host.py) in the `-m "not gpu"` tier: every case of tests/test_gpu_pnp_topk.py except the
end-to-end ones (they render, refine and score on the device) and the dispatcher one (the host tensors are CPU tensors), UNMODIFIED,
in a subprocess under the plugin tests/host_exec/pytest_hostexec.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))

SELECT_K = "not end_to_end and not torch_ops"
EXPECTED = 4 * 4 + 4 + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 1      # the grid, slot 0 per Kt, every slot, two modes, gates, fewer modes, degenerate, one optimum, reruns / batch, bad arguments, ops refusals


def test_pnp_topk_gpu_tests_pass_on_the_host_executed_kernels(tmp_path_factory):
    import build_host
    try:
        build_host.clang()
    except RuntimeError as e:
        pytest.skip(str(e))
    lib = build_host.build(str(tmp_path_factory.mktemp("host_exec")))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + ROOT, HOSTEXEC_DIR=os.path.dirname(lib))
    cmd = [sys.executable, "-m", "pytest", "-p", "host_exec.pytest_hostexec", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-k", SELECT_K,
           "tests/test_gpu_pnp_topk.py"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = r.stdout[-3000:]
    m = re.search(r"(\d+) passed", tail)
    assert r.returncode == 0 and m and " failed" not in tail.splitlines()[-1], tail
    assert int(m.group(1)) == EXPECTED, tail
