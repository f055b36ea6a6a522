"""The object onboarding kernels (csrc/model_prep.cuh through the entry points in csrc/eval_metrics.hip) EXECUTED ON THE HOST
(tests/host_exec/, see tests/test_kernels_on_host.py) in the `-m "not gpu"` tier: every case of tests/test_gpu_model_prep.py except the
end-to-end one (it runs the KPConv networks and renders on the device) and the torch-op one (the dispatcher's CUDA key has no tensors
there), UNMODIFIED, in a subprocess under the plugin tests/host_exec/pytest_hostexec.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))

SELECT_K = "not end_to_end and not torch_ops"
# the diameter grid, its batch / ties / non-finite cases; FPS: lattice starts, duplicates, workgroup edges, batch + reruns, random sets;
# the reference's fragments; bad arguments, ops refusals
EXPECTED = 8 * 3 + 1 + 1 + 1 + 4 + 1 + 6 + 1 + 3 + 1 + 1 + 1


def test_model_prep_gpu_tests_pass_on_the_host_executed_kernels(tmp_path_factory):
    import build_host
    try:
        build_host.clang()
    except RuntimeError as e:
        pytest.skip(str(e))
    lib = build_host.build(str(tmp_path_factory.mktemp("host_exec")))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + ROOT, HOSTEXEC_DIR=os.path.dirname(lib))
    cmd = [sys.executable, "-m", "pytest", "-p", "host_exec.pytest_hostexec", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-k", SELECT_K,
           "tests/test_gpu_model_prep.py"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = r.stdout[-3000:]
    m = re.search(r"(\d+) passed", tail)
    assert r.returncode == 0 and m and " failed" not in tail.splitlines()[-1], tail
    assert int(m.group(1)) == EXPECTED, tail
