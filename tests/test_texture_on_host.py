"""The textured resolve's kernels EXECUTED ON THE HOST (tests/host_exec/, see tests/test_kernels_on_host.py) in the `-m "not gpu"`
tier: the texture and Phong tests of tests/test_gpu_texture.py and ALL of tests/test_gpu_texture_edges.py (the colour of a hit pixel
against the fp64 reference at its edges: no case of it is larger than 64 x 80), UNMODIFIED, in a subprocess under the plugin
tests/host_exec/pytest_hostexec.py.  Mutation record of the second module: profiles/texture_edges_mutation.txt."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))

G = "tests/test_gpu_texture.py::"
SELECT = [G + "test_linear_texture_unshaded_is_exact_at_the_surface_point",
          G + "test_texel_centres_reproduce_texels_and_outside_uvs_take_the_border",
          G + "test_textured_phong_matches_texture_ref", G + "test_phong_on_untextured_mesh_matches_texture_ref",
          G + "test_textured_flat_shading_matches_texture_ref", G + "test_vertex_colour_entry_point_unchanged_next_to_a_textured_mesh",
          "tests/test_gpu_texture_edges.py"]
EXPECTED = 6 + 149                          # (the six above + every case of the edge module: counts only go up)


def test_texture_gpu_tests_pass_on_the_host_executed_kernels(tmp_path_factory):
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
