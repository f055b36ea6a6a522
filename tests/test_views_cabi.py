"""The grouped LM step at the C boundary (no GPU needed): rnnpose_lm_step_views_io_f32 is declared in include/rnnpose_hip.h, exported by
the library and typed in rnnpose_amd/_lib.py with the declared number of arguments; the ABI version stays 4 (an addition); the header
still compiles as strict C99; the host-side refusals come before any launch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = "rnnpose_lm_step_views_io_f32"


@pytest.fixture(scope="module")
def lib():
    from rnnpose_amd import build, _lib
    build.build()
    return _lib.load()


def _declaration():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnpose_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert m, f"{NAME} is not declared in the header"
    return [a.strip() for a in m.group(1).split(",")]


def test_views_symbol_declared_exported_and_typed(lib):
    from rnnpose_amd import _lib
    args = _declaration()
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    res, types = _lib.PROTOTYPES[NAME]
    assert res is C.c_int and len(types) == len(args) == 38
    # pointers, integers and floating-point arguments line up with the declaration
    for decl, t in zip(args, types):
        want = C.c_void_p if ("*" in decl or "rnnpose_stream_t" in decl) else C.c_size_t if decl.startswith("size_t") else \
            C.c_double if decl.startswith("double") else C.c_float if decl.startswith("float") else C.c_int
        assert t is want, (decl, t)
    assert "const int* group_start" in args and "int n_groups" in args and "const float* E" in args
    assert lib.rnnpose_abi_version() == 4 and _lib.ABI_VERSION == 4


def test_views_entry_refuses_on_the_host(lib):
    one, null = C.c_void_p(16), C.c_void_p(0)      # `one`: non-null dummy, never dereferenced on the host
    n = lib.rnnpose_lm_workspace_bytes(3, 8, 8)

    def call(start=one, ng=2, E=one, Hg=one, bg=one, xi=one, info=one, B=3, iters=1, tgt=one, wsb=n, obs=null, S=0):
        return lib.rnnpose_lm_step_views_io_f32(tgt, 0, one, one, 1e-5, one, one, one, B, 8, 8, iters, 100.0, 1e-4, 1.0, obs, null, one, one, S, 4, 4,
                                                1.0, 0.05, 0.02, start, ng, E, one, wsb, one, one, Hg, bg, xi, info, null, null)
    for kw, msg in ((dict(start=null), b"group_start"), (dict(E=null), b"group_start"), (dict(Hg=null), b"group_start"), (dict(bg=null), b"group_start"),
                    (dict(xi=null), b"group_start"), (dict(info=null), b"group_start"), (dict(ng=0), b"n_groups"), (dict(ng=4), b"n_groups"),
                    (dict(tgt=null), b"null pointer"), (dict(B=0), b"bad size"), (dict(iters=0), b"at least one iteration"),
                    (dict(wsb=n - 1), b"workspace too small"), (dict(obs=one, S=0), b"S >= 1"), (dict(obs=one, S=1), b"src_index")):
        assert call(**kw) == 1 and msg in lib.rnnpose_last_error(), (kw, lib.rnnpose_last_error())


def test_views_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "rnnpose_hip.h"\n'
                   "typedef int (*views_fn)(const float*, int, const float*, const float*, float, const float*, const float*, float*, int, int, int, int,\n"
                   "                        double, double, double, const float*, const int*, const float*, const float*, int, int, int, float, float,\n"
                   "                        float, const int*, int, const float*, void*, size_t, double*, double*, double*, double*, float*, int*, double*,\n"
                   "                        rnnpose_stream_t);\n"
                   "int main(void) { views_fn f = rnnpose_lm_step_views_io_f32; return f == 0; }\n")
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
