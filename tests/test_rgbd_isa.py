"""Compile-time check of the depth-aware LM kernel (CPU only: hipcc cross-compiles gfx950), in the manner of tests/test_isa_guard.py:
csrc/lm.hip is compiled with the library's flags, and both DEPTH = true instantiations of lm_eq_kernel (three-launch form, fused tail) must
report no spilled VGPR and must issue their loads in batches -- more global loads than full `s_waitcnt vmcnt(0)` waits.  A load under a
bounds test, or a divergent branch around the tap loads, would bring one full wait per load back (rule 1)."""
import os
import re

from test_isa_guard import ROOT, _isa

KERNEL = "lm_eq_kernelILb1E"       # lm_eq_kernel<DEPTH = true, FUSED> in the mangled symbol; ...ILb0E is the plain step of test_isa_guard


def test_rgbd_kernel_does_not_spill_and_batches_its_loads(tmp_path):
    txt, spills = _isa(os.path.join(ROOT, "rnnpose_amd", "csrc", "lm.hip"), tmp_path)
    bodies = {m.group(1): m.group(0) for m in re.finditer(r"^(_Z\w+):.*?s_endpgm", txt, re.S | re.M)}
    hits = {sym: b for sym, b in bodies.items() if KERNEL in sym}
    assert len(hits) == 2, f"expected the two instantiations of {KERNEL}, found {sorted(hits)}"
    assert sorted(s for s in spills if KERNEL in s) == sorted(hits)
    for sym, body in hits.items():
        loads = len(re.findall(r"global_load|buffer_load", body))
        w0 = len(re.findall(r"s_waitcnt vmcnt\(0\)", body))
        counted = len(re.findall(r"s_waitcnt vmcnt\([1-9]", body))
        print(f"{sym}: {loads} loads, {w0} vmcnt(0) waits, {counted} counted waits, {spills[sym]} spilled VGPRs")
        assert spills[sym] == 0, f"{sym} spills {spills[sym]} VGPRs"
        assert "scratch_" not in body, f"{sym} uses scratch memory"
        # LM_BATCH = 8 pixels a trip: 8 x (weight, depth, target) and 8 x 4 taps are in flight together
        assert loads >= 8 * 3 + 8 * 4, (sym, loads)
        assert loads > w0, f"{sym}: {w0} vmcnt(0) waits for {loads} loads -- the loads are serialised"
        assert counted >= 8, f"{sym}: only {counted} counted waits for {loads} loads"
    # the kernels the existing guard was written for are different symbols: its key matches none of these
    assert not any("lm_eq_kernelILb0E" in sym for sym in hits)
    # the host-execution tier rewrites exactly two full-wait statements of this file (tests/host_exec/build_host.py)
    src = open(os.path.join(ROOT, "rnnpose_amd", "csrc", "lm.hip")).read()
    assert len(re.findall(r'asm volatile\("s_waitcnt vmcnt\(0\)" ::: "memory"\);', src)) == 2
