"""CPU: the short instantiation of the narrow step kernels (k_lm_step_short<NW, KC>: lm_step_body unrolled for
GTO_STEP_T_SHORT = 50 waypoints instead of GTO_MAX_T = 96), read from what the build left next to the library: the compiler's
resource remarks (kernel_resources.txt) and the function symbols of the library's embedded gfx950 image
(tools/code_footprint.py).  Skips when there is no build.

At T = 50 the general instantiation carries 24 registers of av[] that nothing is loaded into and, in each unrolled
per-waypoint loop, twelve bodies of twenty-four that never run.  A later change that gives the registers or the code back
fails here; so does one that copies the exit block into the path every round walks again (the general kernels' sizes)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grasptrajopt_amd", "csrc")
TABLE = os.path.join(CSRC, "kernel_resources.txt")
LIB = os.path.join(CSRC, "libgto_hip.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_FULL = "_Z9k_lm_stepILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
STEP_FEW = "_Z9k_lm_stepILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
SHORT_FULL = "_Z15k_lm_step_shortILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
SHORT_FEW = "_Z15k_lm_step_shortILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
# what this change's build reached (VGPRs, bytes of code), with a little room; its parent had only the general kernels:
#   k_lm_step<4,1>  127 VGPRs, 51 612 B      k_lm_step<8,4>  111 VGPRs, 51 020 B
# this build: k_lm_step_short<4,1> 103 VGPRs, 41 496 B; k_lm_step_short<8,4> 100 VGPRs, 40 920 B;
#             k_lm_step<4,1> 127 VGPRs, 48 240 B; k_lm_step<8,4> 111 VGPRs, 48 468 B (one exit block instead of three)
VGPR_MAX = {SHORT_FULL: 104, SHORT_FEW: 104}
CODE_MAX = {SHORT_FULL: 42 * 1024, SHORT_FEW: 42 * 1024, STEP_FULL: 49 * 1024, STEP_FEW: 49 * 1024}


def _rows():
    if not os.path.exists(TABLE):
        pytest.skip("no build: kernel_resources.txt is written by __graft_entry__.build()")
    rows = {}
    for line in open(TABLE):
        kv = dict(f.split("=", 1) for f in line.split())
        name = kv.pop("name")
        rows[name] = {k: int(v) for k, v in kv.items()}
    return rows


def _sizes():
    if not os.path.exists(LIB):
        pytest.skip("no build: libgto_hip.so")
    import code_footprint as cf
    sizes = {}
    for img in cf.device_images(open(LIB, "rb").read()):
        sizes.update(cf.function_sizes(img))
    return sizes


def test_short_kernels_exist_without_scratch_at_four_waves_per_simd():
    rows = _rows()
    for name in (SHORT_FULL, SHORT_FEW):
        assert name in rows, f"{name} missing from the build"
        r = rows[name]
        assert r["ScratchSize"] == 0 and r["Occupancy"] >= 4 and r["LDS"] == 16, (name, r)
        assert r["VGPRs"] + r["AGPRs"] <= VGPR_MAX[name], (name, r)
    # the registers the short class gives back: av[] of the four-wave kernel alone is 24 of them
    assert rows[SHORT_FULL]["VGPRs"] <= rows[STEP_FULL]["VGPRs"] - 20, (rows[SHORT_FULL], rows[STEP_FULL])


def test_code_sizes_stay_where_this_change_left_them():
    sizes = _sizes()
    for name, most in CODE_MAX.items():
        assert name in sizes, f"{name}: no function symbol in the library's code object"
        assert 0 < sizes[name] <= most, f"{name}: {sizes[name]} B of code > {most}"
    # the whole-file experiment the change started from reached 0.87 and 0.84 of the general kernels' bytes
    assert sizes[SHORT_FULL] <= 0.88 * sizes[STEP_FULL] and sizes[SHORT_FEW] <= 0.88 * sizes[STEP_FEW], sizes


def test_footprint_tool_reports_both_classes():
    if not os.path.exists(LIB):
        pytest.skip("no build: libgto_hip.so")
    import code_footprint as cf
    text = cf.report(LIB)
    assert "T <= 50 (k_lm_step_short)" in text and "any T (k_lm_step)" in text and "full round + tail" in text, text


def test_launch_site_picks_the_class_by_the_calls_T():
    api = open(os.path.join(CSRC, "gto_api.hip")).read()
    hdr = open(os.path.join(CSRC, "gto_kernels.h")).read()
    assert "#define GTO_STEP_T_SHORT 50" in hdr
    assert "h->tu.step_tclass && T <= GTO_STEP_T_SHORT" in api and '"GTO_STEP_TCLASS"' in api
    for k in ("k_lm_step_short<4, 1>", "k_lm_step_short<8, GTO_KSPEC>"):
        assert f"raise_dynamic_lds((const void*){k}" in api, k
