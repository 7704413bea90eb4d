"""CPU: the step kernels' registers, read from what the build left next to the library (kernel_resources.txt, written by
__graft_entry__.build from the compiler's resource remarks) and from the code object's own notes (the .sgpr_spill_count of
each kernel, in the library's embedded gfx950 image).  Skips when there is no build.

The step kernels read their arguments phase by phase (gto_kernels.h, StepKernArgs) so that the compiler has scalar registers
for what a phase needs; held from the entry, the arguments cost k_lm_step<4,1> 219 spilled dwords and 1 423 lane reads to
fetch them back (tools/spill_report.py).  A later change that brings the spills back, or pays for scalar
registers with vector ones, fails here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grasptrajopt_amd", "csrc")
TABLE = os.path.join(CSRC, "kernel_resources.txt")
LIB = os.path.join(CSRC, "libgto_hip.so")

STEP_FULL = "_Z9k_lm_stepILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
STEP_FEW = "_Z9k_lm_stepILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
SEED_BROAD = "_Z12k_seed_broadPK8RobotDev9BatchPtrs11SolveParamsiPyi"
# sgpr_spill_count the build of this change reached (its parent: 219 and 94)
SPILL_MAX = {STEP_FULL: 28, STEP_FEW: 24}


def _rows():
    if not os.path.exists(TABLE):
        pytest.skip("no build: kernel_resources.txt is written by __graft_entry__.build()")
    rows = {}
    for line in open(TABLE):
        kv = dict(f.split("=", 1) for f in line.split())
        name = kv.pop("name")
        rows[name] = {k: int(v) for k, v in kv.items()}
    return rows


def _spill_counts():
    """kernel -> .sgpr_spill_count from the notes of the code object inside the library (msgpack: the key, then a small integer)."""
    if not os.path.exists(LIB):
        pytest.skip("no build: libgto_hip.so")
    blob = open(LIB, "rb").read()
    out = {}
    for name in (STEP_FULL, STEP_FEW, SEED_BROAD):
        # a kernel's map: ... ".name" str ... ".sgpr_spill_count" int ".symbol" str(name + ".kd") ...
        sym = (name + ".kd").encode()
        at = blob.find(b".symbol" + _mp_str_head(len(sym)) + sym)
        if at < 0:
            pytest.skip(f"{name}: not in the library's notes")
        key = b".sgpr_spill_count"
        k = blob.rfind(key, 0, at)
        assert k >= 0 and at - k < 64, "the notes' keys are not in the order this test reads them in"
        out[name] = _mp_uint(blob, k + len(key))
    return out


def _mp_str_head(n):
    return bytes([0xa0 | n]) if n < 32 else (bytes([0xd9, n]) if n < 256 else bytes([0xda, n >> 8, n & 255]))


def _mp_uint(blob, i):
    t = blob[i]
    if t < 0x80:
        return t
    assert t in (0xcc, 0xcd, 0xce), hex(t)
    n = {0xcc: 1, 0xcd: 2, 0xce: 4}[t]
    return int.from_bytes(blob[i + 1:i + 1 + n], "big")


def test_step_kernels_keep_their_register_budgets():
    rows = _rows()
    full, few, seed = rows[STEP_FULL], rows[STEP_FEW], rows[SEED_BROAD]
    # four workgroups of the one-candidate kernel per CU: 128 registers a lane, nothing in scratch, the 16 static bytes of LDS
    assert full["VGPRs"] + full["AGPRs"] <= 128 and full["ScratchSize"] == 0 and full["Occupancy"] >= 4 and full["LDS"] == 16, full
    assert few["VGPRs"] + few["AGPRs"] <= 112 and few["ScratchSize"] == 0, few
    assert seed["ScratchSize"] == 0, seed


def test_dynamic_lds_of_the_one_candidate_launch_is_unchanged():
    """lm_lds_bytes(50, 1) = 40 832 B: with the 16 static bytes, four workgroups in a CU's 160 KiB."""
    T, KL = 50, 1
    m = T - 2
    dbl = KL * (m * 64 + m * 8) + 3 * m * 8 + 8 * T + 16 + 56
    assert dbl * 8 + ((m + 1) & ~1) * 4 == 40832
    src = open(os.path.join(CSRC, "gto_kernels.h")).read()
    assert "const size_t dbl = (size_t)KL * (m * 64 + m * 8) + 3 * m * 8 + 8 * (size_t)T + 16 + lm_red_doubles(KL);" in src
    assert re.search(r"lm_red_doubles\(int KL\) \{ return KL == 1 \? 56 : 96; \}", src)
    assert 4 * (40832 + 16) <= 160 * 1024


def test_scalar_spills_of_the_step_kernels_stay_where_this_change_left_them():
    got = _spill_counts()
    print(got)
    for name, most in SPILL_MAX.items():
        assert got[name] <= most, f"{name}: sgpr_spill_count {got[name]} > {most} (tools/spill_report.py shows where)"
    assert got[SEED_BROAD] == 0  # the same pb_test as the step kernel's tail, in a kernel that has room for it
