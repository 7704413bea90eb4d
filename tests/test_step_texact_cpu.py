"""CPU: the narrow step kernels compiled for T = GTO_STEP_T_EXACT = 50 (k_lm_step_t50<NW, KC>: lm_step_body with the
trajectory length a constant), read from what the build left next to the library: the compiler's resource remarks
(kernel_resources.txt), the function symbols and the notes of the library's embedded gfx950 image (tools/code_footprint.py;
.sgpr_spill_count as test_step_kernel_resources_cpu.py reads it).  Skips when there is no build.

With T a constant the carve-up of the dynamic LDS, the idx < m * 8, s < m and t == T - 1 tests and the trip counts of P2, P4,
P5 and the tail fold at compile time.  Each exact kernel must be no larger than its k_lm_step_short sibling in instructions
(code bytes: the symbol size) and in spilled scalars, within two vector registers of it, at four waves per SIMD, without
scratch.  A later change that makes the constant cost more than it saves fails here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grasptrajopt_amd", "csrc")
TABLE = os.path.join(CSRC, "kernel_resources.txt")
LIB = os.path.join(CSRC, "libgto_hip.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHORT_FULL = "_Z15k_lm_step_shortILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
SHORT_FEW = "_Z15k_lm_step_shortILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
EXACT_FULL = "_Z13k_lm_step_t50ILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
EXACT_FEW = "_Z13k_lm_step_t50ILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
SIBLING = {EXACT_FULL: SHORT_FULL, EXACT_FEW: SHORT_FEW}


def _rows():
    if not os.path.exists(TABLE):
        pytest.skip("no build: kernel_resources.txt is written by __graft_entry__.build()")
    rows = {}
    for line in open(TABLE):
        kv = dict(f.split("=", 1) for f in line.split())
        name = kv.pop("name")
        rows[name] = {k: int(v) for k, v in kv.items()}
    return rows


def _blob():
    if not os.path.exists(LIB):
        pytest.skip("no build: libgto_hip.so")
    return open(LIB, "rb").read()


def _sizes():
    import code_footprint as cf
    sizes = {}
    for img in cf.device_images(_blob()):
        sizes.update(cf.function_sizes(img))
    return sizes


def _mp_str_head(n):
    return bytes([0xa0 | n]) if n < 32 else (bytes([0xd9, n]) if n < 256 else bytes([0xda, n >> 8, n & 255]))


def _mp_uint(blob, i):
    t = blob[i]
    if t < 0x80:
        return t
    assert t in (0xcc, 0xcd, 0xce), hex(t)
    n = {0xcc: 1, 0xcd: 2, 0xce: 4}[t]
    return int.from_bytes(blob[i + 1:i + 1 + n], "big")


def _spill_count(blob, name):
    """.sgpr_spill_count of a kernel from the notes of the code object inside the library (msgpack: the key, then a small integer)"""
    sym = (name + ".kd").encode()
    at = blob.find(b".symbol" + _mp_str_head(len(sym)) + sym)
    assert at >= 0, f"{name}: not in the library's notes"
    key = b".sgpr_spill_count"
    k = blob.rfind(key, 0, at)
    assert k >= 0 and at - k < 64, "the notes' keys are not in the order this test reads them in"
    return _mp_uint(blob, k + len(key))


@pytest.mark.parametrize("name", [EXACT_FULL, EXACT_FEW])
def test_exact_kernel_exists_without_scratch_at_four_waves_per_simd(name):
    rows = _rows()
    assert name in rows, f"{name} missing from the build"
    r, s = rows[name], rows[SIBLING[name]]
    assert r["ScratchSize"] == 0 and r["Occupancy"] >= 4 and r["LDS"] == 16, (name, r)
    assert r["VGPRs"] + r["AGPRs"] <= s["VGPRs"] + s["AGPRs"] + 2, (name, r, s)
    if name == EXACT_FULL:
        assert r["VGPRs"] + r["AGPRs"] <= 104, r  # four workgroups of it per CU next to the evaluation kernel's


def _instruction_counts(blob, names):
    """name -> instructions of the kernel, counted in the disassembly of the library's code object (the toolchain's
    llvm-objdump, next to the compiler the library was built with); None where the tool is not installed"""
    import shutil
    import subprocess
    import tempfile
    import code_footprint as cf
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tool = next((t for t in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-objdump"),
                             "/opt/rocm/llvm/bin/llvm-objdump", shutil.which("llvm-objdump") or "") if t and os.path.exists(t)), None)
    if tool is None:
        return None
    out = {}
    for img in cf.device_images(blob):
        if not all(n in cf.function_sizes(img) for n in names):
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            for n in names:
                res = subprocess.run([tool, "-d", "--no-show-raw-insn", f"--disassemble-symbols={n}", f.name], capture_output=True, text=True, timeout=60)
                assert res.returncode == 0, res.stderr[-2000:]
                out[n] = sum(1 for ln in res.stdout.splitlines() if ln.startswith("\t"))
    return out


@pytest.mark.parametrize("name", [EXACT_FULL, EXACT_FEW])
def test_exact_kernel_is_no_larger_than_its_short_sibling(name):
    """Instructions (counted in the code object's disassembly, and by the bytes of code: the symbol size), spilled scalars by
    the code object's own count."""
    sizes, blob = _sizes(), _blob()
    assert name in sizes, f"{name}: no function symbol in the library's code object"
    n_ins = _instruction_counts(blob, (name, SIBLING[name]))
    print(name, sizes[name], "B against", sizes[SIBLING[name]], "; instructions", n_ins, "; sgpr_spill_count", _spill_count(blob, name),
          "against", _spill_count(blob, SIBLING[name]))
    assert 0 < sizes[name] <= sizes[SIBLING[name]], (name, sizes[name], sizes[SIBLING[name]])
    if n_ins is not None:  # (a machine without the disassembler: the bytes above stand for the count)
        assert 0 < n_ins[name] <= n_ins[SIBLING[name]], n_ins
    assert _spill_count(blob, name) <= _spill_count(blob, SIBLING[name])


def test_footprint_tool_reports_the_exact_class_next_to_the_others():
    import code_footprint as cf
    _blob()
    text = cf.report(LIB)
    assert "T = 50 (k_lm_step_t50)" in text and "T <= 50 (k_lm_step_short)" in text and "any T (k_lm_step)" in text, text


def test_launch_site_picks_the_exact_kernels_at_their_length_only():
    api = open(os.path.join(CSRC, "gto_api.hip")).read()
    hdr = open(os.path.join(CSRC, "gto_kernels.h")).read()
    assert "#define GTO_STEP_T_EXACT 50" in hdr
    assert '"GTO_STEP_TEXACT"' in api and "int step_texact = 1;" in api
    assert "h->tu.step_texact && T == GTO_STEP_T_EXACT" in api
    for k in ("k_lm_step_t50<4, 1>", "k_lm_step_t50<8, GTO_KSPEC>"):
        assert f"raise_dynamic_lds((const void*){k}" in api, k
        assert f"if (t_exact) hipLaunchKernelGGL(({k})" in api, k
    # the launch's LDS size stays the runtime formula, and the constant carve-up is held to it at compile time
    assert "lm_lds_layout(TEXACT, 1).bytes == lm_lds_bytes(TEXACT, 1)" in hdr
