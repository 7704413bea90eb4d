#!/usr/bin/env python3
"""Code sizes of the solve loop's kernels, read from the built library's gfx950 code object (no GPU needed).

With several lanes in different phases one CU holds workgroups of two to four of these kernels at once, and what they
fetch instructions from is the sum of their code.  This tool prints the symbol size of every solve-loop kernel (the
function symbols of the device image embedded in libgto_hip.so) and the sums for the sets that run together:

  full round             the one-candidate step kernel and the itemized obstacle launch (with the crew it may call)
  full round + tail      ... plus another lane's tail: the eight-wave step kernel and both of its obstacle variants
  tail alone             the eight-wave step kernel and the two obstacle variants of the tail

The step kernels are listed as a call with T <= GTO_STEP_T_SHORT launches them (k_lm_step_short) and as any other call
does (k_lm_step); a library without the short instantiation (an older build) gives the second set only.  A library with the
instantiation for T = GTO_STEP_T_EXACT (k_lm_step_t50) gets a third set, listed last.

usage: python tools/code_footprint.py [--lib libgto_hip.so] [-o OUT.txt]
"""
import argparse
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EM_AMDGPU = 224
STT_FUNC = 2

STEP_FULL = "_Z9k_lm_stepILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
STEP_FEW = "_Z9k_lm_stepILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
STEP_FULL_SHORT = "_Z15k_lm_step_shortILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
STEP_FEW_SHORT = "_Z15k_lm_step_shortILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
STEP_FULL_T50 = "_Z13k_lm_step_t50ILi4ELi1EEvPK8RobotDev9BatchPtrs11SolveParamsi"
STEP_FEW_T50 = "_Z13k_lm_step_t50ILi8ELi4EEvPK8RobotDev9BatchPtrs11SolveParamsi"
OBS = "_Z15k_obstacle_gramILi8ELi%dELb%dELb1EE"  # <8, DEEP, ITEMIZED, true>
OBS_ITEM, OBS_TAIL, OBS_TAIL_DEEP = OBS % (1, 1), OBS % (1, 0), OBS % (8, 0)
CREW = "obstacle_gram_crew"


def device_images(blob):
    """every AMDGPU ELF image inside the library: (offset, bytes to the end of its section headers)"""
    out, at = [], 0
    while True:
        at = blob.find(b"\x7fELF\x02\x01", at)
        if at < 0:
            return out
        if len(blob) - at >= 64:
            e_machine = struct.unpack_from("<H", blob, at + 18)[0]
            e_shoff, = struct.unpack_from("<Q", blob, at + 40)
            e_shentsize, e_shnum = struct.unpack_from("<HH", blob, at + 58)
            if e_machine == EM_AMDGPU and e_shoff and at + e_shoff + e_shentsize * e_shnum <= len(blob):
                out.append(blob[at:at + e_shoff + e_shentsize * e_shnum])
        at += 4


def function_sizes(img):
    """name -> st_size of every function symbol of an ELF64 image's .symtab"""
    e_shoff, = struct.unpack_from("<Q", img, 40)
    e_shentsize, e_shnum = struct.unpack_from("<HH", img, 58)
    secs = [struct.unpack_from("<IIQQQQIIQQ", img, e_shoff + i * e_shentsize) for i in range(e_shnum)]
    out = {}
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        off, size, link, entsize = s[4], s[5], s[6], s[9]
        stroff = secs[link][4]
        for i in range(size // entsize):
            st_name, st_info, _, _, _, st_size = struct.unpack_from("<IBBHQQ", img, off + i * entsize)
            if st_info & 0xf == STT_FUNC:
                end = img.index(b"\0", stroff + st_name)
                out[img[stroff + st_name:end].decode()] = st_size
    return out


def find(sizes, key):
    hit = [n for n in sizes if key in n]
    return hit[0] if hit else None


def report(lib):
    blob = open(lib, "rb").read()
    sizes = {}
    for img in device_images(blob):
        sizes.update(function_sizes(img))
    if not sizes:
        raise SystemExit(f"{lib}: no gfx code object with a symbol table found")
    obs_item, obs_tail, obs_deep, crew = (find(sizes, k) for k in (OBS_ITEM, OBS_TAIL, OBS_TAIL_DEEP, CREW))
    missing = [k for k, n in ((STEP_FULL, find(sizes, STEP_FULL)), (STEP_FEW, find(sizes, STEP_FEW)), (OBS_ITEM, obs_item),
                              (OBS_TAIL, obs_tail), (OBS_TAIL_DEEP, obs_deep)) if n is None]
    if missing:
        raise SystemExit(f"{lib}: kernels missing from the code object: {missing}")
    kb = lambda n: f"{sizes[n]:7d} B  {sizes[n] / 1024.0:6.1f} KB"
    lines = [f"library: {os.path.basename(lib)}", "", "solve-loop kernels (function symbol sizes):"]
    names = [STEP_FULL_SHORT, STEP_FEW_SHORT, STEP_FULL, STEP_FEW, obs_item, crew, obs_tail, obs_deep, STEP_FULL_T50, STEP_FEW_T50]
    for n in names:
        if n in sizes:
            lines.append(f"  {kb(n)}  {n}")
    classes = [("T <= 50 (k_lm_step_short)", STEP_FULL_SHORT, STEP_FEW_SHORT)] if STEP_FULL_SHORT in sizes and STEP_FEW_SHORT in sizes else []
    classes.append(("any T (k_lm_step)", STEP_FULL, STEP_FEW))
    if STEP_FULL_T50 in sizes and STEP_FEW_T50 in sizes:
        classes.append(("T = 50 (k_lm_step_t50)", STEP_FULL_T50, STEP_FEW_T50))
    for title, full, few in classes:
        item = sizes[obs_item] + (sizes[crew] if crew else 0)
        tail = sizes[few] + sizes[obs_tail] + sizes[obs_deep]
        lines += ["", f"sets that run together, {title}:",
                  f"  full round          {(sizes[full] + item) / 1024.0:6.1f} KB  (without the crew {(sizes[full] + sizes[obs_item]) / 1024.0:.1f})",
                  f"  full round + tail   {(sizes[full] + item + tail) / 1024.0:6.1f} KB",
                  f"  tail alone          {tail / 1024.0:6.1f} KB"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "grasptrajopt_amd", "csrc", "libgto_hip.so"))
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    text = report(a.lib)
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
