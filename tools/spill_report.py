#!/usr/bin/env python3
"""Scalar-register spills of the step kernels, read off the compiler's own listing (no GPU needed).

The compiler parks scalars it has no register for in the lanes of a few vector registers: one v_writelane_b32 per spilled
dword, one v_readlane_b32 per reload.  A reload computes nothing, and in a kernel bound by instruction issue it is paid in
full.  This tool compiles the device code to assembly with the product's flags (__graft_entry__.HIPCC_FLAGS) and prints, per
kernel: the registers and spill count the code object declares, the spill stores, the reloads of spilled scalars, how many of
the reloads lie inside a loop body (between a label and a backward branch to it), and the reloads per barrier segment (the
code between two s_barrier).  A reload is a v_readlane_b32 from a vector register that the kernel also spills into; other
lane reads (the kernels' own __builtin_amdgcn_readlane) are not counted.  Positions are in the listing's order, which is
the order the blocks were laid out in, not the order they run in.

usage: python tools/spill_report.py [--src DIR] [--asm FILE.s] [--kernels SUBSTR,...] [--segments] [-o OUT.txt]
  --src DIR   the csrc directory of another checkout (default: this tree's)
  --asm FILE  read an existing listing instead of compiling
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_KERNELS = ("k_lm_stepILi4ELi1", "k_lm_stepILi8ELi4", "k_lm_step_wide", "k_seed_broad", "k_obstacle_gramILi8ELi1",
                   "k_lm_step_shortILi4ELi1", "k_lm_step_shortILi8ELi4", "k_lm_step_t50ILi4ELi1", "k_lm_step_t50ILi8ELi4")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
WRITELANE = re.compile(r"^\s*(v\d+),")
READLANE = re.compile(r"^\s*s\d+,\s*(v\d+),")


def compile_listing(src):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", os.path.join(src, "gto_api.hip"), "-o", out]
    subprocess.run(cmd, cwd=src, check=True)
    return out


def functions(lines):
    """name -> list of body lines, for every .type NAME,@function"""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(\w+):\s*(;.*)?$", ln)
        if m and name is None and m.group(1).startswith("_Z"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(ln)
    return out


def metadata(lines):
    """name -> {sgpr_count, sgpr_spill_count, vgpr_count, vgpr_spill_count, private_segment_fixed_size} from the code object's notes"""
    out, cur = {}, {}
    for ln in lines:
        m = re.match(r"^  (- | {2})\.(\w+):\s+(\S+)\s*$", ln)
        if not m:
            continue
        if m.group(1) == "- ":  # a kernel's entry starts
            cur = {}
        k, v = m.group(2), m.group(3)
        if k in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            cur[k] = int(v)
        elif k == "name":
            out[v] = cur
    return out


def analyse(body):
    insns, labels = [], {}  # (mnemonic, operands)
    for ln in body:
        m = LABEL.match(ln)
        if m:
            labels[m.group(1)] = len(insns)
            continue
        m = INSN.match(ln)
        if m and not ln.lstrip().startswith((".", ";")):
            insns.append((m.group(1), m.group(2).split(";")[0]))
    spill_regs, stores = set(), 0
    for op, args in insns:
        if op == "v_writelane_b32":
            m = WRITELANE.match(args)
            if m:
                spill_regs.add(m.group(1))
                stores += 1
    in_loop = [False] * len(insns)
    loops = []
    for i, (op, args) in enumerate(insns):
        if op.startswith("s_cbranch") or op == "s_branch":
            t = labels.get(args.strip())
            if t is not None and t <= i:
                loops.append((t, i))
                for k in range(t, i + 1):
                    in_loop[k] = True
    # outermost backward-branch regions (merged), largest first
    merged = []
    for t, i in sorted(loops):
        if merged and t <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], i)
        else:
            merged.append([t, i])
    reload_at = []
    for i, (op, args) in enumerate(insns):
        if op == "v_readlane_b32":
            m = READLANE.match(args)
            if m and m.group(1) in spill_regs:
                reload_at.append(i)
    segs, start = [], 0
    for i, (op, _) in enumerate(insns):
        if op == "s_barrier":
            segs.append((start, i))
            start = i + 1
    segs.append((start, len(insns)))
    seg_rows = [(e - s, sum(1 for r in reload_at if s <= r < e)) for s, e in segs]
    regions = sorted(((e - s + 1, sum(1 for r in reload_at if s <= r <= e)) for s, e in merged), reverse=True)
    return {"insns": len(insns), "stores": stores, "spill_regs": sorted(spill_regs, key=lambda v: int(v[1:])),
            "reloads": len(reload_at), "reloads_in_loops": sum(1 for r in reload_at if in_loop[r]),
            "barriers": len(segs) - 1, "segments": seg_rows, "loop_regions": regions}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=os.path.join(ROOT, "grasptrajopt_amd", "csrc"))
    ap.add_argument("--asm")
    ap.add_argument("--kernels", default=",".join(DEFAULT_KERNELS))
    ap.add_argument("--segments", action="store_true", help="also list every barrier segment and the large loop regions")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    path = a.asm or compile_listing(a.src)
    lines = open(path).read().splitlines()
    if not a.asm:
        os.unlink(path)
    fns, meta = functions(lines), metadata(lines)
    keys = [k for k in a.kernels.split(",") if k]
    rows = []
    rows.append("| kernel | SGPRs | VGPRs | sgpr_spill_count | scratch B | spill stores (v_writelane_b32) | into | reloads (v_readlane_b32) | in loop bodies | instructions | reloads / instructions |")
    rows.append("|---|---:|---:|---:|---:|---:|---|---:|---:|---:|---:|")
    detail = []
    for name in sorted(fns):
        if not any(k in name for k in keys) or name not in meta:
            continue
        r, md = analyse(fns[name]), meta[name]
        into = ",".join(r["spill_regs"]) or "-"
        rows.append(f"| `{name}` | {md.get('sgpr_count')} | {md.get('vgpr_count')} | {md.get('sgpr_spill_count')} | {md.get('private_segment_fixed_size')} | "
                    f"{r['stores']} | {into} | {r['reloads']} | {r['reloads_in_loops']} | {r['insns']} | {100.0 * r['reloads'] / max(1, r['insns']):.1f} % |")
        if a.segments:
            detail.append(f"\n`{name}`: {r['barriers']} s_barrier; reloads / instructions per barrier segment, in the listing's order:")
            detail.append("  " + "  ".join(f"[{i}] {rl}/{n}" for i, (n, rl) in enumerate(r["segments"])))
            detail.append("  backward-branch regions of 200 instructions or more (instructions, reloads): " +
                          (", ".join(f"({n}, {rl})" for n, rl in r["loop_regions"] if n >= 200) or "none"))
    text = "\n".join(rows + detail) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
