#!/usr/bin/env python3
"""Do two builds of the kernel files compile to the same code?  Per kernel: the ISA body, the kernel descriptor and hipcc's resource-usage remarks.

  python tools/isa_compare.py PARENT_DIR BRANCH_DIR

Each directory holds one sub-directory per kernel translation unit (qr_mpc_kernel, ..., qr_plant_kernel), made there by
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=fast-honor-pragmas -fPIC -Wno-unused-value --save-temps
        -Rpass-analysis=kernel-resource-usage -c csrc/UNIT.hip -o UNIT.o > remarks.txt 2>&1
Normalised: the __hip_cuid_* symbol, white space, assembler comments (no instruction is a comment), and the function's ordinal in local labels
(.LBB<k>_<j>, .LJTI<k>_<j>: <k> counts the functions of the unit, so a kernel added in front of another renumbers it).  The report goes to stdout
in the form of profiles/*_isa_compare.txt."""
import glob
import os
import re
import sys


def kernels(unit_dir):
    """-> {kernel: (body lines, descriptor lines)} of the unit's gfx950 .s file"""
    s = glob.glob(os.path.join(unit_dir, "*gfx950*.s"))
    assert len(s) == 1, (unit_dir, s)
    lines = []
    for ln in open(s[0]):
        ln = re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln.split(";")[0]).strip()
        if ln:
            lines.append(re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1_", re.sub(r"\s+", " ", ln)))
    out, name, body = {}, None, []
    desc = {}
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.fullmatch(r"(\w+):", ln)
        if m and i > 0 and name is None and any(lines[k] == ".type %s,@function" % m.group(1) for k in range(max(0, i - 6), i)):
            name, body = m.group(1), []
        elif name is not None and ln.startswith(".Lfunc_end"):
            out[name] = body; name = None
        elif name is not None:
            body.append(ln)
        m = re.fullmatch(r"\.amdhsa_kernel (\w+)", ln)
        if m:
            k = i
            while lines[k] != ".end_amdhsa_kernel":
                k += 1
            desc[m.group(1)] = lines[i + 1:k]
            i = k
        i += 1
    return {k: (out[k], desc[k]) for k in desc if k in out}


def remarks(unit_dir):
    """-> {kernel: resource string}"""
    res, name = {}, None
    for ln in open(os.path.join(unit_dir, "remarks.txt")):
        m = re.search(r"remark: (?:\S+: )?\s*(.*?) \[-Rpass-analysis", ln)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip(); res[name] = []
        elif name is not None:
            res[name].append(t)
    return {k: ", ".join(v) for k, v in res.items()}


def main():
    parent, branch = sys.argv[1:3]
    compared = differ = 0
    report = []
    for unit in sorted(os.listdir(branch)):
        b, rb = kernels(os.path.join(branch, unit)), remarks(os.path.join(branch, unit))
        has_parent = os.path.isdir(os.path.join(parent, unit))
        p, rp = (kernels(os.path.join(parent, unit)), remarks(os.path.join(parent, unit))) if has_parent else ({}, {})
        print("== %s: parent %d kernels, branch %d kernels" % (unit, len(p), len(b)))
        for k in b:
            if k not in p:
                print("   %-100s NEW (%d lines)" % (k, len(b[k][0])))
                report.append((k, rb.get(k)))
                continue
            compared += 1
            same = (b[k][0] == p[k][0], b[k][1] == p[k][1], rb.get(k) == rp.get(k))
            differ += not all(same)
            print("   %-100s body %s (%d lines)  descriptor %s  resources %s" % (k, "SAME" if same[0] else "DIFFERENT", len(b[k][0]), "SAME" if same[1] else "DIFFERENT",
                                                                              "SAME" if same[2] else "DIFFERENT"))
            if unit.startswith("qr_plant"):
                report.append((k, rb.get(k)))
        for k in p:
            if k not in b:
                differ += 1
                print("   %-100s GONE" % k)
    print("KERNELS COMPARED: %d\nKERNELS THAT DIFFER: %d\n\nResource usage as built (branch), the new kernels and the plant kernels:" % (compared, differ))
    for k, r in report:
        print("   %-100s %s" % (k, r))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
