#!/usr/bin/env python3
"""Do two builds of the kernel files compile to the same code?  Per kernel: the ISA body, the kernel descriptor and hipcc's resource-usage remarks.

  python tools/isa_compare.py PARENT_DIR BRANCH_DIR [OLD=NEW ...]

Each directory holds one sub-directory per kernel translation unit (qr_mpc_kernel, ..., qr_plant_kernel), made there by
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=fast-honor-pragmas -fPIC -Wno-unused-value --save-temps
        -Rpass-analysis=kernel-resource-usage -c csrc/UNIT.hip -o UNIT.o > remarks.txt 2>&1
Normalised: the __hip_cuid_* symbol, white space, assembler comments (no instruction is a comment), and the function's ordinal in local labels
(.LBB<k>_<j>, .LJTI<k>_<j>: <k> counts the functions of the unit, so a kernel added in front of another renumbers it).  OLD=NEW reads the parent's
kernel OLD (its plain name, as in qrgpu::OLD) as NEW, so that a branch kernel is compared with a parent kernel of another name; a parent kernel is
looked for in every unit of the parent, so it may also have moved between units.  The report goes to stdout in the form of
profiles/*_isa_compare.txt."""
import glob
import os
import re
import sys


def renamed(text, names):
    """the mangled form <length><name> of every old name in `names` replaced by that of its new name"""
    for old, new in names.items():
        text = text.replace("%d%sE" % (len(old), old), "%d%sE" % (len(new), new))
    return text


def kernels(unit_dir, names={}):
    """-> {kernel: (body lines, descriptor lines)} of the unit's gfx950 .s file"""
    s = glob.glob(os.path.join(unit_dir, "*gfx950*.s"))
    assert len(s) == 1, (unit_dir, s)
    lines = []
    for ln in renamed(open(s[0]).read(), names).splitlines():
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


def remarks(unit_dir, names={}):
    """-> {kernel: resource string}"""
    res, name = {}, None
    for ln in renamed(open(os.path.join(unit_dir, "remarks.txt")).read(), names).splitlines():
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
    names = dict(a.split("=", 1) for a in sys.argv[3:])
    compared = differ = 0
    report = []
    p, rp, p_unit, seen = {}, {}, {}, set()              # the parent's kernels of all units: a kernel is found wherever it lies
    for unit in sorted(os.listdir(parent)):
        pk = kernels(os.path.join(parent, unit), names)
        p.update(pk); rp.update(remarks(os.path.join(parent, unit), names))
        p_unit.update((k, unit) for k in pk)
    for old, new in sorted(names.items()):
        print("parent's %s read as %s" % (old, new))
    for unit in sorted(os.listdir(branch)):
        b, rb = kernels(os.path.join(branch, unit)), remarks(os.path.join(branch, unit))
        print("== %s: parent %d kernels, branch %d kernels" % (unit, sum(u == unit for u in p_unit.values()), len(b)))
        seen.update(b)
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
            mapped = any("%d%sE" % (len(new), new) in k for new in names.values())
            if unit.startswith("qr_plant") or not all(same) or mapped:
                report.append((k, rb.get(k)))
    for k in p:
        if k not in seen:
            differ += 1
            print("   %-100s GONE (parent's %s)" % (k, p_unit[k]))
    print("KERNELS COMPARED: %d\nKERNELS THAT DIFFER: %d\n\nResource usage as built (branch): the new kernels, the plant kernels, the kernels that differ or were compared under another name:" % (compared, differ))
    for k, r in report:
        print("   %-100s %s" % (k, r))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
