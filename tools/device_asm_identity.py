#!/usr/bin/env python3
"""Device code of two trees, kernel by kernel: hashes of the compiler's assembly, paired by name.

  hipcc $(HIPFLAGS) --cuda-device-only -S csrc/<unit>.hip -o <dir>/<unit>.s     (in both trees)
  tools/device_asm_identity.py PARENT_DIR BRANCH_DIR unit [unit ...] [--rename OLD=NEW]

The assembly is split at the function symbols and the kernels are paired by mangled name.
Normalised before hashing: the function number in block labels (.LBB<n>_, BB<n>_, .Lfunc_end<n>,
which follow the emission order), the comment column, the __hip_cuid_ symbol.  text = the
instructions, the .amdhsa descriptor and the compiler's resource comments; meta = the kernel's
entry of the amdgpu_metadata note.  --rename replaces a symbol name in the parent's text (a
device global that the branch renamed), and is printed in the header.  For a kernel that
differs, the resource figures of both sides are printed.  This compares text; it does not look
at what the instructions are.
"""
import hashlib
import os
import re
import sys

RES = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize", "codeLenInByte")


def norm(line):
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"\bBB\d+_", "BB_", line)
    line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)
    line = re.sub(r"__hip_cuid_\w+", "__hip_cuid_X", line)
    return line


def split(path, renames):
    text = open(path).read()
    for old, new in renames:
        text = text.replace(old, new)
    lines = text.split("\n")
    funcs, order, name, in_res = {}, [], None, False
    meta_at = next((i for i, l in enumerate(lines) if ".amdgpu_metadata" in l), len(lines))
    for l in lines[:meta_at]:
        m = re.match(r"\s*\.type\s+(\S+),@(function|object)", l)
        if m:
            name = m.group(1) if m.group(2) == "function" else None
            in_res = False
            if name:
                funcs[name] = []
                order.append(name)
        if name is None or ".AMDGPU.gpr_maximums" in l:
            name = None
            continue
        if ".AMDGPU.csdata" in l:
            in_res = True
        s = l.rstrip()
        if not in_res:  # drop the comment column
            s = re.sub(r"\s*;.*$", "", s)
        if s.strip():
            funcs[name].append(norm(s))
    metas, cur = {}, None
    for l in lines[meta_at:]:
        if l.startswith("  - "):
            cur = []
            metas[len(metas)] = cur
        elif not l.startswith("    "):
            cur = None
        if cur is not None:
            cur.append(norm(l))
    by_name = {}
    for e in metas.values():
        n = next((re.sub(r".*\.name:\s*", "", x).strip() for x in e if re.match(r"\s+(- )?\.name:", x)), None)
        by_name[n] = e
    return funcs, order, by_name


def h(ls):
    return hashlib.sha256("\n".join(ls).encode()).hexdigest()[:16]


def res(ls):
    out = []
    for key in RES:
        for l in ls:
            m = re.match(r";\s*" + key + r"\s*[:=]\s*(\d+)", l)
            if m:
                out.append(f"{key} {m.group(1)}")
                break
    return ", ".join(out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--rename")]
    renames = [tuple(a.split("=", 2)[1:]) for a in sys.argv[1:] if a.startswith("--rename=")]
    if len(args) < 3:
        sys.exit(__doc__)
    pdir, bdir, units = args[0], args[1], args[2:]
    for old, new in renames:
        print(f"# in the parent's text, symbol {old} is read as {new} (the branch renamed it)")
    print("# columns: kernel, text sha256[:16] parent branch, metadata-entry sha256[:16] parent branch")
    bad = 0
    for u in units:
        pf, po, pm = split(os.path.join(pdir, u + ".s"), renames)
        bf, bo, bm = split(os.path.join(bdir, u + ".s"), renames=[])
        print(f"## {u}.hip")
        same = diff = 0
        for n in sorted(set(pf) | set(bf)):
            if n not in pf or n not in bf:
                print(f"{n} only in {'parent' if n in pf else 'branch'}")
                diff += 1
                continue
            t = (h(pf[n]), h(bf[n]))
            m = (h(pm.get(n, [])), h(bm.get(n, [])))
            ok = t[0] == t[1] and m[0] == m[1]
            print(f"{n} text {t[0]} {t[1]} meta {m[0]} {m[1]} {'same' if ok else 'DIFFERENT'}")
            if not ok:
                print(f"  parent: {res(pf[n])}")
                print(f"  branch: {res(bf[n])}")
            same += ok
            diff += not ok
        print(f"kernels: parent {len(pf)}, branch {len(bf)}; names equal: {set(pf) == set(bf)}; "
              f"emitted in the same order: {po == bo}")
        print(f"identical (instruction text, .amdhsa descriptor, metadata entry): {same}; different: {diff}")
        bad += diff
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
