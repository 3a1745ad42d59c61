#!/usr/bin/env python3
"""Compare the kernels of two device-only assembly files, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S unit.hip -o unit.s

of a parent commit and of a branch (the library's flags, csrc/Makefile), then

    scripts/kernel_diff.py parent/unit.s branch/unit.s [parent/other.s branch/other.s ...]

prints per pair the number of kernels of the parent file and how many of them are identical instruction for instruction in
the branch file, different, or missing there, and how many kernels are new.  A kernel is a symbol with an .amdhsa_kernel
descriptor; its text runs from its label to the end label of the function.  Only instruction lines and the labels between
them are compared: comments, blank lines and assembler directives are dropped, and the ordinal of the function in a local
label (.LBB<ordinal>_<n>) too, which says where in the file the kernel stands and not what it does.  Exit status 1 if
any kernel is different, missing or new."""
import re
import sys

LOCAL_LABEL = re.compile(r"\.LBB\d+_")


def kernels(path):
    """{symbol: [instruction lines]} of the kernels of an assembly file"""
    lines = open(path).read().splitlines()
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
    out, name = {}, None
    for ln in lines:
        text = ln.split(";", 1)[0].split("//", 1)[0].strip()
        if name is None:
            if text.endswith(":") and text[:-1] in names:
                name = text[:-1]
                out[name] = []
            continue
        if text.startswith(".Lfunc_end"):
            name = None
        elif text and (not text.startswith(".") or text.endswith(":")):
            out[name].append(LOCAL_LABEL.sub(".LBB_", " ".join(text.split())))
    return out


def main(argv):
    if len(argv) < 3 or len(argv) % 2 == 0:
        print(__doc__)
        return 2
    status = 0
    for parent_path, branch_path in zip(argv[1::2], argv[2::2]):
        parent, branch = kernels(parent_path), kernels(branch_path)
        same = [k for k in parent if k in branch and parent[k] == branch[k]]
        different = [k for k in parent if k in branch and parent[k] != branch[k]]
        missing = [k for k in parent if k not in branch]
        new = [k for k in branch if k not in parent]
        print(f"{branch_path}: parent kernels {len(parent)}; identical instruction for instruction {len(same)}; "
              f"different {len(different)}; missing {len(missing)}; new {len(new)}")
        for title, group in (("different", different), ("missing", missing), ("new", new)):
            for k in group:
                print(f"  {title}: {k}")
        if different or missing or new:
            status = 1
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
