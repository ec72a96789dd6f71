"""Are the kernels of two sets of device-assembly files the same instructions?  (No GPU needed.)

    cd eprecon_amd/csrc
    hipcc <the build's compile flags> --cuda-device-only -S unit.hip -o unit.s        # once per translation unit and side
    python tools/kernel_isa_diff.py --a old/back_project.s --b new/back_project.s new/views_to_rows.s ...

For a change that moves kernels between translation units without editing them.  Every file is cut at its kernel symbols (the
names of its `.amdhsa_kernel` descriptors): a kernel's text runs from its label to its `.Lfunc_end`.  Assembler comments and
blank lines are dropped and the function index in basic-block labels (`.LBB<idx>_<n>`), which counts the functions in front of
the kernel in its file, is replaced by a constant.  The texts are then compared for equality, kernel by kernel; the report names
the kernels that are missing from --b, added by it, or different.  Exit status 0 only when there are none.
"""
import argparse
import re
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), flags=re.M))
    out, name, body = {}, None, []
    for line in lines:
        label = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if name is None:
            if label and label.group(1) in names:
                name, body = label.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = "\n".join(body), None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).rstrip()
        if line:
            body.append(line)
    assert name is None and set(out) == names, f"{path}: kernel symbols without a body: {sorted(names - set(out))}"
    return out


def gather(paths):
    merged = {}
    for path in paths:
        for name, text in kernels(path).items():
            assert name not in merged, f"{name} is defined twice on one side"
            merged[name] = text
    return merged


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--a", nargs="+", required=True, help="device assembly of the old translation units")
    ap.add_argument("--b", nargs="+", required=True, help="device assembly of the new translation units")
    args = ap.parse_args()
    a, b = gather(args.a), gather(args.b)
    missing, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    different = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"a: {len(a)} kernels in {len(args.a)} file(s); b: {len(b)} kernels in {len(args.b)} file(s); "
          f"{sum(len(t.splitlines()) for t in a.values())} instruction and label lines compared")
    for title, names in (("missing from b", missing), ("added by b", added), ("different", different)):
        print(f"{title}: {len(names)}")
        for n in names:
            print(f"  {n}")
    return 1 if missing or added or different else 0


if __name__ == "__main__":
    sys.exit(main())
