"""Compare the device assembly of two builds kernel by kernel (a refactor's "no instruction changed" check).

    python tools/isa_diff.py <dir_a> <dir_b> [-v]

Each directory holds the .s files of `hipcc <the Makefile's FLAGS> --offload-device-only -S` for every .hip file
(any file names: kernels are matched by symbol across all files of a directory, so a kernel may move between
files).  For every `.amdhsa_kernel` symbol two texts are compared byte for byte: the instruction text from the
symbol's label to its .Lfunc_end label, and the .amdhsa_* descriptor block.  Only the per-function number of the
local labels (.LBB<n>_<k>, BB<n>_<k> in comments, .Lfunc_end<n>) is normalised out, with the padding in front of
a comment on such a line: the number is the kernel's position in its file.  Prints same/different per kernel (the first differing line of a different one) and exits non-zero on
any difference or when the symbol sets differ (missing, added or duplicated kernels).
"""
import glob
import os
import re
import sys

LOCAL = re.compile(r"(\.L|\b)BB\d+_(\d+)")
PAD = re.compile(r"\s+;")
FUNC_END =re.compile(r"^\.Lfunc_end\d+:")


def kernels(directory):
    """symbol -> (code lines, descriptor lines); duplicates listed apart."""
    out, dups = {}, []
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        names = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
        i = 0
        while i < len(lines):
            sym = lines[i].split(":")[0]
            if lines[i][:1] not in "\t .;" and sym in names and lines[i].startswith(sym + ":"):
                code, desc, in_desc = [], [], False
                for j in range(i, len(lines)):
                    l = lines[j]
                    if FUNC_END.match(l):
                        break
                    s = l.strip()
                    if s.startswith(".amdhsa_kernel "):
                        in_desc = True
                    l, n = LOCAL.subn(r"\1BB_\2", l)
                    if n:  # a label's length moves the column of the comment after it
                        l = PAD.sub(" ;", l)
                    (desc if in_desc else code).append(l)
                    if s == ".end_amdhsa_kernel":
                        in_desc = False
                if sym in out:
                    dups.append(sym)
                out[sym] = (code, desc)
                i = j
            i += 1
        for n in names - set(out):
            print(f"{path}: descriptor of {n} without a function body", file=sys.stderr)
    return out, dups


def first_diff(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return k, x, y
    k = min(len(a), len(b))
    return k, (a[k] if k < len(a) else "<end>"), (b[k] if k < len(b) else "<end>")


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    (ka, da), (kb, db) = kernels(args[0]), kernels(args[1])
    bad = 0
    for name, dups in ((args[0], da), (args[1], db)):
        for s in dups:
            print(f"DUPLICATE in {name}: {s}")
            bad += 1
    for s in sorted(set(ka) - set(kb)):
        print(f"MISSING in {args[1]}: {s}")
        bad += 1
    for s in sorted(set(kb) - set(ka)):
        print(f"ADDED in {args[1]}: {s}")
        bad += 1
    same = 0
    for s in sorted(set(ka) & set(kb)):
        what = None
        for part, x, y in (("code", ka[s][0], kb[s][0]), ("descriptor", ka[s][1], kb[s][1])):
            if x != y:
                what = (part,) + first_diff(x, y)
                break
        if what is None:
            same += 1
            if verbose:
                print(f"same      {s}")
        else:
            bad += 1
            print(f"DIFFERENT {s}: {what[0]} line {what[1]}\n  a: {what[2].strip()}\n  b: {what[3].strip()}")
    print(f"{len(ka)} kernels in {args[0]}, {len(kb)} in {args[1]}: {same} same, {bad} problems")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
