"""Same machine code across a refactor: compares the multisets of kernel bodies
of two sets of device assembly listings (hipcc with the Makefile's flags plus
--cuda-device-only -S, one listing per source file).

usage: python tools/kernel_body_diff.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...]

A body runs from the kernel's label to its .Lfunc_end.  Normalised away: the
kernel's own mangled name (template parameters may be renamed or dropped), the
.LBB<n>_ function index, trailing ; comments, the mangled name of the
per-file zero page s3_zero_src and the directive that returns to the kernel's
text section after its descriptor (.text for a plain kernel, a comdat .section
for a template instance: a kernel may become one).  Prints the kernel counts and whether the
multisets are equal; otherwise the demangled names on either side whose body
has no partner (exit status 1).  CPU only."""
import collections
import hashlib
import re
import subprocess
import sys


def bodies(path):
    txt = open(path).read().split("\n")
    names = [ln.split()[1] for ln in txt if ln.strip().startswith(".amdhsa_kernel ")]
    label = {}
    for i, ln in enumerate(txt):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            label[m.group(1)] = i
    out = []
    for n in names:
        body = []
        j = label[n] + 1
        while not txt[j].startswith(".Lfunc_end"):
            ln = txt[j].split(";")[0].rstrip().replace(n, "KERNEL")
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"_ZN2rrL?11s3_zero_srcE[\w.$]*", "ZEROSRC", ln)
            ln = re.sub(r"^\s*\.section\s+\.text\.KERNEL,.*$", "\t.text", ln)
            if ln.strip():
                body.append(ln)
            j += 1
        out.append((n, hashlib.sha256("\n".join(body).encode()).hexdigest(), len(body)))
    return out


def demangle(names):
    return subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True).stdout.split("\n")


def main():
    args = sys.argv[1:]
    if "--" not in args:
        sys.exit(__doc__)
    k = args.index("--")
    old = [b for p in args[:k] for b in bodies(p)]
    new = [b for p in args[k + 1:] for b in bodies(p)]
    co = collections.Counter(h for _, h, _ in old)
    cn = collections.Counter(h for _, h, _ in new)
    print(f"kernels: old {len(old)}, new {len(new)}; multisets equal: {co == cn}")
    for tag, side, extra in (("old", old, co - cn), ("new", new, cn - co)):
        lone = [(n, ln) for n, h, ln in side if extra[h] > 0]
        for d, (_, ln) in zip(demangle([n for n, _ in lone]), lone):
            print(f"  only in {tag} ({ln} lines): {d}")
    return 0 if co == cn else 1


if __name__ == "__main__":
    sys.exit(main())
