"""Compare two `hipcc -S --cuda-device-only` assemblies kernel by kernel, whatever order the kernels were emitted in.

    python scripts/isa_kernel_diff.py parent.s branch.s

Every function — from its `-- Begin function <symbol>` line to `-- End function`: the body and the `.amdhsa_kernel`
descriptor that follows it — is keyed by its symbol and compared as text; local labels carry the function's ordinal in
the file (.LBB12_3) and are renumbered, runs of blanks count as one.  Nothing else is read: the order of the functions, the section directives between
them, the metadata note and the ident lines are excluded.  Prints the symbols that
differ or exist on one side only and exits 1 if there are any."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"; -- Begin function (\S+)\n.*?; -- End function", text, re.S):
        body, names = m.group(0), {}
        body = re.sub(r"(\.LBB|\.Lfunc_begin|\.Lfunc_end|\.Ltmp|BB)(\d+)", lambda g: g.group(1) + names.setdefault(g.group(2), str(len(names))), body)
        body = re.sub(r"[ \t]+", " ", body)   # the comment column moves with the width of the renumbered labels
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = body
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
desc = sum(v.count(".amdhsa_kernel ") for v in a.values())
print(f"{len(a)} / {len(b)} function sections, {desc} kernel descriptors compared, {len(bad)} differ")
for k in bad:
    print(" ", k)
sys.exit(1 if bad else 0)
