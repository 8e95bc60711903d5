"""Compare two device-assembly files of sacenv_boat.hip kernel by kernel.

    python tools/kernel_diff.py PARENT.s HEAD.s

An argument that ends in .hip is compiled first (isa_hist.asm_text: the
library's flags, --cuda-device-only -S). Compared: the set of kernel names;
each kernel's body (and that of any device function kept out of line) with
comments stripped and the function ordinal in local
labels (.LBB<n>_, .LJTI<n>_, .Ltmp<n>_) normalised, so that the order in which
the compiler emits the kernels does not count; each .amdhsa_kernel block
(registers, LDS, scratch). Prints the names that differ and exits non-zero on
any difference: a host-side refactor must leave every kernel as it was.
"""
import re
import sys

import isa_hist

LOCAL = re.compile(r"\.L(BB|JTI|tmp)\d+_")


def clean(lines):
    out = []
    for l in lines:
        l = LOCAL.sub(r".L\1N_", l.split(";")[0]).strip()
        if l:
            out.append(l)
    return out


def descriptors(text):
    """{kernel name: its .amdhsa_kernel block}"""
    out, cur = {}, None
    for l in text.split("\n"):
        s = l.strip()
        if s.startswith(".amdhsa_kernel "):
            cur = out.setdefault(s.split()[1], [])
        elif s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None:
            cur.append(l)
    return {k: clean(v) for k, v in out.items()}


def load(arg):
    text = isa_hist.asm_text(arg) if arg.endswith(".hip") else open(arg).read()
    # (every function the file emits: the kernels and any device function kept out of line)
    return {n: clean(b) for n, b in isa_hist.split_kernels(text).items()}, descriptors(text)


def main(a, b):
    (fa, da), (fb, db) = load(a), load(b)
    bad = []
    for what, x, y in (("body", fa, fb), ("descriptor", da, db)):
        bad += [f"{what} only in {a}: {n}" for n in sorted(set(x) - set(y))]
        bad += [f"{what} only in {b}: {n}" for n in sorted(set(y) - set(x))]
        bad += [f"{what} differs: {n} ({len(x[n])} / {len(y[n])} lines)" for n in sorted(set(x) & set(y)) if x[n] != y[n]]
    bad += [f"kernel without a body: {n}" for n in sorted((set(da) - set(fa)) | (set(db) - set(fb)))]
    print("\n".join(bad + [f"{len(da)} / {len(db)} kernels, {len(fa)} / {len(fb)} functions, {len(bad)} differences"]))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
