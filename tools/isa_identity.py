#!/usr/bin/env python3
"""Are the kernels of two builds the same device code?  Compares gfx950 assembly per kernel symbol, as text.

    hipcc <_build.CFLAGS> -I include --cuda-device-only -S old.hip -o old.s        (likewise every new unit)
    python tools/isa_identity.py old.s new_a.s [new_b.s ...] [--diff] > profiles/<round>/isa_identity.txt

The first file is the build to compare against; the kernels of all further files together are the other build (a source
file that was split into units).  Per kernel symbol two things are compared: the instruction stream between the kernel's
label and its end, and its .amdhsa_ resource block.  Comments and blank lines are dropped, and the labels local to a function
(.LBB<function>_<block>, .Lfunc_end<function>), whose numbers depend on the kernel's position in its file, are renumbered
in order of appearance.  Nothing else is normalised and no instruction is looked for by name: equal means equal text.
Exit status 0 if both builds hold the same kernel symbols, each once, and every kernel is identical."""
import re
import sys


def _strip(line):
    return line.split(";", 1)[0].rstrip()


def kernels(path):
    """{symbol: (instruction and label lines, resource block lines)} of one assembly file."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        code, block, in_block, end = [], [], False, None
        for i in range(start + 1, len(lines)):
            l = _strip(lines[i])
            if re.match(r"\.Lfunc_end\d+:", l):
                end = i
                break
            s = l.strip()
            if not s:
                continue
            if s.startswith(".amdhsa_kernel"):
                in_block = True
            elif s.startswith(".end_amdhsa_kernel"):
                in_block = False
            elif in_block:
                block.append(" ".join(s.split()))
            elif s.startswith(".") and not s.startswith(".LBB"):
                continue                      # .section / .p2align / .text around the resource block
            else:
                code.append(" ".join(s.split()))
        assert end is not None and block, f"{path}: {name}: no end label / no resource block"
        assert name not in out, f"{path}: {name} twice"
        out[name] = (_renumber(code), block)
    return out


def _renumber(code):
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), f".LBB_{len(seen)}")
    return [re.sub(r"\.LBB\d+_\d+", sub, l) for l in code]


def _res(block):
    d = dict(l.split(None, 1) for l in block)
    g = lambda k: int(d["." + k])
    arch = g("amdhsa_accum_offset") if ".amdhsa_accum_offset" in d else g("amdhsa_next_free_vgpr")
    return (min(arch, g("amdhsa_next_free_vgpr")), max(g("amdhsa_next_free_vgpr") - arch, 0), g("amdhsa_next_free_sgpr"),
            g("amdhsa_group_segment_fixed_size"), g("amdhsa_private_segment_fixed_size"))


def _short(sym):
    """ume_dist_kernel<true, false> from _ZN6umereg15ume_dist_kernelILb1ELb0EEEv...: name and template arguments, enough to tell the
    instantiations of this library apart (integers, bools, one class of the namespace); anything else stays mangled."""
    m = re.match(r"_ZN6umereg(\d+)", sym)
    if not m:
        return sym
    n, at = int(m.group(1)), m.end()
    if sym[at:at + n] == "_GLOBAL__N_1":          # a kernel of the unit's anonymous namespace: its own name comes next
        m = re.match(r"(\d+)", sym[at + n:])
        if not m:
            return sym
        at += n + m.end()
        n = int(m.group(1))
    name, rest = sym[at:at + n], sym[at + n:]
    if not rest.startswith("I"):
        return name
    args, rest = [], rest[1:]
    while not rest.startswith("E"):
        m = re.match(r"Li(\d+)E|Lb([01])E|NS_(\d+)", rest)
        if not m:
            return sym
        if m.group(3):
            k = int(m.group(3))
            args.append(rest[m.end():m.end() + k])
            rest = rest[m.end() + k + 1:]
        else:
            args.append(m.group(1) or ("false", "true")[int(m.group(2))])
            rest = rest[m.end():]
    return f"{name}<{', '.join(args)}>"


def main(argv):
    show_diff = "--diff" in argv
    files = [a for a in argv if a != "--diff"]
    if len(files) < 2:
        sys.exit(__doc__)
    old = kernels(files[0])
    new, where, dup = {}, {}, []
    for f in files[1:]:
        for name, k in kernels(f).items():
            if name in new:
                dup.append(name)
            new[name], where[name] = k, f.rsplit("/", 1)[-1]
    names = sorted(set(old) | set(new))
    short = {n: _short(n) for n in names}
    ok = not dup and set(old) == set(new)
    print(f"# {files[0].rsplit('/', 1)[-1]}: {len(old)} kernels; {', '.join(f.rsplit('/', 1)[-1] for f in files[1:])}: {len(new)} kernels")
    print(f"# {'kernel':<42} {'unit':<18} {'instr':>6} {'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'LDS':>7} {'scratch':>7}  identical")
    for n in names:
        if n not in old or n not in new:
            print(f"  {short[n]:<42} {where.get(n, '-'):<18} only in the {'first' if n in old else 'other'} build")
            continue
        (c0, b0), (c1, b1) = old[n], new[n]
        n_instr = sum(1 for l in c1 if not l.endswith(":"))
        same_code, same_res = c0 == c1, b0 == b1
        ok = ok and same_code and same_res
        verdict = "yes" if same_code and same_res else "NO (" + ", ".join(w for w, s in (("code", same_code), ("resources", same_res)) if not s) + ")"
        print(f"  {short[n]:<42} {where[n]:<18} {n_instr:>6} " + " ".join(f"{v:>{w}}" for v, w in zip(_res(b1), (5, 5, 5, 7, 7))) + f"  {verdict}")
        if show_diff and not (same_code and same_res):
            import difflib
            for l in difflib.unified_diff(c0 + b0, c1 + b1, "first", "other", lineterm="", n=2):
                print("      " + l)
    for n in dup:
        print(f"  {short[n]}: defined in more than one unit")
    print(f"# {'every kernel identical' if ok else 'DIFFERENCES'}: {len(names)} kernel symbols")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
