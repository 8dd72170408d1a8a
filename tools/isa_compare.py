"""Dev tool: compare the compiled kernels of two builds of one source, instantiation by instantiation.  No GPU needed.

    python tools/isa_compare.py <before.s> <after.s> <kernel-name-substring> [--rename='<regex>=><replacement>' ...] [-v]

The .s files are hipcc's gfx950 assembly of the same .hip file in two trees (tools/isa_wait_audit.py compile_s, or
`hipcc <build flags> --cuda-device-only -S`).  Kernels are matched by demangled name after the `--rename` substitutions on the
BEFORE side (a refactor that renames a kernel or adds a template argument says how the old spelling maps to the new).  Symbol and label names
are normalised.  Per instantiation: instructions before / after, differing lines, and the verdict
  identical    the same instruction stream
  reordered    the same multiset of instructions in another order
  renamed      the same multiset once register numbers are masked (two values swapped registers), in another order
  CHANGED      anything else
and VGPRs, AGPRs, SGPRs, static LDS bytes, kernarg bytes and scratch bytes (`a->b` where they differ; a differing figure makes
the verdict CHANGED)."""
import collections
import difflib
import re
import subprocess
import sys

META = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "LDSByteSize", "kernarg", "ScratchSize")


def parse(path, part):
    text = open(path).read()
    lines = text.split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", lines[i])
        if not (m and part in m.group(1)):
            i += 1
            continue
        name, body, meta = m.group(1), [], {}
        i += 1
        while not lines[i].startswith(".Lfunc_end"):
            t = re.sub(r"\s*;.*$", "", lines[i].strip())
            if t and (not t.startswith(".") or re.match(r"^\.LBB\d+_\d+:", t)):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", t)))
            i += 1
        while i < len(lines) and not re.match(r"^_Z\w+:", lines[i]):
            mm = re.match(r"^; (\w+): (\d+)", lines[i])
            if mm and mm.group(1) in META:
                meta[mm.group(1)] = int(mm.group(2))
            i += 1
        block = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", text, re.S)
        meta["kernarg"] = int(re.search(r"\.amdhsa_kernarg_size (\d+)", block.group(1)).group(1))
        out[name] = (body, meta)
    return out


def demangled(kernels, renames):
    names = list(kernels)
    plain = subprocess.check_output(["c++filt"] + names, text=True).strip().split("\n")
    out = {}
    for n, d in zip(names, plain):
        d = re.sub(r"^void |\(.*\)$", "", d).replace("mxvl::", "")
        for pat, rep in renames:
            d = re.sub(pat, rep, d)
        out[d] = kernels[n]
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "-v" and not a.startswith("--rename=")]
    renames = [a[len("--rename="):].split("=>") for a in sys.argv[1:] if a.startswith("--rename=")]
    before, after = (demangled(parse(p, args[2]), r) for p, r in ((args[0], renames), (args[1], [])))
    if set(before) != set(after):
        sys.exit("unmatched kernels:\n  " + "\n  ".join(sorted(set(before) ^ set(after))))
    mask = lambda ins: collections.Counter(re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", x) for x in ins)
    print(f"{'kernel':80s} {'insts':>11s} {'lines':>5s} {'verdict':>9s}  vgpr agpr sgpr lds kernarg scratch")
    tally = collections.Counter()
    for k in sorted(before):
        (ia, ma), (ib, mb) = before[k], after[k]
        d = [x for x in difflib.unified_diff(ia, ib, lineterm="", n=0) if x[0] in "+-" and not x.startswith(("+++", "---"))]
        verdict = ("identical" if ia == ib else "CHANGED" if ma != mb else "reordered" if collections.Counter(ia) == collections.Counter(ib)
                   else "renamed" if mask(ia) == mask(ib) else "CHANGED")
        tally[verdict] += 1
        cols = " ".join(str(ma[m]) if ma[m] == mb[m] else f"{ma[m]}->{mb[m]}" for m in META)
        print(f"{k:80s} {len(ia):5d}/{len(ib):5d} {len(d):5d} {verdict:>9s}  {cols}")
        if "-v" in sys.argv and d:
            print("\n".join("      " + x for x in d))
    print("# " + ", ".join(f"{v} {k}" for k, v in sorted(tally.items())))


if __name__ == "__main__":
    main()
