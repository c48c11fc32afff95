"""The compiled code of csrc/hsq_encode_pf.hip's kernels, this tree against another checkout (the parent commit), kernel by kernel.

    python tools/pf_isa_compare.py --parent DIR [--out profiles/hsq_zero_pf_isa.txt]

DIR is a checkout of the commit to compare with (`git worktree add DIR HEAD~1`, or `git archive` unpacked).  Both trees' file is
compiled with build.py's flags + --save-temps into scratch directories (no GPU needed); the kernels are matched by their mangled
names (the template arguments: code type, D, batched, EF, segment records in LDS, DR, row blocks).  Per kernel: the instruction
count (the .s text of the function, labels, directives and comments dropped), registers, scratch and LDS bytes of the kernel's
metadata, both sides, and whether the instruction text is the same once the labels are renumbered.  Whole texts and numbers are
compared; no instruction is looked for (tools/mx_isa_compare.py's method).
Exit status 1 if an instantiation with DR == D (d = 8, 16, 32: bench.py's configurations) has other instruction text than the
parent's."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_isa_compare as mx  # noqa: E402  (build_asm, the label renumbering, META)

ROOT = mx.ROOT
NAME = "hsq_encode_pf.hip"


def kernels(txt):
    """mangled name -> (instruction lines with the labels renumbered, the kernel's metadata numbers)."""
    out = {}
    for m in re.finditer(r"^(_ZN2gq20hsq_encode_pf_kernel\w+):", txt, re.M):
        sym = m.group(1)
        body = txt[m.end():txt.index(".Lfunc_end", m.end())]
        lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
        lines = [ln for ln in lines if ln and not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln)]
        order = {}
        for ln in lines:
            lab = re.match(r"(\.LBB\d+_\d+):", ln)
            if lab:
                order[lab.group(1)] = "L%d" % len(order)
        text = [re.sub(r"\.LBB\d+_\d+", lambda g: order.get(g.group(0), g.group(0)), ln) for ln in lines]
        k = txt.index(".name:           " + sym + "\n", txt.index("amdhsa.kernels:"))
        start = txt.rindex("\n  - ", 0, k)
        end = txt.find("\n  - ", k)
        entry = txt[start:end if end > 0 else len(txt)]
        meta = {f: int(re.search(r"^\s+%s:\s+(\d+)" % re.escape(f), entry, re.M).group(1)) for f in mx.META}
        meta["instructions"] = sum(1 for ln in text if not ln.endswith(":"))
        out[sym] = (text, meta)
    return out


def shape_of(sym):
    """(code type, D, batched, ef, seglds, DR, NRB) from hsq_encode_pf_kernel<CodeT, D, BATCHED, EF, SEGLDS, DR, NRB>."""
    m = re.search(r"hsq_encode_pf_kernelI([hi])Li(\d+)ELb([01])ELb([01])ELb([01])ELi(\d+)ELi(\d+)E", sym)
    assert m, sym
    return ("u8" if m.group(1) == "h" else "i32",) + tuple(int(x) for x in m.groups()[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the commit to compare with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hsq_zero_pf_isa.txt"))
    a = ap.parse_args()
    old, new = kernels(mx.build_asm(os.path.abspath(a.parent), NAME)), kernels(mx.build_asm(ROOT, NAME))
    assert sorted(old) == sorted(new) and new, "%d kernels against %d" % (len(old), len(new))
    rows, bad, differ = [], [], 0
    for sym in sorted(new, key=shape_of):
        (t0, m0), (t1, m1) = old[sym], new[sym]
        ct, D, bat, ef, seglds, DR, nrb = shape_of(sym)
        same = t0 == t1
        differ += not same
        rows.append("%-3s D=%-2d DR=%-2d batched=%d ef=%d seglds=%d nrb=%d  %5d %5d  %3d %3d  %3d %3d  %d %d  %6d %6d  %s"
                    % (ct, D, DR, bat, ef, seglds, nrb, m0["instructions"], m1["instructions"], m0[".vgpr_count"], m1[".vgpr_count"],
                       m0[".sgpr_count"], m1[".sgpr_count"], m0[".private_segment_fixed_size"], m1[".private_segment_fixed_size"],
                       m0[".group_segment_fixed_size"], m1[".group_segment_fixed_size"], "identical" if same else "DIFFERS"))
        if DR == D and not same:
            bad.append("D = DR = %d (%s): other instruction text than the parent's" % (D, sym))
    ndr = sum(1 for s in new if shape_of(s)[1] == shape_of(s)[5])
    head = ["# tools/pf_isa_compare.py: the kernels of hsq_encode_pf.hip, the parent commit against this tree (gfx950, build.py's flags).",
            "# columns: code type, template arguments | instructions parent new | VGPRs parent new | SGPRs parent new |",
            "#          scratch bytes parent new | LDS bytes parent new | instruction text with labels renumbered",
            "# %d kernels, %d with other instruction text than the parent's; %d with DR == D, %d of those differ" % (len(rows), differ, ndr, len(bad))]
    with open(a.out, "w") as f:
        f.write("\n".join(head + rows) + "\n")
    print("\n".join(head[3:] + bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
