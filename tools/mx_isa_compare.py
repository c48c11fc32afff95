"""The compiled code of a family of libraries' kernels, this tree against another checkout (the parent commit), kernel by kernel.

    python tools/mx_isa_compare.py --parent DIR [--family mx] [--family rotq] [--family sparse] [--out profiles/<family>_refactor_isa.txt]

DIR is a checkout of the commit to compare with (`git worktree add DIR HEAD~1`, or `git archive` unpacked).  A family (FAMILIES
below) is a list of csrc files, the number of kernels each holds and a key function:
    mx    mx.hip and mxr.hip, 2 x 56 kernels (csrc/mx_kernels.hpp), matched by library, kind (compress / decode), format, draw
          mode, error feedback and tensor type;
    rotq  drive.hip and eden.hip, 15 + 45 kernels (csrc/rotq_kernels.hpp), matched by library, kind (compress / decode /
          decode-streams), bits, scale mode, error feedback and rotation kind (Signs / Stepped / Streamed);
    sparse topk.hip, stc.hip, thr.hip and maurey.hip, 4 x 9 kernels (csrc/sparse_kernels.hpp), matched by library, the launch's
          stage (the word in front of `_kernel`) and error feedback.
Both trees' files are compiled with build.py's flags + --save-temps into scratch directories (no GPU needed); a kernel's key is
read off the template arguments in its mangled name, whatever the function itself is called.  Per kernel: the instruction count
(the .s text of the function, labels, directives and comments dropped), the registers and the scratch / LDS bytes of the kernel's
metadata, both sides, and whether the instruction text is the same once the labels are renumbered.  Whole texts and numbers are
compared; no instruction is looked for.  With one --family and no --out the result goes to profiles/<family>_refactor_isa.txt;
several families (a change to a header both share) go into the first one's file.
Exit status 1 if a kernel has scratch or LDS (mx, rotq: kernels that stay in registers) or other scratch or LDS bytes than the other
tree's (sparse: kernels that use LDS by design), or if its VGPR count falls into a lower waves-per-SIMD class than the other tree's.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gradient-quantization_amd"
FMT = {0: "fp4", 1: "fp8", 0x23: "fp6_e2m3", 0x32: "fp6_e3m2"}
MODE = {0: "off", 1: "given", 2: "device"}
TT = {0: "f32", 1: "bf16"}
SCALE = {0: "unbiased", 1: "mse"}
META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def build_asm(root, name):
    """The gfx950 assembly of root's csrc/<name>, compiled with root's own build flags."""
    spec = importlib.util.spec_from_file_location("gq_build_" + str(abs(hash(root))), os.path.join(root, PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    d = tempfile.mkdtemp(prefix="gq_mx_isa_")
    flags = [f for f in b.FLAGS if f != "-shared"] + b.EXTRA.get(name, [])
    subprocess.check_call([b.hipcc()] + flags + ["--save-temps", "-c", os.path.join(root, PKG, "csrc", name), "-o", os.path.join(d, "x.o")],
                          cwd=d, stderr=subprocess.DEVNULL)
    return open(os.path.join(d, [f for f in os.listdir(d) if f.endswith("gfx950.s")][0])).read()


def template_args(symbol):
    """The template-argument part of a kernel's mangled name ('' if it is no template) and the integers among the arguments."""
    part = symbol[:symbol.index("EEv")] + "E" if "EEv" in symbol else ""
    return part, [int(v) for v in re.findall(r"L[ib](\d+)E", part)]


def mx_key(symbol):
    """(kind, format, mode, ef, tensor type) of a kernel of mx.hip / mxr.hip."""
    kind = "compress" if "compress_kernel" in symbol else "decode"
    args = template_args(symbol)[1]
    if kind == "compress":
        fmt, mode, ef, tt = args
        return kind, FMT[fmt], MODE[mode], "ef" if ef else "-", TT[tt]
    fmt, tt = args
    return kind, FMT[fmt], "-", "-", TT[tt]


def rotq_key(symbol):
    """(kind, bits, scale mode, ef, rotation kind) of a kernel of drive.hip / eden.hip: the integers are [bits,] scale, ef of a
    compress and [bits] of a decode -- one bit where no width is an argument -- and the rotation is the last argument's type."""
    kind = "compress" if "compress_kernel" in symbol else "decode-streams" if "decode_streams_kernel" in symbol else "decode"
    part, args = template_args(symbol)
    rot = re.findall(r"\d(Signs|Stepped|Streamed)E", part)
    if kind == "compress":
        scale, ef = args[-2:]
        return kind, "b%d" % (args[0] if len(args) == 3 else 1), SCALE[scale], "ef" if ef else "-", rot[0]
    return kind, "b%d" % (args[0] if args else 1), "-", "-", rot[0] if kind == "decode" else "-"


def sparse_key(symbol):
    """(stage, ef) of a kernel of topk.hip / stc.hip / thr.hip / maurey.hip: the stage is the word in front of `_kernel`, whatever
    library or header the function is named after; ef is the bool among the template arguments ('-' where there is none)."""
    stage = re.search(r"(hist|pick|count|scan|write|decode|reduce|sum|offsets|place|item)_kernel", symbol).group(1)
    ef = re.findall(r"Lb(\d)E", template_args(symbol)[0])
    return stage, ("ef" if int(ef[-1]) else "noef") if ef else "-"


# family -> ((csrc file, kernels in it), ...), the key function, the key's column names and format, whether its kernels stay in
# registers (any scratch or LDS is an error) or use LDS by design (other bytes than the parent's are)
FAMILIES = {
    "mx": ((("mx.hip", 56), ("mxr.hip", 56)), mx_key, "kind format mode ef type", "%-8s %-8s %-6s %-2s %-4s", True),
    "rotq": ((("drive.hip", 15), ("eden.hip", 45)), rotq_key, "kind bits scale ef rotation", "%-14s %-2s %-8s %-2s %-8s", True),
    "sparse": ((("topk.hip", 9), ("stc.hip", 9), ("thr.hip", 9), ("maurey.hip", 9)), sparse_key, "stage ef", "%-7s %-4s", False),
}


def kernels(txt, key_of):
    """key -> (instruction lines with the labels renumbered, the kernel's metadata numbers)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+_kernel\w+):", txt, re.M):
        sym = m.group(1)
        body = txt[m.end():txt.index(".Lfunc_end", m.end())]
        lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
        lines = [ln for ln in lines if ln and not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln)]
        order = {}
        for ln in lines:                                   # labels by order of definition: the function's number drops out
            lab = re.match(r"(\.LBB\d+_\d+):", ln)
            if lab:
                order[lab.group(1)] = "L%d" % len(order)
        text = [re.sub(r"\.LBB\d+_\d+", lambda g: order.get(g.group(0), g.group(0)), ln) for ln in lines]
        k = txt.index(".name:           " + sym + "\n", txt.index("amdhsa.kernels:"))
        start = txt.rindex("\n  - ", 0, k)
        end = txt.find("\n  - ", k)
        entry = txt[start:end if end > 0 else len(txt)]
        meta = {f: int(re.search(r"^\s+%s:\s+(\d+)" % re.escape(f), entry, re.M).group(1)) for f in META}
        meta["instructions"] = sum(1 for ln in text if not ln.endswith(":"))
        assert key_of(sym) not in out, "two kernels with the key %s" % (key_of(sym),)
        out[key_of(sym)] = (text, meta)
    return out


def waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per SIMD lane, handed out in blocks of 8, at most 8 waves."""
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the commit to compare with")
    ap.add_argument("--family", action="append", choices=sorted(FAMILIES), help="default: mx")
    ap.add_argument("--out", help="default: profiles/<the first family>_refactor_isa.txt")
    a = ap.parse_args()
    families = a.family or ["mx"]
    out = a.out or os.path.join(ROOT, "profiles", families[0] + "_refactor_isa.txt")
    text, bad, total, differ = [], [], 0, 0
    for fam in families:
        files, key_of, columns, fmt, in_registers = FAMILIES[fam]
        text += ["# tools/mx_isa_compare.py: the kernels of %s, the parent commit against this tree (gfx950, build.py's flags)."
                 % (", ".join(name for name, _ in files[:-1]) + " and " + files[-1][0]),
                 "# columns: library %s | instructions parent new | VGPRs parent new | SGPRs parent new |" % columns,
                 "#          scratch bytes parent new | LDS bytes parent new | instruction text with labels renumbered"]
        for name, count in files:
            old, new = kernels(build_asm(os.path.abspath(a.parent), name), key_of), kernels(build_asm(ROOT, name), key_of)
            assert sorted(old) == sorted(new) and len(new) == count, "%s: %d kernels against %d, %d expected" % (name, len(old), len(new), count)
            for key in sorted(new):
                (t0, m0), (t1, m1) = old[key], new[key]
                same = t0 == t1
                total, differ = total + 1, differ + (not same)
                text.append(("%%-%ds " % max(5, max(len(n) - 4 for n, _ in files)) + fmt + "  %5d %5d  %3d %3d  %3d %3d  %d %d  %d %d  %s")
                            % ((name[:-4],) + key + (m0["instructions"], m1["instructions"], m0[".vgpr_count"], m1[".vgpr_count"],
                                                     m0[".sgpr_count"], m1[".sgpr_count"], m0[".private_segment_fixed_size"],
                                                     m1[".private_segment_fixed_size"], m0[".group_segment_fixed_size"],
                                                     m1[".group_segment_fixed_size"], "identical" if same else "DIFFERS")))
                if in_registers and (m1[".private_segment_fixed_size"] or m1[".group_segment_fixed_size"]):
                    bad.append("%s %s: scratch or LDS" % (name, key))
                for what, field in (("scratch", ".private_segment_fixed_size"), ("LDS", ".group_segment_fixed_size")):
                    if not in_registers and m1[field] != m0[field]:
                        bad.append("%s %s: %d bytes of %s against %d" % (name, key, m1[field], what, m0[field]))
                if waves_per_simd(m1[".vgpr_count"]) < waves_per_simd(m0[".vgpr_count"]):
                    bad.append("%s %s: %d VGPRs against %d: fewer waves per SIMD" % (name, key, m1[".vgpr_count"], m0[".vgpr_count"]))
    tail = "# %d kernels, %d with other instruction text than the parent's" % (total, differ)
    with open(out, "w") as f:
        f.write("\n".join(text + [tail]) + "\n")
    print("\n".join([tail] + bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
