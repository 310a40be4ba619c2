"""Is the device code of two source trees the same?  (CPU only.)  Compiles every csrc/*.hip of both trees with the Makefile's flags plus
`-S --cuda-device-only`, normalises the listings (comments, .file / .loc / .ident, debug sections and the per-translation-unit
__hip_cuid_<hash> symbol dropped) and compares them line for line: every instruction, every .amdhsa_ field, the set of kernel symbols.
A listing is kept beside its source (isa/ or isa_bf16/, ignored by git) and reused while no source or header is newer.
Five verdicts per source file: `identical`; `kernels in common identical` (the kernel sets differ only by symbols of FLAT_FILL_ADDED /
FLAT_FILL_REMOVED, and every kernel both trees have is equal: body, .amdhsa_ fields, metadata -- function numbers dropped as below); `operand order only` (same line counts, and the listings become equal once the two source
operands of every instruction in COMMUTATIVE are put in one order -- the kernels it concerns are named); `instance order only` (the
sources in INSTANCE_ORDER: the compiler emitted the same kernels in another order -- every kernel body is equal once the function number
in its .LBB<n>_<m> labels is dropped, and so is the text outside the bodies when it is compared per kernel symbol and not by position);
DIFFERS with the first differing kernel, or `kernel symbols differ` for any other change of the kernel set.  Exit status 0 iff no file
DIFFERS or has such a change.
usage: python tools/isa_diff.py <parent-tree> <new-tree> [--bf16]"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_scan import kernels  # noqa: E402

CSRC = os.path.join("medical-sam2_amd", "csrc")
# Two-source opcodes whose result bits do not depend on the order of the sources (the compiler picks the order from value numbering,
# which moving code into a helper can change).  Extend only with such opcodes, and only as they show up.  Caveat:
# v_mul_f32 of two NaNs propagates the payload of one source -- which one depends on the order.
COMMUTATIVE = ("s_add_i32", "s_mul_i32", "v_mul_f32_e32")
# Sources whose host dispatch instantiates its kernels from a template (common.h: with_type), which emits them in another order than the
# if / else ladders did.  The order shows in two places only: the function number <n> of the local labels, and the position of a kernel's
# sections, .set lines and metadata entry in the file.  Extend only with sources where that is the cause.
INSTANCE_ORDER = ("backward.hip", "conv.hip", "elementwise.hip")
# The one change of the kernel SET that is accepted: the flat zero fills that three sources spelled out gave way to common.h's fill_kernel<int>
# (the symbols in full: (anonymous namespace)::fill_kernel<int>(int*, long, int), cc_zero_kernel(int*, long), cmp_zero_kernel(int*, long),
# label_zero_kernel(int*, int)).  Every kernel the two trees share must still be equal, body and per-symbol blocks.  Extend only with symbols
# whose coming or going is the whole point of a change.
FLAT_FILL_ADDED = ("_ZN12_GLOBAL__N_111fill_kernelIiEEvPT_lS1_",)
FLAT_FILL_REMOVED = ("_ZN12_GLOBAL__N_114cc_zero_kernelEPil", "_ZN12_GLOBAL__N_115cmp_zero_kernelEPil", "_ZN12_GLOBAL__N_117label_zero_kernelEPii")
FUNC_NUMBER_RE =re.compile(r"\.(LBB|Lfunc_end)\d+")
COMMUTATIVE_RE = re.compile(r"^(\s*(?:%s)\s+[^,]+),\s*([^,]+),\s*([^,]+)$" % "|".join(COMMUTATIVE))


def make_var(makefile, name):
    return re.search(rf"^{name}\s*[:?]?=\s*(.*)$", makefile, re.M).group(1).strip()


def listing(tree, src, bf16):
    """Path of the ISA listing of `src` in `tree`, compiled if stale."""
    csrc = os.path.join(tree, CSRC)
    mk = open(os.path.join(csrc, "Makefile")).read()
    extra = "-DMSAM2_OPERAND_BF16" if bf16 else ""
    flags = make_var(mk, "FLAGS").replace("$(ARCH)", make_var(mk, "ARCH")).replace("$(EXTRA)", extra).split()
    out = os.path.join(csrc, "isa_bf16" if bf16 else "isa", src[:-4] + ".s")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if f == src or f.endswith(".h") or f == "Makefile"]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([make_var(mk, "HIPCC")] + flags + ["-S", "--cuda-device-only", "-o", out, src], cwd=csrc,
                              stderr=subprocess.DEVNULL)
    return out


def normalised(path):
    keep, debug = [], False
    for line in open(path):
        line = re.sub(r"\s*;.*$", "", line.rstrip())
        s = line.strip()
        if s.startswith(".section"):
            debug = ".debug" in s
        if debug or not s or s.startswith(("//", ".file", ".loc", ".ident")) or "__hip_cuid_" in s:
            continue
        keep.append(line)
    return "\n".join(keep) + "\n"


def canonical(line):
    m = COMMUTATIVE_RE.match(line)
    return "%s, %s, %s" % ((m.group(1),) + tuple(sorted(m.group(2, 3)))) if m else line


def by_symbol(text):
    """(kernel bodies, text outside the bodies) of a normalised listing, function numbers dropped.  The outside text is cut into blocks at
    every .section and at every kernel entry of the metadata; a block belongs to the first symbol it names (a list per symbol, in file
    order), the blocks that name none keep their order under the key None."""
    text = FUNC_NUMBER_RE.sub(r".\1", re.sub(r"^(_Z\w+):$", r"\1: ", text, flags=re.M))
    bodies, outside, block, in_body = dict(kernels(text)), {}, [], False

    def close():
        if block:
            m = re.search(r"_Z\w+", "\n".join(block))
            outside.setdefault(m.group(0) if m else None, []).append(list(block))
            block.clear()
    for line in text.split("\n"):
        if in_body:
            in_body = not (line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"))   # (as isa_scan.kernels ends a body)
        elif re.match(r"^_Z\w+:\s", line):
            in_body = True
        else:
            if line.startswith(("\t.section", "  - .", "amdhsa.")):
                close()
            block.append(line)
    close()
    return bodies, outside


def compare(a, b, src=""):
    if a == b:
        return "identical (%d lines)" % a.count("\n")
    ka, kb = (dict(kernels(re.sub(r"^(_Z\w+):$", r"\1: ", t, flags=re.M))) for t in (a, b))
    if set(ka) != set(kb):
        removed, added = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        (ba, oa), (bb, ob) = by_symbol(a), by_symbol(b)
        for d in (ba, oa, bb, ob):
            for sym in removed + added:
                d.pop(sym, None)
        for d in (oa, ob):                                      # a kernel leaves one .section line behind that names nobody (its body: comments)
            d[None] = [blk for blk in d.get(None, []) if not (len(blk) == 1 and blk[0].startswith("\t.section"))]
        if set(removed) <= set(FLAT_FILL_REMOVED) and set(added) <= set(FLAT_FILL_ADDED) and (ba, oa) == (bb, ob):
            return "kernels in common identical (%d: bodies, .amdhsa_ fields and metadata); added %s; removed %s" % (len(ba), added, removed)
        return "kernel symbols differ: only in parent %s, only in new %s" % (removed, added)
    if src in INSTANCE_ORDER and by_symbol(a) == by_symbol(b):
        moved = sum(x != y for x, y in zip(ka, kb))
        return "instance order only (one of %s): %d of %d kernels emitted at another position, every body and every per-symbol block equal" % (
            ", ".join(INSTANCE_ORDER), moved, len(ka))
    swapped = []
    for name in ka:
        if ka[name] != kb[name]:
            if len(ka[name]) == len(kb[name]) and [canonical(l) for l in ka[name]] == [canonical(l) for l in kb[name]]:
                swapped.append(name)
                continue
            n = next((i for i, (x, y) in enumerate(zip(ka[name], kb[name])) if x != y), min(len(ka[name]), len(kb[name])))
            return "DIFFERS: %s at its line %d (%d / %d lines)" % (name, n, len(ka[name]), len(kb[name]))
    if [canonical(l) for l in a.split("\n")] != [canonical(l) for l in b.split("\n")]:
        return "DIFFERS outside the kernel bodies (metadata or .amdhsa_ fields)"
    return "operand order only (%s) in %d of %d kernels, the others identical:\n  %s" % (
        ", ".join(COMMUTATIVE), len(swapped), len(ka), "\n  ".join(swapped))


def main():
    args = [os.path.abspath(a) for a in sys.argv[1:] if a != "--bf16"]   # (the compiler runs inside csrc/)
    bf16 = "--bf16" in sys.argv
    if len(args) != 2:
        sys.exit(__doc__)
    srcs = sorted(f for f in os.listdir(os.path.join(args[1], CSRC)) if f.endswith(".hip"))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        jobs = {(t, s): pool.submit(listing, t, s, bf16) for s in srcs for t in dict.fromkeys(args)}
        bad = 0
        for s in srcs:
            verdict = compare(normalised(jobs[args[0], s].result()), normalised(jobs[args[1], s].result()), s)
            bad += verdict.startswith("DIFFERS") or verdict.startswith("kernel symbols differ")
            print("%-20s %s" % (s, verdict), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
