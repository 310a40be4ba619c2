"""The library pre-sets its tables and workspaces with ONE kernel, never with memset / memcpy calls (csrc/common.h: fill_kernel, DESIGN 7.2:
as nodes of a captured graph those did not order reliably against the neighbouring kernel nodes).  Read from the sources; no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medical-sam2_amd", "csrc")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
# a string or character literal (kept), or a comment (dropped)
TOKEN = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)


def code(path):
    """the source without its comments"""
    return TOKEN.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", open(path).read())


def test_the_comment_stripper():
    src = 'a = "// not a comment"; // hipMemsetAsync(x)\nb /* hipMemcpy\n(y) */ = \'"\'; hipMemsetAsync(z); // "\n'
    stripped = TOKEN.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", src)
    assert '"// not a comment"' in stripped and stripped.count("hipMem") == 1 and "hipMemsetAsync(z)" in stripped


def test_no_memset_or_memcpy_call_in_the_library():
    assert len(SOURCES) > 25
    found = [(os.path.basename(p), m.group(0)) for p in SOURCES for m in re.finditer(r"\bhipMem(?:set|cpy)\w*", code(p))]
    assert not found, found


def test_the_flat_fill_is_defined_once():
    flat = re.compile(r"template\s*<\s*typename\s+\w+\s*>\s*__global__\s+void\s+fill_kernel\s*\(")
    named = re.compile(r"__global__[^;{()]*\bvoid\s+fill_kernel\s*\(")
    where = {os.path.basename(p): (len(flat.findall(code(p))), len(named.findall(code(p)))) for p in SOURCES}
    assert {f: c for f, c in where.items() if c[0]} == {"common.h": (1, 1)}
    # the only other kernel of that name is cc.hip's hole fill (labels, areas, a value for the small components): no flat fill, and older
    assert {f: c for f, c in where.items() if c[1] and not c[0]} == {"cc.hip": (0, 1)}
    # the flat zero fills it replaced stay gone; these are not flat (common.h says why)
    zero = {m for p in SOURCES for m in re.findall(r"\b(\w*zero\w*_kernel)\s*\(", code(p))}
    assert zero == {"gemm_zero_kernel", "gemm_tt_zero_kernel", "zero2_kernel", "srf_zero_kernel"}, zero
