#!/usr/bin/env python3
"""Developer tool (no GPU): the fp32 arithmetic multiset of frame kernels in a built library, from its disassembly.

    python tools/arith_multiset.py [libwofdm_hip.so] [label]

Per kernel: the fma-class instructions (v_fma_f32, v_fmac_f32, v_fmaak_f32, v_fmamk_f32), the multiplies (v_mul_f32) and the adds
(v_add_f32, v_sub_f32, v_subrev_f32), a packed instruction (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32) counted TWICE -- it is two IEEE
operations --, and beside them the packed and plain counts themselves, the MFMAs and the f16-split instructions.  Writing packed
arithmetic per component, or packing it, moves instructions between the packed and the plain columns and leaves the three totals
where they were; anything else changes the arithmetic.  profiles/packed_beside_mfma.txt holds the table of the parent build
(tests/test_arith_multiset.py compares the built library with it)."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc")
_spec = importlib.util.spec_from_file_location("verify_code_layout", os.path.join(CSRC, "verify_code_layout.py"))
V = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(V)

#: the benchmark's kernel (C2: N = 256, k = 4, layout 10, built geometry 1 = wtx) and its layout-11 sibling (built geometry 2 = wrx)
KERNELS = {"C2 <256,4,10,false,false,0,1>": "ILi256ELi4ELi10ELb0ELb0ELi0ELi1E",
           "L11 <256,4,11,false,false,0,2>": "ILi256ELi4ELi11ELb0ELb0ELi0ELi2E"}
CLASSES = [("pk_fma", r"v_pk_fma_f32"), ("pk_mul", r"v_pk_mul_f32"), ("pk_add", r"v_pk_add_f32"),
           ("fma", r"v_(fma|fmac|fmaak|fmamk)_f32"), ("mul", r"v_mul_f32"), ("add", r"v_(add|sub|subrev)_f32"),
           ("mfma", r"v_mfma_"), ("mix", r"v_fma_mix"), ("cvt_pk_f16", r"v_cvt_pk_f16_f32"), ("valu", r"v_")]
TOTALS = ("fma-class", "multiplies", "adds")


def count(lib, tags=None):
    """{kernel label: {class: count}} for the kernels of KERNELS (or `tags`: label -> mangled template arguments)"""
    tags = tags or KERNELS
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in V.code_objects(lib, tmp):
            dis = subprocess.run([os.path.join(V.LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    cur = None
                    for label, tag in tags.items():
                        if "wofdm_frames_kernel" + tag in m.group(1):
                            cur = out.setdefault(label, {c: 0 for c, _ in CLASSES})
                    continue
                if cur is None or "//" not in line:
                    continue
                op = line.split("//")[0].split()
                if not op:
                    continue
                for c, pat in CLASSES:
                    if re.match(pat, op[0]):
                        cur[c] += 1
    for c in out.values():
        c["fma-class"] = c["fma"] + 2 * c["pk_fma"]
        c["multiplies"] = c["mul"] + 2 * c["pk_mul"]
        c["adds"] = c["add"] + 2 * c["pk_add"]
    return out


def rows(lib, label):
    for kern, c in sorted(count(lib).items()):
        yield ("  %-8s %-32s fma-class %4d  multiplies %4d  adds %4d  | v_pk_fma %3d v_pk_mul %3d v_pk_add %2d | plain fma %3d mul %3d add %3d | "
               "MFMA %3d mix %3d cvt_pk_f16 %3d vector %4d" % (label, kern, c["fma-class"], c["multiplies"], c["adds"], c["pk_fma"], c["pk_mul"],
                                                            c["pk_add"], c["fma"], c["mul"], c["add"], c["mfma"], c["mix"], c["cvt_pk_f16"],
                                                            c["valu"]))


def parse(text, label):
    """{kernel label: {total: count}} of the rows `label` of a table printed by rows()"""
    out = {}
    for m in re.finditer(r"^\s+%s\s+(\S+ <[^>]+>)\s+fma-class\s+(\d+)\s+multiplies\s+(\d+)\s+adds\s+(\d+)\s+\|.*MFMA\s+(\d+) mix\s+(\d+) cvt_pk_f16\s+(\d+)"
                         % re.escape(label), text, re.M):
        out[m.group(1)] = {"fma-class": int(m.group(2)), "multiplies": int(m.group(3)), "adds": int(m.group(4)), "mfma": int(m.group(5)),
                           "mix": int(m.group(6)), "cvt_pk_f16": int(m.group(7))}
    return out


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "w-ofdm-optimization_amd", "libwofdm_hip.so")
    for r in rows(lib, sys.argv[2] if len(sys.argv) > 2 else "built"):
        print(r)
