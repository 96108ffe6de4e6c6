#!/usr/bin/env python3
"""Developer tool (build container): registers / spills / scratch of EVERY instantiation of the frame kernel, read
from the metadata notes of the BUILT library (what ships, per-translation-unit compiler flags included).

    python tools/kernel_table.py > profiles/kernel_table.json
    python tools/kernel_table.py --geo > profiles/kernel_table_geo.json

The first lists the 756 kernels that read their geometry at run time; --geo lists the kernels with a built geometry (wofdm_geo_table
in csrc/wofdm_kernel.h): id, structure, k, layout, VGPRs, SGPR spills, scratch, code bytes.  Such a kernel must have ScratchSize 0 and
at most 168 VGPRs (three workgroups per CU); otherwise its row is taken out of wofdm_geo_table (tests/test_geo_table.py).

tests/test_gpu_parity.py reads the committed table and runs the sharp-parity case for every production
(non-instrumented) instantiation whose ScratchSize is not zero; tests/test_code_layout.py checks that the table still
describes the built library."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNEL_HEADER = os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc", "wofdm_kernel.h")


def geo_structures():
    """Names of the rows of wofdm_geo_table in id order, from the "// <id> <name>" comment each row of the header carries."""
    text = open(KERNEL_HEADER).read()
    body = text[text.index("static constexpr wofdm_geo_row wofdm_geo_table[WOFDM_GEO_COUNT] = {"):]
    names = re.findall(r"\{[^{}]*\},\s*//\s*(\d+)\s+(\w+)", body[:body.index("};")])
    assert [int(i) for i, _ in names] == list(range(1, len(names) + 1)), names
    return tuple(n for _, n in names)


GEO_STRUCTURES = geo_structures()
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def table(lib, geo=False):
    """rows of the kernels with the geometry at run time (geo=False: profiles/kernel_table.json) or of those with a built geometry"""
    import test_code_layout as T0
    T = T0.V                                        # (the build's verifier: w-ofdm-optimization_amd/csrc/verify_code_layout.py)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in T.code_objects(lib, tmp):
            notes = subprocess.run([os.path.join(T.LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                t = name and re.search(r"wofdm_frames_kernelILi(\d+)ELi(\d)ELi(\d+)ELb(\d)ELb(\d)ELi(\d)E(?:Li(\d+)E)?", name.group(1))
                if not t:
                    continue
                gid = int(t.group(7) or 0)
                if (gid > 0) != geo:
                    continue
                row = dict(zip(("n_fft", "k", "layout", "inject", "dump", "var"), map(int, t.groups()[:6])))
                for f in FIELDS:
                    row[f] = int(re.search(r"\." + f + r":\s+(\d+)", blk).group(1))
                if geo:
                    sym = subprocess.run([os.path.join(T.LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True,
                                         check=True).stdout
                    size = [int(l.split()[2]) for l in sym.split("\n") if l.endswith(name.group(1)) and " FUNC " in l]
                    row = {"id": gid, "structure": GEO_STRUCTURES[gid - 1], "k": row["k"], "layout": row["layout"],
                           "vgpr_count": row["vgpr_count"], "sgpr_spill_count": row["sgpr_spill_count"],
                           "private_segment_fixed_size": row["private_segment_fixed_size"], "code_bytes": size[0]}
                rows.append(row)
    if geo:
        rows.sort(key=lambda r: (r["id"], r["k"]))
    else:
        rows.sort(key=lambda r: (r["n_fft"], r["k"], r["layout"], r["var"], r["inject"], r["dump"]))
    return rows


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--geo"]
    geo = "--geo" in sys.argv[1:]
    lib = args[0] if args else os.path.join(ROOT, "w-ofdm-optimization_amd", "libwofdm_hip.so")
    json.dump({"source": "metadata notes of libwofdm_hip.so (hipcc, ROCm 7.2, gfx950); tools/kernel_table.py" + (" --geo" if geo else ""),
               "kernels": table(lib, geo)}, sys.stdout, indent=0)
