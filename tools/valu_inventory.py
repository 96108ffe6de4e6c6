#!/usr/bin/env python3
"""Developer tool (no GPU): the vector instructions of the pinned frame kernels that are NOT arithmetic, split, MFMA, RNG or demapper.

    python tools/valu_inventory.py [libwofdm_hip.so] [label]      # the built library's disassembly, per kernel
    python tools/valu_inventory.py --marks [label]                # hipcc -S -DWOFDM_MMARK of the built-geometry unit N = 256, k = 4:
                                                                  # the same per segment of the frame loop

What tests/test_arith_multiset.py freezes (the classes of arith_multiset.CLASSES), the Philox rounds (v_mad_u64_u32, v_bitop3_b32),
the Box-Muller transform (v_log_f32, v_sqrt_f32, v_cos_f32, v_sin_f32, v_alignbit_b32, v_cvt_f32_u32) and the demapper's own
instructions (v_min_f32, v_cvt_pk_u8_f32, v_bcnt_u32_b32) are at the floor of their definitions.  The rest -- "other" -- is lane
bookkeeping, selects, moves and address arithmetic: the part of the vector pipe's instruction stream that can still shrink.  Counts are
static (an instruction inside an inner loop counts once).  profiles/int_bookkeeping.txt holds the table of the parent build
(tests/test_valu_inventory.py compares the built library with it)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arith_multiset as AM  # noqa: E402

V = AM.V
KERNELS = AM.KERNELS
#: vector instructions that are not "other": the frozen classes, the RNG, the demapper
FIXED = [pat for c, pat in AM.CLASSES if c != "valu"] + [
    r"v_mad_u64_u32", r"v_bitop3_b32", r"v_(log|sqrt|cos|sin)_f32", r"v_alignbit_b32", r"v_cvt_f32_u32",
    r"v_min_f32", r"v_cvt_pk_u8_f32", r"v_bcnt_u32_b32"]
#: integer multiplies (quarter rate) that an index held in a lane constant does not need
LANE_MULS = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mul_i32_i24", "v_mul_u32_u24", "v_mul_hi_i32", "v_mul_hi_u32_u24", "v_mul_hi_i32_i24")


def is_other(op):
    return op.startswith("v_") and not any(re.match(p, op) for p in FIXED)


def tally(ops):
    """{"other": {mnemonic: n}, "other_total": n, "valu": n} of a list of mnemonics"""
    other = {}
    for op in ops:
        if is_other(op):
            # (an encoding suffix is not another instruction)
            m = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
            other[m] = other.get(m, 0) + 1
    return {"other": other, "other_total": sum(other.values()), "valu": sum(op.startswith("v_") for op in ops)}


def kernel_ops(lib, tags=None):
    """{kernel label: [(mnemonic, instruction text)]} of the kernels of KERNELS in a built library"""
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
                            cur = out.setdefault(label, [])
                    continue
                if cur is None or "//" not in line:
                    continue
                ins = line.split("//")[0].strip()
                if ins:
                    cur.append((ins.split()[0], ins))
    return out


def count(lib, tags=None):
    return {k: tally([op for op, _ in v]) for k, v in kernel_ops(lib, tags).items()}


def lane_multiplies(lib, tags=None):
    """{kernel label: [instruction text]}: the integer multiplies with a VECTOR multiplicand and a constant or scalar multiplier --
    an index scaled per lane (a product of two vector registers is data, e.g. the demapper's)"""
    out = {}
    for k, v in kernel_ops(lib, tags).items():
        hits = []
        for op, ins in v:
            if re.sub(r"_(e32|e64)$", "", op) in LANE_MULS:
                srcs = [s.strip() for s in ins.split(None, 1)[1].split(",")[1:]]
                if sum(bool(re.match(r"v\d+$", s)) for s in srcs) == 1:
                    hits.append(ins)
        out[k] = hits
    return out


def rows(lib, label):
    for kern, c in sorted(count(lib).items()):
        yield "  %-8s %-32s other %4d  vector %4d" % (label, kern, c["other_total"], c["valu"])


def detail(lib, label):
    for kern, c in sorted(count(lib).items()):
        yield "  %-8s %-32s %s" % (label, kern, " ".join("%s %d" % (m, n) for m, n in sorted(c["other"].items(), key=lambda x: (-x[1], x[0]))))


def parse(text, label):
    """{kernel label: {"other": n, "valu": n}} of the rows `label` of a table printed by rows()"""
    out = {}
    for m in re.finditer(r"^\s+%s\s+(\S+ <[^>]+>)\s+other\s+(\d+)\s+vector\s+(\d+)\s*$" % re.escape(label), text, re.M):
        out[m.group(1)] = {"other": int(m.group(2)), "valu": int(m.group(3))}
    return out


def marks(label, n="256", k="4"):
    """the frame loop of the two pinned kernels, split at the `; wofdm_mark` / `; wofdm_mmark` comments of a -S build of the
    built-geometry unit"""
    import isa_mix as IM
    lines = IM.compile_tu(n, k, ["-DWOFDM_TU_GEO", "-DWOFDM_MMARK"])
    for kern, tag in sorted(KERNELS.items()):
        for _, name, body, meta in IM.kernels(lines):
            if tag not in name:
                continue
            ops, labels = IM.body_ops(body)
            fl = IM.frame_loop(ops, labels)
            yield "  %-8s %-32s vgpr %d scratch %d" % (label, kern, meta.get("vgpr_count", -1), meta.get("private_segment_fixed_size", -1))
            cuts = [(i, re.search(r"wofdm_m?mark\s+(\d+)", l).group(0).replace("wofdm_", "")) for i, l in enumerate(body)
                    if re.search(r"wofdm_m?mark\s+\d+", l) and fl[0] <= i <= fl[1]]
            prev, pname, total = fl[0], "loop head", {"other_total": 0, "valu": 0}
            for i, t in cuts + [(fl[1], None)]:
                c = tally([op for j, op, _ in ops if prev <= j <= i])
                total["other_total"] += c["other_total"]
                total["valu"] += c["valu"]
                top = " ".join("%s %d" % (m, x) for m, x in sorted(c["other"].items(), key=lambda x: (-x[1], x[0]))[:8])
                yield "  %-8s   .. %-10s other %4d  vector %4d | %s" % (label, pname, c["other_total"], c["valu"], top)
                prev, pname = i + 1, t
            yield "  %-8s   .. %-10s other %4d  vector %4d" % (label, "frame loop", total["other_total"], total["valu"])


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--marks"]
    if "--marks" in sys.argv[1:]:
        for r in marks(args[0] if args else "built"):
            print(r)
        sys.exit(0)
    lib = args[0] if args else os.path.join(ROOT, "w-ofdm-optimization_amd", "libwofdm_hip.so")
    label = args[1] if len(args) > 1 else "built"
    for r in rows(lib, label):
        print(r)
    for r in detail(lib, label):
        print(r)
    for kern, hits in sorted(lane_multiplies(lib).items()):
        print("  %-8s %-32s integer multiplies of a lane index: %d%s" % (label, kern, len(hits), "".join("\n      " + h for h in hits)))
