"""The vector instructions of the pinned frame kernels outside arithmetic, split, MFMA, RNG and demapper (no GPU).

tests/test_arith_multiset.py freezes the fp32 arithmetic, the f16 split and the MFMAs of the built-geometry C2 kernel
<256,4,10,false,false,0,1> and its layout-11 sibling; the Philox rounds, the Box-Muller transform and the demapper's own instructions
sit at the floor of their definitions.  What is left -- lane bookkeeping, address arithmetic, selects, moves: "other" in
tools/valu_inventory.py -- was cut in the kernels with a built geometry (profiles/int_bookkeeping.txt), and must not grow back: the
built library's "other" total and its total vector-instruction count stay strictly below the PARENT's rows recorded in that profile,
never below a figure of the build under test.  And no 32-bit or 24-bit signed integer multiply scales a lane index any more: the
lane offsets that needed one are lane constants made in the kernel's prologue."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import valu_inventory as VI  # noqa: E402

LIB = os.path.join(ROOT, "w-ofdm-optimization_amd", "libwofdm_hip.so")
PROFILE = os.path.join(ROOT, "profiles", "int_bookkeeping.txt")
#: the multiplies the cut removed (the parent's kernels held eight and six of them: profiles/int_bookkeeping.txt)
MULS = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mul_i32_i24")

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and VI.V.tools_present()), reason="needs the built library and the ROCm LLVM tools")


def test_the_profile_holds_the_parents_rows():
    want = VI.parse(open(PROFILE).read(), "parent")
    assert sorted(want) == sorted(VI.KERNELS)
    for kern, c in want.items():
        assert 300 < c["other"] < c["valu"] and c["valu"] > 1500, (kern, c)


@needs_tools
def test_built_kernels_hold_less_bookkeeping_than_the_parent():
    want = VI.parse(open(PROFILE).read(), "parent")
    got = VI.count(LIB)
    assert sorted(got) == sorted(VI.KERNELS)
    for kern in VI.KERNELS:
        print("%s: other %d (parent %d), vector %d (parent %d)" % (kern, got[kern]["other_total"], want[kern]["other"], got[kern]["valu"],
                                                                 want[kern]["valu"]))
        assert got[kern]["other_total"] < want[kern]["other"], (kern, got[kern]["other_total"], want[kern]["other"])
        assert got[kern]["valu"] < want[kern]["valu"], (kern, got[kern]["valu"], want[kern]["valu"])


@needs_tools
def test_no_integer_multiply_scales_a_lane_index():
    for kern, hits in VI.lane_multiplies(LIB).items():
        bad = [h for h in hits if re.sub(r"_(e32|e64)$", "", h.split()[0]) in MULS]
        print("%s: %s" % (kern, hits))
        assert not bad, (kern, bad)
