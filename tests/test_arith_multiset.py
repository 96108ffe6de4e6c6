"""The fp32 arithmetic of the benchmark's kernel, counted in the built library's disassembly (no GPU).

Whether complex fp32 arithmetic is issued packed (v_pk_fma_f32 = two IEEE fmas, v_pk_mul_f32 = two multiplies, v_pk_add_f32 = two adds)
or per component is a question of time only (profiles/packed_beside_mfma.txt); the results stay bit for bit where they were as long
as the operations stay the same.  So the built-geometry C2 kernel <256,4,10,false,false,0,1> and its layout-11 sibling hold the
multiset the parent build held -- fma-class, multiply and add instructions, a packed one counted twice -- whichever form a site has;
the table of the parent is the one recorded in that profile (tools/arith_multiset.py prints and parses it).  The MFMAs and the
instructions of the f16 split are pinned beside them: a conversion of packed arithmetic touches neither."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import arith_multiset as AM  # noqa: E402

LIB = os.path.join(ROOT, "w-ofdm-optimization_amd", "libwofdm_hip.so")
PROFILE = os.path.join(ROOT, "profiles", "packed_beside_mfma.txt")

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and AM.V.tools_present()), reason="needs the built library and the ROCm LLVM tools")


def test_the_profile_holds_the_parents_table():
    want = AM.parse(open(PROFILE).read(), "parent")
    assert sorted(want) == sorted(AM.KERNELS)
    for kern, c in want.items():
        assert c["fma-class"] > 200 and c["multiplies"] > 200 and c["adds"] >= 20 and c["mfma"] > 100, (kern, c)


@needs_tools
def test_built_kernels_hold_the_parents_arithmetic_multiset():
    want = AM.parse(open(PROFILE).read(), "parent")
    got = AM.count(LIB)
    assert sorted(got) == sorted(AM.KERNELS)
    for kern in AM.KERNELS:
        g, w = got[kern], want[kern]
        print("%s: %s (packed: fma %d, mul %d, add %d)" % (kern, {t: g[t] for t in AM.TOTALS}, g["pk_fma"], g["pk_mul"], g["pk_add"]))
        for t in AM.TOTALS + ("mfma", "mix", "cvt_pk_f16"):
            assert g[t] == w[t], (kern, t, g[t], w[t])
