"""The table of built geometries (wofdm_geo_table in csrc/wofdm_kernel.h): the geometries whose structure lengths are compile-time
constants of a second build of the plain generate-mode kernel (template parameter GEO of wofdm_frames_kernel).

The header is read as data, the way tests/test_kernel_cases.py reads its layout table: every row must be what make_structure and
make_cfg give for its structure, wofdm_cfg_geo_id (host code, no device) must find exactly these geometries, and
profiles/kernel_table_geo.json must list exactly the kernels the header builds, each within the limits a built geometry has to keep
(no scratch, at most 168 VGPRs = three workgroups per CU) -- a row whose kernel breaks them is taken out of the table, not excused."""
import ctypes as C
import json
import os
import re
import shutil

import pytest

import kernel_cases as KC
import wofdm_amd as W

ROOT = KC.ROOT
GEO_TABLE = os.path.join(ROOT, "profiles", "kernel_table_geo.json")
FIELDS = ("n_fft", "S", "mu", "rho", "beta", "delta", "gamma", "kappa", "L", "P", "B", "T", "NL")
N_FFT, CP, S, TAPS = 256, 32, 16, 21
KBITS = (2, 4, 6)


def header_rows():
    """[{field: value}] of wofdm_geo_table, in the header's order (id = index + 1)."""
    text = open(KC.KERNEL_HEADER).read()
    struct = re.search(r"struct wofdm_geo_row \{\s*int ([^;]+);", text).group(1)
    assert tuple(f.strip() for f in struct.split(",")) == FIELDS
    body = text[text.index("static constexpr wofdm_geo_row wofdm_geo_table[WOFDM_GEO_COUNT] = {"):]
    body = re.sub(r"//[^\n]*", "", body[body.index("{") + 1:body.index("};")])
    rows = [dict(zip(FIELDS, (int(v) for v in m.group(1).split(",")))) for m in re.finditer(r"\{([^{}]*)\}", body)]
    count = int(re.search(r"#define\s+WOFDM_GEO_COUNT\s+(\d+)", text).group(1))
    assert len(rows) == count and all(len(r) == len(FIELDS) for r in rows)
    return rows


def header_names():
    """The structure names of the rows in id order, from the "// <id> <name>" comment each row carries: the one place that names them
    (tools/kernel_table.py reads the same comments), so a row taken out of the table shifts the ids here and there together."""
    text = open(KC.KERNEL_HEADER).read()
    body = text[text.index("static constexpr wofdm_geo_row wofdm_geo_table[WOFDM_GEO_COUNT] = {"):]
    names = re.findall(r"\{[^{}]*\},\s*//\s*(\d+)\s+(\w+)", body[:body.index("};")])
    assert [int(i) for i, _ in names] == list(range(1, len(names) + 1)), names
    return tuple(n for _, n in names)


STRUCTURES = header_names()                                             # ids 1 ... len(STRUCTURES)


def _cfg(system, n_fft=N_FFT, cp=CP, syms=S, taps=TAPS, nbt=True, k=4):
    st = W.make_structure(system, n_fft, cp)
    return st, W.make_cfg(st, k, syms, taps, 8, 12, 1, noise_before_truncate=nbt)


def _geo_id(cfg):
    return W._lib.load().wofdm_cfg_geo_id(C.byref(cfg))


def test_rows_are_the_seven_structures_of_the_reference_experiment():
    rows = header_rows()
    assert len(rows) == len(STRUCTURES) and len(set(STRUCTURES)) == len(STRUCTURES) and set(STRUCTURES) <= set(W.SYSTEMS)
    for i, (system, row) in enumerate(zip(STRUCTURES, rows)):
        st, cfg = _cfg(system)
        want = dict(n_fft=st.n_fft, S=S, mu=st.cp, rho=st.cs, beta=st.tail_tx, delta=st.tail_rx, gamma=st.prefix_rm,
                    kappa=st.circ_shift, L=TAPS, P=st.sym_len, B=st.stride, T=st.frame_len(S),
                    NL=st.frame_len(S) + TAPS - 1)
        assert row == want, (system, row, want)
        assert W._lib.load().wofdm_noise_len(C.byref(cfg)) == row["NL"]
        for k in KBITS:                                            # the id does not depend on the constellation
            assert _geo_id(_cfg(system, k=k)[1]) == i + 1, (system, k)


@pytest.mark.parametrize("system", STRUCTURES)
def test_near_misses_have_no_id(system):
    assert _geo_id(_cfg(system)[1]) > 0
    assert _geo_id(_cfg(system, syms=12)[1]) == 0
    assert _geo_id(_cfg(system, cp=24)[1]) == 0
    assert _geo_id(_cfg(system, taps=20)[1]) == 0
    assert _geo_id(_cfg(system, nbt=False)[1]) == 0
    assert _geo_id(_cfg(system, n_fft=512)[1]) == 0
    # the per-launch sizes are no part of a geometry
    st = W.make_structure(system, N_FFT, CP)
    assert _geo_id(W.make_cfg(st, 4, S, TAPS, 1, 3, 2, frames_per_cell=7, seed=5)) == _geo_id(_cfg(system)[1])


def test_an_invalid_cfg_is_an_error_not_an_id():
    _, cfg = _cfg("wtx")
    cfg.n_fft = 100
    assert _geo_id(cfg) == -2


def test_committed_table_lists_exactly_the_kernels_the_header_builds():
    rows = header_rows()
    listed = json.load(open(GEO_TABLE))["kernels"]
    want = {}
    for i, (system, row) in enumerate(zip(STRUCTURES, rows)):
        layout, var = KC.expected_kernel_id(W.make_structure(system, row["n_fft"], row["mu"]), row["S"], {}, 0)
        assert layout in (10, 11) and var == 0
        for k in KBITS:
            want[(i + 1, k)] = (system, layout)
    assert sorted((r["id"], r["k"]) for r in listed) == sorted(want)
    for r in listed:
        assert (r["structure"], r["layout"]) == want[(r["id"], r["k"])], r
        assert r["private_segment_fixed_size"] == 0, r                  # ScratchSize 0
        assert r["vgpr_count"] <= 168, r                                # three four-wave workgroups per CU (512 / 3, in eights)
        assert r["sgpr_spill_count"] >= 0 and r["code_bytes"] > 0, r


LIB = os.path.join(ROOT, "w-ofdm-optimization_amd", "libwofdm_hip.so")


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") and shutil.which("objcopy")),
                    reason="needs the built library and the ROCm LLVM tools")
def test_committed_table_describes_the_built_library():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    built = kernel_table.table(LIB, geo=True)
    listed = json.load(open(GEO_TABLE))["kernels"]
    key = lambda r: (r["id"], r["k"], r["structure"], r["layout"])   # noqa: E731
    assert sorted(map(key, built)) == sorted(map(key, listed))
    for r in built:
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_count"] <= 168, r
    # ... and the kernels that read their geometry at run time are not in it, nor these in the other table
    assert len(kernel_table.table(LIB)) == 756
