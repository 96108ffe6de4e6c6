"""The case builder of the kernel-matrix tests (kernel_cases.py), checked on the CPU: every row of the build table
profiles/kernel_table.json has a geometry, the Python restatement of the library's choice picks the row's kernel for it,
and the table holds exactly what csrc/wofdm_kernel.h says is built."""
import ctypes
import os
import re

import pytest

import kernel_cases as KC
import wofdm_amd as W

NFFTS, KBITS = (64, 128, 256, 512, 1024), (2, 4, 6)
ALL_ROWS = sorted({(r["n_fft"], r["k"], r["layout"], r["inject"], r["dump"], r["var"]) for r in KC.table_rows()})


def test_table_is_the_full_product():
    rows = KC.table_rows()
    assert len(rows) == len(ALL_ROWS) == 756                       # no duplicate row
    assert len(KC.production_rows()) == len(KC.dump_rows()) == 378
    triples = {(n, lay, var) for n, k, lay, inj, dump, var in ALL_ROWS}
    assert len(triples) == 63
    # every (n_fft, layout, var) is built for every k, both modes, production and instrumented
    assert set(ALL_ROWS) == {(n, k, lay, inj, dump, var) for n, lay, var in triples for k in KBITS for inj in (0, 1)
                             for dump in (0, 1)}
    assert set(KC.spilling_rows()) <= set(KC.production_rows()) and len(KC.spilling_rows()) == 76


@pytest.mark.parametrize("row", ALL_ROWS, ids=lambda r: "N%d-k%d-L%d-i%d-d%d-v%d" % r)
def test_builder_reaches_every_row(row):
    n_fft, k, layout, inject, dump, var = row
    assert (n_fft, layout, var) not in KC.UNREACHABLE
    system, cp, S, options = KC.geometry_for(n_fft, layout, var)
    st = W.make_structure(system, n_fft, cp)
    assert 2 <= S <= 16 and set(options) <= set(W._lib.OPTIONS)
    assert KC.expected_kernel_id(st, S, options, var) == (layout, var)
    # (the geometry passes the plan's own limits: check_cfg in csrc/wofdm_abi.hip)
    assert st.cp + st.cs <= (64 if n_fft >= 1024 else 128) and st.tail_tx <= 16 and st.tail_rx <= 64
    assert st.stride <= 64 * KC.layout_info(1, n_fft)["rb"]


def test_unreachable_rows_are_not_produced():
    triples = {(n, lay, var) for n, k, lay, inj, dump, var in ALL_ROWS}
    assert set(KC.UNREACHABLE) <= triples
    reached = {KC.expected_id_of(*t) + (t[0],) for t in triples - set(KC.UNREACHABLE)}
    for n_fft, layout, var in KC.UNREACHABLE:
        assert (layout, var, n_fft) not in reached


def test_picker_predicts_only_built_kernels():
    """Over a grid of structures, frame lengths and option sets, the restated picker names nothing the table lacks, and
    reaches all of it."""
    triples = {(n, lay, var) for n, k, lay, inj, dump, var in ALL_ROWS}
    option_sets = [{}, {"fir_valu": 1}, {"dft_valu": 1}, {"fir_valu": 1, "max_spw": 2}, {"max_spw": 1}, {"max_spw": 2},
                   {"txmask_direct": 1}, {"txmask_direct": 1, "fir_valu": 1}, {"dft_valu": 1, "max_spw": 4}]
    seen = set()
    for n_fft in NFFTS:
        for system in W.SYSTEMS:
            for cp in (16, 20, 32, 40, 48, 56):
                st = W.make_structure(system, n_fft, cp)
                if st.cp + st.cs > (64 if n_fft >= 1024 else 128):
                    continue
                for S in (16, 9, 12, 7, 2):
                    for options in option_sets:
                        for var in (0, 1, 2):
                            if var >= 2 and n_fft > 512:
                                continue                       # the Tx mask needs n_fft <= 512: the plan refuses it
                            lay, v = KC.expected_kernel_id(st, S, options, var)
                            assert (n_fft, lay, v) in triples, (system, n_fft, cp, S, options, var, lay, v)
                            seen.add((n_fft, lay, v))
    assert seen == triples - set(KC.UNREACHABLE)


# ------------------------------------------------------------------------------------------------------------------
# the header, read as data
def _header_layouts():
    """{layout id: the fields of its `case` row of wofdm_layout_info, as C expressions}, and the header's #defines."""
    text = open(KC.KERNEL_HEADER).read()
    body = text[text.index("static constexpr wofdm_layout wofdm_layout_info"):]
    body = body[:body.index("return {};")]
    rows = {}
    for m in re.finditer(r"case\s+(\d+):\s*return\s*\{([^}]*)\};", body):
        rows[int(m.group(1))] = [f.strip() for f in m.group(2).split(",")]
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(WOFDM_\w+)\s+(\d+)\s", text)}
    return rows, defines


def _c_eval(expr, n_fft):
    env = {"n_fft": n_fft, "f8": KC.fir8_tiles(n_fft), "sm": 1024 // n_fft, "PA": 3, "MASKS": 12, "true": 1, "false": 0,
           "WOFDM_FIR_VALU": 0, "WOFDM_FIR_QUARTER": 1, "WOFDM_FIR_ONE": 2,
           "WOFDM_DFT_VALU": 0, "WOFDM_DFT_MDFT": 1, "WOFDM_DFT_BIG": 2, "WOFDM_DFT_SMALL": 3}
    assert re.fullmatch(r"[\w\s+*/()|-]+", expr), expr
    return eval(re.sub(r"(\d+)u\b", r"\1", expr).replace("/", "//"), {"__builtins__": {}}, env)   # noqa: S307


def test_table_matches_the_header():
    rows, defines = _header_layouts()
    assert len(rows) == 15 and max(rows) + 1 == defines["WOFDM_LAYOUT_COUNT"]
    fields = ("spw", "fir", "dft", "partial", "masked", "nt", "rb", "wg", "min_waves", "n_min", "n_max", "vars")
    built = set()
    for layout, exprs in rows.items():
        assert len(exprs) == len(fields), (layout, exprs)
        for n_fft in NFFTS:
            li = dict(zip(fields, (_c_eval(e, n_fft) for e in exprs)))
            mine = KC.layout_info(layout, n_fft)
            # the restatement in kernel_cases.py holds the same numbers as the header
            assert (mine["spw"], mine["nt"], mine["rb"], mine["n_min"], mine["n_max"]) == \
                   (li["spw"], li["nt"], li["rb"], li["n_min"], li["n_max"]), (layout, n_fft)
            assert sum(1 << v for v in mine["vars"]) == li["vars"], layout
            for var in range(4):                                       # wofdm_layout_built
                if (li["spw"] > 0 and li["n_min"] <= n_fft <= li["n_max"] and (li["vars"] >> var) & 1
                        and (var != 2 or n_fft <= defines["WOFDM_TXMASK_MAX_N"])
                        and (var != 3 or n_fft <= defines["WOFDM_TXFFT_MAX_N"])):
                    built.add((n_fft, layout, var))
    assert KC.layout_info(0, 256) is None and KC.layout_info(3, 256) is None
    assert (defines["WOFDM_TXFFT_MAX_N"], defines["WOFDM_TXFFT_LEN"]) == (KC.TXFFT_MAX_N, KC.TXFFT_LEN)
    assert built == {(n, lay, var) for n, k, lay, inj, dump, var in ALL_ROWS}


def test_spilling_rows_keep_their_geometry():
    """The geometries of the rows test_every_spilling_production_kernel walks, as that test had them before the builder
    covered the whole table."""
    want = {(64, 1, 3): ("wtx", 16, 16, {"fir_valu": 1}), (64, 9, 3): ("WOLA", 16, 16, {}),
            (256, 4, 0): ("wtx", 32, 16, {"fir_valu": 1}), (256, 5, 1): ("CPW", 32, 16, {"fir_valu": 1}),
            (256, 6, 0): ("wtx", 32, 16, {"dft_valu": 1}), (256, 7, 1): ("wtx", 48, 16, {"dft_valu": 1}),
            (256, 9, 3): ("wtx", 32, 16, {"dft_valu": 1}), (256, 15, 3): ("wtx", 32, 16, {}),
            (1024, 8, 0): ("WOLA", 32, 16, {"dft_valu": 1}), (1024, 12, 1): ("WOLA", 32, 16, {})}
    for triple, geo in want.items():
        assert KC.geometry_for(*triple) == geo
    assert {(n, lay, var) for n, k, lay, inj, var in KC.spilling_rows()} >= set(want)


def test_both_noise_orders_in_both_modes():
    """Every (n_fft, layout, var) runs noise_before_truncate = 0 and 1 in generate mode and in injected mode, production
    and instrumented."""
    for rows in (KC.production_rows(), KC.dump_rows()):
        seen = {}
        for row in rows:
            n_fft, k, layout, inject, var = row
            seen.setdefault((n_fft, layout, var, inject), set()).add(bool(KC.noise_before_truncate(row)))
        assert len(seen) == 2 * 63 and all(orders == {False, True} for orders in seen.values())


# ------------------------------------------------------------------------------------------------------------------
# the header, compiled: tests/native/layout_shim.hip exports its pickers and sizing functions (built by make -C tests/native)
def _shim():
    path = os.path.join(KC.ROOT, "tests", "native", "libwofdm_layout_shim.so")
    assert os.path.exists(path), "%s not built (make -C tests/native)" % path
    lib = ctypes.CDLL(path)
    lib.shim_lds_bytes.restype = ctypes.c_uint
    return lib


def test_restated_pickers_and_sizes_match_the_header():
    lib = _shim()
    for n_fft in NFFTS:
        for S in range(2, 17):
            for B in range(n_fft - 8, n_fft + 65):              # (strides below n_fft: the matrix-pipe layouts refuse them)
                assert KC.small_spwr(n_fft, S, B) == lib.shim_small_spwr(n_fft, S, B), (n_fft, S, B)
                for plain in (0, 1):
                    for firm in (0, 1):
                        for mdft in (0, 1):
                            assert KC.pick_layout(n_fft, S, B, bool(plain), bool(firm), bool(mdft)) == \
                                   lib.shim_pick_layout(n_fft, S, B, plain, firm, mdft), (n_fft, S, B, plain, firm, mdft)
                for firm in (0, 1):
                    assert KC.pick_layout_masked(n_fft, B, bool(firm)) == lib.shim_pick_layout_masked(n_fft, B, firm)
                for beta in (0, 1, 8, 10, 16):
                    for layout in (1, 8, 12):
                        if layout == 1 or n_fft >= 512:
                            assert KC.lds_bytes(n_fft, layout, S, B, beta) == \
                                   lib.shim_lds_bytes(n_fft, beta + S * B, layout, S, B), (n_fft, layout, S, B, beta)
        for layout in range(17):
            for var in range(4):
                assert bool(lib.shim_layout_built(layout, n_fft, var)) == \
                       ((n_fft, layout, var) in {(n, lay, v) for n, k, lay, inj, dump, v in ALL_ROWS})
