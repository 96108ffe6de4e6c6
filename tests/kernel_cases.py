"""Case builder for the tests that walk the frame kernel's build table (profiles/kernel_table.json): for every
instantiation wofdm_frames_kernel<N, K, LAY, INJECT, DUMP, VAR> a geometry and plan options that make the plan pick it, and
a restatement in Python of how the library picks (wofdm_pick_layout, wofdm_pick_layout_masked in csrc/wofdm_kernel.h and
configure() in csrc/wofdm_abi.hip).  The restatement is checked against the table and the header on the CPU
(test_kernel_cases.py); on the GPU the authority is the plan's own kernel_id() (test_gpu_kernel_matrix.py,
test_gpu_parity.py)."""
import json
import os

import wofdm_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_TABLE = os.path.join(ROOT, "profiles", "kernel_table.json")
KERNEL_HEADER = os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc", "wofdm_kernel.h")

VAR_PLAIN, VAR_ALLOC, VAR_TXMASK, VAR_TXFFT = 0, 1, 2, 3
TXFFT_MAX_N, TXFFT_LEN = 256, 1024          # WOFDM_TXFFT_MAX_N, WOFDM_TXFFT_LEN

#: (n_fft, layout, var) that no geometry and no option can select, each with the line of configure() that proves it.
#: Dead code to be reported, not skipped silently.  Expected to be empty.
UNREACHABLE = ()


def table_rows():
    with open(KERNEL_TABLE) as f:
        return json.load(f)["kernels"]


def _rows(dump):
    return [(r["n_fft"], r["k"], r["layout"], r["inject"], r["var"]) for r in table_rows() if r["dump"] == dump]


def production_rows():
    """(n_fft, k, layout, inject, var) of every production kernel of the build table."""
    return _rows(0)


def dump_rows():
    """(n_fft, k, layout, inject, var) of every instrumented (stage-dumping) kernel of the build table."""
    return _rows(1)


def spilling_rows():
    """The production kernels the compiler gave a non-zero ScratchSize."""
    return [(r["n_fft"], r["k"], r["layout"], r["inject"], r["var"]) for r in table_rows()
            if not r["dump"] and r["private_segment_fixed_size"] > 0]


def row_id(row):
    return "N%d-k%d-L%d-%s-v%d" % (row[0], row[1], row[2], "inj" if row[3] else "gen", row[4])


def noise_before_truncate(row):
    """The noise order a row's case runs (cfg.noise_before_truncate, a run-time flag of every kernel): chosen from (k, inject) so
    that every (n_fft, layout, var) sees both orders in generate and in injected mode across its three k -- the table lists
    generate and injected kernels alternately, so the parity of the row index would tie the order to the mode."""
    n_fft, k, layout, inject, var = row
    return (k // 2 + inject) % 2 == 0


# ------------------------------------------------------------------------------------------------------------------
# geometry that selects a row
def geometry_for(n_fft, layout, var):
    """(system, cp, S, plan options) that make the plan pick `layout` for variant `var` (0 plain, 1 with a subcarrier
    allocation, 2 / 3 with a Tx mask in direct / fast-convolution form)."""
    env = {}
    if var == VAR_TXMASK and n_fft <= TXFFT_MAX_N:
        env["txmask_direct"] = 1                                                  # (else the mask runs as fast convolution)
    if layout == 1:
        if n_fft >= 512:
            env["fir_valu"] = 1
            return "WOLA", 32, 16, env
        if var >= 2 or n_fft <= 128:
            env["fir_valu"] = 1                                                   # (else the masked variants run layout 9, N <= 128 layout 16)
        return ("wtx", 32 if n_fft == 256 else 16, 16 if var >= 2 else 9, env)   # a mask forces one symbol per wave
    if layout in (9, 15):                                                         # Tx mask + matrix-pipe FIR: strides 4 | B, B >= N
        if layout == 9 and n_fft == 256 and var == 3:
            env["dft_valu"] = 1                                                   # (else the fast-convolution mask runs layout 15)
        return ("wtx" if n_fft >= 256 else "WOLA"), 32 if n_fft >= 256 else 16, 16, env
    if layout == 2:
        env.update(fir_valu=1, max_spw=2)
        return "wtx", 32 if n_fft == 256 else 16, 16, env
    if layout in (4, 5):
        env["fir_valu"] = 1
        return ("wtx" if layout == 4 else "CPW"), 32, 16, env        # strides 288 / 293
    if layout in (6, 7, 10, 11):
        if layout in (6, 7):
            env["dft_valu"] = 1
        return "wtx", (32 if layout in (6, 10) else 48), 16, env        # strides 288 / 304
    if layout == 13:
        return "wtx", 16, 16, env                                       # strides 80 / 144: sixteen / eight symbols within ten tiles
    if layout == 14:
        return "wtx", (20 if n_fft == 64 else 40), 16, env              # strides 84 / 168: between the tenth and the eleventh tile
    if layout == 16:
        if var == VAR_PLAIN:
            # full waves at a stride layouts 13 / 14 do not take: 96 (two waves of eight), 189 (three waves: 6 + 6 + 4)
            return ("wtx", 32, 16, env) if n_fft == 64 else ("wrx", 56, 16, env)
        # a frame that is no multiple of the wave: one wave with nine of its ten slots filled (stride 80), two waves of
        # six and three symbols (stride 160) -- the allocation variant's code for the unfilled slots
        return ("wtx", 16, 9, env) if n_fft == 64 else ("WOLA", 32, 9, env)
    assert layout in (8, 12), layout
    if layout == 8:
        env["dft_valu"] = 1
    return "WOLA", 32, 16, env


# ------------------------------------------------------------------------------------------------------------------
# the library's choice, restated
def fir8_tiles(n_fft):
    return 9 if n_fft >= 1024 else (5 if n_fft >= 512 else 3)


def layout_info(layout, n_fft):
    """spw, nt, rb, n_min, n_max and the variants of wofdm_layout_info(layout, n_fft); None for an id without a layout."""
    f8, sm, q = fir8_tiles(n_fft), 1024 // n_fft, n_fft // 64
    PA, MASKS = (0, 1), (2, 3)
    info = {
        1: (1, 0, q + 1, 64, 1024, PA + MASKS), 2: (2, 0, 2 * q + 2, 64, 256, PA),
        4: (4, 0, 4 * q + 2, 256, 256, PA), 5: (4, 0, 20, 256, 256, PA),
        6: (4, 9, 18, 256, 256, PA), 7: (4, 10, 20, 256, 256, PA),
        8: (1, f8, 2 * f8, 512, 1024, PA), 9: (1, f8, 2 * f8, 64, 1024, MASKS),
        10: (4, 9, 18, 256, 256, PA), 11: (4, 10, 20, 256, 256, PA),
        12: (1, f8, 2 * f8, 512, 1024, PA),
        13: (sm, 10, 20, 64, 128, PA), 14: (sm, 11, 22, 64, 128, PA),
        15: (1, f8, 2 * f8, 256, 256, (3,)), 16: (sm, 10, 20, 64, 128, PA),
    }.get(layout)
    if info is None:
        return None
    return dict(zip(("spw", "nt", "rb", "n_min", "n_max", "vars"), info))


def small_spwr(n_fft, S, B):
    """wofdm_small_spwr: the symbols a wave of layout 16 takes, 0 if the frame does not fit."""
    for waves in range(1, 5):
        spwr = (-(-S // waves) + 1) & ~1
        if spwr <= 1024 // n_fft and spwr * B <= 128 * 10 and (waves - 1) * spwr < S:
            return spwr
    return 0


def pick_layout(n_fft, S, B, plain=False, firm=True, mdft=True):
    """wofdm_pick_layout."""
    firm = firm and B >= n_fft
    if plain and mdft and firm and n_fft <= 128:
        if S % (1024 // n_fft) == 0:
            for lay in (13, 14):
                if (1024 // n_fft) * B <= 128 * layout_info(lay, n_fft)["nt"]:
                    return lay
        if small_spwr(n_fft, S, B) > 0:
            return 16
    if plain and n_fft == 256 and S % 4 == 0:
        if firm and 4 * B <= 128 * layout_info(6, n_fft)["nt"]:
            return 10 if mdft else 6
        if firm and 4 * B <= 128 * layout_info(7, n_fft)["nt"]:
            return 11 if mdft else 7
        if 4 * B <= 64 * layout_info(4, n_fft)["rb"]:
            return 4
        if 4 * B <= 64 * layout_info(5, n_fft)["rb"]:
            return 5
    if firm and plain and n_fft >= 512 and (B % 2 == 0 or mdft) and B <= 128 * fir8_tiles(n_fft):
        return 12 if mdft else 8
    return 2 if (n_fft <= 256 and S % 2 == 0 and 2 * B <= 64 * layout_info(2, n_fft)["rb"]) else 1


def pick_layout_masked(n_fft, B, firm):
    """wofdm_pick_layout_masked."""
    return 9 if (firm and n_fft <= B <= 128 * fir8_tiles(n_fft)) else 1


def lds_bytes(n_fft, layout, S, B, beta):
    """wofdm_lds_bytes for the layouts with one symbol per wave and no Tx mask (1, 8, 12)."""
    assert layout in (1, 8, 12)
    tw = 6 * 64 * 16 if n_fft in (256, 512) else 8 * n_fft
    cpcs = 64 if n_fft >= 1024 else 128
    fixed = tw + 8 * n_fft + 4 * 64 + 4 * 64 + 4 * (n_fft + cpcs) + 4 * (n_fft + 64) + 8 * 64
    if layout == 1:
        fbuf = (20 + beta + S * B + 20 + layout_info(1, n_fft)["rb"] + 8 + 1) // 2 * 2
    else:
        fbuf = (8 + 2 * S * ((B + 3) & ~3) + 2 * 48) // 2          # rows of whole 16-byte operand rows
    return fixed + 8 * fbuf + 8 * S * beta


LDS_MAX = 160 * 1024


def expected_kernel_id(st, S, options=None, var=VAR_PLAIN):
    """(layout, variant) configure() settles on for structure `st` with S symbols per frame, the plan options `options`
    and -- `var` -- nothing set (0), a subcarrier allocation (1) or a Tx mask (2, 3: which of its two forms runs is the
    library's choice, from the symbol length and the option txmask_direct)."""
    opt = dict(options or {})
    n_fft, B, P = st.n_fft, st.stride, st.sym_len
    if var >= 2:
        fft_ok = n_fft <= TXFFT_MAX_N and 3 * P - 2 <= TXFFT_LEN and not opt.get("txmask_direct")
        var = VAR_TXFFT if fft_ok else VAR_TXMASK
    firm, mdft = not opt.get("fir_valu"), not opt.get("dft_valu")
    if var >= 2:
        layout = pick_layout_masked(n_fft, B, firm)
    else:
        layout = pick_layout(n_fft, S, B, True, firm, mdft)
    if var == VAR_TXFFT and n_fft == 256 and layout == 9 and mdft:
        layout = 15
    cap = opt.get("max_spw", 0)
    if cap > 0 and layout_info(layout, n_fft)["spw"] > cap:
        layout = 1 if cap == 1 else pick_layout(n_fft, S, B, False)
    if layout in (8, 12) and lds_bytes(n_fft, layout, S, B, st.tail_tx) > LDS_MAX >= lds_bytes(n_fft, 1, S, B, st.tail_tx):
        layout = 1                               # (the padded rows of layouts 8 / 12 do not fit the LDS, the frame as on air does)
    return layout, var


def expected_id_of(n_fft, layout, var):
    """expected_kernel_id of the geometry geometry_for hands out for a row."""
    system, cp, S, options = geometry_for(n_fft, layout, var)
    return expected_kernel_id(W.make_structure(system, n_fft, cp), S, options, var)
