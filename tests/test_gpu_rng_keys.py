"""The frame kernels on random-stream keys beyond 32 bits, and their counter flush after 2^14 frames.

csrc/philox.h keys the streams by (seed lo, seed hi) and counts by (block, frame lo, frame hi, stream << 28 | cell).  The rest
of the suite stays below 2^32 in seed and frame and below 2^16 in cell: with a zero frame-hi word the first Philox round
multiplies by zero, so a kernel that drops, swaps or truncates a high word passes there.  The frame kernel has three Philox
paths of its own (stream_block with laundered keys: data bits and make_noise; stream_block<false> with the keys hoisted per
phase; the rounds pipelined by hand between the MFMAs of the matrix-pipe FIR tile), so every generate-mode instantiation is
run here on a full 64-bit key against the oracle -- whose reading of the layout tests/test_rng_streams.py pins on the CPU.

The flush: `if (cell != cur_cell || nfr == (1u << 14))` in the frame loop keeps the 32-bit error sums of a long cell from
overflowing.  No other test gives a workgroup 2^14 frames of one cell.

Tolerances are those of tests/test_gpu_kernel_matrix.py / test_gpu_parity.py for the same comparisons: 12 bit errors per cell
at the production_case sizes, 2 per cell for runs of a few frames (_check_decisions), 1e-5 for unit_noise, labels and bit
totals exact."""
import ctypes as C
import time

import numpy as np
import pytest

import kernel_cases as KC
import test_gpu_kernel_matrix as KM
import wofdm_amd as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15                   # distinct, non-zero halves
OFF = 2 ** 32 - 2                           # every launch has frames on both sides of the carry into frame hi
SEED2 = 0xC3A5C85C97CB3127                  # bit 63 set
OFF2 = 0xFEDCBA9876543210                   # all 64 bits of the frame index busy

GEN_PRODUCTION = [r for r in KC.production_rows() if r[3] == 0]
GEN_DUMP = [r for r in KC.dump_rows() if r[3] == 0]


def _second_key_rows():
    """One generate-mode production row per (n_fft, layout) at variant 0, the k rotating."""
    groups = {}
    for r in GEN_PRODUCTION:
        if r[4] == 0:
            groups.setdefault((r[0], r[2]), []).append(r)
    return [sorted(rows)[i % len(rows)] for i, (_, rows) in enumerate(sorted(groups.items()))]


def test_the_cases_are_the_build_table():
    assert len(GEN_PRODUCTION) == 189 and len(GEN_DUMP) == 189
    second = _second_key_rows()
    assert len(second) == len({(r[0], r[2]) for r in GEN_PRODUCTION if r[4] == 0}) and {r[1] for r in second} == {2, 4, 6}
    assert OFF < 2 ** 32 < OFF + 4 and SEED >> 32 != SEED & 0xFFFFFFFF and SEED >> 32 and SEED2 >> 63 and OFF2 >> 32 != OFF2 & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------
# B1: every generate-mode production kernel
def _production_on_key(channels, row, seed, off):
    n_fft, k, layout, inject, var = row
    c = dict(KM.production_case(row), seed=seed, off=off)
    st, S, F = c["st"], c["S"], c["F"]
    assert F >= 4
    cfg = W.make_cfg(st, k, S, 21, 2, 3, 1, noise_before_truncate=c["matlab"], seed=seed)
    h = channels[11:13].astype(np.complex64)
    with W.Plan(cfg, c["w_tx"], c["w_rx"], h, c["snrs"]) as plan:
        KM._configure(plan, c["options"], c["active"], c["mask"], layout, var)
        got = plan.run(off, F)
    want = KM.oracle_counts(c, h)
    d = np.abs(got[..., 0].astype(np.int64) - want[..., 0].astype(np.int64))
    print("row %s seed %#x frames [%#x, +%d): max |bit errors - oracle| %d, fewest expected errors %d"
          % (KC.row_id(row), seed, off, F, d.max(), want[..., 0].min()))
    assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 3], want[..., 3])
    assert want[..., 0].min() > 2e2
    assert d.max() <= 12, (d, got[..., 0], want[..., 0])


@pytest.mark.parametrize("row", GEN_PRODUCTION, ids=KC.row_id)
def test_production_kernel_on_a_64_bit_key(channels, row):
    _production_on_key(channels, row, SEED, OFF)


@pytest.mark.parametrize("row", _second_key_rows(), ids=KC.row_id)
def test_production_kernel_on_a_key_with_every_bit_busy(channels, row):
    _production_on_key(channels, row, SEED2, OFF2)


# ------------------------------------------------------------------------------------------------------------------
# B2: the instrumented kernels' draws
@pytest.mark.parametrize("row", GEN_DUMP, ids=KC.row_id)
def test_dump_kernel_draws_on_a_64_bit_key(channels, row):
    n_fft, k, layout, inject, var = row
    system, cp, S, options = KC.geometry_for(n_fft, layout, var)
    st = W.make_structure(system, n_fft, cp)
    frame, cell = 2 ** 32 + 1, 5                                  # the plan's last cell: snr index 1, channel 2
    matlab = KC.noise_before_truncate(row)
    w_tx, w_rx = KM._test_windows(st, n_fft + cp + k)
    active, mask = KM._allocation_and_mask(st, k, layout, var)
    h = channels[4:7].astype(np.complex64)
    snrs = np.array([8.0, 22.0], dtype=np.float32)
    cfg = W.make_cfg(st, k, S, 21, 3, 2, 1, noise_before_truncate=matlab, seed=SEED)
    assert cell == cfg.n_cells - 1
    osys = KM._osys(st, k, S, matlab, active, mask)
    lab, noise = O.gen_labels(osys, SEED, cell, frame), O.gen_noise(osys, SEED, cell, frame)
    with W.Plan(cfg, w_tx, w_rx, h, snrs) as plan:
        KM._configure(plan, options, active, mask, layout, var)
        gc, gd = plan.dump_frame(cell, frame)
    nact = n_fft if active is None else int(active.sum())
    assert np.array_equal(gd["labels_tx"], lab)
    fig = KM._rel(gd["unit_noise"], noise)
    print("row %s: unit_noise %.3g" % (KC.row_id(row), fig))
    assert fig < 1e-5
    assert int(gc[1]) == (S - 1) * nact * k and int(gc[3]) == (S - 1) * nact
    # ... and the rest of the frame, stage by stage
    oc, od = O.frame(osys, w_tx.astype(np.float64), w_rx.astype(np.float64), h[2].astype(np.complex128), float(snrs[1]), lab,
                     noise, dump=True)
    KM._check_frame("row %s" % KC.row_id(row), gc, gd, oc, od, lab, noise, st, k, S, matlab, 0, active, w_tx, var >= 2)


# ------------------------------------------------------------------------------------------------------------------
# B3: a launch split at the carry
def test_frame_ranges_add_up_across_the_carry(channels):
    """test_frame_ranges_add_up_bit_exactly with the range around frame 2^32: frame_offset + fidx is a 64-bit sum in every
    workgroup, wherever the launch starts."""
    st = W.make_structure("wtx", 256, 32)
    w_tx, w_rx = W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32)
    snrs = np.linspace(-5, 50, 12).astype(np.float32)
    cfg = W.make_cfg(st, 4, 16, 21, 1, 12, 1, seed=SEED)
    lo = 2 ** 32 - 1500
    with W.Plan(cfg, w_tx, w_rx, channels[:1].astype(np.complex64), snrs) as plan:
        whole = plan.run(lo, 4000)
        at_carry = plan.run(lo, 1500) + plan.run(2 ** 32, 2500)
        first_off = plan.run(lo, 1) + plan.run(lo + 1, 3999)
        above = plan.run(2 ** 32, 2500)
        low_words = plan.run(0, 2500)
    assert np.array_equal(whole, at_carry)
    assert np.array_equal(whole, first_off)
    assert np.array_equal(whole[..., 1], np.full((1, 12, 1), 4000 * 15 * 256 * 4))
    # (frames 2^32 ... are other frames than 0 ...: their high word counts)
    assert np.array_equal(low_words[..., 1], above[..., 1]) and not np.array_equal(low_words[..., 0], above[..., 0])


# ------------------------------------------------------------------------------------------------------------------
# B4: more than 2^16 cells
def test_more_than_65536_cells(channels):
    """70 000 cells of one frame each: the cell index in the counter's fourth word, in the counter addresses and in the
    (pair, snr, channel) split, above 16 bits."""
    n_fft, k, S, n_ch, n_snr = 64, 2, 2, 100, 700
    frame = 2 ** 32 + 1
    st = W.make_structure("wtx", n_fft, 16)
    w_tx, w_rx = W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32)
    h = channels[:n_ch].astype(np.complex64)
    snrs = np.linspace(-2.0, 12.0, n_snr).astype(np.float32)
    cfg = W.make_cfg(st, k, S, 21, n_ch, n_snr, 1, seed=SEED)
    assert cfg.n_cells == 70000 > 2 ** 16
    osys = KM._osys(st, k, S, True)
    last = cfg.n_cells - 1
    with W.Plan(cfg, w_tx, w_rx, h, snrs) as plan:
        got = plan.run(frame, 1)
        gc, gd = plan.dump_frame(last, frame)
    want = O.run(osys, w_tx.astype(np.float64), w_rx.astype(np.float64), h.astype(np.complex128), snrs.astype(np.float64),
                 SEED, frame, 1)
    bits = (S - 1) * n_fft * k
    assert np.array_equal(got[..., 1], np.full((1, n_snr, n_ch), bits)) and np.array_equal(got[..., 1], want[..., 1])
    assert np.array_equal(got[..., 3], np.full((1, n_snr, n_ch), bits // k)) and np.array_equal(got[..., 3], want[..., 3])
    d = got[..., 0].astype(np.int64) - want[..., 0].astype(np.int64)
    print("70 000 cells: bit errors %d (oracle %d), cells that differ %d, max |difference| %d"
          % (got[..., 0].sum(), want[..., 0].sum(), int((d != 0).sum()), np.abs(d).max()))
    assert want[..., 0].sum() > 70000                             # (errors to compare: more than one per cell on average; BER 0.3 ... 0.04 over the SNR points)
    assert np.abs(d).max() <= 2, (np.argwhere(np.abs(d) > 2)[:10], d[np.abs(d) > 2][:10])
    assert abs(int(d.sum())) <= 2 * cfg.n_cells
    assert np.array_equal(gd["labels_tx"], O.gen_labels(osys, SEED, last, frame))
    assert KM._rel(gd["unit_noise"], O.gen_noise(osys, SEED, last, frame)) < 1e-5
    assert int(gc[1]) == bits and int(gc[3]) == bits // k


# ------------------------------------------------------------------------------------------------------------------
# B5: the flush after 2^14 frames
#: (n_fft, k, layout, variant, frame length): the per-lane sums (13, 10), the wave totals in scalar registers (12: N >= 512;
#: 15: the masked kernel with its transforms on the matrix pipe).  All of them refill their window tables per cell (matrix-pipe
#: transforms).
FLUSH_CASES = [(64, 2, 13, 0, 16), (256, 4, 10, 0, 16), (512, 4, 12, 0, 16), (256, 4, 15, 3, 16)]


@pytest.mark.parametrize("n_fft,k,layout,var,S", FLUSH_CASES, ids=lambda v: str(v))
def test_counter_flush_after_16384_frames(channels, n_fft, k, layout, var, S):
    """Every workgroup runs about 16 400 consecutive frames of a two-cell plan, so each meets the 2^14 flush inside a cell and
    the one that crosses the cell boundary both flushes; the same frames in five launches of about 4 100 frames per workgroup
    -- the regime the oracle comparisons cover -- must add up to the same counters, bit for bit."""
    system, cp, S0, options = KC.geometry_for(n_fft, layout, var)
    assert S0 == 16
    st = W.make_structure(system, n_fft, cp)
    w_tx, w_rx = W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32)
    active, mask = KM._allocation_and_mask(st, k, layout, var)
    assert active is not None or var == 0
    nact = n_fft if active is None else int(active.sum())
    snrs = np.array([5.0, 23.0], np.float32) + (k - 4) * 3.0       # BER near 0.3 and 0.02 (production_case's scale)
    cfg = W.make_cfg(st, k, S, 21, 1, 2, 1, seed=SEED)
    with W.Plan(cfg, w_tx, w_rx, channels[11:12].astype(np.complex64), snrs) as plan:
        KM._configure(plan, options, active, mask, layout, var)
        grid = plan.info()["workgroups"]                          # cus * occ: what launch() splits the items over
        F = grid * 8200 + 7
        assert grid > 0 and 2 * F // grid > 2 ** 14               # items per workgroup: beyond the flush threshold
        assert 2 * (F // 4) // grid < 2 ** 13                     # ... and the parts far below it
        t0 = time.perf_counter()
        whole = plan.run(0, F)
        seconds = time.perf_counter() - t0
        q = F // 4
        parts = sum(plan.run(i * q, min(q, F - i * q)) for i in range(5))
        again = plan.run(0, F)
    ber = whole[0, :, 0, 0] / whole[0, :, 0, 1]
    print("N %d layout %d: %d workgroups, %d frames per cell, %d items per workgroup, one launch %.3f s, BER %s"
          % (n_fft, layout, grid, F, 2 * F // grid, seconds, ber))
    assert 4 * q + 3 == F
    assert np.array_equal(whole, parts), (whole, parts)
    assert np.array_equal(whole[..., 1], np.full((1, 2, 1), F * (S - 1) * nact * k))
    assert np.array_equal(whole[..., 3], np.full((1, 2, 1), F * (S - 1) * nact))
    assert np.array_equal(whole, again)
    assert 0.5 > ber[0] > ber[1] > 0


# ------------------------------------------------------------------------------------------------------------------
def test_cell_limit_is_refused():
    """The cell index shares the counter's fourth word with the stream id: 2^28 cells or more are WOFDM_E_UNSUPPORTED
    (check_cfg), from the cfg alone."""
    lib = W._lib.load()
    st = W.make_structure("wtx", 64, 16)
    ok = W.make_cfg(st, 2, 2, 21, 3 * 5 * 29 * 43, 113 * 127, 1)
    assert ok.n_cells == 2 ** 28 - 1 and lib.wofdm_noise_len(C.byref(ok)) == st.tail_tx + 2 * st.stride + 20
    for n_ch, n_snr, pairs in ((2 ** 14, 2 ** 14, 1), (2 ** 10, 2 ** 10, 2 ** 8), (2 ** 15, 2 ** 15, 2 ** 2)):
        bad = W.make_cfg(st, 2, 2, 21, n_ch, n_snr, pairs)
        assert lib.wofdm_noise_len(C.byref(bad)) == -2
        assert b"2^28" in lib.wofdm_last_error()
        with pytest.raises(W._lib.WofdmError) as e:
            W._lib.check(lib.wofdm_noise_len(C.byref(bad)))
        assert e.value.code == -2
