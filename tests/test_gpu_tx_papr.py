"""``wofdm_tx_papr`` on the GPU (wofdm_papr_gen_kernel<N>, the waveform kernels of wofdm_tx_psd_batch[_masked] with one
job per frame, wofdm_papr_period_kernel) against the CPU oracle: ``oracle.frame`` on ``oracle.gen_labels`` of (seed,
cell = pair, frame), its ``tx`` dump cut into symbol periods (tests/papr_cases.py) -- never against the GPU path itself.

Bounds: energy within 1e-5 relative (the Parseval tolerance of test_gpu_tx_psd_*), peak within 2e-5 relative (PSD_RTOL
there), max_papr within 3e-5 relative.  Histogram: every row sums to frames * S exactly, and sum |hist_gpu - hist_ref| <=
2 near, near = periods whose fp64 PAPR lies within 2e-4 dB of a bin edge (a relative error of 3e-5 moves a value by
1.3e-4 dB), near <= 1 % of the periods by the choice of seed (papr_cases.pick_seed, an oracle-only property).

Measured on an MI355X, worst over the systems and variants of each N (energy / peak / max_papr, relative): N = 64:
3.4e-7 / 5.6e-7 / 3.2e-7; 128: 4.2e-7 / 6.7e-7 / 4.3e-7; 256: 3.8e-7 / 6.1e-7 / 2.6e-7; 512: 4.0e-7 / 7.5e-7 / 2.9e-7;
1024: 4.0e-7 / 6.4e-7 / 1.5e-7; every histogram equal to the oracle's (profiles/tx_papr.txt)."""
import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import timefreq as T

import papr_cases as PC

pytestmark = pytest.mark.gpu

E_RTOL, PK_RTOL, MAX_RTOL = 1e-5, 2e-5, 3e-5


def rel(got, want):
    return float((np.abs(np.asarray(got, np.float64) - want) / want).max())


def check_periods(got, want, tag):
    e, pk = rel(got[..., 1], want[..., 1]), rel(got[..., 0], want[..., 0])
    print("%s: energy %.2e, peak %.2e (relative, worst period)" % (tag, e, pk))
    assert e < E_RTOL, (tag, e)
    assert pk < PK_RTOL, (tag, pk)
    return e, pk


def check_max(max_papr, want_periods, B, tag):
    want = (B * want_periods[..., 0] / want_periods[..., 1]).reshape(want_periods.shape[0], -1).max(axis=1)
    m = rel(max_papr, want)
    print("%s: max_papr %.2e relative" % (tag, m))
    assert m < MAX_RTOL, (tag, m)


@pytest.mark.parametrize("variant", PC.VARIANTS)
@pytest.mark.parametrize("system", PC.SYSTEMS)
@pytest.mark.parametrize("n_fft", PC.NS)
def test_periods_histogram_and_maximum_against_the_oracle(n_fft, system, variant):
    r = PC.reference(n_fft, system, variant)
    st, S = r["st"], r["S"]
    B = st.sym_len - st.tail_tx
    tag = "N=%d %s %s S=%d k=%d B=%d" % (n_fft, system, variant, S, r["k"], B)
    hist, mx, per = T.tx_papr_gpu(st, r["k"], S, r["w"], r["seed"], 0, PC.FRAMES, active=r["active"], mask=r["mask"],
                                  lo_db=PC.LO_DB, step_db=PC.STEP_DB, n_bins=PC.N_BINS, periods=True)
    assert per.shape == r["periods"].shape
    check_periods(per, r["periods"], tag)
    diff = PC.check_hist(hist, r["periods"], B, r["near"])
    print("%s: histogram differs by %d counts (near %d of %d periods)" % (tag, diff, r["near"], per.size // 2))
    check_max(mx, r["periods"], B, tag)


def test_both_end_bins_take_what_lies_outside():
    """7 ... 9 dB in 8 bins: the oracle's periods of the case lie on both sides"""
    r = PC.reference(256, "wtx", "plain")
    st = r["st"]
    B = st.sym_len - st.tail_tx
    db = T.papr_db(r["periods"], B)
    assert (db < 7.0).any() and (db > 9.0).any()
    hist, _ = T.tx_papr_gpu(st, r["k"], r["S"], r["w"], r["seed"], 0, PC.FRAMES, lo_db=7.0, step_db=0.25, n_bins=8)
    near = PC.near_edges(r["periods"], B, 7.0, 0.25)
    PC.check_hist(hist, r["periods"], B, near, 7.0, 0.25, 8)
    assert hist[:, 0].sum() >= (db < 7.25).sum() - near and hist[:, -1].sum() >= (db >= 8.75).sum() - near


def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32"""
    st, k, S = PC.structure(128, "wtx"), 4, 9
    B = st.sym_len - st.tail_tx
    w = PC.random_windows(st, 2, 77)
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    want = PC.oracle_periods(st, k, S, w, None, None, seed, f0, 8)
    hist, mx, per = T.tx_papr_gpu(st, k, S, w, seed, f0, 8, lo_db=PC.LO_DB, step_db=PC.STEP_DB, n_bins=PC.N_BINS, periods=True)
    check_periods(per, want, "keys beyond 32 bits")
    check_max(mx, want, B, "keys beyond 32 bits")
    # the low words alone are another experiment
    low = PC.oracle_periods(st, k, S, w, None, None, seed & 0xFFFFFFFF, f0 & 0xFFFFFFFF, 2)
    assert rel(per[:, :2, :, 1], low[..., 1]) > 1e-3


def test_labels_are_keyed_by_cell_equal_pair():
    """pair 1 of a two-pair call = the oracle's cell 1 with window 1 (and not cell 0)"""
    r = PC.reference(256, "CPW", "half")
    st = r["st"]
    _, _, per = T.tx_papr_gpu(st, r["k"], r["S"], r["w"], r["seed"], 0, PC.FRAMES, active=r["active"], periods=True)
    check_periods(per[1:], r["periods"][1:], "pair 1 = cell 1")
    cell0 = PC.oracle_periods(st, r["k"], r["S"], r["w"][[1, 1]], r["active"], None, r["seed"], 0, 1, pairs=[0])
    assert rel(per[1:, :1, :, 1], cell0[..., 1]) > 1e-3


def test_split_frame_ranges_accumulate_to_one_call():
    r = PC.reference(256, "wtx", "half_masked")
    st = r["st"]
    kw = dict(active=r["active"], mask=r["mask"], lo_db=PC.LO_DB, step_db=PC.STEP_DB, n_bins=PC.N_BINS)
    one_h, one_m = T.tx_papr_gpu(st, r["k"], r["S"], r["w"], r["seed"], 0, 8, **kw)
    h, m = T.tx_papr_gpu(st, r["k"], r["S"], r["w"], r["seed"], 0, 5, **kw)
    first = h.copy()
    h2, m2 = T.tx_papr_gpu(st, r["k"], r["S"], r["w"], r["seed"], 5, 3, hist=h, max_papr=m, **kw)
    assert h2 is h and m2 is m and (h >= first).all() and h.sum() > first.sum()
    assert np.array_equal(h, one_h) and np.array_equal(m, one_m)
    PC.check_hist(one_h, r["periods"], st.sym_len - st.tail_tx, r["near"])


def test_repeated_calls_are_identical():
    r = PC.reference(512, "CPW", "masked")
    kw = dict(active=r["active"], mask=r["mask"], lo_db=PC.LO_DB, step_db=PC.STEP_DB, n_bins=PC.N_BINS, periods=True)
    a = T.tx_papr_gpu(r["st"], r["k"], r["S"], r["w"], r["seed"], 0, PC.FRAMES, **kw)
    b = T.tx_papr_gpu(r["st"], r["k"], r["S"], r["w"], r["seed"], 0, PC.FRAMES, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_chunks_at_n1024():
    """N = 1024, S = 16, one pair, unmasked: one full chunk of the documented budget and 37 frames of a second"""
    st, k, S = PC.structure(1024, "wtx"), 4, 16
    B = st.sym_len - st.tail_tx
    per_chunk = T.tx_papr_chunk_frames(st, S, False)
    assert per_chunk == min(65535, _lib.TX_PAPR_CHUNK_BYTES // (8 * (S * 1024 + st.tail_tx + S * B))) and 500 < per_chunk < 2000
    frames = per_chunk + 37
    w = PC.random_windows(st, 1, 9)
    seed, want, near = PC.pick_seed(lambda sd: PC.oracle_periods(st, k, S, w, None, None, sd, 0, frames), B, 40)
    hist, mx = T.tx_papr_gpu(st, k, S, w, seed, 0, frames, lo_db=PC.LO_DB, step_db=PC.STEP_DB, n_bins=PC.N_BINS)
    diff = PC.check_hist(hist, want, B, near)
    print("chunks: %d + 37 frames, histogram differs by %d counts (near %d of %d periods)" % (per_chunk, diff, near, frames * S))
    check_max(mx, want, B, "chunks")
    # the last frames alone, as a call of their own, see the same periods as the tail of the second chunk
    _, _, tail = T.tx_papr_gpu(st, k, S, w, seed, per_chunk - 2, 39, periods=True)
    check_periods(tail, want[:, per_chunk - 2:], "frames around the chunk boundary")


def test_agrees_with_the_frame_kernels_tx_stage(channels):
    """N = 256, one frame: the periods of wofdm_tx_papr and those of Plan.dump_frame(...)['tx'] of a plan with the same
    seed, allocation and mask -- two independently written device paths"""
    r = PC.reference(256, "wtx", "half_masked")
    st, k, S = r["st"], r["k"], r["S"]
    B = st.sym_len - st.tail_tx
    cfg = W.make_cfg(st, k, S, 21, 1, 1, PC.PAIRS, seed=r["seed"])
    w_rx = np.stack([W.rx_rc_window(st)] * PC.PAIRS)
    with W.Plan(cfg, r["w"], w_rx, channels[:1].astype(np.complex64), np.array([20.0], np.float32)) as plan:
        plan.set_allocation(r["active"])
        plan.set_tx_mask(r["mask"])
        for pair, frame in ((0, 0), (1, 3)):
            _, d = plan.dump_frame(pair, frame)
            want = PC.periods_of(d["tx"].astype(np.complex128), S, B)
            _, _, per = T.tx_papr_gpu(st, k, S, r["w"], r["seed"], frame, 1, active=r["active"], mask=r["mask"], periods=True)
            assert rel(per[pair, 0], want) < 2e-5, (pair, frame, rel(per[pair, 0], want))
            assert rel(per[pair, 0], r["periods"][pair, frame]) < 2e-5


def test_n1024_takes_a_mask_up_to_its_transform_length():
    """P = (8 N + 2) / 3 is served (masked, against the oracle: one frame of two symbols); one sample more is refused"""
    n, k, S = 1024, 2, 2
    pmax = (8 * n + 2) // 3
    st = PC.V.Structure("wrx", n, 1024, 0, 0, pmax - n - 1024, pmax - n, 0)         # (B = N + prefix_rm)
    assert st.sym_len == pmax and st.cs <= n
    w = np.linspace(0.5, 1.0, pmax).astype(np.float32)[None]
    mask = CM.tx_mask(pmax).astype(np.float32)
    want = PC.oracle_periods(st, k, S, w, None, mask, 5, 0, 1)
    _, _, per = T.tx_papr_gpu(st, k, S, w, 5, 0, 1, mask=mask, periods=True)
    check_periods(per, want, "N=1024 P=%d masked" % pmax)
    over = PC.V.Structure("wrx", n, 1024, 0, 0, pmax + 1 - n - 1024, pmax + 1 - n, 0)
    with pytest.raises(_lib.WofdmError) as ei:
        T.tx_papr_gpu(over, k, S, np.ones((1, pmax + 1), np.float32), 5, 0, 1, mask=np.ones(2 * pmax + 1, np.float32))
    assert ei.value.code == -2 and "3 P - 2 <= 8 n_fft" in str(ei.value)
    T.tx_papr_gpu(over, k, S, np.ones((1, pmax + 1), np.float32), 5, 0, 1)        # unmasked: no such limit
