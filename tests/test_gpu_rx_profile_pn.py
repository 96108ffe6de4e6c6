"""``wofdm_rx_profile_pn`` on the GPU (the Tx chain of wofdm_rx_profile once, wofdm_pn_walk_kernel, wofdm_rxprof_pn_kernel<N>,
wofdm_rxprof_sync_reduce_kernel<N>) against the fp64 host route ``rx_profile_pn_host``: the same frames, the same unit walks,
the same points, from the same Philox streams (the mirror itself is tied to ``frame_profile``, and through it to the CPU
oracle, in tests/test_rx_profile_pn_host.py).

Rules, per point: those of rx_profile_cases.check_profile with the mirror in the oracle's place -- per cell sum_n |sym_gpu -
sym_ref| <= near and sum_n |bit_gpu - bit_ref| <= k near, unloaded bins exactly 0, |err_power - ref| <= POW_TOL (ref[n] + mean_n
ref); the per-symbol counters under the same near bound per cell (sums over s), the per-symbol power under the same ratio rule
(over s).  The seed of a case is the first from its base seed on, of 32, for which the mirror alone has at most 1 % near
decisions at EVERY point (``RC.pick_seed``'s cap, decided on the CPU).  No case needed another SNR pair than ``RC.SNR_DB``'s.

The cases are the smallest shapes that still exercise every transform size, a partly filled and a multi-round wave loop, both
BINS extremes, the mask path and both noise orders; the geometry is RC.make_case's (2 pairs x 2 SNR points x 2 channels x 8
frames).

Measured on an MI355X: profiles/rx_profile_pn.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC

pytestmark = pytest.mark.gpu

#: name -> (n_fft, system, cp, k, S, variant, nbt)
CASES = {
    "n64_wtx_plain": (64, "wtx", 8, 2, 4, "plain", 1),
    "n128_wrx_half": (128, "wrx", 16, 2, 9, "half", 1),
    "n256_cpw_half_masked": (256, "CPW", 32, 6, 16, "half_masked", 1),
    "n512_wola_plain": (512, "WOLA", 64, 4, 3, "plain", 1),
    "n1024_wtx_half_masked": (1024, "wtx", 128, 4, 2, "half_masked", 1),
    "n128_cpw_half_nbt0": (128, "CPW", 32, 4, 4, "half", 0),
    "n64_cp_masked": (64, "CP", 16, 4, 5, "masked", 1),
}
#: (linewidth, cpe_tracked): the identity point; a narrow line, free-running and tracked; a 28 GHz-class one, tracked and
#: free-running; a wide tracked one; the widest allowed, free-running
POINTS = [R.PnPoint(0.0, 1), R.PnPoint(1e-3, 0), R.PnPoint(1e-3, 1), R.PnPoint(0.02, 1), R.PnPoint(0.02, 0), R.PnPoint(0.3, 1),
          R.PnPoint(1.0, 0)]


@functools.lru_cache(maxsize=None)
def case(name):
    n, system, cp, k, S, variant, nbt = CASES[name]
    c = RC.make_case(W.make_structure(system, n, cp), k, S, variant, 5000 + n + len(name), nbt)
    c["points"] = list(POINTS)
    return c


def host(c, seed, frame_offset, frames, points=None):
    """the mirror's profile and its near decisions [points, pairs, n_snr, n_ch]"""
    return R.rx_profile_pn_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                c["points"] if points is None else points, active=c["active"], mask=c["mask"],
                                noise_before_truncate=c["nbt"], with_near=True)


def decisions_of(c, frames):
    n_on = c["st"].n_fft if c["active"] is None else int(np.count_nonzero(c["active"]))
    return RC.PAIRS * RC.N_SNR * RC.N_CH * frames * (c["S"] - 1) * n_on


def pick_seed(c, base_seed, frame_offset=0, frames=RC.FRAMES, tries=32):
    """first seed from base_seed on whose MIRROR profile has at most 1 % near decisions at every point (RC.pick_seed's cap)"""
    for seed in range(base_seed, base_seed + tries):
        prof, near = host(c, seed, frame_offset, frames)
        if (near.sum(axis=(1, 2, 3)) <= 0.01 * decisions_of(c, frames)).all():
            return seed, prof, near
    raise AssertionError("no seed in [%d, %d) keeps the mirror's decisions clear of the thresholds" % (base_seed, base_seed + tries))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    seed, prof, near = pick_seed(c, 100 * (1 + list(CASES).index(name)))
    return c, seed, prof, near


def run_gpu(c, seed, frame_offset, frames, points=None, **kw):
    return W.rx_profile_pn_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                               c["points"] if points is None else points, active=c["active"], mask=c["mask"],
                               noise_before_truncate=c["nbt"], **kw)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    c, seed, _, _ = reference(name)
    return run_gpu(c, seed, 0, RC.FRAMES)


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_points(prof, ref, near, c, frames, tag):
    """the rules of the module docstring for every point; returns the largest err_power and per-symbol power ratio"""
    k, worst, worst_sym = c["k"], 0.0, 0.0
    assert len(c["points"]) == prof.bit_err.shape[0]
    for i, q in enumerate(c["points"]):
        rd = dict(bit=ref.bit_err[i].astype(np.int64), sym=ref.sym_err[i].astype(np.int64), pow=ref.err_power[i], near=near[i],
                  decisions=decisions_of(c, frames))
        ptag = "%s %s" % (tag, tuple(q))
        worst = max(worst, RC.check_profile(R.RxProfile(prof.bit_err[i], prof.sym_err[i], prof.err_power[i], prof.decisions), rd, c,
                                            ptag))
        ds = np.abs(prof.sym_err_sym[i].astype(np.int64) - ref.sym_err_sym[i].astype(np.int64)).sum(axis=-1)
        db = np.abs(prof.bit_err_sym[i].astype(np.int64) - ref.bit_err_sym[i].astype(np.int64)).sum(axis=-1)
        ratio = RC.pow_ratio(prof.err_power_sym[i], ref.err_power_sym[i])
        print("%s: per symbol: sym diff %d, bit diff %d, power ratio %.2e" % (ptag, ds.sum(), db.sum(), ratio))
        assert (ds <= near[i]).all() and (db <= k * near[i]).all(), (ptag, ds, db, near[i])
        assert ratio <= RC.POW_TOL, (ptag, ratio)
        worst_sym = max(worst_sym, ratio)
    # per point and cell the symbols add up to the bins, exactly
    assert np.array_equal(prof.bit_err_sym.sum(axis=-1), prof.bit_err.sum(axis=-1))
    assert np.array_equal(prof.sym_err_sym.sum(axis=-1), prof.sym_err.sum(axis=-1))
    print("%s: largest err_power ratio %.2e, per symbol %.2e" % (tag, worst, worst_sym))
    return worst, worst_sym


@pytest.mark.parametrize("name", list(CASES))
def test_profile_against_the_mirror(name):
    c, seed, ref, near = reference(name)
    prof = gpu_profile(name)
    st = c["st"]
    tag = "%s S=%d k=%d B=%d gamma=%d seed=%d" % (name, c["S"], c["k"], st.stride, st.prefix_rm, seed)
    print("%s: near shares per point %s" % (tag, np.round(near.sum(axis=(1, 2, 3)) / decisions_of(c, RC.FRAMES), 4)))
    check_points(prof, ref, near, c, RC.FRAMES, tag)
    on = np.ones(st.n_fft, bool) if c["active"] is None else c["active"]
    assert np.array_equal(prof.decisions, np.where(on, RC.FRAMES * (c["S"] - 1), 0))
    assert prof.bit_err.shape == (7, RC.PAIRS, RC.N_SNR, RC.N_CH, st.n_fft)
    assert prof.err_power_sym.shape == (7, RC.PAIRS, RC.N_SNR, RC.N_CH, c["S"] - 1)
    # the phase noise is on: every point of a positive linewidth differs from the linewidth-0 point, on every cell
    for i in range(1, 7):
        assert (np.abs(prof.err_power[i] - prof.err_power[0]).max(axis=-1) > 0).all(), i


@pytest.mark.parametrize("name", list(CASES))
def test_the_point_of_linewidth_0_is_the_plain_call(name):
    c, seed, _, _ = reference(name)
    prof = gpu_profile(name)
    plain = RC.run_gpu(c, seed, 0, RC.FRAMES)
    free = run_gpu(c, seed, 0, RC.FRAMES, points=[R.PnPoint(0.0, 0)])
    for got in (R.RxProfile(prof.bit_err[0], prof.sym_err[0], prof.err_power[0], prof.decisions),
                R.RxProfile(free.bit_err[0], free.sym_err[0], free.err_power[0], free.decisions)):
        for x, y in zip(got, plain):
            assert np.array_equal(x, y)
        assert np.ascontiguousarray(got.err_power).tobytes() == plain.err_power.tobytes()


@pytest.mark.parametrize("name", ("n64_wtx_plain", "n256_cpw_half_masked", "n1024_wtx_half_masked"))
def test_a_sweep_is_its_points_one_per_call(name):
    c, seed, _, _ = reference(name)
    prof = gpu_profile(name)
    for i, q in enumerate(c["points"]):
        one = run_gpu(c, seed, 0, RC.FRAMES, points=[q])
        assert same_bits(one[:6], [a[i:i + 1] for a in prof[:6]]), (name, q)
    # and in another order, beside other points
    other = run_gpu(c, seed, 0, RC.FRAMES, points=[c["points"][6], R.PnPoint(0.11, 0), c["points"][2]])
    assert same_bits([a[0] for a in other[:6]], [a[6] for a in prof[:6]])
    assert same_bits([a[2] for a in other[:6]], [a[2] for a in prof[:6]])


def test_repeated_calls_are_identical():
    for name in ("n512_wola_plain", "n64_cp_masked"):
        c, seed, _, _ = reference(name)
        assert same_bits(gpu_profile(name), run_gpu(c, seed, 0, RC.FRAMES))


def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked"
    c, seed, _, _ = reference(name)
    one = gpu_profile(name)
    a = run_gpu(c, seed, 0, 5)
    both = run_gpu(c, seed, 5, 3, out=a)
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert (both.bit_err >= a.bit_err).all() and both.bit_err.sum() > a.bit_err.sum()
    assert RC.pow_ratio(both.err_power, one.err_power) < 1e-12              # fp64 sums of the same fp32 frame sums
    assert RC.pow_ratio(both.err_power_sym, one.err_power_sym) < 1e-12


def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32"""
    c = case("n128_cpw_half_nbt0")
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    ref, near = host(c, seed, f0, 8)
    assert (near.sum(axis=(1, 2, 3)) <= 0.01 * decisions_of(c, 8)).all()
    prof = run_gpu(c, seed, f0, 8)
    check_points(prof, ref, near, c, 8, "keys beyond 32 bits")
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    assert not np.array_equal(run_gpu(c, seed & 0xFFFFFFFF, f0, 8).bit_err, prof.bit_err)
    high, low = run_gpu(c, seed, 2 ** 32, 5), run_gpu(c, seed, 0, 5)
    assert not np.array_equal(high.bit_err, low.bit_err) and not np.array_equal(high.err_power, low.err_power)
    assert np.array_equal(run_gpu(c, seed, f0, 3).bit_err + high.bit_err, prof.bit_err)


def test_pn_for_window_file_equals_its_host_route(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    pts = [(0.0, 0), (0.02, 1), (0.02, 0)]
    gpu = W.pn_for_window_file("wtx", 8, win, h, snr, pts, gpu=True, **kw)
    hst = W.pn_for_window_file("wtx", 8, win, h, snr, pts, gpu=False, **kw)
    assert list(gpu) == list(hst) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    plain = W.profile_for_window_file("wtx", 8, win, h, snr, gpu=True, **kw)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want, near = R.rx_profile_pn_host(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, active=alloc, mask=mask, with_near=True)
        for i, name in enumerate(("opt", "rc")):
            g, hh = gpu[name][key], hst[name][key]
            assert np.array_equal(hh.bit_err, want.bit_err[:, i]) and np.array_equal(hh.err_power, want.err_power[:, i])
            assert np.array_equal(hh.bit_err_sym, want.bit_err_sym[:, i])
            assert g.bit_err.shape == (3, 2, 2, 64) and g.err_power_sym.shape == (3, 2, 2, 3)
            assert np.array_equal(g.decisions, hh.decisions)
            ds = np.abs(g.sym_err.astype(np.int64) - hh.sym_err.astype(np.int64)).sum(axis=-1)
            db = np.abs(g.bit_err.astype(np.int64) - hh.bit_err.astype(np.int64)).sum(axis=-1)
            assert (ds <= near[:, i]).all() and (db <= 4 * near[:, i]).all(), (name, key, ds, db, near[:, i])
            assert (g.bit_err[..., ~alloc] == 0).all() and (g.err_power[..., ~alloc] == 0).all()
            for p in range(3):
                assert RC.pow_ratio(g.err_power[p], hh.err_power[p]) <= RC.POW_TOL
                assert RC.pow_ratio(g.err_power_sym[p], hh.err_power_sym[p]) <= RC.POW_TOL
            # the point of linewidth 0 is profile_for_window_file
            assert np.array_equal(g.bit_err[0], plain[name][key].bit_err)
            assert np.ascontiguousarray(g.err_power[0]).tobytes() == plain[name][key].err_power.tobytes()


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two points: a chunk of the documented budget ends inside a cell; neither the split of the
    frame range nor the other chunking of the plain call changes an integer counter"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    pts = [R.PnPoint(0.0, 1), R.PnPoint(0.01, 0)]
    c.update(active=CM.half_band_allocation(1024), points=pts)
    Tv = st.frame_len(S)
    per_chunk = R.rx_profile_pn_chunk_frames(st, S, False, 2)
    assert per_chunk == _lib.RX_PROFILE_CHUNK_BYTES // (8 * (S * 1024 + Tv) + 8 * S * st.stride + 8 * 2 * (1024 + S))
    assert 250 < per_chunk < R.rx_profile_sync_chunk_frames(st, S, False, 2)
    frames = per_chunk // 2 + 19                                            # 8 cells: four chunks and a bit
    one = run_gpu(c, 7000, 0, frames)
    assert int(one.decisions.max()) == frames * (S - 1)
    parts = run_gpu(c, 7000, frames - 7, 7, out=run_gpu(c, 7000, 0, frames - 7))
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym"):
        assert np.array_equal(getattr(parts, f), getattr(one, f)), f
    assert RC.pow_ratio(parts.err_power, one.err_power) < 1e-12
    assert RC.pow_ratio(parts.err_power_sym, one.err_power_sym) < 1e-12
    assert R.rx_profile_kernel_ms() > 0.0
    plain = RC.run_gpu(c, 7000, 0, frames)
    assert np.array_equal(one.bit_err[0], plain.bit_err) and np.array_equal(one.sym_err[0], plain.sym_err)
    assert RC.pow_ratio(one.err_power[0], plain.err_power) < 1e-12
    assert not np.array_equal(one.bit_err[1], plain.bit_err)
