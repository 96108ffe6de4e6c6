"""``wofdm_rx_profile_pa`` on the GPU (the Tx chain of wofdm_rx_profile once, wofdm_pa_wave_kernel, wofdm_rxprof_pa_kernel<N>,
wofdm_rxprof_sync_reduce_kernel<N>, wofdm_pa_power_reduce_kernel) against the fp64 host route ``rx_profile_pa_host``: the same
frames, the same amplifiers, from the same Philox streams (the mirror itself is tied to ``frame_profile`` in
tests/test_rx_profile_pa_host.py).

Rules, per point: those of tests/test_gpu_rx_profile_doppler.py's ``check_tracks`` with the points for its tracks -- per cell
sum_n |sym_gpu - sym_ref| <= near and sum_n |bit_gpu - bit_ref| <= k near, unloaded bins exactly 0, |err_power - ref| <= POW_TOL
(ref[n] + mean_n ref); the per-symbol counters under the same near bound per cell, the per-symbol power under the same ratio
rule; per point and cell the per-symbol counters add up to the per-bin counters exactly.  ``pa_power`` against the mirror by
the same ratio rule (over its two entries).  The seed of a case is the first from its base seed on, of 32, for which the mirror
alone has at most 1 % near decisions on EVERY point (decided on the CPU); cases, points and back-offs: tests/pa_cases.py.

Measured on an MI355X: profiles/rx_profile_pa.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import pa_cases as PC
import rx_profile_cases as RC
import test_gpu_rx_profile_doppler as TD

pytestmark = pytest.mark.gpu

CASES = PC.CASES


def run_gpu(c, seed, frame_offset, frames, points=None, ref=None, **kw):
    return W.rx_profile_pa_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                               c["points"] if points is None else points,
                               PC.ref_power(c["name"], seed, frame_offset, frames) if ref is None else ref,
                               active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], **kw)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    c, seed, _, _ = PC.reference(name)
    return run_gpu(c, seed, 0, RC.FRAMES)


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def point_of(prof, i):
    return R.RxProfile(prof.bit_err[i], prof.sym_err[i], prof.err_power[i], prof.decisions)


def check_points(prof, ref, near, c, frames, tag):
    """the rules of the module docstring for every point (``check_tracks`` reads the fields both tuples share by name), and
    pa_power; returns the largest err_power, per-symbol power and pa_power ratio"""
    worst, worst_sym = TD.check_tracks(prof, ref, near, c, frames, tag)
    ratio = RC.pow_ratio(prof.pa_power, ref.pa_power)
    print("%s: pa_power ratio %.2e; mean output over input power per point %s"
          % (tag, ratio, np.round((prof.pa_power[..., 1] / prof.pa_power[..., 0]).mean(axis=(1, 2, 3)), 4)))
    assert prof.pa_power.shape == ref.pa_power.shape and ratio <= RC.POW_TOL, (tag, ratio)
    return worst, worst_sym, ratio


@pytest.mark.parametrize("name", list(CASES))
def test_profile_against_the_mirror(name):
    c, seed, ref, near = PC.reference(name)
    prof = gpu_profile(name)
    st = c["st"]
    tag = "%s S=%d k=%d ibo=%s snr=%s seed=%d" % (name, c["S"], c["k"], PC.IBO_DB[name], tuple(float(v) for v in c["snr"]), seed)
    print("%s: near shares per point %s" % (tag, np.round(near.sum(axis=(1, 2, 3)) / PC.decisions_of(c, RC.FRAMES), 4)))
    PC.check_error_rates(c, ref, RC.FRAMES, tag)
    check_points(prof, ref, near, c, RC.FRAMES, tag)
    on = np.ones(st.n_fft, bool) if c["active"] is None else c["active"]
    assert np.array_equal(prof.decisions, np.where(on, RC.FRAMES * (c["S"] - 1), 0))
    assert prof.bit_err.shape == (3, RC.PAIRS, RC.N_SNR, RC.N_CH, st.n_fft)
    assert prof.err_power_sym.shape == (3, RC.PAIRS, RC.N_SNR, RC.N_CH, c["S"] - 1)
    assert prof.pa_power.shape == (3, RC.PAIRS, RC.N_SNR, RC.N_CH, 2)
    # the amplifier compresses: every amplified point differs from the linear one, and from the other, on every cell, and
    # gives power away; the linear point gives none away, bit for bit, and every point saw the same input
    for i, j in ((1, 0), (2, 0), (2, 1)):
        assert (np.abs(prof.err_power[i] - prof.err_power[j]).max(axis=-1) > 0).all(), (i, j)
        assert (np.abs(prof.err_power_sym[i] - prof.err_power_sym[j]).max(axis=-1) > 0).all(), (i, j)
    assert (prof.pa_power[1:, ..., 1] < prof.pa_power[1:, ..., 0]).all()
    assert np.array_equal(prof.pa_power[0, ..., 1], prof.pa_power[0, ..., 0])
    assert np.array_equal(prof.pa_power[1, ..., 0], prof.pa_power[0, ..., 0]) and np.array_equal(prof.pa_power[2, ..., 0], prof.pa_power[0, ..., 0])


@pytest.mark.parametrize("name", list(CASES))
def test_the_linear_point_is_the_plain_call(name):
    c, seed, _, _ = PC.reference(name)
    prof = gpu_profile(name)
    plain = RC.run_gpu(c, seed, 0, RC.FRAMES)
    alone = run_gpu(c, seed, 0, RC.FRAMES, points=c["points"][:1])
    for got in (point_of(prof, 0), point_of(alone, 0)):
        for x, y in zip(got, plain):
            assert np.array_equal(x, y)
        assert np.ascontiguousarray(got.err_power).tobytes() == plain.err_power.tobytes()
    assert plain.bit_err.sum() > 0


@pytest.mark.parametrize("name", ("n64_wtx_plain", "n256_cpw_half_masked", "n1024_wtx_half_masked"))
def test_a_call_is_its_points_one_per_call(name):
    c, seed, _, _ = PC.reference(name)
    prof = gpu_profile(name)
    pts = c["points"]
    for i in range(3):
        one = run_gpu(c, seed, 0, RC.FRAMES, points=pts[i:i + 1])
        assert same_bits(one[:7], [a[i:i + 1] for a in prof[:7]]), (name, i)
    # and in another order, beside another point
    other = run_gpu(c, seed, 0, RC.FRAMES, points=[pts[2], R.PaPoint(R.PA_RAPP, pts[1].ibo_db, 3.0), pts[0], pts[1]])
    for at, i in ((0, 2), (2, 0), (3, 1)):
        assert same_bits([a[at] for a in other[:7]], [a[i] for a in prof[:7]]), (name, at, i)
    assert not same_bits([other.err_power[1]], [prof.err_power[1]])          # (another smoothness: another point)


def test_repeated_calls_are_identical():
    for name in ("n512_wola_plain", "n64_cp_masked"):
        c, seed, _, _ = PC.reference(name)
        assert same_bits(gpu_profile(name), run_gpu(c, seed, 0, RC.FRAMES))


def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked"
    c, seed, _, _ = PC.reference(name)
    one = gpu_profile(name)
    ref = PC.ref_power(name, seed)
    a = run_gpu(c, seed, 0, 5, ref=ref)
    both = run_gpu(c, seed, 5, 3, ref=ref, out=a)
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert (both.bit_err >= a.bit_err).all() and both.bit_err.sum() > a.bit_err.sum()
    assert RC.pow_ratio(both.err_power, one.err_power) < 1e-12              # fp64 sums of the same fp32 frame sums
    assert RC.pow_ratio(both.err_power_sym, one.err_power_sym) < 1e-12
    assert RC.pow_ratio(both.pa_power, one.pa_power) < 1e-12


def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32"""
    c = PC.case("n128_cpw_half_nbt0")
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    ref = PC.ref_power(c["name"], seed, f0, 8)
    want, near = PC.host(c, seed, f0, 8)
    assert (near.sum(axis=(1, 2, 3)) <= 0.01 * PC.decisions_of(c, 8)).all()
    prof = run_gpu(c, seed, f0, 8)
    check_points(prof, want, near, c, 8, "keys beyond 32 bits")
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    assert not np.array_equal(run_gpu(c, seed & 0xFFFFFFFF, f0, 8, ref=ref).bit_err, prof.bit_err)
    high, low = run_gpu(c, seed, 2 ** 32, 5, ref=ref), run_gpu(c, seed, 0, 5, ref=ref)
    assert not np.array_equal(high.bit_err, low.bit_err) and not np.array_equal(high.err_power, low.err_power)
    assert np.array_equal(run_gpu(c, seed, f0, 3, ref=ref).bit_err + high.bit_err, prof.bit_err)


def test_deep_saturation():
    """ibo = -20 dB: rho around 10 and beyond on nearly every sample, the form (1 / rho) (1 + rho^(-2p))^(-1/(2p)) of the Rapp
    gain with p = 16, and the soft limiter -- a constant-envelope transmitter; the same rules, no overflow, no NaN"""
    c = PC.case("n64_wtx_plain")
    pts = (R.PaPoint(R.PA_CLIP, -20.0), R.PaPoint(R.PA_RAPP, -20.0, 16.0))
    seed, want, near = PC.pick_seed(c, 1500, points=pts)
    prof = run_gpu(c, seed, 0, RC.FRAMES, points=pts)
    assert all(np.isfinite(a).all() for a in (prof.err_power, prof.err_power_sym, prof.pa_power))
    check_points(prof, want, near, c, RC.FRAMES, "deep saturation seed %d" % seed)
    # the output is all but a constant envelope at a_sat, 20 dB below the pair's mean power (a cell's own eight frames carry
    # that mean within a factor of two)
    ratio = prof.pa_power[..., 1] / prof.pa_power[..., 0]
    assert (ratio < 0.02).all() and (ratio > 0.005).all(), ratio


def test_pa_for_window_file_equals_its_host_route(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = np.asarray(channels[:2], np.complex64), [8.0, 16.0]
    pts = [R.PaPoint(R.PA_LINEAR, 0.0), R.PaPoint(R.PA_RAPP, 4.0, 2.0), R.PaPoint(R.PA_CLIP, 3.0)]
    symbols = np.random.RandomState(9).choice(W.timefreq.SYMBOLS_16QAM, size=(32, 16))
    gpu = W.pa_for_window_file("wtx", 8, win, h, snr, pts, gpu=True, symbols=symbols, **kw)
    hst = W.pa_for_window_file("wtx", 8, win, h, snr, pts, gpu=False, symbols=symbols, **kw)
    assert list(gpu) == list(hst) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    plain = W.profile_for_window_file("wtx", 8, win, h, snr, gpu=True, **kw)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        sfx = key[len("profile"):]
        ref_h = np.array([hst[name]["ref_power" + sfx] for name in ("opt", "rc")])
        ref_g = np.array([gpu[name]["ref_power" + sfx] for name in ("opt", "rc")])
        assert np.abs(ref_g - ref_h).max() <= 1e-5 * ref_h.min()          # (fp32 period energies against fp64)
        want, near = R.rx_profile_pa_host(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, ref_h, active=alloc, mask=mask, with_near=True)
        for i, name in enumerate(("opt", "rc")):
            g, hh = gpu[name][key], hst[name][key]
            assert np.array_equal(hh.bit_err, want.bit_err[:, i]) and np.array_equal(hh.err_power, want.err_power[:, i])
            assert np.array_equal(hh.bit_err_sym, want.bit_err_sym[:, i])
            assert g.bit_err.shape == (3, 2, 2, 64) and g.err_power_sym.shape == (3, 2, 2, 3) and g.pa_power.shape == (3, 2, 2, 2)
            assert np.array_equal(g.decisions, hh.decisions)
            ds = np.abs(g.sym_err.astype(np.int64) - hh.sym_err.astype(np.int64)).sum(axis=-1)
            db = np.abs(g.bit_err.astype(np.int64) - hh.bit_err.astype(np.int64)).sum(axis=-1)
            assert (ds <= near[:, i]).all() and (db <= 4 * near[:, i]).all(), (name, key, ds, db, near[:, i])
            assert (g.bit_err[..., ~alloc] == 0).all() and (g.err_power[..., ~alloc] == 0).all()
            for p in range(3):
                assert RC.pow_ratio(g.err_power[p], hh.err_power[p]) <= RC.POW_TOL
                assert RC.pow_ratio(g.err_power_sym[p], hh.err_power_sym[p]) <= RC.POW_TOL
            assert RC.pow_ratio(g.pa_power, hh.pa_power) <= RC.POW_TOL
            # the linear point is profile_for_window_file
            assert np.array_equal(g.bit_err[0], plain[name][key].bit_err)
            assert np.ascontiguousarray(g.err_power[0]).tobytes() == plain[name][key].err_power.tobytes()
            # the spectrum side: the periodograms per point under the PSD tests' tolerance, the OBR under their ratio
            gp, hp = gpu[name]["psd" + sfx], hst[name]["psd" + sfx]
            assert gp.shape == hp.shape == (3, 512)
            assert (np.abs(gp - hp) < 2e-5 * hp.max(axis=-1, keepdims=True)).all()             # (PSD_RTOL of the PSD tests)
            assert np.abs(gpu[name]["obr" + sfx] / hst[name]["obr" + sfx] - 1).max() <= 2e-4
            assert hst[name]["obr" + sfx][2] > hst[name]["obr" + sfx][0]            # regrowth behind the limiter


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two points: a chunk of the documented budget ends inside a cell; neither the split of the
    frame range nor the other chunking of the plain call changes an integer counter"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    c.update(active=CM.half_band_allocation(1024), name="over_the_frame_limit")
    pts = (R.PaPoint(R.PA_LINEAR, 0.0), R.PaPoint(R.PA_RAPP, 3.0, 2.0))
    Tv = st.frame_len(S)
    per_chunk = R.rx_profile_pa_chunk_frames(st, S, False, 2)
    assert per_chunk == _lib.RX_PROFILE_CHUNK_BYTES // (8 * (S * 1024 + Tv) + 8 * 2 * (1024 + S + Tv))
    assert 200 < per_chunk < R.rx_profile_sync_chunk_frames(st, S, False, 2)
    frames = per_chunk // 2 + 19                                            # 8 cells: four chunks and a bit
    ref = np.full(RC.PAIRS, 1.0 / 1024, np.float32)                         # (unit-power symbols on the half band: some 0.5 / N)
    one = run_gpu(c, 7000, 0, frames, points=pts, ref=ref)
    assert int(one.decisions.max()) == frames * (S - 1)
    parts = run_gpu(c, 7000, frames - 7, 7, points=pts, ref=ref, out=run_gpu(c, 7000, 0, frames - 7, points=pts, ref=ref))
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym"):
        assert np.array_equal(getattr(parts, f), getattr(one, f)), f
    assert RC.pow_ratio(parts.err_power, one.err_power) < 1e-12
    assert RC.pow_ratio(parts.err_power_sym, one.err_power_sym) < 1e-12
    assert RC.pow_ratio(parts.pa_power, one.pa_power) < 1e-12
    assert R.rx_profile_kernel_ms() > 0.0
    plain = RC.run_gpu(c, 7000, 0, frames)
    assert np.array_equal(one.bit_err[0], plain.bit_err) and np.array_equal(one.sym_err[0], plain.sym_err)
    assert RC.pow_ratio(one.err_power[0], plain.err_power) < 1e-12
    assert not np.array_equal(one.bit_err[1], plain.bit_err)
    assert (one.pa_power[1, ..., 1] < one.pa_power[1, ..., 0]).all()
