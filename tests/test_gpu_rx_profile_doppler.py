"""``wofdm_rx_profile_doppler`` on the GPU (the Tx chain of wofdm_rx_profile once, wofdm_rxprof_doppler_kernel<N>,
wofdm_rxprof_sync_reduce_kernel<N>) against the fp64 host route ``rx_profile_doppler_host``: the same frames, the same tracks,
from the same Philox streams (the mirror itself is tied to ``frame_profile`` in tests/test_rx_profile_doppler_host.py).

Rules, per track: those of rx_profile_cases.check_profile with the mirror in the oracle's place -- per cell sum_n |sym_gpu -
sym_ref| <= near and sum_n |bit_gpu - bit_ref| <= k near, unloaded bins exactly 0, |err_power - ref| <= POW_TOL (ref[n] + mean_n
ref); the per-symbol counters under the same near bound per cell (sums over s), the per-symbol power under the same ratio rule
(over s).  The seed of a case is the first from its base seed on, of 32, for which the mirror alone has at most 1 % near
decisions on EVERY track (``RC.pick_seed``'s cap, decided on the CPU); cases, tracks, SNR points and Doppler values:
tests/doppler_cases.py.

Measured on an MI355X: profiles/rx_profile_doppler.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import channels as CH
from wofdm_amd import rx_profile as R

import doppler_cases as DC
import rx_profile_cases as RC

pytestmark = pytest.mark.gpu

CASES = DC.CASES


def run_gpu(c, seed, frame_offset, frames, tracks=None, knot_step=None, **kw):
    return W.rx_profile_doppler_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["tracks"] if tracks is None else tracks,
                                    c["knot_step"] if knot_step is None else knot_step, c["snr"], seed, frame_offset, frames,
                                    active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], **kw)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    c, seed, _, _ = DC.reference(name)
    return run_gpu(c, seed, 0, RC.FRAMES)


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def track_of(prof, i):
    return R.RxProfile(prof.bit_err[i], prof.sym_err[i], prof.err_power[i], prof.decisions)


def check_tracks(prof, ref, near, c, frames, tag):
    """the rules of the module docstring for every track; returns the largest err_power and per-symbol power ratio"""
    k, worst, worst_sym = c["k"], 0.0, 0.0
    assert ref.bit_err.shape[0] == prof.bit_err.shape[0] == near.shape[0]
    for i in range(prof.bit_err.shape[0]):
        rd = dict(bit=ref.bit_err[i].astype(np.int64), sym=ref.sym_err[i].astype(np.int64), pow=ref.err_power[i], near=near[i],
                  decisions=DC.decisions_of(c, frames))
        ttag = "%s track %d" % (tag, i)
        worst = max(worst, RC.check_profile(track_of(prof, i), rd, c, ttag))
        ds = np.abs(prof.sym_err_sym[i].astype(np.int64) - ref.sym_err_sym[i].astype(np.int64)).sum(axis=-1)
        db = np.abs(prof.bit_err_sym[i].astype(np.int64) - ref.bit_err_sym[i].astype(np.int64)).sum(axis=-1)
        ratio = RC.pow_ratio(prof.err_power_sym[i], ref.err_power_sym[i])
        print("%s: per symbol: sym diff %d, bit diff %d, power ratio %.2e" % (ttag, ds.sum(), db.sum(), ratio))
        assert (ds <= near[i]).all() and (db <= k * near[i]).all(), (ttag, ds, db, near[i])
        assert ratio <= RC.POW_TOL, (ttag, ratio)
        worst_sym = max(worst_sym, ratio)
    # per track and cell the symbols add up to the bins, exactly
    assert np.array_equal(prof.bit_err_sym.sum(axis=-1), prof.bit_err.sum(axis=-1))
    assert np.array_equal(prof.sym_err_sym.sum(axis=-1), prof.sym_err.sum(axis=-1))
    print("%s: largest err_power ratio %.2e, per symbol %.2e" % (tag, worst, worst_sym))
    return worst, worst_sym


@pytest.mark.parametrize("name", list(CASES))
def test_profile_against_the_mirror(name):
    c, seed, ref, near = DC.reference(name)
    prof = gpu_profile(name)
    st = c["st"]
    tag = "%s S=%d k=%d B=%d nu=%s snr=%s seed=%d" % (name, c["S"], c["k"], st.stride, DC.NU[name], tuple(float(v) for v in c["snr"]), seed)
    print("%s: near shares per track %s" % (tag, np.round(near.sum(axis=(1, 2, 3)) / DC.decisions_of(c, RC.FRAMES), 4)))
    DC.check_error_rates(c, ref, RC.FRAMES, tag)
    check_tracks(prof, ref, near, c, RC.FRAMES, tag)
    on = np.ones(st.n_fft, bool) if c["active"] is None else c["active"]
    assert np.array_equal(prof.decisions, np.where(on, RC.FRAMES * (c["S"] - 1), 0))
    assert prof.bit_err.shape == (3, RC.PAIRS, RC.N_SNR, RC.N_CH, st.n_fft)
    assert prof.err_power_sym.shape == (3, RC.PAIRS, RC.N_SNR, RC.N_CH, c["S"] - 1)
    # the channel moves: every moving track differs from the static one, and from the other, on every cell
    for i, j in ((1, 0), (2, 0), (2, 1)):
        assert (np.abs(prof.err_power[i] - prof.err_power[j]).max(axis=-1) > 0).all(), (i, j)
        assert (np.abs(prof.err_power_sym[i] - prof.err_power_sym[j]).max(axis=-1) > 0).all(), (i, j)


def test_steps_and_knot_counts_against_the_mirror():
    """a step that divides nothing (37), two knots whose interval ends on the last sample of conv (the clamp on q), 64 knots; each
    with a seed of its own, picked on the CPU as a case's is"""
    c = DC.case(DC.EXTRA)
    for tracks, step in DC.extra_tracks(c):
        seed, ref, near = DC.pick_seed(c, 900 + step, tracks=tracks, knot_step=step)
        prof = run_gpu(c, seed, 0, RC.FRAMES, tracks=tracks, knot_step=step)
        check_tracks(prof, ref, near, c, RC.FRAMES, "%s step %d knots %d seed %d" % (DC.EXTRA, step, tracks.shape[2], seed))
        plain = RC.run_gpu(c, seed, 0, RC.FRAMES)
        if tracks.shape[0] == 2:
            # the static track does not care how it is cut into knots
            assert same_bits(track_of(prof, 0), plain), step
            assert (np.abs(prof.err_power[1] - prof.err_power[0]).max(axis=-1) > 0).all()
        else:
            assert (np.abs(prof.err_power[0] - plain.err_power).max(axis=-1) > 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_the_static_track_is_the_plain_call(name):
    c, seed, _, _ = DC.reference(name)
    prof = gpu_profile(name)
    plain = RC.run_gpu(c, seed, 0, RC.FRAMES)
    alone = run_gpu(c, seed, 0, RC.FRAMES, tracks=c["tracks"][:1])
    for got in (track_of(prof, 0), track_of(alone, 0)):
        for x, y in zip(got, plain):
            assert np.array_equal(x, y)
        assert np.ascontiguousarray(got.err_power).tobytes() == plain.err_power.tobytes()
    assert plain.bit_err.sum() > 0


@pytest.mark.parametrize("name", ("n64_wtx_plain", "n256_cpw_half_masked", "n1024_wtx_half_masked"))
def test_a_call_is_its_tracks_one_per_call(name):
    c, seed, _, _ = DC.reference(name)
    prof = gpu_profile(name)
    for i in range(3):
        one = run_gpu(c, seed, 0, RC.FRAMES, tracks=c["tracks"][i:i + 1])
        assert same_bits(one[:6], [a[i:i + 1] for a in prof[:6]]), (name, i)
    # and in another order, beside another track
    other = run_gpu(c, seed, 0, RC.FRAMES, tracks=np.stack([c["tracks"][2], c["tracks"][1][::-1], c["tracks"][0], c["tracks"][1]]))
    for at, i in ((0, 2), (2, 0), (3, 1)):
        assert same_bits([a[at] for a in other[:6]], [a[i] for a in prof[:6]]), (name, at, i)
    assert not same_bits([other.err_power[1]], [prof.err_power[1]])          # (the channels swapped: another track)


def test_repeated_calls_are_identical():
    for name in ("n512_wola_plain", "n64_cp_masked"):
        c, seed, _, _ = DC.reference(name)
        assert same_bits(gpu_profile(name), run_gpu(c, seed, 0, RC.FRAMES))


def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked"
    c, seed, _, _ = DC.reference(name)
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
    c = DC.case("n128_cpw_half_nbt0")
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    ref, near = DC.host(c, seed, f0, 8)
    assert (near.sum(axis=(1, 2, 3)) <= 0.01 * DC.decisions_of(c, 8)).all()
    prof = run_gpu(c, seed, f0, 8)
    check_tracks(prof, ref, near, c, 8, "keys beyond 32 bits")
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    assert not np.array_equal(run_gpu(c, seed & 0xFFFFFFFF, f0, 8).bit_err, prof.bit_err)
    high, low = run_gpu(c, seed, 2 ** 32, 5), run_gpu(c, seed, 0, 5)
    assert not np.array_equal(high.bit_err, low.bit_err) and not np.array_equal(high.err_power, low.err_power)
    assert np.array_equal(run_gpu(c, seed, f0, 3).bit_err + high.bit_err, prof.bit_err)


def test_doppler_for_window_file_equals_its_host_route(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = np.asarray(channels[:2], np.complex64), [8.0, 16.0]
    B = st.stride
    tracks = np.stack([np.stack([np.tile(h[ch], (6, 1)) for ch in range(2)])] +
                      [np.stack([CH.gen_chan_track("vehicularA", h.shape[1], nu * DC.FS / B, DC.FS, B, 6, np.random.RandomState(30 + ch))
                                 for ch in range(2)]) for nu in (0.01, 0.03)]).astype(np.complex64)
    gpu = W.doppler_for_window_file("wtx", 8, win, tracks, B, snr, gpu=True, **kw)
    hst = W.doppler_for_window_file("wtx", 8, win, tracks, B, snr, gpu=False, **kw)
    assert list(gpu) == list(hst) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    plain = W.profile_for_window_file("wtx", 8, win, h, snr, gpu=True, **kw)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want, near = R.rx_profile_doppler_host(st, 4, 4, w_tx, w_rx, tracks, B, snr, 21, 0, 4, active=alloc, mask=mask, with_near=True)
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
            # the static track is profile_for_window_file
            assert np.array_equal(g.bit_err[0], plain[name][key].bit_err)
            assert np.ascontiguousarray(g.err_power[0]).tobytes() == plain[name][key].err_power.tobytes()


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two tracks: a chunk of the documented budget ends inside a cell; neither the split of the
    frame range nor the other chunking of the plain call changes an integer counter"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    c.update(active=CM.half_band_allocation(1024), knot_step=st.stride)
    c["tracks"] = DC.tracks_of(c, (0.0, 0.002), st.stride, S + 2)
    Tv = st.frame_len(S)
    per_chunk = R.rx_profile_doppler_chunk_frames(st, S, False, 2)
    assert per_chunk == _lib.RX_PROFILE_CHUNK_BYTES // (8 * (S * 1024 + Tv) + 8 * 2 * (1024 + S))
    assert 250 < per_chunk < R.rx_profile_chunk_frames(st, S, False)
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
