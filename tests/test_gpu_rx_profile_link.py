"""``wofdm_rx_profile_link`` on the GPU (the Tx chain once, the neighbour's, wofdm_pa_wave_kernel, wofdm_pn_walk_kernel,
wofdm_rxprof_link_kernel<N>, wofdm_rxprof_sync_reduce_kernel<N>, wofdm_pa_power_reduce_kernel).

1. Six identities, by bytes: a call whose points switch on one impairment each returns, point by point, the bytes of that
   impairment's own entry point with the same cfg and seed -- wofdm_rx_profile, _sync, _pn, _pa (pa_power included), _doppler and
   _aci (its three per-bin fields).
2. Composed points against the fp64 host route ``rx_profile_link_host`` (tied to the arms' mirrors in
   tests/test_rx_profile_link_host.py) under the rules of test_gpu_rx_profile_pn.check_points: per cell sum_n |sym_gpu - sym_ref|
   <= near and sum_n |bit_gpu - bit_ref| <= k near, unloaded bins exactly 0, |err_power - ref| <= POW_TOL (ref[n] + mean_n ref),
   the same per data symbol, and the symbols add up to the bins exactly.  The composed points are COMPOSED below: everything on
   at moderate levels (6 dB Rapp, a 185 Hz track, timing +2, cfo 0.02 tracked, linewidth 1e-3 tracked, a neighbour at 0 dB), the
   same free-running with timing -3, amplifier + neighbour only, track + phase noise only.  The seed of a case is the first of 32
   from its base seed for which the MIRROR alone has at most 1 % near decisions at every composed point (``RC.pick_seed``'s cap,
   decided on the CPU).  No point had to be made milder.
3. - 8.: a sweep is its points one per call, repeated calls, split frame ranges, keys beyond 32 bits, chunks that end inside a
   cell, ``link_for_window_file``.

The geometry is RC.make_case's (2 pairs x 2 SNR points x 2 channels x 8 frames), the shapes test_gpu_rx_profile_pn.py's seven, the
tracks tests/doppler_cases.py's, the amplifier points' reference power tests/pa_cases.py's.

Measured on an MI355X: profiles/rx_profile_link.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import doppler_cases as DC
import pa_cases as PAC
import rx_profile_cases as RC

pytestmark = pytest.mark.gpu

CASES = DC.CASES
L = R.LinkPoint
RAPP6 = R.PaPoint(R.PA_RAPP, 6.0, 2.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """tests/pa_cases.py's case (doppler_cases' shape, SNR points and tracks) with a fourth track at 185 Hz, the neighbour's
    allocation, and the points of test 2: the four composed ones, then the single-impairment points they are made of"""
    c = dict(PAC.case(name))
    st, S = c["st"], c["S"]
    B = st.stride
    c["tracks"] = np.concatenate([c["tracks"], DC.tracks_of(c, (185.0 * B / DC.FS,), B, S + 2)])
    # the knots cover the frame and the two samples the late window of the composed points reaches
    assert (S + 1) * B >= st.frame_len(S) + c["h"].shape[1] - 2 + 2
    c["aci_active"] = CM.half_band_allocation(st.n_fft) if c["active"] is None else ~np.asarray(c["active"], bool)
    d = B // 3
    c["delay"] = d
    c["composed"] = [
        L(RAPP6, 3, 2, 0.02, 1, 1e-3, 1, (d, 0.0)),
        L(RAPP6, 3, -3, 0.02, 0, 1e-3, 0, (d, 0.0)),
        L(pa=RAPP6, aci=(d, 0.0)),
        L(track=3, linewidth=1e-3, cpe_tracked=1),
    ]
    c["singles"] = [L(pa=RAPP6), L(track=3), L(timing=2, cfo=0.02, cfo_tracked=1), L(linewidth=1e-3, cpe_tracked=1), L(aci=(d, 0.0)),
                    L(timing=-3, cfo=0.02, cfo_tracked=0), L(linewidth=1e-3, cpe_tracked=0)]
    #: composed point -> the single-impairment points it is made of
    c["parts"] = {0: (0, 1, 2, 3, 4), 1: (0, 1, 5, 6, 4), 2: (0, 4), 3: (1, 3)}
    c["points"] = c["composed"]
    return c


def base_seed(name):
    return 100 * (1 + list(CASES).index(name))


def sides(c, seed, frame_offset, frames):
    return dict(tracks=c["tracks"], knot_step=c["knot_step"], aci_active=c["aci_active"],
                ref_power=PAC.ref_power(c["name"], seed, frame_offset, frames), active=c["active"], mask=c["mask"],
                noise_before_truncate=c["nbt"])


def host(c, seed, frame_offset, frames, points=None):
    """the mirror's profile and its near decisions [points, pairs, n_snr, n_ch]"""
    return R.rx_profile_link_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                  c["points"] if points is None else points, with_near=True, **sides(c, seed, frame_offset, frames))


def run_gpu(c, seed, frame_offset, frames, points=None, ref_frames=None, **kw):
    """(ref_frames: the (first, count) the reference power was measured over, where it is not the call's own range)"""
    s = sides(c, seed, *((frame_offset, frames) if ref_frames is None else ref_frames))
    return W.rx_profile_link_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                 c["points"] if points is None else points, **s, **kw)


decisions_of = DC.decisions_of


def pick_seed(c, base, frame_offset=0, frames=RC.FRAMES, tries=32):
    """first seed from base on whose MIRROR profile has at most 1 % near decisions at every composed point (RC.pick_seed's cap)"""
    for seed in range(base, base + tries):
        prof, near = host(c, seed, frame_offset, frames)
        if (near.sum(axis=(1, 2, 3)) <= 0.01 * decisions_of(c, frames)).all():
            return seed, prof, near
    raise AssertionError("no seed in [%d, %d) keeps the mirror's decisions clear of the thresholds" % (base, base + tries))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    seed, prof, near = pick_seed(c, base_seed(name))
    return c, seed, prof, near


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    """the composed points and, behind them, their single-impairment points, in one call"""
    c, seed, _, _ = reference(name)
    return run_gpu(c, seed, 0, RC.FRAMES, points=c["composed"] + c["singles"])


def same_bits(a, b):
    a, b = [np.ascontiguousarray(x) for x in a], [np.ascontiguousarray(x) for x in b]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_points(prof, ref, near, c, frames, tag):
    """test_gpu_rx_profile_pn.check_points on the points c["points"]; returns the largest err_power and per-symbol power ratio"""
    k, worst, worst_sym = c["k"], 0.0, 0.0
    assert len(c["points"]) == prof.bit_err.shape[0]
    for i, q in enumerate(c["points"]):
        rd = dict(bit=ref.bit_err[i].astype(np.int64), sym=ref.sym_err[i].astype(np.int64), pow=ref.err_power[i], near=near[i],
                  decisions=decisions_of(c, frames))
        ptag = "%s point %d" % (tag, i)
        worst = max(worst, RC.check_profile(R.RxProfile(prof.bit_err[i], prof.sym_err[i], prof.err_power[i], prof.decisions), rd, c,
                                            ptag))
        ds = np.abs(prof.sym_err_sym[i].astype(np.int64) - ref.sym_err_sym[i].astype(np.int64)).sum(axis=-1)
        db = np.abs(prof.bit_err_sym[i].astype(np.int64) - ref.bit_err_sym[i].astype(np.int64)).sum(axis=-1)
        ratio = RC.pow_ratio(prof.err_power_sym[i], ref.err_power_sym[i])
        print("%s: per symbol: sym diff %d, bit diff %d, power ratio %.2e" % (ptag, ds.sum(), db.sum(), ratio))
        assert (ds <= near[i]).all() and (db <= k * near[i]).all(), (ptag, ds, db, near[i])
        assert ratio <= RC.POW_TOL, (ptag, ratio)
        worst_sym = max(worst_sym, ratio)
        assert RC.pow_ratio(prof.pa_power[i], ref.pa_power[i]) <= RC.POW_TOL, ptag        # (test_gpu_rx_profile_pa.py's rule)
    assert np.array_equal(prof.bit_err_sym.sum(axis=-1), prof.bit_err.sum(axis=-1))
    assert np.array_equal(prof.sym_err_sym.sum(axis=-1), prof.sym_err.sum(axis=-1))
    print("%s: largest err_power ratio %.2e, per symbol %.2e" % (tag, worst, worst_sym))
    return worst, worst_sym


# ---- 1. the six identities ----

@pytest.mark.parametrize("name", list(CASES))
def test_one_impairment_is_its_own_entry_point_by_bytes(name):
    c, seed = case(name), base_seed(name)
    st, k, S, B = c["st"], c["k"], c["S"], c["st"].stride
    sync, pn, pa, aci = R.SyncPoint(-3, 0.05, 0), R.PnPoint(0.02, 1), R.PaPoint(R.PA_RAPP, 3.0, 2.0), (B // 3, 10.0)
    got = run_gpu(c, seed, 0, RC.FRAMES, points=[L(), L(timing=-3, cfo=0.05, cfo_tracked=0), L(linewidth=0.02, cpe_tracked=1),
                                                 L(pa=pa), L(track=1), L(aci=aci)])
    head = (st, k, S, c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, 0, RC.FRAMES)
    kw = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    ref = PAC.ref_power(name, seed)
    assert got.bit_err.shape == (6, RC.PAIRS, RC.N_SNR, RC.N_CH, st.n_fft) and got.pa_power.shape == (6, RC.PAIRS, RC.N_SNR, RC.N_CH, 2)
    plain = W.rx_profile_gpu(*head, **kw)
    assert same_bits([a[0] for a in got[:3]], plain[:3]), "all off"
    assert np.array_equal(got.decisions, plain.decisions)
    one = W.rx_profile_sync_gpu(*head, [sync], **kw)
    assert same_bits([a[1] for a in got[:6]], [a[0] for a in one[:6]]), "sync"
    one = W.rx_profile_pn_gpu(*head, [pn], **kw)
    assert same_bits([a[2] for a in got[:6]], [a[0] for a in one[:6]]), "pn"
    one = W.rx_profile_pa_gpu(*head, [pa], ref, **kw)
    assert same_bits([a[3] for a in got[:7]], [a[0] for a in one[:7]]), "pa"
    one = W.rx_profile_doppler_gpu(st, k, S, c["w_tx"], c["w_rx"], c["tracks"], c["knot_step"], c["snr"], seed, 0, RC.FRAMES, **kw)
    assert same_bits([a[4] for a in got[:6]], [a[1] for a in one[:6]]), "doppler"
    one = W.rx_profile_aci_gpu(*head, c["aci_active"], aci[0], aci[1], **kw)
    assert same_bits([a[5] for a in got[:3]], one[:3]), "aci"
    # each impairment is on: its point differs from the all-off point on every cell
    for i in range(1, 6):
        assert (np.abs(got.err_power[i] - got.err_power[0]).max(axis=-1) > 0).all(), i
    # a point without an amplifier: the power behind it is the power before it
    for i in (0, 1, 2, 4, 5):
        assert np.array_equal(got.pa_power[i, ..., 0], got.pa_power[i, ..., 1]) and (got.pa_power[i] > 0).all()


# ---- 2. composed points against the mirror ----

@pytest.mark.parametrize("name", list(CASES))
def test_composed_points_against_the_mirror(name):
    c, seed, ref, near = reference(name)
    allp = gpu_profile(name)
    nc = len(c["composed"])
    prof = R.RxProfileLink(*(a[:nc] for a in allp[:-1]), allp.decisions)
    st = c["st"]
    tag = "%s S=%d k=%d B=%d gamma=%d seed=%d" % (name, c["S"], c["k"], st.stride, st.prefix_rm, seed)
    print("%s: near shares per point %s" % (tag, np.round(near.sum(axis=(1, 2, 3)) / decisions_of(c, RC.FRAMES), 4)))
    check_points(prof, ref, near, c, RC.FRAMES, tag)
    on = np.ones(st.n_fft, bool) if c["active"] is None else c["active"]
    assert np.array_equal(prof.decisions, np.where(on, RC.FRAMES * (c["S"] - 1), 0))
    # every composed point differs from each of its single-impairment points on every cell
    for i, parts in c["parts"].items():
        for j in parts:
            assert (np.abs(allp.err_power[i] - allp.err_power[nc + j]).max(axis=-1) > 0).all(), (i, j)


# ---- 3. a sweep is its points ----

@pytest.mark.parametrize("name", ("n64_wtx_plain", "n256_cpw_half_masked", "n1024_wtx_half_masked"))
def test_a_sweep_is_its_points_one_per_call(name):
    c, seed, _, _ = reference(name)
    allp = gpu_profile(name)
    pts = c["composed"] + c["singles"]
    for i in (0, 1, 2, 3, 5, 8):
        one = run_gpu(c, seed, 0, RC.FRAMES, points=[pts[i]])
        assert same_bits(one[:7], [a[i:i + 1] for a in allp[:7]]), (name, i)
    # and in another order, beside other points
    other = run_gpu(c, seed, 0, RC.FRAMES, points=[pts[1], L(linewidth=0.11), pts[0], L(track=2, aci=(0, -3.0))])
    assert same_bits([a[0] for a in other[:7]], [a[1] for a in allp[:7]])
    assert same_bits([a[2] for a in other[:7]], [a[0] for a in allp[:7]])


# ---- 4. repeated calls ----

def test_repeated_calls_are_identical():
    for name in ("n512_wola_plain", "n64_cp_masked"):
        c, seed, _, _ = reference(name)
        assert same_bits(gpu_profile(name), run_gpu(c, seed, 0, RC.FRAMES, points=c["composed"] + c["singles"]))


# ---- 5. split frame ranges ----

def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked"
    c, seed, _, _ = reference(name)
    one = run_gpu(c, seed, 0, RC.FRAMES)
    a = run_gpu(c, seed, 0, 5, ref_frames=(0, RC.FRAMES))
    both = run_gpu(c, seed, 5, 3, ref_frames=(0, RC.FRAMES), out=a)
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert (both.bit_err >= a.bit_err).all() and both.bit_err.sum() > a.bit_err.sum()
    assert RC.pow_ratio(both.err_power, one.err_power) < 1e-12              # fp64 sums of the same fp32 frame sums
    assert RC.pow_ratio(both.err_power_sym, one.err_power_sym) < 1e-12
    assert RC.pow_ratio(both.pa_power, one.pa_power) < 1e-12


# ---- 6. keys beyond 32 bits ----

def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32"""
    c = case("n128_cpw_half_nbt0")
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    ref, near = host(c, seed, f0, 8)
    assert (near.sum(axis=(1, 2, 3)) <= 0.01 * decisions_of(c, 8)).all()
    prof = run_gpu(c, seed, f0, 8)
    check_points(prof, ref, near, c, 8, "keys beyond 32 bits")
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    assert not np.array_equal(run_gpu(c, seed & 0xFFFFFFFF, f0, 8, ref_frames=(f0, 8)).bit_err, prof.bit_err)
    high, low = run_gpu(c, seed, 2 ** 32, 5, ref_frames=(f0, 8)), run_gpu(c, seed, 0, 5, ref_frames=(f0, 8))
    assert not np.array_equal(high.bit_err, low.bit_err) and not np.array_equal(high.err_power, low.err_power)
    assert np.array_equal(run_gpu(c, seed, f0, 3, ref_frames=(f0, 8)).bit_err + high.bit_err, prof.bit_err)


# ---- 7. chunks ----

def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two points: a chunk of the documented budget ends inside a cell; neither the split of the
    frame range nor the other chunking of the plain call changes an integer counter"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    pts = [L(), L(linewidth=0.01)]
    c.update(active=CM.half_band_allocation(1024))
    Tv = st.frame_len(S)
    per_chunk = R.rx_profile_link_chunk_frames(st, S, False, 2, False)
    assert per_chunk == _lib.RX_PROFILE_CHUNK_BYTES // (8 * (S * 1024 + Tv) + 8 * 2 * (1024 + S + Tv) + 8 * S * st.stride)
    with_nb = R.rx_profile_link_chunk_frames(st, S, False, 2, True)
    assert with_nb == _lib.RX_PROFILE_CHUNK_BYTES // (8 * (S * 1024 + Tv) + 8 * 2 * (1024 + S + Tv) + 8 * S * st.stride +
                                                      8 * ((S + 1) * 1024 + Tv + st.stride))
    assert 250 < with_nb < per_chunk < R.rx_profile_pn_chunk_frames(st, S, False, 2)
    frames = per_chunk // 2 + 19                                            # 8 cells: four chunks and a bit

    def run(f0, n, **kw):
        return W.rx_profile_link_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, f0, n, pts, active=c["active"], **kw)
    one = run(0, frames)
    assert int(one.decisions.max()) == frames * (S - 1)
    parts = run(frames - 7, 7, out=run(0, frames - 7))
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym"):
        assert np.array_equal(getattr(parts, f), getattr(one, f)), f
    assert RC.pow_ratio(parts.err_power, one.err_power) < 1e-12
    assert RC.pow_ratio(parts.err_power_sym, one.err_power_sym) < 1e-12
    assert R.rx_profile_kernel_ms() > 0.0
    plain = RC.run_gpu(c, 7000, 0, frames)
    assert np.array_equal(one.bit_err[0], plain.bit_err) and np.array_equal(one.sym_err[0], plain.sym_err)
    assert RC.pow_ratio(one.err_power[0], plain.err_power) < 1e-12
    assert not np.array_equal(one.bit_err[1], plain.bit_err)


# ---- 8. the window file ----

def test_link_for_window_file_equals_its_host_route(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    B = st.stride
    tracks = DC.tracks_of(dict(st=st, h=np.asarray(h, np.complex64)), (0.01,), B, 6)
    pts = [L(), L(RAPP6, 0, 2, 0.02, 1, 1e-3, 1, (B // 3, 0.0)), L(pa=RAPP6, aci=(5, 3.0))]
    gpu = W.link_for_window_file("wtx", 8, win, h, snr, pts, tracks=tracks, knot_step=B, gpu=True, **kw)
    hst = W.link_for_window_file("wtx", 8, win, h, snr, pts, tracks=tracks, knot_step=B, gpu=False, **kw)
    assert list(gpu) == list(hst) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    plain = W.profile_for_window_file("wtx", 8, win, h, snr, gpu=True, **kw)
    near_kw = dict(tracks=tracks, knot_step=B, aci_active=~alloc, active=alloc, with_near=True)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        ref = R.pa_ref_power(st, 4, 4, w_tx, 21, 0, 4, active=alloc, mask=mask, gpu=False)
        want, near = R.rx_profile_link_host(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, ref_power=ref, mask=mask, **near_kw)
        for i, name in enumerate(("opt", "rc")):
            g, hh = gpu[name][key], hst[name][key]
            assert np.array_equal(hh.bit_err, want.bit_err[:, i]) and np.array_equal(hh.err_power, want.err_power[:, i])
            assert g.bit_err.shape == (3, 2, 2, 64) and g.err_power_sym.shape == (3, 2, 2, 3) and g.pa_power.shape == (3, 2, 2, 2)
            assert np.array_equal(g.decisions, hh.decisions)
            ds = np.abs(g.sym_err.astype(np.int64) - hh.sym_err.astype(np.int64)).sum(axis=-1)
            db = np.abs(g.bit_err.astype(np.int64) - hh.bit_err.astype(np.int64)).sum(axis=-1)
            assert (ds <= near[:, i]).all() and (db <= 4 * near[:, i]).all(), (name, key, ds, db, near[:, i])
            assert (g.bit_err[..., ~alloc] == 0).all() and (g.err_power[..., ~alloc] == 0).all()
            for p in range(3):
                assert RC.pow_ratio(g.err_power[p], hh.err_power[p]) <= RC.POW_TOL
                assert RC.pow_ratio(g.err_power_sym[p], hh.err_power_sym[p]) <= RC.POW_TOL
            # the all-off point is profile_for_window_file
            assert np.array_equal(g.bit_err[0], plain[name][key].bit_err)
            assert np.ascontiguousarray(g.err_power[0]).tobytes() == plain[name][key].err_power.tobytes()
