"""``wofdm_rx_profile_tracking`` on the GPU (the soft call's kernels with wofdm_rxprof_tracking_kernel<N> in the soft kernel's
place), on the geometry of tests/rx_profile_cases.py (2 pairs x 2 SNR points x 2 channels x 8 frames).

Shapes: the seven of tests/doppler_cases.py as tests/test_gpu_rx_profile_link.py prepares them, and one of this file's own, N =
1024, wtx, half band, unmasked, S = 5 -- more symbols than the four waves of the N = 1024 kernel, so the order 0, S - 1, 1, ... of a
point with a postamble spans two rounds there.  Link points: the link test's first composed point (everything on), a free-running
carrier offset of 0.02, and the case's track 2; each behind the receivers (0, 0), (1, 0), (0, 1), (1, 1) -- those with a postamble
where S >= 3.  The comb is every eighth loaded bin; four scales.

1. Byte identities against ``rx_profile_soft_gpu``: without a comb and with every point (0, 0) all nine fields; with the comb the
   (0, 0) points' bit_err, sym_err, err_power and bit_penalty on every data bin.
2. Against the fp64 host route ``rx_profile_tracking_host`` (tests/test_rx_profile_tracking_host.py) under
   ``RC.check_profile``'s rules per point: sums of count differences at most near, at most k near for bits, ``RC.POW_TOL`` = 1e-3 on
   err_power per bin and per symbol, ``pen_ratio`` <= 1e-3 on both penalties; pilot bins, unloaded bins and a postamble are exact
   zeros.  The near rule's weight is max_n |Hh_s| / |Hh_s[n]| per symbol.
3. The seed of a case is the first of 32 from its base seed for which the MIRROR alone has at most 1 % near decisions at every
   point (of the point's own decisions), decided on the CPU.  n64_cp_masked (full band, masked, 16-QAM) finds none at its SNR
   points 14 and 22 dB -- the share of near decisions grows with the SNR there, as tests/rx_profile_cases.py notes -- and runs at
   ``RC.SNR_DB[4]``, 8 and 16 dB; the cap is never lifted.
4. A sweep is its points one per call, a scale its own call; repeated calls; a frame range split in two; keys beyond 32 bits; N =
   1024, S = 16, cp + cs = 64 with a chunk that ends inside a cell, by bytes; ``tracking_for_window_file``.

Measured on an MI355X: profiles/rx_profile_tracking.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import doppler_cases as DC
import rx_profile_cases as RC
import test_gpu_rx_profile_link as TL

pytestmark = pytest.mark.gpu

OWN = "n1024_wtx_half_s5"
CASES = list(TL.CASES) + [OWN]
L, TP = R.LinkPoint, R.TrackingPoint
SCALES = (1.0, 0.5, 0.2, 0.05)
#: the case that finds no seed at its own SNR points (see 3. above) and runs at RC.SNR_DB[4]
LOWER_SNR = "n64_cp_masked"


@functools.lru_cache(maxsize=None)
def case(name):
    """the link test's case, or this file's own shape prepared the same way; with the comb, the link points and the receivers"""
    if name == OWN:
        c = RC.make_case(W.make_structure("wtx", 1024, 128), 4, 5, "half", 7024)
        c["snr"] = np.array((10.0, 18.0), np.float32)
        st, S = c["st"], c["S"]
        B = st.stride
        c["knot_step"] = B
        c["tracks"] = DC.tracks_of(c, (0.0, 0.02, 0.04, 185.0 * B / DC.FS), B, S + 2)
        assert (S + 1) * B >= st.frame_len(S) + c["h"].shape[1] - 2 + 2
        c["aci_active"] = ~np.asarray(c["active"], bool)
        c["composed"] = [L(TL.RAPP6, 3, 2, 0.02, 1, 1e-3, 1, (B // 3, 0.0))]
    else:
        c = dict(TL.case(name))
    if name == LOWER_SNR:
        c["snr"] = np.array(RC.SNR_DB[4], np.float32)
    c["name"] = name
    on = np.ones(c["st"].n_fft, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    c["on"], c["pilots"] = on, R.pilot_comb(on, 8)
    receivers = [TP(0, 0), TP(1, 0)] + ([TP(0, 1), TP(1, 1)] if c["S"] >= 3 else [])
    links = [c["composed"][0], L(cfo=0.02, cfo_tracked=0), L(track=2)]
    c["points"] = [q for q in links for _ in receivers]
    c["tracking"] = receivers * len(links)
    return c


def base_seed(name):
    return 100 * (1 + CASES.index(name))


@functools.lru_cache(maxsize=None)
def ref_power(name, seed, frame_offset, frames):
    c = case(name)
    return R.pa_ref_power(c["st"], c["k"], c["S"], c["w_tx"], seed, frame_offset, frames, active=c["active"], mask=c["mask"],
                          gpu=False).astype(np.float32)


def sides(c, seed, frame_offset, frames):
    return dict(tracks=c["tracks"], knot_step=c["knot_step"], aci_active=c["aci_active"],
                ref_power=ref_power(c["name"], seed, frame_offset, frames), active=c["active"], mask=c["mask"],
                noise_before_truncate=c["nbt"])


def head(c, seed, frame_offset, frames):
    return (c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames)


def host(c, seed, frame_offset, frames, points=None, tracking=None, pilots="comb", scales=SCALES):
    """the mirror's profile and its near decisions [points, pairs, n_snr, n_ch]"""
    return R.rx_profile_tracking_host(*head(c, seed, frame_offset, frames), c["points"] if points is None else points,
                                      c["tracking"] if tracking is None else tracking, c["pilots"] if pilots == "comb" else pilots,
                                      scales, with_near=True, **sides(c, seed, frame_offset, frames))


def run_gpu(c, seed, frame_offset, frames, points=None, tracking=None, pilots="comb", scales=SCALES, ref_frames=None, **kw):
    s = sides(c, seed, *((frame_offset, frames) if ref_frames is None else ref_frames))
    return W.rx_profile_tracking_gpu(*head(c, seed, frame_offset, frames), c["points"] if points is None else points,
                                     c["tracking"] if tracking is None else tracking, c["pilots"] if pilots == "comb" else pilots,
                                     scales, **s, **kw)


def run_soft(c, seed, frame_offset, frames, points=None, scales=SCALES):
    return W.rx_profile_soft_gpu(*head(c, seed, frame_offset, frames), c["points"] if points is None else points, scales,
                                 **sides(c, seed, frame_offset, frames))


def pick_seed(c, base, frame_offset=0, frames=RC.FRAMES, tries=32):
    """first seed from base on whose MIRROR profile every point has at most 1 % near decisions (RC.pick_seed's cap)"""
    cells = RC.PAIRS * RC.N_SNR * RC.N_CH
    for seed in range(base, base + tries):
        prof, near = host(c, seed, frame_offset, frames)
        if (near.sum(axis=(1, 2, 3)) <= 0.01 * cells * prof.decisions.sum(axis=-1).astype(np.float64)).all():
            return seed, prof, near
    raise AssertionError("no seed in [%d, %d) keeps the mirror's decisions clear of the thresholds" % (base, base + tries))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, seed, the mirror's profile, its near decisions); computed once, not to be modified"""
    c = case(name)
    seed, prof, near = pick_seed(c, base_seed(name))
    return c, seed, prof, near


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    c, seed, _, _ = reference(name)
    return run_gpu(c, seed, 0, RC.FRAMES)


same_bits = TL.same_bits
pen_ratio = RC.pow_ratio


def check_tracking(prof, ref, near, c, tag):
    """the rules of 2. per point; prints every figure before it asserts; returns the largest ratios (err_power, per symbol,
    bit_penalty, per symbol)"""
    k, S, pil, on = c["k"], c["S"], c["pilots"], c["on"]
    cells = RC.PAIRS * RC.N_SNR * RC.N_CH
    worst = np.zeros(4)
    assert type(prof) is R.RxProfileTracking and prof.bit_err.shape[0] == len(c["points"])
    assert np.array_equal(prof.decisions, ref.decisions) and np.array_equal(prof.decisions_sym, ref.decisions_sym)
    for i, tp in enumerate(c["tracking"]):
        ptag = "%s point %d (%d, %d)" % (tag, i, tp.cpe, tp.post)
        rd = dict(bit=ref.bit_err[i].astype(np.int64), sym=ref.sym_err[i].astype(np.int64), pow=ref.err_power[i], near=near[i],
                  decisions=cells * int(ref.decisions[i].sum()))
        r0 = RC.check_profile(R.RxProfile(prof.bit_err[i], prof.sym_err[i], prof.err_power[i], prof.decisions[i]), rd, c, ptag)
        ds = np.abs(prof.sym_err_sym[i].astype(np.int64) - ref.sym_err_sym[i].astype(np.int64)).sum(axis=-1)
        db = np.abs(prof.bit_err_sym[i].astype(np.int64) - ref.bit_err_sym[i].astype(np.int64)).sum(axis=-1)
        r1 = RC.pow_ratio(prof.err_power_sym[i], ref.err_power_sym[i])
        r2, r3 = pen_ratio(prof.bit_penalty[i], ref.bit_penalty[i]), pen_ratio(prof.bit_penalty_sym[i], ref.bit_penalty_sym[i])
        print("%s: per symbol: sym diff %d, bit diff %d, power ratio %.2e; bit_penalty ratio %.2e, per symbol %.2e"
              % (ptag, ds.sum(), db.sum(), r1, r2, r3))
        assert (ds <= near[i]).all() and (db <= k * near[i]).all(), (ptag, ds, db, near[i])
        assert r1 <= RC.POW_TOL and r2 <= RC.POW_TOL and r3 <= RC.POW_TOL, (ptag, r1, r2, r3)
        assert RC.pow_ratio(prof.pa_power[i], ref.pa_power[i]) <= RC.POW_TOL, ptag
        for a in (prof.bit_err[i], prof.sym_err[i], prof.err_power[i], prof.bit_penalty[i]):
            assert (a[..., pil | ~on] == 0).all(), ptag                   # exact zeros: pilot bins as unloaded ones
        if tp.post:
            for a in (prof.bit_err_sym[i], prof.sym_err_sym[i], prof.err_power_sym[i], prof.bit_penalty_sym[i]):
                assert (a[..., S - 2] == 0).all(), ptag                   # and the postamble
        worst = np.maximum(worst, (r0, r1, r2, r3))
    assert np.isfinite(prof.bit_penalty).all() and (prof.bit_penalty >= 0).all()
    assert np.array_equal(prof.bit_err_sym.sum(axis=-1), prof.bit_err.sum(axis=-1))
    assert np.array_equal(prof.sym_err_sym.sum(axis=-1), prof.sym_err.sum(axis=-1))
    print("%s: largest ratios: err_power %.2e, per symbol %.2e, bit_penalty %.2e, per symbol %.2e" % ((tag,) + tuple(worst)))
    return worst


# ---- 1. the byte identities ----

@pytest.mark.parametrize("name", CASES)
def test_the_one_shot_receiver_is_the_soft_calls_bytes(name):
    c, seed, _, _ = reference(name)
    links = c["points"][::len(c["tracking"]) // 3]
    assert len(links) == 3
    soft = run_soft(c, seed, 0, RC.FRAMES, links)
    none = run_gpu(c, seed, 0, RC.FRAMES, links, [TP()] * 3, None)
    assert type(none) is R.RxProfileTracking and same_bits(none[:10], soft[:10]), name
    assert (none.decisions == soft.decisions[None, :]).all()
    comb = gpu_profile(name)
    pil, data = c["pilots"], c["on"] & ~c["pilots"]
    step = len(c["tracking"]) // 3
    for f in ("bit_err", "sym_err", "err_power", "bit_penalty"):
        got, want = getattr(comb, f)[::step], getattr(soft, f)
        assert same_bits([got[..., data]], [want[..., data]]), (name, f)
        assert (got[..., pil] == 0).all() and (want[..., pil] != 0).any(), (name, f)
    assert same_bits([comb.pa_power[::step]], [soft.pa_power])


# ---- 2. against the mirror ----

@pytest.mark.parametrize("name", CASES)
def test_against_the_mirror(name):
    """Measured on an MI355X: profiles/rx_profile_tracking.txt"""
    c, seed, ref, near = reference(name)
    cells = RC.PAIRS * RC.N_SNR * RC.N_CH
    share = near.sum(axis=(1, 2, 3)) / (cells * ref.decisions.sum(axis=-1).astype(np.float64))
    print("%s seed=%d snr=%s: near decisions per point %s %%" % (name, seed, c["snr"], np.round(100 * share, 2)))
    assert (share <= 0.01).all()
    ser = ref.sym_err.sum(axis=(1, 2, 3, 4)) / (cells * ref.decisions.sum(axis=-1).astype(np.float64))
    print("%s: the mirror's symbol-error rate per point %s" % (name, np.round(ser, 3)))
    check_tracking(gpu_profile(name), ref, near, c, "%s seed=%d" % (name, seed))


# ---- 4. the invariances ----

@pytest.mark.parametrize("name", ("n64_wtx_plain", "n256_cpw_half_masked", OWN))
def test_a_point_and_a_scale_do_not_depend_on_their_neighbours(name):
    c, seed, _, _ = reference(name)
    allp = gpu_profile(name)
    pts, tps = c["points"], c["tracking"]
    last = len(pts) - 1
    for i in (0, 1, last - 1, last):
        alone = run_gpu(c, seed, 0, RC.FRAMES, [pts[i]], [tps[i]])
        assert same_bits(alone[:9], [a[i:i + 1] for a in allp[:9]]), (name, i)
        assert np.array_equal(alone.decisions, allp.decisions[i:i + 1]) and np.array_equal(alone.decisions_sym, allp.decisions_sym[i:i + 1])
    other = run_gpu(c, seed, 0, RC.FRAMES, [pts[last], L(linewidth=0.11), pts[1]], [tps[last], TP(1, 0), tps[1]])
    assert same_bits([a[0] for a in other[:9]], [a[last] for a in allp[:9]])
    assert same_bits([a[2] for a in other[:9]], [a[1] for a in allp[:9]])
    three = run_gpu(c, seed, 0, RC.FRAMES, scales=(0.7, SCALES[2], 0.03))
    one = run_gpu(c, seed, 0, RC.FRAMES, scales=(SCALES[2],))
    assert same_bits(three[:7], one[:7]) and same_bits(three[:7], allp[:7])
    for f in ("bit_penalty", "bit_penalty_sym"):
        mid = np.ascontiguousarray(getattr(three, f)[..., 1, :])
        assert mid.tobytes() == np.ascontiguousarray(getattr(one, f)[..., 0, :]).tobytes(), f
        assert mid.tobytes() == np.ascontiguousarray(getattr(allp, f)[..., 2, :]).tobytes(), f
        assert not np.array_equal(getattr(three, f)[..., 0, :], mid)


def test_repeated_calls_are_identical():
    for name in ("n512_wola_plain", "n64_cp_masked", OWN):
        c, seed, _, _ = reference(name)
        assert same_bits(gpu_profile(name)[:9], run_gpu(c, seed, 0, RC.FRAMES)[:9]), name


def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked"
    c, seed, _, _ = reference(name)
    one = gpu_profile(name)
    a = run_gpu(c, seed, 0, 5, ref_frames=(0, RC.FRAMES))
    both = run_gpu(c, seed, 5, 3, ref_frames=(0, RC.FRAMES), out=a)
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym", "decisions", "decisions_sym"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert (both.bit_penalty >= a.bit_penalty).all() and both.bit_penalty.sum() > a.bit_penalty.sum()
    for f in ("err_power", "err_power_sym", "pa_power", "bit_penalty", "bit_penalty_sym"):
        assert RC.pow_ratio(getattr(both, f), getattr(one, f)) < 1e-12, f
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, RC.FRAMES), scales=(1.0,), out=a)


def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32 (tests/test_gpu_rng_keys.py's pattern)"""
    c = case("n128_cpw_half_nbt0")
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    pts, tps, sc = [c["points"][0], L(cfo=0.02, cfo_tracked=0)], [TP(1, 1), TP(1, 0)], (0.5, 0.1)
    ref = host(c, seed, f0, 8, pts, tps, scales=sc)[0]
    got = run_gpu(c, seed, f0, 8, pts, tps, scales=sc)
    for i in range(2):
        rp, rb = RC.pow_ratio(got.err_power[i], ref.err_power[i]), pen_ratio(got.bit_penalty[i], ref.bit_penalty[i])
        rs = pen_ratio(got.bit_penalty_sym[i], ref.bit_penalty_sym[i])
        print("keys beyond 32 bits, point %d: err_power ratio %.2e, bit_penalty ratio %.2e, per symbol %.2e" % (i, rp, rb, rs))
        assert rp <= RC.POW_TOL and rb <= RC.POW_TOL and rs <= RC.POW_TOL
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    low_seed = run_gpu(c, seed & 0xFFFFFFFF, f0, 8, pts, tps, scales=sc, ref_frames=(f0, 8))
    assert pen_ratio(low_seed.bit_penalty, got.bit_penalty) > 1e-2
    high = run_gpu(c, seed, 2 ** 32, 5, pts, tps, scales=sc, ref_frames=(f0, 8))
    low = run_gpu(c, seed, 0, 5, pts, tps, scales=sc, ref_frames=(f0, 8))
    assert pen_ratio(high.bit_penalty, low.bit_penalty) > 1e-2
    part = run_gpu(c, seed, f0, 3, pts, tps, scales=sc, ref_frames=(f0, 8))
    assert RC.pow_ratio(part.bit_penalty + high.bit_penalty, got.bit_penalty) < 1e-12
    assert np.array_equal(part.bit_err + high.bit_err, got.bit_err)


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two points, two scales: a chunk of the documented budget (the soft call's) ends inside a cell;
    neither the split of the frame range nor another chunking changes a byte -- no mirror here"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    act = CM.half_band_allocation(1024)
    pil = R.pilot_comb(act, 8)
    pts, tps, sc = [L(linewidth=0.01), L(cfo=0.01, cfo_tracked=0)], [TP(1, 1), TP(0, 1)], (0.5, 0.1)
    per_chunk = R.rx_profile_tracking_chunk_frames(st, S, False, 2, False, 2)
    assert per_chunk == R.rx_profile_soft_chunk_frames(st, S, False, 2, False, 2) and 250 < per_chunk
    frames = per_chunk // 2 + 19                                            # 8 cells: four chunks and a bit

    def run(f0, n, points=pts, tracking=tps, scales=sc, **kw):
        return W.rx_profile_tracking_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, f0, n, points, tracking, pil,
                                         scales, active=act, **kw)
    one = run(0, frames)
    assert int(one.decisions.max()) == frames * (S - 2) and (frames * 8) % per_chunk != 0 and frames % per_chunk != 0
    assert R.rx_profile_kernel_ms() > 0.0
    assert (one.bit_err_sym[..., S - 2] == 0).all() and (one.bit_err[..., pil] == 0).all() and (one.bit_err.sum(axis=-1) > 0).all()
    parts = run(frames - 7, 7, out=run(0, frames - 7))
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym", "decisions", "decisions_sym"):
        assert np.array_equal(getattr(parts, f), getattr(one, f)), f
    assert RC.pow_ratio(parts.bit_penalty, one.bit_penalty) < 1e-12 and RC.pow_ratio(parts.err_power, one.err_power) < 1e-12
    # other chunkings of the same frames: one scale, or one point, makes a frame smaller and a chunk longer
    one_scale = R.rx_profile_tracking_chunk_frames(st, S, False, 2, False, 1)
    one_point = R.rx_profile_tracking_chunk_frames(st, S, False, 1, False, 2)
    assert per_chunk < one_scale < one_point and frames % one_scale != 0 and frames % one_point != 0
    alone = run(0, frames, scales=sc[:1])
    assert same_bits(alone[:7], one[:7])
    assert same_bits([a[..., 0, :] for a in alone[7:9]], [a[..., 0, :] for a in one[7:9]])
    alone = run(0, frames, points=pts[1:], tracking=tps[1:])
    assert same_bits(alone[:9], [a[1:] for a in one[:9]])
    assert not np.array_equal(one.bit_penalty[0], one.bit_penalty[1])


def test_tracking_for_window_file_equals_the_direct_calls(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr, B = channels[:2], [8.0, 16.0], st.stride
    pts = [L(), L(TL.RAPP6, None, 2, 0.02, 0, 1e-3, 0, (B // 3, 0.0)), L(cfo=0.02, cfo_tracked=0)]
    tps, sc = [TP(0, 0), TP(1, 1), TP(1, 0)], (0.5, 0.25, 0.05)
    gpu = W.tracking_for_window_file("wtx", 8, win, h, snr, pts, tps, 4, sc, gpu=True, **kw)
    hst = W.tracking_for_window_file("wtx", 8, win, h, snr, pts, tps, 4, sc, gpu=False, **kw)
    assert list(gpu) == list(hst) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    pil = R.pilot_comb(alloc, 4)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        ref = R.pa_ref_power(st, 4, 4, w_tx, 21, 0, 4, active=alloc, mask=mask, gpu=True)
        want = W.rx_profile_tracking_gpu(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, tps, pil, sc, aci_active=~alloc, ref_power=ref,
                                         active=alloc, mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g, hh = gpu[name][key], hst[name][key]
            assert type(g) is R.RxProfileTracking and g.bit_penalty.shape == (3, 2, 2, 3, 64) and g.bit_penalty_sym.shape == (3, 2, 2, 3, 3)
            assert same_bits(g[:9], [a[:, i] for a in want[:9]]), (name, key)
            for f in ("scales", "decisions", "decisions_sym"):
                assert np.array_equal(getattr(g, f), getattr(want, f)) and np.array_equal(getattr(g, f), getattr(hh, f)), f
            assert (g.bit_penalty[..., ~alloc | pil] == 0).all()
            for p in range(3):
                assert pen_ratio(g.bit_penalty[p], hh.bit_penalty[p]) <= RC.POW_TOL
                assert pen_ratio(g.bit_penalty_sym[p], hh.bit_penalty_sym[p]) <= RC.POW_TOL
