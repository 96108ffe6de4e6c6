"""The fp64 host mirror of ``wofdm_rx_profile_soft`` (``bit_llrs``, ``soft_penalties``, ``frame_profile_soft``,
``rx_profile_soft_host``) without a GPU, on the shapes n64_wtx_plain and n64_cp_masked of tests/doppler_cases.py, 8 frames:

- its hard fields are ``rx_profile_host``'s for the all-off point and ``rx_profile_link_host``'s for composed points;
- the count of wrongly signed metrics, (1 - 2 b_i) Lambda_i < 0, is the mirror's bit errors, for k = 2, 4, 6;
- for the plain point the penalties recomputed from the ORACLE's dump (Xhat, Y, gain and the frame's unit noise) agree with the
  mirror's to 1e-9 relative on every cell's totals (fp64 against fp64, the margin by which the other host tests tie mirrors to the
  oracle);
- ``bit_llrs`` (brute force over the constellation) against a separable per-axis restatement: 1e-12 (1 + |e|^2);
- the rate at the best scale lies in (0, k] and does not fall from the lower to the higher SNR point of a case, for the points
  whose matched scale the default list covers (the test says which, and why the everything-on point of the full-band case is not
  one); at most k for every point."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R
from wofdm_amd import timefreq as T

import pa_cases as PAC
import rx_profile_cases as RC

L = R.LinkPoint
SHAPES = ("n64_wtx_plain", "n64_cp_masked")
FRAMES = RC.FRAMES
SEED = 31
SCALES = (1.0, 0.5, 0.2, 0.05)
RAPP6 = R.PaPoint(R.PA_RAPP, 6.0, 2.0)


def composed(c):
    B = c["st"].stride
    return [L(), L(RAPP6, 2, 2, 0.02, 1, 1e-3, 1, (B // 3, 0.0)), L(track=1, linewidth=1e-3, cpe_tracked=1)]


def sides(c, name):
    iact = CM.half_band_allocation(c["st"].n_fft) if c["active"] is None else ~np.asarray(c["active"], bool)
    return dict(tracks=c["tracks"], knot_step=c["knot_step"], aci_active=iact, ref_power=PAC.ref_power(name, SEED, 0, FRAMES),
                active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])


@functools.lru_cache(maxsize=None)
def soft_host(name):
    """the mirror's soft profile of the case's composed points, default scales; computed once, not to be modified"""
    c = PAC.case(name)
    head = (c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], SEED, 0, FRAMES)
    return c, head, R.rx_profile_soft_host(*head, composed(c), **sides(c, name))


@pytest.mark.parametrize("name", SHAPES)
def test_hard_fields_are_the_link_mirrors_and_the_plain_mirrors(name):
    c, head, got = soft_host(name)
    assert type(got) is R.RxProfileSoft and got._fields[:7] == R.RxProfileLink._fields[:7] and got._fields[-1] == "decisions"
    n, S, ns = c["st"].n_fft, c["S"], len(R.SOFT_SCALES)
    assert got.bit_penalty.shape == (3, RC.PAIRS, RC.N_SNR, RC.N_CH, ns, n)
    assert got.bit_penalty_sym.shape == (3, RC.PAIRS, RC.N_SNR, RC.N_CH, ns, S - 1)
    assert got.scales.dtype == np.float32 and np.allclose(got.scales, [2.0 ** (1 - j / 2) for j in range(16)], rtol=1e-7)
    link = R.rx_profile_link_host(*head, composed(c), **sides(c, name))
    for f in R.RxProfileLink._fields:
        assert np.array_equal(getattr(got, f), getattr(link, f)), f
    plain = R.rx_profile_host(*head, active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    for f in ("bit_err", "sym_err", "decisions"):
        assert np.array_equal(getattr(got, f)[0] if f != "decisions" else got.decisions, getattr(plain, f)), f
    assert np.allclose(got.err_power[0], plain.err_power, rtol=1e-12, atol=0.0)
    # points=None is one all-off point; another scale list is the same sums at those scales
    one = R.rx_profile_soft_host(*head[:-1], 2, scales=SCALES, active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    two = R.rx_profile_soft_host(*head[:-1], 2, [L()], (0.5,), active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    assert one.bit_err.shape[0] == 1 and np.array_equal(one.bit_penalty[..., 1, :], two.bit_penalty[..., 0, :])
    # the symbols' sums and the bins' sums are the same decisions; unloaded bins are exactly 0
    assert np.allclose(got.bit_penalty.sum(axis=-1), got.bit_penalty_sym.sum(axis=-1), rtol=1e-12)
    on = np.ones(n, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    assert (got.bit_penalty[..., ~on] == 0).all() and (got.bit_penalty[..., on] > 0).all()


def frame_inputs(name, k, cell=5, frame=3):
    c = dict(PAC.case(name), k=k)
    st, S = c["st"], c["S"]
    p, s, ch = cell // 4, (cell // 2) % 2, cell % 2
    on = np.ones(st.n_fft, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    grid = T.qam_table(k)[R.gen_labels(st.n_fft, k, S, SEED, cell, frame)] * on[None, :]
    B = st.stride
    lo, hi = -2 * B, st.frame_len(S) + 2 * B
    noise_at = R._noise_lookup(R.gen_noise_at(np.arange(lo, hi), SEED, cell, frame), lo)
    walk = R.pn_walk(S * B, SEED, cell, frame)
    args = (st, grid, noise_at, c["w_tx"][p], c["w_rx"][p], c["h"][ch])
    kw = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    return c, args, float(c["snr"][s]), walk, kw, on, (p, s, ch)


@pytest.mark.parametrize("k", (2, 4, 6))
@pytest.mark.parametrize("name", SHAPES)
def test_wrongly_signed_metrics_are_the_bit_errors(name, k):
    for cell in (1, 5):
        c, args, snr, walk, kw, on, (p, s, ch) = frame_inputs(name, k, cell)
        st, S = c["st"], c["S"]
        B = st.stride
        for point, extra in ((L(), {}), (L(timing=2, cfo=0.02, linewidth=1e-3, cpe_tracked=1, track=0),
                                         dict(track=c["tracks"][1, ch], knot_step=c["knot_step"]))):
            out = R.frame_profile_soft(*args, point, snr, k, walk, SCALES, **extra, **kw)
            assert len(out) == 12
            bit, xhat, nu, bpen, spen = out[0], out[3], out[9], out[10], out[11]
            assert nu.shape == (st.n_fft,) and (nu[on] > 0).all() and (nu[~on] == 0).all()
            assert bpen.shape == (len(SCALES), st.n_fft) and spen.shape == (len(SCALES), S - 1)
            X = args[1][1:]
            lab = R.slice_labels(k, X)
            sign = np.stack([1.0 - 2.0 * ((lab >> (k - 1 - i)) & 1) for i in range(k)], axis=-1)
            lam = R.bit_llrs(k, xhat, np.where(on, nu, 1.0)[None, :])
            wrong = ((sign * lam < 0) & on[None, :, None]).sum(axis=(0, 2))
            assert np.array_equal(wrong.astype(np.uint64), bit), (name, k, cell)
            assert bit.sum() > 0 or snr > 15.0
            # the sign of the metric is the slicer's bit
            rx = R.slice_labels(k, xhat)
            for i in range(k):
                assert np.array_equal((lam[..., i] < 0)[:, on], (((rx >> (k - 1 - i)) & 1) != 0)[:, on])
            # the penalties are the sums of soft_penalties, and every scale's symbols add up to its bins
            pen = R.soft_penalties(k, X, xhat, nu, np.asarray(SCALES, np.float32), on)       # (the scales as the library stores them)
            assert np.array_equal(pen.sum(axis=1), bpen) and np.array_equal(pen.sum(axis=2), spen)
            assert np.allclose(bpen.sum(axis=-1), spen.sum(axis=-1), rtol=1e-12)
            # the first nine outputs are frame_profile_link's
            linkout = R.frame_profile_link(*args, point, snr, k, walk, **extra, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(out[:9], linkout))
            assert R.frame_profile_soft(*args, point, snr, k, walk, SCALES, with_y=True, **extra, **kw)[12].shape == (S, st.n_fft)


def separable_llrs(k, e):
    """the kernel's form written out on the host: per axis the squared distances to the levels, split by the bit of the
    level's Gray index; the other axis' distance is common to both minima and is left out"""
    hb = k // 2
    m = 1 << hb
    a = np.sqrt(2.0 * (m * m - 1) / 3.0)
    e = np.asarray(e, np.complex128)
    out = np.empty(e.shape + (k,))
    for ax, u in enumerate((e.real * a, -e.imag * a)):
        lv = np.arange(m)
        d = (u[..., None] - (2.0 * lv - (m - 1))) ** 2 / (a * a)
        gray = lv ^ (lv >> 1)
        for i in range(hb):
            one = ((gray >> (hb - 1 - i)) & 1) != 0
            out[..., ax * hb + i] = d[..., one].min(axis=-1) - d[..., ~one].min(axis=-1)
    return out


@pytest.mark.parametrize("k", (2, 4, 6))
def test_bit_llrs_against_the_separable_form(k):
    rs = np.random.RandomState(k)
    e = np.concatenate([1.5 * (rs.randn(4000) + 1j * rs.randn(4000)), T.qam_table(k), 40.0 * (rs.randn(50) + 1j * rs.randn(50))])
    got, want = R.bit_llrs(k, e), separable_llrs(k, e)
    assert got.shape == (e.size, k)
    assert (np.abs(got - want) <= 1e-12 * (1.0 + np.abs(e) ** 2)[:, None]).all()
    # on a constellation point every metric has the sign of the point's own bit and the size of a squared half distance at least
    lab = np.arange(1 << k)
    own = R.bit_llrs(k, T.qam_table(k))
    for i in range(k):
        assert ((own[:, i] < 0) == (((lab >> (k - 1 - i)) & 1) != 0)).all()
    assert np.allclose(R.bit_llrs(k, e, 0.25), 4.0 * got) and R.bit_llrs(k, e.reshape(2, -1)).shape == (2, e.size // 2, k)


@pytest.mark.parametrize("name", SHAPES)
def test_plain_point_penalties_from_the_oracles_dump(name):
    """the all-off point: Xhat, Y and the noise gain from the CPU oracle's dump, v = gain^2 mean |unit noise|^2 over the samples
    the power pass reads, nu = |X_0 / Y_0|^2 v W2, the penalties by the formula written out here"""
    c = PAC.case(name)
    st, k, S, n = c["st"], c["k"], c["S"], c["st"].n_fft
    osys = RC.oracle_sys(c)
    on = np.ones(n, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    sc = np.asarray(SCALES, np.float32).astype(np.float64)
    cells = RC.PAIRS * RC.N_SNR * RC.N_CH
    want_b, want_s = np.zeros((cells, sc.size, n)), np.zeros((cells, sc.size, S - 1))
    nl = O.noise_len(osys) if c["nbt"] else S * st.stride
    for cell in range(cells):
        p, s, ch = cell // 4, (cell // 2) % 2, cell % 2
        w2 = float((c["w_rx"][p].astype(np.float64) ** 2).sum())
        for f in range(FRAMES):
            lab, noise = O.gen_labels(osys, SEED, cell, f), O.gen_noise(osys, SEED, cell, f)
            _, d = O.frame(osys, c["w_tx"][p].astype(np.float64), c["w_rx"][p].astype(np.float64), c["h"][ch].astype(np.complex128),
                           float(c["snr"][s]), lab, noise, dump=True)
            v = float(d["gain"][0]) ** 2 * np.mean(np.abs(noise[:nl]) ** 2)
            nu = np.abs(d["X"][0, on] / d["Y"][0, on]) ** 2 * v * w2
            tab = T.qam_table(k)
            dist = np.abs(d["Xhat"][:, on, None] - tab) ** 2
            pen = np.zeros((sc.size, S - 1, int(on.sum())))
            for i in range(k):
                one = ((np.arange(1 << k) >> (k - 1 - i)) & 1) != 0
                lam = (dist[..., one].min(axis=-1) - dist[..., ~one].min(axis=-1)) / nu[None, :]
                z = sc[:, None, None] * (1.0 - 2.0 * ((lab[1:, on] >> (k - 1 - i)) & 1)) * lam
                pen += np.logaddexp(0.0, -z) / np.log(2.0)
            want_b[cell][:, on] += pen.sum(axis=1)
            want_s[cell] += pen.sum(axis=2)
    got = R.rx_profile_soft_host(st, k, S, c["w_tx"], c["w_rx"], c["h"], c["snr"], SEED, 0, FRAMES, scales=SCALES, active=c["active"],
                                 mask=c["mask"], noise_before_truncate=c["nbt"])
    shp = (RC.PAIRS, RC.N_SNR, RC.N_CH)
    gb, gs = got.bit_penalty[0].reshape((cells,) + want_b.shape[1:]), got.bit_penalty_sym[0].reshape((cells,) + want_s.shape[1:])
    assert got.bit_penalty[0].shape == shp + (sc.size, n)
    rel_b = np.abs(gb.sum(axis=-1) - want_b.sum(axis=-1)) / want_b.sum(axis=-1)
    rel_s = np.abs(gs.sum(axis=-1) - want_s.sum(axis=-1)) / want_s.sum(axis=-1)
    print("%s: cell totals against the oracle's dump: bins %.2e, symbols %.2e" % (name, rel_b.max(), rel_s.max()))
    assert (want_b.sum(axis=-1) > 0).all() and rel_b.max() <= 1e-9 and rel_s.max() <= 1e-9
    assert RC.pow_ratio(gb, want_b) <= 1e-9


@pytest.mark.parametrize("name", SHAPES)
def test_rate_lies_in_zero_k_and_grows_with_the_snr(name):
    c, head, got = soft_host(name)
    k, n, S = c["k"], c["st"].n_fft, c["S"]
    on = got.decisions > 0
    rb, ib = R.gmi_per_bin(got, k)
    assert rb.shape == got.bit_err.shape and ib.shape == rb.shape and np.isnan(rb[..., ~on]).all() and (ib[..., ~on] == 0).all()
    rs_, is_ = R.gmi_per_symbol(got, k)
    assert rs_.shape == got.bit_err_sym.shape and is_.shape == rs_.shape
    r1, i1 = R.gmi(got, k)
    r0, i0 = R.gmi(got, k, per_bin_scale=False)
    assert r1.shape == r0.shape == i0.shape == got.bit_err.shape[:-1] and i1.shape == rb.shape
    print("%s: rate per point and SNR point (best scale per bin) %s, (one scale per cell) %s, scales %s"
          % (name, np.round(r1.mean(axis=(1, 3)), 3), np.round(r0.mean(axis=(1, 3)), 3), got.scales[i0].mean(axis=(1, 3))))
    # Points 0 and 2 (all off; a moving channel with phase noise): the disturbance the receiver does not model is small against
    # the noise it does, the matched scale lies inside the list, and the rate is positive and grows with the SNR.  Point 1 has
    # the neighbour at 0 dB -- on the full band of n64_cp_masked it sits ON the victim's bins, a signal-to-interference ratio of 0
    # dB that the assumed noise variance knows nothing of: the matched scale, about 10^(-SNR / 10), lies below the list's smallest
    # 0.011, and k - penalty / decisions at a scale that large is negative.  That is the formula's value, not a defect: only the
    # upper bound holds for every scale.
    for r in (r1, r0):
        assert (r <= k).all()
        assert (r[[0, 2]] > 0).all()
        assert (r[[0, 2]][:, :, 1] >= r[[0, 2]][:, :, 0]).all()         # the higher SNR point carries no less, cell by cell
    # a scale per bin can only gain on one scale per cell, and the all-off point carries more than the everything-on point
    assert (r1 >= r0 - 1e-12).all() and (r1[0] >= r1[1]).all()
    # by hand: the rate of a scale is k less the penalty per decision, and the helpers take the maximum over the scales
    dec = got.decisions.astype(np.float64)
    by_hand = (k - got.bit_penalty[..., on] / dec[on]).max(axis=-2)
    assert np.allclose(rb[..., on], by_hand, rtol=0, atol=1e-15)
    per_sym = (k - got.bit_penalty_sym / (FRAMES * on.sum())).max(axis=-2)
    assert np.allclose(rs_, per_sym, rtol=0, atol=1e-12)
    assert np.allclose(r0, (k - got.bit_penalty.sum(axis=-1) / dec.sum()).max(axis=-1), rtol=0, atol=1e-12)
    # the best scale is inside the default list, not at its ends, for the cells' totals
    assert (i0[[0, 2]] > 0).all() and (i0[[0, 2]] < len(R.SOFT_SCALES) - 1).all()


def test_scales_and_chunks():
    c = PAC.case("n64_wtx_plain")
    head = (c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], SEED, 0, 1)
    for bad in ((), (0.0,), (-1.0,), (np.nan,), (np.inf, 1.0), tuple([1.0] * 17)):
        with pytest.raises(ValueError):
            R.rx_profile_soft_host(*head, scales=bad)
    assert _lib.SOFT_MAX_SCALES == 16 == len(R.SOFT_SCALES)
    st, S = W.make_structure("CPW", 256, 32), 16
    for masked in (False, True):
        for n_points, nb, ns in ((1, False, 1), (4, True, 16), (16, False, 8)):
            link = (256 << 20) / R.rx_profile_link_chunk_frames(st, S, masked, n_points, nb)        # bytes of a frame, about
            got = R.rx_profile_soft_chunk_frames(st, S, masked, n_points, nb, ns)
            P, B = st.sym_len, st.stride
            Tv = st.tail_tx + S * B
            per = 8 * (S * 256 + Tv + (S * (2 * P - 1) if masked else 0)) + 8 * n_points * (256 + S + Tv) + 8 * S * B
            per += 8 * ((S + 1) * 256 + Tv + B + ((S + 1) * (2 * P - 1) if masked else 0)) if nb else 0
            per += 4 * n_points * ns * ((S - 1) * 256 + S)
            assert got == min(65535, (256 << 20) // per) and per > link * 0.99


def test_soft_for_window_file_on_the_host(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=2, seed=21)
    h, snr, B = channels[:2], [8.0, 16.0], st.stride
    pts = [L(), L(R.PaPoint(R.PA_RAPP, 6.0), None, 2, 0.02, 1, 1e-3, 1, (B // 3, 0.0))]
    got = W.soft_for_window_file("wtx", 8, win, h, snr, pts, SCALES, gpu=False, **kw)
    link = W.link_for_window_file("wtx", 8, win, h, snr, pts, gpu=False, **kw)
    assert list(got) == ["opt", "rc"]
    for name in got:
        for key in ("profile", "profile_masked"):
            g = got[name][key]
            assert type(g) is R.RxProfileSoft and g.bit_penalty.shape == (2, 2, 2, 4, 64) and g.bit_penalty_sym.shape == (2, 2, 2, 4, 3)
            assert np.array_equal(g.scales, np.asarray(SCALES, np.float32))
            for f in R.RxProfileLink._fields:
                assert np.array_equal(getattr(g, f), getattr(link[name][key], f)), f
            assert (R.gmi(g, 4)[0] > 0).all()
    assert W.soft_for_window_file("wtx", 8, win, h, snr, gpu=False, **kw)["rc"]["profile"].bit_penalty.shape == (1, 2, 2, 16, 64)
