"""The fp64 host mirror of ``wofdm_rx_profile_link`` (``frame_profile_link``, ``rx_profile_link_host``) without a GPU: with one
impairment on it is that impairment's own mirror (which the arms' host tests tie to ``frame_profile`` and the CPU oracle) --
integers equal, floats equal or within 1e-12 relative --, an all-off point is ``rx_profile_host``, the walk is read by the clamp
rule of include/wofdm.h, invalid points are refused, and ``link_for_window_file(gpu=False)`` is the host route."""
import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R
from wofdm_amd import timefreq as T

import doppler_cases as DC
import pa_cases as PAC

L = R.LinkPoint
FRAMES = 2
SHAPES = ("n64_wtx_plain", "n128_wrx_half", "n256_cpw_half_masked", "n128_cpw_half_nbt0", "n64_cp_masked")
RAPP3 = R.PaPoint(R.PA_RAPP, 3.0, 2.0)


def same(got, want, tag):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, tag
        if x.dtype == np.uint64:
            assert np.array_equal(x, y), tag
        else:
            assert np.allclose(x, y, rtol=1e-12, atol=0.0), (tag, float(np.abs(x - y).max()))


def sweep(name, seed=5):
    c = PAC.case(name)
    head = (c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, 3, FRAMES)
    kw = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    iact = CM.half_band_allocation(c["st"].n_fft) if c["active"] is None else ~np.asarray(c["active"], bool)
    return c, head, kw, iact, PAC.ref_power(name, seed, 3, FRAMES)


@pytest.mark.parametrize("name", SHAPES)
def test_one_impairment_is_its_own_mirror(name):
    c, head, kw, iact, ref = sweep(name)
    st, B = c["st"], c["st"].stride
    pts = [L(), L(timing=-3, cfo=0.05, cfo_tracked=0), L(timing=2, cfo=-0.3, cfo_tracked=1), L(linewidth=0.02, cpe_tracked=1),
           L(linewidth=0.3, cpe_tracked=0), L(pa=RAPP3), L(pa=R.PaPoint(R.PA_CLIP, 2.0)), L(track=1), L(track=0), L(aci=(B // 3, 10.0)),
           L(pa=R.PaPoint(R.PA_LINEAR, 0.0), track=-1)]
    got, near = R.rx_profile_link_host(*head, pts, tracks=c["tracks"], knot_step=c["knot_step"], aci_active=iact, ref_power=ref,
                                       with_near=True, **kw)
    assert type(got) is R.RxProfileLink and got._fields == R.RxProfilePa._fields
    assert got.bit_err.shape[0] == len(pts) == near.shape[0]
    plain, pnear = R.rx_profile_host(*head, with_near=True, **kw)
    for i in (0, 8, 10):                                               # all off; the static track; a linear amplifier on track -1
        same([a[i] for a in got[:3]], plain[:3], "plain")
        assert np.array_equal(near[i], pnear)
    assert np.array_equal(got.decisions, plain.decisions)
    one = R.rx_profile_sync_host(*head, [(-3, 0.05, 0), (2, -0.3, 1)], **kw)
    same([a[1:3] for a in got[:6]], one[:6], "sync")
    one = R.rx_profile_pn_host(*head, [(0.02, 1), (0.3, 0)], **kw)
    same([a[3:5] for a in got[:6]], one[:6], "pn")
    one = R.rx_profile_pa_host(*head, [RAPP3, (R.PA_CLIP, 2.0)], ref, **kw)
    same([a[5:7] for a in got[:7]], one[:7], "pa")
    one = R.rx_profile_doppler_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["tracks"], c["knot_step"], c["snr"], 5, 3, FRAMES,
                                    **kw)
    same([a[7] for a in got[:6]], [a[1] for a in one[:6]], "doppler")
    same([a[8] for a in got[:6]], [a[0] for a in one[:6]], "doppler, static")
    one = R.rx_profile_aci_host(*head, iact, B // 3, 10.0, **kw)
    same([a[9] for a in got[:3]], one[:3], "aci")
    # without an amplifier the power behind it is the power before it
    for i in (0, 1, 3, 7, 9):
        assert np.array_equal(got.pa_power[i, ..., 0], got.pa_power[i, ..., 1]) and (got.pa_power[i] > 0).all()
    # what no point uses is not needed
    alone = R.rx_profile_link_host(*head, [L(), L(timing=-3, cfo=0.05, cfo_tracked=0)], **kw)
    same([a[:2] for a in alone[:7]], [a[:2] for a in got[:7]], "no side arguments")


def frame_inputs(name, cell=5, frame=11, seed=9):
    c = PAC.case(name)
    st, k, S = c["st"], c["k"], c["S"]
    p, s, ch = cell // 4, (cell // 2) % 2, cell % 2
    on = np.ones(st.n_fft, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    grid = T.qam_table(k)[R.gen_labels(st.n_fft, k, S, seed, cell, frame)] * on[None, :]
    B = st.stride
    lo, hi = -2 * B, st.frame_len(S) + 2 * B
    noise_at = R._noise_lookup(R.gen_noise_at(np.arange(lo, hi), seed, cell, frame), lo)
    walk = R.pn_walk(S * B, seed, cell, frame)
    args = (st, grid, noise_at, c["w_tx"][p], c["w_rx"][p], c["h"][ch])
    kw = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    return c, args, float(c["snr"][s]), walk, kw, (seed, cell, frame, ch)


@pytest.mark.parametrize("name", ("n64_wtx_plain", "n128_cpw_half_nbt0", "n64_cp_masked"))
def test_one_frame_all_off_and_single_stages(name):
    c, args, snr, walk, kw, (seed, cell, frame, ch) = frame_inputs(name)
    st, k, S = c["st"], c["k"], c["S"]
    unit = R.gen_noise(R._noise_len(st, S, c["h"].shape[1], c["nbt"]), seed, cell, frame)
    got = R.frame_profile_link(*args, L(), snr, k, walk, **kw)
    assert len(got) == 9
    same(got[:5], R.frame_profile(st, args[1], unit, *args[3:], snr, k, c["active"], c["mask"], c["nbt"]), "frame_profile")
    q = R.SyncPoint(-4, 0.11, 0)
    same(R.frame_profile_link(*args, L(timing=-4, cfo=0.11, cfo_tracked=0), snr, k, walk, **kw)[:8],
         R.frame_profile_sync(*args, q, snr, k, **kw), "frame_profile_sync")
    same(R.frame_profile_link(*args, L(linewidth=0.05), snr, k, walk, **kw)[:8],
         R.frame_profile_pn(st, args[1], unit, *args[3:], walk, R.PnPoint(0.05, 0), snr, k, **kw), "frame_profile_pn")
    same(R.frame_profile_link(*args, L(pa=RAPP3), snr, k, walk, ref_power=0.9, **kw),
         R.frame_profile_pa(st, args[1], unit, *args[3:], RAPP3, 0.9, snr, k, **kw), "frame_profile_pa")
    tr = c["tracks"][2, ch]
    same(R.frame_profile_link(*args, L(track=0), snr, k, walk, track=tr, knot_step=c["knot_step"], **kw)[:8],
         R.frame_profile_doppler(st, args[1], unit, args[3], args[4], tr, c["knot_step"], snr, k, **kw), "frame_profile_doppler")
    igrid = T.qam_table(k)[R.gen_labels(st.n_fft, k, S + 1, seed, cell, frame, R.STREAM_ACI)]
    same(R.frame_profile_link(*args, L(aci=(7, -2.0)), snr, k, walk, aci_grids=igrid, **kw)[:5],
         R.frame_profile_aci(st, args[1], igrid, unit, *args[3:], None, 7, -2.0, snr, k, **kw), "frame_profile_aci")
    y = R.frame_profile_link(*args, L(), snr, k, walk, with_y=True, **kw)
    assert len(y) == 10 and y[9].shape == (S, st.n_fft)


@pytest.mark.parametrize("tracked", (0, 1))
def test_the_walk_is_read_at_the_clamped_index(tracked):
    """timing != 0, linewidth > 0: a sample at on-air index a outside [0, S B) reads u[clamp(a, 0, S B - 1)], and the tracked
    mean is taken over the same clamped values -- against the rule written out sample by sample"""
    c, args, snr, walk, kw, _ = frame_inputs("n64_wtx_plain")
    st, k, S = c["st"], c["k"], c["S"]
    B, n, delta, gam = st.stride, st.n_fft, st.tail_rx, st.prefix_rm
    beta = np.float32(0.05)
    turn = np.sqrt(float(beta) / (2.0 * np.pi * n))
    assert np.array_equal(R._link_walk_index(np.array([-7, -1, 0, 3, S * B - 1, S * B, S * B + 9]), S * B),
                          [0, 0, 0, 3, S * B - 1, S * B - 1, S * B - 1])
    for theta in (-(gam + 5), 6):
        met = set()

        def phase(a):
            out = np.zeros(a.shape, complex)
            for s in range(a.shape[0]):
                idx = [0 if v < 0 else (S * B - 1 if v > S * B - 1 else int(v)) for v in a[s]]
                met.update(v for v, i in zip(a[s], idx) if v != i)
                u = walk[idx]
                cpe = u[0] + np.mean(u - u[0]) if tracked else 0.0
                out[s] = np.exp(2j * np.pi * (u - cpe) * turn)
            return out
        front = R._sync_front(*args[:4], args[5], snr, c["active"], c["mask"], c["nbt"])
        want = R._sync_point(st, front, args[2], args[4], R.SyncPoint(theta, 0.0, 1), k, None, phase)
        got = R.frame_profile_link(*args, L(timing=theta, linewidth=beta, cpe_tracked=tracked), snr, k, walk, **kw)
        assert met and (min(met) < 0) == (theta < 0) and (max(met) > S * B - 1) == (theta > 0)
        for x, y in zip(got[:8], want[:8]):
            if np.asarray(x).dtype == np.uint64:
                assert np.array_equal(x, y)
            else:
                assert np.allclose(x, y, rtol=1e-9, atol=0.0)
        # and the rule matters: holding another phase outside the frame is another result
        other = np.concatenate([walk[:-1], [walk[-1] + 40.0]]) if theta > 0 else np.concatenate([[walk[0] + 40.0], walk[1:]])
        assert not np.allclose(R.frame_profile_link(*args, L(timing=theta, linewidth=beta, cpe_tracked=tracked), snr, k, other, **kw)[2],
                               got[2], rtol=1e-6)
    # at timing 0 the clamp is never met: the largest index read is S B - 1
    a = (np.arange(S) * B + gam)[:, None] + np.arange(n + delta)[None, :]
    assert a.min() >= 0 and a.max() == S * B - 1


def test_invalid_points_are_refused():
    c, head, kw, iact, ref = sweep("n64_wtx_plain")
    B = c["st"].stride
    side = dict(tracks=c["tracks"], knot_step=c["knot_step"], aci_active=iact, ref_power=ref, **kw)
    for bad in (L(timing=B), L(timing=-B), L(cfo=4.5), L(cfo_tracked=2), L(linewidth=-0.1), L(linewidth=1.5), L(cpe_tracked=3),
                L(track=3), L(track=-2), L(aci=(B, 0.0)), L(aci=(-1, 0.0)), L(aci=(3, np.inf)), L(pa=R.PaPoint(7, 0.0)),
                L(pa=R.PaPoint(R.PA_RAPP, 61.0)), L(pa=R.PaPoint(R.PA_RAPP, 3.0, 0.1))):
        with pytest.raises(ValueError):
            R.rx_profile_link_host(*head, [L(), bad], **side)
    with pytest.raises(ValueError):
        R.rx_profile_link_host(*head, [], **side)
    for point, missing in ((L(track=0), "tracks"), (L(aci=(3, 0.0)), "aci_active"), (L(pa=RAPP3), "ref_power")):
        with pytest.raises(ValueError):
            R.rx_profile_link_host(*head, [point], **{k: v for k, v in side.items() if k != missing})
    with pytest.raises(ValueError):
        R.rx_profile_link_host(*head, [L()], **dict(side, tracks=c["tracks"][:, :1]))
    # every field defaults to "off", and tuples in the fields' order are points
    assert L() == (None, None, 0, 0.0, 1, 0.0, 0, None)
    a = R.rx_profile_link_host(*head, [(RAPP3, 1, 2, 0.02, 1, 1e-3, 1, (5, 0.0))], **side)
    b = R.rx_profile_link_host(*head, [L(RAPP3, 1, 2, 0.02, 1, 1e-3, 1, (5, 0.0))], **side)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_chunk_frames_is_the_headers_formula():
    st, S = W.make_structure("CPW", 256, 32), 16
    P, B = st.sym_len, st.stride
    Tv = st.tail_tx + S * B
    for masked in (False, True):
        base = 8 * (S * 256 + Tv + (S * (2 * P - 1) if masked else 0))
        for n_points in (1, 4, 16):
            per = base + 8 * n_points * (256 + S + Tv) + 8 * S * B
            assert R.rx_profile_link_chunk_frames(st, S, masked, n_points, False) == min(65535, (256 << 20) // per)
            per += 8 * ((S + 1) * 256 + Tv + B + ((S + 1) * (2 * P - 1) if masked else 0))
            assert R.rx_profile_link_chunk_frames(st, S, masked, n_points, True) == min(65535, (256 << 20) // per)
    assert R.rx_profile_link_chunk_frames(st, S, False, 1, False) < R.rx_profile_pa_chunk_frames(st, S, False, 1)


def test_link_for_window_file_on_the_host(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=3, seed=21)
    h, snr, B = channels[:2], [8.0, 16.0], st.stride
    tracks = DC.tracks_of(dict(st=st, h=np.asarray(h, np.complex64)), (0.01,), B, 6)
    pts = [L(), L(R.PaPoint(R.PA_RAPP, 6.0), 0, 2, 0.02, 1, 1e-3, 1, (B // 3, 0.0)), L(aci=(5, 3.0))]
    got = W.link_for_window_file("wtx", 8, win, h, snr, pts, tracks=tracks, knot_step=B, gpu=False, **kw)
    assert list(got) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    plain = W.profile_for_window_file("wtx", 8, win, h, snr, gpu=False, **kw)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        ref = R.pa_ref_power(st, 4, 4, w_tx, 21, 0, 3, active=alloc, mask=mask, gpu=False)
        want = R.rx_profile_link_host(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 3, pts, tracks=tracks, knot_step=B, aci_active=~alloc,
                                      ref_power=ref, active=alloc, mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g = got[name][key]
            assert type(g) is R.RxProfileLink and g.bit_err.shape == (3, 2, 2, 64) and g.pa_power.shape == (3, 2, 2, 2)
            for x, y in zip(g[:-1], want[:-1]):
                assert np.array_equal(x, y[:, i])
            assert np.array_equal(g.decisions, want.decisions)
            same([g.bit_err[0], g.sym_err[0], g.err_power[0]], plain[name][key][:3], "the all-off point")
