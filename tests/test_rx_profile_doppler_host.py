"""``wofdm_rx_profile_doppler`` without a GPU: header, binding and exports; every argument check through the C ABI (they all
come before the device is touched); the time-varying convolution ``tv_conv`` against a literal double loop, ``np.convolve``
and the two-knot identity; the fp64 mirror ``frame_profile_doppler`` on a static track against ``frame_profile`` (which
tests/test_rx_profile_host.py ties to the CPU oracle); the channel tracks of ``channels.gen_chan_track`` /
``gen_channel_tracks`` against ``gen_chan`` / ``gen_channel_file``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import channels as CH
from wofdm_amd import rx_profile as R
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

import doppler_cases as DC
import rx_profile_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_U, POISON_F = 0xA5A5A5A5A5A5A5A5, -12345.678


# ---- header, binding, exports ----

def test_rx_profile_doppler_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_doppler\((.*?)\);", hdr, flags=re.M | re.S)
    assert m
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["const wofdm_cfg *cfg", "int device", "const float *w_tx", "const float *w_rx", "const float *h_track",
                    "int32_t n_tracks", "int32_t n_knots", "int32_t knot_step", "const float *snr_db", "const uint8_t *active",
                    "const float *tx_mask", "uint64_t *errs", "double *err_power", "uint64_t *sym_errs", "double *sym_power"]
    assert re.search(r"^#define WOFDM_DOPPLER_MAX_TRACKS 16$", hdr, flags=re.M) and _lib.DOPPLER_MAX_TRACKS == 16
    assert re.search(r"^#define WOFDM_DOPPLER_MAX_KNOTS  64$", hdr, flags=re.M) and _lib.DOPPLER_MAX_KNOTS == 64
    lib = _lib.load()
    at = lib.wofdm_rx_profile_doppler.argtypes
    assert len(at) == len(args) and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    assert at[5] == at[6] == at[7] == C.c_int32
    assert all(t == C.c_void_p for i, t in enumerate(at) if i >= 2 and i not in (5, 6, 7))
    assert "wofdm_rx_profile_doppler" in _lib.EXPORTS and hasattr(lib, "wofdm_rx_profile_doppler")
    kms = hdr[hdr.index("/* *ms = milliseconds (HIP events) the kernels of the calling thread's last successful wofdm_rx_profile or"):
              hdr.index("int wofdm_rx_profile_kernel_ms")]
    assert "wofdm_rx_profile_doppler call" in kms
    doc = hdr[hdr.index("/* wofdm_rx_profile over channels that MOVE"):hdr.index("#define WOFDM_DOPPLER_MAX_TRACKS")]
    for text in ("min(a div knot_step, n_knots - 2)", "f = (a - q knot_step) / knot_step", "K[q][l] + f (K[q+1][l] - K[q][l])",
                 "OUTPUT sample's time", "8 (S n_fft + T + [mask] S (2P-1)) + 8 n_tracks (n_fft + S)",
                 "(n_knots - 1) knot_step < tail_tx + S B + n_taps - 2"):
        assert text in doc, text
    for name in ("tv_conv", "frame_profile_doppler", "rx_profile_doppler_host", "rx_profile_doppler_gpu",
                 "rx_profile_doppler_chunk_frames", "doppler_for_window_file"):
        assert hasattr(W, name), name
    assert hasattr(W.channels, "gen_chan_track") and hasattr(W.channels, "gen_channel_tracks")


def test_chunk_formula_of_the_header():
    for st, S, masked, tracks in ((V.make_structure("wtx", 1024, 56), 16, False, 2), (V.make_structure("CPW", 256, 32), 16, True, 4),
                                  (V.make_structure("wrx", 64, 8), 2, True, 16), (V.make_structure("CP", 64, 16), 2, False, 1)):
        P, N = st.sym_len, st.n_fft
        Tv = st.tail_tx + S * (P - st.tail_tx)
        per = 8 * (S * N + Tv + (S * (2 * P - 1) if masked else 0)) + 8 * tracks * (N + S)
        assert R.rx_profile_doppler_chunk_frames(st, S, masked, tracks) == min(65535, (256 << 20) // per)
        assert R.rx_profile_doppler_chunk_frames(st, S, masked, tracks) == R.rx_profile_sync_chunk_frames(st, S, masked, tracks)


# ---- argument checks without a device ----

def _call(st=None, k=4, S=4, n_taps=3, n_ch=2, n_snr=2, pairs=2, frames=3, device=99, null=(), mask=False, active=None,
          n_tracks=2, n_knots=None, knot_step=None, held=None, edit=None, cfg_edit=None):
    """rc of one call on small arrays; `edit` changes the arrays, `cfg_edit` the cfg, before the call; `held`: (tracks, knots) the
    track array holds, where the counts passed are not to be believed"""
    st = V.make_structure("CPW", 128, 32) if st is None else st
    cfg = W.make_cfg(st, k, S, n_taps, n_ch, n_snr, pairs, seed=3, frames_per_cell=frames)
    P, NW, N = st.sym_len, st.n_fft + st.tail_rx, st.n_fft
    knot_step = st.stride if knot_step is None else knot_step
    n_knots = S + 2 if n_knots is None else n_knots
    ht, hk = (max(1, n_tracks), max(2, n_knots)) if held is None else held
    a = dict(w_tx=np.ones((pairs, P), np.float32), w_rx=np.ones((pairs, NW), np.float32),
             h_track=np.ones((ht, n_ch, hk, n_taps, 2), np.float32), snr=np.full(n_snr, 10.0, np.float32),
             active=None if active is None else np.ascontiguousarray(active, np.uint8),
             mask=np.ones(2 * P - 1, np.float32) if mask else None)
    cells = pairs * n_ch * n_snr
    errs = np.full((ht, cells, N, 2), POISON_U, np.uint64)
    pw = np.full((ht, cells, N), POISON_F, np.float64)
    serrs = np.full((ht, cells, max(1, S - 1), 2), POISON_U, np.uint64)
    spw = np.full((ht, cells, max(1, S - 1)), POISON_F, np.float64)
    a.update(errs=errs, pw=pw, serrs=serrs, spw=spw)
    if edit:
        edit(a)
    if cfg_edit:
        cfg_edit(cfg)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_doppler(None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"],
                                              ptr["h_track"], n_tracks, n_knots, knot_step, ptr["snr"], ptr["active"], ptr["mask"],
                                              ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"])
    assert (errs == POISON_U).all() and (pw == POISON_F).all()          # no failed call writes its outputs
    assert (serrs == POISON_U).all() and (spw == POISON_F).all()
    return rc


def _set(name, index, value):
    def edit(a):
        a[name].reshape(-1)[index] = value
    return edit


def _last():
    return _lib.load().wofdm_last_error().decode()


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _last()
    assert _call(device=-1) == -3
    assert _call(mask=True, active=CM.half_band_allocation(128)) == -3
    assert _call(n_tracks=1) == -3 and _call(n_tracks=16) == -3 and _call(n_knots=64) == -3
    st = V.make_structure("CPW", 128, 32)
    last = st.tail_tx + 4 * st.stride + 3 - 2                               # T + n_taps - 2: the last sample of conv
    assert _call(n_knots=2, knot_step=last) == -3                           # the limit itself is inside
    assert _call(n_knots=2, knot_step=2 ** 31 - 1) == -3
    assert _call(n_knots=64, knot_step=(last + 62) // 63) == -3
    assert _call(st=V.make_structure("wtx", 1024, 128), S=2, mask=True, knot_step=37, n_knots=64) == -3
    assert _call(st=V.make_structure("wtx", 1024, 56), S=16) == -3
    assert _call(n_taps=21) == -3 and _call(S=16) == -3 and _call(S=2) == -3
    assert _call(frames=0) == -3
    for name in ("pw", "serrs", "spw"):                                     # three of the outputs are optional
        assert _call(null=(name,)) == -3, name
    assert _call(null=("pw", "serrs", "spw")) == -3


def test_rx_profile_doppler_refuses_invalid_arguments():
    for name in ("cfg", "w_tx", "w_rx", "h_track", "snr", "errs"):
        assert _call(null=(name,)) == -1, name
    for n in (0, -1, -(2 ** 31)):
        assert _call(n_tracks=n) == -1 and "n_tracks" in _last()
        assert _call(knot_step=n) == -1 and "knot_step" in _last()
    for n in (1, 0, -1, -(2 ** 31)):
        assert _call(n_knots=n) == -1 and "n_knots" in _last()
    for bad in (np.nan, np.inf, -np.inf):
        for index in (0, 7, -1):                                           # the first knot, one inside, the last track's last
            assert _call(edit=_set("h_track", index, bad)) == -1 and "knots must be finite" in _last()
        for name in ("w_tx", "w_rx", "snr"):                               # the checks of wofdm_rx_profile
            assert _call(edit=_set(name, -1, bad)) == -1, name
        assert _call(mask=True, edit=_set("mask", -1, bad)) == -1
    # a track that does not cover the frame
    st = V.make_structure("CPW", 128, 32)
    last = st.tail_tx + 4 * st.stride + 3 - 2
    assert _call(n_knots=2, knot_step=last - 1) == -1 and "knots end at sample" in _last()
    assert _call(n_knots=5) == -1 and _call(n_knots=6) == -3               # S + 1 knots a stride apart end before the tail
    assert _call(n_knots=64, knot_step=(last + 62) // 63 - 1) == -1
    assert _call(n_knots=2, n_taps=21, knot_step=last + 18) == -3 and _call(n_knots=2, n_taps=21, knot_step=last + 17) == -1
    assert _call(active=np.zeros(128, np.uint8)) == -1 and "loads no subcarrier" in _last()
    for field in ("n_channels", "n_snr", "n_window_pairs"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, 0)) == -1, field
    for field in ("cp", "cs", "tail_tx", "prefix_rm", "circ_shift", "n_taps"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, -1)) == -1, field


def test_rx_profile_doppler_refuses_what_lies_outside_its_limits():
    for n in (17, 64, 2 ** 31 - 1):
        assert _call(n_tracks=n, held=(1, 6)) == -2 and "n_tracks" in _last(), n
    for n in (65, 1000, 2 ** 31 - 1):
        assert _call(n_knots=n, held=(2, 6)) == -2 and "n_knots" in _last(), n
    for n in (32, 96, 2048):
        assert _call(cfg_edit=lambda c, n=n: setattr(c, "n_fft", n)) == -2, n
    for k in (1, 3, 8):
        assert _call(k=k) == -2, k
    for S in (1, 17):
        assert _call(S=S) == -2, S
    assert _call(n_taps=22) == -2
    assert _call(cfg_edit=lambda c: (setattr(c, "tail_rx", 11), setattr(c, "prefix_rm", c.prefix_rm - 1))) == -2
    assert _call(cfg_edit=lambda c: setattr(c, "prefix_rm", c.prefix_rm + 1)) == -2
    pmax = (8 * 128 + 2) // 3
    over = V.Structure("wrx", 128, 128, 0, 0, pmax + 1 - 256, pmax + 1 - 128, 0)
    assert _call(st=over, mask=True) == -2 and _call(st=over) == -3
    assert _call(cfg_edit=lambda c: (setattr(c, "n_channels", 1 << 14), setattr(c, "n_snr", 1 << 14)), held=(2, 6)) == -2


# ---- the time-varying convolution ----

def _literal(track, ks, x):
    K, x = np.asarray(track, np.complex128), np.asarray(x, np.complex128)
    out = np.zeros(x.size + K.shape[1] - 1, np.complex128)
    for a in range(out.size):
        q = min(a // ks, K.shape[0] - 2)
        f = (a - q * ks) / ks
        for l in range(K.shape[1]):
            if 0 <= a - l < x.size:
                out[a] += (K[q][l] + f * (K[q + 1][l] - K[q][l])) * x[a - l]
    return out


@pytest.mark.parametrize("n_knots,ks,taps,n", ((2, 70, 5, 60), (7, 11, 4, 63), (64, 1, 3, 61), (5, 37, 21, 128), (3, 40, 1, 81)))
def test_tv_conv_is_the_double_loop(n_knots, ks, taps, n):
    rs = np.random.RandomState(n_knots + ks)
    K = rs.randn(n_knots, taps) + 1j * rs.randn(n_knots, taps)
    x = rs.randn(n) + 1j * rs.randn(n)
    got, want = R.tv_conv(K, ks, x), _literal(K, ks, x)
    assert got.shape == want.shape == (n + taps - 1,) and got.dtype == np.complex128
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(got - np.convolve(K[0], x)).max() > 0.1                   # (the track moves)


def test_tv_conv_of_equal_knots_is_convolve_and_refuses_a_short_track():
    rs = np.random.RandomState(5)
    h = rs.randn(21) + 1j * rs.randn(21)
    x = rs.randn(300) + 1j * rs.randn(300)
    for n_knots, ks in ((2, 319), (6, 64), (64, 37), (40, 9)):
        assert np.array_equal(R.tv_conv(np.tile(h, (n_knots, 1)), ks, x), np.convolve(h, x)), (n_knots, ks)
    with pytest.raises(ValueError):
        R.tv_conv(np.tile(h, (2, 1)), 318, x)
    with pytest.raises(ValueError):
        R.tv_conv(h[None, :], 400, x)
    assert R.tv_conv(np.tile(h, (2, 1)), 319, x).shape == (320,)


def test_tv_conv_between_two_knots_blends_their_convolutions():
    rs = np.random.RandomState(6)
    hA, hB = rs.randn(2, 9) + 1j * rs.randn(2, 9)
    x = rs.randn(200) + 1j * rs.randn(200)
    A = 208                                                                 # one interval over the whole output, 208 samples
    w = np.arange(208) / A
    want = (1.0 - w) * np.convolve(hA, x) + w * np.convolve(hB, x)
    got = R.tv_conv(np.stack([hA, hB]), A, x)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # and a longer interval: the clamp on q keeps the single pair
    got = R.tv_conv(np.stack([hA, hB]), 1000, x)
    w = np.arange(208) / 1000
    assert np.abs(got - ((1.0 - w) * np.convolve(hA, x) + w * np.convolve(hB, x))).max() <= 1e-14 * np.abs(want).max()


# ---- the mirror ----

@pytest.mark.parametrize("n_fft,system,variant,nbt", ((64, "wtx", "half", 1), (128, "CPW", "half_masked", 0),
                                                      (64, "wrx", "plain", 1)))
def test_mirror_on_a_static_track_is_frame_profile(n_fft, system, variant, nbt):
    cp, S, k = RC.shape_of(n_fft, system, variant)
    c = RC.make_case(W.make_structure(system, n_fft, cp), k, S, variant, 11, nbt)
    st = c["st"]
    on = np.ones(n_fft, bool) if c["active"] is None else c["active"]
    nl = R._noise_len(st, S, c["h"].shape[1], nbt)
    grid = T.qam_table(k)[R.gen_labels(n_fft, k, S, 9, 3, 1)] * on[None, :]
    noise = R.gen_noise(nl, 9, 3, 1)
    want = R.frame_profile(st, grid, noise, c["w_tx"][1], c["w_rx"][1], c["h"][0], c["snr"][1], k, c["active"], c["mask"], nbt)
    sync = R.frame_profile_sync(st, grid, lambda idx: R.gen_noise_at(idx, 9, 3, 1), c["w_tx"][1], c["w_rx"][1], c["h"][0],
                                R.SyncPoint(0, 0.0, 1), c["snr"][1], k, c["active"], c["mask"], nbt)
    for n_knots, ks in ((S + 2, st.stride), (64, -(-(st.frame_len(S) + 19) // 63)), (2, st.frame_len(S) + 21)):
        got = R.frame_profile_doppler(st, grid, noise, c["w_tx"][1], c["w_rx"][1], np.tile(c["h"][0], (n_knots, 1)), ks,
                                      c["snr"][1], k, c["active"], c["mask"], nbt)
        assert len(got) == 8 and len(want) == 5 and len(sync) == 8
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        for g, w in zip(got, sync):                                         # all eight: the per-symbol sums too
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
        assert got[5].sum() == want[0].sum() > 0 and got[6].sum() == want[1].sum()
    # a moving track is another result; with_y adds Y
    moving = DC.tracks_of(c, [0.0, 0.02], st.stride, S + 2)[1, 0]
    got = R.frame_profile_doppler(st, grid, noise, c["w_tx"][1], c["w_rx"][1], moving, st.stride, c["snr"][1], k, c["active"],
                                  c["mask"], nbt, with_y=True)
    assert len(got) == 9 and got[8].shape == (S, n_fft) and not np.array_equal(got[2], want[2])
    # and the host route: a static track of a call is rx_profile_host, whatever shares the call
    tracks = DC.tracks_of(c, [0.03, 0.0], st.stride, S + 2)
    args = (st, k, S, c["w_tx"], c["w_rx"])
    tail = (c["snr"], 9, 0, 2)
    a, near = R.rx_profile_doppler_host(*args, tracks, st.stride, *tail, active=c["active"], mask=c["mask"],
                                        noise_before_truncate=nbt, with_near=True)
    b, near_b = R.rx_profile_host(*args, c["h"], *tail, active=c["active"], mask=c["mask"], noise_before_truncate=nbt, with_near=True)
    assert a.bit_err.shape == (2,) + b.bit_err.shape and a.bit_err_sym.shape == (2,) + b.bit_err.shape[:-1] + (S - 1,)
    assert np.array_equal(a.bit_err[1], b.bit_err) and np.array_equal(a.sym_err[1], b.sym_err)
    assert np.array_equal(a.err_power[1], b.err_power) and np.array_equal(a.decisions, b.decisions)
    assert np.array_equal(near[1], near_b) and not np.array_equal(a.err_power[0], b.err_power)
    assert np.array_equal(a.bit_err_sym.sum(axis=-1), a.bit_err.sum(axis=-1))
    assert np.array_equal(a.sym_err_sym.sum(axis=-1), a.sym_err.sum(axis=-1))


# ---- the channel tracks ----

def test_gen_chan_track_begins_at_gen_chan_and_holds_still_without_doppler():
    fs = 5e6
    for seed, doppler in ((1, 185.0), (2, 50.0), (3, 0.0), (4, 5000.0)):
        want = CH.gen_chan("vehicularA", 21, doppler, fs, 16 * 256 / fs, 1, np.random.RandomState(seed))[:, 0]
        got = CH.gen_chan_track("vehicularA", 21, doppler, fs, 296, 18, np.random.RandomState(seed))
        assert got.shape == (18, 21) and got.dtype == np.complex128
        assert np.abs(got[0] - want).max() <= 1e-14 * np.abs(want).max(), (seed, doppler)
        if doppler == 0.0:
            assert all(np.array_equal(got[q], got[0]) for q in range(18))
        else:
            assert np.abs(got[-1] - got[0]).max() > 1e-3
    # knot 0 does not depend on the Doppler, the knot's time does: q knot_step / fs
    a = CH.gen_chan_track("vehicularA", 21, 185.0, fs, 296, 18, np.random.RandomState(7))
    b = CH.gen_chan_track("vehicularA", 21, 740.0, fs, 74, 18, np.random.RandomState(7))
    c = CH.gen_chan_track("vehicularA", 21, 185.0, fs, 148, 35, np.random.RandomState(7))
    assert np.array_equal(a[0], b[0]) and np.abs(a - b).max() <= 1e-12 and np.abs(a - c[::2]).max() <= 1e-12


def test_gen_channel_tracks_share_phases_across_speeds_and_begin_at_the_channel_file():
    v = [0.0, 30 / 3.6, 100 / 3.6]
    tr = CH.gen_channel_tracks("vehicularA", 5, v, knot_step=296, n_knots=18, rng=np.random.RandomState(11))
    want = CH.gen_channel_file("vehicularA", 5, rng=np.random.RandomState(11))
    assert tr.shape == (3, 5, 18, 21) and want.shape == (21, 5)
    for i in range(5):
        for s in range(3):
            assert np.abs(tr[s, i, 0] - want[:, i]).max() <= 1e-14 * np.abs(want[:, i]).max(), (s, i)
        assert np.array_equal(tr[1, i, 0], tr[2, i, 0]) and np.array_equal(tr[0, i, 0], tr[2, i, 0])
        assert all(np.array_equal(tr[0, i, q], tr[0, i, 0]) for q in range(18))              # 0 m/s: the column held
        # the same phases at 30 and 100 km/h: knot 10 at 30 km/h is the time of knot 3 at 100 km/h
        assert np.abs(tr[1, i, 10] - tr[2, i, 3]).max() <= 1e-12
    # a speed of its own is the same track, whatever shares the call
    one = CH.gen_channel_tracks("vehicularA", 5, v[2:], knot_step=296, n_knots=18, rng=np.random.RandomState(11))
    assert np.array_equal(one[0], tr[2])
    doppler = (100 / 3.6) / 299792458.0 * 2e9
    assert abs(doppler - 185.3) < 0.1
    assert np.allclose(tr[2, 0], CH.gen_chan_track("vehicularA", 21, doppler, 5e6, 296, 18, np.random.RandomState(11)), rtol=0, atol=1e-14)
