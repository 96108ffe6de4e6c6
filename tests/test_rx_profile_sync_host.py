"""wofdm_rx_profile_sync without a GPU: its place in the public header, the binding and the package; its argument checks, all
answered before the device is touched (the calls name a device that does not exist: one that passes them ends in WOFDM_E_HIP) with the four
outputs left as they were; and the fp64 mirror ``frame_profile_sync`` -- equal to ``frame_profile`` at timing 0, offset 0, the
sign of its timing tied to the CPU oracle through a delayed channel (early and late), the unit and sign of its carrier offset
through the bin shift of CP-OFDM, the free-running phase through the tracked one, and the noise of any sample index against a
direct restatement of Philox."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

import rx_profile_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_U, POISON_F = 0xA5A5A5A5A5A5A5A5, -12345.678


# ---- header, binding, exports ----

def test_rx_profile_sync_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_sync\((.*?)\);", hdr, flags=re.M | re.S)
    assert m
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["const wofdm_cfg *cfg", "int device", "const float *w_tx", "const float *w_rx", "const float *h",
                    "const float *snr_db", "const uint8_t *active", "const float *tx_mask", "int32_t n_points",
                    "const wofdm_sync_point *points", "uint64_t *errs", "double *err_power", "uint64_t *sym_errs",
                    "double *sym_power"]
    assert hdr.index("int wofdm_rx_profile_sync(") > hdr.index("int wofdm_rx_profile_kernel_ms(")
    assert re.search(r"^#define WOFDM_SYNC_MAX_POINTS 64$", hdr, flags=re.M) and _lib.SYNC_MAX_POINTS == 64
    body = hdr[hdr.index("typedef struct wofdm_sync_point {"):hdr.index("} wofdm_sync_point;")]
    fields = re.findall(r"^\s*(int32_t|float)\s+(\w+);", body, flags=re.M)
    assert fields == [("int32_t", "timing"), ("float", "cfo"), ("int32_t", "cfo_tracked"), ("int32_t", "reserved")]
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert _lib.SyncPoint._fields_ == [(name, ctype[t]) for t, name in fields] and C.sizeof(_lib.SyncPoint) == 16
    lib = _lib.load()
    at = lib.wofdm_rx_profile_sync.argtypes
    assert len(at) == len(args) and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    assert at[8] == C.c_int32 and at[9] == C.POINTER(_lib.SyncPoint)
    assert all(t == C.c_void_p for i, t in enumerate(at) if i >= 2 and i not in (8, 9))
    assert "wofdm_rx_profile_sync" in _lib.EXPORTS and hasattr(lib, "wofdm_rx_profile_sync")
    # the header says what the call's kernel time is read with, the sample index, both rotations and the chunk formula
    kms = hdr[hdr.index("/* *ms = milliseconds (HIP events) the kernels of the calling thread's last successful wofdm_rx_profile or"):
              hdr.index("int wofdm_rx_profile_kernel_ms")]
    assert "wofdm_rx_profile_sync call" in kms and "wofdm_rx_profile_aci call took (whichever came last)" in kms
    doc = hdr[hdr.index("/* wofdm_rx_profile under receiver timing"):hdr.index("#define WOFDM_SYNC_MAX_POINTS")]
    for text in ("a = s B + prefix_rm + timing + m", "e^{+2 pi i cfo a / n_fft}", "e^{+2 pi i cfo m / n_fft}", "a mod 2^32",
                 "8 (S n_fft + T + [mask] S (2P-1)) + 8 n_points (n_fft + S)"):
        assert text in doc, text
    for name in ("SyncPoint", "RxProfileSync", "rx_profile_sync_gpu", "rx_profile_sync_host", "frame_profile_sync", "gen_noise_at",
                 "rx_profile_sync_chunk_frames", "sync_for_window_file"):
        assert hasattr(W, name), name
    assert R.SyncPoint(3) == (3, 0.0, 1) and R.RxProfileSync._fields[:3] == R.RxProfile._fields[:3]


def test_chunk_formula_of_the_header():
    for st, S, masked, pts in ((V.make_structure("wtx", 1024, 56), 16, False, 2), (V.make_structure("CPW", 256, 32), 9, True, 9),
                               (V.make_structure("wrx", 64, 8), 2, True, 64), (V.make_structure("CP", 64, 16), 2, False, 1)):
        P, N = st.sym_len, st.n_fft
        Tv = st.tail_tx + S * (P - st.tail_tx)
        per = 8 * (S * N + Tv + (S * (2 * P - 1) if masked else 0)) + 8 * pts * (N + S)
        assert R.rx_profile_sync_chunk_frames(st, S, masked, pts) == min(65535, (256 << 20) // per)
        assert R.rx_profile_sync_chunk_frames(st, S, masked, pts) <= R.rx_profile_chunk_frames(st, S, masked)


# ---- argument checks without a device ----

def _call(st=None, k=4, S=4, n_taps=3, n_ch=2, n_snr=2, pairs=2, frames=3, device=99, null=(), mask=False, active=None,
          points=((0, 0.0, 1, 0), (5, 0.25, 0, 0)), n_points=None, edit=None, cfg_edit=None):
    """rc of one call on small arrays; `edit` changes the arrays, `cfg_edit` the cfg, before the call"""
    st = V.make_structure("CPW", 128, 32) if st is None else st
    cfg = W.make_cfg(st, k, S, n_taps, n_ch, n_snr, pairs, seed=3, frames_per_cell=frames)
    P, NW, N = st.sym_len, st.n_fft + st.tail_rx, st.n_fft
    a = dict(w_tx=np.ones((pairs, P), np.float32), w_rx=np.ones((pairs, NW), np.float32),
             h=np.ones((n_ch, n_taps, 2), np.float32), snr=np.full(n_snr, 10.0, np.float32),
             active=None if active is None else np.ascontiguousarray(active, np.uint8),
             mask=np.ones(2 * P - 1, np.float32) if mask else None)
    cpts = (_lib.SyncPoint * max(1, len(points)))(*[_lib.SyncPoint(*q) for q in points])
    n_points = len(points) if n_points is None else n_points
    cells, held = pairs * n_ch * n_snr, max(1, len(points))
    errs = np.full((held, cells, N, 2), POISON_U, np.uint64)
    pw = np.full((held, cells, N), POISON_F, np.float64)
    serrs = np.full((held, cells, max(1, S - 1), 2), POISON_U, np.uint64)
    spw = np.full((held, cells, max(1, S - 1)), POISON_F, np.float64)
    a.update(errs=errs, pw=pw, serrs=serrs, spw=spw)
    if edit:
        edit(a)
    if cfg_edit:
        cfg_edit(cfg)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_sync(None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"],
                                           ptr["snr"], ptr["active"], ptr["mask"], n_points, None if "points" in null else cpts,
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
    B = V.make_structure("CPW", 128, 32).stride
    assert _call(points=((B - 1, 4.0, 0, 0), (-(B - 1), -4.0, 1, 0))) == -3        # the limits themselves are inside
    assert _call(points=((0, 0.0, 0, 0),) * 64) == -3
    assert _call(points=((7, -0.5, 1, 0),)) == -3
    assert _call(st=V.make_structure("wtx", 1024, 128), S=2, mask=True) == -3
    assert _call(st=V.make_structure("wtx", 1024, 56), S=16) == -3
    assert _call(n_taps=21) == -3 and _call(S=16) == -3 and _call(S=2) == -3
    assert _call(frames=0) == -3
    for name in ("pw", "serrs", "spw"):                                     # three of the outputs are optional
        assert _call(null=(name,)) == -3, name
    assert _call(null=("pw", "serrs", "spw")) == -3


def test_rx_profile_sync_refuses_invalid_arguments():
    for name in ("cfg", "w_tx", "w_rx", "h", "snr", "errs", "points"):
        assert _call(null=(name,)) == -1, name
    assert "points" in _last()
    for n in (0, -1, -(2 ** 31)):
        assert _call(n_points=n) == -1 and "n_points" in _last()
    for bad in (np.nan, np.inf, -np.inf):
        assert _call(points=((0, 0.0, 1, 0), (0, bad, 1, 0))) == -1 and "cfo" in _last()
        assert _call(points=((0, bad, 0, 0),)) == -1
        for name in ("w_tx", "w_rx", "h", "snr"):                          # the checks of wofdm_rx_profile
            assert _call(edit=_set(name, -1, bad)) == -1, name
        assert _call(mask=True, edit=_set("mask", -1, bad)) == -1
    for r in (1, -1, 2 ** 31 - 1):
        assert _call(points=((0, 0.0, 1, 0), (0, 0.0, 1, r))) == -1 and "reserved" in _last()
    for t in (2, -1, 256):
        assert _call(points=((0, 0.0, t, 0),)) == -1 and "cfo_tracked" in _last()
    assert _call(active=np.zeros(128, np.uint8)) == -1 and "loads no subcarrier" in _last()
    for field in ("n_channels", "n_snr", "n_window_pairs"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, 0)) == -1, field
    for field in ("cp", "cs", "tail_tx", "prefix_rm", "circ_shift", "n_taps"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, -1)) == -1, field


def test_rx_profile_sync_refuses_what_lies_outside_its_limits():
    st = V.make_structure("CPW", 128, 32)
    B = st.stride
    assert _call(points=((0, 0.0, 0, 0),) * 65) == -2 and "n_points" in _last()
    for t in (B, -B, 2 ** 31 - 1, -(2 ** 31)):
        assert _call(points=((0, 0.0, 1, 0), (t, 0.0, 1, 0))) == -2 and "timing" in _last(), t
    for e in (4.0001, -4.0001, 1e30):
        assert _call(points=((0, e, 1, 0),)) == -2 and "cfo" in _last(), e
        assert _call(points=((0, e, 0, 0),)) == -2
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
    assert _call(cfg_edit=lambda c: (setattr(c, "n_channels", 1 << 14), setattr(c, "n_snr", 1 << 14))) == -2


# ---- the mirror ----

def channels8():
    """[2, 8] complex64: the first 8 taps of two channels of the golden file"""
    return np.load(os.path.join(RC.GOLDEN, "channels_vehA.npz"), allow_pickle=False)["h"][:2, :8].astype(np.complex64)


@pytest.mark.parametrize("n_fft,system,variant,nbt", ((64, "wtx", "half", 1), (128, "CPW", "half_masked", 0),
                                                      (64, "wrx", "plain", 1)))
def test_mirror_at_no_offset_is_frame_profile(n_fft, system, variant, nbt):
    cp, S, k = RC.shape_of(n_fft, system, variant)
    c = RC.make_case(W.make_structure(system, n_fft, cp), k, S, variant, 11, nbt)
    st = c["st"]
    on = np.ones(n_fft, bool) if c["active"] is None else c["active"]
    nl = R._noise_len(st, S, c["h"].shape[1], nbt)
    grid = T.qam_table(k)[R.gen_labels(n_fft, k, S, 9, 3, 1)] * on[None, :]
    want = R.frame_profile(st, grid, R.gen_noise(nl, 9, 3, 1), c["w_tx"][1], c["w_rx"][1], c["h"][0], c["snr"][1], k, c["active"],
                           c["mask"], nbt)
    for tracked in (0, 1):
        got = R.frame_profile_sync(st, grid, lambda idx: R.gen_noise_at(idx, 9, 3, 1), c["w_tx"][1], c["w_rx"][1], c["h"][0],
                                   R.SyncPoint(0, 0.0, tracked), c["snr"][1], k, c["active"], c["mask"], nbt)
        assert len(got) == 8 and len(want) == 5
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        assert got[5].shape == got[6].shape == got[7].shape == (S - 1,)
        assert got[5].sum() == want[0].sum() > 0 and got[6].sum() == want[1].sum() and abs(got[7].sum() - want[2].sum()) < 1e-9
    # and the host route: the point (0, 0) of a sweep is rx_profile_host, whatever shares the call
    args = (st, k, S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 9, 0, 2)
    a, near = R.rx_profile_sync_host(*args, [(3, 0.1, 0), (0, 0.0, 1), R.SyncPoint(-5)], active=c["active"], mask=c["mask"],
                                     noise_before_truncate=nbt, with_near=True)
    b, near_b = R.rx_profile_host(*args, active=c["active"], mask=c["mask"], noise_before_truncate=nbt, with_near=True)
    assert a.bit_err.shape == (3,) + b.bit_err.shape and a.bit_err_sym.shape == (3,) + b.bit_err.shape[:-1] + (S - 1,)
    assert np.array_equal(a.bit_err[1], b.bit_err) and np.array_equal(a.sym_err[1], b.sym_err)
    assert np.array_equal(a.err_power[1], b.err_power) and np.array_equal(a.decisions, b.decisions)
    assert np.array_equal(near[1], near_b) and not np.array_equal(a.bit_err[0], b.bit_err)
    assert np.array_equal(a.bit_err_sym.sum(axis=-1), a.bit_err.sum(axis=-1))
    assert np.array_equal(a.sym_err_sym.sum(axis=-1), a.sym_err.sum(axis=-1))


def _oracle_y(st, k, S, lab, w_tx, w_rx, taps):
    osys = O.make_sys(st.n_fft, k, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, taps.size, 1)
    _, d = O.frame(osys, w_tx, w_rx, taps, 300.0, lab, np.zeros(O.noise_len(osys), np.complex128) + 1.0, dump=True)
    return d["Y"]


def _ones(idx):
    return np.ones(np.shape(idx), np.complex128)


@pytest.mark.parametrize("system,d", (("wtx", 1), ("CPW", 5), ("wrx", 13), ("CP", 13), ("WOLA", 9)))
def test_timing_sign_against_the_oracle(system, d):
    """A receiver that begins d samples EARLY (timing = -d) sees what a synchronised one sees behind the channel [0_d, h], and
    one that begins d samples LATE (timing = +d) behind [0_d, h] sees what a synchronised one sees behind h.  The oracle
    transmits both synchronised frames (d + taps <= 21, 300 dB).  Early: every symbol; late: every symbol as well -- the last
    one reads d samples past S B, which the mirror's conv still holds (the oracle's frame with h has them inside its last
    block).  Agreement: 1e-9 of max |Y| asked; observed 5.0e-16 early and 6.9e-16 late (fp64 rounding of two transform chains)."""
    n, k, S, L = 64, 4, 5, 8
    st = V.make_structure(system, n, 16)
    assert d + L <= 21 and d < st.stride
    h = channels8()[0].astype(np.complex128)
    hd = np.concatenate((np.zeros(d), h))
    w_tx = RC.PC.random_windows(st, 1, 60 + d)[0].astype(np.float64)
    w_rx = RC.random_rx_windows(st, 1, 70 + d)[0].astype(np.float64)
    lab = R.gen_labels(n, k, S, 8, 2, 4)
    grid = T.qam_table(k)[lab]
    early = R.frame_profile_sync(st, grid, _ones, w_tx, w_rx, h, R.SyncPoint(-d), 300.0, k, with_y=True)[8]
    want = _oracle_y(st, k, S, lab, w_tx, w_rx, hd)
    e_early = np.abs(early - want).max() / np.abs(want).max()
    late = R.frame_profile_sync(st, grid, _ones, w_tx, w_rx, hd, R.SyncPoint(+d), 300.0, k, with_y=True)[8]
    want_l = _oracle_y(st, k, S, lab, w_tx, w_rx, h)
    e_late = np.abs(late - want_l).max() / np.abs(want_l).max()
    wrong = R.frame_profile_sync(st, grid, _ones, w_tx, w_rx, h, R.SyncPoint(+d), 300.0, k, with_y=True)[8]
    print("%s d=%d: early %.2e, late %.2e of max |Y|; the other sign: %.2e"
          % (system, d, e_early, e_late, np.abs(wrong - want).max() / np.abs(want).max()))
    assert np.abs(want).max() > 0.1 and e_early < 1e-9 and e_late < 1e-9
    assert np.abs(wrong - want).max() / np.abs(want).max() > 1e-3


def test_units_and_sign_of_the_carrier_offset():
    """CP-OFDM, N = 64, CP 16, rectangular windows, 8 taps, 300 dB, every bin loaded, tracked: an offset of a whole number eps
    of subcarrier spacings moves what was sent on bin n - eps onto bin n and nothing else (the window holds eps whole turns),
    the pilot included, so Xhat[s][n] = X_s[n - eps] X_0[n] / X_0[n - eps] -- the channel drops out, H[n - eps] both in Y_s and
    in Y_0.  Timing 0, -3, -8: inside the CP behind 8 taps.  Observed: at most 6.2e-14 (fp64 rounding through the division by
    the faded bins of Y_0); asserted: ten times that."""
    st = V.make_structure("CP", 64, 16)
    n, k, S = 64, 4, 6
    w_tx, w_rx = np.ones(st.sym_len), np.ones(n)
    tab = T.qam_table(k)
    worst = 0.0
    for ch, h in enumerate(channels8()):
        X = tab[R.gen_labels(n, k, S, 5, ch, 1)]
        for eps in (1, -2):
            for theta in (0, -3, -8):
                xhat = R.frame_profile_sync(st, X, _ones, w_tx, w_rx, h, R.SyncPoint(theta, float(eps), 1), 300.0, k)[3]
                want = np.roll(X[1:], eps, axis=1) * (X[0] / np.roll(X[0], eps))[None, :]
                worst = max(worst, np.abs(xhat - want).max())
                other = np.roll(X[1:], -eps, axis=1) * (X[0] / np.roll(X[0], -eps))[None, :]
                assert np.abs(xhat - other).max() > 0.1
    print("whole-bin carrier offsets: Xhat against the shifted symbols %.2e" % worst)
    assert worst <= 6.2e-13


@pytest.mark.parametrize("system,n_fft,cp,theta,eps", (("wtx", 64, 16, 0, 0.37), ("CPW", 128, 32, -9, -1.6), ("WOLA", 64, 16, 21, 4.0),
                                                       ("wrx", 64, 8, -71, 0.02)))
def test_free_running_is_tracked_times_the_phase_at_the_window(system, n_fft, cp, theta, eps):
    """Y of a free-running oscillator = Y of a tracked one times e^{2 pi i eps (s B + gamma + theta) / N}, symbol by symbol,
    for any structure, noise included (12 dB).  Observed: at most 3.9e-15 of max |Y|; asserted: ten times that."""
    st = V.make_structure(system, n_fft, cp)
    k, S = 4, 5
    h = channels8()[1]
    w_tx = RC.PC.random_windows(st, 1, 5)[0].astype(np.float64)
    w_rx = RC.random_rx_windows(st, 1, 6)[0].astype(np.float64)
    grid = T.qam_table(k)[R.gen_labels(n_fft, k, S, 8, 1, 2)]
    e32 = float(np.float32(eps))

    def y(tracked):
        return R.frame_profile_sync(st, grid, lambda idx: R.gen_noise_at(idx, 8, 1, 2), w_tx, w_rx, h, R.SyncPoint(theta, eps, tracked),
                                    12.0, k, with_y=True)[8]
    phase = np.exp(2j * np.pi * e32 * (np.arange(S) * st.stride + st.prefix_rm + theta) / n_fft)
    free, tracked = y(0), y(1)
    err = np.abs(free - tracked * phase[:, None]).max() / np.abs(free).max()
    print("%s theta %d eps %g: free-running against tracked times the base phasor %.2e of max |Y|" % (system, theta, eps, err))
    assert err <= 3.9e-14 and np.abs(free - tracked).max() / np.abs(free).max() > 1e-3


# ---- the noise of any sample index ----

def test_noise_at_any_index_against_philox_restated():
    for seed, cell, frame in ((1, 0, 0), (0x9E3779B97F4A7C15, 5, 2 ** 32 + 7), (77, (1 << 28) - 1, 2 ** 40)):
        nl = 333
        assert np.array_equal(R.gen_noise_at(np.arange(nl), seed, cell, frame), R.gen_noise(nl, seed, cell, frame))
        idx = np.array([[-1, -2, -3, -1202], [0, 1, 2 ** 31 - 1, 2 ** 31], [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, -(2 ** 31)]])
        got = R.gen_noise_at(idx, seed, cell, frame)
        assert got.shape == idx.shape and got.dtype == np.complex128
        for a, z in zip(idx.reshape(-1), got.reshape(-1)):
            # restated: counter ((uint32) a >> 1, frame lo, frame hi, 1 << 28 | cell), key (seed lo, seed hi); word pair a & 1
            u = int(a) % 2 ** 32
            w = O.philox([u >> 1, frame & 0xFFFFFFFF, frame >> 32, (1 << 28) | cell], [seed & 0xFFFFFFFF, seed >> 32])
            wa, wb = int(w[2 * (u & 1)]), int(w[2 * (u & 1) + 1])
            u1 = float(np.float32(float(np.float32(wa)) * 2.0 ** -32 + 2.0 ** -33))
            want = np.sqrt(-2.0 * np.log(u1)) * np.exp(2j * np.pi * (wb >> 9) * 2.0 ** -23)
            assert z == want, (a, z, want)
        # the index is taken modulo 2^32, and a negative one is no sample of the frame
        assert got[2, 1] == got[1, 0] and got[2, 0] == got[0, 0] and got[2, 3] == got[1, 3]
        assert not np.isin(got[0], R.gen_noise(4096, seed, cell, frame)).any()
