"""wofdm_rx_profile_tracking without a GPU: its place in the public header and the binding, and its argument checks -- the new
conditions of include/wofdm.h (a pilot on a bin that is not loaded, a comb that leaves no data bin, cpe without a pilot bin, post
with S = 2, flags outside {0, 1}, reserved not 0, NULL tracking: WOFDM_E_INVALID) and those it inherits from
wofdm_rx_profile_soft are answered before the device is touched (this machine has none: a call that passes the checks ends in
WOFDM_E_HIP), and a failed call leaves the seven outputs as they were.  The pattern, the shapes and the points are
tests/test_rx_profile_soft_abi.py's.  ``tracking_for_window_file(gpu=False)`` is the host route."""
import ctypes as C
import os
import re

import numpy as np

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R
from wofdm_amd import variants as V

import test_rx_profile_link_abi as LA

ROOT = LA.ROOT
POISON_U, POISON_F = LA.POISON_U, LA.POISON_F
N, S, TAPS, N_CH, N_SNR, PAIRS = LA.N, LA.S, LA.TAPS, LA.N_CH, LA.N_SNR, LA.PAIRS
COMB = tuple(range(0, N, 8))


def _call(points=({},), tracking=None, pilots=COMB, active=None, scales=(1.0, 0.5), null=(), n_points=None, n_tracks=2, syms=S,
          edit=None, cfg_edit=None, device=99):
    """rc of one call on small arrays (the soft test's, with the comb -- the indices of the pilot bins, None: NULL -- and one
    tracking point (cpe, post, reserved) per point, default (0, 0, (0, 0)))"""
    st = V.make_structure("CPW", N, 32)
    cfg = W.make_cfg(st, 4, syms, TAPS, N_CH, N_SNR, PAIRS, seed=3, frames_per_cell=3)
    B, P = st.stride, st.sym_len
    n_knots, knot_step = syms + 2, B
    pil = None
    if pilots is not None:
        pil = np.zeros(N, np.uint8)
        pil[list(pilots)] = 1
    a = dict(w_tx=np.ones((PAIRS, P), np.float32), w_rx=np.ones((PAIRS, N + st.tail_rx), np.float32),
             h=np.ones((N_CH, TAPS, 2), np.float32), snr=np.full(N_SNR, 10.0, np.float32),
             active=None if active is None else np.asarray(active, np.uint8), mask=None,
             h_track=np.ones((max(n_tracks, 1), N_CH, n_knots, TAPS, 2), np.float32),
             aci_active=np.ones(N, np.uint8), aci_h=np.ones((N_CH, TAPS, 2), np.float32), ref_power=np.ones(PAIRS, np.float32),
             scales=np.asarray(scales, np.float32), pilots=pil)
    NP = max(len(points), 1)
    cpts = (_lib.LinkPoint * NP)()
    for q, over in zip(cpts, points):
        for f, v in dict(LA.OK_POINT, **over).items():
            if f == "reserved":
                q.reserved = (C.c_int32 * 4)(*v)
            else:
                setattr(q, f, v)
    ctps = (_lib.TrackingPoint * NP)()
    for q, (cpe, post, res) in zip(ctps, tracking or [(0, 0, (0, 0))] * NP):
        q.cpe, q.post, q.reserved = cpe, post, (C.c_int32 * 2)(*res)
    cells, NS = PAIRS * N_CH * N_SNR, len(scales)
    outs = dict(errs=np.full((NP, cells, N, 2), POISON_U, np.uint64), pw=np.full((NP, cells, N), POISON_F, np.float64),
                serrs=np.full((NP, cells, syms - 1, 2), POISON_U, np.uint64), spw=np.full((NP, cells, syms - 1), POISON_F, np.float64),
                ppw=np.full((NP, cells, 2), POISON_F, np.float64), bpen=np.full((NP, cells, NS, N), POISON_F, np.float64),
                spen=np.full((NP, cells, NS, syms - 1), POISON_F, np.float64))
    a.update(outs)
    if edit:
        edit(a)
    if cfg_edit:
        cfg_edit(cfg)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_tracking(
        None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], n_tracks, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"],
        len(points) if n_points is None else n_points, None if "points" in null else cpts, len(scales), ptr["scales"],
        ptr["pilots"], None if "tracking" in null else ctps,
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"], ptr["bpen"], ptr["spen"])
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_F)).all(), n
    return rc


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_tracking_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_tracking\((.*?)\);", hdr, flags=re.M | re.S)
    soft = re.search(r"^int wofdm_rx_profile_soft\((.*?)\);", hdr, flags=re.M | re.S)
    assert m and soft

    def args_of(text):
        return [a.strip() for a in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    args, sargs = args_of(m.group(1)), args_of(soft.group(1))
    # every argument of the soft call up to the scales, the comb and the tracking points, its seven outputs
    assert args == sargs[:19] + ["const uint8_t *pilots", "const wofdm_tracking_point *tracking"] + sargs[19:]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_tracking.argtypes
    assert len(at) == len(args) == 28 and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else
                     C.POINTER(_lib.TrackingPoint) if "wofdm_tracking_point" in arg else C.c_void_p), arg
    st = re.search(r"typedef struct wofdm_tracking_point \{(.*?)\} wofdm_tracking_point;", hdr, flags=re.S)
    fields = re.findall(r"int32_t\s+(\w+)(\[\d+\])?;", st.group(1))
    assert [f for f, _ in fields] == [f for f, _ in _lib.TrackingPoint._fields_] == ["cpe", "post", "reserved"]
    assert C.sizeof(_lib.TrackingPoint) == 16 and fields[2][1] == "[2]"
    assert "wofdm_rx_profile_tracking" in _lib.EXPORTS and hasattr(lib, "wofdm_rx_profile_tracking")
    for name in ("RxProfileTracking", "TrackingPoint", "pilot_comb", "tracking_equalise", "frame_profile_tracking",
                 "rx_profile_tracking_host", "rx_profile_tracking_gpu", "rx_profile_tracking_chunk_frames", "tracking_for_window_file"):
        assert hasattr(W, name), name
    # the existing struct and its check stay as they are
    assert C.sizeof(_lib.LinkPoint) == 64


def test_a_valid_call_reaches_the_device_and_no_further():
    everything = dict(pa_model=1, pa_ibo_db=3.0, track=1, timing=2, cfo=0.02, linewidth=1e-3, cpe_tracked=1, aci_on=1, aci_delay=7,
                      aci_level_db=10.0)
    assert _call() == -3 and "device" in _err()
    assert _call(points=({}, everything, {}, everything), tracking=[(0, 0, (0, 0)), (1, 0, (0, 0)), (0, 1, (0, 0)), (1, 1, (0, 0))]) == -3
    assert _call(pilots=None) == -3                                    # no comb
    assert _call(pilots=None, tracking=[(0, 1, (0, 0))]) == -3         # the postamble needs none
    assert _call(pilots=(5,), tracking=[(1, 0, (0, 0))]) == -3         # one pilot is a comb
    assert _call(pilots=(), tracking=[(0, 1, (0, 0))]) == -3           # an empty comb is no comb
    assert _call(syms=3, tracking=[(1, 1, (0, 0))]) == -3
    half = CM.half_band_allocation(N)
    assert _call(active=half, pilots=np.flatnonzero(half)[::8]) == -3
    assert _call(active=half, pilots=np.flatnonzero(half)[1:], tracking=[(1, 1, (0, 0))]) == -3   # one data bin left
    for out in ("pw", "serrs", "spw", "ppw", "spen"):
        assert _call(null=(out,)) == -3, out


def test_tracking_refuses_invalid_arguments():
    half = CM.half_band_allocation(N)
    off = int(np.flatnonzero(~half)[0])
    assert _call(null=("tracking",)) == -1 and "NULL" in _err()
    assert _call(active=half, pilots=(int(np.flatnonzero(half)[0]), off)) == -1 and "pilots[%d]" % off in _err()
    assert _call(pilots=range(N)) == -1 and "data bin" in _err()
    assert _call(active=half, pilots=np.flatnonzero(half)) == -1 and "data bin" in _err()
    assert _call(pilots=None, tracking=[(1, 0, (0, 0))]) == -1 and "pilot" in _err()
    assert _call(pilots=(), points=({}, {}), tracking=[(0, 0, (0, 0)), (1, 1, (0, 0))]) == -1 and "tracking[1]" in _err()
    assert _call(syms=2, tracking=[(0, 1, (0, 0))]) == -1 and "post" in _err()
    assert _call(syms=2, tracking=[(1, 0, (0, 0))]) == -3              # the comb alone needs no third symbol
    for bad in ((2, 0, (0, 0)), (-1, 0, (0, 0)), (0, 2, (0, 0)), (0, -1, (0, 0)), (0, 0, (1, 0)), (1, 1, (0, 7))):
        assert _call(points=({}, {}), tracking=[(1, 1, (0, 0)), bad]) == -1 and "tracking[1]" in _err(), bad
    # the documented order: the comb before the points
    assert _call(active=half, pilots=(off,), tracking=[(2, 0, (0, 0))]) == -1 and "pilots" in _err()
    # the soft call's own, each before the device as well
    for name in ("scales", "bpen", "cfg", "w_tx", "w_rx", "h", "snr", "errs", "points"):
        assert _call(null=(name,)) == -1, name
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert _call(scales=(1.0, bad)) == -1 and "scales[1]" in _err(), bad
    assert _call(n_points=0) == -1
    assert _call(points=(dict(track=0),), null=("h_track",)) == -1
    assert _call(points=({}, dict(aci_on=1)), null=("aci_active",)) == -1
    assert _call(points=({}, dict(pa_model=1)), null=("ref_power",)) == -1
    for bad in (dict(track=-2), dict(aci_on=2), dict(reserved=(0, 0, 1, 0)), dict(cfo=np.nan), dict(linewidth=-1e-3)):
        assert _call(points=({}, bad)) == -1, bad
    assert _call(edit=LA._set("h", -1, np.nan)) == -1
    assert _call(cfg_edit=lambda c: setattr(c, "n_snr", 0)) == -1


def test_tracking_refuses_what_lies_outside_its_limits():
    assert _call(scales=[1.0] * 17) == -2 and "n_scales" in _err()
    assert _call(n_points=17, points=[{}] * 17) == -2
    B = V.make_structure("CPW", N, 32).stride
    for bad in (dict(timing=B), dict(cfo=4.5), dict(linewidth=1.5), dict(aci_delay=B), dict(pa_model=3)):
        assert _call(points=({}, bad)) == -2, bad
    assert _call(cfg_edit=lambda c: setattr(c, "n_fft", 96)) == -2
    assert _call(cfg_edit=lambda c: setattr(c, "syms_per_frame", 17)) == -2


def test_tracking_for_window_file_takes_the_host_route(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=2, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    pts = [R.LinkPoint(), R.LinkPoint(cfo=0.02, cfo_tracked=0), R.LinkPoint(linewidth=1e-3)]
    tps, sc = [(0, 0), (1, 0), (1, 1)], (0.5, 0.1)
    got = W.tracking_for_window_file("wtx", 8, win, h, snr, pts, tps, 4, sc, gpu=False, **kw)
    assert list(got) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    pil = R.pilot_comb(alloc, 4)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want = R.rx_profile_tracking_host(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 2, pts, tps, pil, sc, active=alloc, mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g = got[name][key]
            assert type(g) is R.RxProfileTracking and g.bit_penalty.shape == (3, 2, 2, 2, 64) and g.bit_err_sym.shape == (3, 2, 2, 3)
            for f in R.RxProfileTracking._fields[:-3]:
                assert np.array_equal(getattr(g, f), getattr(want, f)[:, i]), (name, key, f)
            for f in ("scales", "decisions_sym", "decisions"):
                assert np.array_equal(getattr(g, f), getattr(want, f)), f
            assert (g.decisions[:, pil] == 0).all() and (g.decisions[2, alloc & ~pil] == 2 * 2).all()
            assert (g.bit_err[..., pil] == 0).all() and np.isfinite(R.gmi(g, 4)[0]).all()
    # no comb, every point (0, 0): soft_for_window_file's fields
    plain = W.tracking_for_window_file("wtx", 8, win, h, snr, pts, None, None, sc, gpu=False, **kw)
    soft = W.soft_for_window_file("wtx", 8, win, h, snr, pts, sc, gpu=False, **kw)
    for name in ("opt", "rc"):
        for f in ("bit_err", "sym_err", "bit_err_sym"):
            assert np.array_equal(getattr(plain[name]["profile_masked"], f), getattr(soft[name]["profile_masked"], f)), f
        assert np.allclose(plain[name]["profile"].bit_penalty, soft[name]["profile"].bit_penalty, rtol=1e-12, atol=0.0)
