"""wofdm_rx_profile_soft without a GPU: its place in the public header and the binding, and its argument checks -- the new
conditions of include/wofdm.h (NULL scales or bit_penalty, n_scales < 1, a scale that is not finite or not positive:
WOFDM_E_INVALID; n_scales above WOFDM_SOFT_MAX_SCALES: WOFDM_E_UNSUPPORTED) and those it inherits from wofdm_rx_profile_link are
answered before the device is touched (this machine has none: a call that passes the checks ends in WOFDM_E_HIP), and a failed call
leaves the seven outputs as they were.  The pattern, the shapes and the points are tests/test_rx_profile_link_abi.py's."""
import ctypes as C
import os
import re

import numpy as np

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import variants as V

import test_rx_profile_link_abi as LA

ROOT = LA.ROOT
POISON_U, POISON_F = LA.POISON_U, LA.POISON_F
N, S, TAPS, N_CH, N_SNR, PAIRS = LA.N, LA.S, LA.TAPS, LA.N_CH, LA.N_SNR, LA.PAIRS


def _call(points=({},), scales=(1.0, 0.5), n_scales=None, null=(), n_points=None, n_tracks=2, edit=None, cfg_edit=None, device=99):
    """rc of one call on small arrays (LA._call's, with the scales and the two further outputs)"""
    st = V.make_structure("CPW", N, 32)
    cfg = W.make_cfg(st, 4, S, TAPS, N_CH, N_SNR, PAIRS, seed=3, frames_per_cell=3)
    B, P = st.stride, st.sym_len
    n_knots, knot_step = S + 2, B
    a = dict(w_tx=np.ones((PAIRS, P), np.float32), w_rx=np.ones((PAIRS, N + st.tail_rx), np.float32),
             h=np.ones((N_CH, TAPS, 2), np.float32), snr=np.full(N_SNR, 10.0, np.float32), active=None, mask=None,
             h_track=np.ones((max(n_tracks, 1), N_CH, n_knots, TAPS, 2), np.float32),
             aci_active=np.ones(N, np.uint8), aci_h=np.ones((N_CH, TAPS, 2), np.float32), ref_power=np.ones(PAIRS, np.float32),
             scales=np.asarray(scales if len(scales) else (1.0,), np.float32))
    cpts = (_lib.LinkPoint * max(len(points), 1))()
    for q, over in zip(cpts, points):
        for f, v in dict(LA.OK_POINT, **over).items():
            if f == "reserved":
                q.reserved = (C.c_int32 * 4)(*v)
            else:
                setattr(q, f, v)
    NP, cells, NS = max(len(points), 1), PAIRS * N_CH * N_SNR, max(len(scales), 1)
    outs = dict(errs=np.full((NP, cells, N, 2), POISON_U, np.uint64), pw=np.full((NP, cells, N), POISON_F, np.float64),
                serrs=np.full((NP, cells, S - 1, 2), POISON_U, np.uint64), spw=np.full((NP, cells, S - 1), POISON_F, np.float64),
                ppw=np.full((NP, cells, 2), POISON_F, np.float64), bpen=np.full((NP, cells, NS, N), POISON_F, np.float64),
                spen=np.full((NP, cells, NS, S - 1), POISON_F, np.float64))
    a.update(outs)
    if edit:
        edit(a)
    if cfg_edit:
        cfg_edit(cfg)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_soft(
        None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], n_tracks, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"],
        len(points) if n_points is None else n_points, None if "points" in null else cpts,
        len(scales) if n_scales is None else n_scales, ptr["scales"],
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"], ptr["bpen"], ptr["spen"])
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_F)).all(), n
    return rc


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_soft_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_soft\((.*?)\);", hdr, flags=re.M | re.S)
    link = re.search(r"^int wofdm_rx_profile_link\((.*?)\);", hdr, flags=re.M | re.S)
    assert m and link

    def args_of(text):
        return [a.strip() for a in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    args, largs = args_of(m.group(1)), args_of(link.group(1))
    # every argument of the link call up to points, the scales, its five outputs, the two penalties
    assert args == largs[:17] + ["int32_t n_scales", "const float *scales"] + largs[17:] + ["double *bit_penalty", "double *sym_penalty"]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_soft.argtypes
    assert len(at) == len(args) == 26 and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else C.c_void_p)
    assert re.search(r"^#define WOFDM_SOFT_MAX_SCALES 16$", hdr, flags=re.M) and _lib.SOFT_MAX_SCALES == 16
    assert "wofdm_rx_profile_soft" in _lib.EXPORTS and hasattr(lib, "wofdm_rx_profile_soft")
    for name in ("RxProfileSoft", "SOFT_SCALES", "bit_llrs", "soft_penalties", "frame_profile_soft", "rx_profile_soft_host",
                 "rx_profile_soft_gpu", "rx_profile_soft_chunk_frames", "gmi_per_bin", "gmi_per_symbol", "gmi", "soft_for_window_file"):
        assert hasattr(W, name), name


def test_a_valid_call_reaches_the_device_and_no_further():
    everything = dict(pa_model=1, pa_ibo_db=3.0, track=1, timing=2, cfo=0.02, linewidth=1e-3, cpe_tracked=1, aci_on=1, aci_delay=7,
                      aci_level_db=10.0)
    assert _call() == -3 and "device" in _err()
    assert _call(points=({}, everything), scales=(0.3,)) == -3
    assert _call(points=[everything] * 16, scales=[2.0 ** (1 - j / 2) for j in range(16)]) == -3
    assert _call(scales=(1e-30, 1e30)) == -3                           # any finite positive scale
    assert _call(null=("h_track", "aci_active", "aci_h", "ref_power"), n_tracks=0) == -3
    for out in ("pw", "serrs", "spw", "ppw", "spen"):
        assert _call(null=(out,)) == -3, out                           # only errs and bit_penalty are needed


def test_soft_refuses_invalid_arguments():
    for name in ("scales", "bpen"):
        assert _call(null=(name,)) == -1 and "NULL" in _err(), name
    assert _call(n_scales=0) == -1 and _call(n_scales=-3) == -1 and "n_scales" in _err()
    for bad in (0.0, -1.0, -0.0, np.nan, np.inf, -np.inf):
        assert _call(scales=(1.0, bad)) == -1 and "scales[1]" in _err(), bad
        assert _call(scales=(bad,)) == -1
    # the link call's own, each before the device as well
    for name in ("cfg", "w_tx", "w_rx", "h", "snr", "errs", "points"):
        assert _call(null=(name,)) == -1, name
    assert _call(n_points=0) == -1
    assert _call(points=(dict(track=0),), null=("h_track",)) == -1
    assert _call(points=({}, dict(aci_on=1)), null=("aci_active",)) == -1
    assert _call(points=({}, dict(pa_model=1)), null=("ref_power",)) == -1
    for bad in (dict(track=-2), dict(aci_on=2), dict(reserved=(0, 0, 1, 0)), dict(cfo=np.nan), dict(linewidth=-1e-3)):
        assert _call(points=({}, bad)) == -1, bad
    assert _call(edit=LA._set("h", -1, np.nan)) == -1
    assert _call(cfg_edit=lambda c: setattr(c, "n_snr", 0)) == -1


def test_soft_refuses_what_lies_outside_its_limits():
    assert _call(scales=[1.0] * 17) == -2 and "n_scales" in _err()
    assert _call(n_scales=17) == -2
    assert _call(n_points=17, points=[{}] * 17) == -2
    B = V.make_structure("CPW", N, 32).stride
    for bad in (dict(timing=B), dict(cfo=4.5), dict(linewidth=1.5), dict(aci_delay=B), dict(pa_model=3)):
        assert _call(points=({}, bad)) == -2, bad
    assert _call(cfg_edit=lambda c: setattr(c, "n_fft", 96)) == -2
    assert _call(cfg_edit=lambda c: setattr(c, "syms_per_frame", 17)) == -2
