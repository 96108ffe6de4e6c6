"""wofdm_rx_profile_link without a GPU: its place in the public header and the binding, and its argument checks -- every
WOFDM_E_INVALID / WOFDM_E_UNSUPPORTED condition of include/wofdm.h (the union of the five arms', each with the code its own arm
gives it) is answered before the device is touched (this machine has none: a call that passes the checks ends in WOFDM_E_HIP),
and a failed call leaves the five outputs as they were."""
import ctypes as C
import os
import re

import numpy as np

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_U, POISON_F = 0xA5A5A5A5A5A5A5A5, -12345.678
OK_POINT = dict(pa_model=0, pa_ibo_db=0.0, pa_smooth=2.0, track=-1, timing=0, cfo=0.0, cfo_tracked=1, linewidth=0.0, cpe_tracked=0,
                aci_on=0, aci_delay=0, aci_level_db=0.0)
N, S, TAPS, N_CH, N_SNR, PAIRS = 128, 4, 3, 2, 2, 2


def _call(points=({},), null=(), n_points=None, n_tracks=2, n_knots=None, knot_step=None, edit=None, cfg_edit=None, device=99):
    """rc of one call on small arrays.  points: per point the fields that differ from OK_POINT ("reserved": the four words);
    null: the arguments passed as NULL; `edit` changes the arrays, `cfg_edit` the cfg, before the call"""
    st = V.make_structure("CPW", N, 32)
    cfg = W.make_cfg(st, 4, S, TAPS, N_CH, N_SNR, PAIRS, seed=3, frames_per_cell=3)
    B, P = st.stride, st.sym_len
    n_knots = S + 2 if n_knots is None else n_knots
    knot_step = B if knot_step is None else knot_step
    a = dict(w_tx=np.ones((PAIRS, P), np.float32), w_rx=np.ones((PAIRS, N + st.tail_rx), np.float32),
             h=np.ones((N_CH, TAPS, 2), np.float32), snr=np.full(N_SNR, 10.0, np.float32), active=None, mask=None,
             h_track=np.ones((max(n_tracks, 1), N_CH, max(n_knots, 2), TAPS, 2), np.float32),
             aci_active=np.ones(N, np.uint8), aci_h=np.ones((N_CH, TAPS, 2), np.float32), ref_power=np.ones(PAIRS, np.float32))
    cpts = (_lib.LinkPoint * max(len(points), 1))()
    for q, over in zip(cpts, points):
        for f, v in dict(OK_POINT, **over).items():
            if f == "reserved":
                q.reserved = (C.c_int32 * 4)(*v)
            else:
                setattr(q, f, v)
    NP, cells = max(len(points), 1), PAIRS * N_CH * N_SNR
    outs = dict(errs=np.full((NP, cells, N, 2), POISON_U, np.uint64), pw=np.full((NP, cells, N), POISON_F, np.float64),
                serrs=np.full((NP, cells, S - 1, 2), POISON_U, np.uint64), spw=np.full((NP, cells, S - 1), POISON_F, np.float64),
                ppw=np.full((NP, cells, 2), POISON_F, np.float64))
    a.update(outs)
    if edit:
        edit(a)
    if cfg_edit:
        cfg_edit(cfg)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_link(
        None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], n_tracks, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"],
        len(points) if n_points is None else n_points, None if "points" in null else cpts,
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"])
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_F)).all(), n
    return rc


def _set(name, index, value):
    def edit(a):
        a[name].reshape(-1)[index] = value
    return edit


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_link_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_link\((.*?)\);", hdr, flags=re.M | re.S)
    assert m
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["const wofdm_cfg *cfg", "int device", "const float *w_tx", "const float *w_rx", "const float *h",
                    "const float *snr_db", "const uint8_t *active", "const float *tx_mask", "const float *h_track",
                    "int32_t n_tracks", "int32_t n_knots", "int32_t knot_step", "const uint8_t *aci_active", "const float *aci_h",
                    "const float *ref_power", "int32_t n_points", "const wofdm_link_point *points", "uint64_t *errs",
                    "double *err_power", "uint64_t *sym_errs", "double *sym_power", "double *pa_power"]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_link.argtypes
    assert len(at) == len(args) and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else C.c_void_p)
    # the struct: the header's fields in the header's order, 64 bytes
    body = re.search(r"typedef struct wofdm_link_point \{(.*?)\} wofdm_link_point;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|float)\s+(\w+)(\[4\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [f[1] for f in fields] == [f[0] for f in _lib.LinkPoint._fields_]
    for (ctype, _, arr), (_, pyt) in zip(fields, _lib.LinkPoint._fields_):
        assert pyt == (C.c_int32 * 4 if arr else C.c_int32 if ctype == "int32_t" else C.c_float)
    assert C.sizeof(_lib.LinkPoint) == 64
    assert re.search(r"^#define WOFDM_LINK_MAX_POINTS 16$", hdr, flags=re.M) and _lib.LINK_MAX_POINTS == 16
    assert "wofdm_rx_profile_link" in _lib.EXPORTS and hasattr(lib, "wofdm_rx_profile_link")
    for name in ("LinkPoint", "RxProfileLink", "frame_profile_link", "rx_profile_link_host", "rx_profile_link_gpu",
                 "rx_profile_link_chunk_frames", "link_for_window_file"):
        assert hasattr(W, name)


def test_a_valid_call_reaches_the_device_and_no_further():
    everything = dict(pa_model=1, pa_ibo_db=3.0, track=1, timing=2, cfo=0.02, linewidth=1e-3, cpe_tracked=1, aci_on=1, aci_delay=7,
                      aci_level_db=10.0)
    assert _call() == -3 and "device" in _err()
    assert _call(points=({}, everything, dict(timing=-3, cfo=-4.0, cfo_tracked=0))) == -3
    assert _call(points=[everything] * 16) == -3
    # what no point uses may be NULL, the knot integers anything
    assert _call(null=("h_track", "aci_active", "aci_h", "ref_power"), n_tracks=0, n_knots=0, knot_step=0) == -3
    assert _call(points=(dict(aci_on=1),), null=("aci_h", "h_track", "ref_power")) == -3
    assert _call(points=(dict(track=0),), null=("aci_active", "ref_power")) == -3
    assert _call(points=(dict(pa_model=2),), null=("aci_active", "h_track")) == -3
    for out in ("pw", "serrs", "spw", "ppw"):
        assert _call(null=(out,)) == -3, out                          # only errs is needed
    # the largest timing the knots of S + 2 = 6 steps of B cover: (S + 1) B - (tail_tx + S B + n_taps - 2)
    st = V.make_structure("CPW", N, 32)
    room = st.stride - st.tail_tx - TAPS + 2
    assert 0 < room < st.stride
    assert _call(points=(dict(track=0, timing=room),)) == -3
    assert _call(points=(dict(track=0), dict(timing=room + 1))) == -1 and "largest positive timing" in _err()
    assert _call(points=(dict(timing=room + 1),)) == -3                # (no point names a track: no knots to cover anything)


def test_link_refuses_invalid_arguments():
    for name in ("cfg", "w_tx", "w_rx", "h", "snr", "errs", "points"):
        assert _call(null=(name,)) == -1, name
    assert _call(n_points=0) == -1 and _call(n_points=-1) == -1
    # a needed argument that is NULL
    assert _call(points=(dict(track=0),), null=("h_track",)) == -1
    assert _call(points=({}, dict(aci_on=1)), null=("aci_active",)) == -1
    assert _call(points=({}, dict(pa_model=1)), null=("ref_power",)) == -1
    # the points' own fields
    for bad in (dict(track=-2), dict(track=2), dict(aci_on=2), dict(aci_on=-1), dict(aci_delay=-1), dict(aci_level_db=np.nan),
                dict(aci_level_db=np.inf), dict(aci_level_db=800.0), dict(reserved=(0, 0, 1, 0)), dict(reserved=(7, 0, 0, 0)),
                dict(cfo=np.nan), dict(cfo_tracked=2), dict(linewidth=-1e-3), dict(linewidth=np.nan), dict(cpe_tracked=-1),
                dict(pa_ibo_db=np.inf), dict(pa_smooth=np.nan)):
        assert _call(points=({}, bad)) == -1, bad
    # the side arrays
    for bad in (np.nan, np.inf):
        assert _call(edit=_set("h", -1, bad)) == -1
        assert _call(points=(dict(track=0),), edit=_set("h", 0, bad)) == -1            # (h is read beside the tracks)
        assert _call(points=(dict(track=1),), edit=_set("h_track", -1, bad)) == -1
        assert _call(points=(dict(aci_on=1),), edit=_set("aci_h", -1, bad)) == -1
        assert _call(points=(dict(pa_model=1),), edit=_set("ref_power", -1, bad)) == -1
    assert _call(points=(dict(pa_model=1),), edit=_set("ref_power", 0, 0.0)) == -1
    # the knots
    assert _call(points=(dict(track=0),), n_tracks=0) == -1
    assert _call(points=(dict(track=0),), n_knots=1) == -1
    assert _call(points=(dict(track=0),), knot_step=0) == -1
    assert _call(points=(dict(track=0),), n_knots=S + 1) == -1 and "knots end" in _err()
    # wofdm_rx_profile's own
    assert _call(cfg_edit=lambda c: setattr(c, "n_snr", 0)) == -1
    assert _call(edit=lambda a: a.update(active=np.zeros(N, np.uint8))) == -1 and "loads no subcarrier" in _err()


def test_link_refuses_what_lies_outside_its_limits():
    st = V.make_structure("CPW", N, 32)
    B = st.stride
    assert _call(n_points=17, points=[{}] * 17) == -2
    for bad in (dict(timing=B), dict(timing=-B), dict(cfo=4.5), dict(cfo=-4.5), dict(linewidth=1.5), dict(aci_delay=B),
                dict(pa_model=3), dict(pa_model=-1), dict(pa_model=1, pa_ibo_db=61.0), dict(pa_model=1, pa_ibo_db=-41.0),
                dict(pa_model=1, pa_smooth=0.4), dict(pa_model=1, pa_smooth=17.0)):
        assert _call(points=({}, bad)) == -2, bad
    assert _call(points=(dict(timing=B - 1),)) == -3 and _call(points=(dict(aci_on=1, aci_delay=B - 1),)) == -3
    assert _call(points=(dict(track=0),), n_tracks=17) == -2
    assert _call(points=(dict(track=0),), n_knots=65) == -2
    assert _call(cfg_edit=lambda c: setattr(c, "n_fft", 96)) == -2
    assert _call(cfg_edit=lambda c: setattr(c, "syms_per_frame", 17)) == -2
