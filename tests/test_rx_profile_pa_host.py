"""``wofdm_rx_profile_pa`` without a GPU: header, binding and exports, the argument checks through the C ABI (a valid call gets as
far as the device and no further), the chunk formula, the amplifier's gain, and the fp64 mirror (``pa_gain``, ``pa_apply``,
``frame_profile_pa``, ``rx_profile_pa_host``, ``pa_ref_power``) against ``frame_profile`` / ``rx_profile_host`` /
``frame_papr``; the cases of tests/pa_cases.py meet their conditions on the mirror alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

import pa_cases as PC
import rx_profile_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_U, POISON_F = 0xA5A5A5A5A5A5A5A5, -12345.678


# ---- header, binding, exports ----

def test_rx_profile_pa_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_pa\((.*?)\);", hdr, flags=re.M | re.S)
    assert m
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["const wofdm_cfg *cfg", "int device", "const float *w_tx", "const float *w_rx", "const float *h",
                    "const float *snr_db", "const uint8_t *active", "const float *tx_mask", "int32_t n_points",
                    "const wofdm_pa_point *points", "const float *ref_power", "uint64_t *errs", "double *err_power",
                    "uint64_t *sym_errs", "double *sym_power", "double *pa_power"]
    for name, value in (("WOFDM_PA_LINEAR", 0), ("WOFDM_PA_RAPP", 1), ("WOFDM_PA_CLIP", 2), ("WOFDM_PA_MAX_POINTS", 16)):
        assert re.search(r"^#define %s +%d$" % (name, value), hdr, flags=re.M), name
    assert (_lib.PA_LINEAR, _lib.PA_RAPP, _lib.PA_CLIP, _lib.PA_MAX_POINTS) == (0, 1, 2, 16)
    assert (R.PA_LINEAR, R.PA_RAPP, R.PA_CLIP) == (0, 1, 2)
    body = hdr[hdr.index("typedef struct wofdm_pa_point {"):hdr.index("} wofdm_pa_point;")]
    fields = re.findall(r"\b(?:int32_t|float)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _lib.PaPoint._fields_] == ["model", "ibo_db", "smooth", "reserved"]
    assert C.sizeof(_lib.PaPoint) == 16
    lib = _lib.load()
    at = lib.wofdm_rx_profile_pa.argtypes
    assert len(at) == len(args) and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int and at[8] == C.c_int32
    assert at[9] == C.POINTER(_lib.PaPoint)
    assert all(t == C.c_void_p for i, t in enumerate(at) if i >= 2 and i not in (8, 9))
    assert "wofdm_rx_profile_pa" in _lib.EXPORTS and hasattr(lib, "wofdm_rx_profile_pa")
    kms = hdr[hdr.index("/* *ms = milliseconds (HIP events) the kernels of the calling thread's last successful wofdm_rx_profile or"):
              hdr.index("int wofdm_rx_profile_kernel_ms")]
    assert "wofdm_rx_profile_pa call" in kms
    doc = hdr[hdr.index("/* wofdm_rx_profile behind the power amplifier"):hdr.index("int wofdm_rx_profile_pa(")]
    for text in ("8 (S n_fft + T + [mask] S (2P-1)) + 8 n_points (n_fft + S + T)", "before the channel", "Pn with the first point",
                 "WOFDM_PA_LINEAR point gives the bits of", "leaves all five outputs as they were"):
        assert text in doc, text
    amp = hdr[hdr.index("/* The transmitter's last stage"):hdr.index("#define WOFDM_PA_LINEAR")]
    for text in ("(1 + rho^(2p))^(-1/(2p))", "(1 / rho) (1 + rho^(-2p))^(-1/(2p))", "g = 1 at r = 0", "[0.5, 16]", "[-40, 60]",
                 "the last ramp-down included", "over the symbol"):
        assert text in amp, text
    for name in ("pa_gain", "pa_apply", "frame_profile_pa", "rx_profile_pa_host", "rx_profile_pa_gpu", "rx_profile_pa_chunk_frames",
                 "pa_ref_power", "pa_for_window_file", "PaPoint", "RxProfilePa", "estimate_obr"):
        assert hasattr(W, name), name


def test_chunk_formula_of_the_header():
    for st, S, masked, points in ((V.make_structure("wtx", 1024, 56), 16, False, 2), (V.make_structure("CPW", 256, 32), 16, True, 4),
                                  (V.make_structure("wrx", 64, 8), 2, True, 16), (V.make_structure("CP", 64, 16), 2, False, 1)):
        P, N = st.sym_len, st.n_fft
        Tv = st.tail_tx + S * (P - st.tail_tx)
        per = 8 * (S * N + Tv + (S * (2 * P - 1) if masked else 0)) + 8 * points * (N + S + Tv)
        assert R.rx_profile_pa_chunk_frames(st, S, masked, points) == min(65535, (256 << 20) // per)
        assert R.rx_profile_pa_chunk_frames(st, S, masked, points) <= R.rx_profile_sync_chunk_frames(st, S, masked, points)
    # the cap: S = 2 at N = 64 without a point's waveform would hold more than 65535 frames
    st = V.make_structure("CP", 64, 16)
    assert (256 << 20) // (8 * (2 * 64 + 160)) > 65535 and R.rx_profile_chunk_frames(st, 2, False) == 65535


# ---- argument checks without a device ----

def _call(st=None, k=4, S=4, n_taps=3, n_ch=2, n_snr=2, pairs=2, frames=3, device=99, null=(), mask=False, active=None,
          n_points=3, points=None, held=None, edit=None, cfg_edit=None):
    """rc of one call on small arrays; `edit` changes the arrays, `cfg_edit` the cfg, before the call; `points`: the (model,
    ibo_db, smooth, reserved) of the table; `held`: the points the arrays hold, where the count passed is not to be believed"""
    st = V.make_structure("CPW", 128, 32) if st is None else st
    cfg = W.make_cfg(st, k, S, n_taps, n_ch, n_snr, pairs, seed=3, frames_per_cell=frames)
    P, NW, N = st.sym_len, st.n_fft + st.tail_rx, st.n_fft
    hp = max(1, n_points) if held is None else held
    if points is None:
        points = [((0, 1, 2)[i % 3], 3.0, 2.0, 0) for i in range(hp)]
    cpts = (_lib.PaPoint * len(points))(*[_lib.PaPoint(*q) for q in points])
    a = dict(w_tx=np.ones((pairs, P), np.float32), w_rx=np.ones((pairs, NW), np.float32),
             h=np.ones((n_ch, n_taps, 2), np.float32), snr=np.full(n_snr, 10.0, np.float32),
             active=None if active is None else np.ascontiguousarray(active, np.uint8),
             mask=np.ones(2 * P - 1, np.float32) if mask else None, ref=np.full(pairs, 0.01, np.float32))
    cells = pairs * n_ch * n_snr
    errs = np.full((hp, cells, N, 2), POISON_U, np.uint64)
    pw = np.full((hp, cells, N), POISON_F, np.float64)
    serrs = np.full((hp, cells, max(1, S - 1), 2), POISON_U, np.uint64)
    spw = np.full((hp, cells, max(1, S - 1)), POISON_F, np.float64)
    ppw = np.full((hp, cells, 2), POISON_F, np.float64)
    a.update(errs=errs, pw=pw, serrs=serrs, spw=spw, ppw=ppw)
    if edit:
        edit(a)
    if cfg_edit:
        cfg_edit(cfg)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_pa(None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"],
                                         ptr["snr"], ptr["active"], ptr["mask"], n_points, None if "points" in null else cpts,
                                         ptr["ref"], ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"])
    assert (errs == POISON_U).all() and (pw == POISON_F).all()          # no failed call writes its outputs
    assert (serrs == POISON_U).all() and (spw == POISON_F).all() and (ppw == POISON_F).all()
    return rc


def _set(name, index, value):
    def edit(a):
        a[name].reshape(-1)[index] = value
    return edit


def _last():
    return _lib.load().wofdm_last_error().decode()


def _one(model=1, ibo=3.0, smooth=2.0, reserved=0):
    """a three-point table whose last point is the one given"""
    return dict(points=[(0, 0.0, 0.0, 0), (2, 1.0, 99.0, 0), (model, ibo, smooth, reserved)])


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _last()
    assert _call(device=-1) == -3
    assert _call(mask=True, active=CM.half_band_allocation(128)) == -3
    assert _call(n_points=1) == -3 and _call(n_points=16) == -3
    # the limits themselves are inside; the linear point and the limiter ignore smooth
    for kw in (_one(ibo=-40.0), _one(ibo=60.0), _one(smooth=0.5), _one(smooth=16.0), _one(model=0, smooth=-3.0), _one(model=2, smooth=1e9)):
        assert _call(**kw) == -3, kw
    assert _call(edit=_set("ref", 0, 1e-38), **_one(ibo=-40.0)) == -3 and _call(edit=_set("ref", 1, 3e38), **_one(ibo=60.0)) == -3
    assert _call(st=V.make_structure("wtx", 1024, 128), S=2, mask=True) == -3
    assert _call(st=V.make_structure("wtx", 1024, 56), S=16) == -3
    assert _call(n_taps=21) == -3 and _call(S=16) == -3 and _call(S=2) == -3
    assert _call(frames=0) == -3
    for name in ("pw", "serrs", "spw", "ppw"):                              # four of the outputs are optional
        assert _call(null=(name,)) == -3, name
    assert _call(null=("pw", "serrs", "spw", "ppw")) == -3


def test_rx_profile_pa_refuses_invalid_arguments():
    for name in ("cfg", "w_tx", "w_rx", "h", "snr", "errs", "points", "ref"):
        assert _call(null=(name,)) == -1, name
    for n in (0, -1, -(2 ** 31)):
        assert _call(n_points=n) == -1 and "n_points" in _last()
    for bad in (np.nan, np.inf, -np.inf):
        assert _call(**_one(ibo=bad)) == -1 and "finite" in _last()
        assert _call(**_one(smooth=bad)) == -1 and "finite" in _last()
        assert _call(**_one(model=2, smooth=bad)) == -1                     # (ignored by the limiter, but not a number)
        assert _call(edit=_set("ref", 1, bad)) == -1 and "ref_power" in _last()
        for name in ("w_tx", "w_rx", "snr", "h"):                           # the checks of wofdm_rx_profile
            assert _call(edit=_set(name, -1, bad)) == -1, name
        assert _call(mask=True, edit=_set("mask", -1, bad)) == -1
    for bad in (0.0, -0.01, -1e30):
        assert _call(edit=_set("ref", 0, bad)) == -1 and "ref_power" in _last()
    for r in (1, -1, 2 ** 31 - 1):
        assert _call(**_one(reserved=r)) == -1 and "reserved" in _last()
    assert _call(active=np.zeros(128, np.uint8)) == -1 and "loads no subcarrier" in _last()
    for field in ("n_channels", "n_snr", "n_window_pairs"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, 0)) == -1, field
    for field in ("cp", "cs", "tail_tx", "prefix_rm", "circ_shift", "n_taps"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, -1)) == -1, field


def test_rx_profile_pa_refuses_what_lies_outside_its_limits():
    for n in (17, 64, 2 ** 31 - 1):
        assert _call(n_points=n, held=1) == -2 and "exceed" in _last(), n
    for s in (0.49, 0.0, -2.0, 16.5, 1e9):
        assert _call(**_one(smooth=s)) == -2 and "smooth" in _last(), s
    for ibo in (-40.5, -1e9, 60.5, 1e9):
        assert _call(**_one(ibo=ibo)) == -2 and "ibo_db" in _last(), ibo
    for model in (3, -1, 2 ** 31 - 1):
        assert _call(**_one(model=model)) == -2 and "model" in _last(), model
    # what wofdm_rx_profile refuses
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


# ---- the amplifier's gain ----

def test_gain_at_rest_below_saturation_and_in_the_limit():
    rho = np.concatenate(([0.0], np.logspace(-6, 6, 241)))
    for model, p in ((R.PA_LINEAR, 2.0), (R.PA_CLIP, 2.0)) + tuple((R.PA_RAPP, p) for p in (0.5, 1.0, 2.0, 3.0, 16.0)):
        g = R.pa_gain(model, rho, p)
        assert g.shape == rho.shape and np.isfinite(g).all() and g[0] == 1.0 and (g > 0).all() and (g <= 1.0).all(), (model, p)
        if model == R.PA_LINEAR:
            assert (g == 1.0).all()
            continue
        # |y| = g rho a_sat stays below a_sat -- the Rapp curve strictly, up to where 1 + rho^(-2p) rounds to 1; the limiter
        # reaches it: g rho = rho fl(1 / rho), a_sat within an ulp -- and grows with rho
        out = g * rho
        assert (out <= 1.0 + 2.0 ** -52).all(), (model, p)
        if model == R.PA_RAPP:
            assert (out[rho ** (2 * p) < 1e15] < 1.0).all(), p
        assert (np.diff(out) >= -2.0 ** -52).all(), (model, p)
    # deep saturation: rho = 1e4 with p = 16 is rho^(2p) = 1e128 -- and rho = 1e300 beyond any power --, no overflow, no NaN
    with np.errstate(over="raise", invalid="raise", divide="raise"):           # (rho^(-2p) may underflow to 0: harmless)
        for r in (1e4, 1e20, 1e300):
            g = float(R.pa_gain(R.PA_RAPP, r, 16.0))
            assert abs(g * r - 1.0) <= 2.0 ** -51, r
        assert float(R.pa_gain(R.PA_RAPP, 1e-300, 16.0)) == 1.0 and float(R.pa_gain(R.PA_RAPP, 1e-300, 0.5)) == 1.0
    # the closed form where it does not overflow, both sides of rho = 1
    for p in (0.5, 2.0, 16.0):
        r = np.array([0.3, 0.999, 1.0, 1.001, 3.0])
        assert np.abs(R.pa_gain(R.PA_RAPP, r, p) / (1.0 + r ** (2 * p)) ** (-0.5 / p) - 1).max() < 1e-14, p
    # Rapp tends to the limiter as p grows: sup |g_p - g_clip| = 1 - 2^(-1/(2p)) at rho = 1, falling in p
    dev = [np.abs(R.pa_gain(R.PA_RAPP, rho, p) - R.pa_gain(R.PA_CLIP, rho)).max() for p in (1.0, 2.0, 4.0, 8.0, 16.0)]
    assert all(a > b for a, b in zip(dev, dev[1:])) and dev[-1] <= 1.0 - 2.0 ** (-1.0 / 32.0) + 1e-15
    with pytest.raises(ValueError):
        R.pa_gain(7, rho)


def test_pa_apply_keeps_the_phase_and_counts_the_back_off_from_the_reference():
    rs = np.random.RandomState(1)
    x = (rs.randn(4000) + 1j * rs.randn(4000)) * np.exp(rs.uniform(-6, 1, 4000))
    ref = float(np.mean(np.abs(x) ** 2))
    for q in (R.PaPoint(R.PA_RAPP, 3.0, 2.0), R.PaPoint(R.PA_RAPP, -20.0, 16.0), R.PaPoint(R.PA_CLIP, 0.0), (1, 6.0, 0.5)):
        y = R.pa_apply(x, q, ref)
        a_sat = R.pa_saturation(q, ref)
        assert a_sat == np.float32(np.sqrt(ref * 10.0 ** (0.1 * R.PaPoint(*q).ibo_db)))        # stored in single precision
        assert np.abs(np.angle(y * np.conj(x))).max() < 1e-15                                   # the phase is kept
        assert (np.abs(y) <= np.abs(x)).all() and (np.abs(y) <= a_sat * (1 + 1e-15)).all()
        assert np.abs(y).max() > 0.5 * min(a_sat, np.abs(x).max())
    assert R.pa_apply(x, R.PaPoint(R.PA_LINEAR, -40.0), ref) is not None
    assert np.array_equal(R.pa_apply(x, R.PaPoint(R.PA_LINEAR, -40.0), ref), x)
    assert np.array_equal(R.pa_apply(np.zeros(5), R.PaPoint(R.PA_RAPP, 0.0, 1.0), 1.0), np.zeros(5))
    # 60 dB of back-off is all but linear
    assert np.abs(R.pa_apply(x, R.PaPoint(R.PA_CLIP, 60.0), ref) - x).max() == 0.0
    for bad in ((3, 0.0, 2.0), (1, 61.0, 2.0), (1, 0.0, 0.4), (1, 0.0, 17.0)):
        with pytest.raises(ValueError):
            R.pa_apply(x, bad, ref)


# ---- the mirror ----

@pytest.mark.parametrize("n_fft,system,variant,nbt", ((64, "wtx", "half", 1), (128, "CPW", "half_masked", 0),
                                                      (64, "wrx", "plain", 1)))
def test_mirror_on_a_linear_point_is_frame_profile(n_fft, system, variant, nbt):
    cp, S, k = RC.shape_of(n_fft, system, variant)
    c = RC.make_case(W.make_structure(system, n_fft, cp), k, S, variant, 11, nbt)
    st = c["st"]
    on = np.ones(n_fft, bool) if c["active"] is None else c["active"]
    nl = R._noise_len(st, S, c["h"].shape[1], nbt)
    grid = T.qam_table(k)[R.gen_labels(n_fft, k, S, 9, 3, 1)] * on[None, :]
    noise = R.gen_noise(nl, 9, 3, 1)
    front = (st, grid, noise, c["w_tx"][1], c["w_rx"][1], c["h"][0])
    tail = (c["snr"][1], k, c["active"], c["mask"], nbt)
    want = R.frame_profile(*front, *tail)
    x = T.tx_waveform(st, grid.T, np.asarray(c["w_tx"][1], np.float64), st.tail_tx, c["mask"], guard_band=None)
    ref = float(np.mean(np.abs(x) ** 2))
    got = R.frame_profile_pa(*front, R.PaPoint(R.PA_LINEAR, 3.0), ref, *tail)
    assert len(got) == 9 and len(want) == 5
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert got[5].sum() == want[0].sum() > 0 and got[6].sum() == want[1].sum() and got[7].sum() == pytest.approx(want[2].sum(), rel=1e-12)
    assert got[8][0] == got[8][1] == (np.abs(x) ** 2).sum()
    # an amplified point is another result, gives power away, and with_y adds Y
    amp = R.frame_profile_pa(*front, R.PaPoint(R.PA_RAPP, 3.0, 2.0), ref, *tail, with_y=True)
    assert len(amp) == 10 and amp[9].shape == (S, n_fft) and not np.array_equal(amp[2], want[2])
    assert amp[8][0] == got[8][0] and amp[8][1] == (np.abs(R.pa_apply(x, (1, 3.0, 2.0), ref)) ** 2).sum() < amp[8][0]
    # at 60 dB of back-off the limiter is the linear point, exactly
    far = R.frame_profile_pa(*front, R.PaPoint(R.PA_CLIP, 60.0), ref, *tail)
    for g, w in zip(far, got):
        assert np.array_equal(g, w)
    # and the host route is its frames added up: the linear point of a call is rx_profile_host, whatever shares the call
    pts = [R.PaPoint(R.PA_CLIP, 2.0), R.PaPoint(R.PA_LINEAR, 0.0)]
    refs = np.array([ref, 1.3 * ref], np.float32)
    args = (st, k, S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 9, 0, 2)
    kw = dict(active=c["active"], mask=c["mask"], noise_before_truncate=nbt, with_near=True)
    a, near = R.rx_profile_pa_host(*args, pts, refs, **kw)
    b, near_b = R.rx_profile_host(*args, **kw)
    assert a.bit_err.shape == (2,) + b.bit_err.shape and a.pa_power.shape == (2,) + b.bit_err.shape[:-1] + (2,)
    assert np.array_equal(a.bit_err[1], b.bit_err) and np.array_equal(a.sym_err[1], b.sym_err)
    assert np.array_equal(a.err_power[1], b.err_power) and np.array_equal(a.decisions, b.decisions)
    assert np.array_equal(near[1], near_b) and not np.array_equal(a.err_power[0], b.err_power)
    assert np.array_equal(a.bit_err_sym.sum(axis=-1), a.bit_err.sum(axis=-1))
    assert np.array_equal(a.sym_err_sym.sum(axis=-1), a.sym_err.sum(axis=-1))
    tab = T.qam_table(k)
    for cell, i in ((0, 0), (5, 1)):
        p, s, ch = cell // 4, (cell // 2) % 2, cell % 2
        acc = [np.zeros(n_fft, np.uint64), np.zeros(n_fft), np.zeros(2)]
        for f in range(2):
            one = R.frame_profile_pa(st, tab[R.gen_labels(n_fft, k, S, 9, cell, f)] * on[None, :], R.gen_noise(nl, 9, cell, f),
                                     c["w_tx"][p], c["w_rx"][p], c["h"][ch], pts[i], refs[p], c["snr"][s], k, c["active"], c["mask"], nbt)
            acc[0] += one[0]
            acc[1] += one[2]
            acc[2] += one[8]
        assert np.array_equal(a.bit_err[i, p, s, ch], acc[0]) and np.array_equal(a.err_power[i, p, s, ch], acc[1])
        assert np.array_equal(a.pa_power[i, p, s, ch], acc[2])


def test_pa_ref_power_on_the_host_is_the_mean_of_the_period_energies():
    st = V.make_structure("CPW", 64, 16)
    rs = np.random.RandomState(2)
    w = np.stack([V.tx_rc_window(st), V.tx_rc_window(st) * rs.uniform(0.8, 1.2)])
    alloc, mask = CM.half_band_allocation(64), CM.tx_mask(st.sym_len)
    k, S, seed, f0, frames = 4, 5, 77, 3, 6
    for m in (None, mask):
        got = R.pa_ref_power(st, k, S, w, seed, f0, frames, active=alloc, mask=m, gpu=False)
        assert got.shape == (2,) and got.dtype == np.float64
        for p in range(2):
            grids = np.stack([T.qam_table(k)[R.gen_labels(64, k, S, seed, p, f0 + f)] * alloc[None, :] for f in range(frames)])
            per = T.frame_papr(st, grids, w[p].astype(np.float32), None if m is None else m.astype(np.float32))
            assert got[p] == pytest.approx(per[..., 1].mean() / st.stride, rel=1e-14)
        assert 0.3 / 64 < got[0] < 0.7 / 64                                 # unit-power symbols on half of the bins: some 0.5 / N


@pytest.mark.parametrize("name", list(PC.CASES))
def test_the_cases_meet_their_conditions_on_the_mirror(name):
    """what tests/pa_cases.py promises, decided here on the CPU: errors in every cell, fewer than half of a point's decisions
    wrong, every amplified point another result in every cell, at most 1 % near decisions on every point"""
    c, seed, prof, near = PC.reference(name)
    assert len(c["points"]) == 3 and [q.model for q in c["points"]] == [R.PA_LINEAR, R.PA_RAPP, R.PA_CLIP] and c["points"][1].smooth == 2.0
    PC.check_error_rates(c, prof, RC.FRAMES, name)
    assert (near.sum(axis=(1, 2, 3)) <= 0.01 * PC.decisions_of(c, RC.FRAMES)).all()
    assert np.array_equal(prof.pa_power[0, ..., 0], prof.pa_power[0, ..., 1])
    # the linear point is the plain mirror
    plain = R.rx_profile_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, 0, RC.FRAMES, active=c["active"],
                              mask=c["mask"], noise_before_truncate=c["nbt"])
    assert np.array_equal(prof.bit_err[0], plain.bit_err) and np.array_equal(prof.err_power[0], plain.err_power)
