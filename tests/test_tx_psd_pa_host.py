"""``wofdm_tx_psd_batch_pa`` without a GPU: its place in the public header and the binding, its argument checks through the C
ABI (a valid call gets as far as the device and no further; a refused one leaves its outputs alone), and the host route
``timefreq.tx_waveform(..., pa=)``: the spectral regrowth behind the amplifier, decided here on the CPU."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -12345.678


def test_tx_psd_batch_pa_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_tx_psd_batch_pa\((.*?)\);", hdr, flags=re.M | re.S)
    assert m
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    masked = re.search(r"^int wofdm_tx_psd_batch_masked\((.*?)\);", hdr, flags=re.M | re.S)
    margs = [" ".join(a.split()) for a in masked.group(1).split(",")]
    # wofdm_tx_psd_batch_masked with three more inputs and one more output
    assert args == margs[:9] + ["int32_t n_pa", "const wofdm_pa_point *pa", "const int32_t *job_pa"] + margs[9:] + ["float *job_power"]
    assert hdr.index("} wofdm_pa_point;") < m.start()                      # (declared before its first use: the header is plain C)
    lib = _lib.load()
    at, mt = lib.wofdm_tx_psd_batch_pa.argtypes, lib.wofdm_tx_psd_batch_masked.argtypes
    assert list(at) == list(mt[:9]) + [C.c_int32, C.POINTER(_lib.PaPoint), C.c_void_p] + list(mt[9:]) + [C.c_void_p]
    assert "wofdm_tx_psd_batch_pa" in _lib.EXPORTS and hasattr(lib, "wofdm_tx_psd_batch_pa")
    doc = hdr[hdr.index("/* wofdm_tx_psd_batch_masked behind the amplifier"):m.start()]
    for text in ("-1 = none (NULL = none anywhere)", "the last ramp-down", "in a fixed order", "A job\n * without power passes through unchanged",
                 "wofdm_tx_psd_batch_masked gives for it", "job_pa entry outside"):
        assert text in doc, text
    amp = hdr[hdr.index("/* The transmitter's last stage"):hdr.index("#define WOFDM_PA_LINEAR")]
    assert "take a little\n * differently" in amp and "measures it on the device over a job's whole" in amp


def _call(n_fft=128, device=99, jobs=None, n_jobs=None, n_blocks=2, no_symbols=3, masks=1, job_mask=(0, -1), pa=None, n_pa=None,
          job_pa=(1, -1), null=(), edit=None):
    """rc of one call on small arrays; pa: the (model, ibo_db, smooth, reserved) of the table"""
    lib = _lib.load()
    jobs = [(0, 12, 8, 8), (1, 0, 0, 0)] if jobs is None else jobs
    cj = (_lib.PsdJob * max(1, len(jobs)))()
    for i, (b, cp, cs, ov) in enumerate(jobs):
        cj[i].block, cj[i].cp, cj[i].cs, cj[i].overlap = b, cp, cs, ov
    pa = [(0, 0.0, 0.0, 0), (1, 3.0, 2.0, 0), (2, 1.0, 0.0, 0)] if pa is None else pa
    cpa = (_lib.PaPoint * max(1, len(pa)))(*[_lib.PaPoint(*q) for q in pa])
    P0 = n_fft + jobs[0][1] + jobs[0][2]
    a = dict(w=np.ones(sum(n_fft + cp + cs for _, cp, cs, _ in jobs) + 1, np.float32),
             X=np.zeros((max(n_blocks, 1), max(no_symbols, 1), max(n_fft, 1), 2), np.float32),
             mask_len=np.full(max(1, masks), 2 * P0 - 1, np.int32), gains=np.ones(max(1, masks) * (2 * P0 - 1), np.float32),
             job_mask=np.array(job_mask, np.int32), job_pa=np.array(job_pa, np.int32),
             psd=np.full((max(1, len(jobs)), 8 * max(n_fft, 1)), POISON, np.float32),
             power=np.full((max(1, len(jobs)), 2), POISON, np.float32))
    if edit:
        edit(a)
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in a.items()}
    rc = lib.wofdm_tx_psd_batch_pa(n_fft, device, len(jobs) if n_jobs is None else n_jobs, None if "jobs" in null else C.addressof(cj),
                                   ptr["w"], masks, ptr["mask_len"], ptr["gains"], ptr["job_mask"], len(pa) if n_pa is None else n_pa,
                                   None if "pa" in null else cpa, ptr["job_pa"], n_blocks, no_symbols, ptr["X"], ptr["psd"],
                                   ptr["power"])
    assert (a["psd"] == np.float32(POISON)).all() and (a["power"] == np.float32(POISON)).all()      # no failed call writes its outputs
    return rc


def _last():
    return _lib.load().wofdm_last_error().decode()


def _one(model=1, ibo=3.0, smooth=2.0, reserved=0):
    return dict(pa=[(0, 0.0, 0.0, 0), (model, ibo, smooth, reserved)])


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _last()
    assert _call(device=-1) == -3
    for n in (64, 256, 512, 1024):
        assert _call(n_fft=n) == -3, n
    # no table, no job_pa, no job_power: each is optional; so are the masks
    assert _call(pa=[], n_pa=0, job_pa=(-1, -1)) == -3 and _call(n_pa=0, null=("pa",), job_pa=(-1, -1)) == -3
    assert _call(null=("job_pa",)) == -3 and _call(null=("power",)) == -3
    assert _call(masks=0, null=("mask_len", "gains", "job_mask")) == -3
    assert _call(pa=[(1, 0.0, 2.0, 0)] * 16, job_pa=(15, 0)) == -3
    for kw in (_one(ibo=-40.0), _one(ibo=60.0), _one(smooth=0.5), _one(smooth=16.0), _one(model=0, smooth=-3.0), _one(model=2, smooth=1e9)):
        assert _call(**kw) == -3, kw


def test_tx_psd_batch_pa_refuses_bad_arguments():
    # its own checks
    assert _call(n_pa=-1) == -1 and _call(null=("pa",)) == -1
    for bad in ((3, -1), (-2, 0), (0, 2 ** 31 - 1)):
        assert _call(job_pa=bad) == -1 and "amplifier index" in _last(), bad
    assert _call(pa=[], n_pa=0, job_pa=(0, -1)) == -1
    assert _call(pa=[(1, 0.0, 2.0, 0)] * 17) == -2 and "exceed" in _last()
    for bad in (np.nan, np.inf, -np.inf):
        assert _call(**_one(ibo=bad)) == -1 and _call(**_one(smooth=bad)) == -1 and _call(**_one(model=2, smooth=bad)) == -1
    for r in (1, -1):
        assert _call(**_one(reserved=r)) == -1 and "reserved" in _last()
    for s in (0.49, -2.0, 16.5):
        assert _call(**_one(smooth=s)) == -2 and "smooth" in _last(), s
    for ibo in (-40.5, 60.5, 1e9):
        assert _call(**_one(ibo=ibo)) == -2 and "ibo_db" in _last(), ibo
    for model in (3, -1):
        assert _call(**_one(model=model)) == -2 and "model" in _last(), model
    # a point no job uses is checked too
    assert _call(pa=[(0, 0.0, 0.0, 0), (1, 3.0, 2.0, 0), (1, 3.0, 99.0, 0)]) == -2
    # the checks of wofdm_tx_psd_batch_masked
    for k in ("jobs", "w", "X", "psd", "mask_len", "gains"):
        assert _call(null=(k,)) == -1, k
    for n in (32, 192, 2048, 0):
        assert _call(n_fft=n) == -2, n
    assert _call(n_jobs=0) == -1 and _call(n_blocks=0) == -1 and _call(no_symbols=0) == -1
    for job in ((2, 12, 8, 8), (0, 129, 0, 0), (0, 12, 8, -1), (0, 12, 8, (128 + 20) // 2 + 1)):
        assert _call(jobs=[job, (0, 0, 0, 0)], job_mask=(-1, -1)) == -1, job
    assert _call(job_mask=(1, -1)) == -1 and _call(job_mask=(0, 0)) == -1            # (the second job's P is another)

    def nan_gain(a):
        a["gains"][3] = np.nan
    assert _call(edit=nan_gain) == -1
    pmax = (8 * 128 + 2) // 3
    assert _call(jobs=[(0, 128, pmax + 1 - 256, 0), (1, 0, 0, 0)]) == -2 and "3 P - 2" in _last()


# ---- the host route ----

def test_tx_waveform_behind_an_amplifier():
    st = V.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(3)
    X = T.draw_symbols(64, rs, 64, 12)
    w, mask = V.tx_rc_window(st), CM.tx_mask(st.sym_len)
    x = T.tx_waveform(st, X, w, st.tail_tx, mask, guard_band=12)
    assert np.array_equal(T.tx_waveform(st, X, w, st.tail_tx, mask, guard_band=12, pa=None), x)
    assert np.array_equal(T.tx_waveform(st, X, w, st.tail_tx, mask, guard_band=12, pa=R.PaPoint(R.PA_LINEAR, 0.0)), x)
    # the back-off counts from the mean over the WHOLE waveform, the last ramp-down included
    ref = np.mean(np.abs(x) ** 2)
    q = R.PaPoint(R.PA_CLIP, 3.0)
    y = T.tx_waveform(st, X, w, st.tail_tx, mask, guard_band=12, pa=q)
    assert np.array_equal(y, R.pa_apply(x, q, ref)) and x.size == st.tail_tx + 64 * st.stride
    assert np.abs(y).max() <= R.pa_saturation(q, ref) * (1 + 1e-15) < np.abs(x).max()
    assert np.abs(np.angle(y * np.conj(x))).max() < 1e-15
    # a waveform without power passes unchanged
    z = T.tx_waveform(st, np.zeros_like(X), w, st.tail_tx, mask, guard_band=12, pa=q)
    assert z.shape == x.shape and not z.any()


@pytest.mark.parametrize("model", (R.PA_RAPP, R.PA_CLIP))
def test_regrowth_rises_as_the_back_off_falls(model):
    """the masked RC window at N = 64: the out-of-band mean of the periodogram rises monotonically as the back-off falls through
    9, 6, 3 and 0 dB, from the unamplified level on"""
    st = V.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(3)
    X = T.draw_symbols(64, rs, 64, 12)
    w, mask = V.tx_rc_window(st), CM.tx_mask(st.sym_len)

    def obr(pa):
        est = T.psd_estimate(T.tx_waveform(st, X, w, st.tail_tx, mask, guard_band=12, pa=pa), 512)
        return np.mean(np.hstack((est[:96], est[-96:])))
    levels = [obr(None)] + [obr(R.PaPoint(model, ibo, 2.0)) for ibo in (9.0, 6.0, 3.0, 0.0)]
    print("model %d: out-of-band mean unamplified and at 9, 6, 3, 0 dB: %s" % (model, ["%.3e" % v for v in levels]))
    assert all(a < b for a, b in zip(levels, levels[1:])), levels
    assert levels[-1] > 5 * levels[0]                                      # at 0 dB the mask's advantage is gone


def test_estimate_obr_and_the_job_tuple_take_the_amplifier_on_the_host():
    st = V.make_structure("wtx", 256, 32)
    rs = np.random.RandomState(5)
    X = T.draw_symbols(256, rs, 16)
    w = V.expand_tx_window(st, np.concatenate(([1.02], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))
    mask, q = CM.tx_mask(st.sym_len), R.PaPoint(R.PA_RAPP, 3.0, 2.0)
    amp, lin = T.estimate_obr(st, w, X=X, mask=mask, pa=q), T.estimate_obr(st, w, X=X, mask=mask)
    for tag, a, b, (win, ov) in zip(("opt", "rc", "cp"), amp, lin, T._obr_windows(st, w)):
        assert a["obr_" + tag] > b["obr_" + tag] and np.array_equal(a["S_" + tag], b["S_" + tag])
        assert np.array_equal(a["X_est_" + tag], T.psd_estimate(T.tx_waveform(st, X, win, ov, mask, pa=q), 2048))
    assert hasattr(W, "estimate_obr") and "pa" in T.tx_psd_batch_gpu.__doc__
