"""``wofdm_tx_psd_batch_pa`` on the GPU (the waveform kernels of wofdm_tx_psd_batch_masked, wofdm_pa_job_power_kernel,
wofdm_pa_job_apply_kernel, then the periodogram kernels) against the fp64 host mirror ``timefreq.tx_waveform(..., pa=)`` +
``psd_estimate`` -- never against the GPU path itself.

Tolerances as tests/test_gpu_tx_psd_masked.py: periodogram within 2e-5 of its peak (PSD_RTOL), Parseval 1e-5 relative, OBR
figure 2e-4 relative, repeated calls bit-exact.  job_power against the host's two means under 1e-5 relative, Parseval's bound:
both are sums of squares of the same fp32 samples.  Unamplified jobs and jobs with a linear point give the bytes of
``wofdm_tx_psd_batch_masked``."""
import numpy as np
import pytest

from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

import test_gpu_tx_psd_masked as TM

pytestmark = pytest.mark.gpu

PSD_RTOL = TM.PSD_RTOL
IBOS = (9.0, 3.0, 0.0)


def check_job(got_raw, power, st, X, w, ov, mask, pa, n, tag):
    """one job's undivided slice sums against the mirror: periodogram, Parseval (on the amplified waveform), OBR; job_power"""
    fl = 8 * n
    w32, m32 = np.asarray(w, np.float32), None if mask is None else np.asarray(mask, np.float32)
    x = T.tx_waveform(st, X, w32, ov, m32, guard_band=TM.guard(n))
    y = T.tx_waveform(st, X, w32, ov, m32, guard_band=TM.guard(n), pa=pa)
    want = T.psd_estimate(y, fl) * (y.size // fl + 1)
    g = got_raw.astype(np.float64)
    err = np.abs(g - want).max() / want.max()
    par = abs(g.sum() / (fl * (np.abs(y) ** 2).sum()) - 1)
    ratio = abs(TM.obr(g, n) / TM.obr(want, n) - 1)
    pin, pout = np.mean(np.abs(x) ** 2), np.mean(np.abs(y) ** 2)
    dp = max(abs(power[0] / pin - 1), abs(power[1] / pout - 1))
    print("%s: psd %.2e of the peak, Parseval %.2e, OBR %.2e (level %.1e of the peak), job_power %.2e, out / in %.4f"
          % (tag, err, par, ratio, TM.obr(want, n) / want.max(), dp, pout / pin))
    assert err < PSD_RTOL, (tag, err)
    assert par < 1e-5, (tag, par)
    assert ratio < 2e-4, (tag, ratio)
    assert dp < 1e-5, (tag, dp, power, pin, pout)
    return want


def job_set(n, S, seed):
    """plain and masked (the reference's mask), unamplified, linear, and Rapp p = 2 and soft limiter at three back-offs"""
    st = V.make_structure("wtx", n, n // 8)
    rs = np.random.RandomState(seed)
    w = TM.random_window(rs, st)
    X = T.draw_symbols(n, rs, S, TM.guard(n))
    pas = [None, R.PaPoint(R.PA_LINEAR, 3.0)] + [R.PaPoint(m, ibo, 2.0) for ibo in IBOS for m in (R.PA_RAPP, R.PA_CLIP)]
    jobs = [(0, st.cp, st.cs, st.tail_tx, w, m, pa) for m in (None, CM.tx_mask(st.sym_len)) for pa in pas]
    return st, X, w, jobs


@pytest.mark.parametrize("n_fft,S", [(64, 16), (256, 12), (1024, 8)])
def test_amplified_periodogram_and_obr_against_the_mirror(n_fft, S):
    n = n_fft
    st, X, w, jobs = job_set(n, S, 40 + n)
    grid = T._full_grid(n, X, TM.guard(n))[None]
    got, power = T.tx_psd_batch_gpu(n, grid, jobs, divide=False, power=True)
    assert got.shape == (16, 8 * n) and power.shape == (16, 2) and power.dtype == np.float32
    obrs = {}
    for i, j in enumerate(jobs):
        tag = "N=%d S=%d %s %s" % (n, S, "masked" if j[5] is not None else "plain", j[6])
        want = check_job(got[i], power[i], st, X, w, j[3], j[5], j[6], n, tag)
        obrs[(j[5] is not None, j[6])] = TM.obr(want, n)
    # unamplified and linear jobs: the bytes of wofdm_tx_psd_batch_masked, and no power given away
    base = T.tx_psd_batch_gpu(n, grid, [j[:6] for j in jobs], divide=False)
    for i, j in enumerate(jobs):
        if j[6] is None or j[6].model == R.PA_LINEAR:
            assert got[i].tobytes() == base[i].tobytes(), i
            assert power[i, 0] == power[i, 1]
        elif j[6].model == R.PA_RAPP:                                       # (the limiter at 9 dB may meet no peak in a short run)
            assert power[i, 1] < power[i, 0] and not np.array_equal(got[i], base[i])
        else:
            assert power[i, 1] <= power[i, 0]
    assert np.array_equal(power[:8, 0], np.repeat(power[0, 0], 8)) and np.array_equal(power[8:, 0], np.repeat(power[8, 0], 8))
    # regrowth (the mirror's figures): behind either amplifier the masked waveform's out-of-band level rises as the back-off
    # falls, from the unamplified level on.  (The plain waveform's is the window's own sidelobes: compression gives power
    # away there too, and the level may fall.)
    for model in (R.PA_RAPP, R.PA_CLIP):
        lv = [obrs[(True, R.PaPoint(model, ibo, 2.0))] for ibo in IBOS]
        assert obrs[(True, None)] <= lv[0] < lv[1] < lv[2], (model, lv)
    # repeated calls are identical, the powers included
    again, power2 = T.tx_psd_batch_gpu(n, grid, jobs, divide=False, power=True)
    assert got.tobytes() == again.tobytes() and power.tobytes() == power2.tobytes()


def test_a_call_without_amplifiers_is_the_masked_call_and_measures_the_power():
    """power=True alone goes through the new entry point: job_pa NULL, no table"""
    n = 256
    st, X, w, jobs = job_set(n, 9, 7)
    grid = T._full_grid(n, X, TM.guard(n))[None]
    bare = [j[:6] for j in jobs[::8]]
    got, power = T.tx_psd_batch_gpu(n, grid, bare, divide=False, power=True)
    assert got.tobytes() == T.tx_psd_batch_gpu(n, grid, bare, divide=False).tobytes()
    for i, j in enumerate(bare):
        x = T.tx_waveform(st, X, np.asarray(w, np.float32), j[3], None if j[5] is None else np.asarray(j[5], np.float32),
                          guard_band=TM.guard(n))
        assert abs(power[i, 0] / np.mean(np.abs(x) ** 2) - 1) < 1e-5 and power[i, 0] == power[i, 1]


def test_a_job_without_power_passes_through():
    n = 64
    st = V.make_structure("wtx", n, 8)
    w = V.tx_rc_window(st)
    grid = np.zeros((1, 8, n), np.complex64)
    got, power = T.tx_psd_batch_gpu(n, grid, [(0, st.cp, st.cs, st.tail_tx, w, None, R.PaPoint(R.PA_RAPP, 0.0, 2.0))], divide=False,
                                    power=True)
    assert not got.any() and not power.any()


@pytest.mark.parametrize("n_fft", [256, 1024])
def test_estimate_obr_behind_the_amplifier_matches_the_host_route(n_fft):
    st = V.make_structure("wtx", n_fft, 32)
    rs = np.random.RandomState(n_fft + 1)
    w_tx = TM.random_window(rs, st)
    X = T.draw_symbols(n_fft, rs, 16)
    mask = CM.tx_mask(st.sym_len)
    pa = R.PaPoint(R.PA_RAPP, 3.0, 2.0)
    gpu = T.estimate_obr(st, w_tx, X=X, mask=mask, pa=pa, gpu=True)
    cpu = T.estimate_obr(st, w_tx, X=X, mask=mask, pa=pa)
    linear = T.estimate_obr(st, w_tx, X=X, mask=mask)
    for tag, g, c, u in zip(("opt", "rc", "cp"), gpu, cpu, linear):
        assert np.abs(g["X_est_" + tag] - c["X_est_" + tag]).max() < PSD_RTOL * c["X_est_" + tag].max(), tag
        print("estimate_obr N=%d %s: OBR %.3e (linear %.3e), GPU off by %.2e" % (n_fft, tag, c["obr_" + tag], u["obr_" + tag],
                                                                              abs(g["obr_" + tag] / c["obr_" + tag] - 1)))
        assert abs(g["obr_" + tag] / c["obr_" + tag] - 1) < 2e-4, tag
        assert c["obr_" + tag] > u["obr_" + tag], tag                       # regrowth
