"""``wofdm_tx_psd_batch_masked`` on the GPU (wofdm_txmask_batch_kernel<N> + wofdm_txmask_ola_kernel<N>, then the
periodogram kernels of wofdm_tx_psd_batch) against the fp64 host mirror ``timefreq.tx_waveform`` +
``psd_estimate`` -- never against the GPU path itself.

Tolerances as tests/test_gpu_aux_kernels.py / test_gpu_tx_psd_batch.py: periodogram within 2e-5 of its peak
(PSD_RTOL), Parseval 1e-5 relative, OBR figure 2e-4 relative, repeated calls bit-exact.  Every masked case asserts
the OBR ratio too: at N = 1024 the masked out-of-band level is about 3e-5 of the peak, the size of PSD_RTOL itself,
so the peak-relative check alone says nothing about the masked band.

Symbols are ``draw_symbols``' 16-QAM with the guard band of ``estimate_obr`` (48) where N allows it (N >= 256) and
the same fraction of the band, 3 N / 16, below; the OBR figure is ``estimate_obr``'s mean over the guard-band bins
of the 8 N grid."""
import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

pytestmark = pytest.mark.gpu

PSD_RTOL = 2e-5
NS = [64, 128, 256, 512, 1024]


def guard(n):
    return T.GUARD_BAND if n >= 256 else 3 * n // 16


def obr(est, n):
    gb = 8 * guard(n)
    return np.mean(np.hstack((est[:gb], est[-gb:])))


def random_window(rs, st):
    if not st.tail_tx:
        return np.ones(st.sym_len)
    return V.expand_tx_window(st, np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1])))


class Geo:
    def __init__(self, n, cp, cs):
        self.n_fft, self.cp, self.cs, self.sym_len = n, cp, cs, n + cp + cs


def check_job(got_raw, st, X, w, ov, mask, n, tag, gb="default"):
    """one job's undivided slice sums against the mirror: periodogram, Parseval, OBR"""
    gb = guard(n) if gb == "default" else gb
    fl = 8 * n
    x = T.tx_waveform(st, X, np.asarray(w, np.float32), ov, None if mask is None else np.asarray(mask, np.float32), guard_band=gb)
    assert x.size == ov + X.shape[1] * (st.sym_len - ov)
    want = T.psd_estimate(x, fl) * (x.size // fl + 1)
    g = got_raw.astype(np.float64)
    err = np.abs(g - want).max() / want.max()
    par = abs(g.sum() / (fl * (np.abs(x) ** 2).sum()) - 1)
    ratio = abs(obr(g, n) / obr(want, n) - 1)
    print("%s: psd %.2e of the peak, Parseval %.2e, OBR %.2e (level %.1e of the peak)"
          % (tag, err, par, ratio, obr(want, n) / want.max()))
    assert err < PSD_RTOL, (tag, err)
    assert par < 1e-5, (tag, par)
    assert ratio < 2e-4, (tag, ratio)
    return want


@pytest.mark.parametrize("system", ["wtx", "CPW", "wrx"])
@pytest.mark.parametrize("n_fft", NS)
def test_masked_periodogram_and_obr_against_the_mirror(n_fft, system):
    """The reference's mask (tx_mask(P), roll-off 10), a random positive mask (gains in [0.2, 1.2]) and the all-ones
    mask, overlaps tail_tx and 0, runs of 1, 2 and 300 symbols; one call per run length holds the masked jobs and
    the unmasked job of each overlap.  The all-ones job agrees with the unmasked job of the same call."""
    n = n_fft
    st = V.make_structure(system, n, n // 8)
    P = st.sym_len
    rs = np.random.RandomState(n + len(system))
    w = random_window(rs, st)
    masks = {"ref": CM.tx_mask(P), "rand": rs.uniform(0.2, 1.2, 2 * P - 1), "ones": np.ones(2 * P - 1)}
    for S in (1, 2, 300):
        X = T.draw_symbols(n, rs, S, guard(n))
        grid = T._full_grid(n, X, guard(n))
        overlaps = sorted({st.tail_tx, 0})
        jobs = [(0, st.cp, st.cs, ov, w, m) for ov in overlaps for m in list(masks.values()) + [None]]
        got = T.tx_psd_batch_gpu(n, grid[None], jobs, divide=False)
        for k, ov in enumerate(overlaps):
            for i, name in enumerate(masks):
                check_job(got[4 * k + i], st, X, w, ov, masks[name], n, "N=%d %s S=%d ov=%d %s" % (n, system, S, ov, name))
            plain = check_job(got[4 * k + 3], st, X, w, ov, None, n, "N=%d %s S=%d ov=%d unmasked" % (n, system, S, ov))
            assert np.abs(got[4 * k + 2].astype(np.float64) - got[4 * k + 3]).max() < PSD_RTOL * plain.max(), (S, ov)


@pytest.mark.parametrize("n_fft", NS)
def test_masked_waveform_ending_on_a_slice_boundary(n_fft):
    """cp = N / 4, no overlap, 32 symbols: 40 N samples, exactly five slices of 8 N -- and 33, one symbol more"""
    n = n_fft
    cp, cs, P = n // 4, 0, n + n // 4
    rs = np.random.RandomState(n)
    w = rs.uniform(0.3, 1.1, P)
    mask = CM.tx_mask(P)
    for S in (32, 33):
        assert (S * P) % (8 * n) == (0 if S == 32 else P)
        X = T.draw_symbols(n, rs, S, guard(n))
        got = T.tx_psd_batch_gpu(n, T._full_grid(n, X, guard(n))[None], [(0, cp, cs, 0, w, mask)], divide=False)
        check_job(got[0], Geo(n, cp, cs), X, w, 0, mask, n, "N=%d boundary S=%d" % (n, S))


@pytest.mark.parametrize("n_fft", [64, 1024])
def test_geometry_edges(n_fft):
    """cp + cs = N / 2 (at N = 1024: 3 P - 2 = 4606, the 8192-point transform), odd and even P, cp = cs = 0, and the
    largest P the kernel takes, (8 N + 2) / 3; the first P beyond it is refused with the limit in the message."""
    n = n_fft
    pmax = (8 * n + 2) // 3
    geos = [(n // 4 + 3, n // 4 - 3), (n // 2, 0), (0, n // 2), (n // 4 + 3, n // 4 - 4), (0, 0), (3, 0),
            (n, pmax - 2 * n), ((pmax - n) // 2, pmax - n - (pmax - n) // 2)]
    assert {(n + a + b) % 2 for a, b in geos} == {0, 1} and max(n + a + b for a, b in geos) == pmax
    rs = np.random.RandomState(5 + n)
    S = 19
    X = T.draw_symbols(n, rs, S, guard(n))
    jobs, meta = [], []
    for cp, cs in geos:
        P = n + cp + cs
        w = rs.uniform(0.3, 1.1, P)
        mask = CM.tx_mask(P) if (cp + cs) % 3 else rs.uniform(0.2, 1.2, 2 * P - 1)
        for ov in (8, P // 2):
            jobs.append((0, cp, cs, ov, w, mask))
            meta.append((Geo(n, cp, cs), w, ov, mask))
    got = T.tx_psd_batch_gpu(n, T._full_grid(n, X, guard(n))[None], jobs, divide=False)
    for g, (geo, w, ov, mask) in zip(got, meta):
        check_job(g, geo, X, w, ov, mask, n, "N=%d cp=%d cs=%d ov=%d" % (n, geo.cp, geo.cs, ov))
    cp, cs = (pmax + 1 - n) // 2, pmax + 1 - n - (pmax + 1 - n) // 2
    P = n + cp + cs
    with pytest.raises(_lib.WofdmError) as e:
        T.tx_psd_batch_gpu(n, T._full_grid(n, X, guard(n))[None], [(0, cp, cs, 0, np.ones(P), np.ones(2 * P - 1))])
    assert e.value.code == -2 and "3 P - 2 <= 8 n_fft" in str(e.value) and str(pmax) in str(e.value)


def heterogeneous_set(n=256, seed=17):
    """the 72-job set of test_gpu_tx_psd_batch.py::test_heterogeneous_batch_matches_the_mirror_job_by_job"""
    rs = np.random.RandomState(seed)
    grids, jobs, host = [], [], []
    for system in [s for s in V.SYSTEMS if s != "CP"]:
        for cp in (10, 16, 24, 32):
            st = V.make_structure(system, n, cp)
            X = T.draw_symbols(n, rs)
            tail = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1]))
            w_tx = V.expand_tx_window(st, tail) if st.tail_tx else np.ones(st.sym_len)
            for w, ov in T._obr_windows(st, w_tx):
                jobs.append((len(grids), st.cp, st.cs, ov, w))
                host.append((st, X, w, ov))
            grids.append(T._full_grid(n, X))
    return np.stack(grids), jobs, host


def test_heterogeneous_batch_every_other_job_masked():
    """Masks shared between the jobs of equal P; job by job against the mirror; the unmasked jobs bit for bit what a
    plain wofdm_tx_psd_batch call gives for them; the whole call repeatable bit for bit."""
    n = 256
    grids, jobs, host = heterogeneous_set(n)
    assert len(jobs) == 72
    mixed = [j + (CM.tx_mask(n + j[1] + j[2]),) if i % 2 else j for i, j in enumerate(jobs)]
    assert len({n + j[1] + j[2] for j in mixed if len(j) == 6}) < sum(len(j) == 6 for j in mixed)      # shared tables
    got = T.tx_psd_batch_gpu(n, grids, mixed, divide=False)
    for i, (g, (st, X, w, ov)) in enumerate(zip(got, host)):
        check_job(g, st, X, w, ov, mixed[i][5] if i % 2 else None, n, "job %d %s cp=%d ov=%d" % (i, st.system, st.cp, ov),
                  gb=T.GUARD_BAND)
    plain = T.tx_psd_batch_gpu(n, grids, jobs[0::2], divide=False)
    assert np.array_equal(got[0::2], plain)
    assert np.array_equal(got, T.tx_psd_batch_gpu(n, grids, mixed, divide=False))


def test_long_masked_run_is_repeatable():
    """20 000 symbols at N = 1024 (2 500 workgroups of the mask kernel, ~2 550 slices): two identical calls agree bit
    for bit; the all-ones job of the call stays at the unmasked job's spectrum."""
    n, cp, cs, ov, S = 1024, 12, 8, 8, 20000
    P = n + cp + cs
    rs = np.random.RandomState(23)
    X = (rs.randn(S, n) + 1j * rs.randn(S, n)).astype(np.complex64)
    w = rs.uniform(0.3, 1.1, P).astype(np.float32)
    jobs = [(0, cp, cs, ov, w, CM.tx_mask(P)), (0, cp, cs, ov, w, np.ones(2 * P - 1)), (0, cp, cs, ov, w)]
    a = T.tx_psd_batch_gpu(n, X[None], jobs, divide=False)
    b = T.tx_psd_batch_gpu(n, X[None], jobs, divide=False)
    assert np.array_equal(a, b)
    assert np.abs(a[1].astype(np.float64) - a[2]).max() < PSD_RTOL * a[2].max()
    assert 0.3 < a[0].astype(np.float64).sum() / a[2].astype(np.float64).sum() < 1.0      # the mask passes half the band and more


@pytest.mark.parametrize("n_fft", [256, 1024])
def test_estimate_obr_masked_gpu_matches_the_host_route(n_fft):
    st = V.make_structure("wtx", n_fft, 32)
    rs = np.random.RandomState(n_fft)
    w_tx = random_window(rs, st)
    X = T.draw_symbols(n_fft, rs)
    mask = CM.tx_mask(st.sym_len)
    gpu = T.estimate_obr(st, w_tx, X=X, mask=mask, gpu=True)
    cpu = T.estimate_obr(st, w_tx, X=X, mask=mask)
    unmasked = T.estimate_obr(st, w_tx, X=X)
    for tag, g, c, u in zip(("opt", "rc", "cp"), gpu, cpu, unmasked):
        assert np.abs(g["X_est_" + tag] - c["X_est_" + tag]).max() < PSD_RTOL * c["X_est_" + tag].max(), tag
        print("estimate_obr N=%d %s: OBR %.3e (unmasked %.3e), GPU off by %.2e" % (n_fft, tag, c["obr_" + tag], u["obr_" + tag],
                                                                               abs(g["obr_" + tag] / c["obr_" + tag] - 1)))
        assert abs(g["obr_" + tag] / c["obr_" + tag] - 1) < 2e-4, tag
        assert c["obr_" + tag] < u["obr_" + tag], tag
        assert np.array_equal(g["S_" + tag], c["S_" + tag])
    single = T.psd_estimate_gpu(st, X, w_tx, st.tail_tx, mask=mask)
    assert np.abs(single - cpu[0]["X_est_opt"]).max() < PSD_RTOL * cpu[0]["X_est_opt"].max()


@pytest.mark.parametrize("n_fft", [256, 1024])
@pytest.mark.parametrize("system", ["wtx", "CPW"])
def test_spectrum_for_window_file_gpu_matches_the_host_route(system, n_fft):
    st = V.make_structure(system, n_fft, 32, 8, 10 if system in V.RX_WINDOWED else 0)
    rs = np.random.RandomState(9)
    keys = ("optimizedWindow", "optimizedWindowCaseAStep1", "optimizedWindowCaseAStep3", "optimizedWindowCaseBStep1",
            "optimizedWindowCaseBStep2", "optimizedWindowCaseBStep3")
    windows = {k: random_window(rs, st) for k in keys}
    sym = rs.choice(T.SYMBOLS_16QAM, size=(n_fft // 2, 256), replace=True)
    gpu = W.spectrum_for_window_file(system, 32, windows, num_subcar=n_fft, symbols=sym, gpu=True)
    cpu = W.spectrum_for_window_file(system, 32, windows, num_subcar=n_fft, symbols=sym, gpu=False)
    assert list(gpu) == list(cpu)
    for name in cpu:
        g, c = gpu[name], cpu[name]
        for k in ("psd", "psd_masked"):
            assert np.abs(g[k] - c[k]).max() < PSD_RTOL * c[k].max(), (name, k)
        for k in ("obr", "obr_masked"):
            print("spectrum N=%d %s %s %s: %.3e of the peak, GPU off by %.2e"
                  % (n_fft, system, name, k, c[k] / c["psd"].max(), abs(g[k] / c[k] - 1)))
            assert abs(g[k] / c[k] - 1) < 2e-4, (name, k)
        assert np.array_equal(g["f_axis"], c["f_axis"])
    assert cpu["rc"]["obr_masked"] < cpu["rc"]["obr"]
