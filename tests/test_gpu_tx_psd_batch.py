"""Row f4 at every N on the GPU: ``wofdm_tx_psd_batch`` (wofdm_txwave_batch_kernel<N> + wofdm_psd_batch_kernel<8 N>
+ wofdm_psd_reduce_kernel<8 N>) against the reference's own periodograms and OBR figures at N = 512 / 1024
(tests/golden/psd_large.npz, made by make_golden_psd_large.py), against fp64 host mirrors at the run lengths and
overlaps where the index arithmetic has edges, job by job in a heterogeneous batch, over many workgroups, and
through run_timefreq against its host route.

Tolerances as tests/test_gpu_aux_kernels.py: 2e-5 of the peak for the periodograms (PSD_RTOL), Parseval 1e-5
relative, OBR figures 2e-4 relative; repeated calls bit-exact (fixed-order sums, no atomics in the periodogram)."""
import os

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LARGE = np.load(os.path.join(GOLDEN, "psd_large.npz"))
PSD_RTOL = 2e-5


def waveform(seed, length):
    rs = np.random.RandomState(int(seed))
    return ((rs.randn(int(length)) + 1j * rs.randn(int(length))) / np.sqrt(2)).astype(np.complex64)


def host_wave(n_fft, cp, cs, X, w, overlap):
    """fp64 waveform straight from X [S][N]: IDFT, CP / CS copy, window, overlap-add."""
    t = np.fft.ifft(np.asarray(X, np.complex128), axis=1)
    idx = (np.arange(n_fft + cp + cs) - cp) % n_fft
    return T.overlap_and_add(np.asarray(w, np.float64)[None, :] * t[:, idx], overlap)


def raw_batch(n_fft, grids, jobs):
    return T.tx_psd_batch_gpu(n_fft, grids, jobs, divide=False)


@pytest.mark.parametrize("n_fft", [512, 1024])
def test_batch_periodogram_reproduces_the_reference(n_fft):
    """psd_large.npz: the reference's periodograms at FL = 4096 / 8192, the rebuilt waveform fed through the
    waveform kernel unchanged (cp = cs = overlap = 0, unit window, X = FFT of each N-block)."""
    fl = 8 * n_fft
    for tag in ("exact", "plusN", "long"):
        key = "pl%d_%s" % (fl, tag)
        x = waveform(LARGE[key + "_seed"], LARGE[key + "_len"])
        ref = LARGE[key + "_psd"].astype(np.float64)
        X = np.fft.fft(x.astype(np.complex128).reshape(-1, n_fft), axis=1)
        got = T.tx_psd_batch_gpu(n_fft, X[None], [(0, 0, 0, 0, np.ones(n_fft))])[0]
        err = np.abs(got - ref).max() / ref.max()
        print("psd FL=%d %s: %.2e" % (fl, tag, err))
        assert err < PSD_RTOL, (tag, err)


@pytest.mark.parametrize("system", ["wtx", "CPW", "wrx", "CPwtx"])
@pytest.mark.parametrize("n_fft", [512, 1024])
def test_estimate_obr_on_gpu_replays_the_reference_at_large_n(n_fft, system):
    cp = int(LARGE["obr_cp"])
    pre = "obr%d_%s_" % (n_fft, system)
    st = V.make_structure(system, n_fft, cp)
    w_tx = V.expand_tx_window(st, LARGE[pre + "xt"])
    rng = np.random.RandomState(int(LARGE[pre + "seed"]))
    for tag, d in zip(("opt", "rc", "cp"), T.estimate_obr(st, w_tx, 200e-9, rng=rng, gpu=True)):
        ref = LARGE[pre + "X_est_" + tag].astype(np.float64)
        err = np.abs(d["X_est_" + tag] - ref).max() / ref.max()
        print("obr N=%d %s %s: X_est %.2e, obr %.2e" % (n_fft, system, tag, err,
                                                        abs(d["obr_" + tag] / LARGE[pre + "obr_" + tag] - 1)))
        assert err < PSD_RTOL, tag
        assert abs(d["obr_" + tag] / LARGE[pre + "obr_" + tag] - 1) < 2e-4, tag


def _run_lengths(n_fft, P, overlap):
    fl, bo = 8 * n_fft, P - overlap
    runs = [1, 15, 16, 17, 300, max(1, (fl - 1 - overlap) // bo)]      # ... and the longest run shorter than FL
    exact = [s for s in range(1, 4 * fl) if (overlap + s * bo) % fl == 0]
    if exact:
        runs.append(exact[0])
    return runs, bool(exact)


@pytest.mark.parametrize("cp,cs", [(0, 0), (12, 8)])
@pytest.mark.parametrize("n_fft", [512, 1024])
def test_batch_full_band_against_fp64(n_fft, cp, cs):
    """Full-band complex Gaussian symbols for every run length and overlap {0, 1, 8, P // 2}, against
    psd_estimate(overlap_and_add(...)) in fp64; Parseval on the undivided sum.  The overlaps of one run length
    are the jobs of one call."""
    P = n_fft + cp + cs
    fl = 8 * n_fft
    rs = np.random.RandomState(n_fft + cp + cs)
    w = rs.uniform(0.3, 1.1, P).astype(np.float32)
    by_len, n_exact = {}, 0
    for overlap in sorted({0, 1, 8, P // 2}):
        runs, has_exact = _run_lengths(n_fft, P, overlap)
        n_exact += has_exact
        for S in runs:
            by_len.setdefault(S, []).append(overlap)
    for S, overlaps in sorted(by_len.items()):
        X = (rs.randn(S, n_fft) + 1j * rs.randn(S, n_fft)).astype(np.complex64)
        got = raw_batch(n_fft, X[None], [(0, cp, cs, ov, w) for ov in overlaps])
        for ov, g in zip(overlaps, got):
            x = host_wave(n_fft, cp, cs, X, w, ov)
            assert x.size == ov + S * (P - ov)
            want = T.psd_estimate(x, fl) * (x.size // fl + 1)
            err = np.abs(g - want).max() / want.max()
            assert err < PSD_RTOL, (ov, S, err)
            assert abs(float(g.astype(np.float64).sum()) / (fl * (np.abs(x) ** 2).sum()) - 1) < 1e-5, (ov, S)
    assert n_exact >= 1


def test_heterogeneous_batch_matches_the_mirror_job_by_job():
    """The N = 256 run_timefreq set -- 6 systems x 4 CPs x (optimised, RC, plain CP) windows, each (system, CP)
    on its own symbol block -- in one call, against the fp64 mirror and against one wofdm_tx_psd call per job."""
    n = 256
    rs = np.random.RandomState(17)
    systems = [s for s in V.SYSTEMS if s != "CP"]
    cps = (10, 16, 24, 32)
    grids, jobs, host = [], [], []
    for system in systems:
        for cp in cps:
            st = V.make_structure(system, n, cp)
            X = T.draw_symbols(n, rs)
            tail = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1]))
            w_tx = V.expand_tx_window(st, tail) if st.tail_tx else np.ones(st.sym_len)
            for w, ov in T._obr_windows(st, w_tx):
                jobs.append((len(grids), st.cp, st.cs, ov, w))
                host.append((st, X, w, ov))
            grids.append(T._full_grid(n, X))
    assert len(jobs) == 72
    got = T.tx_psd_batch_gpu(n, np.stack(grids), jobs)
    worst = 0.0
    for g, (st, X, w, ov) in zip(got, host):
        want = T.psd_estimate(T.overlap_and_add(T.tx_symbols(st, X, w.astype(np.float32)), ov), 8 * n)
        single = T.psd_estimate_gpu(st, X, w, ov)
        worst = max(worst, np.abs(g - want).max() / want.max())
        assert np.abs(g - want).max() < PSD_RTOL * want.max(), (st.system, st.cp, ov)
        assert np.abs(g - single).max() < PSD_RTOL * want.max(), (st.system, st.cp, ov)
    print("heterogeneous batch: worst %.2e of the peak" % worst)


def test_long_run_over_many_workgroups_is_exact_and_repeatable():
    """20 000 symbols at N = 1024: ~2 550 slices of 8192 points, spread over ~640 workgroups and summed in
    item order; against the fp64 mirror, and two identical calls agree bit for bit."""
    n, cp, cs, ov, S = 1024, 12, 8, 8, 20000
    rs = np.random.RandomState(23)
    X = (rs.randn(S, n) + 1j * rs.randn(S, n)).astype(np.complex64)
    w = rs.uniform(0.3, 1.1, n + cp + cs).astype(np.float32)
    jobs = [(0, cp, cs, ov, w)]
    a = raw_batch(n, X[None], jobs)[0]
    b = raw_batch(n, X[None], jobs)[0]
    assert np.array_equal(a, b)
    x = host_wave(n, cp, cs, X, w, ov)
    want = T.psd_estimate(x, 8 * n) * (x.size // (8 * n) + 1)
    err = np.abs(a - want).max() / want.max()
    print("long run: %.2e of the peak" % err)
    assert err < PSD_RTOL, err
    assert abs(float(a.astype(np.float64).sum()) / (8 * n * (np.abs(x) ** 2).sum()) - 1) < 1e-5


def _write_windows(folder, systems, cps, seed=5):
    rs = np.random.RandomState(seed)
    for system in systems:
        for cp in cps:
            if system not in V.TX_WINDOWED:
                continue
            xt = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(0.02, 0.98, 8))[::-1]))
            xr = np.concatenate(([1.0], np.sort(rs.uniform(0.02, 0.48, 5))[::-1]))
            vec = np.concatenate((xt, xr)) if system in ("WOLA", "CPW") else xt
            np.save(os.path.join(folder, "%s_%d.npy" % (system, cp)), vec)


@pytest.mark.parametrize("n_fft", [256, 1024])
def test_run_timefreq_gpu_matches_the_host_route(tmp_path, n_fft):
    systems, cps = ("CPW", "wrx"), (12, 20)
    _write_windows(str(tmp_path), systems, cps)
    gpu = W.run_timefreq(cps, systems, str(tmp_path), str(tmp_path / "g"), n_fft=n_fft,
                         rng=np.random.RandomState(8), gpu=True)
    cpu = W.run_timefreq(cps, systems, str(tmp_path), str(tmp_path / "c"), n_fft=n_fft,
                         rng=np.random.RandomState(8))
    assert set(gpu) == set(cpu)
    names = sorted(os.listdir(tmp_path / "c" / "timefreq"))
    assert names == sorted(os.listdir(tmp_path / "g" / "timefreq")) and len(names) == 10
    for name in names:
        g, c = np.load(tmp_path / "g" / "timefreq" / name), np.load(tmp_path / "c" / "timefreq" / name)
        assert set(g.files) == set(c.files), name
        for k in c.files:
            if k.startswith("X_est_") or k.startswith("mf_band_"):
                peak = c["X_est_" + k.split("_")[-1]].max()
                assert np.abs(g[k] - c[k]).max() < PSD_RTOL * peak, (name, k)
            elif k.startswith("obr_"):
                assert abs(g[k] / c[k] - 1) < 2e-4, (name, k)
            else:
                assert np.array_equal(g[k], c[k]), (name, k)
