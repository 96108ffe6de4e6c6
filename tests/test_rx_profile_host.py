"""The host side of the receive profile (wofdm_amd.rx_profile) without a GPU: the fp64 numpy mirror ``frame_profile`` and
the host's Philox streams against the CPU oracle, and the oracle-only conditions the GPU tests rely on
(tests/rx_profile_cases.py): at most 1 % near decisions in every case, errors of both kinds at both SNR points."""
import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import rx_profile as R
from wofdm_amd import timefreq as T

import rx_profile_cases as RC

SMALL = ((64, "wtx", "plain"), (128, "CPW", "half_masked"), (64, "wrx", "masked"))


@pytest.mark.parametrize("nbt", (1, 0))
@pytest.mark.parametrize("n_fft,system,variant", SMALL)
def test_frame_profile_against_the_oracle(n_fft, system, variant, nbt):
    cp, S, k = RC.shape_of(n_fft, system, variant)
    c = RC.make_case(W.make_structure(system, n_fft, cp), k, S, variant, 11, nbt)
    st, osys = c["st"], RC.oracle_sys(c)
    on = np.ones(n_fft, bool) if c["active"] is None else c["active"]
    for cell, frame in ((0, 0), (5, 3)):
        p, s, ch = cell // 4, (cell // 2) % 2, cell % 2
        lab, noise = O.gen_labels(osys, 9, cell, frame), O.gen_noise(osys, 9, cell, frame)
        _, d = O.frame(osys, c["w_tx"][p].astype(np.float64), c["w_rx"][p].astype(np.float64),
                       c["h"][ch].astype(np.complex128), float(c["snr"][s]), lab, noise, dump=True)
        grid = T.qam_table(k)[lab] * on[None, :]
        assert np.abs(grid - d["X"]).max() < 1e-15
        bit, sym, pw, xhat, y0 = R.frame_profile(st, grid, noise, c["w_tx"][p], c["w_rx"][p], c["h"][ch], c["snr"][s], k,
                                                 c["active"], c["mask"], nbt)
        assert np.abs(xhat - d["Xhat"]).max() < 1e-10 * max(1.0, np.abs(d["Xhat"]).max())
        assert np.abs(y0[on] - d["Y"][0][on]).max() < 1e-10 * np.abs(d["Y"][0]).max()
        want = RC.oracle_frame(c, 9, cell, frame, osys)
        assert np.array_equal(bit.astype(np.int64), want[0]) and np.array_equal(sym.astype(np.int64), want[1])
        assert np.abs(pw - want[2]).max() < 1e-10 * want[2].max()
        assert (bit[~on] == 0).all() and (pw[~on] == 0).all()
        # the slicer is the inverse of the constellation table
        assert np.array_equal(R.slice_labels(k, T.qam_table(k)), np.arange(1 << k))


def test_host_streams_are_the_oracles():
    """labels and unit normals of (seed, cell, frame), 64-bit seed and a frame index beyond 2^32"""
    for n_fft, k, S in ((64, 2, 3), (128, 6, 2), (256, 4, 5)):
        osys = O.make_sys(n_fft, k, S, 16, 8, 8, 0, 16, 0, 21, 1)
        for seed, cell, frame in ((1, 0, 0), (0x9E3779B97F4A7C15, 5, 2 ** 32 + 7), (77, (1 << 28) - 1, 2 ** 40)):
            assert np.array_equal(R.gen_labels(n_fft, k, S, seed, cell, frame), O.gen_labels(osys, seed, cell, frame))
            want = O.gen_noise(osys, seed, cell, frame)
            assert np.abs(R.gen_noise(want.size, seed, cell, frame) - want).max() < 1e-12


def test_rx_profile_host_adds_up_to_the_oracles_counters():
    c, seed, ref = RC.reference(64, "CPW", "half")
    prof, near = W.rx_profile_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, 0, RC.FRAMES,
                                   active=c["active"], with_near=True)
    assert np.array_equal(prof.bit_err.sum(axis=-1), ref["counts"][..., 0])
    assert np.array_equal(prof.sym_err.sum(axis=-1), ref["counts"][..., 2])
    assert np.array_equal(near, ref["near"])
    assert int(prof.decisions.sum()) * c["k"] == int(ref["counts"][0, 0, 0, 1])
    assert RC.pow_ratio(prof.err_power, ref["pow"]) < 1e-10
    ber, evm = W.ber_per_bin(prof, c["k"]), W.evm_db(prof)
    on = c["active"]
    assert np.isnan(ber[..., ~on]).all() and np.isnan(evm[..., ~on]).all()
    assert np.allclose(np.nanmean(ber, axis=-1), ref["counts"][..., 0] / ref["counts"][..., 1].astype(float))
    # lower SNR: more errors and a larger error vector on every cell
    assert (np.nanmean(evm[:, 0], axis=-1) > np.nanmean(evm[:, 1], axis=-1)).all()


@pytest.mark.parametrize("n_fft", RC.NS)
def test_every_case_meets_the_seed_condition_and_counts_errors(n_fft):
    for system in RC.SYSTEMS:
        for variant in RC.VARIANTS:
            c, seed, ref = RC.reference(n_fft, system, variant)
            assert ref["near"].sum() <= 0.01 * ref["decisions"], (system, variant)
            assert int(ref["counts"][..., 3].sum()) == ref["decisions"]
            for s in range(RC.N_SNR):
                assert ref["bit"][:, s].sum() > 0 and ref["sym"][:, s].sum() > 0, (system, variant, s)
    if n_fft == 512:                                   # wrx at the CP the frame kernels take (the plan comparison)
        for variant in RC.VARIANTS:
            c, seed, ref = RC.reference(512, "wrx", variant, 1, 32)
            assert c["st"].stride - 512 == 37 and ref["near"].sum() <= 0.01 * ref["decisions"] and ref["sym"].sum() > 0
    if n_fft == 1024:
        c, seed, ref = RC.reference_over_the_frame_limit()
        assert ref["near"].sum() <= 0.01 * ref["decisions"] and ref["sym"].sum() > 0


def brute_threshold_distance(k, z):
    """the slicer's thresholds written out: (2 j - m) / a, j = 1 .. m - 1, per component"""
    m = 1 << (k // 2)
    a = {2: np.sqrt(2.0), 4: np.sqrt(10.0), 6: np.sqrt(42.0)}[k]
    th = np.array([(2 * j - m) / a for j in range(1, m)])
    return min(np.abs(z.real - th).min(), np.abs(z.imag - th).min())


def test_threshold_distance_and_near_decisions_by_hand():
    """the yardstick of the GPU comparisons against hand-computed thresholds"""
    s10, s42 = np.sqrt(10.0), np.sqrt(42.0)
    # QPSK: one threshold per component, at 0
    assert np.isclose(R.threshold_distance(2, 0.3 - 0.05j), 0.05) and np.isclose(R.threshold_distance(2, -5.0 + 4.0j), 4.0)
    # 16-QAM: 0 and +-2 / sqrt(10); beyond the outermost point only the last threshold counts
    assert np.isclose(R.threshold_distance(4, 0.1 + 0.5j), 0.1)
    assert np.isclose(R.threshold_distance(4, 0.3 + 0.5j), 2 / s10 - 0.5)
    assert np.isclose(R.threshold_distance(4, 2.0 - 3.0j), 2.0 - 2 / s10)
    # 64-QAM: 0, +-2, +-4, +-6 over sqrt(42)
    assert np.isclose(R.threshold_distance(6, 5 / s42 + 0.01 + 3j / s42), 1 / s42 - 0.01)
    assert np.isclose(R.threshold_distance(6, -7.5 / s42 - 9j), 1.5 / s42)
    rs = np.random.RandomState(1)
    for k in (2, 4, 6):
        z = 1.5 * (rs.randn(200) + 1j * rs.randn(200))
        assert np.allclose(R.threshold_distance(k, z), [brute_threshold_distance(k, v) for v in z], rtol=0, atol=1e-14)
        # a threshold lies midway between two neighbouring points, and the decision changes across it
        pts = T.qam_table(k)
        assert np.allclose(R.threshold_distance(k, pts), 1.0 / np.sqrt(2.0 * ((1 << k) - 1) / 3.0))
    # near: within tol max(1, |xhat|) max|y0| / |y0[n]| of a threshold; bin 1 is faded by 10, bin 2 unloaded
    xhat = np.array([[0.5 + 0.00009j, 0.5 + 0.0009j, 0.0j], [0.5 + 0.00011j, 0.5 + 0.0011j, 0.0j],
                     [30.0 + 0.0029j, 0.5 + 0.5j, 0.0j]])
    y0 = np.array([2.0, 0.2, 0.0])
    want = np.array([[True, True, False], [False, False, False], [True, False, False]])
    assert np.array_equal(R.near_decisions(2, xhat, y0, 1e-4), want)


def frame_power_single(c, grid, noise, p, s, ch):
    """err_power [N] of one frame with EVERY stage in single precision (numpy's complex64 transforms, a complex64
    convolution, float32 powers and gain, complex64 equaliser): an independent fp32 chain beside the GPU's"""
    st, f, r_ = c["st"], np.complex64, np.float32
    n, delta, gam, P = st.n_fft, st.tail_rx, st.prefix_rm, st.sym_len
    S, B = grid.shape[0], st.stride
    on = np.ones(n, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    rows = (np.fft.ifft(grid.astype(f), axis=1)[:, (np.arange(P) - st.cp) % n] * c["w_tx"][p][None, :]).astype(f)
    if c["mask"] is not None:
        y = np.fft.ifft(np.fft.fft(rows, 2 * P - 1, axis=1) * c["mask"][None, :], axis=1).astype(f)
        rows = y[:, :P].copy()
        rows[1:, :P - 1] += y[:-1, P:]
    conv = np.convolve(c["h"][ch].astype(f), T.overlap_and_add(rows, st.tail_tx))
    nz = noise.astype(f)
    assert conv.dtype == f and nz.size == conv.size
    ps, pn = (np.abs(conv) ** 2).mean(dtype=r_), (np.abs(nz) ** 2).mean(dtype=r_)
    g = r_(np.sqrt(ps * r_(10.0 ** (-0.1 * float(c["snr"][s]))) / pn))
    blocks = (conv[:S * B] + g * nz[:S * B]).reshape(S, B)[:, gam:gam + n + delta] * c["w_rx"][p][None, :]
    z = blocks[:, :n].copy()
    z[:, :delta] += blocks[:, n:]
    Y = np.fft.fft(np.roll(z, -(st.circ_shift + delta // 2), axis=1), axis=1)
    assert Y.dtype == f
    xhat = np.zeros((S - 1, n), f)
    xhat[:, on] = Y[1:, on] * (grid[0, on].astype(f) / Y[0, on])[None, :]
    return np.where(on[None, :], np.abs(xhat.astype(np.complex128) - grid[1:]) ** 2, 0.0).sum(axis=0)


@pytest.mark.parametrize("n_fft,system,variant,gpu", ((1024, "wtx", "masked", 2.93e-4), (512, "wtx", "masked", 1.13e-4)))
def test_a_single_precision_chain_deviates_as_the_gpu_does(n_fft, system, variant, gpu):
    """Why POW_TOL is 1e-3 and not less: the two cases with the largest err_power deviation on the GPU (`gpu`,
    profiles/rx_profile.txt), run through an independently written single-precision chain on the host, deviate from the
    oracle's fp64 sums by the same amount (2.8e-4 and 1.3e-4 here) -- it is what fp32 gives on the faded bins of these
    cases (Xhat = Y X0 / Y0 carries the error of Y0 times max |Y0| / |Y0[n]|), not a defect of one of the GPU's stages."""
    c, seed, ref = RC.reference(n_fft, system, variant)
    st, k, S = c["st"], c["k"], c["S"]
    nl = st.frame_len(S) + c["h"].shape[1] - 1
    on = np.ones(n_fft, bool) if c["active"] is None else c["active"]
    pw = np.zeros((8, n_fft))
    for cell in range(8):
        for f in range(RC.FRAMES):
            grid = T.qam_table(k)[R.gen_labels(n_fft, k, S, seed, cell, f)] * on[None, :]
            pw[cell] += frame_power_single(c, grid, R.gen_noise(nl, seed, cell, f), cell // 4, (cell // 2) % 2, cell % 2)
    ratio = RC.pow_ratio(pw.reshape(ref["pow"].shape), ref["pow"])
    print("N=%d %s %s: single-precision host chain %.2e, GPU %.2e" % (n_fft, system, variant, ratio, gpu))
    assert gpu / 2 < ratio < 2 * gpu and ratio < RC.POW_TOL and gpu < RC.POW_TOL
