"""Rows f2 and f4 on the GPU: ``wofdm_interference`` (wofdm_interf_kernel<N>, N = 64 ... 1024) and
``wofdm_tx_psd`` (wofdm_txwave_kernel<N> + wofdm_psd_kernel<8 N>, N = 64 / 128 / 256) against the
reference's own numbers (tests/golden/interference*.npz, psd_slices.npz) and against fp64 host
references at the shapes where the kernels' index arithmetic has edges; and the closed form's
A_0 / A_1 tied to the instrumented frame kernel (Y[s] = A_0 X[s] + A_1 X[s-1]) at every N.

Tolerances (fp32 kernels against fp64):
  * interference: 5e-5 of max|ref| (as before) plus the fp32 floor, which carries the cases with none
    to speak of (cp >= L - 1 and the like: the fp64 reference holds rounding only, ~1e-26).  The host
    mirror evaluated in complex64 (windows, DFT / IDFT factors and channel rounded to fp32, the products
    accumulated in fp32) is the floor of an fp32 evaluation of the same matrices; its deviation from the fp64 mirror, in units of the largest wanted power
    max_n |A_0[n, n]|^2, times 10 is the bound (``fp32_floor``).  Where there is no interference it
    comes out at 5e-13 ... 1.5e-12 of the wanted power (N = 128 ... 1024); the former absolute 1e-9 was
    1e-9 of a wanted power of ~1.
  * Tx PSD: 2e-5 of max (the existing rule), Parseval 1e-5 relative (fp32 sums of 8 N ... 8 N x 40
    squared magnitudes), repeatability bit-exact (the overlap atomics add two addends to a zero)."""
import ctypes as C
import os

import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import _lib
from wofdm_amd import interference as I
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SIZES = np.load(os.path.join(GOLDEN, "interference_sizes.npz"))
PSD = np.load(os.path.join(GOLDEN, "psd_slices.npz"))
CHANNELS = np.load(os.path.join(GOLDEN, "channels_vehA.npz"))["h"]       # [100][21] complex128
STAGE_RTOL = 2e-5          # as test_gpu_parity.py: fp32 chain of an N <= 1024 FFT + 21-tap FIR vs fp64
MATERIAL_RTOL = 5e-5
PSD_RTOL = 2e-5
NEAR_ZERO = 1e-12          # max P below this fraction of the wanted power: no interference to speak of


# ---------------------------------------------------------------------------------------------
# row f2: closed-form interference

def _mirror(st, w_tx, w_rx, h, dtype=np.complex128):
    """(P [N], wanted |A_0[n, n]|^2 [N]) of the host mirror, evaluated in ``dtype``."""
    T_ = I.tx_matrix(st, np.asarray(w_tx, np.float64)).astype(dtype)
    R_ = I.rx_matrix(st, np.asarray(w_rx, np.float64)).astype(dtype)
    H_ = I.channel_tensor(st, np.asarray(h).astype(dtype)).astype(dtype)
    A = R_ @ H_ @ T_
    a0 = A[0]
    off = a0 - np.diag(np.diag(a0))
    p = (np.abs(off) ** 2).sum(axis=1, dtype=np.float64) + (np.abs(A[1:]) ** 2).sum(axis=(0, 2), dtype=np.float64)
    return p, np.abs(np.diag(a0).astype(np.complex128)) ** 2


def fp32_floor(st, w_tx, w_rx, h):
    """10 x the complex64 mirror's deviation from the fp64 one, in absolute power (module docstring)."""
    p64, wanted = _mirror(st, w_tx, w_rx, h)
    p32, _ = _mirror(st, w_tx, w_rx, h, np.complex64)
    return 10 * np.abs(p32 - p64).max(), p64, wanted


def check_interference(got, want, st, w_tx, w_rx, h, what):
    """|got - want| < MATERIAL_RTOL max|want| + fp32_floor: the relative rule carries material interference,
    the floor the cases with next to none.  Returns (regime, deviation / bound)."""
    err = float(np.abs(got - want).max())
    bound, _, wanted = fp32_floor(st, w_tx, w_rx, h)
    tol = MATERIAL_RTOL * np.abs(want).max() + bound
    assert err < tol, (what, err, np.abs(want).max(), bound)
    return ("material" if np.abs(want).max() >= NEAR_ZERO * wanted.max() else "none"), err / tol


def _windows(st, rs):
    """A non-RC pair: tails from sorted uniforms, flat levels != 1."""
    xt = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(.02, .98, st.tail_tx))[::-1]))
    xr = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(.02, .48, st.tail_rx // 2))[::-1]))
    return (V.expand_tx_window(st, xt) if st.tail_tx else np.full(st.sym_len, xt[0]),
            V.expand_rx_window(st, xr) if st.tail_rx else np.full(st.rx_win_len, xr[0]))


def _size_cases(n_fft):
    for i in range(int(SIZES["n_cases"])):
        key = "case%d" % i
        n, cp, cs, ttx, trx, rm, shift = (int(v) for v in SIZES[key + "_cfg"])
        if n != n_fft:
            continue
        st = V.Structure(str(SIZES[key + "_system"]), n, cp, ttx, trx, cs, rm, shift)
        pairs = [("rc", V.tx_rc_window(st), V.rx_rc_window(st))]
        if key + "_P_opt" in SIZES:
            pairs.append(("opt", V.expand_tx_window(st, SIZES[key + "_xt"]) if ttx else np.ones(st.sym_len),
                          V.expand_rx_window(st, SIZES[key + "_xr"]) if trx else np.ones(st.rx_win_len)))
        yield key, st, pairs


@pytest.mark.parametrize("n_fft", [128, 256, 512, 1024])
def test_interference_matches_the_reference_at_every_size(n_fft):
    """All seven structures x {cp < L - 1, cp 32} x {RC, non-RC} pairs (one launch per structure, the
    pairs batched) against the reference's interf_power (interference_sizes.npz)."""
    h = SIZES["h"]
    worst = {}
    for key, st, pairs in _size_cases(n_fft):
        w_tx = np.stack([p[1] for p in pairs])
        w_rx = np.stack([p[2] for p in pairs])
        got = I.interf_power_gpu(st, w_tx, w_rx, h)
        assert got.shape == (len(pairs), 1, n_fft)
        for pi, (tag, wt, wr) in enumerate(pairs):
            want = SIZES["%s_P_%s" % (key, tag)]
            kind, dev = check_interference(got[pi, 0], want, st, wt, wr, h, (st.system, st.cp, tag))
            worst[kind] = max(worst.get(kind, 0.0), dev)
    assert set(worst) == {"material", "none"}
    print("interference N=%d worst deviation / bound: %s" % (n_fft, worst))


def test_interference_n64_reference_and_both_regimes(golden):
    """N = 64: the reference's RC numbers (interference.npz, cp 12) with the floor rule in place of the
    former + 1e-9, and the non-RC pair and cp 32 against the mirror (pinned to the reference at the
    other sizes by test_aux_mirrors.py)."""
    g = golden("interference.npz")
    rs = np.random.RandomState(64)
    worst = {}
    for system in W.SYSTEMS:
        n_fft, cp, cs, ttx, trx, rm, shift = [int(v) for v in g[system + "_cfg"]]
        st = V.Structure(system, n_fft, cp, ttx, trx, cs, rm, shift)
        got = I.interf_power_gpu(st, V.tx_rc_window(st), V.rx_rc_window(st), g["h"])[0, 0]
        kind, dev = check_interference(got, g[system + "_P_rc"], st, V.tx_rc_window(st), V.rx_rc_window(st),
                                       g["h"], (system, "ref"))
        worst[kind] = max(worst.get(kind, 0.0), dev)
        for cp in (12, 32):
            st = W.make_structure(system, 64, cp)
            wt, wr = _windows(st, rs)
            got = I.interf_power_gpu(st, wt, wr, g["h"])[0, 0]
            kind, dev = check_interference(got, I.interf_power(st, wt, wr, g["h"]), st, wt, wr, g["h"],
                                           (system, cp))
            worst[kind] = max(worst.get(kind, 0.0), dev)
    assert set(worst) == {"material", "none"}
    print("interference N=64 worst deviation / bound: %s" % worst)


@pytest.mark.parametrize("pairs,n_ch,system,n_fft,cp", [(1, 7, "WOLA", 64, 12), (5, 1, "CPW", 512, 16),
                                                        (3, 4, "wtx", 128, 12)])
def test_interference_batch_indexing(pairs, n_ch, system, n_fft, cp):
    """job = pair * n_channels + channel: every [pair, channel] slice against its own mirror value,
    all windows and channels distinct."""
    st = W.make_structure(system, n_fft, cp)
    rs = np.random.RandomState(pairs * 10 + n_ch)
    wins = [_windows(st, rs) for _ in range(pairs)]
    w_tx, w_rx = np.stack([w[0] for w in wins]), np.stack([w[1] for w in wins])
    h = CHANNELS[20:20 + n_ch]
    got = I.interf_power_gpu(st, w_tx, w_rx, h)
    assert got.shape == (pairs, n_ch, n_fft)
    for pi in range(pairs):
        for ci in range(n_ch):
            check_interference(got[pi, ci], I.interf_power(st, w_tx[pi], w_rx[pi], h[ci]), st, w_tx[pi],
                               w_rx[pi], h[ci], (pi, ci))


@pytest.mark.parametrize("n_taps", [1, 5, 21])
@pytest.mark.parametrize("system,n_fft,cp", [("WOLA", 256, 12), ("wrx", 1024, 16), ("CPwtx", 128, 16)])
def test_interference_short_channels(n_taps, system, n_fft, cp):
    st = W.make_structure(system, n_fft, cp)
    wt, wr = _windows(st, np.random.RandomState(n_taps))
    h = CHANNELS[30, :n_taps]
    got = I.interf_power_gpu(st, wt, wr, h)[0, 0]
    check_interference(got, I.interf_power(st, wt, wr, h), st, wt, wr, h, n_taps)


def _edge_structures(n_fft):
    """cp + cs - tail_tx = 64 (B = N + 64: the 64 lanes' RB2 FIR outputs are exactly 2 B), and hand-built
    geometries with circ_shift = N - 1 and the largest prefix_rm that B = N + delta + gamma allows."""
    out = [W.make_structure("CP", n_fft, 64)]
    out.append(W.make_structure("WOLA", n_fft, 64) if n_fft <= 512 else W.make_structure("wrx", n_fft, 59))
    out.append(V.Structure("CP", n_fft, 64, 0, 0, 0, 64, n_fft - 1))
    cp = 64 if n_fft <= 512 else 56                   # cp + cs <= 64 at N = 1024
    out.append(V.Structure("WOLA", n_fft, cp, 8, 10, 8, cp - 10, n_fft - 1))
    out.append(V.Structure("wrx", n_fft, 16, 0, 10, 5, 11, n_fft - 1))
    for st in out:
        assert st.stride == n_fft + st.tail_rx + st.prefix_rm
    return out


@pytest.mark.parametrize("n_fft", [64, 128, 256, 512, 1024])
def test_interference_geometry_edges(n_fft):
    rs = np.random.RandomState(n_fft)
    for st in _edge_structures(n_fft):
        wt = rs.uniform(0.2, 1.2, st.sym_len)          # arbitrary windows: the kernel assumes no shape
        wr = rs.uniform(0.2, 1.2, st.rx_win_len)
        h = CHANNELS[40]
        got = I.interf_power_gpu(st, wt, wr, h)[0, 0]
        check_interference(got, I.interf_power(st, wt, wr, h), st, wt, wr, h, st)


@pytest.mark.parametrize("system,n_fft,cp", [("CPW", 64, 12), ("WOLA", 256, 16), ("CPwrx", 1024, 12)])
def test_interference_channel_scaling(system, n_fft, cp):
    """P(a h) = |a|^2 P(h); a unit phase changes nothing."""
    st = W.make_structure(system, n_fft, cp)
    wt, wr = _windows(st, np.random.RandomState(1))
    h = CHANNELS[50]
    a, u = 0.35 - 1.6j, np.exp(0.7j)
    got = I.interf_power_gpu(st, wt, wr, np.stack([h, a * h, u * h]))[0]
    ref = np.abs(got[0]).max()
    assert np.abs(got[1] - abs(a) ** 2 * got[0]).max() < MATERIAL_RTOL * abs(a) ** 2 * ref
    assert np.abs(got[2] - got[0]).max() < MATERIAL_RTOL * ref


@pytest.mark.parametrize("n_fft", [64, 128, 256, 512, 1024])
def test_interference_cp_ofdm_one_tap_is_zero(n_fft):
    st = W.make_structure("CP", n_fft, 16)
    h = np.array([0.8 - 0.3j])
    got = I.interf_power_gpu(st, np.ones(st.sym_len), np.ones(st.rx_win_len), h)[0, 0]
    bound, p64, _ = fp32_floor(st, np.ones(st.sym_len), np.ones(st.rx_win_len), h)
    assert np.abs(got).max() < bound


# ---------------------------------------------------------------------------------------------
# cross-row: closed form (f2) vs the frame kernel (8a)

@pytest.mark.parametrize("system,n_fft,cp", [("WOLA", 64, 12), ("CPW", 128, 16), ("wtx", 256, 12),
                                             ("CPwrx", 512, 16), ("wrx", 1024, 12)])
def test_frame_kernel_is_the_interference_matrices(system, n_fft, cp):
    """The instrumented frame kernel (injected labels and unit noise, 150 dB): its received blocks are
    A_0 X[s] + A_1 X[s-1] with the closed form's matrices -- no oracle in the loop."""
    from test_aux_mirrors import cross_row_case, predicted_y
    st, w_tx, w_rx, h = cross_row_case(system, n_fft, cp)
    S, seed, cell, frame = 16, 3, 0, 17
    osys = O.make_sys(n_fft, 4, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, 21, 1)
    lab = O.gen_labels(osys, seed, cell, frame)
    noise = O.gen_noise(osys, seed, cell, frame)
    cfg = W.make_cfg(st, 4, S, 21, 1, 1, 1, seed=seed)
    with W.Plan(cfg, w_tx, w_rx, h[None], np.array([150.0], np.float32)) as plan:
        _, gd = plan.dump_frame(cell, frame, lab, noise.astype(np.complex64))
    want = predicted_y(st, w_tx, w_rx, h, gd["X"].astype(np.complex128))
    err = np.abs(gd["Y"] - want).max() / np.abs(want).max()
    print("cross-row N=%d: %.2e" % (n_fft, err))
    assert err < STAGE_RTOL, err


# ---------------------------------------------------------------------------------------------
# row f4: Tx waveform + averaged periodogram

def tx_psd_raw(n_fft, cp, cs, X, w, overlap):
    """wofdm_tx_psd on the full grid X [S][N] (every bin as given): (rc, undivided float32 [8 N])."""
    lib = _lib.load()
    cfg = _lib.Cfg()
    cfg.n_fft, cfg.cp, cfg.cs = n_fft, cp, cs
    grid = _lib.c64_as_f32(np.ascontiguousarray(X, dtype=np.complex64))
    wf = np.ascontiguousarray(w, dtype=np.float32)
    out = np.zeros(8 * n_fft, np.float32)
    rc = lib.wofdm_tx_psd(C.byref(cfg), 0, wf.ctypes.data, grid.ctypes.data, int(X.shape[0]), int(overlap),
                          out.ctypes.data)
    return rc, out


def host_wave(n_fft, cp, cs, X, w, overlap):
    """fp64 waveform straight from X [S][N]: IDFT, CP / CS copy, window, overlap-add."""
    t = np.fft.ifft(np.asarray(X, np.complex128), axis=1)
    idx = (np.arange(n_fft + cp + cs) - cp) % n_fft
    return T.overlap_and_add(np.asarray(w, np.float64)[None, :] * t[:, idx], overlap)


def _run_lengths(n_fft, P, overlap):
    fl, bo = 8 * n_fft, P - overlap
    runs = [1, 15, 16, 17, 300, max(1, (fl - 1 - overlap) // bo)]      # ... and the longest run shorter than FL
    exact = [s for s in range(1, 4 * fl) if (overlap + s * bo) % fl == 0]
    if exact:
        runs.append(exact[0])
    return runs, bool(exact)


@pytest.mark.parametrize("cp,cs,tail", [(0, 0, 8), ("N", 0, 8), (12, 8, 8)])
@pytest.mark.parametrize("n_fft", [64, 128, 256])
def test_tx_psd_full_band_against_fp64(n_fft, cp, cs, tail):
    """Full-band complex Gaussian symbols (bin 0 and the bins around N/2 loaded too) for every run length
    and overlap of the issue grid, against psd_estimate(overlap_and_add(...)) in fp64; and Parseval on
    the undivided sum."""
    cp = n_fft if cp == "N" else cp
    P = n_fft + cp + cs
    fl = 8 * n_fft
    rs = np.random.RandomState(n_fft + cp + cs)
    w = rs.uniform(0.3, 1.1, P)
    n_exact = 0
    for overlap in sorted({0, 1, tail, P // 2}):
        runs, has_exact = _run_lengths(n_fft, P, overlap)
        n_exact += has_exact
        for S in runs:
            X = (rs.randn(S, n_fft) + 1j * rs.randn(S, n_fft)).astype(np.complex64)
            rc, got = tx_psd_raw(n_fft, cp, cs, X, w.astype(np.float32), overlap)
            assert rc == 0, _lib.load().wofdm_last_error()
            x = host_wave(n_fft, cp, cs, X, w.astype(np.float32), overlap)
            assert x.size == overlap + S * (P - overlap)
            want = T.psd_estimate(x, fl) * (x.size // fl + 1)
            err = np.abs(got - want).max() / want.max()
            assert err < PSD_RTOL, (overlap, S, err)
            assert abs(float(got.astype(np.float64).sum()) / (fl * (np.abs(x) ** 2).sum()) - 1) < 1e-5, (overlap, S)
    assert n_exact >= 1


def test_tx_psd_repeatable():
    rs = np.random.RandomState(9)
    n_fft, cp, cs = 128, 12, 8
    P = n_fft + cp + cs
    X = (rs.randn(300, n_fft) + 1j * rs.randn(300, n_fft)).astype(np.complex64)
    w = rs.uniform(0.3, 1.1, P)
    for overlap in (1, P // 2):
        a = tx_psd_raw(n_fft, cp, cs, X, w, overlap)
        b = tx_psd_raw(n_fft, cp, cs, X, w, overlap)
        assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("n_fft", [64, 128, 256])
def test_psd_kernel_reproduces_the_reference_periodogram(n_fft):
    """psd_slices.npz: the reference's own periodograms at FL = 512 / 1024 / 2048, the stored waveform fed
    through the waveform kernel unchanged (cp = cs = overlap = 0, unit window, X = FFT of each N-block)."""
    fl = 8 * n_fft
    for tag in ("exact", "plusN", "long"):
        x = PSD["N%d_%s_x" % (n_fft, tag)].astype(np.complex128)
        ref = PSD["N%d_%s_psd" % (n_fft, tag)]
        X = np.fft.fft(x.reshape(-1, n_fft), axis=1)
        rc, got = tx_psd_raw(n_fft, 0, 0, X, np.ones(n_fft), 0)
        assert rc == 0
        err = np.abs(got / (x.size // fl + 1) - ref).max() / ref.max()
        print("psd N=%d %s: %.2e" % (n_fft, tag, err))
        assert err < PSD_RTOL, (tag, err)


@pytest.mark.parametrize("system", ["wtx", "CPW", "wrx", "CPwtx"])
def test_estimate_obr_on_gpu_replays_the_reference_at_n256(system):
    n_fft, cp = (int(v) for v in PSD["obr_cfg"])
    st = V.make_structure(system, n_fft, cp)
    w_tx = V.expand_tx_window(st, PSD["obr_%s_xt" % system])
    rng = np.random.RandomState(int(PSD["obr_%s_seed" % system]))
    for tag, d in zip(("opt", "rc", "cp"), T.estimate_obr(st, w_tx, 200e-9, rng=rng, gpu=True)):
        ref = PSD["obr_%s_X_est_%s" % (system, tag)]
        assert np.abs(d["X_est_" + tag] - ref).max() < PSD_RTOL * ref.max(), tag
        assert abs(d["obr_" + tag] / PSD["obr_%s_obr_%s" % (system, tag)] - 1) < 2e-4, tag
