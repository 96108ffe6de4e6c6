"""Host mirrors of rows f2 (closed-form interference) and f4 (Tx PSD) against the reference's own
numbers at every DFT length they serve (tests/golden/interference_sizes.npz, psd_slices.npz, made by
tests/golden/make_golden.py), and the closed form tied to the frame pipeline through the oracle:
Y[s] = A_0 X[s] + A_1 X[s-1].  The GPU twins of these checks are in test_gpu_aux_kernels.py."""
import os

import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import interference as I
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SIZES = np.load(os.path.join(GOLDEN, "interference_sizes.npz"))
PSD = np.load(os.path.join(GOLDEN, "psd_slices.npz"))


def size_cases(n_fft=None):
    """(key, Structure, [(tag, w_tx, w_rx)]) of interference_sizes.npz (RC pair, non-RC pair)."""
    out = []
    for i in range(int(SIZES["n_cases"])):
        key = "case%d" % i
        n, cp, cs, ttx, trx, rm, shift = (int(v) for v in SIZES[key + "_cfg"])
        if n_fft is not None and n != n_fft:
            continue
        st = V.Structure(str(SIZES[key + "_system"]), n, cp, ttx, trx, cs, rm, shift)
        pairs = [("rc", V.tx_rc_window(st), V.rx_rc_window(st))]
        if key + "_P_opt" in SIZES:
            xt, xr = SIZES[key + "_xt"], SIZES[key + "_xr"]
            pairs.append(("opt", V.expand_tx_window(st, xt) if ttx else np.ones(st.sym_len),
                          V.expand_rx_window(st, xr) if trx else np.ones(st.rx_win_len)))
        out.append((key, st, pairs))
    return out


def wanted_power(st, w_tx, w_rx, h):
    """|A_0[n, n]|^2, the per-subcarrier power of the wanted term."""
    a0, _ = I.interference_matrices(st, w_tx, w_rx, h)
    return np.abs(np.diag(a0)) ** 2


def test_interference_sizes_fixture_covers_the_issue_grid():
    got = {}
    for key, st, pairs in size_cases():
        got.setdefault(st.n_fft, set()).add((st.system, st.cp, len(pairs)))
    for n_fft, cps in ((128, (16, 32)), (256, (12, 32)), (512, (16, 32)), (1024, (12, 32))):
        assert got[n_fft] == {(s, cp, 1 if s == "CP" else 2) for s in W.SYSTEMS for cp in cps}


@pytest.mark.parametrize("n_fft", [128, 256, 512, 1024])
def test_interf_power_mirror_matches_the_reference_at_every_size(n_fft):
    """Mirror (FFT-free index formulas) vs the reference's dense W K P V_rx R H_m V_tx Gamma W^-1 chain.
    Material interference: 1e-9 of max|ref|.  Where there is none (cp >= L - 1 for wtx, wrx, CPwrx,
    CP) both sides hold fp64 rounding only: 1e-20 of the wanted power."""
    h = SIZES["h"]
    for key, st, pairs in size_cases(n_fft):
        for tag, w_tx, w_rx in pairs:
            want = SIZES["%s_P_%s" % (key, tag)]
            got = I.interf_power(st, w_tx, w_rx, h)
            assert got.shape == want.shape == (n_fft,)
            wanted = wanted_power(st, w_tx, w_rx, h)
            err = np.abs(got - want).max()
            assert err < 1e-9 * np.abs(want).max() + 1e-20 * wanted.max(), (key, st.system, st.cp, tag, err)


def test_interference_fixture_has_both_regimes():
    """cp 32 >= L - 1 leaves wtx, wrx, CPwrx and CP without interference; cp < 20 never does."""
    h = SIZES["h"]
    for key, st, pairs in size_cases(256):
        for tag, w_tx, w_rx in pairs:
            rel = np.abs(SIZES["%s_P_%s" % (key, tag)]).max() / wanted_power(st, w_tx, w_rx, h).max()
            if st.cp < 20:
                assert rel > 1e-6, (st.system, st.cp, tag)
            elif st.system in ("wtx", "wrx", "CPwrx", "CP"):
                assert rel < 1e-20, (st.system, st.cp, tag)


@pytest.mark.parametrize("n_fft", [64, 128, 256])
def test_psd_estimate_matches_the_reference_periodogram(n_fft):
    """psd_estimate vs the reference's __psd_estimate at FL = 8 N: an exact multiple of FL (its divisor
    counts the empty remainder), FL + N and a long run with a partial slice."""
    fl = 8 * n_fft
    for tag, n_full in (("exact", 2), ("plusN", 1), ("long", 5)):
        x = PSD["N%d_%s_x" % (n_fft, tag)].astype(np.complex128)
        ref = PSD["N%d_%s_psd" % (n_fft, tag)]
        assert x.size % n_fft == 0 and x.size // fl == n_full and (x.size % fl == 0) == (tag == "exact")
        got = T.psd_estimate(x, fl)
        assert np.abs(got - ref).max() < 1e-12 * ref.max(), tag


@pytest.mark.parametrize("system", ["wtx", "CPW", "wrx", "CPwtx"])
def test_estimate_obr_replays_the_reference_at_n256(system):
    n_fft, cp = (int(v) for v in PSD["obr_cfg"])
    st = V.make_structure(system, n_fft, cp)
    w_tx = V.expand_tx_window(st, PSD["obr_%s_xt" % system])
    rng = np.random.RandomState(int(PSD["obr_%s_seed" % system]))
    for tag, d in zip(("opt", "rc", "cp"), T.estimate_obr(st, w_tx, 200e-9, rng=rng)):
        for k in ("X_est_" + tag, "obr_" + tag):
            ref = PSD["obr_%s_%s" % (system, k)]
            assert np.shape(d[k]) == ref.shape
            assert np.allclose(d[k], ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max()), k


# one structure per DFT length, CP below L - 1 so that A_1 (ISI) is material
CROSS_ROW = [("WOLA", 64, 12), ("CPW", 128, 16), ("wtx", 256, 12), ("CPwrx", 512, 16), ("wrx", 1024, 12)]


def cross_row_case(system, n_fft, cp, seed=5):
    """(Structure, w_tx, w_rx, h) of the Y = A_0 X[s] + A_1 X[s-1] check: non-RC windows (fp32),
    channel 7 of channels_vehA.npz (complex64)."""
    st = W.make_structure(system, n_fft, cp)
    rs = np.random.RandomState(seed + n_fft)
    xt = np.concatenate(([1.02], np.sort(rs.uniform(.05, .95, st.tail_tx))[::-1])) if st.tail_tx else [1.0]
    xr = np.concatenate(([0.98], np.sort(rs.uniform(.05, .45, st.tail_rx // 2))[::-1])) if st.tail_rx else [1.0]
    w_tx = (W.expand_tx_window(st, xt) if st.tail_tx else np.ones(st.sym_len)).astype(np.float32)
    w_rx = (W.expand_rx_window(st, xr) if st.tail_rx else np.ones(st.rx_win_len)).astype(np.float32)
    h = np.load(os.path.join(GOLDEN, "channels_vehA.npz"))["h"][7].astype(np.complex64)
    return st, w_tx, w_rx, h


def predicted_y(st, w_tx, w_rx, h, X):
    """[S, N]: A_0 X[s] + A_1 X[s-1] (X[-1] = 0) from the closed form's matrices."""
    a0, am = I.interference_matrices(st, w_tx.astype(np.float64), w_rx.astype(np.float64),
                                     h.astype(np.complex128))
    assert am.shape[0] == 1                    # M = 2 for every supported structure
    y = X @ a0.T
    y[1:] += X[:-1] @ am[0].T
    return y


@pytest.mark.parametrize("system,n_fft,cp", CROSS_ROW)
def test_oracle_frame_is_the_interference_matrices(system, n_fft, cp):
    """The BER pipeline (CPU oracle, 150 dB) received block by block is the closed form's A_0 / A_1."""
    st, w_tx, w_rx, h = cross_row_case(system, n_fft, cp)
    S, seed, cell, frame = 16, 3, 0, 17
    osys = O.make_sys(n_fft, 4, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, 21, 1)
    lab = O.gen_labels(osys, seed, cell, frame)
    noise = O.gen_noise(osys, seed, cell, frame)
    _, od = O.frame(osys, w_tx.astype(np.float64), w_rx.astype(np.float64), h.astype(np.complex128), 150.0,
                    lab, noise, dump=True)
    want = predicted_y(st, w_tx, w_rx, h, od["X"])
    err = np.abs(od["Y"] - want).max() / np.abs(want).max()
    # 150 dB: noise amplitude 10^-7.5 of the signal's; without A_1 the error is the ISI, >= 1e-3 here
    assert err < 1e-6, err


# ---------------------------------------------------------------------------------------------
# argument checks of the two entry points: host-side, before any device is touched

def _cfg(st, **kw):
    cfg = W.make_cfg(st, 4, 16, 21, 1, 1, 1)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_interference_abi_refuses_bad_arguments():
    import ctypes as C
    from wofdm_amd import _lib
    lib = _lib.load()
    st = W.make_structure("WOLA", 256, 16)
    wt, wr = np.ones(st.sym_len, np.float32), np.ones(st.rx_win_len, np.float32)
    h, out = np.zeros(42, np.float32), np.zeros(256, np.float32)
    ptrs = [wt.ctypes.data, wr.ctypes.data, h.ctypes.data, out.ctypes.data]
    good = _cfg(st)
    for i in range(4):
        args = list(ptrs)
        args[i] = None
        assert lib.wofdm_interference(C.byref(good), 0, *args) == -1, i
    assert lib.wofdm_interference(None, 0, *ptrs) == -1
    for kw, code in (({"n_fft": 2048}, -2), ({"n_taps": 22}, -2), ({"n_taps": 0}, -2),
                     ({"circ_shift": 256}, -1), ({"tail_rx": 9}, -1), ({"prefix_rm": st.prefix_rm + 1}, -1),
                     ({"n_channels": 0}, -1), ({"n_window_pairs": 0}, -1), ({"cp": 257}, -1),
                     ({"cp": 120, "cs": 16, "prefix_rm": 118}, -2),         # cp + cs > 128
                     ({"cp": 100, "cs": 20, "prefix_rm": 102}, -2)):        # B = N + 112 > the FIR tiling
        assert lib.wofdm_interference(C.byref(_cfg(st, **kw)), 0, *ptrs) == code, kw


def test_tx_psd_abi_refuses_bad_arguments():
    import ctypes as C
    from wofdm_amd import _lib
    lib = _lib.load()
    st = W.make_structure("wtx", 64, 12)
    P = st.sym_len
    w, X, out = np.ones(P, np.float32), np.zeros(2 * 64 * 4, np.float32), np.zeros(512, np.float32)
    ok = (w.ctypes.data, X.ctypes.data)

    def call(cfg, no_symbols=4, overlap=8, ptrs=ok, psd=out.ctypes.data):
        return lib.wofdm_tx_psd(C.byref(cfg) if cfg is not None else None, 0, ptrs[0], ptrs[1], no_symbols,
                                overlap, psd)
    good = _cfg(st)
    assert call(None) == -1
    assert call(good, ptrs=(None, ok[1])) == -1 and call(good, ptrs=(ok[0], None)) == -1
    assert call(good, psd=None) == -1
    assert call(_cfg(st, n_fft=512)) == -2 and call(_cfg(st, n_fft=1024)) == -2
    assert call(good, overlap=P // 2 + 1) == -1 and call(good, overlap=-1) == -1
    assert call(good, no_symbols=0) == -1
    assert call(_cfg(st, cp=65)) == -1 and call(_cfg(st, cs=65)) == -1 and call(_cfg(st, cp=-1)) == -1
