"""``wofdm_interference_masked`` on the GPU (wofdm_interf_pulse_kernel<N> + wofdm_interf_masked_kernel<N>, N = 64 ...
1024): power and wanted power against the fp64 host mirror ``interference.interf_power_masked`` in the three modes
(allocation only, mask only, both), the unmasked call against ``wofdm_interference`` bit for bit, repeatability, the
closed form's three matrices tied to the masked frame kernel (Y[s] = A_0 X[s] + A_1 X[s-1] + A_2 X[s-2]), and the
refusals the header states.

Tolerance (fp32 kernels against fp64): the rule of tests/test_gpu_aux_kernels.py::check_interference, restated here --
|got - want| < 5e-5 max|want| + floor, floor = FLOOR_FACTOR x the deviation of the same mirror evaluated in complex64
(windows, masked pulses, channel and Rx matrix rounded to fp32, products accumulated in fp32) from the fp64 one.
FLOOR_FACTOR = 10, the project's factor.

Worst deviation / bound per N over the cases below (MI355X, all three modes, power and wanted; must stay < 1):
see profiles/interference_masked.txt."""
import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import interference as I
from wofdm_amd import variants as V

from test_interference_masked_host import CASES, nonrc_windows

pytestmark = pytest.mark.gpu

MATERIAL_RTOL = 5e-5
FLOOR_FACTOR = 10
STAGE_RTOL = 2e-5          # as test_gpu_parity.py: fp32 chain of an N <= 1024 FFT + 21-tap FIR vs fp64


def _mirror(st, w_tx, w_rx, h, active, mask, dtype=np.complex128):
    """(power [N], wanted [N]) of the host mirror, evaluated in ``dtype``."""
    U = I.masked_tx_pulse(st, np.asarray(w_tx, np.float64), mask).astype(dtype)
    R = I.rx_matrix(st, np.asarray(w_rx, np.float64)).astype(dtype)
    hh = np.asarray(h).astype(dtype)
    B = st.stride
    conv = np.zeros((3 * B + hh.size - 1, st.n_fft), dtype=dtype)
    for l in range(hh.size):
        conv[l:l + 3 * B] += hh[l] * U
    A = np.stack([R @ conv[m * B:(m + 1) * B] for m in range(3)])
    if active is not None:
        A[:, ~active, :] = 0
        A[:, :, ~active] = 0
    d = np.diag(A[0])
    off = A[0] - np.diag(d)
    p = (np.abs(off) ** 2).sum(axis=1, dtype=np.float64) + (np.abs(A[1:]) ** 2).sum(axis=(0, 2), dtype=np.float64)
    return p, np.abs(d.astype(np.complex128)) ** 2


def check(got_p, got_w, st, w_tx, w_rx, h, active, mask, what):
    """Both outputs under the rule of the module docstring; returns the larger deviation / bound."""
    p64, w64 = _mirror(st, w_tx, w_rx, h, active, mask)
    p32, w32 = _mirror(st, w_tx, w_rx, h, active, mask, np.complex64)
    ref_p, ref_w = I.interf_power_masked(st, w_tx, w_rx, h, active, mask)
    assert np.abs(p64 - ref_p).max() <= 1e-9 * max(np.abs(ref_p).max(), 1e-30) + 1e-20 * w64.max()   # the helper IS the mirror
    assert np.abs(w64 - ref_w).max() <= 1e-12 * w64.max()
    out = 0.0
    for name, got, want, lo in (("power", got_p, p64, p32), ("wanted", got_w, w64, w32)):
        err = float(np.abs(got - want).max())
        tol = MATERIAL_RTOL * np.abs(want).max() + FLOOR_FACTOR * np.abs(lo - want).max()
        print("  %s %s: deviation %.3e, bound %.3e (5e-5 term %.3e), ratio %.3f"
              % (what, name, err, tol, MATERIAL_RTOL * np.abs(want).max(), err / tol))
        assert err < tol, (what, name, err, tol)
        out = max(out, err / tol)
    if active is not None:
        assert np.all(got_p[~active] == 0) and np.all(got_w[~active] == 0)
    return out


MODES = ("alloc", "mask", "both")


@pytest.mark.parametrize("system,n_fft,cp", CASES)
def test_masked_interference_matches_the_mirror(channels, system, n_fft, cp):
    """RC and a non-RC pair x three channels in one call per mode: every [pair, channel] slice against its own mirror."""
    st = W.make_structure(system, n_fft, cp)
    nr = nonrc_windows(st, np.random.RandomState(n_fft + cp))
    w_tx = np.stack([V.tx_rc_window(st), nr[0]]).astype(np.float32)
    w_rx = np.stack([V.rx_rc_window(st), nr[1]]).astype(np.float32)
    h = channels[[3, 40, 77]].astype(np.complex64)
    alloc = CM.half_band_allocation(n_fft)
    gains = CM.tx_mask(st.sym_len).astype(np.float32)
    worst = 0.0
    for mode in MODES:
        active = alloc if mode in ("alloc", "both") else None
        mask = gains if mode in ("mask", "both") else None
        p, w = I.interf_power_masked_gpu(st, w_tx, w_rx, h, active=active, mask=mask)
        assert p.shape == w.shape == (2, 3, n_fft) and p.dtype == np.float32
        for pi in range(2):
            for ci in range(3):
                worst = max(worst, check(p[pi, ci], w[pi, ci], st, w_tx[pi], w_rx[pi], h[ci], active,
                                         None if mask is None else mask.astype(np.float64),
                                         "%s N=%d cp=%d %s pair %d ch %d" % (system, n_fft, cp, mode, pi, ci)))
    print("masked interference %s N=%d cp=%d: worst deviation / bound %.3f" % (system, n_fft, cp, worst))


@pytest.mark.parametrize("system,n_fft,cp", [("WOLA", 64, 12), ("CPW", 128, 20), ("WOLA", 256, 32), ("wrx", 256, 10),
                                             ("WOLA", 512, 32), ("CPW", 1024, 32)])
def test_without_mask_and_allocation_it_is_wofdm_interference(channels, system, n_fft, cp):
    st = W.make_structure(system, n_fft, cp)
    nr = nonrc_windows(st, np.random.RandomState(1))
    w_tx, w_rx = np.stack([V.tx_rc_window(st), nr[0]]), np.stack([V.rx_rc_window(st), nr[1]])
    h = channels[10:13]
    want = I.interf_power_gpu(st, w_tx, w_rx, h)
    p, w = I.interf_power_masked_gpu(st, w_tx, w_rx, h)
    assert np.array_equal(p, want)
    ref = np.array([[I.interf_power_masked(st, w_tx[i], w_rx[i], h[c])[1] for c in range(3)] for i in range(2)])
    assert np.abs(w - ref).max() < MATERIAL_RTOL * ref.max()
    # wanted = NULL: the call is wofdm_interference itself
    import ctypes as C
    cfg = W.make_cfg(st, 4, 16, 21, 3, 1, 2)
    out = np.zeros_like(want)
    wt32, wr32, h32 = _lib.f32(w_tx), _lib.f32(w_rx), _lib.c64_as_f32(h)     # (kept alive across the call)
    _lib.check(_lib.load().wofdm_interference_masked(C.byref(cfg), 0, wt32.ctypes.data, wr32.ctypes.data,
                                                     h32.ctypes.data, None, None, out.ctypes.data, None))
    assert np.array_equal(out, want)


@pytest.mark.parametrize("system,n_fft,cp", [("WOLA", 256, 32), ("CPW", 1024, 32), ("wtx", 64, 16)])
def test_masked_interference_is_repeatable(channels, system, n_fft, cp):
    st = W.make_structure(system, n_fft, cp)
    w_tx, w_rx = np.tile(V.tx_rc_window(st), (3, 1)), np.tile(V.rx_rc_window(st), (3, 1))
    args = dict(active=CM.half_band_allocation(n_fft), mask=CM.tx_mask(st.sym_len))
    a = I.interf_power_masked_gpu(st, w_tx, w_rx, channels[:5], **args)
    b = I.interf_power_masked_gpu(st, w_tx, w_rx, channels[:5], **args)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0][0], a[0][2]) and np.array_equal(a[1][0], a[1][1])      # equal pairs, equal bits
    assert np.isfinite(a[0]).all() and a[0].max() > 0


@pytest.mark.parametrize("system,n_fft,cp", [("WOLA", 64, 12), ("CPwtx", 256, 32), ("wrx", 256, 10), ("WOLA", 512, 32)])
def test_masked_frame_kernel_is_the_three_interference_matrices(channels, system, n_fft, cp):
    """The instrumented masked frame kernel (injected labels and unit noise, 150 dB, allocation + Tx mask): its received
    blocks are A_0 X[s] + A_1 X[s-1] + A_2 X[s-2] with the closed form's matrices -- no oracle in the loop -- and the GPU's
    closed form agrees with the power those matrices give."""
    st = W.make_structure(system, n_fft, cp)
    nr = nonrc_windows(st, np.random.RandomState(n_fft))
    w_tx, w_rx = nr[0].astype(np.float32), nr[1].astype(np.float32)
    h = channels[7].astype(np.complex64)
    active = CM.half_band_allocation(n_fft)
    mask = CM.tx_mask(st.sym_len).astype(np.float32)
    S, seed, cell, frame = 16, 3, 0, 17
    osys = O.make_sys(n_fft, 4, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, 21, 1)
    lab = O.gen_labels(osys, seed, cell, frame)
    noise = O.gen_noise(osys, seed, cell, frame)
    cfg = W.make_cfg(st, 4, S, 21, 1, 1, 1, seed=seed)
    with W.Plan(cfg, w_tx, w_rx, h[None], np.array([150.0], np.float32)) as plan:
        plan.set_allocation(active)
        plan.set_tx_mask(mask)
        assert plan.kernel_id()[1] in (2, 3)
        _, gd = plan.dump_frame(cell, frame, lab, noise.astype(np.complex64))
    X = gd["X"].astype(np.complex128)
    assert np.all(X[:, ~active] == 0)
    A = I.interference_matrices_masked(st, w_tx.astype(np.float64), w_rx.astype(np.float64), h.astype(np.complex128),
                                       active, mask.astype(np.float64))
    want = X @ A[0].T
    want[1:] += X[:-1] @ A[1].T
    want[2:] += X[:-2] @ A[2].T
    err = np.abs(gd["Y"][:, active] - want[:, active]).max() / np.abs(want).max()
    print("masked cross-row %s N=%d: %.2e" % (system, n_fft, err))
    assert err < STAGE_RTOL, err
    p, w = I.interf_power_masked_gpu(st, w_tx, w_rx, h, active=active, mask=mask)
    check(p[0, 0], w[0, 0], st, w_tx, w_rx, h, active, mask.astype(np.float64), "cross-row closed form")


def test_unsupported_geometry_is_refused_and_leaves_the_outputs(channels):
    """The limits include/wofdm.h states for wofdm_interference_masked, on the device that exists: -2, outputs untouched;
    the same geometries one step inside the limits run."""
    import ctypes as C

    def geo(n, cp, cs, ttx, trx):
        return V.Structure("WOLA", n, cp, ttx, trx, cs, cp + cs - ttx - trx, 0)

    def call(st):
        cfg = W.make_cfg(st, 4, 16, 21, 1, 1, 1)
        w_tx, w_rx = np.ones((1, st.sym_len), np.float32), np.ones((1, st.rx_win_len), np.float32)
        h = _lib.c64_as_f32(channels[:1])
        act = CM.half_band_allocation(st.n_fft).astype(np.uint8)
        gains = CM.tx_mask(st.sym_len).astype(np.float32)
        p = np.full((1, 1, st.n_fft), -7.0, np.float32)
        w = np.full((1, 1, st.n_fft), -7.0, np.float32)
        rc = _lib.load().wofdm_interference_masked(C.byref(cfg), 0, w_tx.ctypes.data, w_rx.ctypes.data, h.ctypes.data,
                                                   act.ctypes.data, gains.ctypes.data, p.ctypes.data, w.ctypes.data)
        return rc, p, w

    for st in (geo(256, 65, 16, 17, 64), geo(256, 64, 16, 14, 66), geo(256, 41, 24, 0, 0), geo(1024, 33, 32, 1, 10)):
        rc, p, w = call(st)
        assert rc == -2, st
        assert np.all(p == -7.0) and np.all(w == -7.0)
    for st in (geo(256, 64, 16, 16, 64), geo(256, 40, 24, 0, 0), geo(1024, 32, 32, 0, 10), geo(512, 70, 10, 16, 10),
               geo(64, 60, 20, 16, 64)):
        rc, p, w = call(st)
        assert rc == 0, (st, _lib.load().wofdm_last_error())
        check(p[0, 0], w[0, 0], st, np.ones(st.sym_len), np.ones(st.rx_win_len), channels[0].astype(np.complex64),
              CM.half_band_allocation(st.n_fft), CM.tx_mask(st.sym_len).astype(np.float32).astype(np.float64), st)


def test_interference_for_window_file_gpu_matches_its_host_route(channels):
    from test_interference_masked_host import _windows_for_plan
    st = W.make_structure("WOLA", 256, 32)
    wins = _windows_for_plan(V.matlab_pair_plan("WOLA"), st, np.random.RandomState(4))
    h = channels[20:23]
    got = CM.interference_for_window_file("WOLA", 32, wins, h)
    want = CM.interference_for_window_file("WOLA", 32, wins, h, gpu=False)
    assert list(got) == list(want) and len(got) == 7
    rc = {"rc_tx": V.tx_rc_window(st), "rc_rx": V.rx_rc_window(st)}
    alloc, gains = CM.half_band_allocation(256), CM.tx_mask(st.sym_len)
    for name, (ktx, krx) in V.matlab_pair_plan("WOLA"):
        wt = (rc["rc_tx"] if ktx == "rc" else wins[ktx]).astype(np.float32)
        wr = (rc["rc_rx"] if krx == "rc" else wins[krx]).astype(np.float32)
        for ci in range(3):
            hc = h[ci].astype(np.complex64)
            for sfx, mask in (("", None), ("_masked", gains.astype(np.float32).astype(np.float64))):
                assert got[name]["power" + sfx].shape == (3, 256)
                check(got[name]["power" + sfx][ci], got[name]["wanted" + sfx][ci], st, wt, wr, hc, alloc, mask,
                      "window file %s%s ch %d" % (name, sfx, ci))
                assert np.abs(got[name]["power" + sfx][ci] - want[name]["power" + sfx][ci]).max() \
                    < 1e-3 * want[name]["power" + sfx][ci].max() + 1e-9 * want[name]["wanted" + sfx][ci].max()
