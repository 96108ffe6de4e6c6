"""Closed-form ICI + ISI of the half-band, spectrally masked system without a GPU: the fp64 host mirror
(``interference.interference_matrices_masked`` / ``interf_power_masked``) against the unmasked mirror and, by
linearity, against the oracle's masked frame pipeline; the cost of the mask pinned; the argument checks of
``wofdm_interference_masked`` (all made before the device is touched); the host route of
``channel_mask.interference_for_window_file``.

Bounds: the unmasked agreement is two orders of summation of the same fp64 products (1e-12 of max|A|); the
linearity check compares two fp64 evaluations of the same linear map on |Y| ~ 3 with the oracle's noise at 300 dB
(1e-15 of the signal): 1e-11 of max|Y|."""
import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import interference as I
from wofdm_amd import variants as V

#: (system, n_fft, cp) of the linearity check and of the GPU tests
CASES = [("wtx", 64, 16), ("WOLA", 64, 12), ("CPW", 128, 20), ("CPwtx", 256, 32), ("wrx", 256, 10),
         ("WOLA", 512, 32), ("CPW", 1024, 32), ("CP", 256, 32)]


def nonrc_windows(st, rs):
    """A non-RC pair: tails from sorted uniforms, flat levels != 1."""
    xt = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(.02, .98, st.tail_tx))[::-1]))
    xr = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(.02, .48, st.tail_rx // 2))[::-1]))
    return (V.expand_tx_window(st, xt) if st.tail_tx else np.full(st.sym_len, xt[0]),
            V.expand_rx_window(st, xr) if st.tail_rx else np.full(st.rx_win_len, xr[0]))


@pytest.mark.parametrize("n_fft", [64, 128, 256, 512, 1024])
def test_masked_mirror_without_mask_and_allocation_is_the_plain_one(channels, n_fft):
    for system in ("WOLA", "CP", "wrx"):
        st = W.make_structure(system, n_fft, 12)
        wt, wr = nonrc_windows(st, np.random.RandomState(n_fft))
        a0, am = I.interference_matrices(st, wt, wr, channels[3])
        A = I.interference_matrices_masked(st, wt, wr, channels[3])
        assert A.shape == (3, n_fft, n_fft) and am.shape[0] == 1
        scale = np.abs(a0).max()
        assert np.abs(A[0] - a0).max() <= 1e-12 * scale and np.abs(A[1] - am[0]).max() <= 1e-12 * scale
        assert np.all(A[2] == 0)
        p, wanted = I.interf_power_masked(st, wt, wr, channels[3])
        want = I.interf_power(st, wt, wr, channels[3])
        assert np.abs(p - want).max() <= 1e-12 * scale ** 2
        assert np.abs(wanted - np.abs(np.diag(a0)) ** 2).max() <= 1e-12 * scale ** 2


@pytest.mark.parametrize("system,n_fft,cp", CASES)
def test_oracle_masked_frame_is_the_three_interference_matrices(channels, system, n_fft, cp):
    """Half-band allocation + the raised-cosine Tx mask, random labels, 300 dB: the oracle's received blocks are
    Y[s] = sum_{m <= min(s, 2)} A_m X[s - m] on the loaded bins."""
    S, k, seed, cell, frame = 6, 4, 11, 0, 5
    st = W.make_structure(system, n_fft, cp)
    wt, wr = nonrc_windows(st, np.random.RandomState(n_fft + cp))
    h = channels[3]
    active = CM.half_band_allocation(n_fft)
    mask = CM.tx_mask(st.sym_len)
    osys = O.make_sys(n_fft, k, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, h.size, 1,
                      active=active, tx_mask=mask)
    lab = np.random.RandomState(seed).randint(0, 1 << k, size=(S, n_fft)).astype(np.uint8)
    noise = O.gen_noise(osys, seed, cell, frame)
    _, od = O.frame(osys, wt, wr, h, 300.0, lab, noise, dump=True)
    X = od["X"].copy()
    X[:, ~active] = 0
    A = I.interference_matrices_masked(st, wt, wr, h, active, mask)
    want = np.zeros((S, n_fft), dtype=np.complex128)
    for s in range(S):
        for m in range(min(s, 2) + 1):
            want[s] += A[m] @ X[s - m]
    err = np.abs(od["Y"][:, active] - want[:, active]).max()
    scale = np.abs(od["Y"][:, active]).max()
    print("%s N=%d cp=%d: |Y - sum A_m X| = %.2e at max|Y| = %.2f" % (system, n_fft, cp, err, scale))
    assert err < 1e-11 * scale, (err, scale)
    # and the third period is needed: without A_2 the prediction is off by far more than the bound
    short = want - np.concatenate([np.zeros((2, n_fft)), X[:-2] @ A[2].T])
    if np.abs(A[2]).max() > 0:
        assert np.abs(od["Y"][:, active] - short[:, active]).max() > 1e3 * 1e-11 * scale
    assert np.all(want[:, ~active] == 0)


def test_the_mask_lays_an_interference_floor(channels):
    """CP-OFDM, N = 256, cp 32 > L - 1: no interference under half-band loading alone, a floor of ~2e-3 of the wanted
    power under the mask, which also changes the wanted power."""
    st = W.make_structure("CP", 256, 32)
    wt, wr = np.ones(st.sym_len), np.ones(st.rx_win_len)
    active = CM.half_band_allocation(256)
    p0, w0 = I.interf_power_masked(st, wt, wr, channels[3], active=active)
    p1, w1 = I.interf_power_masked(st, wt, wr, channels[3], active=active, mask=CM.tx_mask(st.sym_len))
    # total interference in units of the largest wanted power max_n |A_0[n, n]|^2 (~4.36 here; the unit of
    # tests/test_gpu_aux_kernels.py's floor): 9e-26 / 4.36 with the allocation alone, 8.0e-3 / 4.36 = 1.8e-3 with the mask
    print("allocation only: %.2e, with mask: %.2e of the wanted power %.3f" % (p0.sum() / w0.max(), p1.sum() / w1.max(),
                                                                               w0.max()))
    assert p0.sum() < 1e-20 * w0.max()
    assert p1.sum() > 1e-4 * w1.max()
    assert np.all(p0[~active] == 0) and np.all(w0[~active] == 0) and np.all(p1[~active] == 0)
    assert np.abs(w1 - w0)[active].max() > 1e-6 * w0.max()
    with pytest.raises(ValueError):
        I.interf_power_masked(st, wt, wr, channels[3], mask=np.ones(2 * st.sym_len))
    with pytest.raises(ValueError):
        I.interf_power_masked(st, wt, wr, channels[3], active=np.ones(128, bool))


# ---------------------------------------------------------------------------------------------
# argument checks of wofdm_interference_masked: host-side, before any device is touched

def _call(st=None, device=0, n_taps=21, pairs=1, n_ch=1, mask="ones", active="half", null=(), tweak=None):
    st = W.make_structure("WOLA", 256, 32) if st is None else st
    cfg = W.make_cfg(st, 4, 16, n_taps, n_ch, 1, pairs)
    if tweak:
        for key, val in tweak.items():
            setattr(cfg, key, val)
    n = max(int(cfg.n_fft), 1)
    P = max(n + cfg.cp + cfg.cs, 1)
    bufs = {"w_tx": np.ones((pairs, P + 64), np.float32), "w_rx": np.ones((pairs, n + 128), np.float32),
            "h": np.ones((n_ch, n_taps, 2), np.float32),
            "active": None if active is None else (np.arange(n) < n // 2).astype(np.uint8) if isinstance(active, str)
            else np.asarray(active, np.uint8),
            "mask": None if mask is None else np.ones(2 * P - 1, np.float32) if isinstance(mask, str)
            else np.asarray(mask, np.float32),
            "power": np.full((pairs, n_ch, n), -7.0, np.float32),
            "wanted": np.full((pairs, n_ch, n), -7.0, np.float32)}
    ptr = {k: (None if v is None or k in null else v.ctypes.data) for k, v in bufs.items()}
    import ctypes as C
    rc = _lib.load().wofdm_interference_masked(None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"],
                                               ptr["h"], ptr["active"], ptr["mask"], ptr["power"], ptr["wanted"])
    assert np.all(bufs["power"] == -7.0) and np.all(bufs["wanted"] == -7.0) or rc == 0
    return rc


def test_interference_masked_refuses_bad_arguments():
    for k in ("cfg", "w_tx", "w_rx", "h", "power"):
        assert _call(null=(k,)) == -1, k
    for n in (32, 192, 2048, 0):
        assert _call(tweak={"n_fft": n}) == -2, n
    st = W.make_structure("WOLA", 256, 32)
    L = 2 * st.sym_len - 1
    for bad in (np.nan, np.inf, -np.inf):
        gains = np.ones(L)
        gains[L // 3] = bad
        assert _call(mask=gains) == -1, bad
    assert _call(active=np.zeros(256)) == -1                       # nothing loaded
    assert _call(n_taps=22) == -2 and _call(n_taps=0) == -2
    assert _call(tweak={"tail_rx": 11}) == -1                      # odd tail_rx
    # whatever passes the checks reaches the device: a device that does not exist is the HIP error
    assert _call(device=99) == -3 and _call(device=-1) == -3
    for null in (("wanted",), ("mask",), ("active",), ("mask", "active"), ("mask", "active", "wanted")):
        assert _call(device=99, null=null) == -3, null
    for n_fft in (64, 128, 512, 1024):
        assert _call(st=W.make_structure("CPW", n_fft, 32), device=99) == -3, n_fft
    assert "device" in _lib.load().wofdm_last_error().decode()


def test_interference_masked_geometry_limits_are_those_of_the_header():
    """include/wofdm.h: cp + cs - tail_tx <= 64, tail_tx <= 16, tail_rx <= 64, cp + cs <= 64 at n_fft = 1024:
    each limit is met exactly (-3: only the missing device stops the call) and crossed by one (-2)."""
    def geo(n, cp, cs, ttx, trx):
        return V.Structure("WOLA", n, cp, ttx, trx, cs, n + cp + cs - ttx - n - trx, 0)
    ok = [geo(256, 64, 16, 16, 64), geo(256, 40, 24, 0, 0), geo(1024, 32, 32, 0, 10), geo(64, 60, 20, 16, 64),
          geo(512, 70, 10, 16, 10)]
    for st in ok:
        assert st.stride == st.n_fft + st.tail_rx + st.prefix_rm
        assert _call(st=st, device=99) == -3, st
    bad = [geo(256, 65, 16, 17, 64),        # tail_tx 17
           geo(256, 64, 16, 14, 66),        # tail_rx 66
           geo(256, 41, 24, 0, 0),          # cp + cs - tail_tx = 65
           geo(1024, 33, 32, 1, 10)]        # cp + cs = 65 at n_fft = 1024
    for st in bad:
        assert st.stride == st.n_fft + st.tail_rx + st.prefix_rm
        assert _call(st=st, device=99) == -2, st
    assert _call(tweak={"n_window_pairs": 65536}, device=99) == -2      # refused before any buffer is read


def test_interference_masked_is_declared_bound_and_exported():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wofdm.h")).read()
    assert re.search(r"^int wofdm_interference_masked\(const wofdm_cfg \*cfg, int device, const float \*w_tx,", hdr, flags=re.M)
    flat = re.sub(r"\s*\n \* ", " ", hdr)
    assert "main_channel_mask.m:387-390" in flat and "main_channel_mask.m:398-417" in flat
    assert "main_interference_calculation.m:177-225" in flat
    assert "wofdm_interference_masked" in _lib.EXPORTS and hasattr(_lib.load(), "wofdm_interference_masked")


# ---------------------------------------------------------------------------------------------
# channel_mask.interference_for_window_file, host route

def test_interference_for_window_file_host_route(channels):
    st = W.make_structure("WOLA", 64, 12)
    rs = np.random.RandomState(2)
    plan = V.matlab_pair_plan("WOLA")
    wins = _windows_for_plan(plan, st, rs)
    h = channels[3:6]
    out = CM.interference_for_window_file("WOLA", 12, wins, h, num_subcar=64, gpu=False)
    assert list(out) == [name for name, _ in plan] and len(out) == 7
    for name, res in out.items():
        assert set(res) == {"power", "power_masked", "wanted", "wanted_masked"}
        for v in res.values():
            assert v.shape == (3, 64) and v.dtype == np.float64
    active = CM.half_band_allocation(64)
    wt, wr = V.tx_rc_window(st), V.rx_rc_window(st)
    for ci in range(3):
        p0, w0 = I.interf_power_masked(st, wt, wr, h[ci], active=active)
        p1, w1 = I.interf_power_masked(st, wt, wr, h[ci], active=active, mask=CM.tx_mask(st.sym_len))
        assert np.array_equal(out["rc"]["power"][ci], p0) and np.array_equal(out["rc"]["wanted"][ci], w0)
        assert np.array_equal(out["rc"]["power_masked"][ci], p1) and np.array_equal(out["rc"]["wanted_masked"][ci], w1)
    assert not np.array_equal(out["rc"]["power"], out["1A"]["power"])


def _windows_for_plan(plan, st, rs):
    """a window 'file': one array per key the pair plan names (Tx keys of length P, Rx keys of length N + tail_rx)"""
    wins = {}
    for _, (ktx, krx) in plan:
        wt, wr = nonrc_windows(st, rs)
        if ktx != "rc":
            wins.setdefault(ktx, wt)
        if krx != "rc":
            wins.setdefault(krx, wr)
    return wins
