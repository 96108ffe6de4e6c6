"""Closed-form ICI + ISI power of a w-OFDM structure (host, numpy) -- SURVEY.md 8f row f2.

Mirrors ``calculate_interference`` (matlab/main_interference_calculation.m:177-225) and
``interf_power`` (python/ofdm_utils/interf_calc.py:20-113):

    A_m = W K P V_rx R  H_m  V_tx Gamma W^-1,      H_m[b, c] = h[m (N+mu+rho-beta) + b - c]
    P[n] = sum_{n' != n} |A_0[n, n']|^2 + sum_{m >= 1} sum_{n'} |A_m[n, n']|^2

built from the same index formulas as the kernels (no dense DFT loops): the Tx map is an IDFT
matrix with rows picked by the CP/CS copy and scaled by the Tx window, the Rx map is the DFT of
the windowed fold of SURVEY.md 3.4-10.  It is the deterministic companion of every BER curve
and an analytic, RNG-free check of the frame pipeline.

``interference_matrices_masked`` / ``interf_power_masked`` are the same closed form for the system of
matlab/main_channel_mask.m (half-band loading, 387-390; the spectral Tx mask ``dft_rc_filt``, 398-417): the mask's
spill into the next symbol's row makes the pulse three periods long, A_m with m = 0, 1, 2, and the wanted term
|A_0[n, n]|^2 is returned beside the power because the mask attenuates it too.
"""
import numpy as np


def tx_matrix(st, w_tx):
    """[P, N]: V_tx Gamma W^-1 (transmitter.py:13-58, wofdm_simulation.py:464)."""
    n = st.n_fft
    i = np.arange(st.sym_len)
    t = (i - st.cp) % n
    return np.asarray(w_tx)[:, None] * np.exp(2j * np.pi * np.outer(t, np.arange(n)) / n) / n


def rx_matrix(st, w_rx):
    """[N, B]: W K P V_rx R (receiver.py:13-133, wofdm_simulation.py:468-469)."""
    n, delta = st.n_fft, st.tail_rx
    fold = np.zeros((n, st.stride))
    for t in range(n):
        m0 = (t + st.circ_shift + delta // 2) % n
        fold[t, st.prefix_rm + m0] += w_rx[m0]
        if m0 + n < n + delta:
            fold[t, st.prefix_rm + m0 + n] += w_rx[m0 + n]
    return np.fft.fft(fold, axis=0)


def channel_tensor(st, h):
    """[M, B, P] with H_m[b, c] = h[m*B + b - c] (channel.py:14-53, channel_array.m:20-36)."""
    h = np.asarray(h).reshape(-1)
    B, P = st.stride, st.sym_len
    M = 1 + int(np.ceil((h.size - 1 + st.tail_tx) / B))
    idx = (np.arange(M)[:, None, None] * B + np.arange(B)[None, :, None] - np.arange(P)[None, None, :])
    ok = (idx >= 0) & (idx < h.size)
    return np.where(ok, h[np.clip(idx, 0, h.size - 1)], 0)


def interference_matrices(st, w_tx, w_rx, h):
    """(A_0 [N, N], A_m [M-1, N, N])."""
    T, R, H = tx_matrix(st, w_tx), rx_matrix(st, w_rx), channel_tensor(st, h)
    A = R @ H @ T
    return A[0], A[1:]


def interf_power(st, w_tx, w_rx, h):
    """Per-subcarrier ICI + ISI power, ``np.diag(PISI + PICI1)`` of interf_calc.py:91-100."""
    a0, am = interference_matrices(st, w_tx, w_rx, h)
    off = a0 - np.diag(np.diag(a0))
    return (np.abs(off) ** 2).sum(axis=1) + (np.abs(am) ** 2).sum(axis=(0, 2))


def total_interference(st, w_tx, w_rx, h):
    """Scalar of the MATLAB function: tr(offdiag(A0)^H offdiag(A0)) + sum_m tr(A_m^H A_m)."""
    return float(interf_power(st, w_tx, w_rx, h).sum())


def masked_tx_pulse(st, w_tx, mask=None):
    """[3 B, N]: the on-air pulse of a unit symbol on every bin under the spectral Tx mask (``dft_rc_filt``,
    matlab/main_channel_mask.m:398-417; semantics of ``wofdm_plan_set_tx_mask``): the Tx column zero-padded to
    2P-1, times the DFT-domain gains, transformed back; samples [0, P) stay in the symbol's row, [P, 2P-1) are
    added to the next row, which goes on air B later.  ``mask=None``: the Tx column itself."""
    P, B = st.sym_len, st.stride
    T = tx_matrix(st, w_tx)
    U = np.zeros((3 * B, st.n_fft), dtype=np.complex128)
    if mask is None:
        U[:P] = T
        return U
    mask = np.asarray(mask, dtype=np.float64).reshape(-1)
    if mask.size != 2 * P - 1:
        raise ValueError("the mask needs 2 P - 1 = %d gains, got %d" % (2 * P - 1, mask.size))
    y = np.fft.ifft(np.fft.fft(T, 2 * P - 1, axis=0) * mask[:, None], axis=0)
    U[:P] = y[:P]
    U[B:B + P - 1] += y[P:]
    return U


def interference_matrices_masked(st, w_tx, w_rx, h, active=None, mask=None):
    """A [3, N, N] of the half-band / masked system (matlab/main_channel_mask.m:387-390, 398-417):
    A_m[:, n'] = rx_matrix . conv(h, pulse of bin n')[m B : (m + 1) B], m = 0, 1, 2 -- the mask's spill into the
    next row makes the pulse longer than two periods, it ends before the fourth.  Columns of unloaded bins are
    dropped, rows of unloaded bins are zero.  ``active=None, mask=None``: ``interference_matrices`` with A[2] = 0."""
    h = np.asarray(h).reshape(-1)
    B = st.stride
    if B + st.sym_len - 1 + h.size - 1 > 3 * B:
        raise ValueError("the filtered pulse does not end within three symbol periods")
    U = masked_tx_pulse(st, w_tx, mask)
    conv = np.zeros((3 * B + h.size - 1, st.n_fft), dtype=np.complex128)
    for l in range(h.size):
        conv[l:l + 3 * B] += h[l] * U
    R = rx_matrix(st, w_rx)
    A = np.stack([R @ conv[m * B:(m + 1) * B] for m in range(3)])
    if active is not None:
        active = np.asarray(active).astype(bool).reshape(-1)
        if active.size != st.n_fft:
            raise ValueError("the allocation needs n_fft = %d flags, got %d" % (st.n_fft, active.size))
        A[:, ~active, :] = 0
        A[:, :, ~active] = 0
    return A


def interf_power_masked(st, w_tx, w_rx, h, active=None, mask=None):
    """(power [N], wanted [N]): sum_{n' != n} |A_0[n, n']|^2 + sum_{m = 1, 2} sum_{n'} |A_m[n, n']|^2 and
    |A_0[n, n]|^2 of ``interference_matrices_masked`` (the mask attenuates the wanted term too: SIR needs both)."""
    A = interference_matrices_masked(st, w_tx, w_rx, h, active, mask)
    d = np.diag(A[0])
    off = A[0] - np.diag(d)
    return (np.abs(off) ** 2).sum(axis=1) + (np.abs(A[1:]) ** 2).sum(axis=(0, 2)), np.abs(d) ** 2


def interf_power_gpu(st, w_tx, w_rx, h, device=0):
    """The same per-subcarrier power on the GPU (``wofdm_interference``: the frame kernels' own Tx /
    FIR / Rx chain applied to the N unit symbols, one workgroup per (window pair, channel)), batched:
    w_tx [pairs][P], w_rx [pairs][N + tail_rx], h [n_channels][taps]  ->  float32 [pairs][n_channels][N].
    No CPU fallback."""
    import ctypes as C
    from . import _lib
    from .simulation import make_cfg
    w_tx = _lib.f32(np.atleast_2d(w_tx))
    w_rx = _lib.f32(np.atleast_2d(w_rx))
    hh = np.atleast_2d(np.asarray(h))
    if w_tx.shape != (w_rx.shape[0], st.sym_len) or w_rx.shape[1] != st.rx_win_len:
        raise ValueError("window shapes %s / %s do not fit the structure" % (w_tx.shape, w_rx.shape))
    cfg = make_cfg(st, 4, 16, hh.shape[1], hh.shape[0], 1, w_tx.shape[0])
    hf = _lib.c64_as_f32(hh, (cfg.n_channels, cfg.n_taps))
    out = np.zeros((w_tx.shape[0], hh.shape[0], st.n_fft), dtype=np.float32)
    lib = _lib.load()
    _lib.check(lib.wofdm_interference(C.byref(cfg), int(device), w_tx.ctypes.data, w_rx.ctypes.data,
                                      hf.ctypes.data, out.ctypes.data))
    return out


def interf_power_masked_gpu(st, w_tx, w_rx, h, active=None, mask=None, device=0):
    """``interf_power_masked`` on the GPU (``wofdm_interference_masked``: the masked Tx pulses once per window
    pair, then one workgroup per (window pair, channel) over three symbol periods), batched like
    ``interf_power_gpu``: (power, wanted), float32 [pairs][n_channels][N] each.  No CPU fallback."""
    import ctypes as C
    from . import _lib
    from .simulation import make_cfg
    w_tx = _lib.f32(np.atleast_2d(w_tx))
    w_rx = _lib.f32(np.atleast_2d(w_rx))
    hh = np.atleast_2d(np.asarray(h))
    if w_tx.shape != (w_rx.shape[0], st.sym_len) or w_rx.shape[1] != st.rx_win_len:
        raise ValueError("window shapes %s / %s do not fit the structure" % (w_tx.shape, w_rx.shape))
    cfg = make_cfg(st, 4, 16, hh.shape[1], hh.shape[0], 1, w_tx.shape[0])
    hf = _lib.c64_as_f32(hh, (cfg.n_channels, cfg.n_taps))
    act = None if active is None else np.ascontiguousarray(np.asarray(active).astype(bool), dtype=np.uint8)
    if act is not None and act.shape != (st.n_fft,):
        raise ValueError("the allocation needs n_fft = %d flags, got shape %s" % (st.n_fft, act.shape))
    gains = None if mask is None else _lib.f32(np.asarray(mask).reshape(-1), (2 * st.sym_len - 1,))
    power = np.zeros((w_tx.shape[0], hh.shape[0], st.n_fft), dtype=np.float32)
    wanted = np.zeros_like(power)
    lib = _lib.load()
    _lib.check(lib.wofdm_interference_masked(C.byref(cfg), int(device), w_tx.ctypes.data, w_rx.ctypes.data,
                                             hf.ctypes.data, None if act is None else act.ctypes.data,
                                             None if gains is None else gains.ctypes.data, power.ctypes.data,
                                             wanted.ctypes.data))
    return power, wanted
