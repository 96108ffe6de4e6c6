"""Tx-side spectrum analysis (host, numpy) -- SURVEY.md 8f row f4.

Mirrors ``python/ofdm_utils/timefreq_simulation.py``: the averaged-periodogram PSD estimate of
the transmitted w-OFDM waveform (lines 101-123), the out-of-band-radiation figure and main-band
samples (216-296), the closed-form PSD (155-214) and the per-(system, CP) work item with its
``timefreq/{opt,rc}_<sys>_<cp>.npz`` / ``CP_<cp>.npz`` outputs (17-76).

The Tx chain is the same index arithmetic as the BER kernels' phase A (IDFT, CP/CS copy, window,
overlap-add of the tails) written with FFTs; no dense matrices.  Reference behaviours kept:
16-QAM symbols are *not* normalised (line 239), the last (partial, zero-padded) periodogram slice
counts as a full one in the average (118-121), the cosine term of the closed form takes
``f/delta_f`` without the 2 pi (207-213).
"""
import os

import numpy as np

from . import variants as V

#: timefreq_simulation.py:235-238
SYMBOLS_16QAM = np.array([a + 1j * b for a in (-3, -1, 1, 3) for b in (-3, -1, 1, 3)])
NO_SYMBOLS = 256          # line 219
GUARD_BAND = 48           # line 220


def allocation_index(n_fft, guard_band=GUARD_BAND):
    """Bins that carry data (subcar_alloc_mat, lines 223-233): 1..N/2-gb and N/2+gb..N-1."""
    half = n_fft // 2 - guard_band
    return np.r_[1:1 + half, n_fft // 2 + guard_band:n_fft]


def draw_symbols(n_fft, rng=None, no_symbols=NO_SYMBOLS, guard_band=GUARD_BAND):
    """[N-2gb, no_symbols] 16-QAM draw of line 240; ``rng`` a ``RandomState`` (the reference
    uses numpy's global legacy generator) or None for a fresh one."""
    rng = np.random.RandomState() if rng is None else rng
    return rng.choice(SYMBOLS_16QAM, size=(n_fft - 2 * guard_band, no_symbols), replace=True)


def tx_symbols(st, X, w_tx, guard_band=GUARD_BAND):
    """[no_symbols, P]: window x (CP/CS copy of the IDFT of the allocated bins), lines 242-246."""
    n = st.n_fft
    grid = np.zeros((n, X.shape[1]), dtype=np.complex128)
    grid[allocation_index(n, guard_band)] = X
    t = np.fft.ifft(grid, axis=0)                     # idft_mat = conj(DFT)/N
    idx = (np.arange(st.sym_len) - st.cp) % n
    return (np.asarray(w_tx)[:, None] * t[idx]).T


def overlap_and_add(x, beta):
    """[S, P] -> serialised frame (lines 84-99)."""
    if beta == 0:
        return x.reshape(-1)
    body = x[:, beta:].copy()
    body[:-1, -beta:] += x[1:, :beta]
    return np.concatenate([x[0, :beta], body.reshape(-1)])


def mask_rows(rows, mask):
    """Spectral Tx mask on [S, P] rows (``dft_rc_filt``, main_channel_mask.m:398-417, for any gain vector; the
    semantics of ``wofdm_plan_set_tx_mask``): every row zero-padded to L = 2P-1, its DFT times ``mask`` [L]
    (real gains, natural bin order), back; the first P samples replace the row, the other P-1 are added to
    the head of the NEXT row (no spill into the first row, the last row's spill is dropped)."""
    rows = np.asarray(rows, dtype=np.complex128)
    P = rows.shape[1]
    L = 2 * P - 1
    mask = np.asarray(mask, dtype=np.float64).reshape(-1)
    if mask.shape != (L,):
        raise ValueError("mask must hold 2 P - 1 = %d gains, got %s" % (L, mask.shape))
    y = np.fft.ifft(np.fft.fft(rows, L, axis=1) * mask[None, :], axis=1)
    out = y[:, :P].copy()
    out[1:, :P - 1] += y[:-1, P:]
    return out


def tx_waveform(st, X, w_tx, overlap, mask=None, guard_band=GUARD_BAND, pa=None):
    """fp64 host mirror of the waveform the spectrum kernels transmit: ``overlap_and_add`` of the
    ``tx_symbols``, each passed through ``mask_rows`` first when ``mask`` [2P-1] is given.  X as
    ``draw_symbols`` gives it, or [N, S] on every bin with guard_band=None.  pa: an amplifier
    (``rx_profile.PaPoint`` or (model, ibo_db, smooth)) behind the finished waveform, as ``wofdm_tx_psd_batch_pa``
    places it: its back-off counts from the mean of |x|^2 over the WHOLE waveform, the last ramp-down included
    (``rx_profile.pa_apply``); a waveform without power passes unchanged."""
    if guard_band is None:
        t = np.fft.ifft(np.asarray(X, dtype=np.complex128), axis=0)
        rows = (np.asarray(w_tx)[:, None] * t[(np.arange(st.sym_len) - st.cp) % st.n_fft]).T
    else:
        rows = tx_symbols(st, X, w_tx, guard_band)
    if mask is not None:
        rows = mask_rows(rows, mask)
    x = overlap_and_add(rows, overlap)
    if pa is not None:
        from . import rx_profile as R
        ref = float(np.mean(np.abs(x) ** 2))
        if ref > 0:
            x = R.pa_apply(x, pa, ref)
    return x


def psd_estimate(x, fft_len):
    """Mean of |fftshift(FFT)|^2 over consecutive length-``fft_len`` slices, the zero-padded
    remainder included as one more slice (lines 101-123)."""
    n_full = len(x) // fft_len
    acc = (np.abs(np.fft.fft(x[:n_full * fft_len].reshape(n_full, fft_len), axis=1)) ** 2).sum(axis=0)
    rest = x[n_full * fft_len:]
    if rest.size:
        acc = acc + np.abs(np.fft.fft(rest, fft_len)) ** 2
    return np.fft.fftshift(acc) / (n_full + 1)


def _full_grid(n, X, guard_band=GUARD_BAND):
    """[N - 2 gb, S] symbols -> [S, N] complex64 grid, zeros on the unloaded bins"""
    X = np.asarray(X)
    grid = np.zeros((X.shape[1], n), dtype=np.complex64)
    grid[:, allocation_index(n, guard_band)] = X.T
    return grid


def psd_estimate_gpu(st, X, w_tx, overlap, guard_band=GUARD_BAND, device=0, mask=None):
    """``psd_estimate(tx_waveform(st, X, w_tx, overlap, mask), 8 N)`` on the GPU
    (``wofdm_tx_psd``: the frame kernel's Tx half on the given symbols + the averaged periodogram).
    X: [N - 2 gb, no_symbols] like ``draw_symbols``.  No CPU fallback; N in {64, 128, 256} by
    ``wofdm_tx_psd``, N = 512 / 1024 by ``wofdm_tx_psd_batch`` (one job); with a spectral Tx mask
    ([2P-1] gains) by ``wofdm_tx_psd_batch_masked`` at every N."""
    import ctypes as C
    from . import _lib
    from .simulation import make_cfg
    n = st.n_fft
    grid = _full_grid(n, X, guard_band)
    if mask is not None:
        return tx_psd_batch_gpu(n, grid[None], [(0, st.cp, st.cs, overlap, w_tx, mask)], device)[0]
    if n > 256:
        return tx_psd_batch_gpu(n, grid[None], [(0, st.cp, st.cs, overlap, w_tx)], device)[0]
    w = _lib.f32(np.asarray(w_tx).reshape(-1), (st.sym_len,))
    cfg = make_cfg(st, 4, 16, 1, 1, 1, 1)
    out = np.zeros(8 * n, dtype=np.float32)
    gf = _lib.c64_as_f32(grid)
    _lib.check(_lib.load().wofdm_tx_psd(C.byref(cfg), int(device), w.ctypes.data, gf.ctypes.data,
                                        int(grid.shape[0]), int(overlap), out.ctypes.data))
    length = overlap + grid.shape[0] * (st.sym_len - overlap)
    return out.astype(np.float64) / (length // (8 * n) + 1)


def tx_psd_batch_gpu(n_fft, grids, jobs, device=0, divide=True, power=False):
    """Averaged periodograms of many Tx waveforms in one ``wofdm_tx_psd_batch`` call, any N in
    {64, ..., 1024}.  grids: [n_blocks, no_symbols, N] complex symbols on every bin (as given);
    jobs: sequence of (block, cp, cs, overlap, w_tx) or (block, cp, cs, overlap, w_tx, mask), w_tx of
    length P = N + cp + cs, mask None or the [2P-1] DFT-domain gains of a spectral Tx mask
    (``mask_rows``).  A call with any mask goes through ``wofdm_tx_psd_batch_masked`` (equal masks
    share one table entry; masked jobs need 3P-2 <= 8N), the others through ``wofdm_tx_psd_batch``.
    Returns [n_jobs, 8 N] float64: ``psd_estimate(tx_waveform(...), 8 N)`` of each job's waveform, i.e.
    the kernel's slice sums divided by the reference's slice count (length // 8 N + 1); with
    divide=False the undivided float32 sums.  A job may carry a seventh field, pa: None or the amplifier
    behind its finished waveform (``rx_profile.PaPoint`` or (model, ibo_db, smooth); its back-off counts from the
    mean power of the job's whole waveform, measured on the device).  A call with any such field, or with
    power=True, goes through ``wofdm_tx_psd_batch_pa`` (equal points share one table entry, at most
    ``_lib.PA_MAX_POINTS`` of them); calls without go exactly where they went.  power=True: returns (periodograms,
    job_power [n_jobs, 2] float32 = the mean power of every job's waveform before and behind its amplifier).
    No CPU fallback."""
    import ctypes as C
    from . import _lib
    n = int(n_fft)
    grids = np.asarray(grids)
    if grids.ndim != 3 or grids.shape[2] != n:
        raise ValueError("grids must be [n_blocks, no_symbols, %d], got %s" % (n, grids.shape))
    n_blocks, no_symbols = grids.shape[:2]
    jobs = [tuple(j) + (None,) * (7 - len(j)) for j in jobs]
    use_pa = bool(power) or any(j[6] is not None for j in jobs)
    pa_tab, pa_of = [], {}
    job_pa = np.full(max(1, len(jobs)), -1, dtype=np.int32)
    cj = (_lib.PsdJob * max(1, len(jobs)))()
    wins, lengths, tables, table_of = [], [], [], {}
    job_mask = np.full(max(1, len(jobs)), -1, dtype=np.int32)
    for j, (block, cp, cs, overlap, w, mask, pa) in enumerate(jobs):
        cj[j].block, cj[j].cp, cj[j].cs, cj[j].overlap = int(block), int(cp), int(cs), int(overlap)
        wins.append(_lib.f32(np.asarray(w).reshape(-1), (n + cp + cs,)))
        lengths.append(overlap + no_symbols * (n + cp + cs - overlap))
        if mask is not None:
            m = _lib.f32(np.asarray(mask).reshape(-1), (2 * (n + cp + cs) - 1,))
            job_mask[j] = table_of.setdefault(m.tobytes(), len(tables))
            if job_mask[j] == len(tables):
                tables.append(m)
        if pa is not None:
            from . import rx_profile as R
            q = R._pa_point(pa)
            job_pa[j] = pa_of.setdefault(q, len(pa_tab))
            if job_pa[j] == len(pa_tab):
                pa_tab.append(q)
    w_all = _lib.f32(np.concatenate(wins) if wins else np.zeros(1))
    gf = _lib.c64_as_f32(grids)
    out = np.zeros((max(1, len(jobs)), 8 * n), dtype=np.float32)
    jpow = np.zeros((max(1, len(jobs)), 2), dtype=np.float32)
    if use_pa:
        mask_len = np.array([t.size for t in tables] or [0], dtype=np.int32)
        gains = _lib.f32(np.concatenate(tables) if tables else np.zeros(1))
        cpa = (_lib.PaPoint * max(1, len(pa_tab)))(*[_lib.PaPoint(q.model, q.ibo_db, q.smooth, 0) for q in pa_tab])
        _lib.check(_lib.load().wofdm_tx_psd_batch_pa(
            n, int(device), len(jobs), C.addressof(cj), w_all.ctypes.data, len(tables), mask_len.ctypes.data,
            gains.ctypes.data, job_mask.ctypes.data, len(pa_tab), cpa, job_pa.ctypes.data, int(n_blocks), int(no_symbols),
            gf.ctypes.data, out.ctypes.data, jpow.ctypes.data))
    elif tables:
        mask_len = np.array([t.size for t in tables], dtype=np.int32)
        gains = _lib.f32(np.concatenate(tables))
        _lib.check(_lib.load().wofdm_tx_psd_batch_masked(
            n, int(device), len(jobs), C.addressof(cj), w_all.ctypes.data, len(tables), mask_len.ctypes.data,
            gains.ctypes.data, job_mask.ctypes.data, int(n_blocks), int(no_symbols), gf.ctypes.data, out.ctypes.data))
    else:
        _lib.check(_lib.load().wofdm_tx_psd_batch(n, int(device), len(jobs), C.addressof(cj), w_all.ctypes.data,
                                                  int(n_blocks), int(no_symbols), gf.ctypes.data, out.ctypes.data))
    if divide:
        out = out.astype(np.float64) / (np.array(lengths, dtype=np.int64) // (8 * n) + 1)[:, None]
    return (out, jpow) if power else out


def analytical_psd(st, w_tx, sampling_period, guard_band=GUARD_BAND, fft_len=None):
    """(S_opt, S_rc, S_cp) of lines 155-214 for the Tx window ``w_tx`` (vector, length P)."""
    from scipy.signal import firwin
    n, cp, cs = st.n_fft, st.cp, st.cs
    fft_len = 8 * n if fft_len is None else fft_len
    up = fft_len / n
    f_axis = np.linspace(-.5, .5 - 1 / fft_len, fft_len) / sampling_period
    delta_f = 1 / (n * sampling_period)
    sigma2 = (n / (n - guard_band)) ** 2
    g_i = firwin(st.sym_len, [f_axis[int(fft_len / 2 + up)], f_axis[-int(guard_band * up)]],
                 window="boxcar", fs=1 / sampling_period, pass_zero=False)

    def corr(win):
        return ((win ** 2).sum(), (win[:cp] * win[n:n + cp]).sum(),
                (win[n + cp:n + cp + cs] * win[cp:cp + cs]).sum())

    def spectrum(win, denom, c):
        G = np.abs(np.fft.fftshift(np.fft.fft(g_i * win, fft_len))) ** 2
        return G * (n * sigma2 / denom) / up * (c[0] + 2 * (c[1] + c[2]) * np.cos(f_axis / delta_f))

    w_tx = np.asarray(w_tx, dtype=np.float64)
    w_rc = V.tx_rc_window(st)
    return (spectrum(w_tx, st.sym_len, corr(w_tx)), spectrum(w_rc, st.sym_len, corr(w_rc)),
            spectrum(np.ones(st.sym_len), n + cp, (n + cp, cp, 0.0)))


def _obr_windows(st, w_tx):
    """(window, overlap) of the three estimates of estimate_obr: optimised, RC, plain CP-OFDM"""
    overlap = st.tail_tx if st.system in ("wtx", "CPwtx", "WOLA", "CPW") else 0
    return ((np.asarray(w_tx, dtype=np.float64), overlap), (V.tx_rc_window(st), overlap),
            (np.ones(st.sym_len), 0))


def _obr_dicts(st, w_tx, samp_period, ests):
    """the three result dicts of estimate_obr from the three periodograms"""
    n = st.n_fft
    fft_len = 8 * n
    f_axis = np.linspace(-.5, .5 - 1 / fft_len, fft_len) / 200e-9
    interp = fft_len / n
    gb = int(interp * GUARD_BAND)
    S = analytical_psd(st, np.asarray(w_tx, dtype=np.float64), samp_period, GUARD_BAND, fft_len)
    out = []
    for tag, est, s in zip(("opt", "rc", "cp"), ests, S):
        out.append({"X_est_" + tag: est, "S_" + tag: s, "f_axis": f_axis,
                    "obr_" + tag: np.mean(np.hstack((est[:gb], est[-gb:]))),
                    "mf_band_" + tag: np.hstack((est[gb:fft_len // 2],
                                                 est[-int(fft_len / 2 - interp):-gb]))})
    return tuple(out)


def estimate_obr(st, w_tx, samp_period=200e-9, X=None, rng=None, gpu=False, mask=None, pa=None):
    """``wOFDMSystem.estimate_obr`` (lines 216-296): three dicts (optimised window, RC window,
    plain CP-OFDM) with the reference's keys.  gpu=True: waveform and periodogram on the GPU,
    ``wofdm_tx_psd`` per window at N <= 256, one ``wofdm_tx_psd_batch`` call for the three at
    N = 512 / 1024.  mask: [2P-1] gains of a spectral Tx mask (``mask_rows``) applied to all three
    waveforms; the host route is ``tx_waveform``, the GPU route one ``wofdm_tx_psd_batch_masked`` call.  pa: an
    amplifier (``rx_profile.PaPoint``) behind all three waveforms, each backed off from its own mean power: the
    spectral regrowth; the host route is ``tx_waveform(..., pa=pa)``, the GPU route one ``wofdm_tx_psd_batch_pa`` call."""
    n = st.n_fft
    fft_len = 8 * n
    X = draw_symbols(n, rng) if X is None else np.asarray(X)
    wins = _obr_windows(st, w_tx)
    if not gpu:
        ests = [psd_estimate(tx_waveform(st, X, w, ov, mask, pa=pa), fft_len) for w, ov in wins]
    elif pa is not None:
        ests = list(tx_psd_batch_gpu(n, _full_grid(n, X)[None], [(0, st.cp, st.cs, ov, w, mask, pa) for w, ov in wins]))
    elif mask is not None:
        ests = list(tx_psd_batch_gpu(n, _full_grid(n, X)[None], [(0, st.cp, st.cs, ov, w, mask) for w, ov in wins]))
    elif n <= 256:
        ests = [psd_estimate_gpu(st, X, w, ov) for w, ov in wins]
    else:
        ests = list(tx_psd_batch_gpu(n, _full_grid(n, X)[None], [(0, st.cp, st.cs, ov, w) for w, ov in wins]))
    return _obr_dicts(st, w_tx, samp_period, ests)


def _timefreq_setup(system, n_fft, cp, tail_tx, tail_rx, window_path):
    """structure and Tx window of a ``-m run_timefreq`` work item (lines 17-61)"""
    st = V.make_structure(system, n_fft, cp, tail_tx if system in V.TX_WINDOWED else 0,
                          tail_rx if system in V.RX_WINDOWED else 0)
    if system in V.TX_WINDOWED:
        vec = np.load(os.path.join(window_path, "%s_%d.npy" % (system, cp)))
        xt, _ = V.split_tail_file(st, vec)
        w_tx = V.expand_tx_window(st, xt)
    else:
        w_tx = np.ones(st.sym_len)
    return st, w_tx


def _timefreq_save(folder_path, system, cp, opt, rc, cpd):
    path = os.path.join(folder_path, "timefreq")
    os.makedirs(path, exist_ok=True)
    np.savez(os.path.join(path, "opt_%s_%d.npz" % (system, cp)), **opt)
    np.savez(os.path.join(path, "rc_%s_%d.npz" % (system, cp)), **rc)
    np.savez(os.path.join(path, "CP_%d.npz" % cp), **cpd)


def timefreq_fun(data, rng=None):
    """Work item of ``-m run_timefreq`` (lines 17-76): data = (system, dft_len, cp_len, tail_tx,
    tail_rx, window_path, folder_path)."""
    system, n_fft, cp, tail_tx, tail_rx, window_path, folder_path = data
    st, w_tx = _timefreq_setup(system, n_fft, cp, tail_tx, tail_rx, window_path)
    opt, rc, cpd = estimate_obr(st, w_tx, 200e-9, rng=rng)
    _timefreq_save(folder_path, system, cp, opt, rc, cpd)
    return opt, rc, cpd


def run_timefreq(cp_list, sys_list, window_path, folder_path, n_fft=256, rng=None, gpu=False):
    """``-m run_timefreq`` (wofdm_optimization.py:133-154): the work item of every (system, CP),
    systems outer, tails 8 / 10, the same ``timefreq/`` files.  The symbols are drawn per item in
    that order from ``rng``, as successive ``timefreq_fun`` calls with it would.  gpu=True: all
    3 x len(sys_list) x len(cp_list) periodograms in ONE ``wofdm_tx_psd_batch`` call.  Returns
    {(system, cp): (opt, rc, cp_dict)}."""
    items = [(system, cp) for system in sys_list for cp in cp_list]
    out = {}
    if not gpu:
        for system, cp in items:
            data = (system, n_fft, cp, 8 if system in V.TX_WINDOWED else 0,
                    10 if system in V.RX_WINDOWED else 0, window_path, folder_path)
            out[(system, cp)] = timefreq_fun(data, rng)
        return out
    setups, grids, jobs = [], [], []
    for b, (system, cp) in enumerate(items):
        st, w_tx = _timefreq_setup(system, n_fft, cp, 8, 10, window_path)
        grids.append(_full_grid(n_fft, draw_symbols(n_fft, rng)))
        jobs += [(b, st.cp, st.cs, ov, w) for w, ov in _obr_windows(st, w_tx)]
        setups.append((st, w_tx))
    ests = tx_psd_batch_gpu(n_fft, np.stack(grids), jobs)
    for b, ((system, cp), (st, w_tx)) in enumerate(zip(items, setups)):
        dicts = _obr_dicts(st, w_tx, 200e-9, list(ests[3 * b:3 * b + 3]))
        _timefreq_save(folder_path, system, cp, *dicts)
        out[(system, cp)] = dicts
    return out


# ---- Tx PAPR of the frames the BER loop transmits (wofdm_tx_papr; the reference has no PAPR figure) ----

def qam_table(bits_per_sc):
    """Constellation point of every label: MATLAB ``qammod`` with Gray labels and unit average power, label = first bit
    in the top position (the table of the frame kernels), k = 2, 4, 6."""
    k = int(bits_per_sc)
    if k not in (2, 4, 6):
        raise ValueError("bits_per_sc must be 2, 4 or 6")
    half = k // 2
    m = 1 << half
    lab = np.arange(1 << k)

    def gray_dec(g):
        b = g.copy()
        for sh in (1, 2):
            b ^= g >> sh
        return b
    scale = 1.0 / np.sqrt(2.0 * (m * m - 1) / 3.0)
    return scale * ((2.0 * gray_dec(lab >> half) - (m - 1)) + 1j * ((m - 1) - 2.0 * gray_dec(lab & (m - 1))))


def frame_papr(st, grids, w_tx, mask=None):
    """fp64 host mirror of ``wofdm_tx_papr``'s periods.  grids: [frames, S, N] symbols on every bin (zeros on the
    unloaded ones); each frame through ``tx_waveform`` with overlap ``st.tail_tx`` (and ``mask`` [2P-1]); symbol period
    s is tx[s B, (s + 1) B), B = P - tail_tx -- the trailing tail_tx samples belong to no period.  Returns
    [frames, S, 2] = {peak, energy} = {max |tx|^2, sum |tx|^2} over the period."""
    grids = np.asarray(grids, dtype=np.complex128)
    if grids.ndim != 3 or grids.shape[2] != st.n_fft:
        raise ValueError("grids must be [frames, S, %d], got %s" % (st.n_fft, grids.shape))
    n_sym, stride = grids.shape[1], st.sym_len - st.tail_tx
    out = np.empty(grids.shape[:2] + (2,))
    for f, grid in enumerate(grids):
        x = tx_waveform(st, grid.T, w_tx, st.tail_tx, mask, guard_band=None)
        p = np.abs(x[:n_sym * stride].reshape(n_sym, stride)) ** 2
        out[f, :, 0], out[f, :, 1] = p.max(axis=1), p.sum(axis=1)
    return out


def papr_db(periods, B):
    """10 log10(B peak / energy) of [..., 2] = {peak, energy}; -inf for a period without energy."""
    periods = np.asarray(periods, dtype=np.float64)
    peak, energy = periods[..., 0], periods[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(energy > 0, 10.0 * np.log10(B * peak / np.where(energy > 0, energy, 1.0)), -np.inf)


def papr_hist(periods, B, lo_db, step_db, n_bins):
    """The binning rule of ``wofdm_tx_papr`` on [..., 2] = {peak, energy}: bin = clamp(floor((10 log10(B peak /
    energy) - lo_db) / step_db), 0, n_bins - 1), a period without energy in bin 0.  Returns the counts [n_bins]
    (uint64) over all the periods given."""
    db = papr_db(periods, B).reshape(-1)
    with np.errstate(invalid="ignore"):
        t = np.floor((db - lo_db) / step_db)
    bins = np.clip(np.where(np.isnan(t), -1.0, t), 0, n_bins - 1).astype(np.int64)
    return np.bincount(bins, minlength=n_bins).astype(np.uint64)


def papr_ccdf(hist):
    """Complementary CDF from histogram counts [..., n_bins]: ccdf[..., i] = share of the periods in the bins i and
    above, i.e. Pr(PAPR >= lower edge of bin i); ccdf[..., 0] = 1 (zeros for an empty histogram)."""
    hist = np.asarray(hist, dtype=np.float64)
    tail = np.cumsum(hist[..., ::-1], axis=-1)[..., ::-1]
    total = hist.sum(axis=-1, keepdims=True)
    return tail / np.where(total > 0, total, 1.0)


def tx_papr_chunk_frames(st, syms, masked):
    """Frames one chunk of ``wofdm_tx_papr`` holds (include/wofdm.h: WOFDM_TX_PAPR_CHUNK_BYTES over the bytes of a
    frame's symbol grid, waveform and -- masked -- filtered symbols; at most 65535)."""
    from . import _lib
    P = st.sym_len
    T = st.tail_tx + syms * (P - st.tail_tx)
    per_frame = 8 * (syms * st.n_fft + T + (syms * (2 * P - 1) if masked else 0))
    return min(65535, max(1, _lib.TX_PAPR_CHUNK_BYTES // per_frame))


def tx_papr_gpu(st, bits_per_sc, syms, w_tx_pairs, seed, frame_offset, frames, active=None, mask=None, lo_db=0.0,
                step_db=0.25, n_bins=64, periods=False, device=0, hist=None, max_papr=None):
    """``wofdm_tx_papr``: PAPR histogram of the symbol periods of the frames [frame_offset, frame_offset + frames) that
    window pair p transmits as cell p of a plan with one SNR point and one channel (same seed, allocation ``active``
    [N] and Tx mask ``mask`` [2P-1]).  w_tx_pairs: [pairs, P].  lo_db and step_db are taken in single precision.
    Returns (hist [pairs, n_bins] uint64, max_papr [pairs] float32 -- linear), and with periods=True also
    [pairs, frames, S, 2] float32 = {peak, energy}.  ``hist`` / ``max_papr`` given: accumulated into (and returned).
    No CPU fallback."""
    import ctypes as C
    from . import _lib
    from .simulation import make_cfg
    w = _lib.f32(np.atleast_2d(w_tx_pairs))
    pairs = w.shape[0]
    if w.shape[1] != st.sym_len:
        raise ValueError("w_tx_pairs must be [pairs, %d], got %s" % (st.sym_len, w.shape))
    cfg = make_cfg(st, int(bits_per_sc), int(syms), 1, 1, 1, pairs, seed=int(seed), frames_per_cell=int(frames),
                   frame_offset=int(frame_offset))
    act = None if active is None else np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, dtype=np.uint8)
    if act is not None and act.shape != (st.n_fft,):
        raise ValueError("active must hold %d flags" % st.n_fft)
    m = None if mask is None else _lib.f32(np.asarray(mask).reshape(-1), (2 * st.sym_len - 1,))
    hist = np.zeros((pairs, int(n_bins)), dtype=np.uint64) if hist is None else hist
    max_papr = np.zeros(pairs, dtype=np.float32) if max_papr is None else max_papr
    if hist.dtype != np.uint64 or hist.shape != (pairs, int(n_bins)) or not hist.flags.c_contiguous:
        raise ValueError("hist must be a contiguous uint64 array [pairs, n_bins]")
    if max_papr.dtype != np.float32 or max_papr.shape != (pairs,) or not max_papr.flags.c_contiguous:
        raise ValueError("max_papr must be a contiguous float32 array [pairs]")
    per = np.zeros((pairs, int(frames), int(syms), 2), dtype=np.float32) if periods else None
    _lib.check(_lib.load().wofdm_tx_papr(
        C.byref(cfg), int(device), w.ctypes.data, None if act is None else act.ctypes.data,
        None if m is None else m.ctypes.data, float(lo_db), float(step_db), int(n_bins), hist.ctypes.data,
        max_papr.ctypes.data, None if per is None else per.ctypes.data))
    return (hist, max_papr, per) if periods else (hist, max_papr)
